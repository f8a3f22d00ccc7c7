"""Meshes shared by the mesh-SDF tests (test_mesh_sdf_cpu.py, test_gpu_mesh_sdf.py): boxes, icospheres, poses."""
from __future__ import annotations

import numpy as np

BOX_HALF = (0.05, 0.08, 0.03)  # the 0.10 x 0.16 x 0.06 m box of the tests


def box_mesh(half, pose=None, flip=False):
    """8 vertices, 12 outward-facing triangles of the box [-half, half], moved by pose [4,4]."""
    h = np.asarray(half, np.float64)
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    if flip:
        f = f[:, ::-1].copy()
    if pose is not None:
        v = v @ pose[:3, :3].T + pose[:3, 3]
    return v, f


def pose(rotvec=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    """[4,4] from a rotation vector (Rodrigues) and a translation."""
    r = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(r)
    P = np.eye(4)
    if th > 0:
        k = r / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        P[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    P[:3, 3] = t
    return P


def box_distance(half, pose_mat, p):
    """The exact signed distance of scenes.box_sdf's formula, evaluated in the box's frame, at the points p [N,3] (float64)."""
    loc = (p - pose_mat[:3, 3]) @ pose_mat[:3, :3]
    q = np.abs(loc) - np.asarray(half, np.float64)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def icosphere(level: int, radius: float = 0.06, centre=(0.0, 0.0, 0.0)):
    """Icosahedron subdivided `level` times (20 * 4^level faces: 20, 80, 320, 1280), vertices pushed to the sphere; faces outward."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(centre, np.float64), np.array(f, np.int32)


def inside_convex(verts, faces, p):
    """p [N,3] strictly inside the convex polyhedron (every face plane on its inner side) -> (inside [N], on_surface [N])."""
    c = verts.mean(0)
    a, b, cc = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = np.cross(b - a, cc - a)
    n *= np.sign(np.einsum("fk,fk->f", n, a - c))[:, None]  # outward
    s = np.einsum("fk,nfk->nf", n, p[:, None, :] - a[None])
    return (s < 0).all(1), (s <= 0).all(1) & (s == 0).any(1)
