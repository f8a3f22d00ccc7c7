"""Rays and meshes shared by the grasp-sampling tests (test_grasp_sampling_cpu.py, test_gpu_grasp_sampling.py)."""
from __future__ import annotations

import numpy as np

from tests import mesh_cases as MC

BOX_POSE = MC.pose((0.3, -0.5, 0.8), (0.2, 0.1, -0.3))
SLAB = (0.10, 0.16, 0.06)  # the box's thickness along its own x, y, z
_AXIS_SIGN = [(0, -1.0), (0, 1.0), (1, -1.0), (1, 1.0), (2, -1.0), (2, 1.0)]  # quad q of MC.box_mesh: the face at sign * half[axis]


def _move(pose_mat, p, vector=False):
    if pose_mat is None:
        return p
    return p @ pose_mat[:3, :3].T + (0.0 if vector else pose_mat[:3, 3])


def box_inward_rays(pose_mat=None, per_face=8, seed=0):
    """Rays from random points of each box face along the inward normal -> (origins, dirs, slab distance [N], the two faces of the
    opposite quad [N,2])."""
    rng = np.random.RandomState(seed)
    h = np.asarray(MC.BOX_HALF)
    o, d, want, opp = [], [], [], []
    for q, (axis, sign) in enumerate(_AXIS_SIGN):
        p = rng.uniform(-0.9, 0.9, (per_face, 3)) * h
        p[:, axis] = sign * h[axis]
        n = np.zeros(3)
        n[axis] = -sign
        o.append(p), d.append(np.tile(n, (per_face, 1))), want.append(np.full(per_face, SLAB[axis]))
        opp.append(np.tile([2 * (q ^ 1), 2 * (q ^ 1) + 1], (per_face, 1)))
    return _move(pose_mat, np.concatenate(o)), _move(pose_mat, np.concatenate(d), True), np.concatenate(want), np.concatenate(opp)


def box_diagonal_rays(pose_mat=None, per_quad=99):
    """Rays from 5 cm outside straight down onto the shared diagonal of each box quad's two triangles -> (origins, dirs, the two
    faces of the quad [N,2])."""
    v, f = MC.box_mesh(MC.BOX_HALF)
    o, d, quad = [], [], []
    for q, (axis, sign) in enumerate(_AXIS_SIGN):
        a, c = v[f[2 * q][0]], v[f[2 * q][2]]  # triangles (q0, q1, q2), (q0, q2, q3): the diagonal q0 - q2
        s = np.linspace(0.01, 0.99, per_quad)[:, None]
        n = np.zeros(3)
        n[axis] = sign
        o.append(a + s * (c - a) + 0.05 * n), d.append(np.tile(-n, (per_quad, 1))), quad.append(np.tile([2 * q, 2 * q + 1], (per_quad, 1)))
    return _move(pose_mat, np.concatenate(o)), _move(pose_mat, np.concatenate(d), True), np.concatenate(quad)


def sphere_crack_rays(verts, faces, limit=None):
    """Rays from the centre of an icosphere (at the origin) through its vertices and through three points of each edge ->
    (origins, dirs, incident: a list of the face indices that share the vertex or edge)."""
    vert_faces = {}
    edge_faces = {}
    for fi, (a, b, c) in enumerate(faces):
        for x in (a, b, c):
            vert_faces.setdefault(int(x), []).append(fi)
        for x, y in ((a, b), (b, c), (c, a)):
            edge_faces.setdefault((min(x, y), max(x, y)), []).append(fi)
    d, inc = [], []
    for x, fs in sorted(vert_faces.items()):
        d.append(verts[x]), inc.append(fs)
    for (x, y), fs in sorted(edge_faces.items()):
        for s in (0.25, 0.5, 0.8):
            d.append(verts[x] + s * (verts[y] - verts[x])), inc.append(fs)
    d = np.array(d)
    d /= np.sqrt((d * d).sum(1))[:, None]
    if limit is not None:
        pick = np.linspace(0, len(d) - 1, limit).astype(int)
        d, inc = d[pick], [inc[i] for i in pick]
    return np.zeros_like(d), d, inc


def two_boxes():
    """The test box and a second one whose middle the first one's top plane cuts: a ray in that plane at y = 0.12 passes the
    first box by and hits the second one's near face (x = 0.25) inside a triangle, at t = 0.45 from x = -0.2."""
    v1, f1 = MC.box_mesh(MC.BOX_HALF)
    v2, f2 = MC.box_mesh(MC.BOX_HALF, MC.pose(t=(0.3, 0.1, 0.03)))
    return np.concatenate([v1, v2]), np.concatenate([f1, f2 + 8]).astype(np.int32)


PLANE_RAY = (np.array([[-0.2, 0.12, 0.03]]), np.array([[1.0, 0.0, 0.0]]))  # lies in the plane z = 0.03 of the first box's top


def outward_rays(verts, faces, count=16, seed=1):
    """Rays that leave a convex mesh from points of its faces along the outward normal: all miss."""
    rng = np.random.RandomState(seed)
    f = faces[rng.randint(0, len(faces), count)]
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    w = rng.dirichlet((2.0, 2.0, 2.0), count)
    n = np.cross(b - a, c - a)
    return w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c, n / np.linalg.norm(n, axis=1)[:, None]


def mixed_rays(verts, faces, count, seed):
    """`count` rays for bit comparisons on any mesh (open ones too): random rays from inside and outside the bounding box, rays
    from the centroid through vertices and edge midpoints (cracks), rays in the planes of faces (parallels) and rays that miss."""
    rng = np.random.RandomState(seed)
    lo, hi = verts.min(0), verts.max(0)
    ctr, ext = 0.5 * (lo + hi), (hi - lo)
    o, d = [], []
    n_rand = max(count // 2, 1)
    o.append(ctr + rng.uniform(-0.8, 0.8, (n_rand, 3)) * ext)
    d.append(rng.normal(size=(n_rand, 3)))
    k = max(count // 6, 1)
    vi = rng.randint(0, len(verts), k)
    o.append(np.tile(ctr, (k, 1))), d.append(verts[vi] - ctr)                                       # through vertices
    f = faces[rng.randint(0, len(faces), k)]
    o.append(np.tile(ctr, (k, 1))), d.append(0.5 * (verts[f[:, 0]] + verts[f[:, 1]]) - ctr)          # through edge midpoints
    f = faces[rng.randint(0, len(faces), k)]
    o.append(verts[f[:, 0]] - 2.0 * (verts[f[:, 1]] - verts[f[:, 0]])), d.append(verts[f[:, 1]] - verts[f[:, 0]])  # along edges: in the face's plane
    o.append(ctr + 3.0 * ext * np.sign(rng.normal(size=(k, 3)))), d.append(np.tile([1.0, 1.0, 1.0], (k, 1)) * np.sign(o[-1] - ctr))  # misses
    o, d = np.concatenate(o), np.concatenate(d)
    d = d / np.sqrt((d * d).sum(1))[:, None]
    while len(o) < count:
        o, d = np.concatenate([o, o]), np.concatenate([d, d])
    return np.ascontiguousarray(o[:count]), np.ascontiguousarray(d[:count])
