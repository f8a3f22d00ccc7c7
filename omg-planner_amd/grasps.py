"""Antipodal grasp sets from triangle meshes: the specification of omgx_mesh_raycast / omgx_grasp_poses (csrc/omg_grasp.hip follows
it operation by operation) and the device path `sample_grasp_sets`.

The reference has no sampler: it reads grasp poses from data/grasps/simulated/<object>.npy (omg/planner.py:457-500).  Here rays
from sampled surface points, along the inward normal jittered inside the friction cone, are cast through the mesh; a ray whose
two contacts face each other within the cone is an antipodal pair; every pair gives `n_angles` hand poses about the closing axis,
and the object's own signed distance volume decides which of them the gripper fits.

Frame: a grasp is the pose of the hand link in the object's frame — what pipeline.plan_grasps(obj_coord=True) takes.  The hand
is the reference's drawing (omg/util.py:308-320): z the approach direction, y the closing axis, the fingers at y = +-0.043, the
palm at z = 0.058, the finger tips at z = 0.098.

Everything specified is plain numpy float64 with every dot and cross product written out elementwise ((x*x' + y*y') + z*z',
a*b - c*d), so that the device can equal the bits.  Not part of the contract: grasp quality beyond the cone test, the one-voxel
volume lookup, meshes that intersect themselves.
"""
from __future__ import annotations

import numpy as np

from . import scenes as _sc

# the six anchor points of the reference's hand drawing (omg/util.py:308-320), as numbers
HAND_FINGER_Y = 0.043
HAND_PALM_Z = 0.058
HAND_TIP_Z = 0.098
PAD_DEPTH = 0.088  # the contacts sit 1 cm behind the drawn finger tips


def _dot3(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross3(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _cols(x):
    x = np.asarray(x, np.float64)
    return [x[..., 0], x[..., 1], x[..., 2]]


def default_probe() -> np.ndarray:
    """[100,3] points of the gripper in the hand frame, the lattice the collision check looks up: two finger bars (x in
    {-0.01, 0, 0.01}, six z from the palm 0.058 to the tips 0.098, on the inner face |y| = 0.043 and the outer face |y| = 0.050:
    72 points) and a palm slab (z = 0.058, seven y across [-0.043, 0.043], x in {-0.01, 0, 0.01}: 21 points, and the seven y at
    x = 0 one centimetre behind it, z = 0.048)."""
    xs = (-0.01, 0.0, 0.01)
    pts = [(x, sy * y, z) for sy in (-1.0, 1.0) for y in (HAND_FINGER_Y, 0.050) for x in xs for z in np.linspace(HAND_PALM_Z, HAND_TIP_Z, 6)]
    ys = np.linspace(-HAND_FINGER_Y, HAND_FINGER_Y, 7)
    pts += [(x, y, HAND_PALM_Z) for x in xs for y in ys]
    pts += [(0.0, y, HAND_PALM_Z - 0.01) for y in ys]
    return np.array(pts, np.float64)


def face_normals(verts, faces):
    """(unit normals [F,3], areas [F]) of the faces: n = (b - a) x (c - a), |n| = sqrt((nx*nx + ny*ny) + nz*nz), area = |n| / 2."""
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = _cross3(_cols(b - a), _cols(c - a))
    ln = np.sqrt(_dot3(n, n))
    return np.stack([n[k] / ln for k in range(3)], -1), 0.5 * ln


def outward_mesh(verts, faces):
    """clean_mesh's output with the faces flipped if the signed volume sum a . (b x c) / 6 is negative, so that the normals point
    outwards -> (verts, faces)."""
    verts, faces, _ = _sc.clean_mesh(verts, faces)
    a, b, c = (_cols(verts[faces[:, k]]) for k in range(3))
    if float(np.sum(_dot3(a, _cross3(b, c)))) < 0.0:
        faces = np.ascontiguousarray(faces[:, ::-1])
    return verts, faces


def surface_samples(verts, faces, n: int, rng):
    """n points on the mesh (verts, faces as outward_mesh returns them), faces drawn with probability proportional to area ->
    (p1 [n,3], face [n] int32, normals [n,3]: the unit normals of the drawn faces).
    Consumes `r = rng.random_sample((n, 3))` once: r[:, 0] picks the face (searchsorted into the normalised cumulative area, side
    "right"), r[:, 1] and r[:, 2] are r1 and r2 of the barycentric point (1 - sqrt(r1)) a + sqrt(r1) (1 - r2) b + sqrt(r1) r2 c."""
    nrm, area = face_normals(verts, faces)
    r = rng.random_sample((int(n), 3))
    cum = np.cumsum(area)
    f = np.minimum(np.searchsorted(cum / cum[-1], r[:, 0], side="right"), len(faces) - 1).astype(np.int32)
    s1 = np.sqrt(r[:, 1])
    wa, wb, wc = 1.0 - s1, s1 * (1.0 - r[:, 2]), s1 * r[:, 2]
    a, b, c = verts[faces[f, 0]], verts[faces[f, 1]], verts[faces[f, 2]]
    p = (wa[:, None] * a + wb[:, None] * b) + wc[:, None] * c
    return np.ascontiguousarray(p), f, np.ascontiguousarray(nrm[f])


def _basis(d):
    """(b1, b2) for unit d (lists of three arrays): k the first axis with the smallest |d_k|, b1 = (e_k x d) / |e_k x d| with
    e_0 x d = (0, -dz, dy), e_1 x d = (dz, 0, -dx), e_2 x d = (-dy, dx, 0) and one sqrt, one division per component; b2 = d x b1."""
    k = np.argmin(np.stack([np.abs(d[0]), np.abs(d[1]), np.abs(d[2])]), axis=0)  # the first of equal minima
    zero = np.zeros_like(d[0])
    c = [np.where(k == 0, zero, np.where(k == 1, d[2], -d[1])),
         np.where(k == 0, -d[2], np.where(k == 1, zero, d[0])),
         np.where(k == 0, d[1], np.where(k == 1, -d[0], zero))]
    n = np.sqrt(_dot3(c, c))
    b1 = [c[0] / n, c[1] / n, c[2] / n]
    return b1, _cross3(d, b1)


def ray_directions(normals, cone: float, rng):
    """A unit direction inside the friction cone (half angle `cone`, radians) about -n for every row of normals [n,3].
    Consumes `r = rng.random_sample((n, 2))` once (also with cone = 0, which returns exactly -n): theta = cone * sqrt(r[:, 0]),
    phi = 2 pi r[:, 1], d = cos(theta) (-n) + sin(theta) (cos(phi) b1 + sin(phi) b2) with _basis(-n), normalised."""
    normals = np.asarray(normals, np.float64)
    r = rng.random_sample((len(normals), 2))
    if cone == 0:
        return np.ascontiguousarray(-normals)
    a = _cols(-normals)
    b1, b2 = _basis(a)
    th, ph = float(cone) * np.sqrt(r[:, 0]), 2.0 * np.pi * r[:, 1]
    d = [np.cos(th) * a[k] + np.sin(th) * (np.cos(ph) * b1[k] + np.sin(ph) * b2[k]) for k in range(3)]
    ln = np.sqrt(_dot3(d, d))
    return np.ascontiguousarray(np.stack([d[k] / ln for k in range(3)], -1))


def mesh_raycast(verts, faces, origins, dirs, t_min: float = 1e-6, tol: float = 1e-9):
    """The nearest hit of every ray origins[i] + t * dirs[i] with the mesh -> (t [N] float64, face [N] int32); (+inf, -1): no hit.
    The specification of omgx_mesh_raycast.  Moeller-Trumbore per face, in face order:
        e1 = b - a, e2 = c - a, h = d x e2, det = e1 . h, inv = 1.0 / det, s = o - a,
        u = (s . h) * inv, q = s x e1, v = (d . q) * inv, t = (e2 . q) * inv
    and the face hits iff (u >= -tol) & (v >= -tol) & (u + v <= 1 + tol) & (t > t_min) & (t < best), from best = +inf, face = -1.
    The strict < makes the lowest face index win a tie; tol makes neighbouring triangles overlap, so a ray through a shared edge
    or vertex cannot fall between them; there is no test on det: a ray parallel to a face gives inf or NaN, every comparison is
    false and the face is skipped.  Vectorised over the rays with a loop over the faces."""
    verts = np.asarray(verts, np.float64)
    o, d = _cols(origins), _cols(dirs)
    N = len(o[0])
    best = np.full(N, np.inf)
    face = np.full(N, -1, np.int32)
    neg_tol, one_tol = -float(tol), 1.0 + float(tol)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for fi, f in enumerate(np.asarray(faces)):
            a, b, c = verts[f[0]], verts[f[1]], verts[f[2]]
            e1, e2 = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
            h = _cross3(d, e2)
            inv = 1.0 / _dot3(e1, h)
            s = [o[k] - a[k] for k in range(3)]
            u = _dot3(s, h) * inv
            q = _cross3(s, e1)
            v = _dot3(d, q) * inv
            t = _dot3(e2, q) * inv
            hit = (u >= neg_tol) & (v >= neg_tol) & (u + v <= one_tol) & (t > t_min) & (t < best)
            best = np.where(hit, t, best)
            face = np.where(hit, np.int32(fi), face)
    return best, face


def approach_angles(n_angles: int) -> np.ndarray:
    """cs [A,2]: (cos, sin) of 2 pi a / A, computed once on the host and handed to the device as data."""
    a = 2.0 * np.pi * np.arange(int(n_angles), dtype=np.float64) / float(n_angles)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], -1))


def grasp_poses(p1, n1, d, t, face2, normals, cs, grid, probe, max_width: float = 0.08, min_width: float = 0.005,
                cone: float = np.deg2rad(15.0), pad_depth: float = PAD_DEPTH, clearance: float = 0.0, sample: str = "centre"):
    """Hand poses of the contact pairs (p1, p1 + t d) -> (poses [N,A,4,4] float64, valid [N,A] bool, width [N] = t).  The
    specification of omgx_grasp_poses.

    p1, n1, d [N,3]: the first contact, its unit face normal, the unit ray direction; t, face2 [N]: mesh_raycast's output;
    normals [F,3]: the unit normals of the mesh's faces; cs [A,2]: approach_angles(A); grid: scenes.SdfGrid of the object
    (sample i at origin + (i + offset) * delta, offset 0.5 for sample="centre", 0.0 for "node"); probe [Q,3]: gripper points in
    the hand frame (default_probe()).

    A ray is antipodal iff face2 >= 0, min_width <= t <= max_width, -(d . n1) >= cos(cone) and d . n2 >= cos(cone) with
    n2 = normals[face2].  Its poses: closing axis y = d, contact centre m = p1 + (0.5 t) d, (b1, b2) = _basis(d),
    z = c b1 + s b2 for (c, s) = cs[a], x = y x z, pose = [x y z | m - pad_depth z].  A ray that is not antipodal has poses of
    zeros.  Gripper check: every probe point w = ((x q0 + y q1) + z q2) + o is looked up in the volume at the nearest sample,
    idx_a = floor((w_a - origin_a) / delta + (0.5 - offset)); a point outside the grid is free, one whose float32 value is
    < float32(clearance) collides; valid = antipodal and no probe point collides.  The lookup is good to one voxel: a gripper
    point within a voxel of the surface may be judged either way."""
    p, n1c, dc = _cols(p1), _cols(n1), _cols(d)
    t = np.asarray(t, np.float64)
    face2 = np.asarray(face2)
    normals = np.asarray(normals, np.float64)
    cs = np.asarray(cs, np.float64)
    probe = np.asarray(probe, np.float64).reshape(-1, 3)
    N, A = len(t), len(cs)
    cos_cone = float(np.cos(cone))
    n2 = _cols(normals[np.clip(face2, 0, len(normals) - 1)])
    with np.errstate(invalid="ignore"):
        anti = (face2 >= 0) & (t >= min_width) & (t <= max_width) & (-_dot3(dc, n1c) >= cos_cone) & (_dot3(dc, n2) >= cos_cone)
    half = 0.5 * np.where(anti, t, 0.0)
    m = [p[k] + half * dc[k] for k in range(3)]
    b1, b2 = _basis(dc)
    c, s = cs[None, :, 0], cs[None, :, 1]
    z = [c * b1[k][:, None] + s * b2[k][:, None] for k in range(3)]     # [N,A]
    y = [np.broadcast_to(dc[k][:, None], (N, A)) for k in range(3)]
    x = _cross3(y, z)
    o = [m[k][:, None] - pad_depth * z[k] for k in range(3)]
    poses = np.zeros((N, A, 4, 4))
    for k in range(3):
        poses[:, :, k, 0], poses[:, :, k, 1], poses[:, :, k, 2], poses[:, :, k, 3] = x[k], y[k], z[k], o[k]
    poses[:, :, 3, 3] = 1.0
    poses[~anti] = 0.0
    data = np.asarray(grid.data, np.float32)
    origin, delta, shift = np.asarray(grid.origin, np.float64), float(grid.delta), 0.5 - _sc.MESH_SAMPLE_OFFSET[sample]
    hit = np.zeros((N, A), bool)
    for q in probe:
        w = [((x[k] * q[0] + y[k] * q[1]) + z[k] * q[2]) + o[k] for k in range(3)]
        fi = [np.floor((w[k] - origin[k]) / delta + shift) for k in range(3)]
        inside = np.ones((N, A), bool)
        for k in range(3):
            inside &= (fi[k] >= 0.0) & (fi[k] < float(data.shape[k]))
        ii = [np.where(inside, fi[k], 0.0).astype(np.int64) for k in range(3)]
        hit |= inside & (data[ii[0], ii[1], ii[2]] < np.float32(clearance))
    return poses, anti[:, None] & ~hit, t


def _keep(G: int, max_grasps, rng):
    if max_grasps is None or G <= int(max_grasps):
        return None
    return np.sort(rng.choice(G, int(max_grasps), replace=False))


def sample_grasps(verts, faces, grid, n_rays: int, n_angles: int, rng, max_width: float = 0.08, min_width: float = 0.005,
                  cone: float = np.deg2rad(15.0), pad_depth: float = PAD_DEPTH, clearance: float = 0.0, sample: str = "centre",
                  probe=None, t_min: float = 1e-6, tol: float = 1e-9, max_grasps=None) -> np.ndarray:
    """Grasp poses [G,4,4] of a mesh in its own frame, on the host: outward_mesh, surface_samples, ray_directions, mesh_raycast,
    grasp_poses, the valid poses in (ray, angle) order; with more than `max_grasps` of them, `rng.choice(G, max_grasps,
    replace=False)` sorted.  rng (a numpy RandomState or anything with random_sample and choice) is consumed in that order.  The
    specification of sample_grasp_sets; it may be slow."""
    verts, faces = outward_mesh(verts, faces)
    p1, _, n1 = surface_samples(verts, faces, n_rays, rng)
    d = ray_directions(n1, cone, rng)
    t, f2 = mesh_raycast(verts, faces, p1, d, t_min, tol)
    poses, valid, _ = grasp_poses(p1, n1, d, t, f2, face_normals(verts, faces)[0], approach_angles(n_angles), grid,
                                  default_probe() if probe is None else probe, max_width, min_width, cone, pad_depth, clearance, sample)
    out = poses[valid]
    keep = _keep(len(out), max_grasps, rng)
    return out if keep is None else out[keep]


def sample_grasp_sets(meshes, table_or_grids, n_rays: int, n_angles: int, rng, max_width: float = 0.08, min_width: float = 0.005,
                      cone: float = np.deg2rad(15.0), pad_depth: float = PAD_DEPTH, clearance: float = 0.0, sample="centre",
                      probe=None, t_min: float = 1e-6, tol: float = 1e-9, max_grasps=None, chunks: int = 0, targets=None,
                      device="cuda:0"):
    """sample_grasps for S meshes on the device -> a list of S arrays [G_s,4,4] (host), equal to sample_grasps' mesh by mesh.

    meshes: S (verts, faces) in the frames of their volumes.  table_or_grids: S scenes.SdfGrid (uploaded as one pool; `sample`
    says where they are sampled, one value or S) or an ops.DeviceScenes whose pool is read in place: scene s's object targets[s]
    (default 0; voxel centres).  rng: one stream, consumed mesh by mesh (surface_samples, ray_directions) and then, with
    max_grasps, once per mesh that has more; or a list of S streams, one per mesh.  One ray-cast launch (chunks: 0 = automatic)
    and one pose launch for all meshes; the valid poses are compacted on the device and downloaded once, after the S counts."""
    import torch
    from . import ops
    S = len(meshes)
    rngs = list(rng) if isinstance(rng, (list, tuple)) else [rng] * S
    if len(rngs) != S:
        raise ValueError("rng must be one stream or one per mesh")
    clean, p1, n1, d, nrm = [], [], [], [], []
    for s, (v, f) in enumerate(meshes):
        v, f = outward_mesh(v, f)
        p, _, n = surface_samples(v, f, n_rays, rngs[s])
        clean.append((v, f)), p1.append(p), n1.append(n), d.append(ray_directions(n, cone, rngs[s])), nrm.append(face_normals(v, f)[0])
    dev = torch.device(device)
    if isinstance(table_or_grids, ops.DeviceScenes):
        tab = table_or_grids
        dev = tab.device
        idx = [int(tab.host_scene_begin[s]) + (0 if targets is None else int(targets[s])) for s in range(S)]
        rec = tab.host_objects[idx]
        pool = tab.pool
        layout = [(rec["lo"][s].astype(np.float64), float(rec["delta"][s]), "centre", tuple(int(x) for x in rec["dim"][s]),
                   int(rec["grid_offset"][s])) for s in range(S)]
    else:
        if len(table_or_grids) != S:
            raise ValueError("one volume per mesh")
        samples = list(sample) if isinstance(sample, (list, tuple)) else [sample] * S
        sizes = [int(np.prod(g.data.shape)) for g in table_or_grids]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        pool = torch.from_numpy(np.concatenate([np.asarray(g.data, np.float32).ravel() for g in table_or_grids])).to(dev)
        layout = [(np.asarray(g.origin, np.float64), float(g.delta), samples[s], tuple(g.data.shape), int(offs[s]))
                  for s, g in enumerate(table_or_grids)]
    batch = ops.RayBatch(clean, [n_rays] * S, chunks=chunks, device=dev, layout=layout)
    to = lambda xs: torch.from_numpy(np.ascontiguousarray(np.concatenate(xs))).to(dev)
    d_p1, d_n1, d_d = to(p1), to(n1), to(d)
    t, f2 = ops.mesh_raycast_batch(batch, d_p1, d_d, t_min, tol)
    poses, valid = ops.grasp_poses(batch, d_p1, d_n1, d_d, t, f2, to(nrm), approach_angles(n_angles),
                                   default_probe() if probe is None else probe, pool, max_width, min_width, float(np.cos(cone)),
                                   pad_depth, clearance)
    flat = valid.view(S, -1).bool()
    counts = flat.sum(1).cpu().numpy()                                   # [S] int64: the only read-back before the poses
    rows = poses.view(-1, 16)[flat.view(-1)].cpu().numpy().reshape(-1, 4, 4)
    out, at = [], 0
    for s in range(S):
        g = rows[at: at + counts[s]]
        at += counts[s]
        keep = _keep(len(g), max_grasps, rngs[s])
        out.append(g.copy() if keep is None else g[keep])
    return out
