"""Camera tracking: a live depth frame aligned to the model's rendering by projective point-to-plane ICP.  The specification of
omgx_track_cameras (include/omg_hip.h section 25; csrc/omg_track_body.h follows it operation by operation) in plain numpy, and
the host-side helpers of camera.Observation.tracked (compose, accepted_mask, valid_pixels).

Every perception op takes cam_from_world as exact.  A camera on a wrist or a stand is known from kinematics and a hand-eye
calibration, or from the frame before, to millimetres or centimetres; a TSDF integrated from such poses smears.  The third piece
of a TSDF stack, beside integration (tsdf.py) and the ray-cast (volume_camera.py), finds T = model_cam_from_live_cam, the pose of
the live camera in the frame of the camera the model was rendered at.  The reference has no tracker: its perception entry is
given exact poses (omg/core.py:826-867).

One camera per view.  Inputs per view: the live depth zl [H,W] (anything not > 0, or +inf, is no information), optionally the
live normals nl [H,W,3] (sensor.depth_normals: unit, camera frame, facing the camera), the model depth zm [H,W] (+inf is
background) and normals nm [H,W,3] as render_volumes writes them, one intrinsics row fx, fy, cx, cy for both images, and the
rows [R t] of T [12].

Pixel (r, c) is USED iff r % stride == 0 and c % stride == 0; the used pixels are numbered row-major over the Hu x Wu used grid,
Hu = (H - 1) // stride + 1, Wu alike.  Per used pixel at the pose (R, t):
  VALID:       z = zl[r,c], z > 0 and z < +inf; with live normals also (m0*m0 + m1*m1) + m2*m2 > 0 for m = nl[r,c]
  P = (dx*z, dy*z, z) with camera.pixel_directions' ray;  Q_a = ((R[a][0]*P0 + R[a][1]*P1) + R[a][2]*P2) + t_a
  FRONT:       Q2 > 0
  ua = (fx*(Q0/Q2) + cx) + 0.5, ub = (fy*(Q1/Q2) + cy) + 0.5;  inside iff ua >= 0, ua < W, ub >= 0, ub < H, tested in float64 before
               any conversion (NaN, +-inf and 1e300 are outside);  cm = int(ua), rm = int(ub)
  THERE:       zq = zm[rm,cm], zq > 0 and zq < +inf;  n = nm[rm,cm], (n0*n0 + n1*n1) + n2*n2 > 0
  M = (dx'*zq, dy'*zq, zq) with the ray of (rm, cm)
  NEAR:        e = Q - M, dd = (e0*e0 + e1*e1) + e2*e2, dd <= dist2  (dist2 = dist_max*dist_max)
  COMPATIBLE   (live normals only): mr_a = (R[a][0]*m0 + R[a][1]*m1) + R[a][2]*m2, cs = (mr0*n0 + mr1*n1) + mr2*n2, cs >= cos_min
  INLIER: all of them.  res = (n0*e0 + n1*e1) + n2*e2;  g_a = (R[0][a]*n0 + R[1][a]*n1) + R[2][a]*n2
          j = (g0, g1, g2, P1*g2 - P2*g1, P2*g0 - P0*g2, P0*g1 - P1*g0): the derivative of res under registration.step_pose's update
An inlier adds j_a*j_b (a <= b, registration's order), j_a*res and res*res to the 28 sums and 1 to the count; a VALID pixel that
is no inlier adds dist2 to the cost; a pixel that is not VALID adds nothing.

The sums have a fixed shape (planes.py's moments shape): chunks of PIXELS_PER_WORKGROUP used pixels in used-pixel order; lane l of
256 adds its chunk's pixels l, l + 256, ... in order from +0.0; the lanes are summed by registration._tree; the chunk totals are
added left to right, beginning with chunk 0's.  The loop is registration.register_clouds' loop with this pass in place of
one_pass: solve6 and step_pose called, FLOOR, LAMBDA_MIN, LAMBDA_MAX and MIN_INLIERS taken from there, the same eight stats and
status bits.  Everything is float64, every operation rounded on its own, + - * / and comparisons only.

Not part of the contract: an image pyramid (beyond stride and tracked's rounds), colour, per-pixel weights, priors beyond poses0,
loop closure, moving objects.
"""
from __future__ import annotations

import numpy as np

from . import _lib, registration as _reg

PIXELS_PER_WORKGROUP = _lib.CONSTANTS["OMGX_TRACK_PIXELS_PER_WORKGROUP"]  # used pixels of one chunk of the sum
MAX_PASSES = _lib.CONSTANTS["OMGX_TRACK_MAX_PASSES"]
STATS = _lib.CONSTANTS["OMGX_TRACK_STATS"]
THREADS, NPART = _reg.THREADS, _reg.NPART
COST0, COST, COUNT0, COUNT, ACCEPTED, TRIALS, LAMBDA, STATUS = range(8)  # columns of stats: registration's
FEW_INLIERS, SINGULAR, LAMBDA_AT_MAX, CONVERGED = _reg.FEW_INLIERS, _reg.SINGULAR, _reg.LAMBDA_AT_MAX, _reg.CONVERGED
IDENTITY = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])


def used_grid(H: int, W: int, stride: int):
    """(Hu, Wu) of the used pixels of an H x W image."""
    return (int(H) - 1) // int(stride) + 1, (int(W) - 1) // int(stride) + 1


def pixel_terms(zl, nl, zm, nm, k, pose, stride: int, dist2: float, cos_min: float):
    """The per-pixel rule for one view at `pose` [12] -> (valid [n] bool, inlier [n] bool, res [n], j [n,6], P [n,3]) over the
    n = Hu*Wu used pixels in used-pixel order; res and j are 0 where the pixel is no inlier."""
    zl, zm, nm = np.asarray(zl, np.float64), np.asarray(zm, np.float64), np.asarray(nm, np.float64)
    H, W = zl.shape
    fx, fy, cx, cy = (float(x) for x in k)
    T = np.asarray(pose, np.float64).reshape(3, 4)
    R, t = T[:, :3], T[:, 3]
    Hu, Wu = used_grid(H, W, stride)
    ru, cu = np.divmod(np.arange(Hu * Wu, dtype=np.int64), Wu)
    r, c = ru * int(stride), cu * int(stride)
    with np.errstate(all="ignore"):
        z = zl[r, c]
        valid = (z > 0.0) & (z < np.inf)
        if nl is not None:
            m = np.asarray(nl, np.float64)[r, c]
            valid &= (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2] > 0.0
        dx, dy = (c.astype(np.float64) - cx) / fx, (r.astype(np.float64) - cy) / fy
        P = [dx * z, dy * z, z]
        Q = [((R[a, 0] * P[0] + R[a, 1] * P[1]) + R[a, 2] * P[2]) + t[a] for a in range(3)]
        front = Q[2] > 0.0
        ua, ub = (fx * (Q[0] / Q[2]) + cx) + 0.5, (fy * (Q[1] / Q[2]) + cy) + 0.5
        inside = (ua >= 0.0) & (ua < float(W)) & (ub >= 0.0) & (ub < float(H))
        ok = valid & front & inside
        cm, rm = np.where(ok, ua, 0.0).astype(np.int64), np.where(ok, ub, 0.0).astype(np.int64)
        zq, n = zm[rm, cm], nm[rm, cm]
        there = (zq > 0.0) & (zq < np.inf) & ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2] > 0.0)
        dxm, dym = (cm.astype(np.float64) - cx) / fx, (rm.astype(np.float64) - cy) / fy
        M = [dxm * zq, dym * zq, zq]
        e = [Q[a] - M[a] for a in range(3)]
        dd = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        inl = ok & there & (dd <= float(dist2))
        if nl is not None:
            mr = [(R[a, 0] * m[:, 0] + R[a, 1] * m[:, 1]) + R[a, 2] * m[:, 2] for a in range(3)]
            cs = (mr[0] * n[:, 0] + mr[1] * n[:, 1]) + mr[2] * n[:, 2]
            inl &= cs >= float(cos_min)
        res = (n[:, 0] * e[0] + n[:, 1] * e[1]) + n[:, 2] * e[2]
        g = [(R[0, a] * n[:, 0] + R[1, a] * n[:, 1]) + R[2, a] * n[:, 2] for a in range(3)]
        j = [g[0], g[1], g[2], P[1] * g[2] - P[2] * g[1], P[2] * g[0] - P[0] * g[2], P[0] * g[1] - P[1] * g[0]]
    res = np.where(inl, res, 0.0)
    j = np.stack([np.where(inl, x, 0.0) for x in j], -1)
    return valid, inl, res, j, np.stack(P, -1)


def one_pass(zl, nl, zm, nm, k, pose, stride: int, dist2: float, cos_min: float):
    """One pass over one view at `pose` -> (cost, count, H [21], b [6]) in the fixed shape of the module docstring."""
    valid, inl, res, j, _ = pixel_terms(zl, nl, zm, nm, k, pose, stride, dist2, cos_min)
    with np.errstate(all="ignore"):
        terms = [j[:, a] * j[:, c] for a, c in _reg._TRI] + [j[:, a] * res for a in range(6)] + [res * res]
    contrib = np.stack([np.where(inl, x, 0.0) for x in terms], -1)
    contrib[:, NPART - 1] = np.where(inl, contrib[:, NPART - 1], np.where(valid, float(dist2), 0.0))
    n = len(contrib)
    chunks = (n + PIXELS_PER_WORKGROUP - 1) // PIXELS_PER_WORKGROUP
    padded = np.zeros((chunks * PIXELS_PER_WORKGROUP, NPART))
    padded[:n] = contrib
    total = None
    with np.errstate(all="ignore"):
        for q in range(chunks):
            acc = np.zeros((THREADS, NPART))
            for i in range(PIXELS_PER_WORKGROUP // THREADS):
                at = q * PIXELS_PER_WORKGROUP + i * THREADS
                acc = acc + padded[at: at + THREADS]
            part = _reg._tree(acc)
            total = part if total is None else total + part
    return float(total[NPART - 1]), int(inl.sum()), total[:21].copy(), total[21:27].copy()


def valid_pixels(zl, nl, stride: int) -> np.ndarray:
    """[V] int64: the VALID used pixels of every view (they do not depend on the pose)."""
    zl = np.asarray(zl, np.float64)
    z = zl[:, ::int(stride), ::int(stride)]
    with np.errstate(all="ignore"):
        valid = (z > 0.0) & (z < np.inf)
        if nl is not None:
            m = np.asarray(nl, np.float64)[:, ::int(stride), ::int(stride)]
            valid &= (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2] > 0.0
    return valid.reshape(len(zl), -1).sum(1).astype(np.int64)


def check_track(zl, nl, zm, nm, intrinsics, poses0, stride, dist_max, cos_min, lambda0, step_tol, max_passes):
    """The argument checks of track_cameras (the wrapper makes the same) -> (zl, nl, zm, nm, intrinsics [V,4], poses0 [V,12])."""
    zl = np.asarray(zl)
    if zl.ndim != 3 or zl.dtype != np.float64:
        raise ValueError(f"live_depth must be [V,H,W] float64, got {zl.shape} {zl.dtype}")
    V, H, W = zl.shape
    if V and (H < 1 or W < 1):
        raise ValueError("H and W must be >= 1")
    zm, nm = np.asarray(zm), np.asarray(nm)
    if zm.shape != (V, H, W) or zm.dtype != np.float64:
        raise ValueError(f"model_depth must be float64 {(V, H, W)}, got {zm.shape} {zm.dtype}")
    if nm.shape != (V, H, W, 3) or nm.dtype != np.float64:
        raise ValueError(f"model_normals must be float64 {(V, H, W, 3)}, got {nm.shape} {nm.dtype}")
    if nl is not None:
        nl = np.asarray(nl)
        if nl.shape != (V, H, W, 3) or nl.dtype != np.float64:
            raise ValueError(f"live_normals must be None or float64 {(V, H, W, 3)}, got {nl.shape} {nl.dtype}")
    check_scalars(stride, dist_max, cos_min, lambda0, step_tol, max_passes)
    k = np.asarray(intrinsics, np.float64)
    if k.shape != (V, 4) or not np.isfinite(k).all() or (k[:, :2] == 0).any():
        raise ValueError(f"intrinsics must be [{V},4], finite, with no focal length of zero")
    poses0 = np.asarray(np.tile(IDENTITY, (V, 1)) if poses0 is None else poses0, np.float64)
    if poses0.shape != (V, 12):
        raise ValueError(f"poses0 must be [{V},12], got {poses0.shape}")
    return zl, nl, zm, nm, np.ascontiguousarray(k), np.ascontiguousarray(poses0)


def check_scalars(stride, dist_max, cos_min, lambda0, step_tol, max_passes) -> None:
    if int(stride) < 1:
        raise ValueError("stride must be >= 1")
    if not 0 <= int(max_passes) <= MAX_PASSES:
        raise ValueError(f"max_passes must be in [0, {MAX_PASSES}]")
    if not (np.isfinite(float(dist_max)) and float(dist_max) > 0 and np.isfinite(float(lambda0)) and float(lambda0) > 0):
        raise ValueError("dist_max and lambda0 must be finite and positive")
    if np.isnan(float(cos_min)):
        raise ValueError("cos_min must not be NaN")
    float(step_tol)


def track_cameras(zl, nl, zm, nm, intrinsics, poses0=None, stride: int = 1, dist_max: float = 0.05, cos_min: float = 0.7,
                  lambda0: float = 2.0 ** -10, step_tol: float = 1e-6, max_passes: int = 12):
    """Refine V camera poses -> (poses [V,12] float64, stats [V,8] float64).  The specification of omgx_track_cameras.

    zl [V,H,W], nl [V,H,W,3] or None, zm [V,H,W], nm [V,H,W,3], intrinsics [V,4], poses0 [V,12] (None: identity): the rows [R t]
    of model_cam_from_live_cam.  The loop is registration.register_clouds' (its docstring lists the order of the tests) with
    one_pass of this module; with max_passes = 0 or fewer than six inliers `poses` has poses0's bits.
    stats: cost at poses0, final cost, inliers at poses0, final inliers, accepted trials, trials run, final lam, status."""
    zl, nl, zm, nm, intr, poses0 = check_track(zl, nl, zm, nm, intrinsics, poses0, stride, dist_max, cos_min, lambda0, step_tol, max_passes)
    V, K = len(zl), int(max_passes)
    dist2 = float(dist_max) * float(dist_max)
    poses, stats = poses0.copy(), np.zeros((V, STATS))
    for v in range(V):
        args = (zl[v], None if nl is None else nl[v], zm[v], nm[v], intr[v])
        pose = poses0[v].copy()
        cost, count, H, b = one_pass(*args, pose, stride, dist2, cos_min)
        cost0, count0, lam, status, accepted, trials = cost, count, float(lambda0), 0, 0, 0
        while True:
            if count < _reg.MIN_INLIERS:
                status |= FEW_INLIERS
                break
            if lam >= _reg.LAMBDA_MAX:
                status |= LAMBDA_AT_MAX
                break
            if trials >= K:
                break
            trials += 1
            ok, xi = _reg.solve6(H, b, lam)
            if not ok:
                status |= SINGULAR
                lam = min(8.0 * lam, _reg.LAMBDA_MAX)
                continue
            trial = _reg.step_pose(pose, xi)
            c1, n1, H1, b1 = one_pass(*args, trial, stride, dist2, cos_min)
            if c1 < cost:
                pose, cost, count, H, b = trial, c1, n1, H1, b1
                accepted += 1
                lam = max(lam / 8.0, _reg.LAMBDA_MIN)
                if np.abs(xi).max() < float(step_tol):
                    status |= CONVERGED
                    break
            else:
                lam = min(8.0 * lam, _reg.LAMBDA_MAX)
        poses[v] = pose
        stats[v] = [cost0, cost, count0, count, accepted, trials, lam, status]
    return poses, stats


def compose(T, cam_from_world0) -> np.ndarray:
    """cam_from_world = inv(T) @ cam_from_world0 [4,4] for T = the rows [R t] of model_cam_from_live_cam [12] and the camera the
    model was rendered at: the live camera's pose.  The rigid inverse is written out: (R^T, -(R^T t))."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    R, t = T[:, :3], T[:, 3]
    inv = np.eye(4)
    inv[:3, :3] = R.T
    inv[:3, 3] = -(R.T @ t)
    return inv @ np.asarray(cam_from_world0, np.float64).reshape(4, 4)


def accepted_mask(stats, min_inliers: int, min_share: float, valid=None) -> np.ndarray:
    """[V] bool: a view is accepted iff its final cost is below its initial cost, it has at least min_inliers final inliers, and
    they are at least min_share times its VALID pixels (valid [V]: valid_pixels; the stats row does not carry them.  None: the
    share is not tested).  registration.accepted_mask's rule plus the share."""
    stats = np.asarray(stats, np.float64).reshape(-1, STATS)
    mask = (stats[:, COST] < stats[:, COST0]) & (stats[:, COUNT] >= int(min_inliers))
    if valid is not None:
        mask &= stats[:, COUNT] >= float(min_share) * np.asarray(valid, np.float64).reshape(len(stats))
    return mask
