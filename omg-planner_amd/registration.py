"""Pose refinement of known objects against observed clouds: the specification of omgx_register_clouds
(csrc/omg_register.hip and csrc/omg_register_body.h follow it operation by operation) and the scene-level call
`refine_scene_poses`.

Every known object carries a signed distance volume in the pool (the `omgx_object` records of scenes.OBJECT_DTYPE).  Given the
points of a cloud that belong to the object and a rough pose, registration looks for the pose at which the volume is zero on
the points: a Levenberg-Marquardt iteration on the truncated residual v(q), q = R^T (p - t), with v the trilinear value of the
volume, its analytic gradient, and a Cayley update of the rotation.  The reference takes these poses from an outside
estimator (real_world/trial.py) or from the scene file; its collision layer is named sdf_matching_loss after this use.

Everything specified is plain numpy float64, one rounded operation per line element, sums in a fixed shape (256 lanes, a tree
inside each group of 64, the four group totals left to right), the 6 x 6 solve written out, and nothing but + - * / in the loop,
so that the device can equal the bits.  Not part of the contract: a global search, colour, point-to-plane ICP on meshes,
segmentation of a cloud into objects.
"""
from __future__ import annotations

import numpy as np

from . import _lib

THREADS = _lib.CONSTANTS["OMGX_REGISTER_THREADS"]        # lanes of the sum (the kernel's workgroup)
MAX_PASSES = _lib.CONSTANTS["OMGX_REGISTER_MAX_PASSES"]  # most trials of one call
STATS = _lib.CONSTANTS["OMGX_REGISTER_STATS"]            # doubles per row of `stats`
# the status word (stats[:, 7])
FEW_INLIERS = _lib.CONSTANTS["OMGX_REGISTER_FEW_INLIERS"]  # the loop ended (or never began) with fewer than six inliers
SINGULAR = _lib.CONSTANTS["OMGX_REGISTER_SINGULAR"]        # a trial's solve met a pivot that is not > 0 or not finite
LAMBDA_AT_MAX = _lib.CONSTANTS["OMGX_REGISTER_LAMBDA_AT_MAX"]  # the loop ended because lambda reached LAMBDA_MAX
CONVERGED = _lib.CONSTANTS["OMGX_REGISTER_CONVERGED"]      # an accepted step had max|xi| < step_tol
# columns of stats
COST0, COST, COUNT0, COUNT, ACCEPTED, TRIALS, LAMBDA, STATUS = range(8)
# Fixed here and, with the same values, inside csrc/omg_register_body.h; the C ABI does not carry them.
FLOOR = 1e-9                  # added to every diagonal entry of the normal matrix: an unobserved direction stays solvable
LAMBDA_MIN = 2.0 ** -20
LAMBDA_MAX = 2.0 ** 20
MIN_INLIERS = 6               # fewer inliers than unknowns: nothing is solved
NPART = 28                    # 21 (upper triangle of H, row-major) + 6 (b) + 1 (cost)
_TRI = [(i, j) for i in range(6) for j in range(i, 6)]


def cayley(a) -> np.ndarray:
    """C(a) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a) -> [3,3], a rotation for every finite a; a = tan(angle / 2) * axis.
    s = (a0*a0 + a1*a1) + a2*a2; the diagonal is ((1 - s) + 2*(a_i*a_i)) / (1 + s), the rest (2*(a_i*a_j) -+ 2*a_k) / (1 + s)."""
    a0, a1, a2 = (float(x) for x in a)
    s = (a0 * a0 + a1 * a1) + a2 * a2
    den = 1.0 + s
    one = 1.0 - s
    return np.array([[(one + 2.0 * (a0 * a0)) / den, (2.0 * (a0 * a1) - 2.0 * a2) / den, (2.0 * (a0 * a2) + 2.0 * a1) / den],
                     [(2.0 * (a0 * a1) + 2.0 * a2) / den, (one + 2.0 * (a1 * a1)) / den, (2.0 * (a1 * a2) - 2.0 * a0) / den],
                     [(2.0 * (a0 * a2) - 2.0 * a1) / den, (2.0 * (a1 * a2) + 2.0 * a0) / den, (one + 2.0 * (a2 * a2)) / den]])


def trilinear(pool, base, sx: int, sy: int, fx, fy, fz, inv_delta: float):
    """The interpolant of value_gradient's docstring from the cell whose corner (0, 0, 0) is pool[base]; base, fx, fy, fz [n];
    sx, sy: the element strides of x and y -> (v, g_x, g_y, g_z) [n] float64.  Shared with volume_camera.sample: the same lines,
    the same order."""
    pool = np.asarray(pool)
    c = lambda dx, dy, dz: pool[base + dx * sx + dy * sy + dz].astype(np.float64)
    c000, c001, c010, c011, c100, c101, c110, c111 = c(0, 0, 0), c(0, 0, 1), c(0, 1, 0), c(0, 1, 1), c(1, 0, 0), c(1, 0, 1), c(1, 1, 0), c(1, 1, 1)
    d00, d01, d10, d11 = c001 - c000, c011 - c010, c101 - c100, c111 - c110
    c00, c01, c10, c11 = c000 + fz * d00, c010 + fz * d01, c100 + fz * d10, c110 + fz * d11
    e0, e1 = c01 - c00, c11 - c10
    c0, c1 = c00 + fy * e0, c10 + fy * e1
    v = c0 + fx * (c1 - c0)
    gx = (c1 - c0) * inv_delta
    gy = (e0 + fx * (e1 - e0)) * inv_delta
    dz0, dz1 = d00 + fy * (d01 - d00), d10 + fy * (d11 - d10)
    gz = (dz0 + fx * (dz1 - dz0)) * inv_delta
    return v, gx, gy, gz


def value_gradient(obj, pool, q):
    """The per-point body: q [n,3] (object frame) -> (inside [n] bool, v [n], g [n,3]); v and g are 0 where not inside.

    u_a = (q_a - float64(lo_a)) * inv_delta - 0.5; inside iff every u_a >= 0 and u_a < dim_a - 1, tested in float64 before
    any conversion (NaN, +-inf and 1e300 are outside); i = int(u), f = u - i; the eight corners c_xyz =
    pool[grid_offset + (i_x*dim_y + i_y)*dim_z + i_z + ...] as float64.  Along z first:
      d00 = c001 - c000, d01 = c011 - c010, d10 = c101 - c100, d11 = c111 - c110;  c00 = c000 + fz*d00, ... c11 = c110 + fz*d11
      e0 = c01 - c00, e1 = c11 - c10;  c0 = c00 + fy*e0, c1 = c10 + fy*e1;  v = c0 + fx*(c1 - c0)
      g_x = (c1 - c0) * inv_delta;  g_y = (e0 + fx*(e1 - e0)) * inv_delta
      dz0 = d00 + fy*(d01 - d00), dz1 = d10 + fy*(d11 - d10);  g_z = (dz0 + fx*(dz1 - dz0)) * inv_delta
    the gradient of that same interpolant, from the same eight loads."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    lo = np.asarray(obj["lo"], np.float32).astype(np.float64)
    dim = [int(d) for d in obj["dim"]]
    inv_delta, off = float(obj["inv_delta"]), int(obj["grid_offset"])
    with np.errstate(invalid="ignore", over="ignore"):
        u = [(q[:, a] - lo[a]) * inv_delta - 0.5 for a in range(3)]
        inside = np.ones(len(q), bool)
        for a in range(3):
            inside &= (u[a] >= 0.0) & (u[a] < float(dim[a] - 1))
    u = [np.where(inside, x, 0.0) for x in u]
    i = [x.astype(np.int64) for x in u]
    fx, fy, fz = (x - k.astype(np.float64) for x, k in zip(u, i))
    base = off + (i[0] * dim[1] + i[1]) * dim[2] + i[2]
    v, gx, gy, gz = trilinear(pool, base, dim[1] * dim[2], dim[2], fx, fy, fz, inv_delta)
    zero = lambda x: np.where(inside, x, 0.0)
    return inside, zero(v), np.stack([zero(gx), zero(gy), zero(gz)], -1)


def _tree(x):
    """[256, k] lane partials -> [k]: inside each group of 64 lanes x[l] += x[l + s] for s = 32 ... 1, then ((w0 + w1) + w2) + w3."""
    w = x.reshape(THREADS // 64, 64, -1).copy()
    for s in (32, 16, 8, 4, 2, 1):
        w[:, :s] = w[:, :s] + w[:, s: 2 * s]
    t = w[:, 0]
    return ((t[0] + t[1]) + t[2]) + t[3]


def one_pass(obj, pool, pose, pts, trunc):
    """One pass at `pose` [12] over the used points pts [n,3] -> (cost, count, H [21], b [6]).

    Per point: d = p - t, q_a = (R[0][a]*d0 + R[1][a]*d1) + R[2][a]*d2; (inside, v, g) = value_gradient; inlier iff inside and
    |v| <= trunc.  j = -(g_x, g_y, g_z, q_y*g_z - q_z*g_y, q_z*g_x - q_x*g_z, q_x*g_y - q_y*g_x).  An inlier adds v*v to the
    cost, j_i*j_k (i <= k) to H and j_i*v to b; every other point adds trunc*trunc to the cost.  Lane l of 256 adds its points
    l, l + 256, ... in order from +0.0; the lanes are summed by _tree."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    P = np.asarray(pose, np.float64).reshape(3, 4)
    R, t = P[:, :3], P[:, 3]
    tau2 = float(trunc) * float(trunc)
    n = len(pts)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [pts[:, a] - t[a] for a in range(3)]
        q = np.stack([(R[0, a] * d[0] + R[1, a] * d[1]) + R[2, a] * d[2] for a in range(3)], -1)
        inside, v, g = value_gradient(obj, pool, q)
        inl = inside & (np.abs(v) <= float(trunc))
        qz = np.where(inl[:, None], q, 0.0)
        j = [-g[:, 0], -g[:, 1], -g[:, 2], -(qz[:, 1] * g[:, 2] - qz[:, 2] * g[:, 1]), -(qz[:, 2] * g[:, 0] - qz[:, 0] * g[:, 2]),
             -(qz[:, 0] * g[:, 1] - qz[:, 1] * g[:, 0])]
        terms = [j[a] * j[c] for a, c in _TRI] + [j[a] * v for a in range(6)] + [v * v]
    contrib = np.stack([np.where(inl, x, 0.0) for x in terms], -1)
    contrib[:, NPART - 1] = np.where(inl, contrib[:, NPART - 1], tau2)
    chunks = (n + THREADS - 1) // THREADS
    padded = np.zeros((chunks * THREADS, NPART))
    padded[:n] = contrib
    acc = np.zeros((THREADS, NPART))
    for k in range(chunks):
        acc = acc + padded[k * THREADS: (k + 1) * THREADS]
    tot = _tree(acc)
    return float(tot[NPART - 1]), int(inl.sum()), tot[:21].copy(), tot[21:27].copy()


def solve6(H, b, lam):
    """A xi = -b with A = H + lam*diag(H) + FLOOR*I (A_ii = (H_ii + lam*H_ii) + FLOOR) by LDL^T without pivoting -> (ok, xi [6]).

    for j = 0..5:  w_k = L_jk*d_k (k < j);  d_j = A_jj - L_j0*w_0 - ... (left to right);  ok only if d_j > 0 and finite;
                   L_ij = (A_ij - L_i0*w_0 - ...) / d_j  (i > j)
    y_i = -b_i - L_i0*y_0 - ...;  z_i = y_i / d_i;  xi_i = z_i - L_(i+1)i*xi_(i+1) - ... - L_5i*xi_5  (i = 5 ... 0)
    ok also needs every xi finite."""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(_TRI):
        A[i, j] = A[j, i] = float(H[k])
    for i in range(6):
        A[i, i] = (A[i, i] + float(lam) * A[i, i]) + FLOOR
    L, d = np.zeros((6, 6)), np.zeros(6)
    with np.errstate(all="ignore"):
        for j in range(6):
            w = [L[j, k] * d[k] for k in range(j)]
            s = A[j, j]
            for k in range(j):
                s = s - L[j, k] * w[k]
            d[j] = s
            if not (s > 0.0 and np.isfinite(s)):
                return False, np.zeros(6)
            for i in range(j + 1, 6):
                s = A[i, j]
                for k in range(j):
                    s = s - L[i, k] * w[k]
                L[i, j] = s / d[j]
        y = np.zeros(6)
        for i in range(6):
            s = -float(b[i])
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s
        x = np.zeros(6)
        for i in range(5, -1, -1):
            s = y[i] / d[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s
    return bool(np.isfinite(x).all()), x


def step_pose(pose, xi):
    """t' = t + R xi_v, R' = R C(xi_w / 2) -> [12]; every product sum as (x*x' + y*y') + z*z'."""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    R, t = P[:, :3], P[:, 3]
    Cm = cayley([0.5 * xi[3], 0.5 * xi[4], 0.5 * xi[5]])
    out = np.zeros((3, 4))
    for i in range(3):
        for k in range(3):
            out[i, k] = (R[i, 0] * Cm[0, k] + R[i, 1] * Cm[1, k]) + R[i, 2] * Cm[2, k]
        out[i, 3] = t[i] + ((R[i, 0] * xi[0] + R[i, 1] * xi[1]) + R[i, 2] * xi[2])
    return out.reshape(12)


def _check_args(objects, pool, obj_index, poses0, points, ranges, stride, trunc, lambda0, step_tol, max_passes):
    from . import scenes as _sc
    objects = np.asarray(objects)
    if objects.dtype != _sc.OBJECT_DTYPE or objects.ndim != 1:
        raise ValueError("objects must be a 1-d array of scenes.OBJECT_DTYPE records")
    pool = np.asarray(pool)
    if pool.dtype != np.float32 or pool.ndim != 1:
        raise ValueError("pool must be a 1-d float32 array")
    obj_index = np.asarray(obj_index, np.int64).reshape(-1)
    M = len(obj_index)
    poses0 = np.ascontiguousarray(poses0, np.float64).reshape(M, 12)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, np.int64).reshape(M, 2)
    if int(stride) < 1:
        raise ValueError("stride must be >= 1")
    if not 0 <= int(max_passes) <= MAX_PASSES:
        raise ValueError(f"max_passes must be in [0, {MAX_PASSES}]")
    if not (np.isfinite(trunc) and trunc > 0 and np.isfinite(lambda0) and lambda0 > 0):
        raise ValueError("trunc and lambda0 must be finite and positive")
    if M and (obj_index.min() < 0 or obj_index.max() >= len(objects)):
        raise ValueError(f"an object index is outside the {len(objects)} records")
    if M and ((ranges < 0).any() or (ranges > len(points)).any() or (ranges[:, 1] < ranges[:, 0]).any()):
        raise ValueError(f"a range is outside [0, {len(points)}] or ends before it begins")
    for o in np.unique(obj_index):
        r = objects[o]
        n = int(np.prod(r["dim"].astype(np.int64)))
        if (r["dim"] < 2).any() or int(r["grid_offset"]) < 0 or int(r["grid_offset"]) + n > len(pool):
            raise ValueError(f"object {o}: every axis needs two samples and the grid must lie inside the pool")
    return objects, pool, obj_index, poses0, points, ranges


def register_clouds(objects, pool, obj_index, poses0, points, ranges, stride: int = 1, trunc: float = 0.03, lambda0: float = 2.0 ** -10,
                    step_tol: float = 1e-6, max_passes: int = 30):
    """Refine M poses -> (poses [M,12] float64, stats [M,8] float64).  The specification of omgx_register_clouds.

    objects: scenes.OBJECT_DTYPE records (only lo, dim, inv_delta and grid_offset are read; pose_inv is float32 and ignored);
    pool: the float32 volume pool; obj_index [M]; poses0 [M,12]: rows 0..2 of world_from_obj; points [N,3] float64 in the world
    frame; ranges [M,2] (begin, end) into points, possibly empty, overlapping or equal; instance m uses the points begin,
    begin + stride, ... < end.  trunc: the truncation of the residual in metres; max_passes = K trials at most.

    cost, count, H, b = one_pass(poses0);  lam = lambda0.  Then, in this order:
      count < 6: status |= FEW_INLIERS, stop;  lam >= LAMBDA_MAX: status |= LAMBDA_AT_MAX, stop;  K trials run: stop.
      One trial: (ok, xi) = solve6(H, b, lam).  Not ok: status |= SINGULAR, lam = min(8 lam, LAMBDA_MAX), next trial.
      cost', ... = one_pass(step_pose(pose, xi)).  cost' < cost: the trial's pose, cost, count, H and b are taken,
      lam = max(lam / 8, LAMBDA_MIN), and max|xi| < step_tol: status |= CONVERGED, stop.  Otherwise lam = min(8 lam, LAMBDA_MAX).
    stats: cost at poses0, final cost, inliers at poses0, final inliers, accepted trials, trials run, final lam, status."""
    objects, pool, obj_index, poses0, points, ranges = _check_args(objects, pool, obj_index, poses0, points, ranges, stride, trunc, lambda0,
                                                                   step_tol, max_passes)
    M, K = len(obj_index), int(max_passes)
    poses, stats = poses0.copy(), np.zeros((M, STATS))
    for m in range(M):
        obj = objects[obj_index[m]]
        pts = points[ranges[m, 0]: ranges[m, 1]: int(stride)]
        pose = poses0[m].copy()
        cost, count, H, b = one_pass(obj, pool, pose, pts, trunc)
        cost0, count0, lam, status, accepted, trials = cost, count, float(lambda0), 0, 0, 0
        while True:
            if count < MIN_INLIERS:
                status |= FEW_INLIERS
                break
            if lam >= LAMBDA_MAX:
                status |= LAMBDA_AT_MAX
                break
            if trials >= K:
                break
            trials += 1
            ok, xi = solve6(H, b, lam)
            if not ok:
                status |= SINGULAR
                lam = min(8.0 * lam, LAMBDA_MAX)
                continue
            trial = step_pose(pose, xi)
            c1, n1, H1, b1 = one_pass(obj, pool, trial, pts, trunc)
            if c1 < cost:
                pose, cost, count, H, b = trial, c1, n1, H1, b1
                accepted += 1
                lam = max(lam / 8.0, LAMBDA_MIN)
                if np.abs(xi).max() < float(step_tol):
                    status |= CONVERGED
                    break
            else:
                lam = min(8.0 * lam, LAMBDA_MAX)
        poses[m] = pose
        stats[m] = [cost0, cost, count0, count, accepted, trials, lam, status]
    return poses, stats


def best_of(stats, groups):
    """Per group (a list of instance indices) the index with the lowest final cost; the lowest index wins a tie."""
    stats = np.asarray(stats, np.float64).reshape(-1, STATS)
    out = []
    for g in groups:
        g = sorted(int(i) for i in g)
        best = g[0]
        for i in g[1:]:
            if stats[i, COST] < stats[best, COST]:
                best = i
        out.append(best)
    return out


def accepted_mask(stats, pairs, min_inliers: int):
    """refine_scene_poses' rule -> [M] bool.  An instance passes iff its final cost is below its initial cost and it has at
    least min_inliers inliers; where several instances name the same (scene, obj) pair only the best_of winner can be accepted,
    and only if it passes itself."""
    stats = np.asarray(stats, np.float64).reshape(-1, STATS)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    passes = (stats[:, COST] < stats[:, COST0]) & (stats[:, COUNT] >= int(min_inliers))
    groups = {}
    for m, p in enumerate(pairs):
        groups.setdefault((int(p[0]), int(p[1])), []).append(m)
    mask = np.zeros(len(pairs), bool)
    for w in best_of(stats, list(groups.values())):
        mask[w] = passes[w]
    return mask


def pose_rows(pose_mats) -> np.ndarray:
    """[M,4,4] object -> world matrices -> [M,12], the rows register_clouds takes."""
    return np.ascontiguousarray(np.asarray(pose_mats, np.float64).reshape(-1, 4, 4)[:, :3, :].reshape(-1, 12))


def pose_mats(rows) -> np.ndarray:
    """[M,12] -> [M,4,4]."""
    rows = np.asarray(rows, np.float64).reshape(-1, 3, 4)
    out = np.tile(np.eye(4), (len(rows), 1, 1))
    out[:, :3, :] = rows
    return out


def refine_scene_poses(dscenes, pairs, poses0, points, ranges, stride: int = 1, trunc: float = 0.03, lambda0: float = 2.0 ** -10,
                       step_tol: float = 1e-6, max_passes: int = 30, min_inliers: int = 30, write_back: bool = True):
    """Register M instances against the volumes of an ops.DeviceScenes in one launch and move the objects
    -> (poses [M,12], stats [M,8], accepted [M] bool), numpy.

    pairs [M,2]: (scene, obj) of every instance; several instances may name one pair (different starts: accepted_mask keeps
    the best).  poses0 [M,12] and points [N,3] float64 (device tensors, e.g. ops.pixel_clouds' points), ranges [M,2] on the
    host.  Poses and stats are downloaded once; the accepted poses are written with DeviceScenes.set_object_poses (one scatter)
    when write_back.  It calls no planner."""
    import torch
    from . import ops
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    d_poses, d_stats = ops.register_clouds(dscenes, pairs, poses0, points, ranges, stride=stride, trunc=trunc, lambda0=lambda0,
                                           step_tol=step_tol, max_passes=max_passes)
    both = torch.cat([d_poses, d_stats], 1).cpu().numpy()  # one download
    poses, stats = np.ascontiguousarray(both[:, :12]), np.ascontiguousarray(both[:, 12:])
    mask = accepted_mask(stats, pairs, min_inliers)
    if write_back and mask.any():
        dscenes.set_object_poses(pairs[mask], pose_mats(poses[mask]))
    return poses, stats, mask
