"""CPU restatement of the reference's goal-set IK, in numpy: the checker of omg_ik.hip (as oracle/ is for the CHOMP step).

* ``solve``: one KDL ``ChainIkSolverPos_NR_JL::CartToJnt`` per chain (robot_pykdl.py:118-146, 257-290), vectorised over chains:
  for i < max_iter: f = FK(q); d = diff(f, target); stop if every |d_j| <= eps; q += J^+ d (SVD pseudo-inverse, singular values
  < pinv_eps dropped: ChainIkSolverVel_pinv); clamp q to the padded limits.  The 100th update is never checked.  Its arithmetic
  follows omg_ik.hip operation by operation (the SVD is a one-sided Jacobi SVD, as on the device), so that a Newton iteration that
  amplifies rounding — near a singular configuration — amplifies the same rounding; ``hand_kinematics`` / ``jacobian`` /
  ``pinv_step`` are the plain definitions the tests check it against.
* ``solve_grasp``: the per-(grasp, seed) chain logic of ``solve_one_pose_ik`` (planner.py:17-86).
* ``inverse_kinematics``: a drop-in for ``robot_kinematics.inverse_kinematics`` (position, xyzw quaternion, seed) -> q | None,
  which tests/golden/make_ik_golden.py plugs into the reference's own Planner.

KDL's solver body is restated from its definition, not executed; see DESIGN.md ("Goal-set IK").
"""
from __future__ import annotations

import math

import numpy as np

MAX_ITER, EPS, PINV_EPS = 100, 1e-6, 1e-5
KDL_EPSILON = 1e-6  # KDL::epsilon: GetRot's margins
_OFFS = [0.0, -np.pi, np.pi, np.pi, -np.pi, np.pi, np.pi]

# omg/util.py:19-35 (radians; the fingers are not used by the IK)
ANCHOR_SEEDS = np.array([
    [2.5, 0.23, -2.89, -1.69, 0.056, 1.46, -1.27], [2.8, 0.23, -2.89, -1.69, 0.056, 1.46, -1.27],
    [2, 0.23, -2.89, -1.69, 0.056, 1.46, -1.27], [2.5, 0.83, -2.89, -1.69, 0.056, 1.46, -1.27],
    [0.049, 1.22, -1.87, -0.67, 2.12, 0.99, -0.85], [-2.28, -0.43, 2.47, -1.35, 0.62, 2.28, -0.27],
    [-2.02, -1.29, 2.20, -0.83, 0.22, 1.18, 0.74], [-2.2, 0.03, -2.89, -1.69, 0.056, 1.46, -1.27],
    [-2.5, -0.71, -2.73, -0.82, -0.7, 0.62, -0.56], [-2, -0.71, -2.73, -0.82, -0.7, 0.62, -0.56],
    [-2.66, -0.55, 2.06, -1.77, 0.96, 1.77, -1.35], [1.51, -1.48, -1.12, -1.55, -1.57, 1.15, 0.24],
    [-2.61, -0.98, 2.26, -0.85, 0.61, 1.64, 0.23]])


def ik_sincos(x):
    """omg_ik.hip's ik_sincos: fdlibm's sin / cos kernels after a three-part pi/2 reduction, in plain IEEE operations (the device's
    bits, where np.sin / np.cos and the device library may differ in the last one).  -> (sin, cos)."""
    x = np.asarray(x, np.float64)
    n = np.rint(x * 6.36619772367581382433e-01)
    r = ((x - n * 1.57079632673412561417e+00) - n * 6.07710050630396597660e-11) - n * 2.02226624871116645580e-21
    z = r * r
    ps = r + r * z * (-1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))))
    hz = 0.5 * z
    w = 1.0 - hz
    rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
              z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))))
    pc = w + (((1.0 - w) - hz) + z * rc)
    qd = n.astype(np.int64) & 3
    sn = np.select([qd == 0, qd == 1, qd == 2], [ps, pc, -ps], -pc)
    cs = np.select([qd == 0, qd == 1, qd == 2], [pc, -ps, -pc], ps)
    return sn, cs


_ATAN_HI = np.array([4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00])
_ATAN_LO = np.array([2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17])


def ik_atan2(y, x):
    """omg_ik.hip's ik_atan2_ynonneg (fdlibm's atan, plain IEEE operations) for y >= 0."""
    y, x = np.broadcast_arrays(np.asarray(y, np.float64), np.asarray(x, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        v = y / np.abs(x)
        i0 = v < 0.4375
        i1 = ~i0 & (v < 1.1875)
        ida = np.where(i0, -1, np.where(i1, np.where(v < 0.6875, 0, 1), np.where(v < 2.4375, 2, 3)))
        t = np.select([ida == 0, ida == 1, ida == 2, ida == 3],
                      [(2.0 * v - 1.0) / (2.0 + v), (v - 1.0) / (v + 1.0), (v - 1.5) / (1.0 + 1.5 * v), -1.0 / v], v)
        z = t * t
        w = z * z
        s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                  w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))))
        s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                  w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))))
        k = np.maximum(ida, 0)
        a = np.where(ida < 0, t - t * (s1 + s2), _ATAN_HI[k] - ((t * (s1 + s2) - _ATAN_LO[k]) - t))
        a = np.where(x > 0.0, a, 3.14159265358979311600e+00 - (a - 1.22464679914735320717e-16))
    a = np.where(y == 0.0, np.where(x > 0.0, 0.0, 3.14159265358979311600e+00), a)
    return np.where(x == 0.0, np.where(y == 0.0, 0.0, 1.57079632679489655800e+00), a)


def hand_kinematics(model, q):
    """q [B,7] radians -> hand frame (R [B,3,3], t [B,3]) of panda_link0 -> panda_hand (robot_pykdl output_pose[:, 7], before
    center_offset) and the joint axes z [B,7,3] / origins p [B,7,3]: z / translation of cur_{i-1} . pose_0[i]."""
    q = np.asarray(q, np.float64)
    B = q.shape[0]
    cur = np.tile(np.eye(4), (B, 1, 1))
    z = np.empty((B, 7, 3))
    p = np.empty((B, 7, 3))
    for i in range(7):
        A = cur @ model.pose_0[i]
        z[:, i], p[:, i] = A[:, :3, 2], A[:, :3, 3]
        c, s = np.cos(q[:, i]), np.sin(q[:, i])
        Rz = np.tile(np.eye(4), (B, 1, 1))
        Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1] = c, -s, s, c
        co, so = np.cos(_OFFS[i]), np.sin(_OFFS[i])
        Rx = np.array([[1, 0, 0, 0], [0, co, -so, 0], [0, so, co, 0], [0, 0, 0, 1.0]])
        b = model.pose_0[i] @ (Rz @ Rx)
        if i > 0:
            b[..., [1, 2]] *= -1
        cur = cur @ b
    hand = cur @ model.pose_0[7]
    return hand[:, :3, :3], hand[:, :3, 3], z, p


def jacobian(t, z, p):
    """6x7 base-frame Jacobian with its reference point at the hand origin t: column i = [z_i x (t - p_i); z_i]."""
    return np.concatenate([np.cross(z, t[:, None] - p), z], axis=-1).transpose(0, 2, 1)


def rotvec(R):
    """KDL Rotation::GetRot (axis * angle of Rotation::GetRotAngle, eps = KDL::epsilon) of R [B,3,3], with its branches at 0 and pi."""
    d = R.reshape(-1, 9)
    e, e2 = KDL_EPSILON, 10 * KDL_EPSILON
    sym = (np.abs(d[:, 1] - d[:, 3]) < e) & (np.abs(d[:, 2] - d[:, 6]) < e) & (np.abs(d[:, 5] - d[:, 7]) < e)
    ident = sym & (np.abs(d[:, 1] + d[:, 3]) < e2) & (np.abs(d[:, 2] + d[:, 6]) < e2) & (np.abs(d[:, 5] + d[:, 7]) < e2) \
        & (np.abs(d[:, 0] + d[:, 4] + d[:, 8] - 3) < e2)
    # general case
    f = (d[:, 0] + d[:, 4] + d[:, 8] - 1) / 2
    ax = np.stack([d[:, 7] - d[:, 5], d[:, 2] - d[:, 6], d[:, 3] - d[:, 1]], axis=-1)
    nrm = np.sqrt((ax * ax).sum(-1))
    ang = ik_atan2(nrm / 2, f)
    ax = np.where((nrm < e)[:, None], np.array([1.0, 0.0, 0.0]), ax / np.where(nrm < e, 1.0, nrm)[:, None])
    out = ax * ang[:, None]
    # angle = pi
    xx, yy, zz = (d[:, 0] + 1) / 2, (d[:, 4] + 1) / 2, (d[:, 8] + 1) / 2
    xy, xz, yz = (d[:, 1] + d[:, 3]) / 4, (d[:, 2] + d[:, 6]) / 4, (d[:, 5] + d[:, 7]) / 4
    with np.errstate(divide="ignore", invalid="ignore"):
        sx, sy, sz = np.sqrt(np.maximum(xx, 0)), np.sqrt(np.maximum(yy, 0)), np.sqrt(np.maximum(zz, 0))
        ax_x = np.stack([sx, xy / sx, xz / sx], -1)
        ax_y = np.stack([xy / sy, sy, yz / sy], -1)
        ax_z = np.stack([xz / sz, yz / sz, sz], -1)
    pi_ax = np.where(((xx > yy) & (xx > zz))[:, None], ax_x, np.where((yy > zz)[:, None], ax_y, ax_z))
    out = np.where((sym & ~ident)[:, None], pi_ax * np.pi, out)
    return np.where(ident[:, None], 0.0, out)


def twist_diff(R, t, TR, Tt):
    """KDL diff(f, target): (target.p - f.p, f.M . rotvec(f.M^-1 . target.M)) as [B,6]."""
    rel = np.einsum("bji,bjk->bik", R, TR)
    return np.concatenate([Tt - t, np.einsum("bij,bj->bi", R, rotvec(rel))], axis=-1)


def pinv_step(J, d, pinv_eps=PINV_EPS):
    """ChainIkSolverVel_pinv: J^+ d with singular values < pinv_eps dropped."""
    U, S, Vt = np.linalg.svd(J, full_matrices=False)
    utd = np.einsum("bji,bj->bi", U, d)
    keep = S >= pinv_eps
    inv = np.where(keep, utd / np.where(keep, S, 1.0), 0.0)
    return np.einsum("bji,bj->bi", Vt, inv)


def limits(model):
    return model.joint_lower_limit[0, :7], model.joint_upper_limit[0, :7]


_TABLES: dict = {}


def _tables(model):
    """The chain constants omg_ik.hip reads from the robot blob: UVW [7][27], TP [7][3], H [12] (rows of pose_0[7]), pose_0."""
    hit = _TABLES.get(id(model))
    if hit is None or hit[0] is not model:
        b = model.blob()
        D = 528 + 30 * model.points_per_link
        hit = (model, (b[D:D + 189].reshape(7, 27), b[D + 189:D + 210].reshape(7, 3), b[D + 210:D + 222], model.pose_0))
        _TABLES[id(model)] = hit
    return hit[1]


def fk_jacobian(model, q):
    """Hand frame and Jacobian rows of q [B,7] in the arithmetic order of omg_ik.hip's ik_fk_jacobian (no fused multiply-adds):
    R [B,9], t [B,3], W [B,6,7].  The same quantities as hand_kinematics + jacobian, re-associated through the blob's UVW tables."""
    UVW, TP, H, P0 = _tables(model)
    B = q.shape[0]
    cR = [np.full(B, v) for v in (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)]
    ct = [np.zeros(B)] * 3
    z, p = [], []
    for i in range(7):
        z.append([cR[3 * r] * P0[i][0, 2] + cR[3 * r + 1] * P0[i][1, 2] + cR[3 * r + 2] * P0[i][2, 2] for r in range(3)])
        s, c = ik_sincos(q[:, i])
        u = UVW[i]
        Bm = [c * u[k] + s * u[9 + k] + u[18 + k] for k in range(9)]
        tp = TP[i]
        nR = [cR[3 * r] * Bm[cc] + cR[3 * r + 1] * Bm[3 + cc] + cR[3 * r + 2] * Bm[6 + cc] for r in range(3) for cc in range(3)]
        ct = [cR[3 * r] * tp[0] + cR[3 * r + 1] * tp[1] + cR[3 * r + 2] * tp[2] + ct[r] for r in range(3)]
        cR = nR
        p.append(ct)
    R = [cR[3 * r] * H[cc] + cR[3 * r + 1] * H[4 + cc] + cR[3 * r + 2] * H[8 + cc] for r in range(3) for cc in range(3)]
    t = [cR[3 * r] * H[3] + cR[3 * r + 1] * H[7] + cR[3 * r + 2] * H[11] + ct[r] for r in range(3)]
    W = np.empty((B, 6, 7))
    for i in range(7):
        ex, ey, ez = t[0] - p[i][0], t[1] - p[i][1], t[2] - p[i][2]
        zi = z[i]
        W[:, 0, i] = zi[1] * ez - zi[2] * ey
        W[:, 1, i] = zi[2] * ex - zi[0] * ez
        W[:, 2, i] = zi[0] * ey - zi[1] * ex
        W[:, 3, i], W[:, 4, i], W[:, 5, i] = zi[0], zi[1], zi[2]
    return np.stack(R, -1), np.stack(t, -1), W


def _dot7(a, b):
    acc = a[:, 0] * b[:, 0]
    for j in range(1, 7):
        acc = acc + a[:, j] * b[:, j]
    return acc


def pinv_step_jacobi(W, d, pinv_eps=PINV_EPS, max_sweeps=32):
    """J^+ d by one-sided (Hestenes) Jacobi on the six rows W [B,6,7] of J, d [B,6] rotated alongside (omg_ik.hip's order):
    J = V W'^T with orthogonal columns w'_a, J^+ d = sum_a w'_a (V^T d)_a / |w'_a|^2 over |w'_a| >= pinv_eps — the truncated SVD
    pseudo-inverse (pinv_step) up to rounding."""
    if W.shape[0] == 1:
        return _pinv_step_jacobi_one(W[0].tolist(), d[0].tolist(), pinv_eps, max_sweeps)
    W, d = W.copy(), d.copy()
    B = W.shape[0]
    sweeping = np.ones(B, bool)
    for _ in range(max_sweeps):
        if not sweeping.any():
            break
        rotated = np.zeros(B, bool)
        norms = [_dot7(W[:, a], W[:, a]) for a in range(6)]  # a row's |w|^2 is a function of the row: recomputed when it turns
        for a in range(5):
            for b in range(a + 1, 6):
                al, be, ga = norms[a], norms[b], _dot7(W[:, a], W[:, b])
                rot = sweeping & (np.abs(ga) > 1e-15 * np.sqrt(al * be)) & (ga != 0.0)
                if not rot.any():
                    continue
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    zeta = (be - al) / (2.0 * ga)
                    az = np.abs(zeta)
                    tn = np.where(az > 1e100, 0.5 / az, 1.0 / (az + np.sqrt(1.0 + zeta * zeta))) * np.where(zeta < 0.0, -1.0, 1.0)
                    c = 1.0 / np.sqrt(1.0 + tn * tn)
                    s = c * tn
                wa, wb = W[:, a].copy(), W[:, b].copy()
                W[:, a] = np.where(rot[:, None], c[:, None] * wa - s[:, None] * wb, wa)
                W[:, b] = np.where(rot[:, None], s[:, None] * wa + c[:, None] * wb, wb)
                da, db = d[:, a].copy(), d[:, b].copy()
                d[:, a] = np.where(rot, c * da - s * db, da)
                d[:, b] = np.where(rot, s * da + c * db, db)
                rotated |= rot
                norms[a], norms[b] = _dot7(W[:, a], W[:, a]), _dot7(W[:, b], W[:, b])
        sweeping &= rotated
    dq = np.zeros((B, 7))
    for a in range(6):
        s2 = _dot7(W[:, a], W[:, a])
        keep = np.sqrt(s2) >= pinv_eps
        with np.errstate(divide="ignore", invalid="ignore"):
            f = d[:, a] / s2
        for j in range(7):
            dq[:, j] = np.where(keep, dq[:, j] + W[:, a, j] * f, dq[:, j])
    return dq


def _pinv_step_jacobi_one(W, d, pinv_eps, max_sweeps):
    """pinv_step_jacobi for one chain in Python floats: the same IEEE double operations in the same order (one solve at a time
    is how the reference calls its IK, and numpy's per-call overhead dominates there)."""
    dot = lambda x, y: ((((((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) + x[3] * y[3]) + x[4] * y[4]) + x[5] * y[5]) + x[6] * y[6])
    for _ in range(max_sweeps):
        rotated = False
        norms = [dot(W[a], W[a]) for a in range(6)]
        for a in range(5):
            for b in range(a + 1, 6):
                al, be, ga = norms[a], norms[b], dot(W[a], W[b])
                if abs(ga) > 1e-15 * math.sqrt(al * be) and ga != 0.0:
                    zeta = (be - al) / (2.0 * ga)
                    az = abs(zeta)
                    tn = (0.5 / az if az > 1e100 else 1.0 / (az + math.sqrt(1.0 + zeta * zeta))) * (-1.0 if zeta < 0.0 else 1.0)
                    c = 1.0 / math.sqrt(1.0 + tn * tn)
                    s = c * tn
                    wa, wb = W[a], W[b]
                    W[a] = [c * x - s * y for x, y in zip(wa, wb)]
                    W[b] = [s * x + c * y for x, y in zip(wa, wb)]
                    d[a], d[b] = c * d[a] - s * d[b], s * d[a] + c * d[b]
                    rotated = True
                    norms[a], norms[b] = dot(W[a], W[a]), dot(W[b], W[b])
        if not rotated:
            break
    dq = [0.0] * 7
    for a in range(6):
        s2 = dot(W[a], W[a])
        if math.sqrt(s2) >= pinv_eps:
            f = d[a] / s2
            dq = [dq[j] + W[a][j] * f for j in range(7)]
    return np.array([dq])


def twist_residual(R, t, TR, Tt):
    """KDL diff(f, target) in omg_ik.hip's order: R [B,9], t [B,3] -> [B,6]."""
    TRf = TR.reshape(-1, 9)
    rel = np.stack([R[:, r] * TRf[:, c] + R[:, 3 + r] * TRf[:, 3 + c] + R[:, 6 + r] * TRf[:, 6 + c]
                    for r in range(3) for c in range(3)], -1)
    w = rotvec(rel.reshape(-1, 3, 3))
    rot = [R[:, 3 * r] * w[:, 0] + R[:, 3 * r + 1] * w[:, 1] + R[:, 3 * r + 2] * w[:, 2] for r in range(3)]
    return np.concatenate([Tt - t, np.stack(rot, -1)], axis=-1)


def solve(model, TR, Tt, seeds, max_iter=MAX_ITER, eps=EPS, pinv_eps=PINV_EPS, record=None):
    """B independent NR_JL solves.  TR [B,3,3], Tt [B,3], seeds [B,7] -> (q [B,7], ok [B], iters [B]).

    q is the joint vector the loop ends with (after max_iter updates for a failure); iters is the number of updates applied.
    The arithmetic follows omg_ik.hip operation by operation (fk_jacobian, twist_residual, pinv_step_jacobi), so the device's
    results are comparable to the last bits, not just to the solver's tolerance.
    `record`, a list, receives per checked iteration the max-norm residual of every chain still running (for margin checks)."""
    lo, hi = limits(model)
    q = np.array(seeds, np.float64).copy()
    TR = np.asarray(TR, np.float64)
    Tt = np.asarray(Tt, np.float64)
    B = q.shape[0]
    ok = np.zeros(B, bool)
    iters = np.full(B, max_iter, np.int64)
    live = np.arange(B)
    for i in range(max_iter):
        if live.size == 0:
            break
        R, t, W = fk_jacobian(model, q[live])
        d = twist_residual(R, t, TR[live], Tt[live])
        res = np.abs(d).max(-1)
        if record is not None:
            record.append(res)
        done = res <= eps
        ok[live[done]] = True
        iters[live[done]] = i
        live, W, d = live[~done], W[~done], d[~done]
        if live.size == 0:
            break
        v = q[live] + pinv_step_jacobi(W, d, pinv_eps)
        v = np.where(v < lo, lo, v)
        q[live] = np.where(v > hi, hi, v)
    return q, ok, iters


def quat_to_matrix(x, y, z, w):
    """KDL Rotation::Quaternion (normalises first)."""
    n = np.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    return np.array([[w2 + x2 - y2 - z2, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y],
                     [2 * x * y + 2 * w * z, w2 - x2 + y2 - z2, 2 * y * z - 2 * w * x],
                     [2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, w2 - x2 - y2 + z2]])


def mat2quat(M):
    """transforms3d.quaternions.mat2quat (Bar-Itzhack), (w, x, y, z) with w >= 0: what omg.util.pack_pose uses."""
    Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz = np.asarray(M, np.float64)[:3, :3].flat
    K = np.array([[Qxx - Qyy - Qzz, 0, 0, 0], [Qyx + Qxy, Qyy - Qxx - Qzz, 0, 0], [Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, 0],
                  [Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    if q[0] < 0:
        q *= -1
    return q


def kdl_target(M):
    """The rotation a pose [4,4] reaches KDL with: pack_pose -> (w,x,y,z) -> ros_quat -> Rotation::Quaternion.  It differs from
    M[:3,:3] by rounding only (~1e-16), which a solve near a singular configuration can amplify to ~1e-8."""
    w, x, y, z = mat2quat(M)
    return quat_to_matrix(x, y, z, w)


class Kinematics:
    """``robot_kinematics.inverse_kinematics(position, orientation_xyzw, seed)`` on the restatement; `record` collects every
    residual the loops check and `iters` every iteration count, for the fixture generator's margin checks."""

    def __init__(self, model, max_iter=MAX_ITER, eps=EPS, pinv_eps=PINV_EPS):
        self.model, self.max_iter, self.eps, self.pinv_eps = model, max_iter, eps, pinv_eps
        self.record, self.iters = [], []

    def inverse_kinematics(self, position, orientation=None, seed=None):
        R = quat_to_matrix(*orientation)
        q, ok, it = solve(self.model, R[None], np.asarray(position, np.float64)[None], np.asarray(seed, np.float64)[None, :7],
                          self.max_iter, self.eps, self.pinv_eps, self.record)
        self.iters.append(int(it[0]))
        return q[0] if ok[0] else None


def solve_grasps(model, targets, seeds, use_standoff=True, attached=False, accept_diff=2.0, **kw):
    """solve_one_pose_ik for G grasps at once: targets [G,T,4,4] (standoff poses k = 0..T-1; T = 1 without standoff), seeds [K,7]
    -> (reach list of [T,9] | [9], goal list of [9]) in (grasp, seed) order.  All chains of a stage are one vectorised solve."""
    fingers = np.array([0.04, 0.04])
    targets = np.asarray(targets, np.float64)
    G, T = targets.shape[:2]
    K = len(seeds)
    q0 = np.tile(np.asarray(seeds, np.float64)[:, :7], (G, 1))                       # chain c = g * K + k
    pose = lambda k: (np.repeat(targets[:, k, :3, :3], K, 0), np.repeat(targets[:, k, :3, 3], K, 0))
    if not use_standoff:
        q, alive, _ = solve(model, *pose(0), q0, **kw)
        sols = q[:, None]
    else:
        q, alive, _ = solve(model, *pose(T - 1), q0, **kw)
        sols = np.zeros((G * K, T, 7))
        for k in range(T):
            idx = np.nonzero(alive)[0]
            TR, Tt = pose(k)
            qk, ok, _ = solve(model, TR[idx], Tt[idx], q[idx], **kw)
            q[idx] = qk
            sols[idx, k] = qk
            alive[idx[~ok]] = False
    reach, goals = [], []
    for c in np.nonzero(alive)[0]:
        if not use_standoff:
            reach.append(np.concatenate([sols[c, 0], fingers]))
            goals.append(np.concatenate([sols[c, 0], fingers]))
            continue
        traj = sols[c] if attached else sols[c, ::-1]
        if np.linalg.norm(np.diff(traj, axis=0)) < accept_diff:
            reach.append(np.concatenate([traj, np.tile(fingers, (T, 1))], axis=-1))
            goals.append(np.concatenate([traj[0] if not attached else traj[-1], fingers]))
    return reach, goals


def solve_grasp(model, targets, seeds, use_standoff=True, attached=False, accept_diff=2.0, **kw):
    """solve_one_pose_ik for one grasp: targets [T,4,4] (T = 1 without standoff), seeds [K,7] -> (reach list, goal list) in seed order."""
    return solve_grasps(model, np.asarray(targets)[None], seeds, use_standoff, attached, accept_diff, **kw)
