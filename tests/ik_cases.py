"""Directed inputs for the goal-set IK tests (test_goal_ik_cpu.py, test_gpu_goal_ik.py): the branches of omg_ik.hip that random
poses do not reach — KDL GetRot's half turn, its identity case, the truncated pseudo-inverse — and chains for the raw contract of
omgx_goal_ik (include/omg_hip.h, section 10).  Pure numpy, deterministic: nothing here draws a random number.

`newton_blocks(model)` -> {name: Block(R [B,3,3], t [B,3], seeds [B,7], k, branch)}: B (target, seed) pairs compared after k
Newton updates, every one of which takes `branch` (a key of branch_census's "first") at its first step.
`chain_blocks(model)` -> {name: ChainBlock}: calls of omgx_goal_ik with standoff, and what each must report.
`trace` / `branch_census` run the restatement's steps (ik_restatement.solve's loop) and record which branch every step took."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import ik_restatement as ikr

HOME = np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785])

# Singular configurations of the arm (sigma_min of the hand Jacobian < 1e-14), polished by Newton steps on u_min^T J(q) v_min from
# Nelder-Mead minima of sigma_min; the first two lie inside the padded limits, the third does not (joint 3 = -3.82; a seed is not
# clamped before its first step).  SLOPE: d sigma_min / d q[3] at each, by numpy's SVD at +-1e-4 (the other joints move sigma_min
# 20 times less, or not at all).
SINGULAR = np.array([
    [-0.637900000000009, -0.6276999999870592, 0.07720000007590712, -0.4282646149598547, 1.5707963267056402, 1.668399890098837,
     1.1646],
    [-0.8755999999999996, 0.9749999999985407, 1.6254000000000486, -0.4670024236484786, 3.022992611846906e-11, 0.36810000000007653,
     -1.7528],
    [-0.4821000000000015, 0.7306999999590497, -3.820200000029488, -0.4105887048523777, -1.570796326760445, 0.6615006020418859,
     -1.2488]])
SINGULAR_JOINT = 3
SINGULAR_SLOPE = np.array([0.156481, 0.136076, 0.130851])
SIGMA_DROPPED, SIGMA_KEPT = 3.2e-6, 3.2e-5  # the geometric middles of [2e-6, 5e-6] and [2e-5, 5e-5]: pinv_eps = 1e-5 between them

# unit axes with a clear largest component: the coordinate axes, then three distinct non-zero components of mixed signs, the
# largest of either sign (GetRot returns a half turn's axis with its largest component positive)
_MIXED = [(0.8, -0.5, 0.33), (-0.8, 0.33, -0.5), (-0.4, 0.85, 0.3), (0.3, -0.85, -0.4), (0.35, -0.45, 0.8), (-0.45, 0.3, -0.8)]
AXES = np.array([(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)] + [tuple(np.array(a) / np.linalg.norm(a)) for a in _MIXED])
AXIS_LARGEST = np.array([0, 1, 2, 0, 0, 1, 1, 2, 2])


def inner_configs(model, n, first=0):
    """n joint vectors inside the padded limits (the middle 80 % of each range), a Weyl sequence: no random draw."""
    lo, hi = ikr.limits(model)
    i = np.arange(first + 1, first + n + 1, dtype=np.float64)[:, None]
    frac = np.mod(i * np.sqrt(np.array([2.0, 3.0, 5.0, 7.0, 11.0, 13.0, 17.0]))[None], 1.0)
    return lo + (hi - lo) * (0.1 + 0.8 * frac)


def rotation(axis, theta):
    """Rodrigues: [3,3] of the turn by theta about the unit axis."""
    k = np.asarray(axis, np.float64)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)


def _turned(model, thetas, n_seeds, first, k, branch):
    """Targets FK(seed) . Rot(axis, theta), 3 cm off in translation, for every axis x theta x seed."""
    q = inner_configs(model, n_seeds, first)
    Rq, tq, _, _ = ikr.hand_kinematics(model, q)
    R, t, seeds = [], [], []
    for a, axis in enumerate(AXES):
        for theta in thetas:
            for s in range(n_seeds):
                R.append(Rq[s] @ rotation(axis, theta))
                t.append(tq[s] + 0.03 * np.roll([1.0, -0.6, 0.4], a + s))
                seeds.append(q[s])
    return SimpleNamespace(R=np.array(R), t=np.array(t), seeds=np.array(seeds), k=k, branch=branch, on_device=True,
                           axis=np.repeat(np.arange(len(AXES)), len(thetas) * n_seeds))


def singular_seeds(sigma):
    """The three singular configurations moved off along SINGULAR_JOINT to sigma_min ~ sigma (0: not moved)."""
    q = SINGULAR.copy()
    q[:, SINGULAR_JOINT] += sigma / SINGULAR_SLOPE
    return q


def _singular(model, sigma, n_targets, k, branch):
    qs = singular_seeds(sigma)
    Rq, tq, _, _ = ikr.hand_kinematics(model, inner_configs(model, n_targets, first=40))
    return SimpleNamespace(R=np.tile(Rq, (3, 1, 1)), t=np.tile(tq, (3, 1)), seeds=np.repeat(qs, n_targets, 0), k=k, branch=branch,
                           on_device=True)


def newton_blocks(model):
    """k is the largest number of updates (up to 3) at which the block keeps its margins and its stability
    (test_goal_ik_cpu.py: test_directed_blocks_keep_their_margins, test_directed_blocks_are_stable).  "near_half_turn" is not
    stable even at k = 1 — its axis is a difference of 2e-5 between entries of size 1, so a rounding of the target moves the
    update by up to 1.4e-10 — and is therefore checked on the CPU only (on_device False)."""
    blocks = {
        "half_turn": _turned(model, (np.pi, np.pi - 1e-7), 4, 0, 3, "half_turn"),
        "near_half_turn": _turned(model, (np.pi - 1e-5,), 4, 8, 1, "general_neg"),
        "tiny_turn_identity": _turned(model, (2e-7,), 4, 16, 3, "identity"),
        "tiny_turn_identity_4e-7": _turned(model, (4e-7,), 4, 16, 3, "identity"),
        "tiny_turn_general": _turned(model, (3e-6,), 4, 24, 2, "general_pos"),
        "singular": _singular(model, 0.0, 6, 3, "dropped"),
        "singular_dropped": _singular(model, SIGMA_DROPPED, 6, 3, "dropped"),
        "singular_kept": _singular(model, SIGMA_KEPT, 6, 1, "kept_small"),
    }
    blocks["near_half_turn"].on_device = False
    return blocks


def random_pairs(model, B, k=1):
    """The (target, seed) pairs of test_gpu_goal_ik.test_newton_iterations_match_restatement at k, its first B."""
    rng = np.random.RandomState(7 + k)
    lo, hi = ikr.limits(model)
    R, t, _, _ = ikr.hand_kinematics(model, rng.uniform(lo, hi, (4096, 7)))
    rng = np.random.RandomState(100 + k)
    t[::2] += rng.normal(0, 0.3, t[::2].shape)
    return R[:B], t[:B], rng.uniform(lo - 0.3, hi + 0.3, (4096, 7))[:B]


def random_full_solves(model, B):
    """The first B solves of test_gpu_goal_ik.test_full_solves_agree_with_restatement (targets x 13 seeds, target-major)."""
    rng = np.random.RandomState(11)
    lo, hi = ikr.limits(model)
    n = -(-B // 13)
    R, t, _, _ = ikr.hand_kinematics(model, rng.uniform(lo, hi, (4096, 7))[:n])
    seeds = np.concatenate([HOME[None], ikr.ANCHOR_SEEDS[:12]])
    return np.repeat(R, 13, 0)[:B], np.repeat(t, 13, 0)[:B], np.tile(seeds, (n, 1))[:B]


def trace(model, R, t, seeds, k, eps=ikr.EPS, pinv_eps=ikr.PINV_EPS):
    """ik_restatement.solve's loop for k updates, recording per step the quantities its branches compare, for the chains still
    running: -> (q [B,7], steps), steps a list of dicts with
      idx [n] the chains; asym [n,3] |d1-d3|, |d2-d6|, |d5-d7| of rel = R^T . target R; ident [n,4] |d1+d3|, |d2+d6|, |d5+d7|,
      |trace - 3|; f [n] the cosine term; diag [n,3] xx, yy, zz of the half-turn arm; sigma [n,6] numpy's singular values of the
      Jacobian; clamped [n,7] the joints the limits moved."""
    lo, hi = ikr.limits(model)
    q = np.array(seeds, np.float64).copy()
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    live = np.arange(q.shape[0])
    steps = []
    for _ in range(k):
        if live.size == 0:
            break
        Rq, tq, W = ikr.fk_jacobian(model, q[live])
        d = ikr.twist_residual(Rq, tq, R[live], t[live])
        going = ~(np.abs(d).max(-1) <= eps)
        live, Rq, W, d = live[going], Rq[going], W[going], d[going]
        if live.size == 0:
            break
        TRf = R[live].reshape(-1, 9)
        r = np.stack([Rq[:, a] * TRf[:, c] + Rq[:, 3 + a] * TRf[:, 3 + c] + Rq[:, 6 + a] * TRf[:, 6 + c]
                      for a in range(3) for c in range(3)], -1)  # twist_residual's rel
        v = q[live] + ikr.pinv_step_jacobi(W, d, pinv_eps)
        q[live] = np.clip(v, lo, hi)
        steps.append(dict(idx=live.copy(),
                          asym=np.abs(np.stack([r[:, 1] - r[:, 3], r[:, 2] - r[:, 6], r[:, 5] - r[:, 7]], -1)),
                          ident=np.abs(np.stack([r[:, 1] + r[:, 3], r[:, 2] + r[:, 6], r[:, 5] + r[:, 7], r[:, 0] + r[:, 4] + r[:, 8] - 3], -1)),
                          f=(r[:, 0] + r[:, 4] + r[:, 8] - 1) / 2, diag=(r[:, [0, 4, 8]] + 1) / 2,
                          sigma=np.linalg.svd(W, compute_uv=False), clamped=(v < lo) | (v > hi)))
    return q, steps


BRANCHES = ("half_turn_x", "half_turn_y", "half_turn_z", "half_turn", "identity", "general_neg", "general_pos", "dropped",
            "kept_small", "clamped")


def step_branches(step, pinv_eps=ikr.PINV_EPS):
    """{branch: [n] bool} of one step of `trace`, by the comparisons of omg_ik.hip's kdl_rotvec and of the truncation."""
    e, e2 = ikr.KDL_EPSILON, 10 * ikr.KDL_EPSILON
    sym = (step["asym"] < e).all(-1)
    ident = sym & (step["ident"] < e2).all(-1)
    half = sym & ~ident
    xx, yy, zz = step["diag"].T
    hx = half & (xx > yy) & (xx > zz)
    hy = half & ~hx & (yy > zz)
    smin = step["sigma"].min(-1)
    return dict(half_turn_x=hx, half_turn_y=hy, half_turn_z=half & ~hx & ~hy, half_turn=half, identity=ident,
                general_neg=~sym & (step["f"] < 0), general_pos=~sym & (step["f"] >= 0), dropped=smin < pinv_eps,
                kept_small=(smin >= pinv_eps) & (smin < 10 * pinv_eps), clamped=step["clamped"].any(-1))


def branch_census(model, R, t, seeds, k):
    """Runs the restatement's steps on the pairs and counts the branches taken: -> dict(steps = Newton steps made,
    counts = {branch: steps that took it}, first = {branch: [B] bool, the pair's first step took it})."""
    _, steps = trace(model, R, t, seeds, k)
    B = np.asarray(seeds).shape[0]
    counts = {b: 0 for b in BRANCHES}
    first = {b: np.zeros(B, bool) for b in BRANCHES}
    for i, step in enumerate(steps):
        for b, hit in step_branches(step).items():
            counts[b] += int(hit.sum())
            if i == 0:
                first[b][step["idx"]] = hit
    return dict(steps=sum(len(s["idx"]) for s in steps), counts=counts, first=first)


# ---- chains -------------------------------------------------------------------------------------------------------------------

CHAIN_MAX_ITER = 100
STANDOFF = 0.08


def standoff_poses(model, q, T):
    """[G,T,4,4]: the hand poses of the configurations q [G,7] and their straight-line standoffs (goal_ik.prepare_poses'), k = 0
    the pose itself."""
    Rq, tq, _, _ = ikr.hand_kinematics(model, q)
    H = np.tile(np.eye(4), (len(q), T, 1, 1))
    H[:, :, :3, :3] = Rq[:, None]
    back = -STANDOFF * np.linspace(0, 1, T, endpoint=False)
    H[:, :, :3, 3] = tq[:, None] + back[None, :, None] * Rq[:, None, :, 2]
    return H


def _near_seeds(q):
    """Two seeds a few tenths of a radian off each configuration: [G,2,7]."""
    off = np.array([[0.10, -0.08, 0.12, 0.09, -0.11, 0.07, -0.10], [-0.05, 0.12, -0.07, 0.15, 0.06, -0.09, 0.13]])
    return q[:, None] + off[None]


def chain_blocks(model):
    """{name: ChainBlock(targets [N,T,4,4], grasp_begin [S+1], seeds [S,K,7], use_standoff, accept_diff, max_iter, status)}:
    `status` is what every chain of the block must report (None: see the block's test).  One scene per grasp except "limits"."""
    q = inner_configs(model, 4, first=60)
    out = {}

    def block(name, targets, seeds, status, accept_diff=2.0, use_standoff=True, grasp_begin=None, max_iter=CHAIN_MAX_ITER):
        gb = np.arange(len(targets) + 1) if grasp_begin is None else np.asarray(grasp_begin)
        out[name] = SimpleNamespace(targets=targets, grasp_begin=gb, seeds=seeds, use_standoff=use_standoff,
                                    accept_diff=accept_diff, max_iter=max_iter, status=status)

    H5, seeds = standoff_poses(model, q, 5), _near_seeds(q)
    block("accepted", H5, seeds, 0)
    for name, k, status in (("presolve_fails", 4, 1), ("chained_fails_0", 0, 2), ("chained_fails_2", 2, 4)):
        far = H5.copy()
        far[:, k, 0, 3] += 3.0
        block(name, far, seeds, status)  # pose T-1 is the pre-solve's: 3 m away there is status 1, never 2 + (T-1)
    H1 = standoff_poses(model, q, 1)
    block("tail_of_one_accepted", H1, seeds, 0, accept_diff=2.0)
    block("tail_of_one_rejected", H1, seeds, -1, accept_diff=0.0)  # !(0 < 0): rejected
    far = H1.copy()
    far[:, 0, 0, 3] += 3.0
    block("single_solve_fails", far, seeds, 1, use_standoff=False)
    # at the limits: T = OMGX_IK_MAX_TAIL, K = OMGX_IK_MAX_SEEDS, two scenes, the first one empty (its seeds are never to be read);
    # 20 updates: from seeds this far off, a chain at 100 moves by 7e-8 between the two target routes, at 20 by 4e-11
    K = 64
    pool = np.concatenate([HOME[None], ikr.ANCHOR_SEEDS[:12], inner_configs(model, K - 13, first=80)])
    block("limits", standoff_poses(model, q[:2], 16), np.stack([np.zeros((K, 7)), pool]), None, grasp_begin=[0, 0, 2],
          max_iter=20)
    return out
