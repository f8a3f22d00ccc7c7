"""Goal-set IK without a GPU: the CPU restatement (tests/ik_restatement.py) against independent kinematics and the reference's
own pipeline (tests/golden/ik_*.npz, tests/golden/make_ik_golden.py), goal_ik.py's pose preparation against the fixtures'
prepared targets, omgx_goal_ik's argument checks, and the IK kernel's register budget."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ik_restatement as ikr
from omg_planner_amd import robot as rb
from omg_planner_amd import scenes as sc
from tests import kernel_build as KB

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
FIXTURES = sorted(GOLDEN.glob("ik_*.npz"))


def load(path):
    with np.load(path, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def model():
    return rb.PandaModel()


def reachable_targets(model, B, seed):
    rng = np.random.RandomState(seed)
    lo, hi = ikr.limits(model)
    q = rng.uniform(lo, hi, (B, 7))
    R, t, _, _ = ikr.hand_kinematics(model, q)
    return q, R, t


def test_jacobian_matches_central_differences(model):
    q, R, t = reachable_targets(model, 256, 1)
    _, _, z, p = ikr.hand_kinematics(model, q)
    J = ikr.jacobian(t, z, p)
    h = 1e-5
    for i in range(7):
        qp, qm = q.copy(), q.copy()
        qp[:, i] += h
        qm[:, i] -= h
        Rp, tp, _, _ = ikr.hand_kinematics(model, qp)
        Rm, tm, _, _ = ikr.hand_kinematics(model, qm)
        np.testing.assert_allclose(J[:, :3, i], (tp - tm) / (2 * h), rtol=0, atol=1e-7)
        W = np.einsum("bij,bkj->bik", (Rp - Rm) / (2 * h), R)  # dR/dq R^T = [w]x
        np.testing.assert_allclose(J[:, 3:, i], np.stack([W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]], -1), rtol=0, atol=1e-7)


def test_solver_arithmetic_is_the_definition(model):
    """The solver's own FK / Jacobian (fk_jacobian, in omg_ik.hip's order through the blob's tables) equals the 4x4 definition, and
    its one-sided Jacobi pseudo-inverse equals the truncated SVD pseudo-inverse (KDL's ChainIkSolverVel_pinv), dropping the same
    singular values."""
    q, R, t = reachable_targets(model, 512, 4)
    _, _, z, p = ikr.hand_kinematics(model, q)
    R2, t2, W = ikr.fk_jacobian(model, q)
    assert np.abs(R2.reshape(-1, 3, 3) - R).max() <= 1e-15 and np.abs(t2 - t).max() <= 1e-15
    J = ikr.jacobian(t, z, p)
    assert np.abs(W - J).max() <= 1e-15
    rng = np.random.RandomState(5)
    d = rng.normal(size=(512, 6))
    S = np.linalg.svd(J, compute_uv=False)
    good = S.min(axis=1) > 1e-2
    np.testing.assert_allclose(ikr.pinv_step_jacobi(J[good], d[good]), ikr.pinv_step(J[good], d[good]), rtol=0, atol=1e-11)
    # a rank-deficient J (two equal rows, one row scaled below pinv_eps): the same truncation
    Jd = J[:64].copy()
    Jd[:, 5] = Jd[:, 4]
    Jd[:, 3] *= 1e-7
    np.testing.assert_allclose(ikr.pinv_step_jacobi(Jd, d[:64]), ikr.pinv_step(Jd, d[:64]), rtol=0, atol=1e-9)


def test_reproducible_transcendentals_are_faithful():
    """ik_sincos / ik_atan2 (the plain-IEEE sin, cos and atan2 omg_ik.hip and the restatement share) agree with the C library's to
    an ulp or two: they exist for bit-reproducibility, not as an approximation."""
    rng = np.random.RandomState(6)
    x = np.concatenate([rng.uniform(-8, 8, 400000), rng.uniform(-1e-3, 1e-3, 1000), [0.0, np.pi, -np.pi / 2, 2.8973, -3.0718]])
    s, c = ikr.ik_sincos(x)
    assert np.abs(s - np.sin(x)).max() <= 2.3e-16 and np.abs(c - np.cos(x)).max() <= 2.3e-16
    y, xx = np.abs(rng.normal(size=400000)), rng.normal(size=400000)
    a, r = ikr.ik_atan2(y, xx), np.arctan2(y, xx)
    assert np.abs(a - r).max() <= 2 * np.spacing(np.pi)
    edge_y, edge_x = np.array([0.0, 0.0, 1.0, 1e-300, 1.0, 0.0]), np.array([1.0, -1.0, 0.0, -1.0, 1e-300, 0.0])
    np.testing.assert_allclose(ikr.ik_atan2(edge_y, edge_x), np.arctan2(edge_y, edge_x), rtol=0, atol=1e-15)


def test_rotvec_branches():
    rng = np.random.RandomState(2)
    # general angles: exp(rotvec) reproduces R
    w = rng.normal(size=(64, 3))
    w *= (rng.uniform(0.1, 3.0, 64) / np.linalg.norm(w, axis=1))[:, None]
    th = np.linalg.norm(w, axis=1)
    k = w / th[:, None]
    Kx = np.zeros((64, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 2] = -k[:, 2], k[:, 1], -k[:, 0]
    Kx -= Kx.transpose(0, 2, 1)
    R = np.eye(3) + np.sin(th)[:, None, None] * Kx + (1 - np.cos(th))[:, None, None] * Kx @ Kx
    np.testing.assert_allclose(ikr.rotvec(R), w, atol=1e-12)
    # identity -> 0; a half turn -> pi times the axis
    assert np.array_equal(ikr.rotvec(np.eye(3)[None]), np.zeros((1, 3)))
    np.testing.assert_allclose(ikr.rotvec(np.diag([1.0, -1.0, -1.0])[None]), [[np.pi, 0, 0]], atol=1e-15)
    np.testing.assert_allclose(ikr.rotvec(np.diag([-1.0, -1.0, 1.0])[None]), [[0, 0, np.pi]], atol=1e-15)


def test_restatement_successes_converge_within_limits(model):
    _, R, t = reachable_targets(model, 200, 3)
    seeds = np.concatenate([rb.HOME_CONFIG[None, :7], ikr.ANCHOR_SEEDS[:12]])
    TR, Tt, S = np.repeat(R, 13, 0), np.repeat(t, 13, 0), np.tile(seeds, (200, 1))
    q, ok, it = ikr.solve(model, TR, Tt, S)
    assert 0.2 < ok.mean() < 1.0 and (it[ok] < ikr.MAX_ITER).all() and (it[~ok] == ikr.MAX_ITER).all()
    lo, hi = ikr.limits(model)
    qs = q[ok]
    assert (qs >= lo).all() and (qs <= hi).all()
    # an independent FK (scenes.hand_pose: position and approach axis)
    pos, zax = sc.hand_pose(model, np.concatenate([qs, np.full((len(qs), 2), 0.04)], axis=1))
    assert np.abs(pos - Tt[ok]).max() <= 1e-6
    assert np.abs(zax - TR[ok][:, :, 2]).max() <= 2e-6


def _post_process(model, goals, reach, start, d):
    """solve_and_process_ik's flip augmentation and filter (planner.py:249-294), numpy, on the restatement's kinematics."""
    if len(goals) == 0 or d["attached"]:
        return goals, reach
    goals, reach = np.array(goals), np.array(reach)
    pad = 0.2

    def flip(g):
        g = g.copy()
        j = g[..., -3]
        g[..., -3] = np.where(j < 0, j + np.pi, np.where(j > 0, j - np.pi, j))
        return g, (g[..., -3] < 2.8973 - pad) & (g[..., -3] > -2.8973 + pad)

    fg, m = flip(goals)
    fr, _ = flip(reach)
    goals, reach = np.concatenate([goals, fg[m]]), np.concatenate([reach, fr[m]])
    Rs = ikr.hand_kinematics(model, start[None, :7])[0][0]
    if d["use_standoff"]:
        t = np.linspace(0, 1, 7)[1:-1]
        pts = (reach[:, -1][:, None] - start[None, None]) * t[None, :, None] + start[None, None]
    else:
        pts = goals[:, None]
    R = ikr.hand_kinematics(model, pts.reshape(-1, 9)[:, :7])[0].reshape(len(goals), -1, 3, 3)
    tr = np.trace(R @ Rs.T, axis1=2, axis2=3)
    with np.errstate(invalid="ignore"):
        ang = np.abs(np.arccos((tr - 1) / 2)) * 180 / np.pi
    xz = R[..., 2, 0] / np.linalg.norm(R[..., :, 0], axis=-1)
    keep = ~((ang > 120) | (xz < -0.3)).any(-1)
    return goals[keep], reach[keep]


@pytest.mark.parametrize("path", FIXTURES, ids=[p.stem for p in FIXTURES])
def test_restatement_reproduces_reference_fixture(model, path):
    d = load(path)
    T = int(d["reach_tail_length"])
    start = d["start"]
    seeds = start[None, :7] if d["one_trial"] else np.concatenate([start[None, :7], ikr.ANCHOR_SEEDS[:int(d["ik_seed_num"])]])
    targets = d["targets"]  # the grasps the reference solved (its parallel path never solves the last one)
    tg = (targets if d["use_standoff"] else targets[:, :1]).copy()
    for g in range(tg.shape[0]):
        for k in range(tg.shape[1]):  # as the reference hands them to KDL (pack_pose -> quaternion)
            tg[g, k, :3, :3] = ikr.kdl_target(tg[g, k])
    reach, goals = ikr.solve_grasps(model, tg, seeds, bool(d["use_standoff"]), bool(d["attached"]))
    if str(d["stage"]) == "process":
        goals, reach = _post_process(model, goals, reach, start, d)
    goals = np.array(goals).reshape(-1, 9)
    reach = np.array(reach).reshape((-1, T, 9) if d["use_standoff"] else (-1, 9))
    assert goals.shape == d["grasps"].shape and reach.shape == d["reach_grasps"].shape
    np.testing.assert_allclose(goals, d["grasps"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(reach, d["reach_grasps"], rtol=0, atol=1e-9)


def test_fixtures_cover_the_issue_cases():
    names = {p.stem for p in FIXTURES}
    assert len(names) >= 8
    ds = [load(p) for p in FIXTURES]
    for key in ("use_standoff", "attached", "ik_parallel", "z_upsample", "y_upsample", "one_trial", "obj_coord"):
        assert {int(d[key]) for d in ds} == {0, 1}, key
    assert any(len(d["grasps"]) > 0 for d in ds) and all(d["grasps"].size < 20000 for d in ds)


@pytest.mark.parametrize("path", FIXTURES, ids=[p.stem for p in FIXTURES])
def test_pose_preparation_matches_fixture(path):
    from omg_planner_amd import goal_ik
    d = load(path)
    p = goal_ik.prepare_poses(d["pose_grasp"], d["object_pose"], bool(d["obj_coord"]), bool(d["z_upsample"]), bool(d["y_upsample"]),
                              int(d["reach_tail_length"]), float(d["standoff_dist"]), bool(d["use_standoff"]), device="cpu").numpy()
    tg = d["targets"] if d["use_standoff"] else d["targets"][:, :1]  # without standoff the reference's T poses are the grasp
    assert p.shape[0] == tg.shape[0] + int(d["ik_parallel"])  # the parallel path never hands the last grasp to a solver
    np.testing.assert_allclose(p[:tg.shape[0]], tg, rtol=0, atol=1e-12)


def test_increment_iks_is_refused():
    from omg_planner_amd import goal_ik
    from omg_planner_amd.config import Config
    with pytest.raises(ValueError, match="increment_iks"):
        goal_ik.solve_raw(rb.PandaModel(), [np.eye(4)[None]], np.eye(4)[None], rb.HOME_CONFIG[None], Config(increment_iks=True),
                          device="cpu")


def test_goal_ik_argument_checks_without_gpu():
    from omg_planner_amd import _lib
    lib = _lib.lib()
    d = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first

    def call(S=2, N=4, begin=(0, 2, 4), K=13, T=5, standoff=1, attached=0, max_iter=100, eps=1e-6, out=d, sols=d, seeds=d):
        hb = (C.c_int32 * len(begin))(*begin) if begin is not None else None
        return lib.omgx_goal_ik(d, 15, d, d, hb, S, N, seeds, K, T, standoff, attached, max_iter, eps, 1e-5, 2.0, out, sols, None, None)

    INV = _lib.OMGX_ERR_INVALID
    assert call(S=-1) == INV and call(N=-1) == INV
    assert call(T=0) == INV and call(T=17) == INV and call(T=5, standoff=0) == INV
    assert call(begin=(0, 3, 2), N=2) == INV and call(begin=(0, 2, 3)) == INV and call(begin=(1, 2, 4)) == INV
    assert call(begin=None) == INV
    assert call(out=None) == INV and call(sols=None) == INV and call(seeds=None) == INV
    assert call(K=0) == INV and call(max_iter=0) == INV and call(eps=-1.0) == INV and call(attached=2) == INV
    assert call(S=2, N=0, begin=(0, 0, 0)) == _lib.OMGX_OK  # nothing to solve: nothing launched


@KB.requires_hipcc
def test_ik_kernel_does_not_spill(tmp_path):
    """k_goal_ik keeps a chain's whole state (the Jacobian's rows, the rotated residual, q, the target) in registers: the
    compiled kernel has no scratch (256 VGPRs + AGPRs, one wave per SIMD)."""
    v = KB.one(KB.kernel_resources("omg_ik.hip", tmp_path), "k_goal_ik")
    assert v["ScratchSize [bytes/lane]"] == 0
    assert v["Occupancy [waves/SIMD]"] >= 1


# ---- the directed cases of tests/ik_cases.py: each is what it claims, away from every threshold, and stable --------------------

import ik_cases as ikc  # noqa: E402


@pytest.fixture(scope="module")
def blocks(model):
    return ikc.newton_blocks(model)


@pytest.fixture(scope="module")
def traces(model, blocks):
    return {name: ikc.trace(model, b.R, b.t, b.seeds, b.k) for name, b in blocks.items()}


def test_trace_is_the_restatements_loop(model, blocks, traces):
    for name, b in blocks.items():
        q, _, _ = ikr.solve(model, b.R, b.t, b.seeds, max_iter=b.k)
        assert np.array_equal(q, traces[name][0]), name


def test_directed_blocks_take_their_branch(model, blocks):
    """Every pair of every block takes the block's branch at its first step; the half turns take all three sub-branches, each
    pair the one of its axis' largest component; the kept near-singular steps are clamped by the limits."""
    for name, b in blocks.items():
        census = ikc.branch_census(model, b.R, b.t, b.seeds, b.k)
        assert census["first"][b.branch].all(), (name, census["counts"])
        assert census["steps"] == b.k * len(b.seeds), name  # nothing converges on the way: every update is compared
        if b.branch == "half_turn":
            for a, sub in enumerate(("half_turn_x", "half_turn_y", "half_turn_z")):
                assert np.array_equal(census["first"][sub], ikc.AXIS_LARGEST[b.axis] == a), (name, sub)
                assert census["counts"][sub] >= 8
        if name == "singular_kept":
            assert census["first"]["clamped"].all()
    lo, hi = ikr.limits(model)
    inside = lambda q: ((q >= lo) & (q <= hi)).all(-1)
    assert inside(blocks["half_turn"].seeds).all()
    assert inside(ikc.SINGULAR).tolist() == [True, True, False]


def test_random_generators_miss_the_directed_branches(model):
    """The gap the directed blocks close: 512 pairs of each random generator of test_gpu_goal_ik.py take no half-turn arm and
    drop no singular value."""
    for k in (1, 5):
        census = ikc.branch_census(model, *ikc.random_pairs(model, 512, k), k)
        print("random pairs, k =", k, census["steps"], census["counts"])
        for b in ("half_turn", "half_turn_x", "half_turn_y", "half_turn_z", "dropped"):
            assert census["counts"][b] == 0, (k, b)
    census = ikc.branch_census(model, *ikc.random_full_solves(model, 512), 100)
    print("random full solves", census["steps"], census["counts"])
    for b in ("half_turn", "half_turn_x", "half_turn_y", "half_turn_z", "dropped"):
        assert census["counts"][b] == 0, b


def _decided(x, lo, hi):
    """A test `every x_i < threshold` is decided away from the threshold: all of x [n,m] below lo, or the largest above hi."""
    top = x.max(-1)
    return bool(((top < lo) | (top > hi)).all())


def test_directed_blocks_keep_their_margins(blocks, traces):
    """No comparison a directed step decides by sits near its threshold, at any of the block's k steps: GetRot's symmetry test
    against 1e-6 (all three asymmetries below 0.5e-6, or one above 2e-6), its identity test against 1e-5 (0.5e-5 / 2e-5), every
    singular value against pinv_eps = 1e-5 (outside [0.5e-5, 2e-5]), and the half turns' largest of xx, yy, zz ahead of the
    next by 0.05.  The one exception is stated with its block: "tiny_turn_identity_4e-7" has the angle the blocks were asked
    with, whose asymmetry 2 sin(4e-7) |axis_i| <= 8e-7 is 20 % below 1e-6, not 50 % (2e-7 away: 1e9 roundings)."""
    for name, (_, steps) in traces.items():
        for i, step in enumerate(steps):
            br = ikc.step_branches(step)
            if name == "tiny_turn_identity_4e-7" and i == 0:
                assert (step["asym"] <= 8.0e-7 * (1 + 1e-9)).all(), name
            else:
                assert _decided(step["asym"], 0.5e-6, 2e-6), (name, i)
            sym = br["half_turn"] | br["identity"]
            assert _decided(step["ident"][sym], 0.5e-5, 2e-5), (name, i)
            assert not ((step["sigma"] >= 0.5e-5) & (step["sigma"] <= 2e-5)).any(), (name, i)
            top = np.sort(step["diag"][br["half_turn"]], axis=-1)
            assert (top[:, 2] - top[:, 1] >= 0.05).all(), (name, i)


def test_near_singular_seeds_bracket_pinv_eps(model):
    for sigma, (a, b) in ((0.0, (0.0, 1e-12)), (ikc.SIGMA_DROPPED, (2e-6, 5e-6)), (ikc.SIGMA_KEPT, (2e-5, 5e-5))):
        _, t, z, p = ikr.hand_kinematics(model, ikc.singular_seeds(sigma))
        S = np.linalg.svd(ikr.jacobian(t, z, p), compute_uv=False)
        assert ((S[:, 5] >= a) & (S[:, 5] < b)).all() and (S[:, 4] > 0.1).all(), (sigma, S[:, 4:])


def test_directed_updates_are_the_definition(model, blocks):
    """One update of the restatement on every directed pair equals clip(q + pinv_step(jacobian, twist_diff)) of the 4x4
    kinematics and LAPACK's SVD, within test_solver_arithmetic_is_the_definition's bars: 1e-11, and 1e-9 where rounding is
    amplified — by a singular value below 1e-2 (that test's own split), or, in "near_half_turn", by the normalisation of an axis
    of length 2e-5 (1e-16 / 2e-5 * pi * |J^+| ~ 1e-10)."""
    lo, hi = ikr.limits(model)
    for name, b in blocks.items():
        R, t, z, p = ikr.hand_kinematics(model, b.seeds)
        J = ikr.jacobian(t, z, p)
        want = np.clip(b.seeds + ikr.pinv_step(J, ikr.twist_diff(R, t, b.R, b.t)), lo, hi)
        got, _, _ = ikr.solve(model, b.R, b.t, b.seeds, max_iter=1)
        small = (np.linalg.svd(J, compute_uv=False).min(-1) <= 1e-2) | (name == "near_half_turn")
        err = np.abs(got - want).max(-1)
        print(name, "restatement - definition:", err[~small].max(initial=0.0), err[small].max(initial=0.0))
        assert (err[~small] <= 1e-11).all() and (err[small] <= 1e-9).all(), name


def test_rotvec_half_turn_arms_return_pi_times_the_axis():
    """All three arms of the half-turn branch, the y-largest one included, on axes with three non-zero components: pi times the
    axis, its largest component positive."""
    for axis, big in zip(ikc.AXES, ikc.AXIS_LARGEST):
        want = np.pi * axis * np.sign(axis[big])
        for theta in (np.pi, np.pi - 1e-7):
            np.testing.assert_allclose(ikr.rotvec(ikc.rotation(axis, theta)[None])[0], want, rtol=0, atol=2e-7)
        np.testing.assert_allclose(ikr.rotvec(ikc.rotation(axis, np.pi)[None])[0], want, rtol=0, atol=1e-15)


def _kdl_route(R):
    H = np.tile(np.eye(4), R.shape[:-2] + (1, 1))
    H[..., :3, :3] = R
    return np.array([ikr.kdl_target(h) for h in H.reshape(-1, 4, 4)]).reshape(R.shape)


def test_directed_blocks_are_stable(model, blocks, traces):
    """A block is compared on the device only where rounding cannot decide it: with its targets through the reference's
    quaternion route (kdl_target: ~1e-16 off) the restatement's result after the block's k updates moves by at most 1e-11, a
    tenth of the device bar.  A block that does not meet this is not compared on the device (ik_cases.newton_blocks)."""
    assert [n for n, b in blocks.items() if not b.on_device] == ["near_half_turn"]
    for name, b in blocks.items():
        if not b.on_device:
            continue
        q, _, _ = ikr.solve(model, _kdl_route(b.R), b.t, b.seeds, max_iter=b.k)
        moved = np.abs(q - traces[name][0]).max()
        print(name, "k =", b.k, "moved", moved)
        assert moved <= 1e-11, (name, moved)


def chain_restatement(model, targets, grasp_begin, seeds, use_standoff=True, accept_diff=2.0, max_iter=ikr.MAX_ITER, record=None):
    """omgx_goal_ik's contract (include/omg_hip.h, section 10) on ikr.solve: targets [N,T,4,4], grasp_begin [S+1], seeds [S,K,7]
    -> (status [N,K], solutions [N,K,T,7], iterations [N,K,1+T] ([N,K,1] without standoff))."""
    targets, seeds = np.asarray(targets, np.float64), np.asarray(seeds, np.float64)
    (N, T), K = targets.shape[:2], seeds.shape[1]
    scene = np.searchsorted(np.asarray(grasp_begin), np.arange(N), side="right") - 1
    q0 = seeds[scene].reshape(N * K, 7)  # chain c = n * K + k
    pose = lambda k: (np.repeat(targets[:, k, :3, :3], K, 0), np.repeat(targets[:, k, :3, 3], K, 0))
    status = np.zeros(N * K, np.int32)
    sols = np.zeros((N * K, T, 7))
    its = np.full((N * K, 1 + T if use_standoff else 1), -1, np.int32)
    q, alive, its[:, 0] = ikr.solve(model, *pose(T - 1 if use_standoff else 0), q0, max_iter=max_iter, record=record)
    status[~alive] = 1
    if not use_standoff:
        sols[:, 0] = q
    else:
        for k in range(T):
            idx = np.nonzero(alive)[0]
            TR, Tt = pose(k)
            q[idx], ok, its[idx, 1 + k] = ikr.solve(model, TR[idx], Tt[idx], q[idx], max_iter=max_iter, record=record)
            sols[idx, k] = q[idx]
            status[idx[~ok]] = 2 + k
            alive[idx[~ok]] = False
        for c in np.nonzero(alive)[0]:
            if not np.linalg.norm(np.diff(sols[c], axis=0)) < accept_diff:
                status[c] = -1
    return status.reshape(N, K), sols.reshape(N, K, T, 7), its.reshape(N, K, -1)


def chain_norms(solutions):
    """The Frobenius norm the acceptance test compares, per chain: [N,K]."""
    return np.sqrt((np.diff(solutions, axis=2) ** 2).sum((-1, -2)))


def run_chain_block(model, b, record=None, route=None, accept_diff=None):
    targets = b.targets
    if route is not None:
        targets = targets.copy()
        targets[..., :3, :3] = route(targets[..., :3, :3])
    return chain_restatement(model, targets, b.grasp_begin, b.seeds, b.use_standoff, b.accept_diff if accept_diff is None else
                             accept_diff, b.max_iter, record)


@pytest.fixture(scope="module")
def chains(model):
    return ikc.chain_blocks(model)


@pytest.mark.parametrize("name", ["accepted", "presolve_fails", "chained_fails_0", "chained_fails_2", "tail_of_one_accepted",
                                  "tail_of_one_rejected", "single_solve_fails", "limits"])
def test_chain_blocks_follow_the_fixture_rules(model, chains, name):
    """make_ik_golden.py's rules for a chain that is compared on the device: no result moves by more than 1e-9 between matrix
    and quaternion-route targets, and every residual a solve checked is at least 0.1 % away from eps; and the block reports
    what ik_cases says it does."""
    b = chains[name]
    record = []
    st, sol, its = run_chain_block(model, b, record)
    st2, sol2, its2 = run_chain_block(model, b, route=_kdl_route)
    assert np.array_equal(st, st2) and np.array_equal(its, its2)
    assert np.abs(sol - sol2).max() <= 1e-9, np.abs(sol - sol2).max()
    res = np.concatenate(record)
    assert (np.abs(res - ikr.EPS) >= 1e-3 * ikr.EPS).all()
    T = b.targets.shape[1]
    if b.status is not None:
        assert (st == b.status).all(), st
    if name == "limits":
        assert b.targets.shape[1] == 16 and b.seeds.shape[1] == 64 and (st == 0).any() and (st > 0).any()
    if b.status in (0, -1) and b.use_standoff:
        assert (its >= 0).all() and (its < b.max_iter).all()
        norm = chain_norms(sol)
        if T > 1:  # accept_diff at half the smallest norm rejects all, at twice the largest accepts all
            assert norm.min() > 1e-3
            assert (run_chain_block(model, b, accept_diff=0.5 * norm.min())[0] == -1).all()
            assert (run_chain_block(model, b, accept_diff=2.0 * norm.max())[0] == 0).all()
        else:
            assert (norm == 0).all()
    if b.status is not None and b.status > 0:  # the failed solve holds max_iter, the ones after it did not run
        j = b.status - 1
        assert (its[..., j] == b.max_iter).all() and (its[..., j + 1:] == -1).all() and (its[..., :j] < b.max_iter).all()
        assert (sol[:, :, max(j, 1):] == 0).all()
