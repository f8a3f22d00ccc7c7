"""omgx_goal_ik / goal_ik.py on the MI355X against the CPU restatement (tests/ik_restatement.py) and the reference's own pipeline
(tests/golden/ik_*.npz), ragged batches against per-scene calls, and one tabletop scene from grasps to a plan."""
from __future__ import annotations

import types
from pathlib import Path

import numpy as np
import pytest

import ik_restatement as ikr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = sorted(GOLDEN.glob("ik_*.npz"))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    from omg_planner_amd import robot as rb
    return rb.PandaModel()


def load(path):
    with np.load(path, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def _rows(R, t):
    return np.concatenate([R.reshape(-1, 9), t], axis=1)


def _device_single(model, dev, R, t, seeds, max_iter=100, want_iterations=False):
    """One solve per (target, seed) pair: no standoff, one scene per pair with its own seed (K = 1)."""
    from omg_planner_amd import ops
    B = R.shape[0]
    targets = torch.as_tensor(_rows(R, t), dtype=torch.float64, device=dev).reshape(B, 1, 12).contiguous()
    sd = torch.as_tensor(seeds, dtype=torch.float64, device=dev).reshape(B, 1, 7).contiguous()
    status, sols, its = ops.goal_ik(ops.robot_blob(model, dev), model.points_per_link, targets, np.arange(B + 1), sd,
                                    use_standoff=False, max_iter=max_iter, want_iterations=want_iterations)
    torch.cuda.synchronize()
    return status.cpu().numpy()[:, 0], sols.cpu().numpy()[:, 0, 0], None if its is None else its.cpu().numpy()[:, 0, 0]


def _random_pairs(model, B, seed, reachable=True):
    rng = np.random.RandomState(seed)
    lo, hi = ikr.limits(model)
    q = rng.uniform(lo, hi, (B, 7))
    R, t, _, _ = ikr.hand_kinematics(model, q)
    if not reachable:
        t = t + rng.normal(0, 0.3, t.shape)
    seeds = np.concatenate([q[:1] * 0 + np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785]), ikr.ANCHOR_SEEDS[:12]])
    return R, t, seeds


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_newton_iterations_match_restatement(dev, model, k):
    """max_iter = k: the joint vector after k updates (or the converged one) on 4096 random (target, seed) pairs, half of the
    targets out of reach — pins the Newton step (FK, twist, pseudo-inverse, clamp) itself."""
    rng = np.random.RandomState(100 + k)
    R, t, _ = _random_pairs(model, 4096, 7 + k, reachable=True)
    t[::2] += rng.normal(0, 0.3, t[::2].shape)
    lo, hi = ikr.limits(model)
    seeds = rng.uniform(lo - 0.3, hi + 0.3, (4096, 7))
    st, q, its = _device_single(model, dev, R, t, seeds, max_iter=k, want_iterations=True)
    qr, ok, itr = ikr.solve(model, R, t, seeds, max_iter=k)
    np.testing.assert_array_equal(st == 0, ok)
    np.testing.assert_array_equal(its, itr)
    assert np.abs(q - qr).max() <= 1e-10, np.abs(q - qr).max()


def test_full_solves_agree_with_restatement(dev, model):
    """4096 reachable targets x 13 seeds, 100 iterations: success flags agree on >= 99.5 % of the solves, solutions on >= 99.5 %
    of the joint successes to 1e-6, and every device success reaches its target by an independent pose_table check."""
    from omg_planner_amd import ops
    R, t, seeds = _random_pairs(model, 4096, 11)
    RR, tt = np.repeat(R, 13, 0), np.repeat(t, 13, 0)
    SS = np.tile(seeds, (4096, 1))
    st, q, its = _device_single(model, dev, RR, tt, SS, want_iterations=True)
    qr, ok, _ = ikr.solve(model, RR, tt, SS)
    dok = st == 0
    assert (dok == ok).mean() >= 0.995, (dok == ok).mean()
    both = dok & ok
    close = np.abs(q[both] - qr[both]).max(axis=1) <= 1e-6
    assert close.mean() >= 0.995, close.mean()
    assert 0.2 < dok.mean() < 1.0
    # independent check: pose_table (the CHOMP path's FK, degree round trip included: ~1e-15 apart) of the device's successes
    qs = np.concatenate([q[dok], np.full((int(dok.sum()), 2), 0.04)], axis=1)
    tab = ops.pose_table(ops.robot_blob(model, dev), model.points_per_link,
                         torch.as_tensor(qs, dtype=torch.float64, device=dev)).cpu().numpy()[:, 7]
    assert np.abs(tab[:, 9:12] - tt[dok]).max() <= 2e-6
    assert np.abs(tab[:, :9].reshape(-1, 3, 3) - RR[dok]).max() <= 2e-6
    lo, hi = ikr.limits(model)
    assert (q[dok] >= lo).all() and (q[dok] <= hi).all()
    hist = np.bincount(its, minlength=101)
    print("iterations histogram (0..100):", hist.tolist())


def _cfg_of(d):
    from omg_planner_amd.config import Config
    return Config(use_standoff=bool(d["use_standoff"]), ik_parallel=bool(d["ik_parallel"]), y_upsample=bool(d["y_upsample"]),
                  reach_tail_length=int(d["reach_tail_length"]), standoff_dist=float(d["standoff_dist"]),
                  ik_seed_num=int(d["ik_seed_num"]))


@pytest.mark.parametrize("path", FIXTURES, ids=[p.stem for p in FIXTURES])
def test_fixture_through_solve_goal_sets_and_drop_in(dev, model, path):
    from omg_planner_amd import goal_ik
    d = load(path)
    cfg = _cfg_of(d)
    kw = dict(attached=bool(d["attached"]), obj_coord=bool(d["obj_coord"]), z_upsample=bool(d["z_upsample"]),
              one_trial=bool(d["one_trial"]), device=dev)
    want_g, want_r = d["grasps"], d["reach_grasps"]
    if str(d["stage"]) == "process":
        gs, rs, counts, failed = goal_ik.solve_goal_sets(model, [d["pose_grasp"]], d["object_pose"][None], d["start"][None], cfg, **kw)
        n = int(counts[0])
        got_g = gs[0, :n].cpu().numpy()
        got_r = rs[0, :n].cpu().numpy()
        if not cfg.use_standoff:
            got_r = got_r[:, 0]
    else:  # solve_goal_set_ik alone (one_trial: the reference's solve_and_process_ik never passes it)
        raw = goal_ik.solve_raw(model, [d["pose_grasp"]], d["object_pose"][None], d["start"][None], cfg, **kw)
        got_g, got_r = raw.goals.cpu().numpy(), raw.reach.cpu().numpy()
        if not cfg.use_standoff:
            got_r = got_r[:, 0]
    assert got_g.shape == want_g.shape and got_r.shape == want_r.shape
    np.testing.assert_allclose(got_g, want_g, rtol=0, atol=1e-6)
    np.testing.assert_allclose(got_r, want_r, rtol=0, atol=1e-6)
    # the drop-ins with the reference's signatures
    planner = types.SimpleNamespace(cfg=cfg, traj=types.SimpleNamespace(start=d["start"]), goal_ik_device=dev)
    target = types.SimpleNamespace(pose=d["obj_pose7"], attached=bool(d["attached"]), name="obj")
    if str(d["stage"]) == "process":
        goal_ik.solve_and_process_ik(planner, target, d["pose_grasp"], bool(d["z_upsample"]), obj_coord=bool(d["obj_coord"]))
        reach, grasps = target.reach_grasps, target.grasps
    else:
        reach, grasps = goal_ik.solve_goal_set_ik(planner, target, None, d["pose_grasp"], one_trial=bool(d["one_trial"]),
                                                  z_upsample=bool(d["z_upsample"]), y_upsample=bool(d["y_upsample"]),
                                                  obj_coord=bool(d["obj_coord"]))
    assert len(grasps) == len(want_g) and len(reach) == len(want_r)
    if len(want_g):
        np.testing.assert_allclose(np.array(grasps), want_g, rtol=0, atol=1e-6)
        np.testing.assert_allclose(np.array(reach), want_r, rtol=0, atol=1e-6)


def _grasps_near(model, center, G, rng, far=0):
    from omg_planner_amd import scenes as sc
    q, pos, _, tree = sc._reach_pool(model)
    idx = np.array(tree.query_ball_point(center, 0.25))
    pick = rng.choice(idx, G, replace=False)
    R, t, _, _ = ikr.hand_kinematics(model, q[pick, :7])
    H = np.tile(np.eye(4), (G, 1, 1))
    H[:, :3, :3], H[:, :3, 3] = R, t
    H[:far, 0, 3] += 3.0
    return H


def test_ragged_batch_equals_per_scene_calls(dev, model):
    """8 scenes with different grasp counts — one with none, one whose grasps are all out of reach — in one call give the
    per-scene calls' results bit for bit."""
    from omg_planner_amd import goal_ik
    from omg_planner_amd.config import Config
    cfg = Config()
    rng = np.random.RandomState(21)
    counts = [5, 0, 3, 7, 4, 1, 6, 2]
    objs, grasps, starts = [], [], []
    for s, G in enumerate(counts):
        obj = np.eye(4)
        obj[:3, 3] = [rng.uniform(0.4, 0.6), rng.uniform(-0.2, 0.2), rng.uniform(0.15, 0.3)]
        H = _grasps_near(model, obj[:3, 3], max(G, 1), rng, far=G if s == 3 else 0)[:G]
        objs.append(obj)
        grasps.append(np.linalg.inv(obj) @ H if G else np.zeros((0, 4, 4)))
        starts.append(np.r_[np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785]) + rng.normal(0, 0.1, 7), 0.04, 0.04])
    gs, rs, cnt, failed = goal_ik.solve_goal_sets(model, grasps, np.stack(objs), np.stack(starts), cfg, device=dev)
    cnt, failed = cnt.cpu().numpy(), failed.cpu().numpy()
    assert cnt[1] == 0 and cnt[3] == 0 and failed[3] == counts[3] - 1  # the parallel path leaves the last grasp unsolved
    assert cnt.sum() > 0
    for s in range(8):
        g1, r1, c1, f1 = goal_ik.solve_goal_sets(model, [grasps[s]], objs[s][None], starts[s][None], cfg, device=dev)
        n = int(c1[0])
        assert n == cnt[s] and int(f1[0]) == failed[s]
        assert torch.equal(gs[s, :n], g1[0, :n]) and torch.equal(rs[s, :n], r1[0, :n])


def test_tabletop_grasps_to_plan(dev, model):
    """A tabletop scene's grasps -> IK -> goal_collision_stats / select_goals -> ChompEngine with use_standoff: 70 iterations
    with finite costs, the final configuration a member of the produced goal set."""
    from omg_planner_amd import goal_ik, goalset, ops
    from omg_planner_amd import scenes as sc
    from omg_planner_amd.config import Config
    from omg_planner_amd.engine import ChompEngine
    cfg = Config(use_standoff=True, timeout=-1)
    scene = sc.make_tabletop_scene(3, grid=32, table_grid=(48, 32, 16))
    obj = scene.objects[scene.target_idx].pose_mat
    rng = np.random.RandomState(5)
    H = _grasps_near(model, obj[:3, 3] + np.array([0, 0, 0.1]), 40, rng)
    start = np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785, 0.04, 0.04])
    gs, rs, cnt, _ = goal_ik.solve_goal_sets(model, [np.linalg.inv(obj) @ H], obj[None], start[None], cfg, device=dev)
    n = int(cnt[0])
    assert n > 0
    batch = sc.pack_table([scene], cfg.layer_kwargs())
    scenes = ops.DeviceScenes(batch, dev)
    col, pot = goalset.goal_collision_stats(ops.robot_blob(model, dev), model.points_per_link, scenes, gs[:, :n].contiguous())
    grasps, reach, _, chosen = goalset.select_goals(list(gs[0, :n].cpu().numpy()), list(rs[0, :n].cpu().numpy()),
                                                    col[0].cpu().numpy(), pot[0].cpu().numpy(), filter_collision=False,
                                                    rng=np.random.RandomState(0))
    assert len(grasps) > 0
    goal_set = np.array(grasps)[None]
    eng = ChompEngine(model, batch, cfg, start[None], goal_set, reach_grasps=np.array(reach)[None], device=dev, ol_alg="MD")
    for t in range(70):
        eng.iterate(t)
    torch.cuda.synchronize()
    info = eng.info.cpu().numpy()
    assert np.isfinite(info[:, 0]).all()
    final = eng.end.cpu().numpy()[0]  # the goal the plan ends at
    assert np.abs(goal_set[0] - final[None]).max(axis=1).min() == 0.0


# ---- the directed cases of tests/ik_cases.py (each proven to take its branch, away from every threshold and stable, by
# test_goal_ik_cpu.py) and the raw contract of omgx_goal_ik (include/omg_hip.h, section 10) -------------------------------------

import ik_cases as ikc  # noqa: E402
from test_goal_ik_cpu import chain_norms, chain_restatement  # noqa: E402

NEWTON_BLOCKS = ["half_turn", "tiny_turn_identity", "tiny_turn_identity_4e-7", "tiny_turn_general", "singular", "singular_dropped",
                 "singular_kept"]
CHAIN_BLOCKS = ["accepted", "presolve_fails", "chained_fails_0", "chained_fails_2", "tail_of_one_accepted", "tail_of_one_rejected",
                "single_solve_fails", "limits"]


@pytest.fixture(scope="module")
def blocks(model):
    return ikc.newton_blocks(model)


@pytest.fixture(scope="module")
def chains(model):
    return ikc.chain_blocks(model)


def test_every_stable_block_is_compared(blocks, chains):
    assert NEWTON_BLOCKS == [n for n, b in blocks.items() if b.on_device] and CHAIN_BLOCKS == list(chains)


@pytest.mark.parametrize("name", NEWTON_BLOCKS)
def test_directed_newton_blocks_match_restatement(dev, model, blocks, name):
    """The joint vector after the block's k updates, every pair of it: GetRot's half-turn arms (x, y, z largest), its identity
    case with the position still off, the general case at 3e-6, and seeds at and next to singular configurations, where the
    pseudo-inverse drops a singular value (sigma_min ~ 0 and 3.2e-6) or keeps a small one (3.2e-5)."""
    b = blocks[name]
    st, q, its = _device_single(model, dev, b.R, b.t, b.seeds, max_iter=b.k, want_iterations=True)
    qr, ok, itr = ikr.solve(model, b.R, b.t, b.seeds, max_iter=b.k)
    np.testing.assert_array_equal(st == 0, ok)
    np.testing.assert_array_equal(its, itr)
    print(name, "max |q - q_ref| =", np.abs(q - qr).max())
    assert np.abs(q - qr).max() <= 1e-10, np.abs(q - qr).max()


def test_half_turn_solves_reach_their_targets(dev, model, blocks):
    """The half-turn pairs run to 100 iterations: what the device reports solved reaches its target by pose_table, as in
    test_full_solves_agree_with_restatement."""
    from omg_planner_amd import ops
    b = blocks["half_turn"]
    st, q, _ = _device_single(model, dev, b.R, b.t, b.seeds)
    dok = st == 0
    assert dok.any()
    qs = np.concatenate([q[dok], np.full((int(dok.sum()), 2), 0.04)], axis=1)
    tab = ops.pose_table(ops.robot_blob(model, dev), model.points_per_link,
                         torch.as_tensor(qs, dtype=torch.float64, device=dev)).cpu().numpy()[:, 7]
    assert np.abs(tab[:, 9:12] - b.t[dok]).max() <= 2e-6
    assert np.abs(tab[:, :9].reshape(-1, 3, 3) - b.R[dok]).max() <= 2e-6
    lo, hi = ikr.limits(model)
    assert (q[dok] >= lo).all() and (q[dok] <= hi).all()


def _device_chains(model, dev, b, accept_diff=None, targets=None, grasp_begin=None, seeds=None):
    from omg_planner_amd import ops
    H = b.targets if targets is None else targets
    K = (b.seeds if seeds is None else seeds).shape[1]
    # the outputs are torch.empty: hand the allocator blocks of their sizes that hold no zeros, so that a slot reads 0 because
    # the kernel wrote it
    poison = [torch.full((H.shape[0], K, H.shape[1], 7), 7.0, dtype=torch.float64, device=dev),
              torch.full((H.shape[0], K, 1 + H.shape[1]), 7, dtype=torch.int32, device=dev)]
    del poison
    rows = np.concatenate([H[..., :3, :3].reshape(*H.shape[:2], 9), H[..., :3, 3]], axis=-1)
    out = ops.goal_ik(ops.robot_blob(model, dev), model.points_per_link, torch.as_tensor(rows, dtype=torch.float64, device=dev).contiguous(),
                      b.grasp_begin if grasp_begin is None else grasp_begin,
                      torch.as_tensor(b.seeds if seeds is None else seeds, dtype=torch.float64, device=dev).contiguous(),
                      use_standoff=b.use_standoff, max_iter=b.max_iter, accept_diff=b.accept_diff if accept_diff is None else accept_diff,
                      want_iterations=True)
    torch.cuda.synchronize()
    return out


def _check_contract(model, b, got, want):
    """status and iterations integer-equal, solutions to 1e-6 (the fixture tests' bar); per chain: the slots after a failed solve
    exactly 0, the failed solve's own slot non-zero and inside the limits, max_iter in its iterations entry and -1 after it."""
    st, sol, its = (x.cpu().numpy() for x in got)
    rst, rsol, rits = want
    np.testing.assert_array_equal(st, rst)
    np.testing.assert_array_equal(its, rits)
    assert np.abs(sol - rsol).max() <= 1e-6, np.abs(sol - rsol).max()
    lo, hi = ikr.limits(model)
    T = sol.shape[2]
    for n, k in np.ndindex(st.shape):
        j = int(st[n, k]) - 1  # the solve that failed: 0 the first, 1 + t the chained solve of pose t
        if j < 0:
            assert (its[n, k] >= 0).all() and (its[n, k] < b.max_iter).all() and (sol[n, k] != 0).any(axis=-1).all()
            continue
        assert its[n, k, j] == b.max_iter and (its[n, k, j + 1:] == -1).all() and (its[n, k, :j] < b.max_iter).all()
        slot = j - 1 if b.use_standoff else 0  # the pre-solve of a chain with standoff has no slot
        assert (sol[n, k, slot + 1:] == 0.0).all()
        if slot >= 0:
            assert (sol[n, k, slot] != 0).any() and (sol[n, k, slot] >= lo).all() and (sol[n, k, slot] <= hi).all()
    return st, sol, its


@pytest.fixture(scope="module")
def chain_refs(model, chains):
    return {n: chain_restatement(model, b.targets, b.grasp_begin, b.seeds, b.use_standoff, b.accept_diff, b.max_iter)
            for n, b in chains.items()}


@pytest.mark.parametrize("name", CHAIN_BLOCKS)
def test_chain_contract(dev, model, chains, chain_refs, name):
    """status 0 / 1 / 2 + k / -1, the solutions' slots and the iterations' entries of section 10, chain by chain.  A pose 3 m away
    at k = T - 1 fails the pre-solve, which solves that pose: status 1, never 2 + (T - 1); T = 1 with standoff has a zero
    norm, accepted under accept_diff = 2 and rejected under 0."""
    b = chains[name]
    st, _, _ = _check_contract(model, b, _device_chains(model, dev, b), chain_refs[name])
    if b.status is not None:
        assert (st == b.status).all()


def test_accept_diff_rejects_and_accepts(dev, model, chains, chain_refs):
    """The accepted chains again with accept_diff at half the smallest Frobenius norm of theirs (the restatement's): all -1;
    at twice the largest: all 0.  Their solutions do not depend on it."""
    b = chains["accepted"]
    rst, rsol, rits = chain_refs["accepted"]
    norm = chain_norms(rsol)
    for accept_diff, status in ((0.5 * norm.min(), -1), (2.0 * norm.max(), 0)):
        st, _, _ = _check_contract(model, b, _device_chains(model, dev, b, accept_diff), (np.full_like(rst, status), rsol, rits))
        assert (st == status).all()


def test_limits_call_equals_per_scene_calls(dev, model, chains):
    """T = OMGX_IK_MAX_TAIL and K = OMGX_IK_MAX_SEEDS, an empty scene before the full one: bit for bit what a call per scene
    gives; one more pose or seed is refused."""
    from omg_planner_amd import _lib
    b = chains["limits"]
    assert b.targets.shape[1] == 16 and b.seeds.shape[1] == 64 and list(b.grasp_begin) == [0, 0, 2]
    st, sol, its = _device_chains(model, dev, b)
    e_st, e_sol, e_its = _device_chains(model, dev, b, targets=b.targets[:0], grasp_begin=[0, 0], seeds=b.seeds[:1])
    assert e_st.shape == (0, 64) and e_sol.shape == (0, 64, 16, 7) and e_its.shape == (0, 64, 17)
    f_st, f_sol, f_its = _device_chains(model, dev, b, grasp_begin=[0, 2], seeds=b.seeds[1:])
    assert torch.equal(st, f_st) and torch.equal(sol, f_sol) and torch.equal(its, f_its)
    with pytest.raises(_lib.OmgHipError):
        _device_chains(model, dev, b, targets=np.concatenate([b.targets, b.targets[:, :1]], axis=1))
    with pytest.raises(_lib.OmgHipError):
        _device_chains(model, dev, b, seeds=np.concatenate([b.seeds, b.seeds[:, :1]], axis=1))
