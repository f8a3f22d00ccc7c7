"""omgx_select_goals / goalset.setup_goal_sets / setup_goal_set / pipeline.plan_grasps on the MI355X: the kernel against
goalset.select_goals (integer equality), ragged batches against per-scene calls, the batched set-up against the host loop on the
same statistics, the drop-in against the reference's own setup_goal_set (tests/golden/setup_*.npz), and tabletop scenes from
grasps to plans."""
from __future__ import annotations

import types
from pathlib import Path

import numpy as np
import pytest

from test_goal_select_cpu import TakeAll, goal_sets, reference_rows  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = sorted(GOLDEN.glob("setup_*.npz"))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    from omg_planner_amd import robot as rb
    return rb.PandaModel()


def ragged_batch(S, seed):
    rng = np.random.RandomState(seed)
    counts = np.concatenate([[0, 1, 2, 65, 2000], rng.randint(0, 2000, S - 5)])
    kinds = ["random", "clustered", "adversarial"]
    sets = [goal_sets(kinds[s % 3], int(n), rng) for s, n in enumerate(counts)]
    G = int(counts.max())
    goals = np.zeros((S, G, 9))
    col = np.zeros((S, G), np.float32)
    for s, g in enumerate(sets):
        goals[s, :len(g)] = g
        col[s, :len(g)] = rng.randint(0, 9, len(g))
    return counts, sets, goals, col


@pytest.mark.parametrize("fc,fd", [(True, True), (False, True), (True, False), (False, False)])
def test_kernel_equals_select_goals(dev, fc, fd):
    from omg_planner_amd import ops
    counts, sets, goals, col = ragged_batch(40, 1)
    d_goals = torch.as_tensor(goals, device=dev)
    d_col = torch.as_tensor(col, device=dev)
    cand, num, free = ops.select_goals(d_goals, counts, d_col if fc else None, 5, fd)
    torch.cuda.synchronize()
    cand, num, free = cand.cpu().numpy(), num.cpu().numpy(), free.cpu().numpy()
    for s, g in enumerate(sets):
        want = reference_rows(g, col[s, :len(g)], 5, fc, fd)
        assert num[s] == want.size, s
        assert np.array_equal(cand[s, :num[s]], want), s
        assert free[s] == (int((col[s, :len(g)] <= 5).sum()) if fc else len(g)), s


def test_ragged_batch_equals_per_scene_calls_and_device_counts(dev):
    from omg_planner_amd import ops
    counts, sets, goals, col = ragged_batch(24, 2)
    d_goals, d_col = torch.as_tensor(goals, device=dev), torch.as_tensor(col, device=dev)
    cand, num, free = ops.select_goals(d_goals, counts, d_col)
    cand2, num2, free2 = ops.select_goals(d_goals, torch.as_tensor(counts, device=dev), d_col)  # counts checked on the device
    bad = counts.copy()
    bad[3] = goals.shape[1] + 1
    _, num3, free3 = ops.select_goals(d_goals, torch.as_tensor(bad, device=dev), d_col)
    torch.cuda.synchronize()
    n = num.cpu().numpy()
    assert torch.equal(num, num2) and torch.equal(free, free2)
    assert num3.cpu().numpy()[3] == -1 and free3.cpu().numpy()[3] == -1
    assert np.array_equal(np.delete(num3.cpu().numpy(), 3), np.delete(n, 3))
    for s, g in enumerate(sets):
        one = torch.as_tensor(g.reshape(1, -1, 9), device=dev).contiguous()
        c1, n1, f1 = ops.select_goals(one, [len(g)], d_col[s:s + 1, :len(g)].contiguous())
        assert int(n1.cpu()[0]) == n[s] and int(f1.cpu()[0]) == int(free.cpu()[s])
        assert torch.equal(c1[0, :n[s]], cand[s, :n[s]]) and torch.equal(cand2[s, :n[s]], cand[s, :n[s]])


def _tabletop(dev, model, S, G, seed):
    from omg_planner_amd import ops
    from omg_planner_amd import scenes as sc
    rng = np.random.RandomState(seed)
    scenes = [sc.make_tabletop_scene(s, grid=32, table_grid=(48, 32, 16)) for s in range(S)]
    counts = np.array([G, 0, G // 2, 1] + [G] * (S - 4))[:S]
    goals = np.zeros((S, G, 9))
    for s in range(S):
        goals[s] = sc.make_goal_set(s, G) + np.r_[rng.normal(0, 0.4, (G, 7)).T, np.zeros((2, G))].T
    reach = goals[:, :, None, :] + rng.normal(0, 0.02, (S, G, 5, 9))
    reach[:, :, -1] = goals
    table = ops.DeviceScenes.from_scenes(scenes, device=dev)
    return scenes, table, counts, torch.as_tensor(goals, device=dev), torch.as_tensor(reach, device=dev)


def test_setup_goal_sets_equals_host_loop(dev, model):
    from omg_planner_amd import goalset, ops
    from omg_planner_amd.config import Config
    cfg = Config(goal_set_max_num=30)
    S, G = 6, 120
    _, table, counts, gs, rs = _tabletop(dev, model, S, G, 3)
    robot = ops.robot_blob(model, dev)
    drawn = np.random.RandomState(9)
    out = goalset.setup_goal_sets(robot, model.points_per_link, table, gs, rs, counts, cfg, rng=drawn)
    col, pot = goalset.goal_collision_stats(robot, model.points_per_link, table, gs)
    col, pot = col.cpu().numpy(), pot.cpu().numpy()
    rng = np.random.RandomState(9)
    K = out[0].shape[1]
    want_g, want_r, want_p = np.zeros((S, K, 9)), np.zeros((S, K, 5, 9)), np.zeros((S, K), np.float32)
    for s in range(S):
        n = int(counts[s])
        g, r, p, _ = goalset.select_goals(list(gs[s, :n].cpu().numpy()), list(rs[s, :n].cpu().numpy()), col[s, :n], pot[s, :n],
                                          cfg.allow_collision_point, cfg.goal_set_max_num, rng=rng)
        assert out[3][s] == len(g)
        if len(g):
            want_g[s, :len(g)], want_r[s, :len(g)], want_p[s, :len(g)] = np.array(g), r, p
    assert (out[3] > 0).sum() >= 3 and out[3].max() == 30
    assert torch.equal(out[0], torch.as_tensor(want_g, device=dev))
    assert torch.equal(out[1], torch.as_tensor(want_r, device=dev))
    assert torch.equal(out[2], torch.as_tensor(want_p, device=dev))
    assert rng.randint(1 << 30) == drawn.randint(1 << 30)  # the stream was consumed as by the loop


class _FixtureCost:
    def __init__(self, d, dev):
        self.d, self.dev = d, dev

    def batch_obstacle_cost(self, goal_set, special_check_id=0, uncheck_finger_collision=-1):
        o = special_check_id
        n = len(goal_set)
        pot = torch.as_tensor(self.d[f"pot_{o}"], device=self.dev).reshape(n, 1, 1)
        col = torch.as_tensor(self.d[f"collide_{o}"], device=self.dev).reshape(n, 1, 1)
        return pot, None, np.arange(n, dtype=np.float64).reshape(n, 1), col


@pytest.mark.parametrize("path", FIXTURES, ids=[p.stem for p in FIXTURES])
def test_drop_in_reproduces_reference_fixture(dev, path):
    from omg_planner_amd import goalset
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    cfg = types.SimpleNamespace(allow_collision_point=int(d["allow_collision_point"]), goal_set_max_num=int(d["goal_set_max_num"]),
                                silent=True)
    objs = [types.SimpleNamespace(name=f"obj_{o}", grasps=list(d[f"goals_{o}"]), reach_grasps=list(d[f"reach_{o}"]),
                                  compute_grasp=bool(d[f"compute_grasp_{o}"]), grasp_potentials=[], grasp_vis_points=[], seeds=[])
            for o in range(int(d["num_objects"]))]
    planner = types.SimpleNamespace(cfg=cfg, cost=_FixtureCost(d, dev), goal_ik_device=dev)
    np.random.seed(int(d["seed"]))
    goalset.setup_goal_set(planner, types.SimpleNamespace(objects=objs), bool(d["filter_collision"]), bool(d["filter_diversity"]))
    for o, ob in enumerate(objs):
        k = int(d[f"out_count_{o}"])
        assert len(ob.grasps) == k and not ob.compute_grasp
        assert np.array_equal(np.array(ob.grasps).reshape(k, 9), d[f"out_grasps_{o}"])
        if not bool(d[f"compute_grasp_{o}"]) or len(d[f"goals_{o}"]) == 0:
            continue
        assert np.array_equal(np.asarray(ob.reach_grasps).reshape(-1), d[f"out_reach_{o}"].reshape(-1))
        pot = np.concatenate([np.asarray(p).reshape(-1) for p in ob.grasp_potentials]) if ob.grasp_potentials else np.zeros(0)
        vis = np.concatenate([np.asarray(v).reshape(-1) for v in ob.grasp_vis_points]) if ob.grasp_vis_points else np.zeros(0)
        assert np.array_equal(pot, d[f"out_potentials_{o}"]) and np.array_equal(vis, d[f"out_vis_{o}"])
        assert np.array_equal(np.array(ob.seeds).reshape(-1, 9), d[f"out_seeds_{o}"])


def _grasps(model, scene, G, rng, far=False):
    import ik_restatement as ikr
    from omg_planner_amd import scenes as sc
    obj = scene.objects[scene.target_idx].pose_mat
    q, _, _, tree = sc._reach_pool(model)
    idx = np.array(tree.query_ball_point(obj[:3, 3] + np.array([0, 0, 0.1]), 0.25))
    R, t, _, _ = ikr.hand_kinematics(model, q[rng.choice(idx, G, replace=False), :7])
    H = np.tile(np.eye(4), (G, 1, 1))
    H[:, :3, :3], H[:, :3, 3] = R, t
    if far:
        H[:, 0, 3] += 3.0  # out of reach: no goal survives IK
    return np.linalg.inv(obj) @ H


def test_plan_grasps_tabletop(dev, model):
    """4 scenes, two without reachable grasps: flagged, not planned; the others' bits equal the hand-chained stages and a run
    without the goal-less scenes (same layout), costs finite, each plan ending on a member of its goal set."""
    from omg_planner_amd import goal_ik, goalset, ops, pipeline
    from omg_planner_amd import scenes as sc
    from omg_planner_amd.config import Config
    from omg_planner_amd.engine import ChompEngine
    cfg = Config(use_standoff=True, timeout=-1, silent=True)
    scenes = [sc.make_tabletop_scene(s, grid=32, table_grid=(48, 32, 16)) for s in (3, 4, 5, 6)]
    rng = np.random.RandomState(5)
    grasps = [_grasps(model, scenes[0], 40, rng), _grasps(model, scenes[1], 20, rng, far=True), _grasps(model, scenes[2], 40, rng),
              np.zeros((0, 4, 4))]
    start = np.tile(np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785, 0.04, 0.04]), (4, 1))
    res = pipeline.plan_grasps(model, scenes, grasps, start, cfg, ol_alg="MD", rng=np.random.RandomState(0), device=dev)
    assert res.planned.tolist() == [True, False, True, False]
    assert (res.goal_idx.cpu().numpy()[[1, 3]] == -1).all() and torch.isnan(res.info[[1, 3]]).all()
    info = res.info.cpu().numpy()
    assert np.isfinite(info[[0, 2], 0]).all()
    gi = res.goal_idx.cpu().numpy()
    traj = res.traj.cpu().numpy()
    for s in (0, 2):
        members = res.goal_set[s, :res.goal_counts[s]].cpu().numpy()
        assert np.abs(members - res.engine.end.cpu().numpy()[[0, 2].index(s)][None]).max(axis=1).min() == 0.0
        assert 0 <= gi[s] < res.goal_counts[s]
    # hand-chained
    objs = np.stack([s_.objects[0].pose_mat for s_ in scenes])
    gs, rs, cnt, _ = goal_ik.solve_goal_sets(model, grasps, objs, start, cfg, device=dev)
    table = ops.DeviceScenes.from_scenes(scenes, cfg.layer_kwargs(), device=dev)
    g2, r2, p2, k2, _, _ = goalset.setup_goal_sets(ops.robot_blob(model, dev), model.points_per_link, table, gs, rs, cnt, cfg,
                                                   rng=np.random.RandomState(0))
    assert torch.equal(g2, res.grasps) and torch.equal(r2, res.reach_grasps) and torch.equal(p2, res.potentials)
    sub = ops.DeviceScenes.from_scenes([scenes[0], scenes[2]], cfg.layer_kwargs(), device=dev)
    eng = ChompEngine.auto(model, sub, cfg, start[[0, 2]], r2[[0, 2], :, -1].cpu().numpy(), layout_scenes=4, for_plan=True,
                           goal_counts=k2[[0, 2]], device=dev, ol_alg="MD", reach_grasps=r2[[0, 2]].cpu().numpy())
    out = eng.plan()
    assert torch.equal(eng.traj, res.traj[[0, 2]]) and torch.equal(out, res.info[[0, 2]])
    # the goal-less scenes do not disturb the others: the two planned scenes alone, layout pinned to 4 scenes
    alone = pipeline.plan_grasps(model, [scenes[0], scenes[2]], [grasps[0], grasps[2]], start[[0, 2]], cfg, ol_alg="MD",
                                 rng=np.random.RandomState(0), device=dev, layout_scenes=4)
    assert torch.equal(alone.traj, res.traj[[0, 2]]) and np.array_equal(traj[[1, 3]], np.zeros_like(traj[[1, 3]]))
