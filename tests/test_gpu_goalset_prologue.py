"""The goal workgroup's PROLOGUE of the batch kernel — (sin, cos) stage, joint matrices, chain, row culling beside or behind the chain,
tile list — at the shapes where it takes another path: windows of 1, 2, 21 | 22 (the chain goes from one wave to two), 30, 32 | 33
(culling beside the chain ends, second layout of the tile bits), 0 / 1 / 5 objects per scene, 1 / 15 collision points per link,
ragged goal sets.  The prologue reads its wave-uniform inputs through scalar copies of its own and takes the interpolation step
1 / (n + 1) from the host; none of that may change a bit.

What has to hold for every case: goal costs, collision counts and the trajectory layer's outputs of the batch launch are BIT-equal to
the latency-mode launch with one part per goal (another instantiation of the kernel with its own prologue: chain constants and joint
matrices in LDS, every wave culling the rows of its own tiles), and the costs stay within the oracle's 1e-5 relative bar.  One case
goes through the engine's three pipeline parts, their measuring launches and the scheduled launches after them."""
from __future__ import annotations

import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S, G, N = 2, 3, 33          # scenes, goals (padded), waypoints of the plan: the longest window is the whole plan
COUNTS = np.array([3, 1, 2])  # ragged goal sets (the third count: the extra scene of the batches without objects, see _scenes)
WINDOWS = [1, 2, 21, 22, 30, 32, 33]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _scenes(objects: int, count: int = S):
    """`objects` records per scene: none at all, the table alone, or four shapes and the table.  The library refuses a batch whose object
    table is empty altogether (a null pointer), so the scenes without objects are followed by one more scene that holds the table."""
    from omg_planner_amd import scenes as sc
    if objects == 0:
        return [sc.Scene([], target_idx=0) for _ in range(count)] + [sc.make_tabletop_scene(count, num_objects=0, grid=24, table_grid=(48, 32, 16))]
    return [sc.make_tabletop_scene(s, num_objects=objects - 1, grid=24, table_grid=(48, 32, 16)) for s in range(count)]


_WORKLOADS: dict = {}


def _workload(dev, objects: int, P: int):
    """(model, host batch, robot blob, device scenes, trajectories [S,N,9], goals [S,G,9], goal counts, dt), built once per (objects, P)."""
    key = (objects, P)
    if key not in _WORKLOADS:
        from omg_planner_amd import ops, robot as rb, scenes as sc
        from omg_planner_amd.config import Config
        cfg = Config(timesteps=N, use_standoff=False)
        model = rb.PandaModel(points_per_link=P, seed=0)
        batch = sc.pack_table(_scenes(objects), cfg.layer_kwargs())
        ns = batch.num_scenes
        assert list(np.diff(batch.scene_begin)[:S]) == [objects] * S
        start = np.tile(rb.HOME_CONFIG, (ns, 1))
        goals = np.stack([sc.make_goal_set(s, G) for s in range(ns)])
        traj = np.stack([sc.cubic_init(start[s], goals[s, 0], N) for s in range(ns)])
        _WORKLOADS[key] = dict(model=model, batch=batch, robot=ops.robot_blob(model, dev), scenes=ops.DeviceScenes(batch, dev),
                               traj=torch.from_numpy(np.ascontiguousarray(traj, np.float64)).to(dev),
                               goals=torch.from_numpy(np.ascontiguousarray(goals, np.float64)).to(dev),
                               count=torch.as_tensor(COUNTS[:ns], dtype=torch.int32, device=dev), dt=cfg.time_interval, ns=ns)
    return _WORKLOADS[key]


def _layer_buffers(dev, ns, P):
    f32 = dict(dtype=torch.float32, device=dev)
    return (torch.full((ns, N, 10, P), float("nan"), **f32), torch.full((ns, N, 10, P, 3), float("nan"), **f32), torch.full((ns, N, 10, P), float("nan"), **f32))


@pytest.mark.parametrize("n_rem", WINDOWS)
@pytest.mark.parametrize("P", [1, 15])
@pytest.mark.parametrize("objects", [0, 1, 5])
def test_batch_prologue_equals_the_latency_mode_prologue_bit_for_bit(dev, objects, P, n_rem):
    from omg_planner_amd import ops
    from oracle import oracle as orc
    w = _workload(dev, objects, P)
    ts, ns = w["traj"][:, N - n_rem], w["ns"]
    nan = lambda: torch.full((ns, G), float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
    cost, col, lay = nan(), nan(), _layer_buffers(dev, ns, P)
    ops.goalset_cost_layer(w["robot"], P, w["scenes"], ts, w["goals"], n_rem, w["dt"], w["traj"], lay, out=(cost, col), goal_count=w["count"])
    lcost, lcol, llay = nan(), nan(), _layer_buffers(dev, ns, P)
    parts = ops.goalset_cost_layer_tiled(w["robot"], P, w["scenes"], ts, w["goals"], n_rem, w["dt"], w["traj"], llay, (lcost, lcol),
                                         goal_count=w["count"], goal_parts=1, spread=True)
    torch.cuda.synchronize()
    assert parts == 1
    c, k, lc, lk = (t.cpu().numpy() for t in (cost, col, lcost, lcol))
    for s in range(ns):
        n = COUNTS[s]
        assert np.array_equal(c[s, :n].view(np.uint32), lc[s, :n].view(np.uint32)), (s, c[s, :n], lc[s, :n])
        assert np.array_equal(k[s, :n].view(np.uint32), lk[s, :n].view(np.uint32)), (s, k[s, :n], lk[s, :n])
        assert np.isnan(c[s, n:]).all() and np.isnan(k[s, n:]).all()  # the padding of a ragged goal set is never written
        assert np.isfinite(c[s, :n]).all() and np.isfinite(k[s, :n]).all()
        gc, _ = orc.goalset_cost(w["model"].blob(), P, w["batch"].subset(s, s + 1), ts[s:s + 1].cpu().numpy(), w["goals"][s:s + 1, :n].cpu().numpy(),
                                 n_rem, w["dt"])
        np.testing.assert_allclose(c[s, :n], np.asarray(gc).reshape(-1), rtol=1e-5, atol=1e-6)
    for a, b in zip(lay, llay):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert not np.isnan(a).any()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if objects == 0:
        assert not c[0, :COUNTS[0]].any() and not k[0, :COUNTS[0]].any()
    if objects == 5 and P == 15 and n_rem >= 21:
        assert (c[0, :COUNTS[0]] > 0).all()  # the case has teeth: pairs survive the culling and reach the exact path


def test_pipeline_parts_measured_and_scheduled_launches_keep_the_bits(dev, monkeypatch):
    """Five objects, 15 points, 30 waypoints through the ENGINE: three pipeline parts against one stream — the second launch measures
    (STAMP instantiation; a batch this small measures only with the threshold lowered), the later ones run the schedule built from
    it — and the first launch's costs against the latency-mode launch on the same inputs."""
    from omg_planner_amd import ops, robot as rb, scenes as sc
    from omg_planner_amd.config import Config
    from omg_planner_amd.engine import ChompEngine
    monkeypatch.setattr(ChompEngine, "MEASURE_MIN_ITEMS", 1)
    n, Se, Ge = 30, 6, 3
    counts = np.array([3, 1, 2, 3, 1, 3])
    cfg = Config(timesteps=n, use_standoff=False)
    model = rb.PandaModel(points_per_link=15, seed=0)
    batch = sc.pack_table(_scenes(5, Se), cfg.layer_kwargs())
    start = np.tile(rb.HOME_CONFIG, (Se, 1))
    goals = np.stack([sc.make_goal_set(s, Ge) for s in range(Se)])
    out = []
    for pipe in (3, 1):
        e = ChompEngine(model, batch, copy.deepcopy(cfg), start, goals, device=dev, ol_alg="MD", goal_counts=counts)
        e.pipeline = pipe
        if pipe == 3:  # the first launch's inputs through the latency-mode kernel, one part per goal
            lc = torch.full((Se, Ge), float("nan"), dtype=torch.float32, device=dev)
            ll = torch.full_like(lc, float("nan"))
            ops.goalset_cost_layer_tiled(e.robot, e.P, e.scenes, e.traj[:, 0], e.cv_goals, n, cfg.time_interval, None, None, (lc, ll),
                                         goal_count=e.goal_count, goal_parts=1, spread=True)
        snaps = []
        for t in (0, 1, 2, 3):
            e.iterate(t)
            e.join()
            torch.cuda.synchronize()
            snaps.append({k: getattr(e, k).cpu().numpy().copy() for k in ("goal_cost", "goal_col", "goal_idx", "traj", "pot", "col")})
        runners = e._parts if pipe > 1 else [e]  # a pipeline part is an engine of its own over a range of the scenes, with its own schedule
        assert len(runners) == pipe
        for r in runners:
            assert r._measured and r.schedule is not None  # its last launches ran the schedule built from the measured durations
        out.append(snaps)
    for a, b in zip(*out):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    first, lc, ll = out[0][0], lc.cpu().numpy(), ll.cpu().numpy()
    for s in range(Se):
        m = counts[s]
        assert np.array_equal(first["goal_cost"].reshape(Se, -1)[s, :m].view(np.uint32), lc[s, :m].view(np.uint32))
        assert np.array_equal(first["goal_col"].reshape(Se, -1)[s, :m].view(np.uint32), ll[s, :m].view(np.uint32))
