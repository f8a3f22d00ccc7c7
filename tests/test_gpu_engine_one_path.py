"""ChompEngine.iterate() runs every iteration through the prepared calls (ops.IterationCalls) and takes the dispatch schedule from
one rule (ChompEngine._dispatch_rule).  What must not move: the launches an engine's life cycle makes — entry point, schedule,
work counters and stream of each, the small schedule-building launches included — and the bits they leave, which are those of the
same life cycle composed from the separate entry points (separate_launches).  One tiny engine, the shape of test_gpu_callpath.py:
2 scenes x 3 goals x 8 waypoints, ragged goal sets, MEASURE_MIN_ITEMS lowered so that its 6 items are measured."""
from __future__ import annotations

import copy

import numpy as np
import pytest

from test_gpu_pipeline import STATE, _assert_same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S, G, N = 2, 3, 8
# entry point -> (position of the schedule argument, of the work argument) from the end of the argument list; the stream is last
ENTRY_POINTS = {
    "omgx_goalset_cost_layer": (-4, -2), "omgx_goalset_cost_layer_parts": (-7, -5), "omgx_goalset_cost_layer_tiled": (None, None),
    "omgx_goalset_cost": (None, None), "omgx_fk_sdf": (None, None), "omgx_goal_update": (None, None), "omgx_chomp_optimize": (None, None),
    "omgx_goal_update_optimize": (None, None),
    # the schedule builders: work is their first argument (null: all items weigh the same)
    "omgx_goalset_schedule": (None, 0), "omgx_goalset_schedule_parts": (None, 0), "omgx_goalset_schedule_ordered": (None, 0),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def workload():
    import bench
    return bench.build_workload(S, G, N, 32, 0, False)


@pytest.fixture
def launches(monkeypatch):
    """A pass-through spy on the library's entry points, installed before any engine is built (IterationCalls takes its functions
    when it is built and reports errors under fn.__name__): a list of (entry point, schedule given, work given, stream handle)."""
    from omg_planner_amd import _lib
    from omg_planner_amd.engine import ChompEngine
    monkeypatch.setattr(ChompEngine, "MEASURE_MIN_ITEMS", 1)
    lib, log = _lib.lib(), []
    given = lambda a: a is not None and bool(getattr(a, "value", a))
    for name, (sched, work) in ENTRY_POINTS.items():
        def spy(*a, _real=getattr(lib, name), _name=name, _sched=sched, _work=work):
            log.append((_name, _sched is not None and given(a[_sched]), _work is not None and given(a[_work]), a[-1].value or 0))
            return _real(*a)
        spy.__name__ = name
        monkeypatch.setattr(lib, name, spy)
    return log


def _engine(workload, dev, layout="whole", alg="MD", **kw):
    from omg_planner_amd.engine import ChompEngine
    cfg, model, batch, start, goals = workload
    kw.update({"whole": {}, "split": dict(goal_parts=2), "latency": dict(latency_mode=True)}[layout])
    return ChompEngine(model, batch, copy.deepcopy(cfg), start, goals, device=dev, ol_alg=alg, goal_counts=np.array([3, 2]), **kw)


def _life_cycle(engines, every, dev, log=None, before_the_mask=None):
    """Bare iterate(t) for t = 0..5, then `active` assigned and three more -> the launches of each iteration."""
    per_iteration = []
    for t in range(9):
        if t == 6:
            if before_the_mask is not None:
                before_the_mask()
            for e in engines:
                e.reschedule_every = every
                e.active = torch.tensor([1, 0], dtype=torch.int32, device=dev)
        for e in engines:
            e.iterate(t)
        if log is not None:
            per_iteration.append(list(log))
            log.clear()
    return per_iteration


GS, UP, TILED = "omgx_goalset_cost_layer", "omgx_goal_update_optimize", "omgx_goalset_cost_layer_tiled"
UNIFORM, ORDERED = "omgx_goalset_schedule", "omgx_goalset_schedule_ordered"
# (entry point, schedule given, work given) per launch and iteration, as the engine made them before iterate() had one path
BATCH_LAUNCHES = {
    0: [
        [(UNIFORM, False, False), (GS, True, False), (UP, False, False)],  # t = 0: the even split is built (no work: all items weigh the same)
        [(GS, True, True), (ORDERED, False, True), (UP, False, False)],    # t = 1: the measuring launch, then the schedule from its durations
        [(GS, True, False), (UP, False, False)],
        [(GS, True, False), (UP, False, False)],
        [(GS, True, False), (UP, False, False)],
        [(GS, True, False), (UP, False, False)],
        [(GS, False, False), (UP, False, False)],                          # under a mask, reschedule_every = 0: scene-major order, no schedule
        [(GS, False, False), (UP, False, False)],
        [(GS, False, False), (UP, False, False)],
    ],
    1: [
        [(UNIFORM, False, False), (GS, True, False), (UP, False, False)],
        [(GS, True, True), (ORDERED, False, True), (UP, False, False)],
        [(GS, True, False), (UP, False, False)],
        [(GS, True, False), (UP, False, False)],
        [(GS, True, False), (UP, False, False)],
        [(GS, True, False), (UP, False, False)],
        [(ORDERED, False, True), (GS, True, False), (UP, False, False)],   # under a mask, reschedule_every = 1: rebuilt for every launch
        [(ORDERED, False, True), (GS, True, False), (UP, False, False)],
        [(ORDERED, False, True), (GS, True, False), (UP, False, False)],
    ],
}
LATENCY_LAUNCHES = [[(TILED, False, False), (UP, False, False)]] * 9  # no schedule, no work, ever


def _expected(layout, every):
    if layout == "latency":
        return LATENCY_LAUNCHES
    if layout == "whole":
        return BATCH_LAUNCHES[every]
    # split goals: the same sequence through the entry points that count (scene, goal, part) items
    names = {GS: GS + "_parts", UNIFORM: UNIFORM + "_parts"}
    return [[(names.get(n, n), s, w) for n, s, w in it] for it in BATCH_LAUNCHES[every]]


@pytest.mark.parametrize("every", [0, 1])
@pytest.mark.parametrize("layout,own_stream", [("whole", False), ("split", False), ("latency", False), ("whole", True), ("split", True)])
def test_an_engines_life_makes_the_same_launches(dev, workload, launches, layout, own_stream, every):
    side = torch.cuda.Stream(device=dev) if own_stream else None
    eng = _engine(workload, dev, layout, stream=side)
    if side is not None:
        side.wait_stream(torch.cuda.current_stream(dev))  # the engine's tensors were filled on the current stream
    launches.clear()
    got = _life_cycle([eng], every, dev, launches)
    torch.cuda.synchronize()
    assert [[rec[:3] for rec in it] for it in got] == _expected(layout, every)
    handle = side.cuda_stream if own_stream else torch.cuda.current_stream(dev).cuda_stream
    assert {rec[3] for it in got for rec in it} == {handle}  # every launch of the iteration, the schedule builds included
    with_work = [(t, rec[0]) for t, it in enumerate(got) for rec in it if rec[0].startswith("omgx_goalset_cost") and rec[2]]
    assert with_work == ([] if layout == "latency" else [(1, _expected(layout, every)[1][0][0])])  # measured once, by the second launch


def _assert_same_under_the_mask(a, b):
    """_assert_same for engines whose scene 1 is switched off and which have not been through a whole-batch operation since: the
    running scene bit for bit; the other one too, but for its layer outputs, which a masked goal-set launch leaves alone (its
    layer skips the scene) and omgx_fk_sdf, which takes no mask, keeps writing."""
    torch.cuda.synchronize()
    for k in STATE:
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert np.array_equal(x[0], y[0], equal_nan=True), k
        assert k in ("pot", "col") or np.array_equal(x[1], y[1], equal_nan=True), k
    assert np.array_equal(a.active.cpu().numpy(), b.active.cpu().numpy())


@pytest.mark.parametrize("layout,alg", [("whole", "MD"), ("split", "MD"), ("latency", "MD"), ("whole", "Proj"), ("split", "Proj"), ("latency", "Proj")])
def test_one_path_leaves_the_bits_of_the_separate_entry_points(dev, workload, launches, layout, alg):
    """The life cycle above and whole plans against an identically built engine with separate_launches = True ("Proj" never selects
    a goal: the fixed-goal iteration alone)."""
    def pair():
        eng, ref = _engine(workload, dev, layout, alg), _engine(workload, dev, layout, alg)
        ref.separate_launches = True
        return eng, ref

    for every in (0, 1):
        eng, ref = pair()
        # _assert_same on the whole STATE up to the mask; after it the one exemption _assert_same_under_the_mask names (the layer
        # outputs of the switched-off scene, which the two compositions never wrote alike) — the whole plans below are compared in full
        _life_cycle([eng, ref], every, dev, before_the_mask=lambda: _assert_same(eng, ref))
        assert (eng.t, eng.step_count, eng._parts_last) == (ref.t, ref.step_count, ref._parts_last)
        _assert_same_under_the_mask(eng, ref)
    for early in (True, False):
        eng, ref = pair()
        a, b = eng.plan(early_stop=early), ref.plan(early_stop=early)
        assert torch.equal(a, b) and eng.iterations_run == ref.iterations_run
        _assert_same(eng, ref)
    assert ("omgx_goal_update" in {rec[0] for rec in launches}) == (alg == "MD")  # the learner's own launch: the separate composition ran


def test_a_failed_persistent_launch_is_seen_by_the_next_iteration(dev, workload, launches, monkeypatch):
    """A persistent launch reports a failure inside it through its control block only, and join() is what looks there: the
    iteration after it raises before it launches anything.  (No failing launch is run: the status is a stand-in.)"""
    from omg_planner_amd import _lib
    eng = _engine(workload, dev)
    for t in range(3):  # into the steady state: schedule measured, calls prepared
        eng.iterate(t)
    torch.cuda.synchronize()
    monkeypatch.setattr(eng, "persistent_status", lambda: {"failure": 2})
    eng._persist_unchecked = True
    launches.clear()
    with pytest.raises(_lib.OmgHipError):
        eng.iterate(3)
    assert launches == []
