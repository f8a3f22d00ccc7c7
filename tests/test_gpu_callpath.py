"""The goal-set and iteration call path of ops.py: the prepared calls (ops.IterationCalls) and the one-shot wrappers build their
argument lists from the same code, so they must write the same bits through every entry point — and every wrapper must reject
what its siblings reject, before anything is launched.  One tiny engine: 2 scenes x 3 goals x 8 waypoints (the smallest shape
where the part count of a split goal changes inside a plan: goalset_parts(8, 2) = 2, goalset_parts(3, 2) = 1)."""
from __future__ import annotations

import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S, G, N = 2, 3, 8
TILING = (4, 10, 16, 1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(dev):
    import bench
    from omg_planner_amd.engine import ChompEngine
    cfg, model, batch, start, goals = bench.build_workload(S, G, N, 32, 0, False)
    return ChompEngine(model, batch, copy.deepcopy(cfg), start, goals, device=dev, ol_alg="MD", goal_counts=np.array([3, 2]))


def _iteration_kwargs(e):
    """IterationCalls' arguments on the engine's own tensors."""
    return dict(robot=e.robot, P=e.P, scenes=e.scenes, goals=e.cv_goals, dt=e.cfg.time_interval, traj=e.traj, layer_out=(e.pot, e.pgrad, e.col),
                goal_out=(e.goal_cost, e.goal_col), goal_set=e.goal_set, reach=e.reach, state=e.learner_state, goal_idx=e.goal_idx, start=e.start,
                end=e.end, goal_rows=e.goal_rows, goal_point=e.goal_point, step_out=(e.grad, e.cost_traj, e.info), cost_vector=e.cost_vec,
                active=e._active, goal_count=e.goal_count, eta=e.eta_s, scene_flags=e._scene_flags)


def _outputs(e, parts):
    """Fresh outputs of a goal-set launch with the layer, filled with a value no launch writes (a masked scene keeps it)."""
    f32 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=e.traj.device)
    return dict(goal=(f32(S, G * parts), f32(S, G * parts)), layer=(f32(S, N, 10, e.P), f32(S, N, 10, e.P, 3), f32(S, N, 10, e.P)),
                poses=torch.full((S, N, 10, 12), -7.0, dtype=torch.float64, device=e.traj.device))


@pytest.mark.parametrize("route", ["whole", "parts", "tiled"])
@pytest.mark.parametrize("mode", ["masked", "prepass"])
def test_prepared_and_one_shot_calls_write_the_same_bits(eng, route, mode):
    """IterationCalls.goalset_layer against goalset_cost_layer / goalset_cost_layer_tiled on the same inputs, through
    omgx_goalset_cost_layer (whole goals), omgx_goalset_cost_layer_parts (goal_parts = 2, and whole goals with the poses) and
    omgx_goalset_cost_layer_tiled: goal cost, collides, the three layer outputs and the poses, at a window of 8 (two parts) and of 3 (one)."""
    from omg_planner_amd import ops
    e = eng
    masked, prepass = mode == "masked", mode == "prepass"
    active = torch.tensor([1, 0], dtype=torch.int32, device=e.traj.device)
    parts = {"whole": 1, "parts": 2, "tiled": TILING[0]}[route]
    stream = torch.cuda.current_stream(e.traj.device).cuda_stream
    for start_idx in (0, 5):
        for poses in (False, True):
            a, b = _outputs(e, parts), _outputs(e, parts)
            calls = ops.IterationCalls(**dict(_iteration_kwargs(e), layer_out=a["layer"], goal_out=a["goal"], layer_poses=a["poses"], active=active,
                                              tiling=TILING if route == "tiled" else None, goal_parts=parts if route == "parts" else 1,
                                              prepass=prepass))
            calls.use_layer_poses = poses
            calls.goalset_layer(start_idx, masked, None, None, stream)
            common = dict(active=active if masked else None, goal_count=e.goal_count, layer_poses=b["poses"] if poses else None, prepass=prepass)
            head = (e.robot, e.P, e.scenes, e.traj[:, start_idx], e.cv_goals, N - start_idx, e.cfg.time_interval, e.traj, b["layer"])
            if route == "tiled":
                ops.goalset_cost_layer_tiled(*head, b["goal"], goal_parts=TILING[0], layer_link_groups=TILING[1], layer_config_block=TILING[2],
                                             spread=bool(TILING[3]), **common)
            else:
                ops.goalset_cost_layer(*head, out=b["goal"], goal_parts=parts, **common)
            torch.cuda.synchronize()
            what = (route, mode, start_idx, poses)
            for x, y in zip(a["goal"] + a["layer"], b["goal"] + b["layer"]):
                assert torch.equal(x, y), what
            assert torch.equal(a["poses"], b["poses"]), what
            assert bool((a["goal"][0][0] != -7.0).any()) and bool((a["layer"][0][0] != -7.0).all()), what  # the launches did write
            if masked:
                assert bool((a["goal"][0][1] == -7.0).all()) and bool((a["layer"][0][1] == -7.0).all()), what  # and skipped the inactive scene
            assert bool((a["poses"][0] != -7.0).all()) == poses, what


# ---- every wrapper rejects what its siblings reject ---------------------------------------------
LAUNCHES = ("omgx_goalset_cost", "omgx_goalset_cost_layer", "omgx_goalset_cost_layer_parts", "omgx_goalset_cost_layer_tiled",
            "omgx_goal_update_optimize", "omgx_plan_persistent")


def _bad_rows(e):
    """name -> {wrapper: the arguments to replace}.  A wrapper is listed under every row whose argument it takes."""
    dev = e.traj.device
    short = lambda t: t[:, :-1].contiguous()  # one row of waypoints short
    lay = (e.pot, e.pgrad, e.col)
    ts = e.traj[:, 0]
    gs = ("goalset_cost", "goalset_cost_layer", "goalset_cost_layer_tiled")
    wide = torch.zeros((S, 18), dtype=torch.float64, device=dev)
    small = torch.zeros(S * G * 2 - 1, dtype=torch.float32, device=dev)  # one element short of S * G * 2 parts
    tiny = torch.zeros(S * G - 1, dtype=torch.float32, device=dev)       # ... of S * G whole goals
    poses_short = e.wp_pose[:, :-1].contiguous()
    return {
        "traj_start non-unit inner stride": {w: dict(traj_start=wide[:, ::2]) for w in gs},
        "traj_start float32": {w: dict(traj_start=ts.float()) for w in gs},
        "traj_start on the host": {w: dict(traj_start=ts.cpu()) for w in gs},
        "a layer output one row short": {**{w: dict(layer_out=(short(e.pot), e.pgrad, e.col)) for w in ("goalset_cost_layer", "goalset_cost_layer_tiled",
                                                                                                    "IterationCalls", "plan_persistent")},
                                         "goal_update_optimize": dict(pot=short(e.pot))},
        "layer_poses of the wrong size": {w: dict(layer_poses=poses_short) for w in ("goalset_cost_layer", "goalset_cost_layer_tiled", "IterationCalls",
                                                                                     "plan_persistent")},
        "layer_poses without a trajectory": {"goalset_cost_layer_tiled": dict(traj=None, layer_out=None, layer_poses=e.wp_pose)},
        "goal outputs too small for the parts": {"goalset_cost": dict(out=(tiny, tiny)),
                                                 "goalset_cost_layer": dict(out=(small, small), goal_parts=2),
                                                 "goalset_cost_layer_tiled": dict(out=(small, small), goal_parts=2),
                                                 "IterationCalls": dict(goal_out=(small, small), goal_parts=2),
                                                 "plan_persistent": dict(goal_out=(tiny, tiny))},
        "goal_idx int64": {w: dict(goal_idx=e.goal_idx.long()) for w in ("IterationCalls", "goal_update_optimize", "plan_persistent")},
        "active one element short": {w: dict(active=e._active[:-1]) for w in gs + ("IterationCalls", "goal_update_optimize", "plan_persistent")},
        "eta float32": {w: dict(eta=e.eta_s.float()) for w in ("IterationCalls", "goal_update_optimize", "plan_persistent")},
        "scene_flags too short": {w: dict(scene_flags=e._scene_flags[:-1]) for w in ("IterationCalls", "goal_update_optimize")},
    }


def test_every_wrapper_rejects_what_its_siblings_reject(eng, monkeypatch):
    """One table of bad arguments, each row applied to every wrapper that takes the argument: OmgHipError, and no entry point
    that launches is reached (they are replaced by counters here, so an accepted bad call would not run either)."""
    from omg_planner_amd import _lib, ops
    e = eng
    lay = (e.pot, e.pgrad, e.col)
    gs_head = dict(robot=e.robot, P=e.P, scenes=e.scenes, traj_start=e.traj[:, 0], goals=e.cv_goals, n_remaining=N, dt=e.cfg.time_interval)
    iters = (_lib.PlanIter * 1)()
    good = {
        "goalset_cost": dict(gs_head, out=(e.goal_cost, e.goal_col), active=e._active),
        "goalset_cost_layer": dict(gs_head, traj=e.traj, layer_out=lay, out=(e.goal_cost, e.goal_col), active=e._active, layer_poses=e.wp_pose),
        "goalset_cost_layer_tiled": dict(gs_head, traj=e.traj, layer_out=lay, out=(e.goal_cost, e.goal_col), active=e._active, goal_parts=1,
                                         layer_poses=e.wp_pose),
        "IterationCalls": dict(_iteration_kwargs(e), layer_poses=e.wp_pose),
        "goal_update_optimize": dict(lparams=e._learner_params(), goal_set=e.goal_set, reach=e.reach, goal_cost=e.goal_cost, state=e.learner_state,
                                     goal_idx=e.goal_idx, robot=e.robot, params=e._params(True), traj=e.traj, start=e.start, end=e.end,
                                     goal=e.goal_rows, goal_point=e.goal_point, pot=e.pot, pgrad=e.pgrad, col=e.col, active=e._active,
                                     out=(e.grad, e.cost_traj, e.info), cost_vector=e.cost_vec, scene_flags=e._scene_flags,
                                     goal_count=e.goal_count, eta=e.eta_s),
        "plan_persistent": dict(robot=e.robot, P=e.P, scenes=e.scenes, goals=e.cv_goals, dt=e.cfg.time_interval, traj=e.traj, layer_out=lay,
                                layer_poses=e.wp_pose, goal_out=(e.goal_cost, e.goal_col), lparams=e._learner_params(), goal_set=e.goal_set,
                                reach=e.reach, state=e.learner_state, goal_idx=e.goal_idx, cost_vector=e.cost_vec, params=e._params(True),
                                start=e.start, end=e.end, goal_rows=e.goal_rows, goal_point=e.goal_point, step_out=(e.grad, e.cost_traj, e.info),
                                iters=iters, d_iters=torch.zeros(len(bytes(iters)), dtype=torch.uint8, device=e.traj.device),
                                workspace=torch.zeros(int(_lib.lib().omgx_plan_persistent_workspace_bytes(S, N)), dtype=torch.uint8,
                                                      device=e.traj.device),
                                active=e._active, goal_count=e.goal_count, eta=e.eta_s),
    }
    launched = []
    for name in LAUNCHES:  # (IterationCalls takes its entry points from the library object when it is built)
        monkeypatch.setattr(_lib.lib(), name, lambda *a, _n=name: launched.append(_n) or _lib.OMGX_OK)
    for w, kwargs in good.items():  # the table's starting points are calls the wrappers accept
        n0 = len(launched)
        getattr(ops, w)(**kwargs)
        assert len(launched) == n0 + (w != "IterationCalls"), w
    launched.clear()
    accepted = []
    for row, wrappers in _bad_rows(e).items():
        for w, over in wrappers.items():
            try:
                getattr(ops, w)(**dict(good[w], **over))
                accepted.append((row, w))
            except _lib.OmgHipError:
                pass
    assert not accepted and not launched, (accepted, launched)
