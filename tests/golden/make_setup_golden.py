"""Generate tests/golden/setup_*.npz: the reference's own Planner.setup_goal_set (omg/planner.py:502-597) on stub Planner / env
objects, with a stub Cost whose batch_obstacle_cost returns recorded per-goal collision counts and potentials (the selection
only reads their sums), under a seeded np.random.

Runs only where the reference tree is present (never on the GPU machine):  python tests/golden/make_setup_golden.py

Each case holds several objects (the reference loops over env.objects): goal sets with clusters and pairs near the 0.5
threshold, some goals over allow_collision_point, an object with compute_grasp = False and one without grasps.  Recorded per
object o: the inputs (goals_o, reach_o, collide_o, pot_o, compute_grasp_o) and what the reference left behind (out_grasps_o,
out_reach_o, out_potentials_o, out_vis_o: the stub's visualisation rows, which are the goal indices, out_seeds_o, out_count_o).
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parents[1]))

import make_golden as mg  # noqa: E402

# name, use_standoff, filter_collision, filter_diversity, goal counts per object, "ikfail" objects (one diverse goal)
CASES = [
    ("standoff", True, True, True, (260, 90, 0), ()),
    ("nostandoff", False, True, True, (180, 40), ()),
    ("nocollision", True, False, True, (150, 70), ()),
    ("nodiversity", True, True, False, (160, 30), ()),
    ("ikfail", False, True, True, (60, 50), (0,)),
]


def make_goals(rng, n, one_diverse=False):
    if one_diverse:  # every goal within 0.5 of the first: the diversity filter leaves nothing ("IK FAIL")
        return np.tile(rng.uniform(-1, 1, 9), (n, 1)) + rng.uniform(-0.05, 0.05, (n, 9))
    centres = rng.uniform(-1.5, 1.5, (max(1, n // 6), 9))
    g = centres[rng.randint(len(centres), size=n)] + rng.normal(0, 0.25, (n, 9))
    k = n // 8  # pairs at 0.5 + a few ulp in random directions
    u = rng.normal(size=(k, 9))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    g[n - k:] = g[:k] + u * (0.5 + rng.randint(-3, 4, (k, 1)) * np.finfo(float).eps)
    return g


class StubCost:
    def __init__(self, records):
        self.records = records

    def batch_obstacle_cost(self, goal_set, special_check_id=0, uncheck_finger_collision=-1):
        import torch
        col, pot = self.records[special_check_id]
        n = len(goal_set)
        assert n == len(col) and uncheck_finger_collision == -1
        return (torch.tensor(pot, dtype=torch.float32).reshape(n, 1, 1), None, np.arange(n, dtype=np.float64).reshape(n, 1),
                torch.tensor(col, dtype=torch.float32).reshape(n, 1, 1))


def run_case(case, config, pl, seed):
    name, standoff, fc, fd, counts, fail = case
    rng = np.random.RandomState(seed)
    cfg = config.cfg
    cfg.silent = True
    data = dict(seed=seed, num_objects=len(counts), use_standoff=standoff, filter_collision=fc, filter_diversity=fd,
                allow_collision_point=cfg.allow_collision_point, goal_set_max_num=cfg.goal_set_max_num)
    objects, records = [], {}
    for o, n in enumerate(counts):
        g = make_goals(rng, n, o in fail)
        reach = (g[:, None, :] + rng.normal(0, 0.05, (n, cfg.reach_tail_length, 9))) if standoff else g.copy()
        if standoff:
            reach[:, -1] = g  # the engine's convention: the tail ends at the goal
        col = rng.choice([0, 0, 0, 1, 3, 5, 6, 9], n).astype(np.float32)
        pot = rng.uniform(0, 2, n).astype(np.float32)
        records[o] = (col, pot)
        compute = o != 1 or name != "nostandoff"  # one object of one case is left alone (compute_grasp False)
        data.update({f"goals_{o}": g, f"reach_{o}": reach, f"collide_{o}": col, f"pot_{o}": pot, f"compute_grasp_{o}": compute})
        objects.append(types.SimpleNamespace(name=f"obj_{o}", grasps=list(g), reach_grasps=list(reach), compute_grasp=compute,
                                             grasp_potentials=[], grasp_vis_points=[], seeds=[]))
    planner = object.__new__(pl.Planner)
    planner.cfg = cfg
    planner.cost = StubCost(records)
    env = types.SimpleNamespace(objects=objects)
    np.random.seed(seed)
    planner.setup_goal_set(env, filter_collision=fc, filter_diversity=fd)
    for o, ob in enumerate(objects):
        k = len(ob.grasps)
        data[f"out_count_{o}"] = k
        data[f"out_grasps_{o}"] = np.array(ob.grasps, np.float64).reshape(k, 9)
        data[f"out_reach_{o}"] = np.array(ob.reach_grasps, np.float64).reshape((k,) + data[f"reach_{o}"].shape[1:])
        data[f"out_potentials_{o}"] = np.concatenate([np.asarray(p).reshape(-1) for p in ob.grasp_potentials]) if ob.grasp_potentials else np.zeros(0, np.float32)
        data[f"out_vis_{o}"] = np.concatenate([np.asarray(v).reshape(-1) for v in ob.grasp_vis_points]) if ob.grasp_vis_points else np.zeros(0)
        data[f"out_seeds_{o}"] = np.array(ob.seeds, np.float64).reshape(-1, 9)
        data[f"out_compute_grasp_{o}"] = bool(ob.compute_grasp)
    return data


def main():
    config, _, _, _, _ = mg.load_reference()
    import importlib
    pl = importlib.import_module("omg.planner")
    for i, case in enumerate(CASES):
        data = run_case(case, config, pl, 7000 + i)
        np.savez_compressed(HERE / f"setup_{case[0]}.npz", **data)
        print(case[0], [int(data[f"out_count_{o}"]) for o in range(data["num_objects"])])


if __name__ == "__main__":
    main()
