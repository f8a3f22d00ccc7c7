"""Host edits between the calls of the planner loop, as shared test data (beside ik_cases.py / camera_cases.py).

A script is a list of (iteration, window, function(env, traj, learner, cost, cfg, rng)).  Window 0 is before that iteration's
`Learner.update_goal()`, window 1 between `update_goal()` and `Optimizer.optimize()`.  The functions touch only attributes the
reference's objects, the oracle loop's plain namespaces (tests/test_oracle_plan.py) and the drop-in classes share, so the SAME
function objects are applied to all three:

    env.objects[k].pose_mat / .reach_grasps, env.target_idx, env.sdf_torch            (indexable, `+=` in place)
    traj.data / .start / .end / .goal_set / .goal_idx, traj.interpolate_waypoints()

What needs a constructor (a re-plan: new trajectory, new Optimizer, new Learner — omg/planner.py:123-153) cannot be written
against all three at once; such a function RETURNS a `Replan` record and the driver builds the objects with its own classes
(`apply_replan` says how, with the driver's factories).

Nothing here reads `traj.goal_idx` / `traj.end` after `update_goal()`: on the drop-in classes that would resolve the promise
and change the path under test.  Goal overrides therefore use fixed indices; make_golden.py refuses a fixture in which the
override equals the learner's own pick.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

ITERATIONS = 24
ARM = np.array([1.0] * 7 + [0.0, 0.0])

# start [9], goal_set [G,9], reach_grasps [G,c,9] of the new plan; reset: keep the Learner / Optimizer objects and call
# learner.reset(traj2) + optim.reset() instead of building new ones
Replan = namedtuple("Replan", "start goal_set reach_grasps reset")


def make_rng():
    """Every driver hands the functions a generator in this state, so all three draw the same numbers."""
    return np.random.RandomState(9001)


def _target(env):
    return env.objects[env.target_idx]


# ---- goal arrays ---------------------------------------------------------------------------------------------------------
def permute_goals_in_place(env, traj, learner, cost, cfg, rng):
    perm = np.roll(np.arange(len(traj.goal_set)), 3)  # every row moves
    traj.goal_set[:] = np.array(traj.goal_set)[perm]


def replace_goals(env, traj, learner, cost, cfg, rng):
    traj.goal_set = np.array(traj.goal_set) + 0.1 * ARM * np.array([1, -1, 1, -1, 1, -1, 1, 0, 0])


def permute_tails_in_place(env, traj, learner, cost, cfg, rng):
    perm = np.roll(np.arange(len(traj.goal_set)), 3)
    reach = _target(env).reach_grasps
    reach[:] = np.array(reach)[perm]
    traj.goal_set[:] = np.array(traj.goal_set)[perm]


def replace_tails(env, traj, learner, cost, cfg, rng):
    d = 0.08 * ARM * np.array([-1, 1, 1, -1, -1, 1, 1, 0, 0])
    _target(env).reach_grasps = np.array(_target(env).reach_grasps) + d
    traj.goal_set = np.array(traj.goal_set) + d


# ---- trajectory ----------------------------------------------------------------------------------------------------------
def bump_trajectory(iteration):
    """In-place edit of traj.data over rows that contain the waypoint this iteration's update_goal() looks at
    (start_idx = min(int(t / T * n), n - 1) with t = iteration + 1; online_learner.py:109-112)."""
    def bump_trajectory_in_place(env, traj, learner, cost, cfg, rng):
        n = traj.data.shape[0]
        s = min(int(((iteration + 1) / cfg.optim_steps) * cfg.timesteps), cfg.timesteps - 1)
        lo, hi = max(s - 2, 0), min(s + 4, n)
        hat = 1.0 - np.abs(np.arange(lo, hi) - s) / 4.0
        traj.data[lo:hi] += 0.25 * hat[:, None] * ARM * np.array([1, 1, -1, 1, -1, 1, -1, 0, 0])
    return bump_trajectory_in_place


def replace_start(env, traj, learner, cost, cfg, rng):
    traj.start = np.array(traj.start) + 0.05 * ARM * np.array([1, -1, 1, 1, -1, 1, -1, 0, 0])


def reinterpolate(env, traj, learner, cost, cfg, rng):
    traj.interpolate_waypoints()  # traj.data replaced by a fresh start -> end curve


# ---- goal override (what grasp_init-style code does) ------------------------------------------------------------------------
def override_goal(k):
    def override_goal_k(env, traj, learner, cost, cfg, rng):
        traj.goal_idx = k
        traj.end = traj.goal_set[k]
    return override_goal_k


# ---- scene ---------------------------------------------------------------------------------------------------------------
def move_obstacle_in_place(env, traj, learner, cost, cfg, rng):
    env.objects[1].pose_mat[:3, 3] += [0.06, -0.05, -0.06]


def raise_volume_in_place(env, traj, learner, cost, cfg, rng):
    env.sdf_torch[2] += 0.02


# ---- re-plan -------------------------------------------------------------------------------------------------------------
def _replan(rows, reset):
    def replan(env, traj, learner, cost, cfg, rng):
        rows_ = np.array(rows)
        d = np.concatenate([rng.normal(0, 0.05, size=(len(rows_), 7)), np.zeros((len(rows_), 2))], 1)
        goals = np.array(traj.goal_set)[rows_] + d
        reach = np.array(_target(env).reach_grasps)[rows_] + d[:, None, :]
        return Replan(np.array(traj.data[4]), goals, reach, reset)
    return replan


def apply_replan(r, env, cost, learner, optim, new_traj, new_optimizer, new_learner):
    """What Planner.update does with a Replan record (omg/planner.py:123-153), with the driver's own factories:
    new_traj(start, goal_set) -> trajectory (goal 0, interpolated), new_optimizer() and new_learner(traj).  Returns
    (traj, learner, optim)."""
    env.objects[env.target_idx].reach_grasps = r.reach_grasps
    traj = new_traj(r.start, r.goal_set)
    cost.env = env
    cost.target_obj = env.objects[env.target_idx]
    if r.reset:
        learner.reset(traj)
        optim.reset()
        return traj, learner, optim
    return traj, new_learner(traj), new_optimizer()


def _both(entries):
    """[(iteration, function)] -> the script with every edit in window 0 and the one with every edit in window 1."""
    return {w: [(it, w, f) for it, f in entries] for w in (0, 1)}


# name -> dict(seed, alg, standoff, scripts={window: script})
SCRIPTS = {
    "goal_inplace": dict(seed=44, alg="MD", standoff=False, scripts=_both([(4, permute_goals_in_place), (12, replace_goals)])),
    # the edited standoff plan terminates early: both edits come before that
    "reach_inplace": dict(seed=47, alg="Exp", standoff=True, scripts=_both([(2, permute_tails_in_place), (5, replace_tails)])),
    "traj_edit": dict(seed=44, alg="MD", standoff=False,
                      scripts=_both([(5, bump_trajectory(5)), (11, replace_start), (16, reinterpolate)])),
    # cfg.optim_steps = 16: from iteration 16 on the planner calls no update_goal() (planner.py:614), so the last override rules
    # the step in window 0 as well — the earlier window-0 overrides are overwritten by update_goal() and show only in its
    # return value
    "goal_override": dict(seed=44, alg="MD", standoff=False, cfg_over=dict(optim_steps=16),
                          scripts=_both([(6, override_goal(5)), (12, override_goal(2)), (19, override_goal(7))])),
    # the raw in-place volume write lands in window 0 in both scripts: between update_goal() and optimize() the old volume no
    # longer exists for a deferred update to read (INTEGRATION.md states that deviation)
    "scene_edit": dict(seed=44, alg="MD", standoff=False,
                       scripts={w: [(2, w, move_obstacle_in_place), (9, 0, raise_volume_in_place)] for w in (0, 1)}),
    "replan": dict(seed=44, alg="MD", standoff=False, scripts=_both([(10, _replan([0, 1, 3, 4, 6, 7], False))])),
    "replan_reset": dict(seed=44, alg="MD", standoff=False, scripts=_both([(10, _replan([5, 2, 7, 0, 3, 6, 1, 4], True))])),
}
REPLAN_ITERATIONS = 22  # ten, then twelve more

CASES = [f"{name}_w{w}" for name in SCRIPTS for w in (0, 1)]


def case(name):
    """'goal_inplace_w1' -> (spec, script, iterations)."""
    base, w = name.rsplit("_w", 1)
    spec = SCRIPTS[base]
    return spec, spec["scripts"][int(w)], (REPLAN_ITERATIONS if base.startswith("replan") else ITERATIONS)


def due(script, iteration, window):
    return [f for it, w, f in script if it == iteration and w == window]


def load(name):
    """The fixture of a case with its scene's arrays (one file per scene, shared by the cases)."""
    from tests import helpers as H
    fx = H.load(f"plan_edit_{name}.npz")
    fx.update(H.load(f"plan_edit_scene_{int(fx['scene'])}.npz"))
    return fx
