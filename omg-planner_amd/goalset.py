"""Planner.setup_goal_set (omg/planner.py:502-597): prune a target's goal set before planning.

Device part: the collision filter's `Cost.batch_obstacle_cost(goal_set, special_check_id=i,
uncheck_finger_collision=-1)` for S scenes at once = one `omgx_fk_sdf(soften_fingers=1)` over [S, G0] goal configurations,
reduced per goal.  The thresholding and the greedy diversity filter run on the device as well (`setup_goal_sets`,
`ops.select_goals`: omgx_select_goals); only the sampling stays on the host, so that the same `np.random`
stream picks the same goals.  `select_goals` is the host restatement of one target, with the reference's indexing quirks;
`setup_goal_set` is the drop-in with the reference's signature.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


def goal_collision_stats(robot, P: int, scenes: "ops.DeviceScenes", goal_sets: torch.Tensor):
    """goal_sets [S,G0,9] float64 (device) -> (collide [S,G0], potentials [S,G0]) float32: per-goal number of colliding
    (link, point, object) lookups and summed potentials with the finger links softened (x0.1, collisions ignored,
    cost.py:350-353), as planner.py:512-524 reduces them."""
    pot, _, col = ops.fk_sdf(robot, P, scenes, goal_sets, soften_fingers=True)
    return col.sum(dim=(-2, -1)), pot.sum(dim=(-2, -1))


def select_goals(goal_set, reach_goal_set, collide, potentials, allow_collision_point: int = 5, goal_set_max_num: int = 100,
                 filter_collision: bool = True, filter_diversity: bool = True, rng=np.random):
    """The host logic of planner.py:526-575 for ONE target object.  Returns (grasps, reach_grasps, potentials, chosen)
    where `chosen` indexes the collision-filtered list — or ([], [], [], []) when nothing survives ("IK FAIL").

    Quirks kept on purpose (they decide which goals the reference ends up with):
      * the diversity filter walks goal_set[1:] but records the loop counter j, i.e. the index of the PREVIOUS element;
        goal 0 seeds `unique_grasps` yet only enters `indexes` through that off-by-one (planner.py:548-558);
      * a candidate closer than 0.5 (joint-space L2) to any kept goal is dropped;
      * `np.random.choice(indexes, min(num, goal_set_max_num), replace=False)` draws from the global numpy stream."""
    goal_set = [np.asarray(g) for g in goal_set]
    reach_goal_set = list(reach_goal_set) if reach_goal_set is not None else []
    collide = np.asarray(collide)
    potentials = np.asarray(potentials)
    if filter_collision:
        free = (collide <= allow_collision_point).nonzero()[0]
        goal_set = [goal_set[i] for i in free]
        try:
            reach_goal_set = [reach_goal_set[i] for i in free]
        except Exception:  # noqa: BLE001  (planner.py:533-536: a short reach list is silently kept as it is)
            pass
        potentials = potentials[free]
    num = len(goal_set)
    indexes = list(range(num))
    if filter_diversity and num > 0:
        unique = [goal_set[0]]
        indexes = []
        for j, joint in enumerate(goal_set[1:]):
            if np.amin(np.linalg.norm(np.array(unique) - joint, axis=-1)) < 0.5:
                continue
            unique.append(joint)
            indexes.append(j)  # sic: j, not j + 1
        num = len(indexes)
    if num == 0:
        return [], [], [], []
    chosen = rng.choice(indexes, min(num, goal_set_max_num), replace=False)
    grasps = [goal_set[int(i)] for i in chosen]
    reach = np.array([reach_goal_set[int(i)] for i in chosen]) if reach_goal_set else np.zeros((0,))
    return grasps, reach, potentials[chosen], chosen


def draw_positions(num_candidates, goal_set_max_num: int, rng=np.random):
    """The sampling of planner.py:562-565 for S scenes in order: scene s with num_candidates[s] > 0 draws
    rng.choice(num, min(num, goal_set_max_num), replace=False) — the positions in its candidate list that the reference's
    rng.choice(indexes, ...) picks, consuming the stream as a loop of the reference's planners over the scenes does; scenes
    without candidates draw nothing.  Returns (positions [S, K] int64 padded with 0, counts [S] int64), K = max(counts)."""
    num = np.asarray(num_candidates, np.int64).reshape(-1)
    k = np.minimum(num, int(goal_set_max_num)).clip(min=0)
    pos = np.zeros((num.size, int(k.max()) if num.size else 0), np.int64)
    for s in range(num.size):
        if num[s] > 0:
            pos[s, :k[s]] = rng.choice(int(num[s]), int(k[s]), replace=False)
    return pos, k


def setup_goal_sets(robot, P: int, scenes: "ops.DeviceScenes", goal_set: torch.Tensor, reach_grasps: torch.Tensor, goal_counts, cfg,
                    rng=np.random, filter_collision: bool = True, filter_diversity: bool = True):
    """Planner.setup_goal_set (planner.py:502-597) for the targets of S scenes at once, from what goal_ik.solve_goal_sets returns:
    goal_set [S,G,9] f64, reach_grasps [S,G,T,9] f64 (device), goal_counts [S] (device tensor or host integers).

    goal_collision_stats -> ops.select_goals (omgx_select_goals: threshold, diversity filter) -> ONE download of the candidate
    counts (the stage's only host sync: the draw needs them) -> draw_positions on `rng` -> gather on the device, in the draw's
    order.  cfg: allow_collision_point, goal_set_max_num.
    Returns (goal_set [S,K,9] f64, reach_grasps [S,K,T,9] f64, potentials [S,K] f32, counts [S] int64, num_free [S],
    num_candidates [S]) — device tensors padded with zeros beyond counts[s], host arrays for the three counts."""
    S, G = int(goal_set.shape[0]), int(goal_set.shape[1])
    dev = goal_set.device
    if G:
        col, pot = goal_collision_stats(robot, P, scenes, goal_set)
    else:
        col = pot = torch.zeros((S, 0), dtype=torch.float32, device=dev)
    cand, num, free = ops.select_goals(goal_set, goal_counts, col if filter_collision else None, cfg.allow_collision_point,
                                       filter_diversity)
    host = torch.stack((num, free)).cpu().numpy().astype(np.int64)
    num_h, free_h = host[0], host[1]
    if (num_h < 0).any():
        raise ValueError(f"goal_counts must lie in [0, {G}]")
    pos, k = draw_positions(num_h, cfg.goal_set_max_num, rng)
    K = pos.shape[1]
    valid = torch.from_numpy(np.arange(K)[None, :] < k[:, None]).to(dev)
    rows = torch.gather(cand, 1, torch.from_numpy(pos).to(dev)).long()
    rows = torch.where(valid, rows, torch.zeros_like(rows))  # padding: row 0, then zeroed
    sidx = torch.arange(S, device=dev)[:, None]
    gs = torch.where(valid[..., None], goal_set[sidx, rows], 0.0)
    rs = torch.where(valid[..., None, None], reach_grasps[sidx, rows], 0.0)
    pt = torch.where(valid, pot[sidx, rows], 0.0)
    return gs, rs, pt, k, free_h, num_h


def _take_vis(vis, rows):
    from .cost import LazyArray
    if isinstance(vis, LazyArray):  # stays lazy, as Cost.batch_obstacle_cost made it
        return LazyArray((len(rows),) + tuple(vis.shape[1:]), lambda v=vis, r=rows: np.asarray(v)[r])
    return np.asarray(vis)[rows] if vis is not None else None


def setup_goal_set(planner, env, filter_collision=True, filter_diversity=True):
    """Planner.setup_goal_set (planner.py:502-597) with the selection on the device and the draw from np.random; same signature,
    same effects on env.objects: for every object with grasps and compute_grasp, `grasps` (list), `reach_grasps` (array),
    `grasp_potentials` / `grasp_vis_points` (appended), `seeds` (extended); on "IK FAIL" those four emptied; compute_grasp =
    False for every object.  The collision statistics come from planner.cost.batch_obstacle_cost(goal_set, special_check_id=i,
    uncheck_finger_collision=-1) (this package's Cost: the device; the visualisation points stay lazy).  A reach list must be
    as long as its goal list (as solve_and_process_ik leaves it)."""
    from .goal_ik import _device_for
    cfg = planner.cfg
    dev = torch.device(_device_for(planner))
    for i, target_obj in enumerate(env.objects):
        goal_set = target_obj.grasps
        reach_goal_set = target_obj.reach_grasps
        if len(goal_set) > 0 and target_obj.compute_grasp:
            potentials, _, vis_points, collide = planner.cost.batch_obstacle_cost(goal_set, special_check_id=i,
                                                                                   uncheck_finger_collision=-1)
            n = len(goal_set)
            collide = torch.as_tensor(collide).sum(-1).sum(-1)
            potentials = torch.as_tensor(potentials).sum(dim=(-2, -1)).detach().cpu().numpy()
            goals = torch.as_tensor(np.asarray(goal_set, np.float64).reshape(1, n, 9), device=dev).contiguous()
            col = collide.to(device=dev, dtype=torch.float32).reshape(1, n).contiguous() if filter_collision else None
            cand, num, _ = ops.select_goals(goals, [n], col, cfg.allow_collision_point, filter_diversity)
            num = int(num.cpu()[0])
            if num > 0:
                rows = cand[0, :num].cpu().numpy().astype(np.int64)
                pick = rows[np.random.choice(num, min(num, cfg.goal_set_max_num), replace=False)]
                target_obj.grasps = [goal_set[int(r)] for r in pick]
                target_obj.reach_grasps = np.array([reach_goal_set[int(r)] for r in pick])
                target_obj.seeds += target_obj.grasps
                target_obj.grasp_potentials.append(potentials[pick])
                target_obj.grasp_vis_points.append(_take_vis(vis_points, pick))
                if not getattr(cfg, "silent", False):
                    print("{} IK FOUND collision-free goal num {}/{}/{}/{}".format(
                        env.objects[i].name, len(target_obj.reach_grasps), len(target_obj.grasps), num, n))
            else:
                print("{} IK FAIL".format(env.objects[i].name))
                target_obj.grasps = []
                target_obj.reach_grasps = []
                target_obj.grasp_potentials = []
                target_obj.grasp_vis_points = []
        target_obj.compute_grasp = False
