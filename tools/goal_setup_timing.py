"""Timing of the goal pipeline from grasp poses to plans on one GPU, stage by stage (each closed by a device sync).

  python tools/goal_setup_timing.py [--scenes 100] [--grasps 200] [--reps 3] [--out profiles/goal_setup_timing.json]

Workload: goal_ik_timing.workload (S scenes x G grasps near each object) on make_tabletop_scene tables whose target object is
moved to the workload's object pose.  Stages: IK (solve_goal_sets), scene table (DeviceScenes.from_scenes), collision statistics
(goal_collision_stats), selection kernel (ops.select_goals), download + draw + gather (the rest of setup_goal_sets), engine
set-up (ChompEngine.auto), plan.  Also: the same batch through a per-scene goalset.select_goals loop on this host's CPU
(the reference's loop), and the whole pipeline.plan_grasps call.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from goal_ik_timing import workload  # noqa: E402
from omg_planner_amd import goal_ik, goalset, ops, pipeline  # noqa: E402
from omg_planner_amd import robot as rb  # noqa: E402
from omg_planner_amd import scenes as sc  # noqa: E402
from omg_planner_amd.config import Config  # noqa: E402
from omg_planner_amd.engine import ChompEngine  # noqa: E402


def timed(f, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize(dev)
    return out, (time.perf_counter() - t0) * 1e3


def one_pass(model, scenes, grasps, objs, starts, cfg, dev, seed):
    ms = {}
    robot = ops.robot_blob(model, dev)
    P = model.points_per_link
    (gs, rs, counts, _), ms["ik"] = timed(lambda: goal_ik.solve_goal_sets(model, grasps, objs, starts, cfg, device=dev), dev)
    table, ms["scene_table"] = timed(lambda: ops.DeviceScenes.from_scenes(scenes, cfg.layer_kwargs(), device=dev), dev)
    (col, pot), ms["collision_stats"] = timed(lambda: goalset.goal_collision_stats(robot, P, table, gs), dev)
    (cand, num, free), ms["select_kernel"] = timed(lambda: ops.select_goals(gs, counts, col, cfg.allow_collision_point, True), dev)

    def rest():
        rng = np.random.RandomState(seed)
        host = torch.stack((num, free)).cpu().numpy().astype(np.int64)
        pos, k = goalset.draw_positions(host[0], cfg.goal_set_max_num, rng)
        valid = torch.from_numpy(np.arange(pos.shape[1])[None, :] < k[:, None]).to(dev)
        rows = torch.where(valid, torch.gather(cand, 1, torch.from_numpy(pos).to(dev)).long(), 0)
        sidx = torch.arange(gs.shape[0], device=dev)[:, None]
        return (torch.where(valid[..., None], gs[sidx, rows], 0.0), torch.where(valid[..., None, None], rs[sidx, rows], 0.0),
                torch.where(valid, pot[sidx, rows], 0.0), k, host)
    (g2, r2, p2, k, host), ms["download_draw_gather"] = timed(rest, dev)
    ms["selection_stage"] = ms["select_kernel"] + ms["download_draw_gather"]
    idx = np.flatnonzero(k > 0)  # scenes without goals are not planned (pipeline.plan_grasps)

    def setup():
        sub = table if idx.size == len(scenes) else ops.DeviceScenes.from_scenes([scenes[i] for i in idx], cfg.layer_kwargs(), device=dev)
        return ChompEngine.auto(model, sub, cfg, starts[idx], r2[idx, :, -1].cpu().numpy(), layout_scenes=len(scenes), for_plan=True,
                                goal_counts=k[idx], reach_grasps=r2[idx].cpu().numpy(), device=dev, ol_alg=cfg.ol_alg)
    eng, ms["engine_setup"] = timed(setup, dev)
    _, ms["plan"] = timed(eng.plan, dev)
    ms["grasps_to_plans_sum"] = sum(ms[key] for key in ("ik", "scene_table", "collision_stats", "selection_stage", "engine_setup", "plan"))
    stats = dict(goals_per_scene_mean=float(counts.float().mean().item()), num_free_mean=float(host[1].mean()),
                 num_candidates_mean=float(host[0].mean()), num_candidates_min=int(host[0].min()),
                 num_candidates_max=int(host[0].max()), goals_after_draw_mean=float(k.mean()), scenes_planned=int((k > 0).sum()))
    return ms, stats, (gs, counts, col, pot, rs)


def host_loop(gs, counts, col, pot, rs, cfg, seed):
    """The reference's per-scene selection on this host: goalset.select_goals over the same statistics."""
    g, c, cl, pt, r = gs.cpu().numpy(), counts.cpu().numpy(), col.cpu().numpy(), pot.cpu().numpy(), rs.cpu().numpy()
    rng = np.random.RandomState(seed)
    t0 = time.perf_counter()
    for s in range(g.shape[0]):
        n = int(c[s])
        goalset.select_goals(list(g[s, :n]), list(r[s, :n]), cl[s, :n], pt[s, :n], cfg.allow_collision_point, cfg.goal_set_max_num,
                             rng=rng)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=100)
    ap.add_argument("--grasps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = rb.PandaModel()
    cfg = Config(timeout=-1, silent=True)
    grasps, objs, starts = workload(model, a.scenes, a.grasps)
    scenes = []
    for s in range(a.scenes):
        scene = sc.make_tabletop_scene(s, grid=32, table_grid=(48, 32, 16))
        scene.objects[scene.target_idx].pose_mat = objs[s].copy()
        scenes.append(scene)
    starts9 = np.ascontiguousarray(starts)
    runs = []
    for r in range(a.reps + 1):  # the first pass warms the process up (code objects, allocator) and is not reported
        ms, stats, keep = one_pass(model, scenes, grasps, objs, starts9, cfg, dev, seed=r)
        if r:
            runs.append(ms)
    med = {k: float(np.median([m[k] for m in runs])) for k in runs[0]}
    loop_ms = [host_loop(*keep, cfg, seed=0) for _ in range(2)]
    full = []
    for r in range(a.reps):
        _, t = timed(lambda: pipeline.plan_grasps(model, scenes, grasps, starts9, cfg, rng=np.random.RandomState(r), device=dev), dev)
        full.append(t)
    res = {"device": torch.cuda.get_device_name(0), "scenes": a.scenes, "grasps_per_scene": a.grasps, "reps": a.reps,
           "stage_ms_median": med, "stage_ms_runs": runs, "workload": stats,
           "host_select_goals_loop_ms": float(np.median(loop_ms)), "host_select_goals_loop_runs_ms": loop_ms,
           "selection_speedup_vs_host_loop": float(np.median(loop_ms) / med["selection_stage"]),
           "plan_grasps_ms_median": float(np.median(full)), "plan_grasps_runs_ms": full,
           "note": "stage times end with a device sync each; the host loop runs goalset.select_goals (the reference's loop) on "
                   "this machine's CPU over the same collision statistics"}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
