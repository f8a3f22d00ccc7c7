"""Timing of the goal-set IK (omgx_goal_ik through goal_ik.solve_goal_sets) on one GPU.

  python tools/goal_ik_timing.py [--scenes 100] [--grasps 200] [--reps 5] [--out profiles/goal_ik_timing.json]

Two batches: S scenes x G grasps x 13 seeds with standoff (5 solves per chain after the pre-solve), and the same scenes with one
placement pose each under z_upsample (50 rotations per grasp).  Reports ms per batch for the kernel alone and for the whole
solve_goal_sets call (pose preparation, kernel, compaction, flips, filter), solves per second, the histogram of iterations per
solve, and the CPU restatement's (tests/ik_restatement.py) time for a subset of the chains, scaled to the batch.  The reference's
own IK (PyKDL on a Pool(4)) cannot run here, so there is no reference time to compare with.
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

from omg_planner_amd import goal_ik, ops  # noqa: E402
from omg_planner_amd import robot as rb  # noqa: E402
from omg_planner_amd import scenes as sc  # noqa: E402
from omg_planner_amd.config import Config  # noqa: E402


def workload(model, S, G, seed=0):
    import ik_restatement as ikr
    rng = np.random.RandomState(seed)
    q, pos, _, tree = sc._reach_pool(model)
    objs, grasps, starts = [], [], []
    for s in range(S):
        obj = np.eye(4)
        obj[:3, 3] = [rng.uniform(0.4, 0.6), rng.uniform(-0.2, 0.2), rng.uniform(0.15, 0.3)]
        idx = np.array(tree.query_ball_point(obj[:3, 3], 0.25))
        pick = rng.choice(idx, G, replace=idx.size < G)
        R, t, _, _ = ikr.hand_kinematics(model, q[pick, :7])
        H = np.tile(np.eye(4), (G, 1, 1))
        H[:, :3, :3], H[:, :3, 3] = R, t
        objs.append(obj)
        grasps.append(np.linalg.inv(obj) @ H)
        starts.append(rb.HOME_CONFIG.copy())
    return grasps, np.stack(objs), np.stack(starts)


def time_batch(model, dev, grasps, objs, starts, cfg, reps, **kw):
    blob = ops.robot_blob(model, dev)
    targets, begin = goal_ik._flat_targets(grasps, objs, cfg, True, kw.get("z_upsample", False), False, dev)
    seeds = torch.as_tensor(np.stack([goal_ik.ik_seeds(s, cfg.ik_seed_num) for s in starts]), dtype=torch.float64, device=dev)
    run = lambda it=False: ops.goal_ik(blob, model.points_per_link, targets, begin, seeds, cfg.use_standoff, kw.get("attached", False),
                                       want_iterations=it)
    _, _, its = run(True)
    torch.cuda.synchronize()
    kern = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        kern.append(a.elapsed_time(b))
    full = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = goal_ik.solve_goal_sets(model, grasps, objs, starts, cfg, device=dev, **kw)
        torch.cuda.synchronize()
        full.append((time.perf_counter() - t0) * 1e3)
    it = its.cpu().numpy().ravel()
    ran = it[it >= 0]
    hist = np.bincount(ran, minlength=101)
    return dict(grasps=int(targets.shape[0]), chains=int(targets.shape[0] * seeds.shape[1]), solves=int(ran.size),
                kernel_ms=float(np.median(kern)), solve_goal_sets_ms=float(np.median(full)),
                solves_per_s=float(ran.size / (np.median(kern) * 1e-3)), failed_solves=int((ran == 100).sum()),
                iteration_hist_0_100=hist.tolist(), goals_per_scene_mean=float(out[2].float().mean().item())), targets, begin


def restatement_time(model, targets, cfg, chains, n_grasps):
    """CPU restatement (vectorised numpy) on the first n_grasps grasps of the batch, scaled to `chains`."""
    import ik_restatement as ikr
    tg = targets[:n_grasps].cpu().numpy()
    seeds = goal_ik.ik_seeds(rb.HOME_CONFIG, cfg.ik_seed_num)
    R = np.zeros(tg.shape[:2] + (4, 4))
    R[..., :3, :3] = tg[..., :9].reshape(tg.shape[:2] + (3, 3))
    R[..., :3, 3] = tg[..., 9:]
    t0 = time.perf_counter()
    ikr.solve_grasps(model, R, seeds, cfg.use_standoff)  # vectorised over the subset's chains
    dt = time.perf_counter() - t0
    return dict(cpu_grasps=n_grasps, cpu_s=dt, cpu_s_scaled_to_batch=dt * chains / (n_grasps * len(seeds)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=100)
    ap.add_argument("--grasps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-grasps", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = rb.PandaModel()
    cfg = Config()
    grasps, objs, starts = workload(model, a.scenes, a.grasps)
    res = {"device": torch.cuda.get_device_name(0), "scenes": a.scenes, "grasps_per_scene": a.grasps, "seeds": 13}
    r, targets, _ = time_batch(model, dev, grasps, objs, starts, cfg, a.reps)
    r.update(restatement_time(model, targets, cfg, r["chains"], a.cpu_grasps))
    res["standoff"] = r
    zg = [g[:1] for g in grasps]
    r, targets, _ = time_batch(model, dev, zg, objs, starts, cfg, a.reps, z_upsample=True, attached=True)
    r.update(restatement_time(model, targets, cfg, r["chains"], a.cpu_grasps))
    res["z_upsample_attached"] = r
    res["note"] = "the reference's own IK time (PyKDL, Pool(4)) cannot be measured here: PyKDL is not available"
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
