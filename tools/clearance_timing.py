"""Timing of plan clearance (omgx_sphere_clearance, omgx_self_clearance) on one GPU, beside what a user would write today.

  python tools/clearance_timing.py [--reps 9] [--out profiles/clearance_timing.json]

The arm: one sphere of radius 0.02 per collision point of PandaModel(seed=0), 150 in all.  The plans: 30 waypoints from the home
configuration to a goal of scenes.make_goal_set, sampled K = 8 times per segment (T = 233 configurations per plan).
  (a) one tabletop scene of 10 objects (scenes.make_tabletop_scene: 64^3 shapes and the table's 128 x 96 x 32), one plan;
  (b) 100 scenes of 5 objects, one plan each: the benchmark table's shape, 23300 configurations.
For each shape, everything already on the device, between two HIP events on the stream, the median of `reps` launches after three
warm-up launches:
  kernel   omgx_sphere_clearance through the C ABI with pads, with its cull and without (the same bits), and
           omgx_self_clearance alone on the world spheres the first wrote
  path     DeviceScenes.plan_clearance as a whole (dense configs, forward kinematics, both launches, the report in torch)
  fk_sdf   ops.fk_sdf on the same configurations with 15 points per link, potentials only: the same (configuration, point,
           object) pairs in a float32 cost layer, the parent's nearest kernel
  torch    the composition a user would write today from the world spheres: per object of a scene the index arithmetic, eight
           gathers from the pool, the interpolant, and amin over spheres and objects (tensors [B,N])
  numpy    the specification once on the CPU, a host clock ((b): on the first 10 scenes)
The float64 VALU-issue bound as DESIGN.md section 5.2 prices it, from the instruction mix of the compiled record loop (counted in
the ISA of csrc/omg_clearance.hip; 4 issue cycles per float64 add / mul / fma / compare / convert / division step, 8 per
v_rcp_f64 / v_rsq_f64, 2 per select, move or integer instruction, on one of 1024 SIMDs at 2.4 GHz), per (64 spheres, record):
  to the vote   83 float64 instructions, 2 transcendental, 18 others = 384 cycles (the point into the grid, the clamp, e: one
                square root of 13 float64 steps and a v_rsq_f64, one division of 10 and a v_rcp_f64); the record's own test
                (vcam_grid_usable, 180 scalar instructions with a 64-bit division) runs on the scalar unit and is not priced
  walked        45 float64 instructions and 34 others = 248 cycles more (eight conversions, the interpolant, two takes)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from omg_planner_amd import _lib, clearance as cl, ops, robot as rb, scenes as sc  # noqa: E402

VOTE_CYCLES, WALK_CYCLES = 83 * 4 + 2 * 8 + 18 * 2, 45 * 4 + 34 * 2
SIMDS, CLOCK_HZ = 1024, 2.4e9
RADIUS, BEYOND = 0.02, 0.1


def by_events(fn, reps, stream, warm_up=3):
    for _ in range(warm_up):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def torch_clearance(table, rec, world, cfg, beyond):
    """clear [B] from world [B,N,4] by tensor operations: the specification's lines on [B,N] tensors, object by object."""
    B, N = world.shape[:2]
    best = torch.full((B,), float("inf"), dtype=torch.float64, device=world.device)
    w, r = [world[:, :, a] for a in range(3)], world[:, :, 3]
    for k in range(rec["count"]):
        P, lo, hi, dim, inv, off, used = (rec[name][k][cfg] for name in ("pose", "lo", "hi", "dim", "inv_delta", "offset", "used"))  # [B, ...]
        u, i, f, x = [], [], [], []
        for a in range(3):
            q = ((P[:, 4 * a, None] * w[0] + P[:, 4 * a + 1, None] * w[1]) + P[:, 4 * a + 2, None] * w[2]) + P[:, 4 * a + 3, None]
            ua = (q - lo[:, a, None]) * inv[:, None] - 0.5
            c = torch.minimum(torch.where(ua >= 0.0, ua, torch.zeros_like(ua)), hi[:, a, None])
            ia = torch.minimum(c.long(), dim[:, a, None] - 2)
            u.append(ua), i.append(ia), f.append(c - ia.double()), x.append(ua - c)
        e = torch.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) / inv[:, None]
        sy, sx = dim[:, 2, None], dim[:, 1, None] * dim[:, 2, None]
        base = off[:, None] + (i[0] * dim[:, 1, None] + i[1]) * sy + i[2]
        g = lambda dx, dy, dz: table.pool[base + dx * sx + dy * sy + dz].double()
        c000, c001, c010, c011, c100, c101, c110, c111 = g(0, 0, 0), g(0, 0, 1), g(0, 1, 0), g(0, 1, 1), g(1, 0, 0), g(1, 0, 1), g(1, 1, 0), g(1, 1, 1)
        d00, d01, d10, d11 = c001 - c000, c011 - c010, c101 - c100, c111 - c110
        c00, c01, c10, c11 = c000 + f[2] * d00, c010 + f[2] * d01, c100 + f[2] * d10, c110 + f[2] * d11
        c0, c1 = c00 + f[1] * (c01 - c00), c10 + f[1] * (c11 - c10)
        d = (c0 + f[0] * (c1 - c0)) - e
        cand = torch.where((e <= beyond) & used[:, None], d - r, torch.full_like(d, float("inf")))
        best = torch.minimum(best, cand.amin(dim=1))
    return best


def record_tensors(table, dev):
    """The records as [Kmax][S, ...] tensors for torch_clearance: object k of every scene (a scene with fewer repeats its first, unused)."""
    h, begin = table.host_objects, table.host_scene_begin
    S, count = table.num_scenes, int(np.diff(begin).max())
    idx = np.array([[begin[s] + k if begin[s] + k < begin[s + 1] else begin[s] for s in range(S)] for k in range(count)])
    used = np.array([[begin[s] + k < begin[s + 1] and h["disabled"][idx[k, s]] == 0 for s in range(S)] for k in range(count)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(count=count, pose=up(h["pose_inv"][idx].astype(np.float64)), lo=up(h["lo"][idx].astype(np.float64)), hi=up((h["dim"][idx] - 1).astype(np.float64)),
                dim=up(h["dim"][idx].astype(np.int64)), inv_delta=up(h["inv_delta"][idx]), offset=up(h["grid_offset"][idx]), used=up(used))


def measure(name, S, objects_per_scene, K, reps, dev, stream, spec_scenes):
    model = rb.PandaModel(seed=0)
    blob, P = ops.robot_blob(model, dev), model.points_per_link
    spheres = ops.RobotSpheres.from_points(model.collision_points, RADIUS, dev)
    spheres.reach_table(model)
    N = spheres.N
    scenes = [sc.make_tabletop_scene(s, num_objects=objects_per_scene - 1) for s in range(S)]
    table = ops.DeviceScenes.from_scenes(scenes, device=dev)
    n = 30
    h_traj = np.stack([sc.linear_init(rb.HOME_CONFIG, sc.make_goal_set(s, 1)[0], n) for s in range(S)])
    traj = torch.from_numpy(np.ascontiguousarray(h_traj)).to(dev)
    T = (n - 1) * K + 1
    B = S * T
    q = ops.dense_configs(traj, K)
    poses = ops.forward_kinematics(blob, P, q.reshape(B, 9), want_joint_info=False)[0]
    h_pad = cl.sample_pads(cl.segment_halves(h_traj, K, spheres.rho), K, 0.0).reshape(B, 10)
    pad = torch.from_numpy(h_pad).to(dev)
    h_cfg = np.ascontiguousarray(np.repeat(np.arange(S), T), np.int32)
    d_cfg = torch.from_numpy(h_cfg).to(dev)
    h_begin = np.ascontiguousarray(table.host_scene_begin, np.int32)
    out = [torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
           torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)]
    world = torch.empty((B, N, 4), dtype=torch.float64, device=dev)
    l, vp = _lib.lib(), C.c_void_p
    p = lambda x: vp(x.data_ptr())

    def kernel(cull):
        _lib.check(l.omgx_sphere_clearance(p(table.objects), vp(table.host_objects.ctypes.data), len(table.host_objects), p(table.scene_begin),
                                           vp(h_begin.ctypes.data), S, p(table.pool), int(table.pool.numel()), None, None, p(d_cfg), vp(h_cfg.ctypes.data), B,
                                           p(poses), p(spheres.local), vp(spheres.h_local.ctypes.data), p(spheres.link), vp(spheres.h_link.ctypes.data), N,
                                           p(pad), BEYOND, cull, *[p(x) for x in out], p(world), vp(stream.cuda_stream)), "omgx_sphere_clearance")
    k_off = by_events(lambda: kernel(0), reps, stream)
    off = [x.clone() for x in out]
    k_on = by_events(lambda: kernel(1), reps, stream)
    same = all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b) for a, b in zip(off, out))
    pairs = ops.default_self_pairs()
    d_pairs = torch.from_numpy(pairs).to(dev)
    own = [torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)]

    def self_kernel():
        _lib.check(l.omgx_self_clearance(p(world), B, p(spheres.link), vp(spheres.h_link.ctypes.data), N, p(d_pairs), p(pad), *[p(x) for x in own],
                                         vp(stream.cuda_stream)), "omgx_self_clearance")
    k_self = by_events(self_kernel, reps, stream)
    path = by_events(lambda: table.plan_clearance(spheres, blob, P, traj, K, beyond=BEYOND, pairs=pairs), reps, stream)
    pot = torch.empty((S, T, 10, P), dtype=torch.float32, device=dev)
    fk = by_events(lambda: ops.fk_sdf(blob, P, table, q, out=(pot, None, None)), reps, stream)
    rec = record_tensors(table, dev)
    tr = by_events(lambda: torch_clearance(table, rec, world, d_cfg.long(), BEYOND), max(reps // 3, 3), stream, warm_up=1)
    t_clear = torch_clearance(table, rec, world, d_cfg.long(), BEYOND)
    torch.cuda.synchronize()
    # the specification on the CPU, on the device's poses
    Bs = min(S, spec_scenes) * T
    h_poses, h_pool = poses[:Bs].cpu().numpy(), table.pool.cpu().numpy()
    t0 = time.perf_counter()
    h_world = cl.world_spheres(h_poses, spheres.h_local, spheres.h_link)
    want = cl.sphere_clearance(table.host_objects, h_begin, h_pool, None, h_cfg[:Bs], h_world, spheres.h_link, h_pad[:Bs], BEYOND)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    equal = all(np.array_equal(w.view(np.int64) if w.dtype == np.float64 else w, x[:Bs].cpu().numpy().view(np.int64) if w.dtype == np.float64 else x[:Bs].cpu().numpy())
                for w, x in zip(want, out))
    used = (table.host_objects["disabled"] == 0)
    groups = sum(T * -(-N // 64) * int(used[h_begin[s]: h_begin[s + 1]].sum()) for s in range(S))
    per_cycle_ms = 1e3 / (SIMDS * CLOCK_HZ)
    res = {"shape": name, "scenes": S, "objects_per_scene": objects_per_scene, "waypoints": n, "K": K, "configurations": B, "spheres": N, "beyond": BEYOND,
           "used_records_per_scene": float(np.mean([used[h_begin[s]: h_begin[s + 1]].sum() for s in range(S)])),
           "configurations_with_an_answer": int((out[1] >= 0).sum().item()), "min_clearance": float(out[0].min().item()),
           "kernel_cull_ms": k_on[0], "kernel_cull_runs_ms": k_on[1], "kernel_no_cull_ms": k_off[0], "kernel_no_cull_runs_ms": k_off[1],
           "same_bits_with_and_without_cull": bool(same), "self_clearance_ms": k_self[0], "self_clearance_runs_ms": k_self[1],
           "plan_clearance_path_ms": path[0], "plan_clearance_path_runs_ms": path[1], "fk_sdf_ms": fk[0], "fk_sdf_runs_ms": fk[1],
           "fk_sdf_over_kernel": fk[0] / k_on[0], "torch_ms": tr[0], "torch_runs_ms": tr[1], "torch_over_kernel": tr[0] / k_on[0],
           "torch_clear_equals_kernel": bool(torch.equal(t_clear.view(torch.int64), out[0].view(torch.int64))),
           "numpy_ms": numpy_ms, "numpy_configurations": Bs, "numpy_equals_kernel": bool(equal),
           "sphere_group_record_pairs": groups, "valu_bound_all_walked_ms": groups * (VOTE_CYCLES + WALK_CYCLES) * per_cycle_ms,
           "valu_bound_all_skipped_ms": groups * VOTE_CYCLES * per_cycle_ms}
    res["kernel_no_cull_over_bound_all_walked"] = k_off[0] / res["valu_bound_all_walked_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clearance_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clearance_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    shapes = [("a_one_scene_10_objects", 1, 10, 8, 1), ("b_100_scenes_5_objects", 100, 5, 8, 10)]
    if a.small:
        shapes = [("a_small", 1, 3, 2, 1), ("b_small", 3, 2, 2, 2)]
    res = {"device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "issue_cycles": {"pair_to_the_vote": VOTE_CYCLES, "pair_walked_more": WALK_CYCLES},
           "shapes": [measure(s[0], s[1], s[2], s[3], a.reps, dev, stream, s[4]) for s in shapes]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in s.items() if not k.endswith("_runs_ms")} for s in res["shapes"]]))


if __name__ == "__main__":
    main()
