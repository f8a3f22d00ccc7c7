"""Timing of the robot self-filter (omgx_render_spheres, omgx_clear_robot) on one GPU, beside what a user would write today.

  python tools/robot_filter_timing.py [--reps 9] [--out profiles/robot_filter_timing.json]

The arm: one sphere of radius 0.04 (+ 0.01 pad) per collision point of PandaModel(seed=0), 150 in all, at configurations drawn
around the home configuration; the camera of tests/robot_filter_cases.py (looking down on the hand from 0.65 m), scaled to the image.
  (a) one 640 x 480 view;
  (b) 100 views of 160 x 120, one configuration each, and omgx_clear_robot on 100 volumes of 64^3 (5 mm, around the hand) with
      three of the views each, states half UNKNOWN and half SURFACE, depths within 5 cm of the arm's.
For each shape:
  kernel   the entry point alone through the C ABI, everything already on the device, between two HIP events on the stream,
           with its cull and without; the median of `reps` launches after three warm-up launches
  torch    the composition a user would write today, the same clock: pixels x spheres broadcast with min (the specification's
           operations on tensors [V,H*W,N]); nodes x spheres with any, per volume and view (tensors [nodes,N])
  equal    whether the composition's t_near / states equal the kernel's (torch may fuse or reorder nothing here: + - * / sqrt)
The float64 VALU-issue bound as DESIGN.md section 5.2 prices it, from the instruction mix of the compiled loops (counted in the
ISA of csrc/omg_robot_filter.hip; 4 issue cycles per float64 add / mul / fma / compare / division step, 8 per v_rcp_f64 /
v_rsq_f64, 2 per select, move or integer instruction, on one of 1024 SIMDs at 2.4 GHz):
  render  a (wave, sphere) pair that the ballot skips: 9 + 0 + 4 instructions = 44 cycles; one that is walked to a hit: 46 + 3 + 14
          = 236 cycles more (the square root is 13 float64 steps and a v_rsq_f64, each division 10 and a v_rcp_f64); without the
          cull every pair costs the 236, or 40 where all lanes miss at the discriminant
  clear   a (wave, staged sphere) pair: 9 float64 instructions and a move = 38 cycles; without the cull every sphere of every
          view is staged.  With the cull the number staged is not read back, so that bound is not priced.
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

from omg_planner_amd import _lib, camera as cam, fusion, ops, robot as rb  # noqa: E402
from tests import fusion_cases as FC, robot_filter_cases as RC  # noqa: E402

SKIP_CYCLES, HIT_CYCLES, MISS_CYCLES, INSIDE_CYCLES = 9 * 4 + 4 * 2, 46 * 4 + 3 * 8 + 14 * 2, 8 * 4 + 4 * 2, 9 * 4 + 2
SIMDS, CLOCK_HZ = 1024, 2.4e9
INF = float("inf")


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


def torch_render(cs, k, H, W, t_min):
    """The specification's operations on [V,H*W,N] tensors -> (t_near [V,H*W], active [V,H*W,N]: the cull's test per pixel)."""
    r, c = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=cs.device), torch.arange(W, dtype=torch.float64, device=cs.device), indexing="ij")
    dx = ((c.reshape(1, -1) - k[:, 2:3]) / k[:, 0:1])[:, :, None]
    dy = ((r.reshape(1, -1) - k[:, 3:4]) / k[:, 1:2])[:, :, None]
    dd = (dx * dx + dy * dy) + 1.0
    x, y, z, R = (cs[:, None, :, j] for j in range(4))
    b = (x * dx + y * dy) + z
    q = ((x * x + y * y) + z * z) - R * R
    disc = b * b - q * dd
    root = torch.sqrt(torch.clamp_min(disc, 0.0))
    t0, t1 = (b - root) / dd, (b + root) / dd
    hit = (disc >= 0.0) & (t1 > t_min)
    entry = torch.where(hit, torch.clamp_min(t0, t_min), torch.full_like(t0, INF))
    return entry.min(dim=2).values, (q <= 0.0) | ((b > 0.0) & (b * b >= q * dd))


def torch_clear(state, nodes, begin, points, views, ranges, depth, t_near, cs, near, tol):
    """Per volume and view: the projection, `front` on the images, and nodes x spheres with any."""
    V, H, W = depth.shape
    for m in range(len(begin)):
        p, mine = points[m], state[begin[m]: begin[m] + nodes]
        inside, front = torch.zeros(nodes, dtype=torch.bool, device=p.device), torch.zeros(nodes, dtype=torch.bool, device=p.device)
        for v in range(ranges[m][0], ranges[m][0] + ranges[m][1]):
            vw = views[v]
            q = [((vw[4 + 4 * j] * p[:, 0] + vw[5 + 4 * j] * p[:, 1]) + vw[6 + 4 * j] * p[:, 2]) + vw[7 + 4 * j] for j in range(3)]
            cf, rf = torch.floor((vw[0] * (q[0] / q[2]) + vw[2]) + 0.5), torch.floor((vw[1] * (q[1] / q[2]) + vw[3]) + 0.5)
            seen = (q[2] > near) & (cf >= 0) & (cf <= W - 1) & (rf >= 0) & (rf <= H - 1)
            at = torch.where(seen, rf * W + cf, torch.zeros_like(cf)).long()
            tn, d = t_near[v].reshape(-1)[at], depth[v].reshape(-1)[at]
            front |= seen & (tn < INF) & (d >= tn - tol) & (q[2] < tn)
            e = [q[j][:, None] - cs[v, None, :, j] for j in range(3)]
            inside |= (((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= cs[v, None, :, 3] * cs[v, None, :, 3]).any(dim=1)
        mine[:] = torch.where(inside | ((mine == fusion.UNKNOWN) & front), torch.zeros_like(mine), mine)
    return state


def measure(name, V, H, W, focal, with_clear, grid, reps, dev, stream, seed):
    rng = np.random.default_rng(seed)
    model = rb.PandaModel(seed=0)
    blob, P = ops.robot_blob(model, dev), model.points_per_link
    spheres = ops.RobotSpheres.from_points(model.collision_points, RC.PANDA_RADIUS, dev)
    N = spheres.N
    joints = np.stack([rb.HOME_CONFIG + np.concatenate([rng.normal(scale=0.15, size=7), [0.0, 0.0]]) for _ in range(V)])
    poses = ops.forward_kinematics(blob, P, torch.from_numpy(joints).to(dev), want_joint_info=False)[0]
    h_poses = np.ascontiguousarray(poses.cpu().numpy())
    cfw = FC.look_at(RC.PANDA_EYE, RC.PANDA_TARGET)
    intr = (focal, focal, 0.5 * (W - 1), 0.5 * (H - 1))
    h_cam = RC.camera_records(np.tile(cfw, (V, 1, 1)), intr)
    d_cam = torch.from_numpy(np.frombuffer(h_cam.tobytes(), np.uint8).copy()).to(dev)
    h_cfg = np.arange(V, dtype=np.int32)
    d_cfg = torch.from_numpy(h_cfg).to(dev)
    t_near = torch.empty((V, H, W), dtype=torch.float64, device=dev)
    which = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    cs = torch.empty((V, N, 4), dtype=torch.float64, device=dev)
    l, vp = _lib.lib(), C.c_void_p
    p = lambda x: vp(x.data_ptr())

    def render(cull):
        _lib.check(l.omgx_render_spheres(p(spheres.local), vp(spheres.h_local.ctypes.data), p(spheres.link), vp(spheres.h_link.ctypes.data), N, p(poses),
                                         vp(h_poses.ctypes.data), V, p(d_cam), vp(h_cam.ctypes.data), p(d_cfg), vp(h_cfg.ctypes.data), V, H, W, RC.PANDA_PAD,
                                         1e-6, cull, p(cs), p(t_near), p(which), vp(stream.cuda_stream)), "omgx_render_spheres")
    k_off = by_events(lambda: render(0), reps, stream)
    t_off = t_near.clone()
    k_on = by_events(lambda: render(1), reps, stream)
    k = torch.from_numpy(np.tile(np.array(intr), (V, 1))).to(dev)
    tr = by_events(lambda: torch_render(cs, k, H, W, 1e-6), max(reps // 3, 3), stream, warm_up=1)
    t_torch, active = torch_render(cs, k, H, W, 1e-6)
    # (wave, sphere) pairs: an 8 x 8 block of pixels is a wave; walked: some pixel of the block passes the cull's test
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    blocks = torch.zeros((V, Hp, Wp, N), dtype=torch.bool, device=dev)
    blocks[:, :H, :W] = active.reshape(V, H, W, N)
    walked = int(blocks.reshape(V, Hp // 8, 8, Wp // 8, 8, N).any(dim=4).any(dim=2).sum().item())
    pairs = V * (Hp // 8) * (Wp // 8) * N
    per_cycle_ms = 1e3 / (SIMDS * CLOCK_HZ)
    res = {"shape": name, "views": V, "H": H, "W": W, "spheres": N, "pad": RC.PANDA_PAD, "hit_pixels": int(torch.isfinite(t_near).sum().item()),
           "share_of_pixels_hit": float(torch.isfinite(t_near).double().mean().item()), "wave_sphere_pairs": pairs, "pairs_walked_with_cull": walked,
           "render_cull_ms": k_on[0], "render_cull_runs_ms": k_on[1], "render_no_cull_ms": k_off[0], "render_no_cull_runs_ms": k_off[1],
           "render_same_bits_with_and_without_cull": bool(torch.equal(t_off.view(torch.int64), t_near.view(torch.int64))),
           "torch_render_ms": tr[0], "torch_render_runs_ms": tr[1], "torch_render_equals_kernel": bool(torch.equal(t_torch.reshape(V, H, W), t_near)),
           "torch_render_over_kernel": tr[0] / k_on[0],
           "render_valu_bound_cull_ms": (pairs * SKIP_CYCLES + walked * HIT_CYCLES) * per_cycle_ms,
           "render_valu_bound_no_cull_ms": (walked * HIT_CYCLES + (pairs - walked) * MISS_CYCLES) * per_cycle_ms}
    res["render_cull_over_bound"] = k_on[0] / res["render_valu_bound_cull_ms"]
    res["render_no_cull_over_bound"] = k_off[0] / res["render_valu_bound_no_cull_ms"]
    del active, blocks, t_torch
    if not with_clear:
        return res
    M, views_per = V, 3
    delta, dims = 0.32 / grid, (grid, grid, grid)
    nodes = grid ** 3
    volumes = [((0.0, -0.16, 0.46), delta, "centre", dims, m * nodes) for m in range(M)]  # (the world frame: around the hand)
    h_views = np.stack([fusion.view_rows(intr, cfw)] * V)
    ranges = [(min(m, V - views_per), views_per) for m in range(M)]
    depth = torch.where(torch.isfinite(t_near), t_near + torch.from_numpy(rng.uniform(-0.05, 0.05, (V, H, W))).to(dev),
                        torch.from_numpy(rng.uniform(0.4, 1.2, (V, H, W))).to(dev)).contiguous()
    start = torch.from_numpy(rng.choice(np.array([1, 2], np.uint8), size=M * nodes)).to(dev)
    state = start.clone()
    batch = ops._VolumeBatch(volumes)
    d_views, h_range = torch.from_numpy(h_views).to(dev), np.ascontiguousarray(ranges, np.int32)
    d_range = torch.from_numpy(h_range).to(dev)
    batch.on(dev)
    vol_args, begin_args = batch.volume_args(), batch.begin_args()

    def clear(cull):
        state.copy_(start)
        _lib.check(l.omgx_clear_robot(*vol_args, p(d_views), vp(h_views.ctypes.data), V, p(d_range), vp(h_range.ctypes.data), *begin_args, p(depth),
                                      p(t_near), H, W, p(cs), None, N, FC.NEAR, RC.PANDA_TOL, cull, p(state), int(state.numel()), vp(stream.cuda_stream)),
                   "omgx_clear_robot")
    copy = by_events(lambda: state.copy_(start), reps, stream)  # (every timed launch starts from the same states: the copy is taken off)
    c_off = by_events(lambda: clear(0), reps, stream)
    s_off = state.clone()
    c_on = by_events(lambda: clear(1), reps, stream)
    points = [torch.from_numpy(fusion.node_points(np.array(v[0]), v[1], 0.5, v[3])).to(dev) for v in volumes[:1]] * M
    begin = [m * nodes for m in range(M)]
    s_torch = start.clone()

    def composed():
        s_torch.copy_(start)
        torch_clear(s_torch, nodes, begin, points, d_views, ranges, depth, t_near, cs, FC.NEAR, RC.PANDA_TOL)
    tc = by_events(composed, 3, stream, warm_up=1)
    runs = M * -(-nodes // 256)
    res.update({"volumes": M, "volume_dims": list(dims), "views_per_volume": views_per, "states_changed": int((state != start).sum().item()),
                "state_copy_ms": copy[0], "clear_cull_ms": c_on[0] - copy[0], "clear_cull_runs_ms": c_on[1], "clear_no_cull_ms": c_off[0] - copy[0],
                "clear_no_cull_runs_ms": c_off[1], "clear_same_bytes_with_and_without_cull": bool(torch.equal(s_off, state)),
                "torch_clear_ms": tc[0] - copy[0], "torch_clear_runs_ms": tc[1], "torch_clear_equals_kernel": bool(torch.equal(s_torch, state)),
                "torch_clear_over_kernel": (tc[0] - copy[0]) / (c_on[0] - copy[0]),
                "clear_valu_bound_no_cull_ms": runs * 4 * views_per * N * INSIDE_CYCLES * per_cycle_ms})
    res["clear_no_cull_over_bound"] = res["clear_no_cull_ms"] / res["clear_valu_bound_no_cull_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "robot_filter_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robot_filter_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    shapes = [("a_one_view_640x480", 1, 480, 640, 800.0, False, 64), ("b_100_views_160x120", 100, 120, 160, 200.0, True, 64)]
    if a.small:
        shapes = [("a_small", 1, 48, 64, 80.0, False, 16), ("b_small", 4, 24, 32, 40.0, True, 16)]
    res = {"device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "issue_cycles": {"render_pair_skipped": SKIP_CYCLES, "render_pair_walked_to_a_hit": HIT_CYCLES, "render_pair_all_lanes_miss": MISS_CYCLES,
                            "clear_pair_staged": INSIDE_CYCLES},
           "shapes": [measure(s[0], *s[1:], a.reps, dev, stream, k) for k, s in enumerate(shapes)]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in s.items() if not k.endswith("_runs_ms")} for s in res["shapes"]]))


if __name__ == "__main__":
    main()
