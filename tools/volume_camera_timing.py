"""Timing of the depth camera on the SDF pool (omgx_render_volumes) on one GPU, beside the route it stands beside.

  python tools/volume_camera_timing.py [--reps 9] [--out profiles/volume_camera_timing.json]

Two shapes (DESIGN.md section 7f's), every object a 64^3 volume of a 0.2 m cube (five spheres and five boxes of different sizes,
stored once each), at a random rotation, 0.5 .. 0.7 m in front of the camera, spread over the image:
  (a) one scene at 640 x 480 with ten objects;
  (b) 100 scenes at 160 x 120 with five objects each.
For each shape, on the same scene table:
  kernel          omgx_render_volumes alone through the C ABI, cameras already on the device, between two HIP events on the
                  stream: t and inst only, and with normals and steps; the median of `reps` launches after three warm-up launches
  observe_volumes the whole camera.observe_volumes (records, upload of the cameras, launch) by a host clock around the call and
                  a device synchronise, median of `reps`
  observe_table   the parent's route, whole: camera.observe_table (surface nets of every volume, download, host records, upload
                  of a mesh pool, ops.render_depth), the same clock
  render_depth    ops.render_depth alone on the meshes observe_table extracted (kernel against kernel), HIP events
  samples         the sum and the maximum of `steps`, and the sum over the 8 x 8 blocks of a wave of the block's largest count: the
                  iterations the waves run, at least
The bound of the kernel as DESIGN.md section 5.2 prices it: the compiled march loop has VALU_F64 + VALU_TRANS + VALU_OTHER
instructions per sample (counted in the ISA of csrc/omg_volume_camera.hip: the loop between the two s_cbranch_execz of the march),
4 / 8 / 2 issue cycles each on one of 1024 SIMDs at 2.4 GHz; a wave-instruction serves 64 samples at best (the sum) and one
sample per iteration of its slowest lane at worst (the block maxima).  Beside it 32 bytes gathered per sample against the L2's
17 TB/s (MI355X_MICROARCH: rows shared by an XCD's workgroups).  The JSON says which is larger.
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

from omg_planner_amd import _lib, ops, volume_camera as vc  # noqa: E402
from omg_planner_amd import camera as cam, scenes as sc  # noqa: E402
from tests import mesh_cases as MC  # noqa: E402

VALU_F64, VALU_TRANS, VALU_OTHER = 71, 2, 62  # per sample of the march loop: f64 add / mul / fma / cvt / div steps; v_rcp_f64; the rest
ISSUE_CYCLES = VALU_F64 * 4 + VALU_TRANS * 8 + VALU_OTHER * 2
SIMDS, CLOCK_HZ, L2_BYTES_PER_S, BYTES_PER_SAMPLE = 1024, 2.4e9, 17e12, 32


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


def by_clock(fn, reps, warm_up=2):
    for _ in range(warm_up):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), ms


def make_table(grids, S, H, W, focal, per_scene, seed, dev):
    rng = np.random.RandomState(seed)
    intr = (focal, focal, 0.5 * (W - 1), 0.5 * (H - 1))
    cols = (per_scene + 1) // 2
    made = []
    for _ in range(S):
        objs = []
        for k in range(per_scene):
            ur, uc = (0.3 + 0.4 * (k // cols)) + rng.uniform(-0.1, 0.1), (k % cols + 0.5) / cols + rng.uniform(-0.05, 0.05)
            z = rng.uniform(0.5, 0.7)
            pose = MC.pose(rng.uniform(-1.5, 1.5, 3), ((uc * W - intr[2]) / focal * z, (ur * H - intr[3]) / focal * z, z))
            objs.append(sc.SceneObject(f"object{k}", np.asarray(pose, np.float64).reshape(4, 4), grids[(len(made) + k) % len(grids)]))
        made.append(sc.Scene(objs, 0))
    return ops.DeviceScenes.from_scenes(made, device=dev), intr


def measure(name, grids, S, H, W, focal, per_scene, reps, dev, stream, march):
    table, intr = make_table(grids, S, H, W, focal, per_scene, S, dev)
    cfw = np.eye(4)
    cameras = np.stack([cam.camera_rows(intr, cfw)] * S)
    d_cameras = torch.from_numpy(cameras).to(dev)
    t, inst = torch.empty((S, H, W), dtype=torch.float64, device=dev), torch.empty((S, H, W), dtype=torch.int32, device=dev)
    normal, steps = torch.empty((S, H, W, 3), dtype=torch.float64, device=dev), torch.empty((S, H, W), dtype=torch.int32, device=dev)
    l, vp, n = _lib.lib(), C.c_void_p, len(table.host_objects)
    p = lambda x: None if x is None else vp(x.data_ptr())
    h_begin = np.ascontiguousarray(table.host_scene_begin, np.int32)

    def kernel(full):
        _lib.check(l.omgx_render_volumes(p(table.objects), vp(table.host_objects.ctypes.data), n, p(table.scene_begin), vp(h_begin.ctypes.data), S,
                                         p(table.pool), int(table.pool.numel()), p(d_cameras), vp(cameras.ctypes.data), None, None, H, W, 0.0, 1e-6,
                                         march["min_step"], 1.0, march["max_steps"], p(t), p(inst), p(normal) if full else None,
                                         p(steps) if full else None, vp(stream.cuda_stream)), "omgx_render_volumes")
    k_plain, k_full = by_events(lambda: kernel(False), reps, stream), by_events(lambda: kernel(True), reps, stream)
    h_steps = steps.cpu().numpy().astype(np.int64)
    hits = int((inst >= 0).sum().item())
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    padded = np.zeros((S, Hp, Wp), np.int64)
    padded[:, :H, :W] = h_steps
    wave_iterations = int(padded.reshape(S, Hp // 8, 8, Wp // 8, 8).max(axis=(2, 4)).sum())
    whole_v = by_clock(lambda: cam.observe_volumes(table, cfw, intr, H, W, **march), reps)
    whole_m = by_clock(lambda: cam.observe_table(table, cfw, intr, H, W), max(reps // 3, 3))
    obs = cam.observe_table(table, cfw, intr, H, W)
    out = (torch.empty_like(t), torch.empty_like(inst), torch.empty_like(inst))
    k_mesh = by_events(lambda: ops.render_depth(obs.batch, H, W, out=out), reps, stream)
    both = torch.isfinite(t) & torch.isfinite(out[0])
    samples = int(h_steps.sum())
    per_sample_s = ISSUE_CYCLES / (SIMDS * CLOCK_HZ)
    bound_best, bound_waves = samples / 64 * per_sample_s * 1e3, wave_iterations * per_sample_s * 1e3
    bound_l2 = samples * BYTES_PER_SAMPLE / L2_BYTES_PER_S * 1e3
    return {
        "shape": name, "scenes": S, "H": H, "W": W, "objects_per_scene": per_scene, "volume_dims": list(grids[0].data.shape), **march,
        "hit_pixels": hits, "share_of_pixels_hit": hits / (S * H * W), "samples_sum": samples, "samples_max_per_pixel": int(h_steps.max()),
        "samples_per_pixel_mean": samples / (S * H * W), "wave_iterations_at_least": wave_iterations,
        "lane_use_of_the_march_at_most": samples / max(64 * wave_iterations, 1),
        "kernel_t_inst_ms": k_plain[0], "kernel_t_inst_runs_ms": k_plain[1], "kernel_with_normals_steps_ms": k_full[0],
        "kernel_with_normals_steps_runs_ms": k_full[1], "observe_volumes_whole_ms": whole_v[0], "observe_volumes_runs_ms": whole_v[1],
        "observe_table_whole_ms": whole_m[0], "observe_table_runs_ms": whole_m[1], "render_depth_kernel_on_extracted_meshes_ms": k_mesh[0],
        "render_depth_runs_ms": k_mesh[1], "extracted_faces": int(obs.batch.faces.shape[0]),
        "observe_table_over_observe_volumes": whole_m[0] / whole_v[0], "render_depth_kernel_over_volume_kernel": k_mesh[0] / k_plain[0],
        "pixels_hit_by_both": int(both.sum().item()),
        "largest_depth_difference_m_where_both_hit": float((t - out[0]).abs()[both].max().item()) if bool(both.any()) else None,
        "valu_issue_cycles_per_sample": ISSUE_CYCLES, "bound_valu_all_lanes_busy_ms": bound_best, "bound_valu_waves_as_marched_ms": bound_waves,
        "bound_l2_gather_ms": bound_l2, "larger_bound": "valu" if bound_waves >= bound_l2 else "l2",
        "kernel_over_valu_bound_as_marched": k_plain[0] / bound_waves if bound_waves else None,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--min-step", type=float, default=vc.MIN_STEP)
    ap.add_argument("--max-steps", type=int, default=vc.DEFAULT_STEPS)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "volume_camera_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("volume_camera_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    g = 16 if a.small else 64
    grids = [sc.sphere_sdf(r, (g,) * 3, 0.2 / g) for r in (0.04, 0.05, 0.06, 0.07, 0.08)]
    grids += [sc.box_sdf(h, (g,) * 3, 0.2 / g) for h in ((0.05, 0.04, 0.06), (0.03, 0.07, 0.05), (0.06, 0.06, 0.03), (0.07, 0.03, 0.04), (0.04, 0.05, 0.07))]
    shapes = [("a_one_scene_640x480", 1, 480, 640, 600.0, 10), ("b_100_scenes_160x120", 100, 120, 160, 150.0, 5)]
    if a.small:
        shapes = [("a_small", 1, 48, 64, 60.0, 10), ("b_small", 3, 24, 32, 30.0, 5)]
    march = dict(min_step=a.min_step, max_steps=a.max_steps)
    res = {"device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "shapes": [measure(s[0], grids, *s[1:], a.reps, dev, stream, march) for s in shapes]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in s.items() if not k.endswith("_runs_ms")} for s in res["shapes"]]))


if __name__ == "__main__":
    main()
