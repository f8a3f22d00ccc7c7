"""Timing of the depth camera (omgx_render_depth, omgx_pixel_count + omgx_pixel_gather) on one GPU.

  python tools/depth_camera_timing.py [--level 4] [--reps 7] [--out profiles/depth_camera_timing.json]

Two shapes, every instance an icosphere of 20 * 4^level faces (level 4: 5120), radius 6 cm, at a random rotation:
  (a) one scene at 640 x 480 with ten instances spread over the image;
  (b) 100 scenes at 160 x 120 with five instances each.
For each shape: the render with the cull, the render without it, the three cloud launches (count, scan, gather of every hit,
into a buffer allocated before), and the composition that gives the same image without the camera kernel: one ray per
(instance, pixel), moved to the instance's frame by the specification's formula, through ops.mesh_raycast_batch (automatic face
chunks), then torch.min over the instances (the instance of a tie taken as the lowest index, explicitly).  The composition is timed twice: the ray cast and the reduction alone, and with the
ray set-up (torch, on the device) before them.  Each figure is the median of `reps` runs after three warm-up runs, between two HIP events
on the stream; meshes, records, rays and outputs are on the device before the first event.  The JSON also says whether the
three images are the same bits.
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

from omg_planner_amd import _lib, ops  # noqa: E402
from omg_planner_amd import camera as cam  # noqa: E402
from tests import mesh_cases as MC  # noqa: E402


def timed(fn, reps, stream, warm_up=3):
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


def make_shape(mesh, S, H, W, focal, per_scene, seed):
    """S scenes of `per_scene` instances of one mesh on a jittered grid over the image, depth 0.5 .. 0.7 m."""
    rng = np.random.RandomState(seed)
    intr = (focal, focal, 0.5 * (W - 1), 0.5 * (H - 1))
    cols = (per_scene + 1) // 2
    recs, begin, rows = [], [0], []
    for _ in range(S):
        poses = []
        for k in range(per_scene):
            ur, uc = (0.3 + 0.4 * (k // cols)) + rng.uniform(-0.1, 0.1), (k % cols + 0.5) / cols + rng.uniform(-0.05, 0.05)
            z = rng.uniform(0.5, 0.7)
            poses.append(MC.pose(rng.uniform(-1.5, 1.5, 3), ((uc * W - intr[2]) / focal * z, (ur * H - intr[3]) / focal * z, z)))
        recs.append(cam.instance_records([mesh], [0] * per_scene, poses, [k % 2 for k in range(per_scene)], np.eye(4)))
        begin.append(begin[-1] + per_scene)
        rows.append(cam.camera_rows(intr, np.eye(4)))
    return np.concatenate(recs), np.array(begin, np.int64), np.stack(rows)


def measure(name, mesh, S, H, W, focal, per_scene, reps, dev, stream):
    instances, begin, cameras = make_shape(mesh, S, H, W, focal, per_scene, seed=S)
    batch = ops.CameraBatch([mesh], instances, begin, cameras, device=dev)
    out = {c: (torch.empty((S, H, W), dtype=torch.float64, device=dev), torch.empty((S, H, W), dtype=torch.int32, device=dev),
               torch.empty((S, H, W), dtype=torch.int32, device=dev)) for c in (True, False)}
    ms = {}
    for c in (True, False):
        ms[c] = timed(lambda: ops.render_depth(batch, H, W, cull=c, out=out[c]), reps, stream)
    t, inst, face = out[True]
    same_cull = bool(torch.equal(t.view(torch.int64), out[False][0].view(torch.int64)) and torch.equal(inst, out[False][1]) and
                     torch.equal(face, out[False][2]))
    # the three cloud launches, every hit, no download in the timed window
    l = _lib.lib()
    ws = torch.empty(max(int(l.omgx_pixel_clouds_workspace_bytes(S, H, W)) // 4, 1), dtype=torch.int32, device=dev)
    d_begin = torch.empty(S + 1, dtype=torch.int32, device=dev)
    hits = int((inst >= 0).sum().item())
    points = torch.empty((hits, 3), dtype=torch.float64, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())

    def clouds():
        sp = C.c_void_p(stream.cuda_stream)
        _lib.check(l.omgx_pixel_count(*batch._records(), H, W, p(inst), -1, p(ws), p(d_begin), sp), "omgx_pixel_count")
        _lib.check(l.omgx_pixel_gather(*batch._records(host=False), H, W, p(t), p(inst), -1, p(ws), p(points), hits, sp), "omgx_pixel_gather")
    cloud_ms = timed(clouds, reps, stream)
    assert int(d_begin[-1].item()) == hits
    # the composition: one mesh entry per instance (a ray batch ties rays to meshes), H * W rays each
    I, N = len(instances), H * W
    rays = ops.RayBatch([mesh] * I, [N] * I, chunks=0, device=dev)
    scene_of = np.repeat(np.arange(S), np.diff(begin))
    m = torch.from_numpy(np.ascontiguousarray(instances["m"])).to(dev)                       # [I,12]
    k = torch.from_numpy(np.ascontiguousarray(cameras[scene_of, :4])).to(dev)                 # [I,4]
    pix = torch.arange(N, device=dev, dtype=torch.int64)
    rr, cc = (pix // W).to(torch.float64), (pix % W).to(torch.float64)
    o = torch.empty((I * N, 3), dtype=torch.float64, device=dev)
    d = torch.empty((I * N, 3), dtype=torch.float64, device=dev)
    rt = torch.empty(I * N, dtype=torch.float64, device=dev)
    rf = torch.empty(I * N, dtype=torch.int32, device=dev)
    result = {}
    order = torch.arange(per_scene, device=dev, dtype=torch.int64)[None, :, None]

    def set_up():
        dx = (cc[None, :] - k[:, 2:3]) / k[:, 0:1]                                            # [I,N]
        dy = (rr[None, :] - k[:, 3:4]) / k[:, 1:2]
        ov, dv = o.view(I, N, 3), d.view(I, N, 3)
        for a in range(3):
            ov[:, :, a] = m[:, 4 * a + 3: 4 * a + 4]
            dv[:, :, a] = (m[:, 4 * a: 4 * a + 1] * dx + m[:, 4 * a + 1: 4 * a + 2] * dy) + m[:, 4 * a + 2: 4 * a + 3]

    def cast_and_min():
        ops.mesh_raycast_batch(rays, o, d, out=(rt, rf))
        per = rt.view(S, per_scene, N)
        best = torch.min(per, dim=1).values
        # torch.min does not promise which index it returns for a tie; the camera's rule is the lowest, so take it explicitly
        arg = torch.where(per == best[:, None, :], order, per_scene).min(dim=1).values
        result["t"], result["inst"] = best, torch.where(torch.isinf(best), torch.full_like(arg, -1), arg)

    def composition():
        set_up()
        cast_and_min()
    set_up()
    comp_ms = timed(cast_and_min, reps, stream)
    comp_all_ms = timed(composition, reps, stream)
    same_t = bool(torch.equal(result["t"].view(torch.int64), t.view(S, N).view(torch.int64)))
    same_inst = bool(torch.equal(result["inst"].to(torch.int32), inst.view(S, N)))
    faces = int(len(mesh[1]))
    active = 0
    for s in range(S):
        dx, dy = cam.pixel_directions(cameras[s], H, W)
        active += sum(int(cam.instance_active(r, dx, dy).sum()) for r in instances[begin[s]: begin[s + 1]])
    return {
        "shape": name, "scenes": S, "H": H, "W": W, "instances_per_scene": per_scene, "faces_per_instance": faces,
        "pixel_instance_pairs": I * N, "pixel_instance_face_tests_without_cull": I * N * faces,
        "share_of_pairs_the_cull_removes": 1.0 - active / (I * N), "hit_pixels": hits, "share_of_pixels_hit": hits / (S * N),
        "render_cull_ms": ms[True][0], "render_cull_runs_ms": ms[True][1], "render_no_cull_ms": ms[False][0], "render_no_cull_runs_ms": ms[False][1],
        "clouds_three_launches_ms": cloud_ms[0], "clouds_runs_ms": cloud_ms[1],
        "composition_chunks_automatic": rays.chunks, "composition_raycast_and_min_ms": comp_ms[0], "composition_raycast_and_min_runs_ms": comp_ms[1],
        "composition_with_ray_setup_ms": comp_all_ms[0], "composition_with_ray_setup_runs_ms": comp_all_ms[1],
        "render_cull_vs_composition": comp_ms[0] / ms[True][0], "render_no_cull_vs_composition": comp_ms[0] / ms[False][0],
        "cull_equals_no_cull_bit_for_bit": same_cull, "composition_t_equals_render_bit_for_bit": same_t,
        "composition_instance_equals_render": same_inst,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "depth_camera_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_camera_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    mesh = MC.icosphere(a.level, 0.06)
    shapes = [("a_one_scene_640x480", 1, 480, 640, 600.0, 10), ("b_100_scenes_160x120", 100, 120, 160, 150.0, 5)]
    if a.small:
        shapes = [("a_small", 1, 48, 64, 60.0, 10), ("b_small", 3, 24, 32, 30.0, 5)]
    res = {"device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "shapes": [measure(s[0], mesh, *s[1:], a.reps, dev, stream) for s in shapes]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in s.items() if not k.endswith("_runs_ms")} for s in res["shapes"]]))


if __name__ == "__main__":
    main()
