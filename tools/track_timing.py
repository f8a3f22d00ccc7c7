"""Timing of camera tracking (omgx_track_cameras) on one GPU, beside what a caller had before it.

  python tools/track_timing.py [--reps 15] [--out profiles/track_timing.json]

The scene: a slab, a sphere and a box as volumes at 1 cm in a scene table; the model is ops.render_volumes at the announced camera,
the live frame the same renderer at a camera moved by up to 30 mm and 8 degrees (seeded), its normals from ops.depth_normals.
  (a) one 640 x 480 view;   (b) 100 views of 160 x 120;   each at stride 1 and 4.
For each:
  whole    omgx_track_cameras with K = 12 through the C ABI, everything already on the device, between two HIP events on the
           stream: the median and the range of `reps` calls after three warm-up calls (27 launches a call)
  turn     the same with K = 0: init, ONE pass and ONE step (the ABI does not expose the kernels one by one; the step's share is
           what remains of a turn at a stride that leaves one chunk of pixels: `turn_one_chunk`)
  launch   the same with K = 0 on a 1 x 1 image: what three launches and the clock cost
  torch    a composition of ONE pass as a caller would write it: projection, gathers, elementwise operations, torch.sum
  numpy    the specification on the CPU (tracking.track_cameras, K = 12), one run, a host clock; the device's poses and stats are
           compared with it bit for bit in every timed case
  register ops.register_clouds of the live sphere's cloud against the sphere's single volume, the alternative a caller had: the
           error of the sphere's centre in the camera's frame, beside the tracked camera's error
The pass's float64 VALU-issue bound as DESIGN.md section 5.2 prices it: PIXEL_F64 float64 instructions per VALID inlier pixel
(counted in the ISA of csrc/omg_track.hip) of 4 issue cycles each, two divisions of 10 steps and a v_rcp_f64 of 8, per wave of 64
pixels on one of 1024 SIMDs at 2.4 GHz.
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

from omg_planner_amd import _lib, camera, ops, registration, scenes, tracking  # noqa: E402

# per used pixel that is an inlier: the ray (2 divisions), P (2), Q (12), the projection (2 divisions, 6), M and e (2 divisions, 5), dd (5),
# the normal test (20), res (5), g (15), j (9), 28 products and 28 additions
PIXEL_F64 = 2 + 12 + 6 + 5 + 5 + 20 + 5 + 15 + 9 + 56
PIXEL_DIVISIONS = 6
PIXEL_CYCLES = PIXEL_F64 * 4 + PIXEL_DIVISIONS * (10 * 4 + 8)
SIMDS, CLOCK_HZ = 1024, 2.4e9
DELTA, TAU, NORMAL_COS = 0.01, (0.012, 0.0, 0.02), 0.15
ARGS = dict(dist_max=0.05, cos_min=0.7, lambda0=2.0 ** -10, step_tol=1e-6)
EYE, TARGET = np.array([0.55, -0.45, 0.5]), np.array([0.0, 0.0, 0.03])
SPHERE_AT = np.array([0.0, 0.0, 0.07])


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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    z = (np.asarray(target, np.float64) - eye) / np.linalg.norm(np.asarray(target, np.float64) - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    w = np.eye(4)
    w[:3, 0], w[:3, 1], w[:3, 2], w[:3, 3] = x, np.cross(z, x), z, eye
    return np.linalg.inv(w)


def moved(cfw, seed):
    rng = np.random.default_rng(seed)
    mm, deg = 30.0 * rng.random(), 8.0 * rng.random()
    d, axis = rng.normal(size=3), rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(np.deg2rad(deg)) * K + (1 - np.cos(np.deg2rad(deg))) * (K @ K)
    M[:3, 3] = 1e-3 * mm * d / np.linalg.norm(d)
    return M @ cfw


def camera_error(cfw, truth):
    a, b = np.linalg.inv(cfw), np.linalg.inv(truth)
    cosine = 0.5 * (np.trace(a[:3, :3].T @ b[:3, :3]) - 1.0)
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), float(np.rad2deg(np.arccos(np.clip(cosine, -1.0, 1.0))))


def table_of(V, dev):
    at = lambda x, y, z: np.array([[1.0, 0, 0, x], [0, 1.0, 0, y], [0, 0, 1.0, z], [0, 0, 0, 1.0]])
    made = [scenes.Scene([scenes.SceneObject("slab", at(0.0, 0.0, -0.02), scenes.box_sdf((0.30, 0.25, 0.02), (72, 60, 16), DELTA)),
                          scenes.SceneObject("sphere", at(*SPHERE_AT), scenes.sphere_sdf(0.07, (24, 24, 24), DELTA)),
                          scenes.SceneObject("box", at(0.17, -0.1, 0.05), scenes.box_sdf((0.04, 0.06, 0.05), (20, 24, 22), DELTA))], 1) for _ in range(V)]
    return ops.DeviceScenes.from_scenes(made, device=dev)


def torch_pass(zl, nl, zm, nm, k, T, stride, dist2, cos_min):
    """ONE pass as a caller would write it -> [V,29] (28 sums, the count); torch's reductions, so the last bits differ."""
    V, H, W = zl.shape
    dev = zl.device
    r, c = torch.meshgrid(torch.arange(0, H, stride, device=dev), torch.arange(0, W, stride, device=dev), indexing="ij")
    r, c = r.reshape(-1), c.reshape(-1)
    z, m = zl[:, r, c], nl[:, r, c]
    fx, fy, cx, cy = (k[:, i, None] for i in range(4))
    R, t = T.view(V, 3, 4)[:, :, :3], T.view(V, 3, 4)[:, :, 3]
    valid = (z > 0) & (z < float("inf")) & ((m * m).sum(-1) > 0)
    P = torch.stack([(c[None] - cx) / fx * z, (r[None] - cy) / fy * z, z], -1)
    Q = P @ R.transpose(1, 2) + t[:, None]
    ua, ub = fx * (Q[..., 0] / Q[..., 2]) + cx + 0.5, fy * (Q[..., 1] / Q[..., 2]) + cy + 0.5
    ok = valid & (Q[..., 2] > 0) & (ua >= 0) & (ua < W) & (ub >= 0) & (ub < H)
    cm, rm = torch.where(ok, ua, torch.zeros_like(ua)).long(), torch.where(ok, ub, torch.zeros_like(ub)).long()
    v = torch.arange(V, device=dev)[:, None]
    zq, n = zm[v, rm, cm], nm[v, rm, cm]
    M = torch.stack([(cm - cx) / fx * zq, (rm - cy) / fy * zq, zq], -1)
    e = Q - M
    inl = ok & (zq > 0) & (zq < float("inf")) & ((n * n).sum(-1) > 0) & ((e * e).sum(-1) <= dist2) & (((m @ R.transpose(1, 2)) * n).sum(-1) >= cos_min)
    res = (n * e).sum(-1)
    g = n @ R
    j = torch.cat([g, torch.cross(P, g, dim=-1)], -1)
    w = inl.to(torch.float64)
    jj = (j[..., :, None] * j[..., None, :])[..., torch.triu(torch.ones(6, 6, dtype=torch.bool, device=dev))]
    terms = torch.cat([jj, j * res[..., None], (res * res)[..., None]], -1) * w[..., None]
    terms[..., 27] += (valid & ~inl).to(torch.float64) * dist2
    return torch.cat([terms.nan_to_num(0.0).sum(1), w.sum(1, keepdim=True)], 1)


def measure(name, V, H, W, f, reps, dev, stream):
    l, vp = _lib.lib(), C.c_void_p
    p = lambda x: vp(x.data_ptr())
    table = table_of(V, dev)
    cfw = look_at(EYE, TARGET)
    truth = np.stack([moved(cfw, 1 + v) for v in range(V)])
    intr = np.tile((f, f, 0.5 * (W - 1), 0.5 * (H - 1)), (V, 1))
    rows = lambda cams: np.stack([camera.camera_rows(intr[v], cams[v]) for v in range(V)])
    march = dict(min_step=DELTA / 16, max_steps=256, want_normals=True)
    zm, _, nm, _ = ops.render_volumes(table, rows(np.stack([cfw] * V)), H, W, **march)
    live, inst, _, _ = ops.render_volumes(table, rows(truth), H, W, **march)
    live = torch.where(torch.isfinite(live), live, torch.zeros_like(live))
    nl, zl, _, _ = ops.depth_normals(live, intr, TAU, NORMAL_COS)
    d_k, p0 = torch.from_numpy(intr).to(dev), torch.from_numpy(np.tile(tracking.IDENTITY, (V, 1))).to(dev)
    poses, stats = torch.empty((V, 12), dtype=torch.float64, device=dev), torch.empty((V, 8), dtype=torch.float64, device=dev)
    host = [x.cpu().numpy() for x in (zl, nl, zm, nm)]
    res = {"shape": name, "views": V, "H": H, "W": W, "runs": []}
    for stride in (1, 4):
        need = ops.track_workspace_bytes(V, H, W, stride)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def call(K, s=stride, ws=ws, need=need):
            _lib.check(l.omgx_track_cameras(p(d_k), vp(intr.ctypes.data), p(zl), p(nl), p(zm), p(nm), V, H, W, s, p(p0), ARGS["dist_max"], ARGS["cos_min"],
                                            ARGS["lambda0"], ARGS["step_tol"], K, p(ws), need, p(poses), p(stats), vp(stream.cuda_stream)), "omgx_track_cameras")
        whole = by_events(lambda: call(12), reps, stream)
        got = (poses.cpu().numpy(), stats.cpu().numpy())
        turn = by_events(lambda: call(0), reps, stream)
        one_chunk = max(stride, -(-max(H, W) // 40))  # at most 40 x 40 used pixels: one chunk
        need1 = ops.track_workspace_bytes(V, H, W, one_chunk)
        turn1 = by_events(lambda: call(0, one_chunk, ws, need1), reps, stream)
        Hu, Wu = tracking.used_grid(H, W, stride)
        tp = by_events(lambda: torch_pass(zl, nl, zm, nm, d_k, p0, stride, ARGS["dist_max"] ** 2, ARGS["cos_min"]), max(reps // 3, 3), stream, warm_up=1)
        t0 = time.perf_counter()
        want = tracking.track_cameras(*host, intr, None, stride=stride, max_passes=12, **ARGS)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        errs = [camera_error(tracking.compose(got[0][v], cfw), truth[v]) for v in range(V)]
        valid = tracking.valid_pixels(host[0], host[1], stride)
        bound_ms = float(valid.sum()) / 64.0 * PIXEL_CYCLES / (SIMDS * CLOCK_HZ) * 1e3
        pass_ms = max(turn["median_ms"] - turn1["median_ms"], 0.0)
        res["runs"].append({"stride": stride, "used_pixels": Hu * Wu, "valid_pixels": int(valid.sum()), "chunks": -(-Hu * Wu // tracking.PIXELS_PER_WORKGROUP),
                            "whole_K12": whole, "turn_K0": turn, "turn_one_chunk": dict(turn1, stride=one_chunk),
                            "pass_over_one_chunk_ms": pass_ms, "valu_bound_pass_ms": bound_ms, "bound_share_of_pass": bound_ms / pass_ms if pass_ms > 0 else None,
                            "torch_one_pass": tp, "torch_pass_over_turn": tp["median_ms"] / turn["median_ms"], "numpy_K12_ms": numpy_ms,
                            "numpy_over_whole": numpy_ms / whole["median_ms"],
                            "device_equals_numpy": bool(np.array_equal(got[0].view(np.int64), want[0].view(np.int64)) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))),
                            "trials": [int(x) for x in got[1][:, 5]][:8], "start_error_mm_deg": [camera_error(cfw, truth[v]) for v in range(min(V, 4))],
                            "tracked_error_mm_max": max(e[0] for e in errs) * 1e3, "tracked_error_mm_median": statistics.median(e[0] for e in errs) * 1e3,
                            "tracked_error_deg_max": max(e[1] for e in errs)})
    # the alternative a caller had: the sphere's pixels of the live frame as a cloud in the announced camera's world, registered
    # against the sphere's volume; what it can give is the sphere's centre, in the camera's frame
    wfc = np.linalg.inv(cfw)
    clouds, ranges = [], [0]
    zl_h, inst_h = host[0], inst.cpu().numpy()
    for v in range(V):
        r, c = np.nonzero((inst_h[v] == 1) & (zl_h[v] > 0))
        z = zl_h[v][r, c]
        pc = np.stack([(c - intr[v, 2]) / intr[v, 0] * z, (r - intr[v, 3]) / intr[v, 1] * z, z], -1)
        clouds.append(pc @ wfc[:3, :3].T + wfc[:3, 3])
        ranges.append(ranges[-1] + len(pc))
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    pairs = [(v, 1) for v in range(V)]
    rr = np.stack([ranges[:-1], ranges[1:]], -1)
    start = registration.pose_rows(np.stack([np.block([[np.eye(3), SPHERE_AT[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]])] * V))
    reg = by_events(lambda: ops.register_clouds(table, pairs, start, pts, rr, max_passes=12), reps, stream)
    rp, _ = ops.register_clouds(table, pairs, start, pts, rr, max_passes=12)
    rp = rp.cpu().numpy()
    # the sphere's centre in the live camera's frame: the truth, and what registration says through the announced camera
    cerr = [float(np.linalg.norm((cfw[:3, :3] @ rp[v].reshape(3, 4)[:, 3] + cfw[:3, 3]) - (truth[v][:3, :3] @ SPHERE_AT + truth[v][:3, 3]))) for v in range(V)]
    res["register_clouds_K12"] = dict(reg, points=int(len(pts)), centre_error_mm_max=max(cerr) * 1e3, centre_error_mm_median=statistics.median(cerr) * 1e3,
                                      note="a sphere fixes a translation only: no rotation comes out of it")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "track_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    shapes = [("a_one_view_640x480", 1, 480, 640, 600.0), ("b_100_views_160x120", 100, 120, 160, 150.0)]
    if a.small:
        shapes = [("a_small", 1, 120, 160, 150.0), ("b_small", 4, 60, 80, 75.0)]
    one = [torch.ones((1, 1, 1), dtype=torch.float64, device=dev), torch.zeros((1, 1, 1, 3), dtype=torch.float64, device=dev)]
    k1 = np.array([[1.0, 1.0, 0.0, 0.0]])
    launch = by_events(lambda: ops.track_cameras(one[0], None, one[0], one[1], k1, max_passes=0), a.reps, stream)
    res = {"device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "issue_cycles_per_wave_and_pixel": PIXEL_CYCLES, "one_pixel_turn_through_the_wrapper": launch,
           "shapes": [measure(s[0], *s[1:], a.reps, dev, stream) for s in shapes]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    brief = lambda d: {k: (brief(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "runs_ms"}
    print(json.dumps({"one_pixel_turn": brief(launch), "shapes": [{**{k: v for k, v in s.items() if k != "runs"}, "runs": [brief(r) for r in s["runs"]],
                                                                   "register_clouds_K12": brief(s["register_clouds_K12"])} for s in res["shapes"]]}))


if __name__ == "__main__":
    main()
