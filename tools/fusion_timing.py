"""Timing of depth fusion (omgx_carve_views, omgx_distance_transform; ops.fuse_views) on one GPU.

  python tools/fusion_timing.py [--reps 7] [--out profiles/fusion_timing.json]

Two shapes, a slab and seven boxes rendered by ops.render_depth:
  (a) one 75 x 75 x 50 grid at 2 cm (the workspace of the reference's PointEnv) from three 640 x 480 views;
  (b) 100 volumes of 64^3 at 1 cm from three 160 x 120 views each (300 cameras around the same boxes), in ONE set of launches,
      and the same 100 as 100 single calls.
For each: the carve launch and the three transform launches apart, between two HIP events on the stream, with records, states,
workspace and pool on the device before the first event; the median of `reps` runs after three warm-up runs, and every run.
The transform's bytes (per node 1 B of state read, a 4-byte intermediate written and read twice, 4 B written) over HBM peak,
and its LDS reads (3 passes x (2 radius + 1) words per node) over the LDS read rate: the larger is the bound that applies.
For cost only, what the tree does today for the same observation: ops.pixel_clouds + ops.point_cloud_sdf with 3 072 drawn points
(one warm-up run; shape (b) half the repeats) and with the whole cloud (ONE run of one call, no warm-up: not a median), and
scipy's distance_transform_edt of both masks on the CPU.  The outputs of the two paths differ:
the fused volume is signed, knows what no camera saw, and measures to voxel centres (at most sqrt(3)/2 delta coarser than
the distance to the true points); point_cloud_sdf is unsigned and exact to its points.
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

from omg_planner_amd import _lib, camera, fusion, ops  # noqa: E402

HBM_PEAK, LDS_READ_B32 = 8.0e12, 75e12  # bytes per second: HBM3E's specification; ds_read_b32 with every CU streaming


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


def box(half, centre):
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * np.asarray(half) + np.asarray(centre)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)


def look_at(eye, target):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross([0.0, 0.0, -1.0], z)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
    return np.linalg.inv(m)


def render(meshes, eyes, target, H, W, f, dev):
    """depth [len(eyes),H,W] on the device, the view rows (grid frame = world frame) and the batch."""
    intr = (f, f, (W - 1) / 2, (H - 1) / 2)
    cfw = [look_at(e, target) for e in eyes]
    idx, poses, labels = list(range(len(meshes))), [np.eye(4)] * len(meshes), [1] * len(meshes)
    inst = np.concatenate([camera.instance_records(meshes, idx, poses, labels, c) for c in cfw])
    batch = ops.CameraBatch(meshes, inst, np.arange(len(eyes) + 1) * len(meshes), np.stack([camera.camera_rows(intr, c) for c in cfw]), device=dev)
    t, inst_img, _ = ops.render_depth(batch, H, W, want_face=False)
    return t, inst_img, np.stack([fusion.view_rows(intr, c) for c in cfw]), batch


class Steps:
    """The two entry points on prepared buffers."""

    def __init__(self, volumes, views, ranges, depth, band, near, radius, dev):
        vp = C.c_void_p
        self.l, self.rec, self.M, self.V = _lib.lib(), ops.surface_records(volumes), len(volumes), len(views)
        self.nodes = np.array([int(np.prod(v[3])) for v in volumes], np.int64)
        self.h_begin = np.cumsum(self.nodes) - self.nodes
        self.h_views, self.h_ranges = np.ascontiguousarray(views, np.float64), np.ascontiguousarray(ranges, np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.d_rec = up(np.frombuffer(bytes(self.rec), np.uint8).copy())
        self.d_views, self.d_ranges, self.d_begin = up(self.h_views), up(self.h_ranges), up(self.h_begin)
        self.depth, self.band, self.near, self.radius = depth, float(band), float(near), int(radius)
        self.state = torch.empty(int(self.nodes.sum()), dtype=torch.uint8, device=dev)
        self.pool = torch.empty(max(int(v[4]) + int(n) for v, n in zip(volumes, self.nodes)), dtype=torch.float32, device=dev)
        self.ws = torch.empty(int(self.l.omgx_distance_transform_workspace_bytes(C.cast(self.rec, vp), self.M, self.radius)), dtype=torch.uint8, device=dev)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def carve(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_carve_views(vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M, vp(self.d_views.data_ptr()), vp(self.h_views.ctypes.data),
                                           self.V, vp(self.d_ranges.data_ptr()), vp(self.h_ranges.ctypes.data), vp(self.d_begin.data_ptr()),
                                           vp(self.h_begin.ctypes.data), vp(self.depth.data_ptr()), int(self.depth.shape[1]), int(self.depth.shape[2]),
                                           self.band, self.near, 0, vp(self.state.data_ptr()), self.state.numel(), self._stream()), "omgx_carve_views")

    def transform(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_distance_transform(vp(self.state.data_ptr()), self.state.numel(), vp(self.d_begin.data_ptr()), vp(self.h_begin.ctypes.data),
                                                  vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M, self.radius, 1, vp(self.ws.data_ptr()),
                                                  vp(self.pool.data_ptr()), self.pool.numel(), self._stream()), "omgx_distance_transform")


def scipy_edt_ms(states, dims_list):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.perf_counter()
    at = 0
    for dims in dims_list:
        n = int(np.prod(dims))
        occ = states[at: at + n].reshape(dims) != 0
        at += n
        ndimage.distance_transform_edt(occ), ndimage.distance_transform_edt(~occ)
    return (time.perf_counter() - t0) * 1e3


def measure(name, volumes, views, ranges, depth, band, near, radius, reps, dev, stream):
    st = Steps(volumes, views, ranges, depth, band, near, radius, dev)
    carve_ms = timed(st.carve, reps, stream)
    transform_ms = timed(st.transform, reps, stream)
    nodes = int(st.nodes.sum())
    hbm_bytes, lds_bytes = nodes * 21, nodes * 3 * (2 * radius + 1) * 4
    hbm_ms, lds_ms = hbm_bytes / HBM_PEAK * 1e3, lds_bytes / LDS_READ_B32 * 1e3
    states = st.state.cpu().numpy()
    want = fusion.carve_views(volumes[:1], views, ranges[:1], depth.cpu().numpy(), band, near)
    want_vol = fusion.distance_transform(want, volumes[:1], radius, True)[0]
    n0, off0 = int(st.nodes[0]), int(volumes[0][4])
    same = bool(np.array_equal(states[:n0], want) and np.array_equal(st.pool[off0: off0 + n0].cpu().numpy().view(np.uint32), want_vol.ravel().view(np.uint32)))
    return st, {
        "shape": name, "volumes": len(volumes), "nodes": nodes, "views": len(views), "image": [int(depth.shape[1]), int(depth.shape[2])], "radius": radius,
        "states": {k: int((states == v).sum()) for k, v in (("free", 0), ("surface", 1), ("unknown", 2))},
        "carve_ms": carve_ms[0], "carve_runs_ms": carve_ms[1], "transform_ms": transform_ms[0], "transform_runs_ms": transform_ms[1],
        "transform_hbm_bytes": hbm_bytes, "transform_hbm_bound_ms": hbm_ms, "transform_lds_read_bytes": lds_bytes, "transform_lds_bound_ms": lds_ms,
        "transform_bound": "LDS reads" if lds_ms > hbm_ms else "HBM", "transform_share_of_bound": max(hbm_ms, lds_ms) / transform_ms[0],
        "transform_GB_per_s": hbm_bytes / transform_ms[0] * 1e-6, "workspace_bytes": int(st.ws.numel()),
        "scipy_edt_cpu_ms": scipy_edt_ms(states, [v[3] for v in volumes]), "first_volume_equals_specification": same,
    }


def todays_path(batch, t, inst_img, scenes, resolution, reps, stream, dev, whole: bool):
    """pixel_clouds of every hit + point_cloud_sdf per group of cameras in `scenes` [[camera indices]]: 3 072 drawn points, and the
    whole cloud (one run: it is the brute-force cost the issue is about)."""
    points, begin = ops.pixel_clouds(batch, t, inst_img, -1)
    clouds = [torch.cat([points[int(begin[s]): int(begin[s + 1])] for s in group]).contiguous() for group in scenes]
    gen = torch.Generator(device=dev).manual_seed(0)
    drawn = [c[torch.randint(len(c), (3072,), device=dev, generator=gen)].contiguous() for c in clouds]
    res = {"cloud_points": [int(len(c)) for c in clouds][:4], "pixel_clouds_ms": timed(lambda: ops.pixel_clouds(batch, t, inst_img, -1), reps, stream)[0]}
    res["point_cloud_sdf_3072_points_ms"] = timed(lambda: [ops.point_cloud_sdf(d, resolution) for d in drawn], reps, stream, warm_up=1)[0]
    res["point_cloud_sdf_grid"] = list(ops.point_cloud_sdf(drawn[0], resolution)[0].shape)
    if whole:
        res["point_cloud_sdf_whole_cloud_calls"] = 1
        res["point_cloud_sdf_whole_cloud_ms_per_call"] = timed(lambda: ops.point_cloud_sdf(clouds[0], resolution), 1, stream, warm_up=0)[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--reach", type=float, default=0.23, help="epsilon + clearance the radius is sized for")
    ap.add_argument("--no-whole-cloud", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fusion_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fusion_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(0)
    meshes = [box((0.6, 0.5, 0.02), (0.5, 0.0, -0.02))] + [box(rng.uniform(0.03, 0.08, 3), (0.5 + rng.uniform(-0.25, 0.25), rng.uniform(-0.3, 0.3), 0.08))
                                                           for _ in range(7)]
    band, near, out = 0.02, 0.1, []
    # (a)
    dims, delta, (H, W) = ((15, 15, 10), 0.1, (48, 64)) if a.small else ((75, 75, 50), 0.02, (480, 640))
    t, inst_img, views, batch = render(meshes, [(1.6, 0.0, 0.9), (0.0, 1.0, 0.9), (0.0, -1.0, 0.9)], (0.5, 0.0, 0.1), H, W, 0.8 * W, dev)
    vol = [((-0.25, -0.75, -0.2), delta, "centre", dims, 0)]
    st, r = measure("a_one_75x75x50_at_2cm_three_640x480_views", vol, views, [(0, 3)], t, band, near, fusion.obstacle_radius(a.reach, delta), a.reps, dev, stream)
    r["today"] = todays_path(batch, t, inst_img, [[0, 1, 2]], delta, a.reps, stream, dev, not a.no_whole_cloud)
    out.append(r)
    # (b)
    n, many, (H, W) = (16, 5, (30, 40)) if a.small else (64, 100, (120, 160))
    delta = 0.64 / n
    eyes = [(0.5 + 0.9 * np.cos(u), 0.9 * np.sin(u), rng.uniform(0.5, 0.9)) for u in rng.uniform(0, 2 * np.pi, 3 * many)]
    t, inst_img, views, batch = render(meshes, eyes, (0.5, 0.0, 0.1), H, W, 0.8 * W, dev)
    vols = [((0.18 + rng.uniform(-0.05, 0.05), -0.32 + rng.uniform(-0.05, 0.05), -0.2), delta, "centre", (n, n, n), m * n ** 3) for m in range(many)]
    ranges = [(3 * m, 3) for m in range(many)]
    radius = fusion.obstacle_radius(a.reach, delta)
    st, r = measure(f"b_{many}_volumes_of_{n}^3_at_1cm_three_160x120_views_each_one_set_of_launches", vols, views, ranges, t, band, near, radius, a.reps, dev, stream)
    r["today"] = todays_path(batch, t, inst_img, [[3 * m, 3 * m + 1, 3 * m + 2] for m in range(many)], delta, max(a.reps // 2, 1), stream, dev,
                             not a.no_whole_cloud)
    out.append(r)
    singles = [Steps([v[:4] + (0,)], views, [rg], t, band, near, radius, dev) for v, rg in zip(vols, ranges)]
    c_ms = timed(lambda: [s.carve() for s in singles], a.reps, stream)
    x_ms = timed(lambda: [s.transform() for s in singles], a.reps, stream)
    out.append({"shape": f"b_{many}_volumes_as_{many}_single_calls", "volumes": many, "carve_ms": c_ms[0], "carve_runs_ms": c_ms[1], "transform_ms": x_ms[0],
                "transform_runs_ms": x_ms[1]})
    res = {"library": Path(_lib.LIB_PATH).name, "device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "reach": a.reach, "band": band, "near": near, "hbm_peak_bytes_per_s": HBM_PEAK, "lds_read_b32_bytes_per_s": LDS_READ_B32, "shapes": out}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in s.items() if not k.endswith("_runs_ms")} for s in out]))


if __name__ == "__main__":
    main()
