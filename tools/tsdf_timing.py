"""Timing of weighted TSDF fusion (omgx_tsdf_integrate, omgx_tsdf_states, omgx_tsdf_blend; ops.fuse_tsdf) on one GPU, beside
omgx_carve_views + omgx_distance_transform of the same run.

  python tools/tsdf_timing.py [--reps 7] [--out profiles/tsdf_timing.json]

The two shapes, the scene (a slab and seven boxes rendered by ops.render_depth) and the rule of measurement are
tools/fusion_timing.py's, whose helpers are imported:
  (a) one 75 x 75 x 50 grid at 2 cm from three 640 x 480 views;
  (b) 100 volumes of 64^3 at 1 cm from three 160 x 120 views each, in ONE set of launches, and the same 100 as 100 single calls.
For each: integrate (a first frame, and a further frame with merge, which also reads the pairs: 16 bytes per node), states and
blend apart, and carve and the transform, each between two HIP events on the stream with records, pairs, states, workspace and
pool on the device before the first event; the median of `reps` runs after three warm-up runs, and every run.
The integrate kernel's two bounds: VALU issue, F64_PER_NODE_VIEW half-rate instructions per (node, view) at 4 cycles and
OTHER_PER_NODE_VIEW full-rate ones at 2 cycles per wave instruction and SIMD, and HBM traffic of 16
bytes per node.
"""
from __future__ import annotations

import argparse
import ctypes as C
import importlib.util
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from omg_planner_amd import _lib, fusion, tsdf  # noqa: E402

_spec = importlib.util.spec_from_file_location("fusion_timing", ROOT / "tools" / "fusion_timing.py")
FT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FT)

# The view loop of k_tsdf_integrate as compiled for gfx950, counted in its assembly: 96 VALU instructions per (node, view) that
# updates, 76 of them float64 (16 mul, 16 add, 15 fma, three divisions of 2 div_scale + rcp + div_fmas + div_fixup, 10 compares,
# 2 floor, 2 conversions; the reciprocal priced like the rest: the bound errs low) and 20 at the full rate (selects, moves, the
# pixel's address).
F64_PER_NODE_VIEW, OTHER_PER_NODE_VIEW, SIMDS, CLOCK = 76, 20, 1024, 2.4e9


class Steps(FT.Steps):
    """The three TSDF entry points on the buffers of fusion_timing.Steps."""

    def __init__(self, volumes, views, ranges, depth, trunc, near, radius, dev):
        super().__init__(volumes, views, ranges, depth, 0.02, near, radius, dev)
        self.trunc = float(trunc)
        self.d = torch.zeros(int(self.nodes.sum()), dtype=torch.float32, device=dev)
        self.w = torch.zeros_like(self.d)
        self.tstate = torch.empty(int(self.nodes.sum()), dtype=torch.uint8, device=dev)

    def integrate(self, merge=0):
        vp = C.c_void_p
        _lib.check(self.l.omgx_tsdf_integrate(vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M, vp(self.d_views.data_ptr()), vp(self.h_views.ctypes.data),
                                              self.V, vp(self.d_ranges.data_ptr()), vp(self.h_ranges.ctypes.data), vp(self.d_begin.data_ptr()),
                                              vp(self.h_begin.ctypes.data), vp(self.depth.data_ptr()), int(self.depth.shape[1]), int(self.depth.shape[2]),
                                              None, None, self.trunc, self.near, 8.0, merge, vp(self.d.data_ptr()), vp(self.w.data_ptr()), self.d.numel(),
                                              self._stream()), "omgx_tsdf_integrate")

    def states(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_tsdf_states(vp(self.d.data_ptr()), vp(self.w.data_ptr()), self.d.numel(), vp(self.d_begin.data_ptr()), vp(self.h_begin.ctypes.data),
                                           vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M, 1.0, vp(self.tstate.data_ptr()), self._stream()),
                   "omgx_tsdf_states")

    def tsdf_transform(self):
        self.state, keep = self.tstate, self.state
        self.transform()
        self.state = keep

    def blend(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_tsdf_blend(vp(self.d.data_ptr()), vp(self.w.data_ptr()), self.d.numel(), vp(self.d_begin.data_ptr()), vp(self.h_begin.ctypes.data),
                                          vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M, self.trunc, 1.0, vp(self.pool.data_ptr()), self.pool.numel(),
                                          self._stream()), "omgx_tsdf_blend")


def measure(name, volumes, views, ranges, depth, trunc, near, radius, reps, dev, stream):
    st = Steps(volumes, views, ranges, depth, trunc, near, radius, dev)
    res = {"shape": name, "volumes": len(volumes), "nodes": int(st.nodes.sum()), "views": len(views), "image": [int(depth.shape[1]), int(depth.shape[2])],
           "radius": radius, "trunc": trunc}
    for key, fn in (("carve", st.carve), ("transform", st.transform), ("integrate_first_frame", st.integrate), ("integrate_merge", lambda: st.integrate(1))):
        res[key + "_ms"], res[key + "_runs_ms"] = FT.timed(fn, reps, stream)
    # the volume as a caller gets it, checked against the specification on the first volume, then the rest of the path on it
    st.integrate(0), st.states(), st.tsdf_transform(), st.blend()
    torch.cuda.synchronize()
    n0, off0 = int(st.nodes[0]), int(volumes[0][4])
    want = tsdf.fuse(volumes[:1], views, ranges[:1], depth.cpu().numpy(), trunc, near, radius, True, 1.0, None, 8.0)[0].data
    res["first_volume_equals_specification"] = bool(np.array_equal(st.pool[off0: off0 + n0].cpu().numpy().view(np.uint32), want.ravel().view(np.uint32)))
    states = st.tstate.cpu().numpy()
    res["states"] = {k: int((states == v).sum()) for k, v in (("free", 0), ("surface", 1), ("unknown", 2))}
    for key, fn in (("states", st.states), ("tsdf_transform", st.tsdf_transform), ("blend", st.blend)):
        res[key + "_ms"], res[key + "_runs_ms"] = FT.timed(fn, reps, stream)
    node_views = int(sum(int(n) * int(r[1]) for n, r in zip(st.nodes, ranges)))
    issue_ms = node_views / 64 * (F64_PER_NODE_VIEW * 4 + OTHER_PER_NODE_VIEW * 2) / (SIMDS * CLOCK) * 1e3
    hbm_ms = res["nodes"] * 16 / FT.HBM_PEAK * 1e3
    res.update(node_views=node_views, integrate_valu_issue_bound_ms=issue_ms, integrate_hbm_bound_ms=hbm_ms,
               integrate_share_of_issue_bound=issue_ms / res["integrate_merge_ms"], integrate_share_of_hbm_bound=hbm_ms / res["integrate_merge_ms"],
               tsdf_path_ms=res["integrate_merge_ms"] + res["states_ms"] + res["tsdf_transform_ms"] + res["blend_ms"],
               carve_path_ms=res["carve_ms"] + res["transform_ms"])
    res["tsdf_over_carve_path"] = res["tsdf_path_ms"] / res["carve_path_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--reach", type=float, default=0.23, help="epsilon + clearance the radius is sized for")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tsdf_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(0)
    meshes = [FT.box((0.6, 0.5, 0.02), (0.5, 0.0, -0.02))] + [FT.box(rng.uniform(0.03, 0.08, 3), (0.5 + rng.uniform(-0.25, 0.25), rng.uniform(-0.3, 0.3), 0.08))
                                                              for _ in range(7)]
    near, out = 0.1, []
    # (a)
    dims, delta, (H, W) = ((15, 15, 10), 0.1, (48, 64)) if a.small else ((75, 75, 50), 0.02, (480, 640))
    t, _, views, _ = FT.render(meshes, [(1.6, 0.0, 0.9), (0.0, 1.0, 0.9), (0.0, -1.0, 0.9)], (0.5, 0.0, 0.1), H, W, 0.8 * W, dev)
    vol = [((-0.25, -0.75, -0.2), delta, "centre", dims, 0)]
    out.append(measure("a_one_75x75x50_at_2cm_three_640x480_views", vol, views, [(0, 3)], t, 3 * delta, near, fusion.obstacle_radius(a.reach, delta), a.reps, dev, stream))
    # (b)
    n, many, (H, W) = (16, 5, (30, 40)) if a.small else (64, 100, (120, 160))
    delta = 0.64 / n
    eyes = [(0.5 + 0.9 * np.cos(u), 0.9 * np.sin(u), rng.uniform(0.5, 0.9)) for u in rng.uniform(0, 2 * np.pi, 3 * many)]
    t, _, views, _ = FT.render(meshes, eyes, (0.5, 0.0, 0.1), H, W, 0.8 * W, dev)
    vols = [((0.18 + rng.uniform(-0.05, 0.05), -0.32 + rng.uniform(-0.05, 0.05), -0.2), delta, "centre", (n, n, n), m * n ** 3) for m in range(many)]
    ranges = [(3 * m, 3) for m in range(many)]
    radius = fusion.obstacle_radius(a.reach, delta)
    out.append(measure(f"b_{many}_volumes_of_{n}^3_at_1cm_three_160x120_views_each_one_set_of_launches", vols, views, ranges, t, 3 * delta, near, radius, a.reps, dev, stream))
    singles = [Steps([v[:4] + (0,)], views, [rg], t, 3 * delta, near, radius, dev) for v, rg in zip(vols, ranges)]
    single = {"shape": f"b_{many}_volumes_as_{many}_single_calls", "volumes": many}
    for key, call in (("carve", lambda s: s.carve()), ("transform", lambda s: s.transform()), ("integrate_merge", lambda s: s.integrate(1)),
                      ("states", lambda s: s.states()), ("blend", lambda s: s.blend())):
        single[key + "_ms"], single[key + "_runs_ms"] = FT.timed(lambda: [call(s) for s in singles], a.reps, stream)
    out.append(single)
    res = {"library": Path(_lib.LIB_PATH).name, "device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "reach": a.reach, "near": near, "wmax": 8.0, "f64_instructions_per_node_view": F64_PER_NODE_VIEW, "other_valu_instructions_per_node_view": OTHER_PER_NODE_VIEW, "hbm_peak_bytes_per_s": FT.HBM_PEAK, "shapes": out}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in s.items() if not k.endswith("_runs_ms")} for s in out]))


if __name__ == "__main__":
    main()
