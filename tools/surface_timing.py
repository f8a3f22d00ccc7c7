"""Timing of surface extraction (omgx_surface_count, omgx_surface_gather; ops.surface_meshes, DeviceScenes.object_surfaces) on one GPU.

  python tools/surface_timing.py [--reps 7] [--out profiles/surface_timing.json]
  make -C omg-planner_amd/csrc BUILD=build_surf1 OUT=libomg_hip_surf1.so EXTRA=-DOMGX_SURFACE_ONE_LOAD=1
  python tools/surface_timing.py --lib omg-planner_amd/csrc/libomg_hip_surf1.so --count-only --out profiles/surface_timing_one_load.json

Three shapes:
  (a) one 64^3 sphere volume (voxel centres, delta 0.6 / 64, radius 0.2);
  (b) 100 such volumes (radii 0.15 .. 0.25) in ONE launch, and the same 100 as 100 single launches;
  (c) the 5 objects x 100 scenes of the benchmark's scene table (scenes.make_tabletop_scene(s, num_objects=4, grid=64), a private
      copy of every volume as bench.py builds it) through DeviceScenes.object_surfaces, and the same table with shared grids.
For each: the count step (k_surface_count + k_surface_scan) and the gather step (k_surface_gather) between two HIP events on the
stream, records, workspace and output pools on the device before the first event; the whole ops.surface_meshes /
object_surfaces call with its allocation and its one download, by a host clock around a call that ends in a synchronise; and
scenes.surface_nets on the CPU for the distinct volumes.  Each device figure is the median of `reps` runs after three warm-up
runs.  The JSON also gives the bytes the two steps must move (every sample read once per step, the rank byte written by count,
the vertices and faces written by gather) over their time, and whether the device meshes equal the specification's.
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

from omg_planner_amd import _lib, ops, scenes as sc  # noqa: E402
from omg_planner_amd.config import Config  # noqa: E402


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


def host_timed(fn, reps, warm_up=2):
    for _ in range(warm_up):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), ms


class Steps:
    """The two entry points on prepared buffers: records, workspace, counts and output pools allocated once."""

    def __init__(self, pool, layouts, level, dev):
        self.l, self.pool, self.level, self.dev = _lib.lib(), pool, float(level), dev
        self.rec = ops.surface_records(layouts)
        self.M = len(self.rec)
        vp = C.c_void_p
        self.ws = torch.empty(int(self.l.omgx_surface_workspace_bytes(C.cast(self.rec, vp), self.M)), dtype=torch.uint8, device=dev)
        self.counts = torch.empty((self.M, 4), dtype=torch.int32, device=dev)
        self.d_rec = self._upload()
        self.count()
        h = self.counts.cpu().numpy().astype(np.int64)
        vb, fb = np.concatenate([[0], np.cumsum(h[:, 0])]), np.concatenate([[0], np.cumsum(h[:, 1])])
        for m, r in enumerate(self.rec):
            r.vert_begin, r.vert_count, r.face_begin, r.face_count = int(vb[m]), int(h[m, 0]), int(fb[m]), int(h[m, 1])
        self.d_rec = self._upload()
        self.verts = torch.empty((int(vb[-1]), 3), dtype=torch.float64, device=dev)
        self.faces = torch.empty((int(fb[-1]), 3), dtype=torch.int32, device=dev)
        self.h = h

    def _upload(self):
        return torch.from_numpy(np.frombuffer(self.rec, np.uint8).copy()).to(self.dev)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def count(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_surface_count(vp(self.pool.data_ptr()), self.pool.numel(), vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M,
                                             self.level, vp(self.ws.data_ptr()), vp(self.counts.data_ptr()), self._stream()), "omgx_surface_count")

    def gather(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_surface_gather(vp(self.pool.data_ptr()), self.pool.numel(), vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M,
                                              self.level, vp(self.ws.data_ptr()), vp(self.verts.data_ptr()), self.verts.shape[0],
                                              vp(self.faces.data_ptr()), self.faces.shape[0], self._stream()), "omgx_surface_gather")


COUNT_ONLY = False  # --count-only: a measurement build whose meshes are wrong (csrc/Makefile `variants`)


def measure(name, pool, layouts, level, reps, dev, stream, grids, whole=None):
    """grids: the distinct host volumes [(data, origin, delta)] the specification is timed on (and compared with, by position in
    `layouts` when there are as many)."""
    st = Steps(pool, layouts, level, dev)
    count_ms = timed(st.count, reps, stream)
    if COUNT_ONLY:
        return {"shape": name, "volumes": len(layouts), "samples": sum(int(np.prod(l[3])) for l in layouts), "count_ms": count_ms[0],
                "count_runs_ms": count_ms[1]}
    gather_ms = timed(st.gather, reps, stream)
    whole = whole or (lambda: ops.surface_meshes(pool, layouts, level))
    whole_ms = host_timed(whole, reps)
    t0 = time.perf_counter()
    spec = [sc.surface_nets(d, o, dl, "centre", level) for d, o, dl in grids]
    spec_ms = (time.perf_counter() - t0) * 1e3
    same = None
    if len(grids) == len(layouts):
        hv, hf = st.verts.cpu().numpy(), st.faces.cpu().numpy()
        vb, fb = np.concatenate([[0], np.cumsum(st.h[:, 0])]), np.concatenate([[0], np.cumsum(st.h[:, 1])])
        same = all(np.array_equal(hv[vb[m]: vb[m + 1]].view(np.int64), spec[m][0].view(np.int64)) and np.array_equal(hf[fb[m]: fb[m + 1]], spec[m][1])
                   and int(st.h[m, 2]) == spec[m][2] for m in range(len(grids)))
    samples = sum(int(np.prod(l[3])) for l in layouts)
    V, F = int(st.h[:, 0].sum()), int(st.h[:, 1].sum())
    count_bytes, gather_bytes = samples * 4 + st.ws.numel(), samples * 4 + V * 24 + F * 12
    return {
        "shape": name, "volumes": len(layouts), "samples": samples, "vertices": V, "faces": F, "open_edges": int(st.h[:, 2].sum()),
        "workspace_bytes": int(st.ws.numel()),
        "count_ms": count_ms[0], "count_runs_ms": count_ms[1], "gather_ms": gather_ms[0], "gather_runs_ms": gather_ms[1],
        "whole_call_with_download_ms": whole_ms[0], "whole_call_runs_ms": whole_ms[1],
        "count_bytes_needed": count_bytes, "count_GB_per_s": count_bytes / count_ms[0] * 1e-6,
        "gather_bytes_needed": gather_bytes, "gather_GB_per_s": gather_bytes / gather_ms[0] * 1e-6,
        "specification_cpu_ms": spec_ms, "specification_volumes": len(grids), "device_equals_specification": same,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "surface_timing.json"))
    ap.add_argument("--lib", help="another build of the library, e.g. omg-planner_amd/csrc/libomg_hip_surf1.so (OMGX_SURFACE_ONE_LOAD)")
    ap.add_argument("--count-only", action="store_true", help="time the count step alone (for a build whose meshes are wrong)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_timing.py needs a GPU")
    global COUNT_ONLY
    COUNT_ONLY = bool(a.count_only)
    if a.lib:
        _lib.LIB_PATH = Path(a.lib).resolve()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    n, many, S = (16, 5, 3) if a.small else (64, 100, 100)
    shape, delta = (n, n, n), 0.6 / n
    grids = [sc.sphere_sdf(r, shape, delta) for r in np.linspace(0.15, 0.25, many)]
    one = sc.sphere_sdf(0.2, shape, delta)
    host = lambda gs: [(g.data, g.min_coords, g.delta) for g in gs]
    out = []
    pool1 = torch.from_numpy(one.data.ravel()).to(dev)
    out.append(measure("a_one_64^3_sphere", pool1, [(one.min_coords, one.delta, "centre", shape, 0)], 0.0, a.reps, dev, stream, host([one])))
    poolN = torch.from_numpy(np.concatenate([g.data.ravel() for g in grids])).to(dev)
    layouts = [(g.min_coords, g.delta, "centre", shape, m * n ** 3) for m, g in enumerate(grids)]
    out.append(measure("b_100_volumes_one_launch", poolN, layouts, 0.0, a.reps, dev, stream, host(grids)))
    if not COUNT_ONLY:
        singles = [Steps(poolN, [l], 0.0, dev) for l in layouts]
        c_ms = timed(lambda: [s.count() for s in singles], a.reps, stream)
        g_ms = timed(lambda: [s.gather() for s in singles], a.reps, stream)
        w_ms = host_timed(lambda: [ops.surface_meshes(poolN, [l], 0.0) for l in layouts], a.reps)
        out.append({"shape": "b_100_volumes_100_single_launches", "volumes": many, "count_ms": c_ms[0], "count_runs_ms": c_ms[1], "gather_ms": g_ms[0],
                    "gather_runs_ms": g_ms[1], "whole_call_with_download_ms": w_ms[0], "whole_call_runs_ms": w_ms[1]})
    scenes = [sc.make_tabletop_scene(s, num_objects=4, grid=n) for s in range(S)]
    for share in (False, True):
        table = ops.DeviceScenes.from_scenes(scenes, Config().layer_kwargs(), device=dev, share_grids=share)
        rec = table.host_objects
        idx = list(range(len(rec))) if not share else sorted({int(o): k for k, o in reversed(list(enumerate(rec["grid_offset"])))}.values())
        layouts = [(rec["lo"][i].astype(np.float64), float(rec["delta"][i]), "centre", tuple(int(d) for d in rec["dim"][i]), int(rec["grid_offset"][i]))
                   for i in idx]
        distinct, seen = [], set()
        for s_ in scenes:
            for ob in s_.objects:
                if id(ob.sdf.data) not in seen:
                    seen.add(id(ob.sdf.data))
                    distinct.append((ob.sdf.data, np.float32(ob.sdf.min_coords).astype(np.float64), float(np.float32(ob.sdf.delta))))
        r = measure(f"c_bench_table_{S}_scenes_x_5_objects_" + ("shared_grids" if share else "private_grids"), table.pool, layouts, 0.0, a.reps, dev,
                    stream, distinct, whole=lambda: table.object_surfaces())
        r["objects"] = len(rec)
        out.append(r)
        del table
    res = {"library": Path(_lib.LIB_PATH).name, "device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small), "shapes": out}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in s.items() if not k.endswith("_runs_ms")} for s in out]))


if __name__ == "__main__":
    main()
