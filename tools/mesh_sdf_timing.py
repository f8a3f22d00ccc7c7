"""Timing of the mesh-to-volume kernel (omgx_mesh_sdf) on one GPU.

  python tools/mesh_sdf_timing.py [--grid 64] [--level 4] [--objects 100] [--reps 7] [--out profiles/mesh_sdf_timing.json]

An icosphere of 20 * 4^level faces (level 4: 5120) on a grid^3 volume:
  (a) one volume, one launch;
  (b) `objects` volumes of that size in ONE batched launch;
  (c) the same volumes as `objects` single launches, one after the other on one stream.
Each figure is the median of `reps` runs after a warm-up, between two HIP events on the stream, of the launches alone: meshes,
records and the output buffer are on the device before the first event (what ops.mesh_sdf adds on the host — cleaning the
mesh, three small uploads — is reported separately as wall time around the whole wrapper call, synchronised).  Beside them the
host specification (scenes.mesh_sdf, plain numpy, one thread) on a `host_grid`^3 volume of the same mesh, scaled by node count.
No reference time exists: the reference makes volumes with an external program that is not part of it.
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
from omg_planner_amd import scenes as sc  # noqa: E402
from tests import mesh_cases as MC  # noqa: E402


def timed(fn, reps, stream):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--objects", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-grid", type=int, default=16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_sdf_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_sdf_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    v, f = MC.icosphere(a.level, 0.06)
    G, M = a.grid, a.objects
    delta = 0.16 / G
    origin, dims = np.full(3, -0.08), (G, G, G)

    rng = np.random.RandomState(0)
    meshes = [(v * rng.uniform(0.9, 1.1), f) for _ in range(M)]  # objects of one size, not one object

    def prepared(batch, offsets):
        """A batch pooled and on the device, volume m at element offsets[m] of the output -> (records, their three tensors)."""
        mp = ops.MeshPool(batch, drop_zero_area=True)
        for m, off in enumerate(offsets):
            mp.set_volume(m, origin, delta, "centre", dims, off)
            mp.rec[m].first_workgroup = m * -(-G ** 3 // _lib.MESH_SDF_NODES_PER_WORKGROUP)
        return (mp.rec, *mp.upload(dev))

    def launch(rec, d_v, d_f, d_rec, out):
        _lib.check(_lib.lib().omgx_mesh_sdf(d_v.data_ptr(), d_f.data_ptr(), d_rec.data_ptr(), C.cast(rec, C.c_void_p), len(rec), out.data_ptr(),
                                           stream.cuda_stream), "omgx_mesh_sdf")

    # (a)
    one, out1 = prepared(meshes[:1], [0]), torch.empty(G ** 3, dtype=torch.float32, device=dev)
    a_ms, a_all = timed(lambda: launch(*one, out1), a.reps, stream)
    # (b)
    many, outM = prepared(meshes, [m * G ** 3 for m in range(M)]), torch.empty(M * G ** 3, dtype=torch.float32, device=dev)
    b_ms, b_all = timed(lambda: launch(*many, outM), a.reps, stream)
    # (c): one record set per object, each a batch of one at its own offset
    singles = [prepared([meshes[m]], [m * G ** 3]) for m in range(M)]
    outC = torch.empty_like(outM)

    def all_single():
        for single in singles:
            launch(*single, outC)
    c_ms, c_all = timed(all_single, a.reps, stream)
    same = bool(torch.equal(outC.view(torch.int32), outM.view(torch.int32)))
    # the wrapper as a user calls it (host work + uploads + launch), wall clock
    wall = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.mesh_sdf(v, f, delta, 0, "centre", origin, dims, device=dev)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    # the host specification on a small grid, scaled by node count
    H = a.host_grid
    t0 = time.perf_counter()
    host = sc.mesh_sdf(v, f, 0.16 / H, 0, "centre", origin, (H, H, H))
    host_s = time.perf_counter() - t0
    pairs = G ** 3 * len(f)
    res = {
        "device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "faces": int(len(f)), "grid": [G, G, G], "objects": M, "reps": a.reps,
        "pairs_per_volume": pairs,
        "a_one_volume_ms": a_ms, "a_runs_ms": a_all, "a_pairs_per_s": pairs / (a_ms * 1e-3),
        "b_batched_ms": b_ms, "b_runs_ms": b_all, "b_ms_per_volume": b_ms / M, "b_pairs_per_s": M * pairs / (b_ms * 1e-3),
        "c_single_launches_ms": c_ms, "c_runs_ms": c_all, "c_ms_per_volume": c_ms / M,
        "b_equals_c_bit_for_bit": same,
        "wrapper_wall_ms_one_volume": statistics.median(wall[1:]),
        "host_spec_grid": [H, H, H], "host_spec_s": host_s, "host_spec_scaled_to_grid_s": host_s * (G / H) ** 3,
        "host_spec_threads": 1, "inside_nodes_host_grid": int((host.data < 0).sum()),
    }
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_runs_ms")}))


if __name__ == "__main__":
    main()
