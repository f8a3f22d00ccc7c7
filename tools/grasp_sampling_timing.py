"""Timing of grasp sampling (omgx_mesh_raycast + omgx_grasp_poses) on one GPU.

  python tools/grasp_sampling_timing.py [--level 4] [--rays 4096] [--angles 8] [--objects 100] [--reps 7]
                                        [--out profiles/grasp_sampling_timing.json]

An icosphere of 20 * 4^level faces (level 4: 5120), radius 3 cm, `rays` rays from its surface and `angles` poses per ray:
  (a) one mesh: the ray cast with the automatic number of face chunks, with one chunk forced (what splitting the faces buys),
      and the pose launch;
  (b) `objects` such meshes (scaled 0.9 .. 1.1) in ONE batched ray cast and ONE pose launch;
  (c) the same meshes as `objects` single launches of each kind, one after the other on one stream.
Each figure is the median of `reps` runs after a warm-up, between two HIP events on the stream, around the launches: meshes,
work lists, rays, volumes and outputs are on the device before the first event.  Beside them the wall time of the host
specification (grasps.mesh_raycast and grasps.grasp_poses, plain numpy, one thread) on `host_rays` rays of the same mesh, scaled
by the ray count.  No reference time exists: the reference reads grasps from files.
"""
from __future__ import annotations

import argparse
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
from omg_planner_amd import grasps as G  # noqa: E402
from omg_planner_amd import scenes as sc  # noqa: E402
from tests import mesh_cases as MC  # noqa: E402

CONE = np.deg2rad(15.0)


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


class Prepared:
    """`meshes` with their rays, volumes (mesh_sdf_batch, delta 5 mm) and outputs on the device, for one chunk setting."""

    def __init__(self, meshes, rays, angles, chunks, dev, seed=0):
        rng = np.random.RandomState(seed)
        M = len(meshes)
        self.host = []
        for v, f in meshes:
            p1, _, n1 = G.surface_samples(v, f, rays, rng)
            self.host.append((p1, n1, G.ray_directions(n1, CONE, rng), G.face_normals(v, f)[0]))
        grids, origins, deltas, _ = ops.mesh_sdf_batch(meshes, 0.005, 4, "centre", device=dev)
        self.pool = grids[0].new_empty(0) if M == 0 else torch.cat([g.reshape(-1) for g in grids])
        offs = np.concatenate([[0], np.cumsum([g.numel() for g in grids])])
        layout = [(origins[m], deltas[m], "centre", tuple(grids[m].shape), int(offs[m])) for m in range(M)]
        self.batch = ops.RayBatch(meshes, [rays] * M, chunks=chunks, device=dev, layout=layout)
        up = lambda k: torch.from_numpy(np.ascontiguousarray(np.concatenate([h[k] for h in self.host]))).to(dev)
        self.p1, self.n1, self.d, self.nrm = up(0), up(1), up(2), up(3)
        N = rays * M
        self.t = torch.zeros(N, dtype=torch.float64, device=dev)
        self.face = torch.zeros(N, dtype=torch.int32, device=dev)
        self.poses = torch.zeros((N, angles, 4, 4), dtype=torch.float64, device=dev)
        self.valid = torch.zeros((N, angles), dtype=torch.uint8, device=dev)
        self.cs = torch.from_numpy(G.approach_angles(angles)).to(dev)
        self.probe = torch.from_numpy(G.default_probe()).to(dev)

    def cast(self):
        ops.mesh_raycast_batch(self.batch, self.p1, self.d, out=(self.t, self.face))

    def pose(self):
        ops.grasp_poses(self.batch, self.p1, self.n1, self.d, self.t, self.face, self.nrm, self.cs, self.probe, self.pool,
                        cos_cone=float(np.cos(CONE)), out=(self.poses, self.valid))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--angles", type=int, default=8)
    ap.add_argument("--objects", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-rays", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "grasp_sampling_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grasp_sampling_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    v, f = G.outward_mesh(*MC.icosphere(a.level, 0.03))
    M = a.objects
    # (a)
    one = Prepared([(v, f)], a.rays, a.angles, 0, dev)
    a_cast, a_cast_all = timed(one.cast, a.reps, stream)
    a_pose, a_pose_all = timed(one.pose, a.reps, stream)
    one1 = Prepared([(v, f)], a.rays, a.angles, 1, dev)
    a1_cast, a1_cast_all = timed(one1.cast, a.reps, stream)
    same_split = bool(torch.equal(one.t.view(torch.int64), one1.t.view(torch.int64)) and torch.equal(one.face, one1.face))
    # (b)
    rng = np.random.RandomState(0)
    meshes = [(v * rng.uniform(0.9, 1.1), f) for _ in range(M)]  # objects of one size, not one object
    many = Prepared(meshes, a.rays, a.angles, 0, dev)
    b_cast, b_cast_all = timed(many.cast, a.reps, stream)
    b_pose, b_pose_all = timed(many.pose, a.reps, stream)
    # (c): the same rays (Prepared draws them mesh by mesh from one stream, so a batch of one starts the stream again: upload b's)
    singles = []
    for m in range(M):
        s = Prepared([meshes[m]], a.rays, a.angles, 0, dev)
        rows = slice(m * a.rays, (m + 1) * a.rays)
        s.p1, s.n1, s.d = many.p1[rows].contiguous(), many.n1[rows].contiguous(), many.d[rows].contiguous()
        singles.append(s)

    def all_cast():
        for s in singles:
            s.cast()

    def all_pose():
        for s in singles:
            s.pose()
    c_cast, c_cast_all = timed(all_cast, a.reps, stream)
    c_pose, c_pose_all = timed(all_pose, a.reps, stream)
    same_batch = bool(torch.equal(torch.cat([s.t for s in singles]).view(torch.int64), many.t.view(torch.int64)) and
                      torch.equal(torch.cat([s.valid for s in singles]), many.valid) and
                      torch.equal(torch.cat([s.poses for s in singles]).view(torch.int64), many.poses.view(torch.int64)))
    # the host specification on fewer rays, scaled by the ray count
    H = a.host_rays
    p1, n1, d, nrm = (x[:H] if i < 3 else x for i, x in enumerate(one.host[0]))
    grid = sc.SdfGrid(one.pool.cpu().numpy().reshape(tuple(one.batch.rec[0].dims)), np.array(one.batch.rec[0].origin), 0.005)
    t0 = time.perf_counter()
    ht, hf = G.mesh_raycast(v, f, p1, d)
    host_cast = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, hv, _ = G.grasp_poses(p1, n1, d, ht, hf, nrm, G.approach_angles(a.angles), grid, G.default_probe(), cone=CONE)
    host_pose = time.perf_counter() - t0
    same_host = bool(np.array_equal(one.t.cpu().numpy()[:H].view(np.int64), ht.view(np.int64)) and
                     np.array_equal(one.valid.cpu().numpy()[:H].astype(bool), hv))
    pairs = a.rays * len(f)
    res = {
        "device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "faces": int(len(f)), "rays": a.rays, "angles": a.angles,
        "objects": M, "reps": a.reps, "ray_face_pairs_per_mesh": pairs, "probe_points": 100,
        "a_chunks_automatic": one.batch.chunks, "a_raycast_ms": a_cast, "a_raycast_runs_ms": a_cast_all, "a_pairs_per_s": pairs / (a_cast * 1e-3),
        "a_raycast_one_chunk_ms": a1_cast, "a_raycast_one_chunk_runs_ms": a1_cast_all, "a_split_equals_one_chunk_bit_for_bit": same_split,
        "a_poses_ms": a_pose, "a_poses_runs_ms": a_pose_all, "a_valid_poses": int(one.valid.sum().item()),
        "b_chunks_automatic": many.batch.chunks, "b_raycast_ms": b_cast, "b_raycast_runs_ms": b_cast_all, "b_raycast_ms_per_mesh": b_cast / M,
        "b_pairs_per_s": M * pairs / (b_cast * 1e-3), "b_poses_ms": b_pose, "b_poses_runs_ms": b_pose_all,
        "c_raycast_single_launches_ms": c_cast, "c_raycast_runs_ms": c_cast_all, "c_poses_single_launches_ms": c_pose, "c_poses_runs_ms": c_pose_all,
        "b_equals_c_bit_for_bit": same_batch,
        "host_spec_rays": H, "host_spec_raycast_s": host_cast, "host_spec_poses_s": host_pose,
        "host_spec_scaled_to_rays_s": (host_cast + host_pose) * a.rays / H, "host_spec_threads": 1, "device_equals_host_spec": same_host,
    }
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_runs_ms")}))


if __name__ == "__main__":
    main()
