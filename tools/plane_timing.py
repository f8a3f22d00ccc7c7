"""Timing of support-plane fitting (omgx_plane_ransac, omgx_plane_moments, omgx_plane_mask) on one GPU.

  python tools/plane_timing.py [--reps 9] [--out profiles/plane_timing.json]

Depth images made on the host: a tilted floor seen by a pinhole camera, 30 % of the pixels in front of it (objects), 10 % holes:
  (a) one 640 x 480 view with 256 hypotheses;
  (b) 100 views of 160 x 120 with 256 hypotheses each, in ONE set of launches, and the same 100 as 100 single calls.
For each entry point: two HIP events on the stream around the call, with images, triples, planes, workspace and outputs on the
device before the first event; the median of `reps` runs after three warm-up runs, and every run.  omgx_plane_ransac is three
launches; the same call with a prior that no hypothesis meets (every row void: the scoring workgroups stage their blocks and
count nothing) is timed too, and the difference is what the counting costs.
The scoring kernel's float64 VALU-issue bound, priced from its own operation count as DESIGN.md section 5.2 prices instructions:
per (pixel, live hypothesis) three multiplications, three additions and one comparison in float64, 7 wave-instructions per 64
pixels at 4 cycles each on one of 1024 SIMDs at 2.4 GHz.
For comparison: the numpy specification on the CPU (ONE run: not a median), and a torch composition of the same passes on the
device (points, a [K,4] x [4,N] product, compare, sum), events around it, the same median.
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

from omg_planner_amd import _lib, planes as pl  # noqa: E402

SIMDS, CLOCK_HZ, CYCLES_F64, F64_PER_PAIR = 1024, 2.4e9, 4.0, 7
TOL = 0.004


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


def views(V, H, W, rng):
    """(intrinsics [V,4], depth [V,H,W]): a floor about a metre away, objects in front of 30 % of it, 10 % holes."""
    f = 0.8 * W
    intr = np.tile(np.array([f, f, (W - 1) / 2, (H - 1) / 2]), (V, 1))
    r, c = np.divmod(np.arange(H * W), W)
    depth = np.empty((V, H * W))
    for v in range(V):
        n = np.array([rng.normal(scale=0.1), -0.8 + rng.normal(scale=0.05), -0.6])
        n /= np.linalg.norm(n)
        off = -float(n @ np.array([0.0, 0.0, rng.uniform(0.8, 1.2)]))
        den = n[0] * (c - intr[v, 2]) / f + n[1] * (r - intr[v, 3]) / f + n[2]
        with np.errstate(all="ignore"):
            d = -off / den
        d = np.where(d > 0, d, np.inf)
        kind = rng.random(H * W)
        d = np.where(kind < 0.3, d * rng.uniform(0.6, 0.95, H * W), d)
        depth[v] = np.where(kind > 0.9, np.inf, d)
    return intr, depth.reshape(V, H, W)


class Steps:
    """The entry points on prepared buffers."""

    def __init__(self, intr, depth, triples, dev):
        self.l = _lib.lib()
        self.h_intr, self.h_tri = np.ascontiguousarray(intr, np.float64), np.ascontiguousarray(triples, np.int32)
        self.V, self.H, self.W = depth.shape
        self.K = self.h_tri.shape[1]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.intr, self.depth, self.tri = up(self.h_intr), up(depth), up(self.h_tri)
        self.up_never = up(np.tile(np.array([0.0, 0.0, 0.0]), (self.V, 1)))  # n.up = 0 < cos_min = 1: every row void
        V, K = self.V, self.K
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
        self.planes, self.best_planes, self.anchors, self.sums = f64(V, K, 4), f64(V, 4), f64(V, 3), f64(V, 9)
        self.counts, self.best, self.count = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((V, K), (V,), (V,)))
        self.ws = torch.empty(max(int(self.l.omgx_plane_workspace_bytes(V, self.H, self.W)), 8), dtype=torch.uint8, device=dev)
        self.mask = torch.empty((V, self.H, self.W), dtype=torch.uint8, device=dev)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ransac(self, void=False):
        vp = C.c_void_p
        _lib.check(self.l.omgx_plane_ransac(vp(self.intr.data_ptr()), vp(self.h_intr.ctypes.data), vp(self.depth.data_ptr()), None, self.V, self.H, self.W,
                                            vp(self.tri.data_ptr()), vp(self.h_tri.ctypes.data), self.K, TOL, 1e-10,
                                            vp(self.up_never.data_ptr()) if void else None, 1.0 if void else -1.0, vp(self.planes.data_ptr()),
                                            vp(self.counts.data_ptr()), vp(self.best.data_ptr()), vp(self.best_planes.data_ptr()),
                                            vp(self.anchors.data_ptr()), self._stream()), "omgx_plane_ransac")

    def moments(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_plane_moments(vp(self.intr.data_ptr()), vp(self.h_intr.ctypes.data), vp(self.depth.data_ptr()), None, self.V, self.H, self.W,
                                             vp(self.best_planes.data_ptr()), vp(self.anchors.data_ptr()), TOL, vp(self.ws.data_ptr()),
                                             vp(self.count.data_ptr()), vp(self.sums.data_ptr()), self._stream()), "omgx_plane_moments")

    def masks(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_plane_mask(vp(self.intr.data_ptr()), vp(self.h_intr.ctypes.data), vp(self.depth.data_ptr()), None, self.V, self.H, self.W,
                                          vp(self.best_planes.data_ptr()), TOL, vp(self.mask.data_ptr()), self._stream()), "omgx_plane_mask")


def torch_score(intr, depth, planes):
    """The same passes as a torch composition: points, a [K,4] x [4,N] product, compare, sum -> counts [V,K] (void rows count
    whatever their zeros give; this is for cost only)."""
    V, H, W = depth.shape
    idx = torch.arange(H * W, device=depth.device)
    r, c = (idx // W).double(), (idx % W).double()
    d = depth.reshape(V, -1)
    dx, dy = (c[None] - intr[:, 2:3]) / intr[:, 0:1], (r[None] - intr[:, 3:4]) / intr[:, 1:2]
    valid = (d > 0) & torch.isfinite(d)
    dz = torch.where(valid, d, torch.zeros_like(d))
    p4 = torch.stack([dz * dx, dz * dy, dz, torch.ones_like(dz)], 1)  # [V,4,N]
    return (((planes @ p4).abs() <= TOL) & valid[:, None]).sum(2)


def measure(name, V, H, W, K, reps, dev, stream, rng, single_calls=False):
    intr, depth = views(V, H, W, rng)
    triples = pl.draw_triples(H, W, K, rng, views=V)
    st = Steps(intr, depth, triples, dev)
    ransac, void = timed(st.ransac, reps, stream), timed(lambda: st.ransac(True), reps, stream)
    st.ransac()
    moments, masks = timed(st.moments, reps, stream), timed(st.masks, reps, stream)
    torch.cuda.synchronize()
    counts = st.counts.cpu().numpy()
    live = int((counts >= 0).sum())
    t0 = time.perf_counter()
    want = pl.ransac(intr, depth, triples, TOL, 1e-10)
    ransac_cpu = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want_count, want_sums = pl.moments(intr, depth, want[3], want[4], TOL)
    moments_cpu = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(counts, want[1]) and np.array_equal(st.planes.cpu().numpy().view(np.uint64), want[0].view(np.uint64))
                and np.array_equal(st.sums.cpu().numpy().view(np.uint64), want_sums.view(np.uint64)) and np.array_equal(st.count.cpu().numpy(), want_count))
    composed = timed(lambda: torch_score(st.intr, st.depth, st.planes), reps, stream)
    pairs = live * H * W
    bound = pairs / 64 * F64_PER_PAIR * CYCLES_F64 / (SIMDS * CLOCK_HZ) * 1e3
    res = {"shape": name, "views": V, "H": H, "W": W, "hypotheses": K, "live_hypotheses": live, "pixel_hypothesis_pairs": pairs,
           "workgroups_of_the_scoring_launch": V * -(-H * W // _lib.PLANE_PIXELS_PER_WORKGROUP),
           "ransac_ms": ransac[0], "ransac_runs_ms": ransac[1], "ransac_every_row_void_ms": void[0], "ransac_every_row_void_runs_ms": void[1],
           "counting_ms": ransac[0] - void[0], "moments_ms": moments[0], "moments_runs_ms": moments[1], "mask_ms": masks[0], "mask_runs_ms": masks[1],
           "scoring_f64_valu_issue_bound_ms": bound, "share_of_bound_whole_ransac_call": bound / ransac[0],
           "share_of_bound_counting_alone": bound / max(ransac[0] - void[0], 1e-9),
           "numpy_specification_ransac_cpu_ms_one_run": ransac_cpu, "numpy_specification_moments_cpu_ms_one_run": moments_cpu,
           "torch_composition_score_ms": composed[0], "torch_composition_score_runs_ms": composed[1], "equals_specification": same}
    out = [res]
    if single_calls:
        singles = [Steps(intr[v: v + 1], depth[v: v + 1], triples[v: v + 1], dev) for v in range(V)]
        r_ms = timed(lambda: [s.ransac() for s in singles], reps, stream)
        m_ms = timed(lambda: [s.moments() for s in singles], reps, stream)
        k_ms = timed(lambda: [s.masks() for s in singles], reps, stream)
        out.append({"shape": f"{name}_as_{V}_single_calls", "views": V, "ransac_ms": r_ms[0], "ransac_runs_ms": r_ms[1], "moments_ms": m_ms[0],
                    "moments_runs_ms": m_ms[1], "mask_ms": k_ms[0], "mask_runs_ms": k_ms[1]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plane_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plane_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(0)
    (ha, wa), (hb, wb), many, K = (((48, 64), (30, 40), 4, 64) if a.small else ((480, 640), (120, 160), 100, 256))
    shapes = measure(f"a_one_{wa}x{ha}_view", 1, ha, wa, K, a.reps, dev, stream, rng)
    shapes += measure(f"b_{many}_views_of_{wb}x{hb}_one_set_of_launches", many, hb, wb, K, a.reps, dev, stream, rng, single_calls=True)
    res = {"library": Path(_lib.LIB_PATH).name, "device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "tol": TOL, "pricing": {"simds": SIMDS, "clock_hz": CLOCK_HZ, "cycles_per_f64_wave_instruction": CYCLES_F64,
                                   "f64_wave_instructions_per_64_pixel_hypothesis_pairs": F64_PER_PAIR},
           "single_runs": ["numpy_specification_ransac_cpu_ms_one_run", "numpy_specification_moments_cpu_ms_one_run"],
           "not_tried": ["splitting the hypotheses of one view over several workgroups (one 640 x 480 view fills 150 workgroups on 256 CUs)",
                         "other chunk sizes than 2048 pixels per workgroup", "float32 scoring with a float64 re-check of the pixels near the threshold",
                         "packing two hypotheses per pass to share the loads of the points", "a graph capture of the three launches"],
           "shapes": shapes}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in s.items() if not k.endswith("_runs_ms")} for s in shapes]))


if __name__ == "__main__":
    main()
