"""Timing of depth conditioning (omgx_depth_condition, omgx_depth_normals) on one GPU, beside what a user would write today.

  python tools/sensor_timing.py [--reps 15] [--out profiles/sensor_timing.json] [--variant csrc/libomg_hip_sndirect.so]

The frames: a tilted plane with a box in front of it through sensor.simulate (uint16 millimetres, noise, 1 % dropout, flying
pixels at the box's silhouette), and the same as float64 metres.
  (a) one 640 x 480 frame;   (b) 100 frames of 160 x 120;   each with R = 3 and R = 7 and both input kinds.
For each:
  kernel   the entry point alone through the C ABI, everything already on the device, between two HIP events on the stream; the
           median of `reps` launches after three warm-up launches.  A launch of an empty kernel's worth of work (V = 1, 1 x 1)
           is timed the same way: what the clock and the launch cost.
  torch    the composition a user would write today, the same clock: unfold over the padded image and elementwise operations
           for the flying test and the bilateral filter (the sums over the window are torch's reductions, so the last bits may
           differ: the largest difference is reported); shifted slices and elementwise operations for the normals
  numpy    the specification on the CPU, one run, a host clock
The float64 VALU-issue bound of the filter's tap loop as DESIGN.md section 5.2 prices it, from the instruction mix of the compiled
loop (counted in the ISA of csrc/omg_sensor.hip: per tap a subtraction, a division of 10 float64 steps and a v_rcp_f64, x*x,
1 - x*x, two compares, u*u, the table's weight, w*z and two additions: 20 float64 instructions of 4 issue cycles, the v_rcp_f64 of
8, a move and an address addition of 2 each = 92 cycles per wave and tap, on one of 1024 SIMDs at 2.4 GHz).  A tile is four
waves whether the image fills it or not.  The staging, the flying test and the stores are not in the bound.
With --variant (a library built with -DOMGX_SENSOR_NORMALS_DIRECT=1: `make variants`) the normals kernel that reads its five
depths straight from global memory is timed against the product's tile staged in LDS, alternating, and its outputs compared.
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
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from omg_planner_amd import _lib, sensor  # noqa: E402

TAP_CYCLES = 20 * 4 + 8 + 2 * 2
SIMDS, CLOCK_HZ = 1024, 2.4e9
SCALE, Z_MIN, Z_MAX, TAU, MIN_SUPPORT, RANGE_SCALE, COS_MIN = 0.001, 0.2, 6.0, (0.004, 0.0, 0.006), 3, 2.0, 0.2
SIGMA = (0.0005, 0.002)


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


def make_frames(V, H, W, seed):
    """(uint16 frames, the same in float64 metres, intrinsics [V,4])"""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    t = np.zeros((V, H, W))
    for v in range(V):
        z = rng.uniform(1.0, 2.0) + rng.uniform(-0.3, 0.3) * r / H + rng.uniform(-0.3, 0.3) * c / W
        r0, c0 = rng.integers(0, H // 2), rng.integers(0, W // 2)
        t[v] = np.where((r >= r0) & (r < r0 + H // 3) & (c >= c0) & (c < c0 + W // 3), z - rng.uniform(0.2, 0.5), z)
    frame, _ = sensor.simulate(t, rng, SCALE, SIGMA, 0.01, flying=TAU)
    f = 0.9 * W
    return frame, frame.astype(np.float64) * SCALE, np.tile((f, f, 0.5 * (W - 1), 0.5 * (H - 1)), (V, 1))


def as_double(frames):
    if frames.dtype == torch.uint16:  # (few torch operations take uint16: through int16's bits)
        return (frames.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float64) * SCALE
    return frames


def torch_condition(frames, R, table):
    """What a user writes today: unfold and elementwise operations -> (depth, flags)."""
    z = as_double(frames)
    V, H, W = z.shape
    ret = (z >= Z_MIN) & (z <= Z_MAX)
    z = torch.where(ret, z, torch.zeros_like(z))
    tau = (TAU[0] + TAU[1] * z) + TAU[2] * (z * z)
    nb = F.unfold(F.pad(z[:, None], (1, 1, 1, 1)), 3).reshape(V, 9, H, W)
    d = nb - z[:, None]
    near = (nb > 0) & (d <= tau[:, None]) & (-d <= tau[:, None])
    keep = ret & ((near.sum(1) - near[:, 4].long()) >= MIN_SUPPORT)
    zs = torch.where(keep, z, torch.zeros_like(z))
    out = zs
    if R > 0:
        nb = F.unfold(F.pad(zs[:, None], (R, R, R, R)), 2 * R + 1).reshape(V, (2 * R + 1) ** 2, H, W)
        x = (nb - zs[:, None]) / (RANGE_SCALE * tau)[:, None]
        u = 1.0 - x * x
        w = torch.where((nb > 0) & (u > 0), table[None, :, None, None] * (u * u), torch.zeros_like(u))
        num, den = (w * nb).sum(1), w.sum(1)
        out = torch.where(den > 0, num / den, zs)
    flags = torch.where(keep, 0, torch.where(ret, 2, 1)).to(torch.uint8)
    return torch.where(keep, out, torch.zeros_like(out)), flags


def _shift(a, dr, dc):
    return F.pad(a, (1, 1, 1, 1))[..., 1 + dr: 1 + dr + a.shape[-2], 1 + dc: 1 + dc + a.shape[-1]]


def torch_normals(z, k):
    """Shifted slices and elementwise operations -> (normals, depth_out)."""
    V, H, W = z.shape
    r, c = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=z.device), torch.arange(W, dtype=torch.float64, device=z.device), indexing="ij")
    dx, dy = (c[None] - k[:, 2, None, None]) / k[:, 0, None, None], (r[None] - k[:, 3, None, None]) / k[:, 1, None, None]
    P = [dx * z, dy * z, z]
    tau = (TAU[0] + TAU[1] * z) + TAU[2] * (z * z)

    def difference(dr, dc):
        zb, za = _shift(z, -dr, -dc), _shift(z, dr, dc)
        before, after = (zb > 0) & (zb - z <= tau) & (z - zb <= tau), (za > 0) & (za - z <= tau) & (z - za <= tau)
        return [torch.where(after, _shift(P[j], dr, dc), P[j]) - torch.where(before, _shift(P[j], -dr, -dc), P[j]) for j in range(3)], before | after
    a, ha = difference(0, 1)
    b, hb = difference(1, 0)
    m = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    s = (m[0] * P[0] + m[1] * P[1]) + m[2] * P[2]
    nn = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
    has = (z > 0) & ha & hb & (s != 0) & (nn > 0)
    length = torch.sqrt(nn)
    n = [torch.where(s > 0, -x, x) / length for x in m]
    cs = -((n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]) / torch.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2])
    good = has & ~(cs < COS_MIN)
    zero = torch.zeros_like(z)
    return torch.stack([torch.where(good, x, zero) for x in n], -1), torch.where((z > 0) & ~(has & (cs < COS_MIN)), z, zero)


def bind(path):
    lib = C.CDLL(str(path))
    for name in ("omgx_depth_condition", "omgx_depth_normals"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.FUNCTIONS[name]
    return lib


def measure(name, V, H, W, reps, dev, stream, seed, variant):
    u16, f64, h_k = make_frames(V, H, W, seed)
    l, vp = _lib.lib(), C.c_void_p
    p = lambda x: vp(x.data_ptr())
    d_k = torch.from_numpy(h_k).to(dev)
    depth, depth2 = torch.empty((V, H, W), dtype=torch.float64, device=dev), torch.empty((V, H, W), dtype=torch.float64, device=dev)
    flags, flags2 = torch.empty((V, H, W), dtype=torch.uint8, device=dev), torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    normals = torch.empty((V, H, W, 3), dtype=torch.float64, device=dev)
    tiles = -(-H // 16) * -(-W // 16) * V
    res = {"shape": name, "views": V, "H": H, "W": W, "tiles": tiles, "bytes_read_uint16": V * H * W * 2, "bytes_written_condition": V * H * W * 9, "runs": []}
    for R in (3, 7):
        h_table = sensor.gaussian_table(R, 0.5 * R)
        d_table = torch.from_numpy(h_table).to(dev)
        bound_ms = tiles * 4 * (2 * R + 1) ** 2 * TAP_CYCLES / (SIMDS * CLOCK_HZ) * 1e3
        for kind, host in (("uint16", u16), ("float64", f64)):
            frames = torch.from_numpy(host).to(dev)

            def condition():
                _lib.check(l.omgx_depth_condition(p(frames), sensor.UINT16 if kind == "uint16" else sensor.FLOAT64, SCALE, V, H, W, Z_MIN, Z_MAX, *TAU,
                                                  MIN_SUPPORT, R, p(d_table), vp(h_table.ctypes.data), RANGE_SCALE, p(depth), p(flags),
                                                  vp(stream.cuda_stream)), "omgx_depth_condition")
            k = by_events(condition, reps, stream)
            tc = by_events(lambda: torch_condition(frames, R, d_table), max(reps // 3, 3), stream, warm_up=1)
            t_depth, t_flags = torch_condition(frames, R, d_table)
            t0 = time.perf_counter()
            want_depth, want_flags = sensor.condition_depth(host, SCALE, Z_MIN, Z_MAX, TAU, MIN_SUPPORT, R, h_table, RANGE_SCALE)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            res["runs"].append({"R": R, "kind": kind, "kernel_ms": k[0], "kernel_runs_ms": k[1], "torch_ms": tc[0], "torch_runs_ms": tc[1],
                                "torch_over_kernel": tc[0] / k[0], "numpy_ms": numpy_ms, "numpy_over_kernel": numpy_ms / k[0],
                                "kernel_equals_numpy": bool(np.array_equal(depth.cpu().numpy().view(np.int64), want_depth.view(np.int64))
                                                            and np.array_equal(flags.cpu().numpy(), want_flags)),
                                "torch_flags_equal_kernel": bool(torch.equal(t_flags, flags)),
                                "torch_largest_difference": float((t_depth - depth).abs().max().item()),
                                "kept_share": float((flags == 0).double().mean().item()), "flying_pixels": int((flags == 2).sum().item()),
                                "valu_bound_tap_loop_ms": bound_ms, "kernel_over_bound": k[0] / bound_ms})
            del t_depth, t_flags

    def normals_with(lib):
        return lambda: _lib.check(lib.omgx_depth_normals(p(depth), p(flags), p(d_k), vp(h_k.ctypes.data), V, H, W, *TAU, COS_MIN, p(normals), p(depth2),
                                                         p(flags2), None, vp(stream.cuda_stream)), "omgx_depth_normals")
    n = by_events(normals_with(l), reps, stream)
    direct = (normals.clone(), depth2.clone(), flags2.clone())  # (the product's outputs)
    tn = by_events(lambda: torch_normals(depth, d_k), max(reps // 3, 3), stream, warm_up=1)
    t_normals, t_depth2 = torch_normals(depth, d_k)
    t0 = time.perf_counter()
    want = sensor.depth_normals(depth.cpu().numpy(), h_k, TAU, COS_MIN, flags.cpu().numpy())
    numpy_ms = (time.perf_counter() - t0) * 1e3
    res["normals"] = {"kernel_ms": n[0], "kernel_runs_ms": n[1], "torch_ms": tn[0], "torch_runs_ms": tn[1], "torch_over_kernel": tn[0] / n[0],
                      "numpy_ms": numpy_ms, "numpy_over_kernel": numpy_ms / n[0],
                      "kernel_equals_numpy": bool(np.array_equal(direct[0].cpu().numpy().view(np.int64), want[0].view(np.int64))
                                                  and np.array_equal(direct[2].cpu().numpy(), want[2])),
                      "torch_equals_kernel": bool(torch.equal(t_normals, direct[0]) and torch.equal(t_depth2, direct[1])),
                      "torch_largest_difference": float((t_normals - direct[0]).abs().max().item()),
                      "grazing_pixels": int((flags2 == 3).sum().item()), "bytes_read": V * H * W * 9, "bytes_written": V * H * W * 33}
    if variant is not None:
        a, b = [], []
        for _ in range(3):  # alternating, so that both see the same neighbours on the machine
            a += by_events(normals_with(l), reps, stream)[1]
            b += by_events(normals_with(variant), reps, stream)[1]
        res["normals"].update({"lds_staged_ms": statistics.median(a), "lds_staged_runs_ms": a, "direct_reads_ms": statistics.median(b), "direct_reads_runs_ms": b,
                               "lds_staged_equals_direct": bool(torch.equal(normals, direct[0]) and torch.equal(depth2, direct[1]) and torch.equal(flags2, direct[2]))})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--variant", default=None, help="a library built with -DOMGX_SENSOR_NORMALS_DIRECT=1")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sensor_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sensor_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    variant = None if a.variant is None else bind(a.variant)
    shapes = [("a_one_frame_640x480", 1, 480, 640), ("b_100_frames_160x120", 100, 120, 160)]
    if a.small:
        shapes = [("a_small", 1, 48, 64), ("b_small", 4, 24, 32)]
    l, vp = _lib.lib(), C.c_void_p
    one = torch.full((1, 1, 1), 1000, dtype=torch.int16, device=dev).view(torch.uint16)
    out1, flag1, tab1 = torch.empty((1, 1, 1), dtype=torch.float64, device=dev), torch.empty((1, 1, 1), dtype=torch.uint8, device=dev), np.ones(1)
    d_tab1 = torch.from_numpy(tab1).to(dev)
    launch = by_events(lambda: _lib.check(l.omgx_depth_condition(vp(one.data_ptr()), 0, SCALE, 1, 1, 1, Z_MIN, Z_MAX, *TAU, 0, 0, vp(d_tab1.data_ptr()),
                                                                 vp(tab1.ctypes.data), RANGE_SCALE, vp(out1.data_ptr()), vp(flag1.data_ptr()),
                                                                 vp(stream.cuda_stream)), "omgx_depth_condition"), a.reps, stream)
    res = {"device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "issue_cycles_per_wave_and_tap": TAP_CYCLES, "one_pixel_launch_ms": launch[0], "one_pixel_launch_runs_ms": launch[1],
           "normals_variant": a.variant, "shapes": [measure(s[0], *s[1:], a.reps, dev, stream, k, variant) for k, s in enumerate(shapes)]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    brief = lambda d: {k: v for k, v in d.items() if not k.endswith("_runs_ms")}
    print(json.dumps({"one_pixel_launch_ms": launch[0], "shapes": [{**brief(s), "runs": [brief(r) for r in s["runs"]], "normals": brief(s["normals"])}
                                                                   for s in res["shapes"]]}))


if __name__ == "__main__":
    main()
