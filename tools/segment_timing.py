"""Timing of object segmentation (omgx_label_components, omgx_component_records, omgx_component_states) on one GPU.

  python tools/segment_timing.py [--reps 7] [--out profiles/segment_timing.json]

States as a carve leaves them, made on the host from analytic solids (a slab and boxes and spheres standing apart above it:
SURFACE within a band of the solids' faces, UNKNOWN deeper inside, FREE outside; the slab's own band is FREE, as after
explained_mask):
  (a) one 75 x 75 x 50 volume;
  (b) 100 volumes of 64^3 in ONE set of launches, and the same 100 as 100 single calls;
  (c) omgx_component_states for 100 targets: the crop of the largest component of every volume of (b) grown by 14 nodes, mode 0.
For each entry point: two HIP events on the stream around the call, with states, records, workspace and outputs on the device
before the first event; the median of `reps` runs after three warm-up runs, and every run.  The bytes-moved bound over HBM peak:
the labelling moves per node 1 B of state, the link written and read three times (4 B each), its rank byte written, and the
label filled and written (4 B twice): 26 B; the records read 4 B per node; a cropped output node reads 1 B + 4 B and writes 1 B.
For cost only, scipy.ndimage.label + find_objects of the same masks on the CPU (ONE run: not a median).
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

from omg_planner_amd import _lib, ops, segmentation as sg  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second: HBM3E's specification
LABEL_BYTES, RECORD_BYTES, CROP_BYTES = 26, 4, 6


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


def carved_states(dims, delta, rng, objects=5, band=1.5):
    """uint8 [X,Y,Z]: `objects` boxes and spheres above z = 4 nodes, their faces' band SURFACE, their insides UNKNOWN."""
    idx = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float32) for d in dims], indexing="ij"), -1)
    dist = np.full(dims, np.inf, np.float32)
    for _ in range(objects):
        half = rng.uniform(3.0, 0.11 * min(dims[:2]), 3).astype(np.float32)
        c = np.array([rng.uniform(half[0] + 2, dims[0] - half[0] - 2), rng.uniform(half[1] + 2, dims[1] - half[1] - 2), 5 + half[2]], np.float32)
        if rng.random() < 0.5:
            d = np.linalg.norm(idx - c, axis=-1) - half.min()
        else:
            q = np.abs(idx - c) - half
            d = np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)
        dist = np.minimum(dist, d)
    return np.where(np.abs(dist) <= band, 1, np.where(dist < 0, 2, 0)).astype(np.uint8)


class Steps:
    """The entry points on prepared buffers."""

    def __init__(self, states, delta, dev):
        vp = C.c_void_p
        self.l, self.M = _lib.lib(), len(states)
        self.volumes = [((0.0, 0.0, 0.0), delta, "centre", s.shape) for s in states]
        self.rec = ops.surface_records([v + (0,) for v in self.volumes])
        self.nodes = np.array([s.size for s in states], np.int64)
        self.h_begin = np.cumsum(self.nodes) - self.nodes
        self.up = lambda a: torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy() if isinstance(a, C.Array) else np.ascontiguousarray(a)).to(dev)
        self.d_rec, self.d_begin = self.up(self.rec), self.up(self.h_begin)
        self.state = self.up(np.concatenate([s.ravel() for s in states]))
        self.elems = int(self.state.numel())
        self.ws = torch.empty(int(self.l.omgx_label_workspace_bytes(C.cast(self.rec, vp), self.M)), dtype=torch.uint8, device=dev)
        self.labels = torch.empty(self.elems, dtype=torch.int32, device=dev)
        self.counts = torch.empty(self.M, dtype=torch.int32, device=dev)
        self.dev = dev

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def label(self, connectivity=6):
        vp = C.c_void_p
        _lib.check(self.l.omgx_label_components(vp(self.state.data_ptr()), self.elems, vp(self.d_begin.data_ptr()), vp(self.h_begin.ctypes.data),
                                                vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M, 1, connectivity, vp(self.ws.data_ptr()),
                                                vp(self.labels.data_ptr()), vp(self.counts.data_ptr()), self._stream()), "omgx_label_components")

    def layout(self):
        """After label(): the host reads the counts and lays out the records."""
        self.comp_begin = np.concatenate([[0], np.cumsum(self.counts.cpu().numpy().astype(np.int64))]).astype(np.int64)
        self.d_comp = self.up(self.comp_begin)
        self.records = torch.empty((max(int(self.comp_begin[-1]), 1), 8), dtype=torch.int32, device=self.dev)

    def fill(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_component_records(vp(self.labels.data_ptr()), self.elems, vp(self.d_begin.data_ptr()), vp(self.h_begin.ctypes.data),
                                                 vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M, vp(self.d_comp.data_ptr()),
                                                 vp(self.comp_begin.ctypes.data), vp(self.records.data_ptr()), int(self.comp_begin[-1]), self._stream()),
                   "omgx_component_records")

    def prepare_crops(self, margin):
        h = self.records.cpu().numpy()
        picks, outs = [], []
        for m in range(self.M):
            rows = h[int(self.comp_begin[m]): int(self.comp_begin[m + 1])]
            if not len(rows):
                continue
            c = int(np.argmax(rows[:, 0]))
            origin, delta, dims, first = sg.crop_layout(self.volumes[m], rows[c], margin)
            picks.append((m,) + first + (int(self.comp_begin[m]) + c, 0, 0, 0))
            outs.append((origin, delta, "centre", dims, 0))
        self.h_picks = np.array(picks, np.int32).reshape(-1, 8)
        self.out_rec = ops.surface_records(outs)
        sizes = np.array([int(np.prod(o[3])) for o in outs], np.int64)
        self.h_ob = np.cumsum(sizes) - sizes
        self.d_picks, self.d_out_rec, self.d_ob = self.up(self.h_picks), self.up(self.out_rec), self.up(self.h_ob)
        self.out = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=self.dev)
        return int(sizes.sum())

    def crop(self):
        vp = C.c_void_p
        _lib.check(self.l.omgx_component_states(vp(self.state.data_ptr()), self.elems, vp(self.d_begin.data_ptr()), vp(self.h_begin.ctypes.data),
                                                vp(self.d_rec.data_ptr()), C.cast(self.rec, vp), self.M, vp(self.labels.data_ptr()), vp(self.d_comp.data_ptr()),
                                                vp(self.comp_begin.ctypes.data), vp(self.records.data_ptr()), int(self.comp_begin[-1]),
                                                vp(self.d_picks.data_ptr()), vp(self.h_picks.ctypes.data), vp(self.d_out_rec.data_ptr()),
                                                C.cast(self.out_rec, vp), len(self.h_picks), vp(self.d_ob.data_ptr()), vp(self.h_ob.ctypes.data),
                                                vp(self.out.data_ptr()), int(self.out.numel()), self._stream()), "omgx_component_states")


def scipy_ms(states):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.perf_counter()
    for s in states:
        lab, _ = ndimage.label(s == 1)
        ndimage.find_objects(lab)
    return (time.perf_counter() - t0) * 1e3


def measure(name, states, delta, reps, dev, stream):
    st = Steps(states, delta, dev)
    label_ms = timed(st.label, reps, stream)
    st.layout()
    fill_ms = timed(st.fill, reps, stream)
    nodes = int(st.nodes.sum())
    labels = st.labels.cpu().numpy()[: states[0].size]
    want = sg.label_components(states[0].ravel(), st.volumes[:1])
    same = bool(np.array_equal(labels, want) and np.array_equal(st.records.cpu().numpy()[: int(st.comp_begin[1])], sg.component_records(want, st.volumes[:1])[1]))
    bound = lambda per_node, n=nodes: n * per_node / HBM_PEAK * 1e3
    return st, {"shape": name, "volumes": len(states), "nodes": nodes, "components": int(st.comp_begin[-1]), "surface_nodes": int(sum((s == 1).sum() for s in states)),
                "label_ms": label_ms[0], "label_runs_ms": label_ms[1], "records_ms": fill_ms[0], "records_runs_ms": fill_ms[1],
                "label_bytes": nodes * LABEL_BYTES, "label_hbm_bound_ms": bound(LABEL_BYTES), "label_share_of_bound": bound(LABEL_BYTES) / label_ms[0],
                "records_bytes": nodes * RECORD_BYTES, "records_hbm_bound_ms": bound(RECORD_BYTES), "records_share_of_bound": bound(RECORD_BYTES) / fill_ms[0],
                "workspace_bytes": int(st.ws.numel()), "scipy_label_find_objects_cpu_ms_one_run": scipy_ms(states),
                "first_volume_equals_specification": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segment_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_timing.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(0)
    out = []
    dims, n, many = ((15, 15, 10), 16, 5) if a.small else ((75, 75, 50), 64, 100)
    _, r = measure("a_one_%dx%dx%d" % dims, [carved_states(dims, 0.02, rng)], 0.02, a.reps, dev, stream)
    out.append(r)
    states = [carved_states((n, n, n), 0.01, rng) for _ in range(many)]
    st, r = measure(f"b_{many}_volumes_of_{n}^3_one_set_of_launches", states, 0.01, a.reps, dev, stream)
    out_nodes = st.prepare_crops(2 if a.small else 14)
    crop_ms = timed(st.crop, a.reps, stream)
    r.update({"crop_targets": len(st.h_picks), "crop_output_nodes": out_nodes, "crop_ms": crop_ms[0], "crop_runs_ms": crop_ms[1],
              "crop_hbm_bound_ms": out_nodes * CROP_BYTES / HBM_PEAK * 1e3})
    out.append(r)
    singles = [Steps([s], 0.01, dev) for s in states]
    l_ms = timed(lambda: [s.label() for s in singles], a.reps, stream)
    for s in singles:
        s.layout()
    f_ms = timed(lambda: [s.fill() for s in singles], a.reps, stream)
    out.append({"shape": f"b_{many}_volumes_as_{many}_single_calls", "volumes": many, "label_ms": l_ms[0], "label_runs_ms": l_ms[1], "records_ms": f_ms[0],
                "records_runs_ms": f_ms[1]})
    res = {"library": Path(_lib.LIB_PATH).name, "device": _lib.device_arch(), "date": time.strftime("%Y-%m-%d"), "reps": a.reps, "rehearsal": bool(a.small),
           "hbm_peak_bytes_per_s": HBM_PEAK, "bytes_per_node": {"label": LABEL_BYTES, "records": RECORD_BYTES, "crop_output_node": CROP_BYTES},
           "single_runs": ["scipy_label_find_objects_cpu_ms_one_run"], "shapes": out}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in s.items() if not k.endswith("_runs_ms")} for s in out]))


if __name__ == "__main__":
    main()
