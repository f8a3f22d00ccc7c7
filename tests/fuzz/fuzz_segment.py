"""Randomised differential test (GPU vs the numpy specification) of omgx_label_components / omgx_component_records /
omgx_component_states, integer for integer: ops.label_components and ops.component_states against segmentation.py on random
ragged batches: 1..4 volumes with dims 1..24 (ones included) or one long thin one, foreground densities from 0 to 1, states
that also hold values above 2, the three connectivities, the three select values, states at offsets with gaps between guard
bytes, picks in both modes with offsets that hang over the grid.  draw() needs neither torch nor a GPU; torch and ops are
imported inside main.

    python tests/fuzz/fuzz_segment.py [trials] [seed]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from omg_planner_amd import segmentation as sg

GUARD_STATE, GUARD_OUT = 1, 0xAB  # (the guard between the states is SURFACE: it must not be labelled)
DENSITIES = (0.0, 0.05, 0.15, 0.31, 0.5, 0.8, 1.0)
SMOKE_SEED, SMOKE_TRIALS = 1806, 24  # the short run of the test suite


def draw(rng):
    M = int(rng.integers(1, 5))
    volumes, begin, parts, at = [], [], [], int(rng.integers(0, 5))
    parts.append(np.full(at, GUARD_STATE, np.uint8))
    for m in range(M):
        kind = rng.random()
        if kind < 0.15:
            dims = tuple(int(d) for d in rng.permutation([int(rng.integers(300, 1400)), 1, int(rng.integers(1, 3))]))
        elif kind < 0.4:
            dims = tuple(int(d) for d in np.where(rng.random(3) < 0.5, 1, rng.integers(1, 25, 3)))
        else:
            dims = tuple(int(d) for d in rng.integers(1, 25, 3))
        density = DENSITIES[int(rng.integers(len(DENSITIES)))]
        fg = rng.random(dims) < density
        s = np.where(fg, 1, rng.choice(np.array([0, 0, 2, 2, 3, 255], np.uint8), size=dims)).astype(np.uint8)
        volumes.append((rng.normal(scale=0.1, size=3), float(rng.uniform(0.004, 0.02)), "centre" if rng.random() < 0.5 else "node", dims))
        begin.append(at)
        gap = int(rng.integers(0, 5))
        parts += [s.ravel(), np.full(gap, GUARD_STATE, np.uint8)]
        at += s.size + gap
    return dict(volumes=volumes, begin=np.array(begin, np.int64), state=np.concatenate(parts), select=int(rng.integers(1, 4)),
                connectivity=int(sg.CONNECTIVITIES[int(rng.integers(3))]), pick_seed=int(rng.integers(1 << 30)))


def draw_picks(c, comp_begin, records):
    """Picks for a drawn case once its components are known -> (picks [K,8] int32, out_volumes, out_begin)."""
    rng = np.random.default_rng(c["pick_seed"])
    picks, outs = [], []
    for m, v in enumerate(c["volumes"]):
        n = int(comp_begin[m + 1] - comp_begin[m])
        for _ in range(int(rng.integers(0, 3)) if n else 0):
            row = int(comp_begin[m]) + int(rng.integers(n))
            if rng.random() < 0.5:
                origin, delta, dims, first = sg.crop_layout(v, records[row], int(rng.integers(0, 4)))
            else:
                dims, first = tuple(int(x) for x in rng.integers(1, 9, 3)), tuple(int(x) for x in rng.integers(-4, 5, 3) + rng.integers(0, 2, 3) * (np.array(v[3]) - 3))
                origin, delta = (0.0, 0.0, 0.0), v[1]
            picks.append((m,) + tuple(first) + (row, int(rng.integers(2)), 0, 0))
            outs.append((origin, delta, "centre", dims))
    sizes = [int(np.prod(o[3])) for o in outs]
    gaps = rng.integers(0, 4, len(outs) + 1)
    begin = (np.cumsum(np.concatenate([[0], sizes]))[:-1] + np.cumsum(gaps)[:-1]).astype(np.int64) if outs else np.zeros(0, np.int64)
    return np.array(picks, np.int32).reshape(-1, 8), outs, begin


def specification(c):
    """-> (labels, comp_begin, records, picks, out_volumes, out_begin, cropped states between GUARD_OUT)."""
    labels = sg.label_components(c["state"], c["volumes"], c["select"], c["connectivity"], state_begin=c["begin"])
    comp_begin, records = sg.component_records(labels, c["volumes"], c["begin"])
    picks, outs, ob = draw_picks(c, comp_begin, records)
    want = sg.component_states(c["state"], c["volumes"], c["begin"], labels, comp_begin, records, picks, outs, ob)
    inside = np.zeros(len(want), bool)
    for k, o in enumerate(outs):
        inside[int(ob[k]): int(ob[k]) + int(np.prod(o[3]))] = True
    want[~inside] = GUARD_OUT
    return labels, comp_begin, records, picks, outs, ob, want


def check(c, torch, ops, dev):
    """-> (errors, nodes compared)."""
    labels, comp_begin, records, picks, outs, ob, want = specification(c)
    state = torch.from_numpy(c["state"]).to(dev) if len(c["state"]) else torch.zeros(1, dtype=torch.uint8, device=dev)
    comps = ops.label_components(state, c["begin"], c["volumes"], c["select"], c["connectivity"])
    torch.cuda.synchronize()
    what = f"(dims {[v[3] for v in c['volumes']]}, select {c['select']}, connectivity {c['connectivity']})"
    errs = []
    got = comps.labels.cpu().numpy()[: len(labels)]
    if not np.array_equal(got, labels):
        errs.append(f"labels differ at {np.flatnonzero(got != labels)[:8].tolist()} {what}")
    if not np.array_equal(comps.comp_begin, comp_begin) or not np.array_equal(comps.records, records):
        errs.append(f"records differ {what}")
    if not errs and len(picks):
        out = torch.full((len(want),), GUARD_OUT, dtype=torch.uint8, device=dev)
        ops.component_states(state, comps, picks, outs, ob, out=out)
        torch.cuda.synchronize()
        if not np.array_equal(out.cpu().numpy(), want):
            errs.append(f"cropped states differ at {np.flatnonzero(out.cpu().numpy() != want)[:8].tolist()} {what}")
    return errs, int(sum(np.prod(v[3]) for v in c["volumes"]))


def main(trials=None, seed=None):
    import torch
    from omg_planner_amd import ops
    trials = int(trials if trials is not None else (sys.argv[1] if len(sys.argv) > 1 else 30))
    seed = int(seed if seed is not None else (sys.argv[2] if len(sys.argv) > 2 else 0))
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda:0")
    bad, total, t0 = 0, 0, time.time()
    for k in range(trials):
        c = draw(rng)
        try:
            errs, n = check(c, torch, ops, dev)
        except Exception as e:  # noqa: BLE001
            # not a mismatch: the device may have faulted, so nothing more is started on it
            print(f"trial {k}: STOP exception {type(e).__name__}: {e}; {trials - k - 1} trials not run", flush=True)
            return 2
        total += n
        if errs:
            bad += 1
            print(f"trial {k}: FAIL " + "; ".join(errs), flush=True)
    print(f"{trials - bad}/{trials} trials agree; {total} nodes compared; seed {seed}; {time.time() - t0:.0f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
