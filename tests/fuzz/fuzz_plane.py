"""Randomised differential test (GPU vs the numpy specification) of omgx_plane_ransac / omgx_plane_moments / omgx_plane_mask /
omgx_plane_volumes, bit for bit: ops.plane_ransac, plane_moments, fit_planes, plane_mask and plane_volumes against planes.py on
random batches: 1..3 views of random sizes (one pixel to a little more than two chunks, sizes that straddle a chunk), random
cameras, planes with outliers, holes, NaNs, zeros and negative depths, all-background views, skip masks, priors, K from 1 to a
few staging blocks, and ragged volume batches with dims of one at offsets with gaps.  draw() needs neither torch nor a GPU; torch
and ops are imported inside main.

    python tests/fuzz/fuzz_plane.py [trials] [seed]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from omg_planner_amd import planes as pl

GUARD = -123.0
SMOKE_SEED, SMOKE_TRIALS = 1907, 16  # the short run of the test suite
INF, NAN = float("inf"), float("nan")


def _plane(rng):
    n = np.array([rng.normal(scale=0.4), rng.normal(scale=0.4), -1.0])
    n /= np.linalg.norm(n)
    off = -float(n @ np.array([0.0, 0.0, rng.uniform(0.4, 2.0)]))
    return np.concatenate([-n, [-off]]) if off < 0 else np.concatenate([n, [off]])


def _depth(rng, intr, H, W, plane):
    r, c = np.divmod(np.arange(H * W), W)
    den = plane[0] * ((c - intr[2]) / intr[0]) + plane[1] * ((r - intr[3]) / intr[1]) + plane[2]
    with np.errstate(all="ignore"):
        d = -plane[3] / den
    d = np.where(d > 0, d, INF)
    n = H * W
    kind = rng.random(n)
    d = np.where(kind < 0.08, d * rng.uniform(0.4, 0.97, n), d)           # outliers in front
    d = np.where((kind >= 0.08) & (kind < 0.16), INF, d)                  # holes
    d = np.where((kind >= 0.16) & (kind < 0.18), NAN, d)
    d = np.where((kind >= 0.18) & (kind < 0.19), 0.0, d)
    d = np.where((kind >= 0.19) & (kind < 0.20), -d, d)
    d = d + np.where(np.isfinite(d), rng.normal(scale=rng.choice([0.0, 0.0005]), size=n), 0.0)
    return d.reshape(H, W)


def draw(rng):
    V = int(rng.integers(1, 4))
    kind = rng.random()
    if kind < 0.2:
        H, W = 1, int(rng.integers(1, 40))
    elif kind < 0.5:
        n = pl.PIXELS_PER_WORKGROUP * int(rng.integers(1, 3)) + int(rng.integers(-3, 4))  # around a chunk border
        H = int(rng.integers(1, 60))
        W = max(1, n // H)
    else:
        H, W = int(rng.integers(2, 70)), int(rng.integers(2, 90))
    K = int(rng.choice([1, int(rng.integers(1, 64)), 63, 64, 65, int(rng.integers(65, 200))]))
    intr = np.stack([[rng.uniform(40, 200), rng.uniform(40, 200), rng.uniform(0, W), rng.uniform(0, H)] for _ in range(V)])
    truth = [_plane(rng) for _ in range(V)]
    depth = np.stack([np.full((H, W), INF) if rng.random() < 0.15 else _depth(rng, intr[v], H, W, truth[v]) for v in range(V)])
    skip = (rng.random((V, H, W)) < rng.uniform(0, 0.3)) if rng.random() < 0.5 else None
    up, cos_min = (np.stack([t[:3] for t in truth]), float(rng.uniform(0.5, 0.9999))) if rng.random() < 0.4 else (None, -1.0)
    triples = rng.integers(0, H * W, (V, K, 3)).astype(np.int32)
    if K > 1 and rng.random() < 0.5:
        triples[:, K // 2] = triples[:, 0]  # a tie
    M = int(rng.integers(1, 5))
    volumes, at = [], int(rng.integers(0, 5))
    for _ in range(M):
        dims = tuple(int(d) for d in (np.where(rng.random(3) < 0.3, 1, rng.integers(1, 20, 3)) if rng.random() < 0.8
                                      else rng.permutation([int(rng.integers(300, 900)), 1, int(rng.integers(1, 3))])))
        volumes.append((rng.normal(scale=0.1, size=3), float(rng.uniform(0.004, 0.02)), "centre" if rng.random() < 0.5 else "node", dims, at))
        at += int(np.prod(dims)) + int(rng.integers(0, 5))
    vplanes = np.stack([_plane(rng) for _ in range(M)])
    return dict(intr=intr, depth=depth, triples=triples, tol=float(rng.choice([0.0, 0.001, 0.004])), min_nn=float(rng.choice([0.0, 1e-10, 1e-6])),
                skip=skip, up=up, cos_min=cos_min, volumes=volumes, volume_planes=vplanes, pool=at)


def specification(c):
    """-> dict of everything the entry points write, from planes.py."""
    kw = dict(min_nn=c["min_nn"], skip=c["skip"], up=c["up"], cos_min=c["cos_min"])
    hyp, counts, best, best_planes, anchors = pl.ransac(c["intr"], c["depth"], c["triples"], c["tol"], **kw)
    count, sums = pl.moments(c["intr"], c["depth"], best_planes, anchors, c["tol"], c["skip"])
    fit = pl.fit_planes(c["intr"], c["depth"], c["triples"], c["tol"], refine=1, **kw)
    mask = pl.plane_mask(c["intr"], c["depth"], fit.planes, c["tol"], c["skip"])
    pool = np.full(c["pool"], GUARD, np.float32)
    for v, p in zip(c["volumes"], c["volume_planes"]):
        pool[v[4]: v[4] + int(np.prod(v[3]))] = pl.halfspace_volume(v[:4], p).ravel()
    return dict(hyp=hyp, counts=counts, best=best, best_planes=best_planes, anchors=anchors, count=count, sums=sums, final=fit.planes,
                inliers=fit.inliers, status=fit.status, mask=mask, pool=pool)


def check(c, torch, ops, dev):
    """-> (errors, pixel-hypothesis pairs compared)."""
    want = specification(c)
    depth = torch.from_numpy(c["depth"]).to(dev)
    skip = None if c["skip"] is None else torch.from_numpy(c["skip"]).to(dev)
    kw = dict(min_nn=c["min_nn"], skip=skip, up=c["up"], cos_min=c["cos_min"])
    hyp, counts, best, best_planes, anchors = ops.plane_ransac(c["intr"], depth, c["triples"], c["tol"], **kw)
    torch.cuda.synchronize()
    count, sums = ops.plane_moments(c["intr"], depth, best_planes, anchors, c["tol"], skip)
    torch.cuda.synchronize()
    fit = ops.fit_planes(c["intr"], depth, c["triples"], c["tol"], refine=1, **kw)
    mask = ops.plane_mask(c["intr"], depth, fit.planes, c["tol"], skip)
    torch.cuda.synchronize()
    pool = torch.full((c["pool"],), GUARD, dtype=torch.float32, device=dev)
    ops.plane_volumes(c["volumes"], c["volume_planes"], out=pool)
    torch.cuda.synchronize()
    what = f"(V {c['depth'].shape}, K {c['triples'].shape[1]}, tol {c['tol']}, skip {c['skip'] is not None}, up {c['up'] is not None})"
    errs = []
    f64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    for name, got, bits in (("hyp", hyp, True), ("counts", counts, False), ("best", best, False), ("best_planes", best_planes, True),
                            ("anchors", anchors, True), ("count", count, False), ("sums", sums, True), ("final", fit.planes, True),
                            ("mask", mask, False)):
        g = got.cpu().numpy()
        same = np.array_equal(f64(g), f64(want[name])) if bits else np.array_equal(g, want[name])
        if not same:
            errs.append(f"{name} differs {what}")
    if not np.array_equal(fit.inliers, want["inliers"]) or not np.array_equal(fit.status, want["status"]):
        errs.append(f"inliers or status differ {what}")
    if not np.array_equal(pool.cpu().numpy().view(np.uint32), want["pool"].view(np.uint32)):
        errs.append(f"volumes differ (dims {[v[3] for v in c['volumes']]})")
    return errs, int(c["depth"].size * c["triples"].shape[1])


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
    print(f"{trials - bad}/{trials} trials agree; {total} pixel-hypothesis pairs compared; seed {seed}; {time.time() - t0:.0f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
