"""Cases shared by the CPU and the GPU tests of support-plane fitting (omg-planner_amd/planes.py, csrc/omg_plane.hip): analytic
depth images of planes (ray-plane intersection in float64), named batches of views at the sizes where the kernels' loops can go
wrong, half-space volumes, and the triples and noise of the observed scene of tests/segment_cases.py."""
from __future__ import annotations

import functools

import numpy as np

from tests import fusion_cases as FC
from tests import segment_cases as SC

CHUNK = 2048  # OMGX_PLANE_PIXELS_PER_WORKGROUP (test_plane_cpu.py asserts it is the header's)
STAGE = 64    # OMGX_PLANE_STAGE_HYPOTHESES
INF, NAN = float("inf"), float("nan")
OBSERVED_K = 256
SIGMA = 0.001  # the depth noise of the observed scene, metres


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def unit_plane(normal, point):
    """(n, off) with |n| = 1 through `point`, the normal facing the camera at the origin (off >= 0)."""
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    off = -float(n @ np.asarray(point, np.float64))
    return np.concatenate([-n, [-off]]) if off < 0 else np.concatenate([n, [off]])


def analytic_depth(intr, H, W, plane):
    """The depth image of a plane: the ray (dx, dy, 1) d meets n.p + off = 0 at d = -off / ((n0*dx + n1*dy) + n2); +inf where
    the ray runs away from it."""
    fx, fy, cx, cy = intr
    r, c = np.divmod(np.arange(H * W), W)
    dx, dy = (c - cx) / fx, (r - cy) / fy
    den = plane[0] * dx + plane[1] * dy + plane[2]
    with np.errstate(all="ignore"):
        d = -plane[3] / den
    return np.where(d > 0, d, INF).reshape(H, W)


def nearer(*images):
    return np.minimum.reduce(images)


INTR = (80.0, 80.0, 31.5, 23.5)
TILTED = unit_plane((0.1, 0.5, -1.0), (0.0, 0.0, 0.7))
FLOOR = unit_plane((0.0, -1.0, -0.35), (0.0, 0.25, 0.8))  # seen from above at a slant: the lower rows of the image
WALL = unit_plane((0.0, 0.0, -1.0), (0.0, 0.0, 1.0))      # faces the camera


def floor_and_wall(H=48, W=64, intr=INTR):
    """One image of a floor and a larger wall behind it -> (depth, floor pixels, wall pixels)."""
    f, w = analytic_depth(intr, H, W, FLOOR), analytic_depth(intr, H, W, WALL)
    d = nearer(f, w)
    return d, f < w, w <= f


def _triples(rng, V, K, pixels):
    return rng.integers(0, pixels, (V, K, 3)).astype(np.int32)


def _spoil(rng, depth, outliers=0.05, holes=0.05):
    """Outliers in front of the surface, holes (+inf), and one each of NaN, 0 and a negative depth."""
    d = depth.copy()
    flat = d.reshape(-1)
    n = flat.size
    idx = rng.permutation(n)
    a, b = int(outliers * n), int(holes * n)
    flat[idx[:a]] *= rng.uniform(0.5, 0.95, a)
    flat[idx[a: a + b]] = INF
    flat[idx[a + b]], flat[idx[a + b + 1]], flat[idx[a + b + 2]] = NAN, 0.0, -0.5
    return d


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(intr [V,4], depth [V,H,W], triples [V,K,3], tol, min_nn, skip, up, cos_min): one batch of views each.
      tilted      48 x 64 (a chunk and a half), K = 63, one clean plane: the known answer
      small       30 x 40 (one partial chunk), K = 1
      odd         67 x 131 = 8 777 pixels (more than four chunks, a multiple of neither 256 nor the chunk), K = 65, outliers,
                  holes, NaN, 0 and a negative depth, a skip mask, different cameras per view, V = 3 with one all-background view
      stage       48 x 64, K = one more than the LDS staging block, floor and wall with a prior, V = 2
      big_k       30 x 40, K = 300 (five staging blocks, the last partial) with many void rows"""
    rng = np.random.default_rng(19)
    out = {}
    d = analytic_depth(INTR, 48, 64, TILTED)[None]
    out["tilted"] = dict(intr=np.array([INTR]), depth=d, triples=_triples(rng, 1, 63, 48 * 64), tol=1e-9, min_nn=1e-10, skip=None, up=None, cos_min=-1.0)
    d = analytic_depth((50.0, 55.0, 19.0, 15.5), 30, 40, TILTED)[None]
    out["small"] = dict(intr=np.array([(50.0, 55.0, 19.0, 15.5)]), depth=d, triples=_triples(rng, 1, 1, 1200), tol=1e-9, min_nn=0.0, skip=None, up=None,
                        cos_min=-1.0)
    H, W = 67, 131
    intr = np.array([(120.0, 118.0, 65.0, 33.0), (100.0, 100.0, 60.5, 30.5), (90.0, 95.0, 70.0, 40.0)])
    pl = [unit_plane((0.2, 0.6, -1.0), (0.0, 0.1, 0.9)), None, unit_plane((-0.3, 0.4, -1.0), (0.05, 0.0, 1.2))]
    depth = np.stack([np.full((H, W), INF) if p is None else _spoil(rng, analytic_depth(intr[v], H, W, p)) for v, p in enumerate(pl)])
    skip = rng.random((3, H, W)) < 0.1
    out["odd"] = dict(intr=intr, depth=depth, triples=_triples(rng, 3, 65, H * W), tol=0.002, min_nn=1e-10, skip=skip, up=None, cos_min=-1.0)
    fw, _, _ = floor_and_wall()
    depth = np.stack([fw, _spoil(rng, fw)])
    up = np.stack([FLOOR[:3], FLOOR[:3]])
    out["stage"] = dict(intr=np.array([INTR, INTR]), depth=depth, triples=_triples(rng, 2, STAGE + 1, 48 * 64), tol=0.001, min_nn=1e-10, skip=None, up=up,
                        cos_min=0.9)
    d = _spoil(rng, analytic_depth((50.0, 55.0, 19.0, 15.5), 30, 40, TILTED), 0.1, 0.4)[None]
    out["big_k"] = dict(intr=np.array([(50.0, 55.0, 19.0, 15.5)]), depth=d, triples=_triples(rng, 1, 300, 1200), tol=0.001, min_nn=1e-9, skip=None, up=None,
                        cos_min=-1.0)
    return out


def arguments(case):
    return (case["intr"], case["depth"], case["triples"]), dict(min_nn=case["min_nn"], skip=case["skip"], up=case["up"], cos_min=case["cos_min"])


# half-space volumes: dims of one, both sample kinds, more than one workgroup; the planes in the grids' frames
VOLUMES = [((-0.16, -0.16, -0.04), 0.02, "centre", (16, 16, 12)), ((-0.1, -0.12, 0.0), 0.013, "node", (17, 9, 5)), ((0.0, 0.0, 0.0), 0.05, "centre", (1, 1, 1)),
           ((0.3, -0.2, 0.1), 0.01, "node", (1, 7, 300)), ((0.0, 0.1, -0.3), 0.007, "centre", (9, 1, 29))]
VOLUME_PLANES = np.array([unit_plane((0.0, 0.0, 1.0), (0.0, 0.0, 0.01)), unit_plane((0.3, -0.2, 1.0), (0.0, 0.0, 0.02)), (1.0, 0.0, 0.0, 0.0),
                          unit_plane((0.0, 1.0, 0.2), (0.3, -0.18, 0.5)), (0.0, -0.6, 0.8, 0.25)])
POOL_GUARD = 7  # elements between the volumes in the pool


def pool_layout():
    """(volumes with their element offsets, pool size): the volumes with POOL_GUARD elements before, between and after them."""
    at, out = POOL_GUARD, []
    for v in VOLUMES:
        out.append(v + (at,))
        at += int(np.prod(v[3])) + POOL_GUARD
    return out, at


# ---------------------------------------------------------------------------------------------------------------------
# the observed scene of segment_cases: a sphere and a box on a slab whose top is z = SLAB_TOP in the world
# ---------------------------------------------------------------------------------------------------------------------
SLAB_TOP = SC.SLAB_HALF[2]


def observed_intrinsics():
    return np.asarray(FC.scene_cameras()[1], np.float64).reshape(4)


@functools.lru_cache(maxsize=None)
def observed_triples(seed=0, K=OBSERVED_K):
    from omg_planner_amd import planes
    return planes.draw_triples(FC.H, FC.W, K, np.random.default_rng(seed), views=3)


def noisy_depth(seed):
    """observed_depth's images with Gaussian noise of SIGMA on the finite pixels."""
    t = SC.observed_depth()[0]
    rng = np.random.default_rng(1000 + seed)
    return np.where(np.isfinite(t), t + SIGMA * rng.standard_normal(t.shape), t)


def plane_in_world(plane, s):
    """A plane of camera s of the observed scene in the world frame."""
    from omg_planner_amd import planes
    return planes.plane_to_frame(plane, np.linalg.inv(FC.scene_cameras()[0][s]))
