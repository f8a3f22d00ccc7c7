"""The cases the TSDF tests share (tests/test_tsdf_cpu.py, tests/test_gpu_tsdf.py, tests/fuzz/fuzz_tsdf.py), built on
tests/fusion_cases.py: the edges of the integrate rule as one ragged batch with the pairs (D, W) written out by hand, the ragged
batch over the scene's images, and the sphere scene with its noisy frames.  Everything is computed once per process
(functools.lru_cache) and never changed."""
from __future__ import annotations

import functools

import numpy as np

from tests import fusion_cases as FC

RAGGED, RAGGED_RANGES, RAGGED_RADIUS = FC.RAGGED, FC.RAGGED_RANGES, FC.RAGGED_RADIUS  # 3 072, 765 and 910 nodes
RAGGED_WEIGHTS, RAGGED_WMAX = (1.0, 0.5, 2.0), 3.0
TRUNC, MIN_WEIGHT = 3 * FC.DELTA, 1.0  # the scene: three voxels
TRUNC_EXACT = 2.0 ** -5  # a truncation that float32 holds exactly: a node that only ever saw free space is saturated, |D| / trunc == 1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# The edges of the rule as ONE ragged batch.  The set-ups are FC.EDGE_CASES' (their volumes, view ranges, the three images of
# 2 x 4 and the three views: 0 and 1 the identity camera with fx = fy = 1, cx = cy = 0, view 2 with fx = fy = 2, cx = 1 standing
# 1 behind the origin), near = 1.0, and trunc = 0.5 in place of the band.  Three more views of the identity camera: view 3 reads
# image 1 again with the weight 0, view 4 reads it with the weight 2, view 5 reads an image of 3.25 everywhere with the weight
# 2.  wmax = 2.5.  Every coordinate, depth, weight and quotient below is exact in binary.
# Image 1 holds d = 3 at row 1, column 0, where the nodes with x = 0, y = 2.5 and z from 2.25 to 4 fall.
# ---------------------------------------------------------------------------------------------------------------------
EDGE_TRUNC, EDGE_NEAR, EDGE_WMAX = 0.5, FC.EDGE_NEAR, 2.5
EDGE_WEIGHTS = np.array([1.0, 1.0, 1.0, 0.0, 2.0, 2.0])
EDGE_DEPTH = np.concatenate([FC.EDGE_DEPTH, FC.EDGE_DEPTH[1:2], FC.EDGE_DEPTH[1:2], np.full((1, 2, 4), 3.25)])
_T = EDGE_TRUNC
_COLUMNS_D, _COLUMNS_W = [0.0] + [_T] * 8 + [0.0, 0.0], [0.0] + [1.0] * 8 + [0.0, 0.0]
_PAIR = ((0.0, 2.5, 2.75), 0.5, "node", (1, 1, 2))  # z = 2.75 and 3.25 under d = 3: s = 0.25 and -0.25
# (what it is about, volume, view range, D, W)
EDGE_CASES = tuple((c[0], c[1], c[2], d, w) for c, (d, w) in zip(FC.EDGE_CASES, (
    ([0.0, 0.0, _T], [0.0, 0.0, 1.0]),                                                # z at near says nothing; +inf gives trunc
    (_COLUMNS_D, _COLUMNS_W),                                                         # pixel -0.5 inside, W - 0.5 outside
    ([0.0, _T, _T, _T, _T, 0.0], [0.0, 1.0, 1.0, 1.0, 1.0, 0.0]),                     # rows alike
    (_COLUMNS_D, _COLUMNS_W),                                                         # voxel centres
    ([0.0, 0.0, 0.0, _T], [0.0, 0.0, 0.0, 1.0]),                                      # NaN, 0, negative: nothing; +inf: trunc
    # z = 2.25 .. 3.75 under d = 3: s = 0.75 (cut to trunc), 0.5 (s exactly trunc), 0.25, 0, -0.25, -0.5 (s exactly -trunc
    # updates), -0.75 (nothing)
    ([_T, _T, 0.25, 0.0, -0.25, -_T, 0.0], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0]),
    # views 0 (+inf: t = 0.5) and 1 (d = 3): z = 3 averages (0.5 + 0) / 2; z = 4 lies 1 behind the surface of view 1
    ([0.25, _T], [2.0, 1.0]),
    # the moved camera: z_cam = 2, columns 0, 1, 1, 2, 2 of image 2 (inf, 3, 2): s = inf, 1, 1, 0, 0
    ([_T, _T, _T, 0.0, 0.0], [1.0] * 5),
    ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0]),                                               # an empty view range
))) + (
    # z = 3.5 is s = -trunc exactly; one step of 2^-40 further it is behind the truncation
    ("s exactly -trunc updates, just below it does not", ((0.0, 2.5, 3.5), 2.0 ** -40, "node", (1, 1, 2)), (1, 1), [-_T, 0.0], [1.0, 0.0]),
    # view 3 has the weight 0 and says nothing; view 4 has the weight 2: D = (0 * 0 + 2 * s) / 2
    ("a weight of 0 says nothing, a weight of 2 counts twice", _PAIR, (3, 2), [0.25, -0.25], [2.0, 2.0]),
    # views 4 and 5 (d = 3.25: s = 0.5 and 0), both of weight 2: D = (2 * 0.25 + 2 * 0.5) / 4 and (2 * -0.25 + 2 * 0) / 4, W = 4 cut to wmax
    ("two weighted views average and the cap is reached", _PAIR, (4, 2), [0.375, -0.125], [EDGE_WMAX, EDGE_WMAX]),
)


def edge_views():
    return np.concatenate([FC.edge_views(), np.stack([FC.view()] * 3)])


def edge_batch():
    """(volumes, view ranges, the answers D and W back to back)"""
    return ([c[1] for c in EDGE_CASES], [c[2] for c in EDGE_CASES], np.concatenate([c[3] for c in EDGE_CASES]).astype(np.float32),
            np.concatenate([c[4] for c in EDGE_CASES]).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# the sphere scene (FC: 32 x 32 x 24 at 1 cm, three 64 x 48 cameras), its noisy frames, and the same cameras without the sphere
# ---------------------------------------------------------------------------------------------------------------------
NOISE = ((0.0, 1), (0.001, 4), (0.003, 8))  # (sigma, frames): seeds 0 .. 3 where sigma > 0
SEEDS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def scene_frames(sigma, frames, seed):
    """depth [3 * frames, H, W] (Gaussian noise of `sigma` on the finite pixels of FC.scene_depth(), frame after frame), the
    view rows [3 * frames, 16]."""
    t, views = FC.scene_depth()
    rng = np.random.default_rng(seed)
    depth = np.concatenate([np.where(np.isfinite(t), t + sigma * rng.standard_normal(t.shape), t) for _ in range(frames)]) if sigma > 0 else np.tile(t, (frames, 1, 1))
    return depth, np.tile(views, (frames, 1))


@functools.lru_cache(maxsize=None)
def scene_depth_without_sphere():
    """What the three cameras see once the sphere is gone: the slab alone."""
    from omg_planner_amd import camera
    meshes, inst, begin, cams = FC.scene_records()
    keep = np.concatenate([inst[int(begin[s]) + 1: int(begin[s + 1])] for s in range(3)])  # (instance 0 of every scene is the sphere)
    t, _, _ = camera.render_depth(meshes, keep, np.arange(4, dtype=np.int64), cams, FC.H, FC.W)
    return t


def sphere_rms(volume):
    """(rms distance to the analytic sphere, count) of the vertices of scenes.surface_nets of `volume` [X,Y,Z] with z > 0.08 that
    lie within 2.5 delta of the sphere: the upper half of the observed sphere."""
    from omg_planner_amd import scenes
    v, _, _ = scenes.surface_nets(np.asarray(volume, np.float32), np.array(FC.ORIGIN), FC.DELTA, "centre", 0.0)
    dist = np.linalg.norm(v - FC.SPHERE_C, axis=1) - FC.SPHERE_R
    sel = (v[:, 2] > 0.08) & (np.abs(dist) < 2.5 * FC.DELTA)
    return float(np.sqrt(np.mean(dist[sel] ** 2))), int(sel.sum())


@functools.lru_cache(maxsize=None)
def scene_pairs(num_views=3, trunc=TRUNC):
    from omg_planner_amd import tsdf
    t, views = FC.scene_depth()
    return tsdf.integrate([FC.SCENE_VOLUME], views, [(0, num_views)], t, trunc, FC.NEAR)


@functools.lru_cache(maxsize=None)
def scene_volume(unknown_occupied=True):
    from omg_planner_amd import tsdf
    t, views = FC.scene_depth()
    return tsdf.fuse([FC.SCENE_VOLUME], views, [(0, 3)], t, TRUNC, FC.NEAR, FC.RADIUS, unknown_occupied, MIN_WEIGHT)[0].data
