"""Volumes, tables and clouds at the sizes the shipped workloads have (test_scale_cpu.py, test_gpu_scale.py): large enough that
the outer loops of k_surface_scan (256 workgroup totals per pass, a carry between passes: more than 65 536 samples),
k_region_maxabs (1 024 blocks: more than 262 144 voxels), k_region_boxes (2 048 blocks: more than 524 288 voxels) and
k_point_cloud_sdf (tiles of 1 024 points) take a second pass.  Every case is built here by name, deterministically and once; the
specification's answers (scenes.surface_nets, scenes.pack_table, scenes.point_cloud_sdf) are computed once per case and never
written to."""
from __future__ import annotations

import functools

import numpy as np

from tests import surface_cases as SC

BLOCK = SC.BLOCK            # samples per workgroup of the surface kernels
PASS = 256                  # workgroup totals k_surface_scan takes per pass
MAXABS_CAP = 1024 * 256     # voxels k_region_maxabs covers before its grid-stride loop repeats
BOXES_CAP = 2048 * 256      # voxels k_region_boxes covers before its wave-stride loop repeats
CLOUD_TILE = 1024           # PCS_TILE


# ---------------------------------------------------------------------------------------------------------------------
# surface volumes (specification: scenes.surface_nets)
# ---------------------------------------------------------------------------------------------------------------------
def _plane(dims, delta=0.01):
    x, y, _ = SC.positions(dims, np.zeros(3), delta, "centre")
    return SC._case(0.6 * (x - 0.223) + 0.8 * (y - 0.2017), np.zeros(3), delta)


def _sdf_sphere(dims):
    from omg_planner_amd import scenes
    g = scenes.sphere_sdf(0.1, dims, 0.6 / 64)
    return SC._case(g.data, g.origin, g.delta)


def _dense(dims=(3, 3, 300)):
    i, j, k = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    return SC._case(np.where((i + j + k) % 2 == 0, -0.01, 0.01), np.zeros(3))


@functools.lru_cache(maxsize=None)
def case(name):
    table = {
        "s256": lambda: SC._small_sphere((64, 32, 32), 0.1),   # 256 workgroups: one full pass, no carry
        "s275": lambda: _plane((44, 40, 40)),                  # 275: the second pass holds 19 entries
        "s513": lambda: _sdf_sphere((48, 48, 57)),             # 513: the third pass holds one entry
        "s1024": lambda: _sdf_sphere((64, 64, 64)),            # four full passes
        "dense": _dense,                                       # every cell active, every edge crossing
    }
    c = table[name]()
    c["data"].setflags(write=False)
    return c


SURFACE = ("s256", "s275", "s513", "s1024", "dense")
WORKGROUPS = {"s256": 256, "s275": 275, "s513": 513, "s1024": 1024, "dense": 11}


def nets(c, level=0.0):
    from omg_planner_amd import scenes
    v, f, o = scenes.surface_nets(c["data"], c["origin"], c["delta"], c["sample"], level)
    v.setflags(write=False), f.setflags(write=False)
    return v, f, o


@functools.lru_cache(maxsize=None)
def spec(name):
    """(verts, faces, open_edges) of scenes.surface_nets at level 0; `name` from SURFACE or from surface_cases."""
    return nets(case(name) if name in SURFACE else SC.case(name))


def active_cell_ids(data, level=0.0):
    """The x-major sample index of every active cell (corner mask neither 0 nor 255), ascending: vertex v belongs to cell ids[v]."""
    ins = np.asarray(data, np.float32) < np.float32(level)
    n = ins.shape
    c = tuple(d - 1 for d in n)
    n_in = sum(ins[dx: dx + c[0], dy: dy + c[1], dz: dz + c[2]].astype(np.int32) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    i, j, k = np.nonzero((n_in > 0) & (n_in < 8))
    return (i.astype(np.int64) * n[1] + j) * n[2] + k


# ---------------------------------------------------------------------------------------------------------------------
# region volumes for the single fit (specification: scenes.pack_table(tight=True))
# ---------------------------------------------------------------------------------------------------------------------
REGION_DIMS, REGION_DELTA = (128, 96, 48), 1.5 / 128
THRESHOLDS = ((0.2, 0.01), (0.1, 0.0))


def _ball(centre_vox):
    """float32 distance from every voxel centre to `centre_vox` (voxel units), minus 0.05."""
    ax = [(np.arange(d, dtype=np.float64) + 0.5 - c) * REGION_DELTA for d, c in zip(REGION_DIMS, centre_vox)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - 0.05).astype(np.float32)


def _r_tail():
    d = _ball((30.3, 40.2, 20.7))
    d[-1, -1, -1] = 40.0
    return d


@functools.lru_cache(maxsize=None)
def region(name):
    """-> SdfGrid."""
    from omg_planner_amd import scenes
    if name == "r_table":
        g = scenes.box_sdf((0.6, 0.4, 0.02), (128, 96, 32), 1.5 / 128)
    else:
        data = {"r_high": lambda: _ball((121.3, 40.2, 20.7)), "r_tail": _r_tail}[name]()
        g = scenes.SdfGrid(data, -0.5 * REGION_DELTA * np.array(REGION_DIMS, np.float64), REGION_DELTA)
    g.data.setflags(write=False)
    return g


REGION_CASES = (("r_high", 0), ("r_tail", 0), ("r_table", 0), ("r_table", 1))  # (volume, index into THRESHOLDS)


def one_object_kwargs(eps, clr):
    return dict(epsilon=eps, target_epsilon=eps, clearance=clr, target_clearance=clr)


@functools.lru_cache(maxsize=None)
def region_spec(name, which):
    """The record scenes.pack_table(tight=True) writes for a scene that holds only this volume."""
    from omg_planner_amd import scenes
    scene = scenes.Scene([scenes.SceneObject("obj", np.eye(4), region(name))], 0)
    rec = scenes.pack_table([scene], one_object_kwargs(*THRESHOLDS[which]), tight=True).objects[0].copy()
    rec.setflags(write=False)
    return rec


def rbox(data, which=0):
    """scenes.influence_rbox of a REGION_DIMS volume with the voxel extents its record has -> (c, h, R)."""
    from omg_planner_amd import scenes
    lo, hi = scenes.grid_limits(region("r_high").origin, data.shape, REGION_DELTA)
    vox = ((hi - lo) / np.array(data.shape, np.float32)).astype(np.float64)
    return scenes.influence_rbox(data, *THRESHOLDS[which], vox)


# ---------------------------------------------------------------------------------------------------------------------
# the mixed table for the batched fit (specification: scenes.pack_table(ragged=True))
# ---------------------------------------------------------------------------------------------------------------------
MIXED_KW = {
    "tabletop": dict(epsilon=0.2, target_epsilon=0.1, clearance=0.01, target_clearance=0.0),
    "targets_only": dict(epsilon=1.5, target_epsilon=0.1, clearance=0.01, target_clearance=0.0),  # only the two targets are culled
}
SCENE0 = ("noise", "far", "weird", "flat", "two", "sph", "sph_copy", "sph_off", "sph_d", "r_table")
SCENE1 = ("sph_copy", "far", "weird", "sph")
TARGET = {0: "sph", 1: "sph_copy"}


@functools.lru_cache(maxsize=None)
def mixed_volumes():
    """name -> SdfGrid; one object per name, so a name that occurs in two scenes is the same ndarray in both."""
    from omg_planner_amd import scenes as sc
    rng = np.random.RandomState(11)
    out = {"noise": sc.SdfGrid(rng.uniform(-0.05, 0.6, size=(24, 20, 28)).astype(np.float32), np.array([-0.2, 0.1, 0.0]), 0.02),
           "far": sc.SdfGrid(np.full((12, 12, 12), 0.9, np.float32), np.zeros(3), 0.05)}
    weird = rng.uniform(0.0, 0.5, size=(16, 16, 16)).astype(np.float32)
    weird[3, 4, 5], weird[9, 9, 9], weird[0, 0, 0] = np.inf, np.nan, -np.inf
    out["weird"] = sc.SdfGrid(weird, np.array([0.1, 0.1, 0.1]), 0.03)
    out["flat"] = sc.SdfGrid(rng.uniform(-0.05, 0.3, size=(1, 9, 7)).astype(np.float32), np.zeros(3), 0.02)
    out["two"] = sc.SdfGrid(rng.uniform(-0.05, 0.3, size=(2, 2, 2)).astype(np.float32), np.array([0.0, -0.1, 0.2]), 0.04)
    sph = sc.sphere_sdf(0.07, (40, 40, 40), 0.6 / 40)
    out["sph"] = sph
    out["sph_copy"] = sc.SdfGrid(sph.data.copy(), sph.origin.copy(), sph.delta)
    off = sph.data.copy()
    off[0, 0, 0] = np.nextafter(off[0, 0, 0], np.float32(np.inf))  # a corner voxel, out of every threshold's reach
    out["sph_off"] = sc.SdfGrid(off, sph.origin.copy(), sph.delta)
    out["sph_d"] = sc.SdfGrid(sph.data.copy(), sph.origin.copy(), sph.delta * 1.25)
    out["r_table"] = region("r_table")
    for g in out.values():
        g.data.setflags(write=False)
    return out


def mixed_scenes(private: bool = False):
    """Three scenes: SCENE0, SCENE1 and an empty one.  private: every object gets a copy of its volume of its own."""
    from omg_planner_amd import scenes as sc
    vols = mixed_volumes()

    def obj(k, name):
        g = vols[name]
        if private:
            g = sc.SdfGrid(g.data.copy(), np.array(g.origin, np.float64), g.delta)
        return sc.SceneObject(name, sc._yaw_pose(0.3 + 0.05 * k, -0.2 + 0.04 * k, 0.1 + 0.01 * k, 0.3 * k), g)
    return [sc.Scene([obj(k, n) for k, n in enumerate(SCENE0)], SCENE0.index(TARGET[0])),
            sc.Scene([obj(k + 3, n) for k, n in enumerate(SCENE1)], SCENE1.index(TARGET[1])),
            sc.Scene([], 0)]


_FITS = {}  # kw name -> the cache of scenes.tighten_far_boxes: one host fit per distinct key, shared by both layouts


@functools.lru_cache(maxsize=None)
def mixed_spec(kw_name, share: bool = True):
    """(SceneBatch, distinct fit keys) of the mixed table: the loose table of scenes.pack_table, then scenes.tighten_far_boxes with a
    cache whose keys are counted — what pack_table(tight=True) does (test_scale_cpu.py asserts the two are equal)."""
    from omg_planner_amd import scenes as sc
    batch = sc.pack_table(mixed_scenes(private=not share), MIXED_KW[kw_name], ragged=True, share_grids=share, tight=False)
    cache = _FITS.setdefault(kw_name, {})
    sc.tighten_far_boxes(batch.objects, batch.pool, cache)
    batch.objects.setflags(write=False), batch.pool.setflags(write=False)
    return batch, len(cache)


REGION_FIELDS = ("rb_c", "rb_h", "rb_r", "rb_r2")


# ---------------------------------------------------------------------------------------------------------------------
# clouds (specification: scenes.point_cloud_sdf)
# ---------------------------------------------------------------------------------------------------------------------
CLOUD_SIZES = (1023, 1024, 1025, 2500)
CLOUD_RES, CLOUD_MARGIN = 0.02, 0.1


@functools.lru_cache(maxsize=None)
def cloud(n):
    """n points uniform in a 0.3 m box, the LAST one moved 0.5 m out along +x: the nodes around it have their nearest point at the
    end of the final tile.  At resolution 0.02 with a margin of 0.1 the grid is 50 x 25 x 25 nodes."""
    p =np.random.default_rng(n).uniform([0.3, -0.15, 0.0], [0.6, 0.15, 0.3], size=(n, 3))
    p[-1, 0] += 0.5
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def cloud_spec(n):
    from omg_planner_amd import scenes
    g = scenes.point_cloud_sdf(cloud(n), CLOUD_RES, CLOUD_MARGIN)
    g.data.setflags(write=False)
    return g
