"""The cases of scale_cases.py have teeth: computed from the specification alone (scenes.surface_nets, scenes.influence_rbox,
scenes.pack_table, scenes.point_cloud_sdf), each of them puts what decides its answer into the SECOND pass of the loop it is
there for — vertices and faces across the 256-total passes of k_surface_scan, the needed windows past voxel 524 288
(k_region_boxes), the largest |g| past voxel 262 144 (k_region_maxabs), the nearest point in the last tile of k_point_cloud_sdf —
so a kernel that drops that pass cannot give the specification's bits (test_gpu_scale.py compares them)."""
from __future__ import annotations

import time

import numpy as np
import pytest

from tests import scale_cases as XC
from tests import surface_cases as SC


# ---------------------------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------------------------
def _passes(name):
    """(pass of every vertex, faces that use vertices of two passes) of the case."""
    c = XC.case(name)
    v, f, _ = XC.spec(name)
    ids = XC.active_cell_ids(c["data"])
    assert len(ids) == len(v) and (np.diff(ids) > 0).all()
    p = (ids // XC.BLOCK) // XC.PASS
    fp = p[f]
    return p, int((fp.min(1) != fp.max(1)).sum())


def test_surface_cases_have_the_workgroups_they_are_named_for():
    assert XC.BLOCK == 256 == XC.PASS
    for name in XC.SURFACE:
        assert -(-XC.case(name)["data"].size // XC.BLOCK) == XC.WORKGROUPS[name], name
    assert XC.WORKGROUPS["s256"] == XC.PASS and XC.WORKGROUPS["s1024"] % XC.PASS == 0
    assert XC.WORKGROUPS["s275"] - XC.PASS == 19 and XC.WORKGROUPS["s513"] - 2 * XC.PASS == 1


@pytest.mark.parametrize("name,per_pass,straddling", [("s275", [2808, 156], 76), ("s513", [1120, 1034, 0], 172), ("s1024", [0, 1125, 1037, 0], 176)])
def test_vertices_and_faces_lie_across_the_passes_of_the_scan(name, per_pass, straddling):
    """Vertices in at least two passes (the later ones take their rows from `carry`), and faces whose corners lie in two passes
    (surf_vertex_index reads an offset another pass wrote)."""
    p, straddle = _passes(name)
    count = np.bincount(p, minlength=len(per_pass)).tolist()
    print(name, count, straddle)
    assert (np.array(count) > 0).sum() >= 2 and straddle >= 1
    assert count == per_pass and straddle == straddling   # as measured when the cases were chosen


def test_control_case_is_a_single_pass():
    p, straddle = _passes("s256")
    assert len(p) > 0 and (p == 0).all() and straddle == 0 and XC.spec("s256")[2] == 0


def test_dense_case_fills_a_workgroup_with_active_cells():
    """Workgroup 0 is samples (0, 0, 0..255): every one of them an active cell, so the ranks run to 255 and every wave's ballot is full."""
    c = XC.case("dense")
    ids = XC.active_cell_ids(c["data"])
    assert np.array_equal(ids[: XC.BLOCK], np.arange(XC.BLOCK))
    v, f, o = XC.spec("dense")
    assert (len(v), len(f), o) == (1196, 2982, 4800) and len(ids) == 2 * 2 * 299
    assert f.min() == 0 and f.max() == len(v) - 1 and np.isfinite(v).all()


# ---------------------------------------------------------------------------------------------------------------------
# single fit
# ---------------------------------------------------------------------------------------------------------------------
def test_region_volumes_cross_the_caps():
    n = int(np.prod(XC.REGION_DIMS))
    assert n == 589824 > XC.BOXES_CAP > XC.MAXABS_CAP and XC.BOXES_CAP == 524288 and XC.MAXABS_CAP == 262144
    assert XC.MAXABS_CAP < XC.region("r_table").data.size == 393216 < XC.BOXES_CAP
    assert XC.region("r_high").data.shape == XC.REGION_DIMS == XC.region("r_tail").data.shape


def test_r_high_is_decided_past_voxel_524288():
    """Without the voxels from flat index 524 288 on (0.9 there: out of reach) the fit comes out different."""
    d = XC.region("r_high").data
    cut = d.copy()
    cut.reshape(-1)[XC.BOXES_CAP:] = 0.9
    full, part = XC.rbox(d), XC.rbox(cut)
    print("r_high", full, part)
    assert full is not None and part is not None
    assert not all(np.array_equal(a, b) for a, b in zip(full, part))
    assert abs(full[0][0] - 1.4238) < 1e-3 and abs(part[0][0] - 1.2539) < 1e-3   # the centre's x, as measured


def test_r_tail_margin_is_decided_past_voxel_262144():
    """The largest |g| is the last voxel, and it moves the margin and with it R."""
    d = XC.region("r_tail").data
    assert int(np.abs(d).argmax()) == d.size - 1 >= XC.MAXABS_CAP and d.reshape(-1)[-1] == 40.0
    plain = d.copy()
    plain[-1, -1, -1] = d[-1, -1, -2]
    assert np.abs(plain).max() < 1.0 + 0.45  # the margin without the voxel: 1e-5 * max(1, max |g|), max |g| about 1.3
    with_v, without = XC.rbox(d), XC.rbox(plain)
    print("r_tail", with_v[2], without[2])
    assert with_v[2] != without[2]
    assert abs(with_v[2] - 0.24918) < 1e-4 and abs(without[2] - 0.24884) < 1e-4   # as measured


@pytest.mark.parametrize("name,which", XC.REGION_CASES)
def test_region_specifications_are_fitted(name, which):
    from omg_planner_amd import scenes
    rec = XC.region_spec(name, which)
    assert scenes.culled(rec[None])[0] and rec["rb_r2"] > 0 and rec["rb_r"] > 0
    assert tuple(rec["dim"]) == XC.region(name).data.shape and (rec["epsilon"], rec["clearance"]) == tuple(np.float32(t) for t in XC.THRESHOLDS[which])
    if name == "r_table":
        assert not np.array_equal(XC.region_spec(name, 0)["rb_r"], XC.region_spec(name, 1)["rb_r"])


# ---------------------------------------------------------------------------------------------------------------------
# batched fit
# ---------------------------------------------------------------------------------------------------------------------
def _rows(batch, scene):
    lo = int(batch.scene_begin[scene])
    return {n: batch.objects[lo + k] for k, n in enumerate((XC.SCENE0, XC.SCENE1, ())[scene])}


def _same_region(a, b):
    return all(np.array_equal(a[f], b[f]) for f in XC.REGION_FIELDS)


def test_mixed_table_tabletop_thresholds():
    from omg_planner_amd import scenes
    batch, keys = XC.mixed_spec("tabletop", True)
    assert batch.scene_begin.tolist() == [0, len(XC.SCENE0), len(XC.SCENE0) + len(XC.SCENE1), len(XC.SCENE0) + len(XC.SCENE1)]
    s0, s1 = _rows(batch, 0), _rows(batch, 1)
    culled = scenes.culled(batch.objects)
    assert [n for n, c in zip(XC.SCENE0 + XC.SCENE1, culled) if not c] == ["flat"]
    loose = scenes.pack_table(XC.mixed_scenes(), XC.MIXED_KW["tabletop"], tight=False)
    assert _same_region(s0["flat"], _rows(loose, 0)["flat"])
    assert s0["far"]["rb_r2"] == -1.0 == s1["far"]["rb_r2"]
    assert s0["sph"]["rb_r2"] != s0["sph_copy"]["rb_r2"]            # the target's thresholds and the others'
    assert _same_region(s0["sph_copy"], s0["sph_off"]) and not np.array_equal(XC.mixed_volumes()["sph_copy"].data, XC.mixed_volumes()["sph_off"].data)
    assert not _same_region(s0["sph_copy"], s0["sph_d"])            # the extent differs
    assert _same_region(s0["sph"], s1["sph_copy"]) and _same_region(s0["sph_copy"], s1["sph"])  # one key each: fitted once, copied
    # shared by identity: stored once
    for n in ("far", "weird", "sph", "sph_copy"):
        assert s0[n]["grid_offset"] == s1[n]["grid_offset"], n
    assert s0["sph"]["grid_offset"] != s0["sph_copy"]["grid_offset"]
    for n in ("noise", "weird", "two", "r_table"):
        assert s0[n]["rb_r2"] > 0 and np.isfinite(s0[n]["rb_h"]).all(), n
    # noise, far, weird, two, sph at the target's thresholds, sph at the others' (sph_copy), sph_off, sph_d, r_table
    assert keys == 9
    # the private layout: the same keys, so nothing is fitted again, and the same regions
    private, keys_p = XC.mixed_spec("tabletop", False)
    assert keys_p == keys and len(np.unique(private.objects["grid_offset"])) == len(private.objects)
    for f in XC.REGION_FIELDS:
        assert np.array_equal(private.objects[f], batch.objects[f]), f


def test_mixed_table_when_only_the_targets_are_culled():
    from omg_planner_amd import scenes
    batch, keys = XC.mixed_spec("targets_only", True)
    culled = scenes.culled(batch.objects)
    assert culled.sum() == 2 and keys == 1
    names = XC.SCENE0 + XC.SCENE1
    assert sorted(np.flatnonzero(culled).tolist()) == [XC.SCENE0.index("sph"), len(XC.SCENE0) + XC.SCENE1.index("sph_copy")]
    loose = scenes.pack_table(XC.mixed_scenes(), XC.MIXED_KW["targets_only"], tight=False).objects
    for k in np.flatnonzero(~culled):
        assert _same_region(batch.objects[k], loose[k]), names[k]
    for k in np.flatnonzero(culled):
        assert not _same_region(batch.objects[k], loose[k]) and batch.objects[k]["rb_r2"] > 0, names[k]


@pytest.mark.parametrize("kw_name", list(XC.MIXED_KW))
def test_mixed_specification_is_pack_table(kw_name):
    """scale_cases.mixed_spec counts the fits' keys on the way; what it returns is scenes.pack_table's table byte for byte."""
    from omg_planner_amd import scenes
    batch, _ = XC.mixed_spec(kw_name, True)
    want = scenes.pack_table(XC.mixed_scenes(), XC.MIXED_KW[kw_name], ragged=True, share_grids=True)
    assert batch.objects.tobytes() == want.objects.tobytes() and np.array_equal(batch.scene_begin, want.scene_begin)
    assert batch.pool.tobytes() == want.pool.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# clouds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", XC.CLOUD_SIZES)
def test_some_nodes_are_nearest_to_the_last_point_of_the_cloud(n):
    """The last point ends the final tile of k_point_cloud_sdf (a partial one for every n but 1 024, after a full one for 1 025 and
    2 500): nodes whose nearest point it is get a wrong distance from a kernel that stops early."""
    from scipy.spatial import cKDTree
    p, g = XC.cloud(n), XC.cloud_spec(n)
    assert len(p) == n and g.data.size < 40000
    ax = [g.origin[a] + XC.CLOUD_RES * np.arange(g.data.shape[a]) for a in range(3)]
    nodes = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    _, idx = cKDTree(p).query(nodes)
    last_tile = (n - 1) // XC.CLOUD_TILE * XC.CLOUD_TILE
    assert (idx == n - 1).sum() > 100 and (idx != n - 1).sum() > 100
    assert {1023: 1023, 1024: 1024, 1025: 1, 2500: 452}[n] == n - last_tile


# ---------------------------------------------------------------------------------------------------------------------
# time
# ---------------------------------------------------------------------------------------------------------------------
def test_building_every_case_and_specification_is_quick():
    """Everything is cached by now; what it cost is printed (measured when written: a region fit at 589 824 voxels 0.3 s,
    surface_nets at 64^3 0.07 s, the mixed table 0.45 s).  Built fresh, three representative ones stay far below a few seconds."""
    from omg_planner_amd import scenes
    t0 = time.perf_counter()
    XC.rbox(XC.region("r_high").data)
    t1 = time.perf_counter()
    XC.nets(XC.case("s1024"))
    t2 = time.perf_counter()
    scenes.pack_table(XC.mixed_scenes(), XC.MIXED_KW["tabletop"], ragged=True, share_grids=True)
    t3 = time.perf_counter()
    print(f"region fit {t1 - t0:.2f} s, surface_nets 64^3 {t2 - t1:.2f} s, mixed pack_table {t3 - t2:.2f} s")
