"""The kernels at the sizes the shipped workloads have, on the MI355X, against the specification bit for bit (cases: scale_cases.py;
why each case decides something in a second pass: test_scale_cpu.py): k_surface_scan's carry and surf_vertex_index across its
passes (more than 65 536 samples), a workgroup whose 256 samples are all active cells, the single influence-region fit past the caps
of k_region_maxabs (262 144 voxels) and k_region_boxes (524 288 voxels), the batched fit on hostile volumes with the dedup of
DeviceScenes.fit_all, and k_point_cloud_sdf with a partial tile after a full one.  No tolerance anywhere."""
from __future__ import annotations

import numpy as np
import pytest

from tests import scale_cases as XC
from tests import surface_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _same(verts, faces, want_v, want_f):
    """verts as int64 bits and faces, device against specification."""
    return (torch.equal(verts.cpu().view(torch.int64), torch.from_numpy(np.array(want_v, np.float64)).view(torch.int64).reshape(-1, 3)) and
            torch.equal(faces.cpu(), torch.from_numpy(np.array(want_f, np.int32)).reshape(-1, 3)))


def _up(a, dev):
    """A host array (the cases are read-only) as a device tensor."""
    return torch.from_numpy(np.array(a)).to(dev)


def _case_of(name):
    return XC.case(name) if name in XC.SURFACE else SC.case(name)


def _single(dev, name):
    from omg_planner_amd import ops
    c = _case_of(name)
    return ops.surface_mesh(_up(c["data"], dev), c["origin"], c["delta"], c["sample"], 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", XC.SURFACE)
def test_surface_of_one_volume_across_the_passes_of_the_scan(dev, name):
    """256 workgroups (one pass, the control), 275, 513 and 1 024 (two to four passes of k_surface_scan, the later ones offset by the
    carry; faces whose four cells lie in two passes), and the volume whose first workgroup holds 256 active cells (ranks 0..255)."""
    want_v, want_f, want_o = XC.spec(name)
    verts, faces, open_edges = _single(dev, name)
    assert tuple(verts.shape) == (len(want_v), 3) and tuple(faces.shape) == (len(want_f), 3) and open_edges == want_o
    assert _same(verts, faces, want_v, want_f)


RAGGED = ("17x9x5", "s1024", "s275", "all_outside", "s513")


def test_ragged_batch_with_multi_pass_volumes_behind_a_small_one(dev):
    """One launch, level 0: the multi-pass volumes start at a first_workgroup that is not 0 (3, 1 027 and 1 303), a small and an empty
    volume follow a multi-pass one, NaN between the volumes: every mesh equals its single launch and the specification."""
    from omg_planner_amd import ops
    want = [XC.spec(n) for n in RAGGED]   # scenes.surface_nets at level 0 (surface_cases.spec has 17x9x5 at its own level, -0.005)
    assert len(want[0][1]) > 0 and len(want[3][0]) == 0
    parts, layouts, at, gap = [], [], 3, 3
    for n in RAGGED:
        c = _case_of(n)
        parts += [np.full(gap, np.nan, np.float32), c["data"].ravel()]
        layouts.append((c["origin"], c["delta"], c["sample"], c["data"].shape, at))
        at += c["data"].size + gap
    pool = torch.from_numpy(np.concatenate(parts + [np.full(gap, np.nan, np.float32)])).to(dev)
    assert [r.first_workgroup for r in ops.surface_records(layouts)] == [0, 3, 1027, 1302, 1303]
    v, f, vrows, frows, o = ops.surface_meshes(pool, layouts, 0.0)
    nv, nf = [len(w[0]) for w in want], [len(w[1]) for w in want]
    assert vrows[:, 1].tolist() == nv and frows[:, 1].tolist() == nf and o.tolist() == [w[2] for w in want]
    assert vrows[:, 0].tolist() == np.concatenate([[0], np.cumsum(nv)[:-1]]).tolist() and frows[:, 0].tolist() == np.concatenate([[0], np.cumsum(nf)[:-1]]).tolist()
    for m, n in enumerate(RAGGED):
        mv, mf = v[vrows[m, 0]: vrows[m, 0] + vrows[m, 1]], f[frows[m, 0]: frows[m, 0] + frows[m, 1]]
        assert _same(mv, mf, want[m][0], want[m][1]), n
        sv, sf, so = _single(dev, n)
        assert so == o[m] and torch.equal(sv.view(torch.int64), mv.view(torch.int64)) and torch.equal(sf, mf), n


def test_object_surfaces_of_a_scene_table_with_a_64_cubed_object(dev):
    """DeviceScenes.object_surfaces on a table with one 64^3 object (1 024 workgroups, read in place from the pool) and one 32^3 object
    behind it: the specification on the record's lo and delta, and not a byte of the pool changes."""
    from omg_planner_amd import ops, scenes as sc
    from omg_planner_amd.config import Config
    big, small = sc.sphere_sdf(0.1, (64, 64, 64), 0.6 / 64), sc.box_sdf((0.05, 0.07, 0.03), (32, 32, 32), 1.0 / 128)
    scene = sc.Scene([sc.SceneObject("ball", sc._yaw_pose(0.5, 0.0, 0.2, 0.4), big), sc.SceneObject("box", sc._yaw_pose(0.4, 0.3, 0.1, -0.2), small)], 0)
    table = ops.DeviceScenes.from_scenes([scene], Config().layer_kwargs(), device=dev)
    torch.cuda.synchronize()
    before = table.pool.cpu().numpy().tobytes()
    verts, faces, vrows, frows, open_edges = table.object_surfaces()
    torch.cuda.synchronize()
    assert table.pool.cpu().numpy().tobytes() == before
    assert vrows[:, 1].sum() == len(verts) and frows[:, 1].sum() == len(faces)
    for k, grid in enumerate((big, small)):
        rec = table.host_objects[k]
        wv, wf, wo = sc.surface_nets(grid.data, rec["lo"].astype(np.float64), float(rec["delta"]), "centre", 0.0)
        assert len(wf) > 0 and wo == 0 == open_edges[k]
        assert _same(verts[vrows[k, 0]: vrows[k, 0] + vrows[k, 1]], faces[frows[k, 0]: frows[k, 0] + frows[k, 1]], wv, wf), k


# ---------------------------------------------------------------------------------------------------------------------
# influence regions
# ---------------------------------------------------------------------------------------------------------------------
RECORD_FIELDS = ("lo", "hi", "dim", "delta", "inv_extent", "inv_delta", "epsilon", "clearance", "inv_2eps", "inv_eps", "pose_inv")


@pytest.mark.parametrize("name,which", XC.REGION_CASES)
def test_single_fit_past_the_block_caps(dev, name, which):
    """omgx_fit_influence_region on 589 824 voxels (both stride loops repeat; r_high is decided in the second pass of
    k_region_boxes, r_tail's margin in the second pass of k_region_maxabs) and on the bench's table volume (393 216: only
    k_region_maxabs repeats) against scenes.pack_table(tight=True): every field of the record."""
    from omg_planner_amd import ops, scenes as sc
    vol = XC.region(name)
    kw = XC.one_object_kwargs(*XC.THRESHOLDS[which])
    want = XC.region_spec(name, which)
    other = sc.Scene([sc.SceneObject("obj", np.eye(4), sc.sphere_sdf(0.05, (8, 8, 8), 0.05))], 0)
    ds = ops.DeviceScenes(sc.pack_table([other], kw, tight=True), dev, reserve_voxels=int(vol.data.size))
    slot = ds.grid_slot(0, 0, vol.data.shape)
    slot.copy_(_up(vol.data, dev))
    ds.replace_grid(0, 0, slot, vol.origin, vol.delta, fit="device")
    torch.cuda.synchronize()
    got = ds.sync_host()[0]
    for f in RECORD_FIELDS:
        assert np.array_equal(got[f], want[f]), f
    for f in XC.REGION_FIELDS:
        assert np.array_equal(got[f], want[f]), (f, got[f], want[f])


@pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")  # the cases are read-only; from_scenes only reads them
@pytest.mark.parametrize("kw_name", list(XC.MIXED_KW))
def test_batched_fit_of_the_mixed_table(dev, kw_name):
    """DeviceScenes.from_scenes on noise, NaN and +-inf voxels, a volume nothing reaches, 1 x 9 x 7 and 2 x 2 x 2 volumes, four
    spheres that differ in thresholds, one ulp of content or extent, the bench's table, volumes shared between scenes and an empty
    scene, against scenes.pack_table: every field of every record, scene_begin, the pool.  With epsilon = 1.5 only the two targets
    are fitted (one fit, one copy) and every other record keeps its loose region."""
    from omg_planner_amd import ops
    want, keys = XC.mixed_spec(kw_name, True)
    ds = ops.DeviceScenes.from_scenes(XC.mixed_scenes(), XC.MIXED_KW[kw_name], dev, share_grids=True)
    got = ds.sync_host()
    assert got.shape == want.objects.shape and np.array_equal(ds.host_scene_begin, want.scene_begin)
    names = XC.SCENE0 + XC.SCENE1
    for f in want.objects.dtype.names:
        for k in range(len(got)):
            assert np.array_equal(got[f][k], want.objects[f][k], equal_nan=True), (f, names[k], got[f][k], want.objects[f][k])
    assert ds.pool[: ds.pool_used].cpu().numpy().tobytes() == want.pool.tobytes()
    assert ds.fit_all() == keys
    again = ds.sync_host()
    assert again.tobytes() == want.objects.tobytes()   # fitting twice changes nothing


def test_batched_and_single_fit_agree_on_the_mixed_table(dev):
    """The mixed table with a private volume per object: the batched fit equals the specification; then every culled record of
    scene 0 takes its own volume again through replace_grid(fit="device") — the single-object kernels — and the four region
    fields come out the same."""
    from omg_planner_amd import ops, scenes as sc
    scenes = XC.mixed_scenes(private=True)
    want, keys = XC.mixed_spec("tabletop", False)
    ds = ops.DeviceScenes.from_scenes(scenes, XC.MIXED_KW["tabletop"], dev, share_grids=False)
    batched = ds.sync_host().copy()
    for f in want.objects.dtype.names:
        assert np.array_equal(batched[f], want.objects[f], equal_nan=True), f
    assert ds.fit_all() == keys
    culled = sc.culled(batched)
    assert culled[: len(XC.SCENE0)].sum() == len(XC.SCENE0) - 1
    used = ds.pool_used
    for o, name in enumerate(XC.SCENE0):
        if not culled[o]:
            continue
        g = scenes[0].objects[o].sdf
        ds.replace_grid(0, o, _up(g.data, dev), g.origin, g.delta, fit="device")
    torch.cuda.synchronize()
    assert ds.pool_used == used  # every volume went back into its own slot
    single = ds.sync_host()
    for o, name in enumerate(XC.SCENE0):
        for f in XC.REGION_FIELDS + RECORD_FIELDS:
            assert np.array_equal(single[f][o], batched[f][o]), (name, f, single[f][o], batched[f][o])
    assert single[len(XC.SCENE0):].tobytes() == batched[len(XC.SCENE0):].tobytes()
    assert ds.pool[: used].cpu().numpy().tobytes() == want.pool.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# clouds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", XC.CLOUD_SIZES)
def test_point_cloud_sdf_around_the_tile_of_1024_points(dev, n):
    """One tile less a point, one tile, a tile and ONE point, two tiles and 452 points; the last point of the cloud is the nearest one
    of several hundred nodes.  The grid as int32 bits and the origin."""
    from omg_planner_amd import ops
    ref = XC.cloud_spec(n)
    grid, origin, res = ops.point_cloud_sdf(_up(XC.cloud(n), dev), XC.CLOUD_RES, XC.CLOUD_MARGIN)
    assert tuple(grid.shape) == ref.data.shape and res == XC.CLOUD_RES
    assert np.array_equal(grid.cpu().numpy().view(np.int32), ref.data.view(np.int32))
    assert np.array_equal(origin, ref.origin)
