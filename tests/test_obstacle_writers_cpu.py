"""CPU test of the call path of the four observed-volume writers of ops.DeviceScenes (fuse_obstacles, integrate_obstacles,
segment_obstacles, plane_obstacles): which entry points a call reaches, in which order and with which host-visible arguments;
that nothing is pending afterwards and a refused call reaches none; how many small arrays a call uploads; and ops._ViewBatch
alone.  The library calls and what needs a device are stubs, as in test_volume_batch_cpu.py; the table lives on "cpu"."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import fusion_cases as FC

LAYOUTS = [((0.0, 0.0, 0.0), 0.01, (4, 4, 4)), ((0.1, 0.0, 0.0), 0.02, (3, 5, 2))]
PAIRS, OTHERS = [(0, 0), (1, 0)], [(0, 1), (1, 1)]
V, H, W, N = 3, 4, 5, 2
RANGES = [(0, 2), (2, 1)]
BAND, NEAR, REACH, TRUNC = 0.01, 0.05, 0.03, 0.03
RADIUS = 5  # fusion.obstacle_radius(0.03, 0.01) = ceil(0.03 / 0.01 + 0.5) + 1 of the finer layout
RECORD = (5, 0, 1, 1, 0, 2, 2, 1)  # what the labelling stub finds in every volume: 5 nodes, the box (1,1,0) .. (2,2,1)
MARGIN = 1  # -> the crop (4, 4, 4) from node (0, 0, -1)

# per entry point: where its host-visible arguments stand (h_volumes and M; what else is named)
VOLUMES_AT = {"omgx_carve_views": 1, "omgx_clear_robot": 1, "omgx_tsdf_integrate": 1, "omgx_plane_volumes": 1, "omgx_distance_transform": 5,
              "omgx_label_components": 5, "omgx_component_records": 5, "omgx_tsdf_states": 6, "omgx_tsdf_blend": 6, "omgx_component_states": 15}
VIEWS = {"omgx_carve_views": (11, {"merge": 15}), "omgx_tsdf_integrate": (11, {"merge": 18}), "omgx_clear_robot": (12, {"N": 16, "cull": 19})}
SCALARS = {"omgx_distance_transform": {"radius": 7, "unknown_occupied": 8}, "omgx_label_components": {"select": 7, "connectivity": 8},
           "omgx_object_set_grid": {"grid_offset": 5}}


def _views():
    return np.stack([FC.view(fx=1.0 + 0.25 * v, fy=2.0, cx=0.5 * v, cy=0.25) for v in range(V)])


class _Stubbed:
    """The library, _need, _stream, _release, torch.cuda.device and _upload replaced; calls and uploads are recorded."""

    def __init__(self, monkeypatch):
        import torch
        from omg_planner_amd import _lib, ops
        self.calls, self.uploads = [], []
        real_upload = ops._upload

        def upload(a, dev):
            self.uploads.append((type(a).__name__, getattr(a, "dtype", None), bytes(a)))
            return real_upload(a, dev)

        monkeypatch.setattr(ops, "_upload", upload)
        monkeypatch.setattr(ops, "_need", lambda t, dtype, name: None)  # (the tensors of this test are on the host)
        monkeypatch.setattr(ops, "_stream", lambda: None)
        monkeypatch.setattr(ops, "_release", lambda dev, *scratch: None)
        monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)
        for name in list(VOLUMES_AT) + ["omgx_object_set_grid", "omgx_fit_influence_region", "omgx_region_scratch_bytes",
                                       "omgx_distance_transform_workspace_bytes", "omgx_label_workspace_bytes"]:
            monkeypatch.setattr(_lib.lib(), name, self._stub(name, _lib))

    def _stub(self, name, _lib):
        def call(*a):
            self.calls.append((name, self._seen(name, a, _lib)))
            if name == "omgx_label_components":  # one component per volume
                (C.c_int32 * a[6]).from_address(a[11].value)[:] = [1] * a[6]
            if name == "omgx_component_records":
                (C.c_int32 * (8 * a[10])).from_address(a[9].value)[:] = list(RECORD) * a[10]
            return 64 if name.endswith("_bytes") else _lib.OMGX_OK
        return call

    @staticmethod
    def _seen(name, a, _lib):
        """The host-visible arguments of one call, as plain values."""
        seen = {}
        if name in VOLUMES_AT:
            at = VOLUMES_AT[name]
            rec = C.cast(a[at], C.POINTER(_lib.Mesh))
            seen["M"], seen["out_offsets"] = a[at + 1], [int(rec[m].out_offset) for m in range(a[at + 1])]
        if name in VIEWS:
            hw, more = VIEWS[name]
            seen.update(V=a[5], H=a[hw], W=a[hw + 1], views=C.string_at(a[4].value, a[5] * 128), ranges=C.string_at(a[7].value, a[2] * 8),
                        **{k: a[i] for k, i in more.items()})
        seen.update({k: a[i] for k, i in SCALARS.get(name, {}).items()})
        return seen

    def names(self):
        return [name for name, _ in self.calls]

    def of(self, name):
        return [seen for n, seen in self.calls if n == name]

    def forget(self):
        del self.calls[:], self.uploads[:]


@pytest.fixture
def stubbed(monkeypatch):
    return _Stubbed(monkeypatch)


def _table():
    """Two scenes of two objects, each with a volume too small to take a layout, and room for every new volume in the reserve."""
    from omg_planner_amd import ops, scenes as sc
    made = [sc.Scene([sc.SceneObject(f"object{k}", np.eye(4), sc.sphere_sdf(0.05, (2, 2, 2), 0.05)) for k in range(2)], 0) for _ in range(2)]
    return ops.DeviceScenes(sc.pack_table(made, share_grids=False), device="cpu", reserve_voxels=1000)


def _inputs(robot: bool):
    import torch
    from omg_planner_amd import ops
    rng = np.random.RandomState(3)
    depth = torch.from_numpy(rng.uniform(0.2, 0.6, (V, H, W)))
    view = None
    if robot:
        t_near = torch.from_numpy(np.where(rng.uniform(size=(V, H, W)) < 0.5, np.inf, rng.uniform(0.1, 0.7, (V, H, W))))
        spheres = torch.from_numpy(rng.uniform(0.01, 0.5, (V, N, 4)))
        view = ops.RobotView(t_near, torch.zeros((V, H, W), dtype=torch.int32), spheres, 0.01)
    return depth, _views(), view


SET_GRID = ["omgx_object_set_grid", "omgx_region_scratch_bytes", "omgx_fit_influence_region"]
TRANSFORM = ["omgx_distance_transform_workspace_bytes", "omgx_distance_transform"]


def _offsets(table, pairs):
    return [int(table.host_objects[table._index(s, o)]["grid_offset"]) for s, o in pairs]


def _check_views(seen, views, **more):
    assert (seen["V"], seen["H"], seen["W"]) == (V, H, W) and seen["views"] == np.ascontiguousarray(views, np.float64).tobytes()
    assert seen["ranges"] == np.array(RANGES, np.int32).tobytes() and all(seen[k] == v for k, v in more.items())


@pytest.mark.parametrize("robot", [False, True])
def test_fuse_obstacles_reaches_these_entry_points_with_these_arguments(stubbed, robot):
    table = _table()
    depth, views, view = _inputs(robot)
    assert table.fuse_obstacles(PAIRS, depth, views, RANGES, LAYOUTS, BAND, NEAR, REACH, unknown_occupied=False, robot=view) == RADIUS
    assert stubbed.names() == ["omgx_carve_views"] + ["omgx_clear_robot"] * robot + TRANSFORM + SET_GRID * 2
    placed = _offsets(table, PAIRS)
    assert len(set(placed)) == 2 and min(placed) >= 32  # both went to the reserve
    for name in ["omgx_carve_views", "omgx_distance_transform"] + ["omgx_clear_robot"] * robot:
        (seen,) = stubbed.of(name)
        assert seen["M"] == 2 and seen["out_offsets"] == placed, name
    _check_views(stubbed.of("omgx_carve_views")[0], views, merge=0)
    if robot:
        _check_views(stubbed.of("omgx_clear_robot")[0], views, N=N, cull=1)
    assert stubbed.of("omgx_distance_transform")[0]["radius"] == RADIUS and stubbed.of("omgx_distance_transform")[0]["unknown_occupied"] == 0
    assert [seen["grid_offset"] for seen in stubbed.of("omgx_object_set_grid")] == placed
    assert not table._slots.pending


def test_integrate_obstacles_reaches_these_entry_points_with_these_arguments(stubbed):
    table = _table()
    depth, views, view = _inputs(True)
    tv = None
    for frame in range(2):
        stubbed.forget()
        radius, tv = table.integrate_obstacles(PAIRS, tv, depth, views, RANGES, LAYOUTS, TRUNC, NEAR, REACH, robot=view)
        assert radius == RADIUS and tv.frames == frame + 1
        assert stubbed.names() == ["omgx_tsdf_integrate", "omgx_tsdf_states", "omgx_clear_robot"] + TRANSFORM + ["omgx_tsdf_blend"] + SET_GRID * 2
        placed = _offsets(table, PAIRS)
        (seen,) = stubbed.of("omgx_tsdf_integrate")
        assert seen["M"] == 2 and seen["out_offsets"] == [0, 64]  # the pairs lie back to back, whatever the pool's slots are
        _check_views(seen, views, merge=frame)
        for name in ("omgx_tsdf_states", "omgx_clear_robot", "omgx_distance_transform", "omgx_tsdf_blend"):
            (seen,) = stubbed.of(name)
            assert seen["M"] == 2 and seen["out_offsets"] == placed, name
        _check_views(stubbed.of("omgx_clear_robot")[0], views, N=N, cull=1)
        assert stubbed.of("omgx_distance_transform")[0]["radius"] == RADIUS and stubbed.of("omgx_distance_transform")[0]["unknown_occupied"] == 1
        assert [seen["grid_offset"] for seen in stubbed.of("omgx_object_set_grid")] == placed
        assert not table._slots.pending


def test_segment_obstacles_reaches_these_entry_points_with_these_arguments(stubbed):
    table = _table()
    depth, views, view = _inputs(True)
    seeds = [(0.02, 0.02, 0.01), (0.13, 0.04, 0.02)]
    radius, records, comps = table.segment_obstacles(PAIRS, OTHERS, depth, views, RANGES, LAYOUTS, BAND, NEAR, REACH, seeds, 1, connectivity=18,
                                                     margin=MARGIN, robot=view)
    assert radius == RADIUS and records.tolist() == [list(RECORD)] * 2 and comps.comp_begin.tolist() == [0, 1, 2]
    assert stubbed.names() == (["omgx_carve_views", "omgx_clear_robot", "omgx_label_workspace_bytes", "omgx_label_components", "omgx_component_records",
                                "omgx_component_states"] + TRANSFORM + SET_GRID * 4)
    for name in ("omgx_carve_views", "omgx_clear_robot", "omgx_label_components", "omgx_component_records"):
        (seen,) = stubbed.of(name)
        assert seen["M"] == 2 and seen["out_offsets"] == [0, 64], name
    _check_views(stubbed.of("omgx_carve_views")[0], views, merge=0)
    _check_views(stubbed.of("omgx_clear_robot")[0], views, N=N, cull=1)
    assert stubbed.of("omgx_label_components")[0]["select"] == 1 and stubbed.of("omgx_label_components")[0]["connectivity"] == 18
    placed = _offsets(table, [PAIRS[0], OTHERS[0], PAIRS[1], OTHERS[1]])  # per scene the target's crop, then the layout
    assert len(set(placed)) == 4
    for name in ("omgx_component_states", "omgx_distance_transform"):
        (seen,) = stubbed.of(name)
        assert seen["M"] == 4 and seen["out_offsets"] == placed, name
    assert stubbed.of("omgx_distance_transform")[0]["radius"] == RADIUS and stubbed.of("omgx_distance_transform")[0]["unknown_occupied"] == 1
    assert [seen["grid_offset"] for seen in stubbed.of("omgx_object_set_grid")] == placed
    dims = [tuple(int(d) for d in table.host_objects[table._index(s, o)]["dim"]) for s, o in (PAIRS[0], OTHERS[0], PAIRS[1], OTHERS[1])]
    assert dims == [(4, 4, 4), (4, 4, 4), (4, 4, 4), (3, 5, 2)]
    assert not table._slots.pending


def test_plane_obstacles_reaches_these_entry_points_with_these_arguments(stubbed):
    table = _table()
    table.plane_obstacles(PAIRS, [(0.0, 0.0, 1.0, -0.01), (0.0, 1.0, 0.0, 0.02)], LAYOUTS)
    assert stubbed.names() == ["omgx_plane_volumes"] + SET_GRID * 2
    placed = _offsets(table, PAIRS)
    (seen,) = stubbed.of("omgx_plane_volumes")
    assert seen["M"] == 2 and seen["out_offsets"] == placed and [s["grid_offset"] for s in stubbed.of("omgx_object_set_grid")] == placed
    assert not table._slots.pending


def test_a_refused_call_reaches_no_entry_point_and_leaves_nothing_pending(stubbed):
    from omg_planner_amd import _lib
    depth, views, view = _inputs(True)
    table = _table()
    bad_view = views.copy()
    bad_view[1, 0] = 0.0
    fuse = dict(pairs=PAIRS, depth=depth, views=views, view_range=RANGES, layouts=LAYOUTS, band=BAND, near=NEAR, reach=REACH, robot=view)
    integrate = dict(fuse, tsdf_volumes=None, trunc=TRUNC)
    del integrate["band"]
    segment = dict(fuse, target_pairs=PAIRS, obstacle_pairs=OTHERS, seeds=np.zeros((2, 3)), min_nodes=1)
    del segment["pairs"]
    for method, good in ((table.fuse_obstacles, fuse), (table.integrate_obstacles, integrate), (table.segment_obstacles, segment)):
        for what, change in (("view_range", dict(view_range=[(0, 2), (2, 2)])), ("2 views but 3 images", dict(views=views[:2])),
                             ("focal length of zero", dict(views=bad_view)), ("must be finite", dict(near=float("nan"))),
                             ("dims >= 1", dict(layouts=[LAYOUTS[0], ((0.0, 0.0, 0.0), 0.01, (4, 0, 4))])), ("reach must be finite", dict(reach=-1.0)),
                             ("RobotView", dict(robot=object()))):
            with pytest.raises(_lib.OmgHipError, match=what):
                method(**{**good, **change})
            assert not stubbed.calls and not table._slots.pending, (method.__name__, what)
    with pytest.raises(_lib.OmgHipError, match="named twice"):
        table.plane_obstacles([(1, 0), (1, 0)], np.zeros((2, 4)), LAYOUTS)
    with pytest.raises(_lib.OmgHipError, match="planes"):
        table.plane_obstacles(PAIRS, np.full((2, 4), np.nan), LAYOUTS)
    with pytest.raises(ValueError, match="named twice"):
        table.set_object_poses([(1, 0), (1, 0)], np.tile(np.eye(4), (2, 1, 1)))
    with pytest.raises(IndexError):
        table.fuse_obstacles(**{**fuse, "pairs": [(0, 0), (1, 2)]})
    assert not stubbed.calls and not stubbed.uploads and not table._slots.pending


def test_no_host_array_is_uploaded_twice_within_one_writer_call(stubbed):
    """The rule: within one writer call no host array goes to the device twice.  What a call needs there:
    fuse_obstacles: the records at the slots' offsets, state_begin, the views, view_range = 4, with the clear step or without (the
    carve does not read the pool offset, so one set of records serves the carve, the clear and the transform);
    integrate_obstacles, first frame: the TsdfVolumes' own records and state_begin (kept for later frames), the views, view_range,
    and the records at this call's slots = 5; a later frame: the views, view_range, the records at the new slots = 3;
    segment_obstacles: the layouts' records, state_begin, the views, view_range (carve, clear, labelling), comp_begin (the
    record launch and the crop), the picks, the outputs' records and their state_begin (the crop and the transform) = 8."""
    depth, views, view = _inputs(True)

    def count(call):
        stubbed.forget()
        call()
        assert len(set(stubbed.uploads)) == len(stubbed.uploads), "a host array went to the device twice"
        return len(stubbed.uploads)

    for robot in (view, None):
        assert count(lambda: _table().fuse_obstacles(PAIRS, depth, views, RANGES, LAYOUTS, BAND, NEAR, REACH, robot=robot)) == 4
    table, kept = _table(), []
    integrate = lambda: kept.append(table.integrate_obstacles(PAIRS, kept[-1] if kept else None, depth, views, RANGES, LAYOUTS, TRUNC, NEAR, REACH, robot=view)[1])
    assert count(integrate) == 5 and count(integrate) == 3 and count(integrate) == 3
    seeds = [(0.02, 0.02, 0.01), (0.13, 0.04, 0.02)]
    assert count(lambda: _table().segment_obstacles(PAIRS, OTHERS, depth, views, RANGES, LAYOUTS, BAND, NEAR, REACH, seeds, 1, margin=MARGIN, robot=view)) == 8
    assert count(lambda: _table().plane_obstacles(PAIRS, np.eye(4)[:2], LAYOUTS)) == 2  # the records and the planes


def test_view_batch_alone(stubbed):
    import torch
    from omg_planner_amd import _lib, ops
    E = _lib.OmgHipError
    depth, views, _ = _inputs(False)
    vb = ops._ViewBatch.of(views, RANGES, depth, 2).on("cpu")
    assert (vb.V, vb.H, vb.W) == (V, H, W) and vb.h_views.dtype == np.float64 and vb.h_views.shape == (V, 16)
    assert vb.h_range.dtype == np.int32 and vb.h_range.tolist() == [list(r) for r in RANGES]
    d_views, h_views, n, d_range, h_range = vb.view_args()
    assert n == V and h_views.value == vb.h_views.ctypes.data and h_range.value == vb.h_range.ctypes.data and len(stubbed.uploads) == 2
    # a batch passes through with its uploads, for images of the same shape (the filtered depth of the same call)
    again = ops._ViewBatch.of(vb, None, depth + 1.0, 2)
    assert again is vb and [p.value for p in again.on(torch.device("cpu")).view_args()[0::3]] == [d_views.value, d_range.value] and len(stubbed.uploads) == 2
    for M, images in ((3, depth), (1, depth), (2, depth[:2]), (2, depth[:, :3]), (2, depth[0])):
        with pytest.raises(E, match="these views are for 2 volumes"):
            ops._ViewBatch.of(vb, None, images, M)
    # no views, no volumes: no pointers and no upload
    stubbed.forget()
    empty = ops._ViewBatch.of(np.zeros((0, 16)), [], torch.zeros((0, H, W), dtype=torch.float64), 0).on("cpu")
    assert empty.view_args() == (None, None, 0, None, None) and (empty.H, empty.W) == (H, W) and not stubbed.uploads
    # the views' and ranges' refusals of test_gpu_fusion's table, with its messages, before any tensor is looked at
    vols = [(o, d, "centre", n) for o, d, n in LAYOUTS]
    nan_view, no_focal = views.copy(), views.copy()
    nan_view[1, 9], no_focal[2, 1] = np.nan, 0.0
    good = dict(volumes=vols, views=views, view_range=RANGES, depth=depth, band=BAND, near=NEAR)
    for what, change in ((r"view_range must be \[2,2\] inside \[0, 3\]", dict(view_range=[(0, 3), (2, 2)])),
                         (r"view_range must be \[2,2\] inside \[0, 3\]", dict(view_range=[(0, 3)])),
                         (r"view_range must be \[2,2\] inside \[0, 3\]", dict(view_range=[(0, 3), (-1, 2)])),
                         ("2 views but 3 images", dict(views=views[:2])), ("a view is not finite or has a focal length of zero", dict(views=nan_view)),
                         ("a view is not finite or has a focal length of zero", dict(views=no_focal)),
                         ("band and near must be finite", dict(band=float("nan"))), ("band and near must be finite", dict(near=float("inf"))),
                         # precedence: the views before band and near, those before the volumes, the volumes before view_range
                         ("2 views but 3 images", dict(views=views[:2], band=float("nan"))), ("band and near must be finite", dict(band=float("nan"), volumes=[vols[0][:3]])),
                         ("got 3 fields", dict(volumes=[vols[0][:3]], view_range=[(0, 4)])), ("depth must be a tensor", dict(depth=depth[0], views=views[:2]))):
        for op in (ops.carve_views, lambda **kw: ops.fuse_views(radius=3, **kw)):
            with pytest.raises(E, match=what):
                op(**{**good, **change})
    assert not stubbed.calls and not stubbed.uploads
