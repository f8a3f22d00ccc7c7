"""The scene table without a device: the one writer of the ragged records (scenes.ragged_records, grid_limits, culled), the
pool's slot bookkeeping (ops.PoolSlots) and the ways into an ops.DeviceScenes (an owned table, a scene range of one, records
around somebody else's pool) on device="cpu"."""
from __future__ import annotations

import numpy as np
import pytest

from omg_planner_amd import _lib, scenes as S

KW = dict(epsilon=0.15, target_epsilon=0.05, clearance=0.02, target_clearance=0.0, disable_collision_set=("obj_1",))


def _tabletops(private: bool):
    scenes = [S.make_tabletop_scene(s, num_objects=3, grid=8, table_grid=(8, 8, 4)) for s in range(3)]
    if private:
        for scn in scenes:
            for ob in scn.objects:
                ob.sdf = S.SdfGrid(ob.sdf.data.copy(), ob.sdf.origin, ob.sdf.delta)
    return scenes


def _one_object():
    return [S.Scene([S.SceneObject("obj", S._yaw_pose(0.4, 0.1, 0.2, 0.3), S.sphere_sdf(0.05, (5, 6, 7), 0.04))], 0)]


CASES = {"tabletops": lambda: _tabletops(False), "private": lambda: _tabletops(True), "one object": _one_object, "empty": lambda: []}


def _restated(scenes, kw, share_grids):
    """The ragged records written object by object, one np.zeros((), OBJECT_DTYPE) each, then finish_records."""
    recs, begins, chunks, offset, seen = [], [0], [], 0, {}
    for scn in scenes:
        poses, eps, pad, clr, dis = S.layer_params(scn, **kw)
        for i, ob in enumerate(scn.objects):
            r = np.zeros((), S.OBJECT_DTYPE)
            r["pose_inv"] = poses[i][:3, :4].ravel()
            mn, mxc = ob.sdf.min_coords, ob.sdf.max_coords
            r["lo"] = mn.astype(np.float32)
            r["hi"] = np.array([mn[a] + (mxc[a] - mn[a]) * 1.0 for a in range(3)], np.float32)
            r["dim"] = ob.sdf.data.shape
            r["delta"] = ob.sdf.delta
            r["epsilon"], r["padding_scale"], r["clearance"] = eps[i], pad[i], clr[i]
            r["disabled"] = 1 if dis[i] > 0 else 0
            if share_grids and id(ob.sdf.data) in seen:
                r["grid_offset"] = seen[id(ob.sdf.data)]
            else:
                r["grid_offset"] = seen[id(ob.sdf.data)] = offset
                chunks.append((offset, np.ascontiguousarray(ob.sdf.data, np.float32).ravel()))
                offset += chunks[-1][1].size
            recs.append(r)
        begins.append(len(recs))
    return S.finish_records(np.array(recs, S.OBJECT_DTYPE)), np.array(begins, np.int32), chunks, offset


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("case", list(CASES))
def test_ragged_records_equal_the_object_by_object_restatement(case, share):
    scenes = CASES[case]()
    want_rec, want_begin, want_chunks, want_elems = _restated(scenes, KW, share)
    rec, begin, chunks, elems = S.ragged_records(scenes, KW, share)
    assert rec.dtype == S.OBJECT_DTYPE and rec.shape == want_rec.shape and rec.tobytes() == want_rec.tobytes()
    assert begin.dtype == np.int32 and np.array_equal(begin, want_begin)
    assert elems == want_elems and [o for o, _ in chunks] == [o for o, _ in want_chunks]
    for (_, got), (_, want) in zip(chunks, want_chunks):
        assert np.asarray(got).size == want.size and np.array_equal(np.asarray(got, np.float32).ravel(), want)
    if case == "tabletops":
        distinct = len({id(ob.sdf.data) for scn in scenes for ob in scn.objects})
        assert len(rec) - distinct >= 3 and len(chunks) == (distinct if share else len(rec))  # the scenes share volumes
    batch = S.pack_table(scenes, KW, ragged=True, share_grids=share, tight=False)
    assert batch.objects.tobytes() == want_rec.tobytes() and np.array_equal(batch.scene_begin, want_begin)
    assert batch.pool.dtype == np.float32 and batch.pool.size == want_elems
    for off, want in want_chunks:
        assert np.array_equal(batch.pool[off: off + want.size], want)


def test_grid_limits_are_the_records_limits_and_round_once():
    for make in CASES.values():
        scenes = make()
        rec = _restated(scenes, KW, True)[0]
        for r, ob in zip(rec, (ob for scn in scenes for ob in scn.objects)):
            lo, hi = S.grid_limits(ob.sdf.origin, ob.sdf.data.shape, ob.sdf.delta)
            assert lo.dtype == hi.dtype == np.float32 and lo.shape == hi.shape == (3,)
            assert lo.tobytes() == r["lo"].tobytes() and hi.tobytes() == r["hi"].tobytes()
    # an origin and a voxel size float32 cannot hold: the far corner is worked out in float64 and rounded once
    origin, shape, delta = np.array([0.1, -0.3, 0.7]), (64, 48, 40), 0.6 / 64
    lo, hi = S.grid_limits(origin, shape, delta)
    far = origin + delta * np.array(shape)
    assert lo.tobytes() == origin.astype(np.float32).tobytes()
    assert hi.tobytes() == np.array([origin[a] + (far[a] - origin[a]) * 1.0 for a in range(3)], np.float32).tobytes()
    early = origin.astype(np.float32) + np.float32(delta) * np.array(shape, np.float32)  # what rounding the inputs first would give
    assert early.dtype == np.float32 and not np.array_equal(hi, early)


def test_culled_is_the_kernels_rule():
    base = np.zeros(1, S.OBJECT_DTYPE)
    base["lo"], base["hi"], base["dim"], base["epsilon"], base["clearance"] = (0.0, 0.0, 0.0), (0.4, 0.4, 0.4), (4, 4, 4), 0.2, 0.01
    below_one, above_one = np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))
    sides = [("hi", (0.4, np.nextafter(np.float32(0), np.float32(1)), 0.4), True), ("hi", (0.4, 0.0, 0.4), False), ("hi", (0.4, -0.1, 0.4), False),
             ("dim", (4, 2, 4), True), ("dim", (4, 1, 4), False),
             ("epsilon", below_one, True), ("epsilon", 1.0, False),
             ("clearance", 1.0, True), ("clearance", above_one, False)]
    rec = np.concatenate([base] * (len(sides) + 1))
    for k, (field, value, _) in enumerate(sides):
        rec[field][k + 1] = value
    got = S.culled(rec)
    assert got.dtype == bool and got.tolist() == [True] + [want for _, _, want in sides]


def test_pool_slots_alone():
    """The allocator of the pool by itself.  Objects 0 and 1 share the volume at 0 (100 elements), object 2 has 60 elements at
    100; behind them 160 elements of reserve."""
    from omg_planner_amd.ops import PoolSlots
    sl = PoolSlots([0, 0, 100], [100, 100, 60], 160, 320)
    state = lambda: (sl.used, dict(sl.refs), list(sl.free), dict(sl.pending))
    assert state() == (160, {0: 2, 100: 1}, [], {})
    # an unshared slot is offered for every volume that fits it
    assert sl.offer(2, 60) == 100 and sl.offer(2, 10) == 100 and state() == (160, {0: 2, 100: 1}, [], {2: (100, 60)})
    assert sl.commit(2) == 100 and state() == (160, {0: 2, 100: 1}, [], {})
    # a shared slot is never offered, not even for a volume that fits: the reserve
    assert sl.offer(0, 50) == 160 and state() == (210, {0: 2, 100: 1}, [], {0: (160, 50)})
    assert (sl.offset[0], sl.cap[0]) == (0, 100)  # nothing about the object changes before the commit
    # an offer that was not committed goes back to the free list and is offered again
    assert sl.offer(0, 40) == 160 and state() == (210, {0: 2, 100: 1}, [], {0: (160, 50)})
    # leaving a slot that another object still uses frees nothing
    assert sl.commit(0) == 160 and state() == (210, {0: 1, 100: 1, 160: 1}, [], {}) and (sl.offset[0], sl.cap[0]) == (160, 50)
    # object 1 is the last user of the volume at 0 now: in place while the volume fits
    assert sl.offer(1, 100) == 0 and sl.commit(1) == 0 and state() == (210, {0: 1, 100: 1, 160: 1}, [], {})
    # it outgrows the slot: the reserve; the slot left behind is free with the commit, not before
    assert sl.offer(1, 110) == 210 and state() == (320, {0: 1, 100: 1, 160: 1}, [], {1: (210, 110)})
    assert sl.commit(1) == 210 and state() == (320, {100: 1, 160: 1, 210: 1}, [(0, 100)], {}) and (sl.offset[1], sl.cap[1]) == (210, 110)
    # a freed slot that fits is preferred to the reserve (which is used up by now), and keeps its whole capacity
    assert sl.offer(2, 80) == 0 and state() == (320, {100: 1, 160: 1, 210: 1}, [], {2: (0, 100)})
    assert sl.commit(2) == 0 and state() == (320, {0: 1, 160: 1, 210: 1}, [(100, 60)], {}) and (sl.offset[2], sl.cap[2]) == (0, 100)
    # no free slot fits and the reserve is exhausted
    with pytest.raises(_lib.OmgHipError, match="no room for 70 more voxels.*reserve_voxels"):
        sl.offer(0, 70)
    assert state() == (320, {0: 1, 160: 1, 210: 1}, [(100, 60)], {})
    # the first free slot that fits; given up for the object's own slot, it is free again
    assert sl.offer(0, 55) == 100 and state() == (320, {0: 1, 160: 1, 210: 1}, [], {0: (100, 60)})
    assert sl.offer(0, 50) == 160 and state() == (320, {0: 1, 160: 1, 210: 1}, [(100, 60)], {0: (160, 50)})
    assert sl.commit(0) == 160 and state() == (320, {0: 1, 160: 1, 210: 1}, [(100, 60)], {})


MUTATORS = [("set_object_pose", lambda ds, torch: ds.set_object_pose(0, 0, np.eye(4))),
            ("set_object_poses", lambda ds, torch: ds.set_object_poses([(0, 0)], np.eye(4)[None])),
            ("grid_slot", lambda ds, torch: ds.grid_slot(0, 0, (2, 2, 2))),
            ("replace_grid", lambda ds, torch: ds.replace_grid(0, 0, torch.zeros((2, 2, 2)), np.zeros(3), 0.1)),
            ("fit_all", lambda ds, torch: ds.fit_all())]


def test_a_scene_range_shares_its_parent_and_refuses_every_change():
    torch = pytest.importorskip("torch")
    from omg_planner_amd import ops
    batch = S.pack_table(_tabletops(False), KW, tight=False)
    ds = ops.DeviceScenes(batch, device="cpu", reserve_voxels=64)
    view = ds.scene_range(1, 3)
    assert view.num_scenes == 2 and view.device == ds.device and view.pool_used == ds.pool_used == batch.pool.size
    assert view.objects.data_ptr() == ds.objects.data_ptr() and view.pool.data_ptr() == ds.pool.data_ptr()
    assert view.host_objects is ds.host_objects
    assert torch.equal(view.scene_begin, ds.scene_begin[1:4]) and view.scene_begin.data_ptr() == ds.scene_begin.data_ptr() + 4
    assert np.array_equal(view.host_scene_begin, batch.scene_begin[1:4]) and np.array_equal(ds.host_scene_begin, batch.scene_begin)
    before = (ds.objects.clone(), ds.host_objects.copy(), ds.pool[: ds.pool_used].clone())
    for name, call in MUTATORS:
        with pytest.raises(_lib.OmgHipError, match="through the table the engine was built on"):
            call(view, torch)
    assert torch.equal(ds.objects, before[0]) and ds.host_objects.tobytes() == before[1].tobytes() and torch.equal(ds.pool[: ds.pool_used], before[2])
    # what the parent changes, the range sees: records, mirror (also after sync_host) and how far the pool is filled
    ds.set_object_pose(2, 1, S._yaw_pose(0.4, 0.1, 0.2, 0.5))
    ds.grid_slot(0, 3, (4, 4, 3))  # the table's volume is shared by the three scenes: space from the reserve
    ds.sync_host()
    assert view.host_objects is ds.host_objects and view.pool_used == ds.pool_used == batch.pool.size + 48
    nested = view.scene_range(1, 2)
    assert nested.num_scenes == 1 and np.array_equal(nested.host_scene_begin, batch.scene_begin[2:4]) and torch.equal(nested.scene_begin, ds.scene_begin[2:4])
    with pytest.raises(IndexError):
        ds.scene_range(2, 4)


def test_records_over_a_borrowed_pool():
    torch = pytest.importorskip("torch")
    from omg_planner_amd import ops
    batch = S.pack_table(_tabletops(True), KW, tight=False)
    owned = ops.DeviceScenes(batch, device="cpu")
    pool = torch.from_numpy(batch.pool.copy()).reshape(-1, 8, 4)
    lent = ops.DeviceScenes.over_pool(batch.objects, batch.scene_begin, pool, "the volumes", device="cpu")
    assert lent.pool.data_ptr() == pool.data_ptr() and lent.pool.shape == (batch.pool.size,) and lent.pool_used == batch.pool.size
    assert lent.num_scenes == 3 and np.array_equal(lent.host_scene_begin, batch.scene_begin) and torch.equal(lent.scene_begin, owned.scene_begin)
    assert torch.equal(lent.objects, owned.objects) and lent.host_objects is not batch.objects
    pose = S._yaw_pose(0.45, 0.12, 0.16, 0.7)
    for ds in (owned, lent):
        ds.set_object_pose(1, 2, pose)
        ds.set_object_poses([(0, 1), (2, 0)], np.stack([S._yaw_pose(0.5, -0.2, 0.1, -1.1), S._yaw_pose(0.3, 0.2, 0.2, 2.0)]))
    idx = int(batch.scene_begin[1]) + 2
    off = idx * S.OBJECT_DTYPE.itemsize
    want = S.se3_inverse(pose)[:3, :4].astype(np.float32).tobytes()
    assert lent.objects[off: off + 48].numpy().tobytes() == want == owned.objects[off: off + 48].numpy().tobytes()
    assert lent.host_objects[idx]["pose_inv"].tobytes() == want
    assert torch.equal(lent.objects, owned.objects) and lent.host_objects.tobytes() == owned.host_objects.tobytes()
    assert not torch.equal(lent.objects, torch.from_numpy(batch.objects.view(np.uint8).copy()))
    assert lent.sync_host().tobytes() == owned.sync_host().tobytes()
    with pytest.raises(IndexError):
        lent.set_object_pose(0, 9, pose)
    for name, call in MUTATORS[2:4]:
        with pytest.raises(_lib.OmgHipError, match="a pool that belongs to somebody else"):
            call(lent, torch)
    for bad, kind in ((pool.double(), "cpu"), (pool.transpose(0, 2), "cpu"), (pool, "cuda")):  # (the kind Cost asks for is the default)
        with pytest.raises(_lib.OmgHipError, match="^env.sdf_torch must be a contiguous float32 device tensor$"):
            ops.DeviceScenes.over_pool(batch.objects, batch.scene_begin, bad, "env.sdf_torch", device=kind)
