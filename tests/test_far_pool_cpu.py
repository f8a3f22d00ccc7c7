"""tests/far_pool.py without a device: `relocate` moves exactly the offset fields and moves them in 64 bits, the constants keep every
32-bit wrap of an offset inside the buffer, DeviceScenes.over_pool takes relocated records around a small pool, and the fill and
guard helpers do on a small buffer what test_gpu_far_pool.py relies on."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from omg_planner_amd import _lib, scenes as S
from tests import far_pool as FP

KW = dict(epsilon=0.15, target_epsilon=0.05, clearance=0.02, target_clearance=0.0, disable_collision_set=("obj_1",))


def _batch():
    return S.pack_table([S.make_tabletop_scene(s, num_objects=3, grid=8, table_grid=(8, 8, 4)) for s in range(3)], KW, tight=False)


def _raw(rec, name):
    """A field's bytes (NaNs compare as what they are)."""
    return np.ascontiguousarray(rec[name]).view(np.uint8)


def test_constants_keep_every_wrapped_offset_inside_the_buffer():
    assert FP.B1 == 2 ** 30 + FP.K and FP.B2 == 2 ** 32 + FP.K and FP.K % 2 == 1 and FP.K >= FP.BAND == 4096
    assert FP.ELEMS == 2 ** 32 + FP.RESERVE and FP.RESERVE <= 32 * 2 ** 20
    assert 4 * FP.B1 >= 2 ** 32 > FP.B1 and FP.B2 >= 2 ** 32   # B1: the byte offset leaves 32 bits; B2: the element offset does
    used = FP.MAX_USED
    for base in FP.BASES:
        for i in (0, used - 1):
            for off in (base + i, 4 * (base + i)):             # as elements and as bytes of float32
                lo = off & 0xFFFFFFFF
                signed = lo - 2 ** 32 if lo >= 2 ** 31 else lo
                if lo == off:                                  # (it fits: nothing wraps)
                    continue
                assert signed == lo                            # never negative: a signed index does not leave the buffer at its front
                elem = lo if off == base + i else lo // 4
                assert elem == FP.K + i and elem < FP.K + used + FP.BAND <= FP.LANE
        assert base + used + FP.BAND <= FP.VIEW
    # no lane's far region or alias window reaches another lane's (element units of 4 bytes; the uint8 lanes are shorter still)
    assert (FP.LANES - 1) * FP.LANE + FP.VIEW <= FP.ELEMS and FP.K + FP.MAX_USED + FP.BAND <= FP.LANE
    assert all(abs(b - 2 ** 31) > 2 ** 29 for b in FP.BASES)   # nothing near 2^31 elements


def test_relocate_moves_exactly_the_offsets_in_64_bits():
    batch = _batch()
    rec = batch.objects
    before = rec.copy()
    for delta in (FP.K, FP.B1, FP.B2, (1 << 40) + 3):
        far = FP.relocate(rec, delta)
        assert far is not rec and far.dtype == S.OBJECT_DTYPE and np.array_equal(rec, before)  # the input is not touched
        assert far["grid_offset"].dtype == np.int64 and np.array_equal(far["grid_offset"], rec["grid_offset"].astype(object) + delta)
        for name in S.OBJECT_DTYPE.names:
            if name != "grid_offset":
                assert np.array_equal(_raw(far, name), _raw(rec, name)), name
        back = FP.relocate(far, -delta)
        assert back.tobytes() == rec.tobytes()
    # omgx_mesh records
    mesh = (_lib.Mesh * 3)()
    for m, r in enumerate(mesh):
        r.origin[:], r.delta, r.sample_offset, r.dims[:] = [0.1 * m, 0.0, -0.2], 0.01 + m, 0.5, [3 + m, 4, 5]
        r.out_offset, r.first_workgroup, r.vert_begin, r.vert_count, r.face_begin, r.face_count = 100 * m + 7, m, 8 * m, 8, 30 * m, 30
    far = FP.relocate(mesh, FP.B2)
    assert [int(r.out_offset) for r in far] == [FP.B2 + 100 * m + 7 for m in range(3)] and [int(r.out_offset) for r in mesh] == [7, 107, 207]
    for r in far:
        r.out_offset -= FP.B2
    assert bytes(far) == bytes(mesh) and C.sizeof(far) == C.sizeof(mesh)
    # layouts and begin tables
    lay = [((0.0, 0.0, 0.0), 0.01, "centre", (2, 3, 4), 5), ((1.0, 0.0, 0.0), 0.02, "node", (1, 1, 9), 40)]
    far = FP.relocate(lay, FP.B2)
    assert [v[4] for v in far] == [FP.B2 + 5, FP.B2 + 40] and [v[:4] for v in far] == [v[:4] for v in lay]
    begin = np.array([0, 24, 99], np.int32)
    far = FP.relocate(begin, FP.B2)
    assert far.dtype == np.int64 and far.tolist() == [FP.B2, FP.B2 + 24, FP.B2 + 99] and begin.dtype == np.int32
    assert FP.relocate([3, 4], FP.B1).tolist() == [FP.B1 + 3, FP.B1 + 4]
    with pytest.raises(AssertionError):
        FP.relocate(np.array([0.5, 1.5]), 1)


def test_spread_and_alias_content():
    offs, used = FP.spread([10, 1, 7])
    assert offs == [0, 10 + FP.BAND, 11 + 2 * FP.BAND] and used == 18 + 2 * FP.BAND and FP.spread([]) == ([], 0)
    v = np.array([0.5, -0.25, 0.0, -0.0, 3.0], np.float32)
    a = FP.alias_content(v)
    assert a.dtype == np.float32 and np.isfinite(a).all() and (a != v).all()
    s = np.array([0, 1, 2, 7, 0], np.uint8)
    assert FP.alias_content(s).tolist() == [1, 0, 2, 7, 1]
    assert FP.alias_content(np.array([1, 2, 3], np.int32)).tolist() == [3, 2, 1]


def test_over_pool_takes_relocated_records_around_a_small_pool():
    torch = pytest.importorskip("torch")
    from omg_planner_amd import ops
    batch = _batch()
    n = batch.pool.size
    base = FP.K + n + 3 * FP.BAND + 1   # modest and odd-ish: behind the alias window, so that the two do not overlap
    pool = torch.full((base + n + FP.BAND,), float("nan"), dtype=torch.float32)
    assert FP.place(pool, np.asarray(batch.pool, np.float32), base) == n
    compact = np.asarray(batch.pool, np.float32).reshape(-1)
    assert np.array_equal(pool[base: base + n].numpy().view(np.uint32), compact.view(np.uint32))
    assert np.array_equal(pool[FP.K: FP.K + n].numpy(), FP.alias_content(compact)) and not torch.isnan(pool[: FP.K + n + FP.BAND]).any()
    assert not torch.isnan(pool[base - FP.BAND: base + n + FP.BAND]).any()
    far = ops.DeviceScenes.over_pool(FP.relocate(batch.objects, base), batch.scene_begin, pool, device="cpu")
    near = ops.DeviceScenes(batch, device="cpu")
    assert far.pool.data_ptr() == pool.data_ptr() and far.num_scenes == near.num_scenes == 3
    assert np.array_equal(far.host_objects["grid_offset"], batch.objects["grid_offset"] + base)
    for name in S.OBJECT_DTYPE.names:
        if name != "grid_offset":
            assert np.array_equal(_raw(far.host_objects, name), _raw(near.host_objects, name)), name
    assert np.array_equal(far.host_scene_begin, near.host_scene_begin) and torch.equal(far.scene_begin, near.scene_begin)
    # the device records are the mirror's bytes: only the eight bytes of grid_offset differ from the compact table's
    a = far.objects.numpy().reshape(len(batch.objects), -1)
    b = near.objects.numpy().reshape(len(batch.objects), -1)
    at = S.OBJECT_DTYPE.fields["grid_offset"][1]
    differ = np.flatnonzero((a != b).any(0))
    assert len(differ) and differ.min() >= at and differ.max() < at + 8
    assert far.objects.numpy().tobytes() == FP.relocate(batch.objects, base).tobytes()
    # a moved object changes its pose rows in both and nothing else
    pose = S._yaw_pose(0.45, 0.12, 0.16, 0.7)
    far.set_object_pose(1, 2, pose), near.set_object_pose(1, 2, pose)
    assert np.array_equal(far.host_objects["pose_inv"], near.host_objects["pose_inv"])
    assert np.array_equal(far.host_objects["grid_offset"], batch.objects["grid_offset"] + base)


def test_guard_helpers_on_a_small_buffer():
    torch = pytest.importorskip("torch")
    offs, used = FP.spread([30, 12])
    base = FP.K + used + 2 * FP.BAND
    for dtype in (torch.float32, torch.uint8, torch.int32):
        view = torch.zeros(base + used + 2 * FP.BAND, dtype=dtype)
        FP.guard(view, base, used)
        compact = FP.guard_compact(used, view, "cpu")
        for o, n in zip(offs, (30, 12)):                       # what a correct writer does, compact and far
            compact[o: o + n] = 3
            view[base + o: base + o + n] = 3
        assert FP.written(view, base, compact) == {"far": True, "bands": True, "alias": True}
        view[base + offs[1] - 1] = 3                           # one element before the second volume: in the gap
        assert FP.written(view, base, compact) == {"far": False, "bands": True, "alias": True}
        view[base + offs[1] - 1] = compact[offs[1] - 1]
        view[base - 1] = 3
        assert FP.written(view, base, compact)["bands"] is False
        view[base - 1] = compact[offs[1] - 1]
        view[FP.K + 5] = 3                                     # where a wrapped offset lands
        assert FP.written(view, base, compact) == {"far": True, "bands": True, "alias": False}
