"""CPU test of the volume batch behind the wrappers over ragged batches of volumes (ops._VolumeBatch): ops.TsdfVolumes uploads its
records and state_begin once per device however often it is asked, new pool offsets upload new records only, and an empty batch
has no pointers.  The library calls and what needs a device are stubs."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np


def test_tsdf_volumes_upload_records_and_state_begin_once_and_an_empty_batch_has_no_pointers(monkeypatch):
    import torch
    from omg_planner_amd import _lib, ops
    uploads, calls = [], []
    real_upload = ops._upload

    def counting_upload(a, dev):
        uploads.append("records" if isinstance(a, C.Array) else "state_begin" if a.dtype == np.int64 else "other")
        return real_upload(a, dev)

    def stub(name):
        def call(*args):
            calls.append((name, args))
            return _lib.OMGX_OK
        return call

    monkeypatch.setattr(ops, "_upload", counting_upload)
    monkeypatch.setattr(ops, "_need", lambda t, dtype, name: None)      # (the tensors of this test are on the host)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)
    monkeypatch.setattr(ops._VolumeBatch, "release", lambda self, *scratch: None)
    for name in ("omgx_tsdf_states", "omgx_distance_transform", "omgx_tsdf_blend"):
        monkeypatch.setattr(_lib.lib(), name, stub(name))

    vols = [((0.0, 0.0, 0.0), 0.01, "centre", (4, 4, 4)), ((0.1, 0.0, 0.0), 0.02, "node", (3, 5, 2))]
    tv = ops.TsdfVolumes(vols, trunc=0.03, near=0.05, device="cpu")
    assert [int(r.out_offset) for r in tv.rec] == [0, 64] and list(tv.state_begin) == [0, 64] and tv.tsdf.numel() == 94

    def launch_arguments():
        """(device records, their out_offsets on the host, M, device state_begin) of each of the three calls, then forgotten."""
        rows = []
        for name, a in calls:
            b, r = (3, 5) if name != "omgx_distance_transform" else (2, 4)  # state_begin, h_state_begin | volumes, h_volumes, M
            h_rec = C.cast(a[r + 1], C.POINTER(_lib.Mesh))
            rows.append((name, a[r].value, [int(h_rec[m].out_offset) for m in range(a[r + 2])], a[b].value))
        calls.clear()
        return rows

    pool = torch.zeros(400)
    tv.signed(3, out=pool)
    first = launch_arguments()
    assert [r[0] for r in first] == ["omgx_tsdf_states", "omgx_distance_transform", "omgx_tsdf_blend"]
    assert sorted(uploads) == ["records", "state_begin"]                # once each, for the three calls together
    assert len({r[1] for r in first}) == 1 and len({r[3] for r in first}) == 1 and all(r[2] == [0, 64] for r in first)
    tv.signed(3, out=pool), tv.states()
    assert sorted(uploads) == ["records", "state_begin"]                # and not again per call
    assert all(r[1] == first[0][1] and r[3] == first[0][3] for r in launch_arguments())
    # other pool offsets: new records, uploaded once for the call; state_begin is the one that is there already
    for offsets in ([200, 10], [100, 300]):
        del uploads[:]
        tv.signed(3, out=pool, offsets=offsets)
        moved = launch_arguments()
        assert uploads == ["records"]
        assert all(r[2] == offsets for r in moved) and moved[0][1] == moved[1][1] == moved[2][1] != first[0][1]
        assert all(r[3] == first[0][3] for r in moved)
    assert [int(r.out_offset) for r in tv.rec] == [0, 64]               # the offsets held for those calls only
    # another device (here: the same one under another name is the same device) is not another upload
    del uploads[:]
    assert tv._batch.on(torch.device("cpu")).volume_args()[0].value == first[0][1] and uploads == []

    empty = ops._VolumeBatch([]).on("cpu")
    assert empty.M == 0 and empty.end() == 0 and empty.pool_end() == 1
    assert empty.volume_args() == (None, None, 0) and empty.host_args() == (None, 0) and empty.begin_args() == (None, None) and uploads == []
