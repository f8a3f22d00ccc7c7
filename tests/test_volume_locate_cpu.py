"""CPU test of csrc/omg_volume_body.h, what every kernel over a ragged batch of volumes does first: the header compiled for the
host, the locator and the decode run for every (workgroup, thread) of a batch and compared with numpy."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import kernel_build as KB

BLOCK = 256
_HOST_HARNESS = r"""
#include "omg_volume_body.h"
// Every (block, thread) of `blocks` workgroups: m, id0, id, total, live, idc as int64 [blocks][per][6], (i, j, k) as int32
// [blocks][per][3] and the node's point as float64 [blocks][per][3].
extern "C" void host_locate(const omgx_mesh* meshes, int num_meshes, int blocks, int per, int64_t* node, int32_t* ijk, double* p) {
    for (int b = 0; b < blocks; ++b)
        for (int t = 0; t < per; ++t) {
            const volume_node n = volume_locate(meshes, num_meshes, (uint32_t)b, (uint32_t)t, per);
            const int64_t at = (int64_t)b * per + t;
            const int64_t row[6] = {n.m, n.id0, n.id, n.total, n.live ? 1 : 0, (int64_t)n.idc};
            for (int c = 0; c < 6; ++c) node[at * 6 + c] = row[c];
            int i, j, k;
            volume_decode(meshes[n.m].dims, n.idc, &i, &j, &k);
            ijk[at * 3] = i, ijk[at * 3 + 1] = j, ijk[at * 3 + 2] = k;
            double q[3];
            volume_node_point(meshes[n.m], n.idc, q);
            fusion_node_point(meshes[n.m].origin, meshes[n.m].delta, meshes[n.m].sample_offset, i, j, k, p + at * 3);
            for (int c = 0; c < 3; ++c)
                if (q[c] != p[at * 3 + c]) p[at * 3 + c] = -1.0e300;  // the two ways to the point must agree
        }
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    vp, i = C.c_void_p, C.c_int
    return KB.host_harness(_HOST_HARNESS, tmp_path_factory.mktemp("volume_locate"), {"host_locate": (None, [vp, i, i, i, vp, vp, vp])})


@KB.requires_host_cxx
@pytest.mark.parametrize("M", (1, 2, 6))
def test_locator_and_decode_equal_numpy_for_every_workgroup_and_thread(host, M):
    """The six volumes of fusion_cases.LOCATE and their prefixes of one and two: every workgroup finds the last volume whose
    first_workgroup is not above it (searchsorted), a live thread its node, (i, j, k) by divmod and the point of
    fusion.node_points; a lane past the volume's last node is not live and holds the last node.  Workgroups 0 to 9 for every M:
    those past a prefix's last workgroup fall to its last volume with no live lane."""
    from omg_planner_amd import fusion, ops
    rec = ops.surface_records([v + (0,) for v in FC.LOCATE[:M]])
    first = np.array([r.first_workgroup for r in rec], np.int64)
    assert tuple(first) == FC.LOCATE_FIRST_WORKGROUP[:M]
    blocks = FC.LOCATE_FIRST_WORKGROUP[-1]
    assert blocks == 10
    node = np.full((blocks, BLOCK, 6), -9, np.int64)
    ijk, p = np.full((blocks, BLOCK, 3), -9, np.int32), np.full((blocks, BLOCK, 3), np.nan)
    host.host_locate(C.cast(rec, C.c_void_p), M, blocks, BLOCK, node.ctypes.data, ijk.ctypes.data, p.ctypes.data)
    seen = [0] * M
    for b in range(blocks):
        m = int(np.searchsorted(first, b, side="right")) - 1
        origin, delta, sample, dims = FC.LOCATE[m]
        total = int(np.prod(dims))
        id0 = (b - int(first[m])) * BLOCK
        ids = id0 + np.arange(BLOCK)
        live = ids < total
        idc = np.where(live, ids, total - 1)
        assert np.array_equal(node[b], np.stack([np.full(BLOCK, m), np.full(BLOCK, id0), ids, np.full(BLOCK, total), live, idc], -1)), b
        i, rest = np.divmod(idc, dims[1] * dims[2])
        j, k = np.divmod(rest, dims[2])
        assert np.array_equal(ijk[b], np.stack([i, j, k], -1)), b
        points = fusion.node_points(np.array(origin), delta, {"centre": 0.5, "node": 0.0}[sample], dims)
        assert np.array_equal(p[b], points[idc]), b
        if b >= FC.LOCATE_FIRST_WORKGROUP[M]:
            assert m == M - 1 and not live.any()
        else:
            assert live[0] and (live.all() or b + 1 == FC.LOCATE_FIRST_WORKGROUP[m + 1])  # only a volume's last workgroup has idle lanes
        seen[m] += int(live.sum())
    assert seen == [int(np.prod(d)) for d in FC.LOCATE_DIMS[:M]]  # every node of every volume exactly once
