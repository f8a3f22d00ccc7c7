"""CPU tests of depth fusion (omg-planner_amd/fusion.py, csrc/omg_fusion.hip): the specification's distance
transform against scipy and brute force; the carve rule at its edges as known answers; a rendered scene of a sphere above a slab;
csrc/omg_fusion_body.h compiled for the host equals the specification bit for bit; every argument error of the C ABI and of the
wrappers; the kernels use no scratch."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import kernel_build as KB

INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the transform against scipy and brute force
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.TRANSFORM)
def test_transform_specification_against_scipy_and_brute_force(name):
    """The integer d2 of both channels equals min(edt^2, R^2) from scipy's nearest-node indices exactly, and all pairs where the
    grid has at most 512 nodes; the float32 value is the formula of the text; occupied <= -0.5 delta, free >= +0.5 delta."""
    pytest.importorskip("scipy.ndimage")
    from omg_planner_amd import fusion
    s, delta = FC.states(name), 0.0125
    for R in FC.RADII:
        for uo in (False, True):
            occ = fusion.occupied(s, uo)
            assert np.array_equal(occ, (s == 1) | ((s != 0) & (s != 1) & uo))
            d2 = {}
            for what, mask in (("occupied", occ), ("free", ~occ)):
                d2[what] = fusion.squared_distances(mask, R)
                assert d2[what].dtype == np.int64 and np.array_equal(d2[what], FC.scipy_d2(mask, R)), (name, R, uo, what)
                if s.size <= 512:
                    assert np.array_equal(d2[what], FC.brute_d2(mask, R)), (name, R, uo, what)
            vol = fusion.signed_volume(s, delta, R, uo)
            want = np.where(occ, -((np.sqrt(d2["free"].astype(np.float64)) - 0.5) * delta), (np.sqrt(d2["occupied"].astype(np.float64)) - 0.5) * delta)
            assert vol.dtype == np.float32 and vol.shape == s.shape and np.array_equal(FC.bits(vol), FC.bits(want.astype(np.float32)))
            half = np.float32(0.5 * delta)
            assert (vol[occ] <= -half).all() and (vol[~occ] >= half).all() and np.abs(vol).max() <= np.float32((R - 0.5) * delta)
            if occ.all() or not occ.any():  # constant: saturated everywhere
                assert (vol == np.float32((-1 if occ.all() else 1) * (R - 0.5) * delta)).all()
            got = fusion.distance_transform(s.ravel(), [((0.0, 0.0, 0.0), delta, "centre", s.shape)], R, uo)
            assert len(got) == 1 and np.array_equal(FC.bits(got[0]), FC.bits(vol))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the carve rule at its edges
# ---------------------------------------------------------------------------------------------------------------------
def _carve(volume, images, band=0.25, near=0.0, views=None, **kw):
    from omg_planner_amd import fusion
    images = np.asarray(images, np.float64)
    views = [FC.view()] * len(images) if views is None else views
    return fusion.carve_views([volume], views, [(0, len(images))], images, band, near, **kw).tolist()


def test_carve_edge_cases_as_known_answers():
    """One camera at the grid's origin looking along its +z with fx = fy = 1, cx = cy = 0: node (x, y, z) falls on column
    floor(x / z + 0.5) and row floor(y / z + 0.5)."""
    from omg_planner_amd import fusion
    F, S, U = fusion.FREE, fusion.SURFACE, fusion.UNKNOWN
    assert (F, S, U) == (0, 1, 2)
    line = FC.line_volume
    # no views: nothing is known
    assert _carve(line([1.0, 2.0, 3.0]), np.zeros((0, 1, 1))) == [U, U, U]
    # z exactly at near gives no information (the test is z > near)
    assert _carve(line([0.5, 1.0, 1.5]), [[[INF]]], near=1.0) == [U, U, F]
    # columns: x / z = -0.75 .. 1.75 in steps of 0.25 on an image of W = 2.  -0.5 is the left edge of pixel 0 (inside),
    # 1.5 = W - 0.5 the right edge of pixel 1 (outside)
    xs = ((-0.75, 0.0, 1.0), 0.25, "node", (11, 1, 1))
    assert _carve(xs, [[[INF, INF]]]) == [U, F, F, F, F, F, F, F, F, U, U]
    ys = ((0.0, -0.75, 1.0), 0.25, "node", (1, 11, 1))  # rows alike, on an image of H = 2
    assert _carve(ys, [[[INF], [INF]]]) == [U, F, F, F, F, F, F, F, F, U, U]
    assert _carve(ys, [[[INF, INF]]]) == [U, F, F, F, F, U, U, U, U, U, U]  # H = 1: rows -0.5 .. 0.25 only
    # (voxel centres: the same nodes from an origin half a voxel lower)
    assert _carve(((-0.875, -0.125, 0.875), 0.25, "centre", (11, 1, 1)), [[[INF, INF]]]) == [U, F, F, F, F, F, F, F, F, U, U]
    # depth values that say nothing: NaN, 0, negative; +inf frees
    assert _carve(((0.0, 0.0, 1.0), 1.0, "node", (4, 1, 1)), [[[NAN, 0.0, -1.0, INF]]]) == [U, U, U, F]
    # z exactly at d - band and d + band is surface; in front free, behind nothing
    assert _carve(line([1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75]), [[[2.0]]], band=0.5) == [F, S, S, S, S, S, U]
    # surface in one view and free in another: surface; behind one surface and free in the other: free
    assert _carve(line([2.0, 3.0]), [[[2.0]], [[INF]]], band=0.5) == [S, F]
    assert _carve(line([2.0, 3.0]), [[[INF]], [[2.0]]], band=0.5) == [S, F]
    # a view with its own intrinsics and a camera moved back by 1: z_cam = z + 1, column floor(2 * x / z_cam + 1 + 0.5)
    moved = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 1.0]])
    assert _carve(((-1.0, 0.0, 1.0), 0.5, "node", (5, 1, 1)), [[[INF, 3.0, 2.0]]], views=[FC.view(2.0, 2.0, 1.0, 0.0, moved)]) == [F, F, F, S, S]
    # view ranges: volume 0 sees image 1 only, volume 1 both, volume 2 none
    vols = [line([2.0, 3.0])] * 3
    got = fusion.carve_views(vols, [FC.view()] * 2, [(1, 1), (0, 2), (2, 0)], np.array([[[INF]], [[2.0]]]), 0.5, 0.0)
    assert got.tolist() == [S, U, S, F, U, U] and fusion.state_offsets(vols).tolist() == [0, 2, 4, 6]
    # the caller's offsets: elements outside every range keep what they held
    got = fusion.carve_views(vols[:1], [FC.view()], [(0, 1)], np.array([[[INF]]]), 0.5, 0.0, state=np.full(5, 9, np.uint8), state_begin=[2])
    assert got.tolist() == [9, 9, F, F, 9]
    for bad in (dict(band=NAN), dict(near=INF), dict(views=[FC.view(fx=0.0)]), dict(views=[FC.view(cx=NAN)])):
        with pytest.raises(ValueError):
            _carve(line([1.0, 2.0]), [[[INF]]], **bad)
    for bad_range in ([(0, 2)], [(-1, 1)], [(1, 1)]):
        with pytest.raises(ValueError):
            fusion.carve_views([line([1.0, 2.0])], [FC.view()], bad_range, np.array([[[INF]]]), 0.5, 0.0)
    for bad_radius in (0, 256):
        with pytest.raises(ValueError):
            fusion.distance_transform(np.zeros(2, np.uint8), [line([1.0, 2.0])], bad_radius)


def test_carve_edges_as_one_ragged_batch_of_known_answers():
    """The same edges on images of one size with one band and one near (FC.EDGE_CASES), so that they can go through ONE launch on
    the device (tests/test_gpu_fusion.py): the specification gives the answers written out there, volume by volume."""
    from omg_planner_amd import fusion
    volumes, ranges = [c[1] for c in FC.EDGE_CASES], [c[2] for c in FC.EDGE_CASES]
    got = fusion.carve_views(volumes, FC.edge_views(), ranges, FC.EDGE_DEPTH, FC.EDGE_BAND, FC.EDGE_NEAR)
    at = fusion.state_offsets(volumes)
    for m, (what, _, _, answer) in enumerate(FC.EDGE_CASES):
        assert got[at[m]: at[m + 1]].tolist() == answer, what
    assert len(got) == at[-1] == sum(len(c[3]) for c in FC.EDGE_CASES)


def test_merge_of_two_carves_equals_one_carve_of_all_views():
    from omg_planner_amd import fusion
    t, views = FC.scene_depth()
    first = fusion.carve_views([FC.SCENE_VOLUME], views, [(0, 1)], t, FC.BAND, FC.NEAR)
    both = fusion.carve_views([FC.SCENE_VOLUME], views, [(1, 2)], t, FC.BAND, FC.NEAR, state=first)
    assert np.array_equal(both.reshape(FC.DIMS), FC.scene_states(3)) and not np.array_equal(first.reshape(FC.DIMS), FC.scene_states(3))
    assert np.array_equal(first.reshape(FC.DIMS), FC.scene_states(1))  # the first call's array is not changed by the merge


# ---------------------------------------------------------------------------------------------------------------------
# 3. the observed scene
# ---------------------------------------------------------------------------------------------------------------------
def test_observed_scene_of_a_sphere_above_a_slab():
    """icosphere(2, 0.06) at (0, 0, 0.08) above the slab box (0.25, 0.25, 0.01), seen by one and by three 64 x 48 cameras, fused on
    a 32 x 32 x 24 grid of 1 cm.
    a: no node deeper inside the analytic solid than sqrt(1/2) * z / f (the pixel-centre ray passes no further from it) is FREE.
       Measured: the depth is 8.2 mm (one view) and 8.6 mm (three), 624 and 552 such nodes, 0 of them FREE.
    b: more views only shrink the UNKNOWN set.
    c: with unknown_occupied, the fused value of a FREE node exceeds the analytic distance by at most band + (sqrt(3)/2) delta =
       0.0237.  Measured: 0.0095 (one view), 0.0078 (three views).
    d: the zero level set has vertices and faces, and every crossing lies at t = 0.5."""
    from omg_planner_amd import fusion, scenes
    t, views = FC.scene_depth()
    assert t.shape == (3, FC.H, FC.W) and 0.3 < np.isfinite(t).mean() < 0.9
    analytic, p = FC.scene_analytic()
    for nv in (1, 3):
        st = FC.scene_states(nv)
        assert all((st == k).sum() > 500 for k in (0, 1, 2))
        z = np.stack([((views[v][12] * p[:, 0] + views[v][13] * p[:, 1]) + views[v][14] * p[:, 2]) + views[v][15] for v in range(nv)])
        depth = np.sqrt(0.5) * z.max() / FC.F
        deep = -analytic > depth
        print(nv, "views: depth", depth, "deep nodes", int(deep.sum()), "of them free", int((st[deep] == fusion.FREE).sum()))
        assert depth < 0.0089 and deep.sum() >= 500 and (st[deep] != fusion.FREE).all()                                   # a
        vol = FC.scene_volume(nv)
        excess = (vol.astype(np.float64) - analytic)[st == fusion.FREE].max()
        print(nv, "views: fused - analytic on free nodes, max", excess)
        assert excess <= FC.BAND + np.sqrt(3.0) / 2.0 * FC.DELTA                                                          # c
        v, f, _ = scenes.surface_nets(vol, np.array(FC.ORIGIN), FC.DELTA, "centre", 0.0)
        assert len(v) > 500 and len(f) > 1000                                                                             # d
        half, crossings = np.float32(0.5 * FC.DELTA), 0
        for axis in range(3):
            a, b = np.moveaxis(vol, axis, 0)[:-1], np.moveaxis(vol, axis, 0)[1:]
            cross = (a < 0) != (b < 0)
            crossings += int(cross.sum())
            assert (np.abs(a[cross]) == half).all() and (a[cross] == -b[cross]).all()  # t = (0 - a) / (b - a) = 0.5
        assert crossings > 1000
    assert not ((FC.scene_states(3) == fusion.UNKNOWN) & (FC.scene_states(1) != fusion.UNKNOWN)).any()                   # b
    grids = fusion.fuse_views([FC.SCENE_VOLUME], views, [(0, 3)], t, FC.BAND, FC.NEAR, FC.RADIUS)
    assert np.array_equal(FC.bits(grids[0].data), FC.bits(FC.scene_volume(3))) and grids[0].delta == FC.DELTA and np.array_equal(grids[0].origin, FC.ORIGIN)
    assert fusion.obstacle_radius(0.1, 0.01) == 12 and fusion.obstacle_radius(0.23, 0.02) == 13


# ---------------------------------------------------------------------------------------------------------------------
# 4. csrc/omg_fusion_body.h on the host
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include "omg_fusion_body.h"
// One volume, node by node in x-major order, as k_carve_views visits them.
extern "C" void host_carve(const double* origin, double delta, double offset, const int32_t* n, const double* views, int v0, int count,
                           const double* depth, int H, int W, double band, double near, int merge, uint8_t* state) {
    int64_t id = 0;
    for (int i = 0; i < n[0]; ++i)
        for (int j = 0; j < n[1]; ++j)
            for (int k = 0; k < n[2]; ++k, ++id) {
                double p[3];
                fusion_node_point(origin, delta, offset, i, j, k, p);
                bool surface = merge && state[id] == FUSION_SURFACE, free_ = merge && state[id] == FUSION_FREE;
                for (int v = v0; v < v0 + count; ++v) {
                    const int says = fusion_view_says(views + 16 * v, depth + (int64_t)v * H * W, H, W, p, band, near);
                    surface = surface || says == FUSION_SAYS_SURFACE, free_ = free_ || says == FUSION_SAYS_FREE;
                }
                state[id] = fusion_state(surface, free_);
            }
}
// The three passes of one volume as the kernels make them: seeds, z (stride 1), y (stride nz), x (stride ny * nz), the value.
extern "C" void host_transform(const uint8_t* state, const int32_t* n, int radius, int unknown_occupied, double delta, uint32_t* a,
                               uint32_t* b, float* out) {
    const int64_t nx = n[0], ny = n[1], nz = n[2], total = nx * ny * nz;
    const uint32_t r2 = (uint32_t)(radius * radius);
    for (int64_t id = 0; id < total; ++id) b[id] = fusion_seed(fusion_occupied(state[id], unknown_occupied), r2);
    for (int64_t id = 0; id < total; ++id) a[id] = fusion_line_pass(b + id, 1, (int)(id % nz), (int)nz, radius, r2);
    for (int64_t id = 0; id < total; ++id) b[id] = fusion_line_pass(a + id, nz, (int)(id / nz % ny), (int)ny, radius, r2);
    for (int64_t id = 0; id < total; ++id) out[id] = fusion_value(fusion_line_pass(b + id, ny * nz, (int)(id / (ny * nz)), (int)nx, radius, r2), delta);
}
"""


def _host_lib(tmp_path):
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    return KB.host_harness(_HOST_HARNESS, tmp_path, {"host_carve": (None, [vp, d, d, vp, vp, i, i, vp, i, i, d, d, i, vp]),
                                                     "host_transform": (None, [vp, vp, i, i, d, vp, vp, vp])})


def host_carve(lib, volume, views, view_range, depth, band, near, state=None):
    origin, delta, sample, dims = volume[:4]
    origin, n = np.asarray(origin, np.float64), np.array(dims, np.int32)
    views, depth = np.ascontiguousarray(views, np.float64).reshape(-1, 16), np.ascontiguousarray(depth, np.float64)
    out = np.full(int(n.prod()), 9, np.uint8) if state is None else np.array(state, np.uint8)
    lib.host_carve(origin.ctypes.data, float(delta), {"centre": 0.5, "node": 0.0}[sample], n.ctypes.data, views.ctypes.data, int(view_range[0]),
                   int(view_range[1]), depth.ctypes.data, depth.shape[-2], depth.shape[-1], float(band), float(near), int(state is not None),
                   out.ctypes.data)
    return out


def host_transform(lib, state, delta, radius, unknown_occupied):
    state = np.ascontiguousarray(state, np.uint8)
    n = np.array(state.shape, np.int32)
    a, b, out = np.zeros(state.size, np.uint32), np.zeros(state.size, np.uint32), np.zeros(state.shape, np.float32)
    lib.host_transform(state.ctypes.data, n.ctypes.data, int(radius), int(bool(unknown_occupied)), float(delta), a.ctypes.data, b.ctypes.data,
                       out.ctypes.data)
    return out


@KB.requires_host_cxx
def test_kernel_body_compiled_for_the_host_equals_the_specification(tmp_path):
    """csrc/omg_fusion_body.h is what a thread of the kernels does for its node; compiled for the host without contraction and
    walked node by node it gives the specification's states and its float32 volumes as uint32 bits: on the transform grids, the
    shapes that straddle a chunk (radius 1, 5, 70, 255), the scene, a ragged batch with both sample offsets, and the carve edges."""
    from omg_planner_amd import _lib, fusion
    assert _lib.FUSION_CHUNK == FC.CHUNK and _lib.FUSION_MAX_RADIUS == fusion.MAX_RADIUS == 255
    lib = _host_lib(tmp_path)
    nodes = 0
    for names, radii in ((FC.TRANSFORM, FC.RADII), (FC.STRADDLE, FC.STRADDLE_RADII)):
        for name in names:
            s = FC.states(name)
            for R in radii:
                for uo in (False, True):
                    want = fusion.signed_volume(s, 0.0125, R, uo)
                    assert np.array_equal(FC.bits(host_transform(lib, s, 0.0125, R, uo)), FC.bits(want)), (name, R, uo)
                    nodes += s.size
    t, views = FC.scene_depth()
    for nv in (1, 3):
        st = host_carve(lib, FC.SCENE_VOLUME, views, (0, nv), t, FC.BAND, FC.NEAR)
        assert np.array_equal(st.reshape(FC.DIMS), FC.scene_states(nv))
        for uo in (False, True):
            assert np.array_equal(FC.bits(host_transform(lib, FC.scene_states(nv), FC.DELTA, FC.RADIUS, uo)), FC.bits(FC.scene_volume(nv, uo)))
    merged = host_carve(lib, FC.SCENE_VOLUME, views, (1, 2), t, FC.BAND, FC.NEAR, state=FC.scene_states(1).ravel())
    assert np.array_equal(merged.reshape(FC.DIMS), FC.scene_states(3))
    want = fusion.carve_views(FC.RAGGED, views, FC.RAGGED_RANGES, t, FC.BAND, FC.NEAR)
    begin = fusion.state_offsets(FC.RAGGED)
    for m, vol in enumerate(FC.RAGGED):
        assert np.array_equal(host_carve(lib, vol, views, FC.RAGGED_RANGES[m], t, FC.BAND, FC.NEAR), want[begin[m]: begin[m + 1]]), m
    # the carve edges: the same known answers
    inf_row = np.array([[[INF, INF]]])
    assert host_carve(lib, ((-0.75, 0.0, 1.0), 0.25, "node", (11, 1, 1)), [FC.view()], (0, 1), inf_row, 0.25, 0.0).tolist() == [2] + [0] * 8 + [2, 2]
    assert host_carve(lib, ((0.0, 0.0, 1.0), 1.0, "node", (4, 1, 1)), [FC.view()], (0, 1), np.array([[[NAN, 0.0, -1.0, INF]]]), 0.25, 0.0).tolist() == [2, 2, 2, 0]
    assert host_carve(lib, FC.line_volume([1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75]), [FC.view()], (0, 1), np.array([[[2.0]]]), 0.5, 0.0).tolist() == [0, 1, 1, 1, 1, 1, 2]
    assert host_carve(lib, FC.line_volume([0.5, 1.0, 1.5]), [FC.view()], (0, 1), np.array([[[INF]]]), 0.25, 1.0).tolist() == [2, 2, 0]
    assert host_carve(lib, FC.line_volume([1.0, 2.0]), np.zeros((0, 16)), (0, 0), np.zeros((0, 1, 1)), 0.25, 0.0).tolist() == [2, 2]
    for what, vol, rng_, answer in FC.EDGE_CASES:
        assert host_carve(lib, vol, FC.edge_views(), rng_, FC.EDGE_DEPTH, FC.EDGE_BAND, FC.EDGE_NEAR).tolist() == answer, what
    assert nodes > 40000  # (the transform cases alone: 43 356 nodes)


@KB.requires_host_cxx
def test_fuzz_generator_against_the_body_compiled_for_the_host(tmp_path):
    """The generator of tests/fuzz/fuzz_fusion.py without a GPU: the draws of the GPU test's seed through the body header on the
    host equal the specification, and between them they reach every state, both flags, empty view ranges and a 1 x 1 image."""
    import importlib.util
    from pathlib import Path
    from omg_planner_amd import fusion
    spec = importlib.util.spec_from_file_location("fuzz_fusion", Path(__file__).resolve().parent / "fuzz" / "fuzz_fusion.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    lib = _host_lib(tmp_path)
    rng = np.random.default_rng(fuzz.SMOKE_SEED)
    seen, flags, empty, tiny, radii, counts = np.zeros(3, np.int64), set(), 0, 0, set(), set()
    for _ in range(fuzz.SMOKE_TRIALS):
        c = fuzz.draw(rng)
        want_state = fusion.carve_views(c["volumes"], c["views"], c["ranges"], c["depth"], c["band"], c["near"],
                                        state=np.full(c["state_elems"], fuzz.GUARD_STATE, np.uint8), state_begin=c["begin"])
        want = fusion.distance_transform(want_state, c["volumes"], c["radius"], c["unknown_occupied"], state_begin=c["begin"])
        for m, v in enumerate(c["volumes"]):
            n, b = int(np.prod(v[3])), int(c["begin"][m])
            depth = c["depth"] if len(c["depth"]) else np.zeros((1, 1, 1))  # (no view: the image is never read)
            got = host_carve(lib, v, c["views"], c["ranges"][m], depth, c["band"], c["near"])
            assert np.array_equal(got, want_state[b: b + n]), (v[3], c["ranges"][m])
            vol = host_transform(lib, got.reshape(v[3]), v[1], c["radius"], c["unknown_occupied"])
            assert np.array_equal(FC.bits(vol), FC.bits(want[m])), (v[3], c["radius"])
            seen += [(got == k).sum() for k in (0, 1, 2)]
            empty += c["ranges"][m][1] == 0
        flags.add(c["unknown_occupied"])
        tiny += c["depth"].shape[1:] == (1, 1) and len(c["views"]) > 0
        radii.add(c["radius"]), counts.add(len(c["views"]))
    print("states free / surface / unknown", seen.tolist(), "empty ranges", empty, "1 x 1 images", tiny)
    assert (seen > 1000).all() and flags == {False, True} and empty > 0 and tiny > 0 and radii == set(fuzz.RADII) and counts == {0, 1, 2, 3, 4}


# ---------------------------------------------------------------------------------------------------------------------
# 5. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _volumes(M=2, **over):
    from omg_planner_amd import _lib
    rec = (_lib.Mesh * M)()
    for m in range(M):
        r = rec[m]
        r.origin[:], r.delta, r.sample_offset, r.dims[:] = [0.0, 0.0, 0.0], 0.01, 0.5, [4, 5, 6 + m]
        r.out_offset, r.first_workgroup = 1000 * m, m
    for k, val in over.items():
        if k in ("origin", "dims"):
            getattr(rec[M - 1], k)[:] = val
        else:
            setattr(rec[M - 1], k, val)
    return rec


def test_c_abi_argument_checks_without_gpu():
    """Every OMGX_ERR_INVALID / OMGX_ERR_UNSUPPORTED case of the three entry points is decided on the host copies before any HIP
    call."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    assert lib.omgx_abi_version() == 14 and _lib.FUSION_NODES_PER_WORKGROUP == 256 and len(_lib.STRUCTS) == 8
    INV, UNS, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED, _lib.OMGX_OK
    vpc = lambda x: C.cast(x, C.c_void_p)
    arr = lambda a: C.c_void_p(a.ctypes.data)
    d = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    good_views = np.stack([FC.view(2.0, 3.0, 1.0, 1.0)] * 3)

    def nbytes(rec, M=None, radius=3):
        return lib.omgx_distance_transform_workspace_bytes(vpc(rec), len(rec) if M is None else M, radius)

    # two 4-byte intermediates per node of every workgroup of 256
    assert nbytes(_volumes()) == 2 * 256 * 8 and nbytes(_volumes(1, dims=[4, 8, 9])) == 2 * 256 * 8 and nbytes(_volumes(1, dims=[64, 64, 64])) == 8 << 18
    assert nbytes(_volumes(), M=0) == 0 and lib.omgx_distance_transform_workspace_bytes(None, 0, 1) == 0
    assert nbytes(_volumes(), M=-1) == INV and lib.omgx_distance_transform_workspace_bytes(None, 1, 1) == INV and nbytes(_volumes(dims=[0, 4, 4])) == INV
    assert nbytes(_volumes(), radius=0) == INV and nbytes(_volumes(), radius=256) == UNS and nbytes(_volumes(), radius=255) == 2 * 256 * 8
    assert nbytes(_volumes(first_workgroup=2)) == INV and nbytes(_volumes(1, dims=[2048, 1024, 1024])) == UNS

    def carve(rec=None, M=None, views=good_views, V=None, ranges=None, begin=(0, 120), H=4, W=5, band=0.01, near=0.05, merge=0,
              state_elems=1 << 20, pool_elems=None, host=True, **ptr):
        rec = _volumes() if rec is None else rec
        views = np.ascontiguousarray(views, np.float64)
        ranges = np.ascontiguousarray([(0, 3), (1, 2)] + [(0, 1)] * (len(rec) - 2) if ranges is None else ranges, np.int32)
        begin = np.ascontiguousarray(begin, np.int64)
        assert len(ranges) >= len(rec) and len(begin) >= len(rec)
        p = dict(volumes=d, views=d, view_range=d, state_begin=d, depth=d, state=d, h_views=arr(views), h_view_range=arr(ranges),
                 h_state_begin=arr(begin), h_volumes=vpc(rec) if host else None)
        p.update(ptr)
        return lib.omgx_carve_views(p["volumes"], p["h_volumes"], len(rec) if M is None else M, p["views"], p["h_views"], len(views) if V is None else V,
                                    p["view_range"], p["h_view_range"], p["state_begin"], p["h_state_begin"], p["depth"], H, W, band, near, merge,
                                    p["state"], state_elems, None)

    def transform(rec=None, M=None, begin=(0, 120), radius=3, state_elems=1 << 20, pool_elems=1 << 20, host=True, **ptr):
        rec = _volumes() if rec is None else rec
        begin = np.ascontiguousarray(begin, np.int64)
        p = dict(state=d, state_begin=d, volumes=d, workspace=d, pool=d, h_state_begin=arr(begin), h_volumes=vpc(rec) if host else None)
        p.update(ptr)
        return lib.omgx_distance_transform(p["state"], state_elems, p["state_begin"], p["h_state_begin"], p["volumes"], p["h_volumes"],
                                           len(rec) if M is None else M, radius, 1, p["workspace"], p["pool"], pool_elems, None)

    for k in ("volumes", "h_volumes", "views", "h_views", "view_range", "h_view_range", "state_begin", "h_state_begin", "depth", "state"):
        assert carve(**{k: None}) == INV, k
    for k in ("state", "state_begin", "h_state_begin", "volumes", "h_volumes", "workspace", "pool"):
        assert transform(**{k: None}) == INV, k
    # M == 0 launches nothing; so does V == 0 need no images
    assert carve(M=0) == OK and transform(M=0) == OK and carve(M=0, volumes=None, h_volumes=None, state=None) == OK
    assert transform(M=0, volumes=None, h_volumes=None, state=None, pool=None, workspace=None) == OK
    assert carve(M=-1) == INV and transform(M=-1) == INV and carve(V=-1) == INV and carve(state_elems=-1) == INV
    assert transform(state_elems=-1) == INV and transform(pool_elems=-1) == INV
    assert carve(H=0) == INV and carve(W=0) == INV and carve(H=-3) == INV
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert carve(band=bad) == INV and carve(near=bad) == INV
    for col in range(16):  # every view field must be finite
        for bad in (NAN, INF):
            v = good_views.copy()
            v[2, col] = bad
            assert carve(views=v) == INV, (col, bad)
    for col in (0, 1):  # fx, fy
        v = good_views.copy()
        v[1, col] = 0.0
        assert carve(views=v) == INV
    for ranges in (((0, 4), (1, 2)), ((0, 3), (3, 1)), ((-1, 2), (1, 2)), ((0, 3), (1, -1))):
        assert carve(ranges=ranges) == INV, ranges
    for fn in (carve, transform):
        for dims in ([0, 4, 4], [4, -1, 4], [4, 4, 0]):
            assert fn(rec=_volumes(dims=dims)) == INV, dims
        for delta in (0.0, -0.01, NAN, INF):
            assert fn(rec=_volumes(delta=delta)) == INV, delta
        for off in (0.25, 1.0, -0.5, NAN):
            assert fn(rec=_volumes(sample_offset=off)) == INV, off
        for origin in ([NAN, 0, 0], [0, INF, 0], [0, 0, -INF]):
            assert fn(rec=_volumes(origin=origin)) == INV, origin
        for wg in (0, 2, -1):
            assert fn(rec=_volumes(first_workgroup=wg)) == INV, wg
        assert fn(rec=_volumes(out_offset=-1)) == INV
        # state ranges: outside [0, state_elems), or two that overlap
        assert fn(begin=(-1, 120)) == INV and fn(begin=(0, (1 << 20) - 139)) == INV and fn(state_elems=120 + 139) == INV
        assert fn(begin=(0, 119)) == INV and fn(begin=(100, 0)) == INV and fn(begin=(139, 0)) == INV
        # limits: an invalid record of any volume is reported first
        assert fn(rec=_volumes(1, dims=[2048, 1024, 1024]), begin=(0,), state_elems=1 << 40, pool_elems=1 << 40) == UNS  # 2^31 nodes
        huge = _volumes(3, dims=[2048, 1024, 1024])
        huge[0].dims[:], huge[1].dims[:] = [2047, 1024, 1024], [1, 1, 1]
        huge[0].out_offset, huge[1].out_offset, huge[2].out_offset = 0, 1 << 32, 1 << 33
        huge[1].first_workgroup, huge[2].first_workgroup = 2047 * 4096, 2047 * 4096 + 1
        assert fn(rec=huge, begin=(0, 1 << 32, 1 << 33), state_elems=1 << 40, pool_elems=1 << 40) == UNS
        huge[1].delta = 0.0
        assert fn(rec=huge, begin=(0, 1 << 32, 1 << 33), state_elems=1 << 40, pool_elems=1 << 40) == INV
    # 257 volumes of 2047 * 2^20 nodes: 257 * 8 384 512 workgroups are more than 2^31 - 1
    many = _volumes(257, dims=[2047, 1024, 1024])
    for m in range(257):
        many[m].dims[:], many[m].out_offset, many[m].first_workgroup = [2047, 1024, 1024], m << 31, m * 2047 * 4096
    begin = [m << 31 for m in range(257)]
    assert carve(rec=many, ranges=[(0, 1)] * 257, begin=begin, state_elems=1 << 40) == UNS
    assert transform(rec=many, begin=begin, state_elems=1 << 40, pool_elems=1 << 40) == UNS
    # V * H * W > 2^31 - 1
    assert carve(V=3, H=1 << 15, W=1 << 15) == UNS and carve(H=1 << 15, W=21846) == UNS and carve(M=0, H=1 << 15, W=1 << 15) == UNS
    # the transform alone: the radius, the volumes' place in the pool
    assert transform(radius=0) == INV and transform(radius=-4) == INV and transform(radius=256) == UNS and transform(M=0, radius=256) == UNS
    assert transform(rec=_volumes(out_offset=(1 << 20) - 139)) == INV and transform(pool_elems=1000 + 139) == INV
    assert transform(rec=_volumes(out_offset=119)) == INV and transform(rec=_volumes(out_offset=0)) == INV  # two volumes overlap in the pool
    assert transform(rec=_volumes(first_workgroup=2), radius=256) == INV  # invalid before unsupported


def test_wrapper_checks_without_gpu():
    import torch
    from omg_planner_amd import _lib, camera, ops
    E = _lib.OmgHipError
    vols = [((0.0, 0.0, 0.0), 0.01, "centre", (4, 4, 4), 0)]
    depth = torch.zeros((1, 4, 4), dtype=torch.float64)
    with pytest.raises(E, match="device tensor"):
        ops.carve_views(vols, [FC.view()], [(0, 1)], depth, 0.01, 0.05)
    with pytest.raises(E, match="tensor"):
        ops.carve_views(vols, [FC.view()], [(0, 1)], depth.numpy(), 0.01, 0.05)
    with pytest.raises(E, match="device tensor"):
        ops.distance_transform(torch.zeros(64, dtype=torch.uint8), None, vols, 3)
    with pytest.raises(E, match="device tensor"):
        ops.fuse_views(vols, [FC.view()], [(0, 1)], depth, 0.01, 0.05, 3)
    assert hasattr(ops.DeviceScenes, "fuse_obstacles") and hasattr(camera.Observation, "fuse_obstacles")
    # the host arguments are checked before the tensors, so every one of these is refused without a GPU
    good = dict(volumes=vols, views=[FC.view()], view_range=[(0, 1)], depth=depth, band=0.01, near=0.05)
    bad_view = lambda col, x: [np.concatenate([FC.view()[:col], [x], FC.view()[col + 1:]])]
    for what, change in (("2 views but 1 images", dict(views=[FC.view()] * 2)), ("0 views but 1 images", dict(views=np.zeros((0, 16)))),
                         ("not finite or has a focal length of zero", dict(views=bad_view(7, NAN))),
                         ("not finite or has a focal length of zero", dict(views=bad_view(2, INF))),
                         ("not finite or has a focal length of zero", dict(views=bad_view(0, 0.0))),
                         ("not finite or has a focal length of zero", dict(views=bad_view(1, 0.0))),
                         ("band and near must be finite", dict(band=NAN)), ("band and near must be finite", dict(band=INF)),
                         ("band and near must be finite", dict(near=NAN)), ("band and near must be finite", dict(near=-INF)),
                         ("view_range", dict(view_range=[(0, 2)])), ("view_range", dict(view_range=[(1, 1)])), ("view_range", dict(view_range=[(-1, 1)])),
                         ("view_range", dict(view_range=[(0, -1)])), ("view_range", dict(view_range=[(0, 1), (0, 1)])), ("view_range", dict(view_range=[])),
                         ("merge needs the state", dict(merge=True)), ("one offset per volume", dict(state_begin=[0, 64])),
                         ("depth must be a tensor", dict(depth=depth[0])), ("sample must be", dict(volumes=[vols[0][:2] + ("corner",) + vols[0][3:]])),
                         ("dims >= 1", dict(volumes=[vols[0][:3] + ((4, 0, 4), 0)])), ("delta must be positive", dict(volumes=[vols[0][:1] + (0.0,) + vols[0][2:]]))):
        with pytest.raises(E, match=what):
            ops.carve_views(**{**good, **change})
        if "merge" not in change and "state_begin" not in change:
            with pytest.raises(E, match=what):
                ops.fuse_views(**{**good, **change}, radius=3)
    state = torch.zeros(64, dtype=torch.uint8)
    for radius in (0, -3, 256, 1000):
        with pytest.raises(E, match=r"radius must lie in \[1, 255\]"):
            ops.distance_transform(state, None, vols, radius)
        with pytest.raises(E, match=r"radius must lie in \[1, 255\]"):
            ops.fuse_views(**good, radius=radius)
    with pytest.raises(E, match="one offset per volume"):
        ops.distance_transform(state, [0, 64], vols, 3)
    with pytest.raises(E, match="dims >= 1"):
        ops.distance_transform(state, None, [vols[0][:3] + ((4, 4, -1), 0)], 3)
    # layouts without an offset lie back to back; the states do by default
    b = ops._VolumeBatch([((0.0, 0.0, 0.0), 0.01, "centre", (2, 2, 2)), ((0.0, 0.0, 0.0), 0.01, "node", (1, 2, 3)),
                          ((0.0, 0.0, 0.0), 0.01, "node", (3, 1, 1), 100)], None)
    assert [r.out_offset for r in b.rec] == [0, 8, 100] and b.nodes.tolist() == [8, 6, 3] and b.begin.tolist() == [0, 8, 14]
    b = ops._VolumeBatch([], None)
    assert [len(x) for x in (b.rec, b.nodes, b.begin)] == [0, 0, 0]
    with pytest.raises(E):
        ops._VolumeBatch([((0.0, 0.0, 0.0), 0.01, "centre")], None)
    with pytest.raises(E, match="one offset per volume"):
        ops._VolumeBatch(vols, [0, 1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. registers
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_fusion_kernels_do_not_spill(tmp_path):
    """The compiler's resource remarks for csrc/omg_fusion.hip: no kernel uses scratch or spills, every one leaves room for eight
    waves per SIMD, and the z pass's static LDS is the 256 + 2 * 255 seeds."""
    seen = KB.kernel_resources("omg_fusion.hip", tmp_path)
    assert len(seen) == 4
    for part in ("k_carve_views", "k_fusion_rows", "k_fusion_slabILb0", "k_fusion_slabILb1"):
        v = KB.one(seen, part)
        print(part, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs"] <= 64, (part, v)
    assert KB.one(seen, "k_fusion_rows")["LDS Size [bytes/block]"] == 4 * (256 + 2 * 255)
