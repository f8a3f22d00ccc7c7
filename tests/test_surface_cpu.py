"""CPU tests of surface extraction (omg-planner_amd/scenes.py surface_nets, csrc/omg_surface.hip): the
specification's meshes are closed, oriented and of the right volume, go back through scenes.mesh_sdf to the volume they came
from, and do what the text says at its edges; csrc/omg_surface_body.h compiled for the host equals the specification bit for bit;
every argument error of the C ABI and of the wrappers; the kernels use no scratch."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import kernel_build as KB
from tests import surface_cases as SC


# ---------------------------------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.N24)
def test_specification_meshes_are_closed_oriented_and_of_the_right_volume(name):
    from omg_planner_amd import grasps
    shape, level = name.rsplit("_", 2)[0], float(name.rsplit("_", 1)[1])
    v, f, open_edges = SC.spec(name)
    assert open_edges == 0 and SC.unpaired_directed_edges(f) == 0
    comps = SC.components(len(v), f)
    assert comps == SC.COMPONENTS[(shape, level)] and SC.euler(len(v), f) == 2 * comps
    assert SC.zero_area_faces(v, f) == 0 and f.min() == 0 and f.max() == len(v) - 1
    vol = SC.signed_volume(v, f)
    print(name, len(v), len(f), vol / SC.ANALYTIC_VOLUME[shape])
    assert vol > 0
    if level == 0.0:
        assert abs(vol / SC.ANALYTIC_VOLUME[shape] - 1.0) < 0.10
    else:  # the shape dilated by 10 mm: larger than the shape itself
        at_zero = SC.spec(f"{shape}_{name.rsplit('_', 2)[1]}_0.0")
        assert vol > SC.signed_volume(at_zero[0], at_zero[1]) and vol > SC.ANALYTIC_VOLUME[shape]
    ov, of = grasps.outward_mesh(v, f)
    assert np.array_equal(of, f) and np.array_equal(SC.bits(ov), SC.bits(v))
    c = SC.case(name)  # every vertex lies inside its cell
    u = (v - c["origin"]) / c["delta"] - SC.OFFSET[c["sample"]]
    assert u.min() >= -1e-9 and (u.max(0) <= np.array(c["data"].shape) - 1 + 1e-9).all()


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_round_trip_through_mesh_sdf(shape):
    """scenes.mesh_sdf of the extracted surface on the volume's own grid: a vertex never leaves its cell, so the surface moves by
    less than one cell diagonal; and no node further than that from the surface changes its sign.  Measured: 0.084 delta on the
    sphere, 0.135 delta on the two spheres, 0.58 delta on the box (its cut corners)."""
    from omg_planner_amd import scenes
    c = SC.case(f"{shape}_centre_0.0")
    v, f, _ = SC.spec(f"{shape}_centre_0.0")
    back = scenes.mesh_sdf(v, f, c["delta"], sample="centre", origin=c["origin"], dims=c["data"].shape).data
    bound = np.sqrt(3.0) * c["delta"]
    diff = np.abs(back.astype(np.float64) - c["data"].astype(np.float64))
    print(shape, diff.max() / c["delta"])
    assert diff.max() <= bound
    far = np.abs(c["data"]) > bound
    assert far.any() and np.array_equal(np.sign(back[far]), np.sign(c["data"][far]))


def _closed(name):
    v, f, o = SC.spec(name)
    return o == 0 and len(f) > 0 and SC.unpaired_directed_edges(f) == 0


def test_edge_cases_of_the_text():
    from omg_planner_amd import scenes
    # one cell: one vertex, no cell has four neighbours, every crossing edge is open
    v, f, o = SC.spec("2x2x2")
    assert v.shape == (1, 3) and f.shape == (0, 3) and o == 3
    # (-1 at corner 000, +1 at its three neighbours: crossings at t = 0.5 on the three axes; voxel centres at 0.005)
    assert np.array_equal(SC.bits(v[0]), SC.bits(np.array([0.0 + ((0.0 + 0.5) + (0.5 + 0.0 + 0.0) / 3.0) * 0.01] * 3)))
    v, f, o = SC.spec("2x2x2_half")
    # (x = 0 all inside, x = 1 all outside: four open x edges at t = 0.5, 0.5, 0.5 and 3 / 5)
    assert v.shape == (1, 3) and len(f) == 0 and o == 4
    assert np.array_equal(SC.bits(v[0]), SC.bits(np.array([0.1 + ((0.0 + 0.0) + (((0.5 + 0.5) + 0.5) + 3.0 / 5.0) / 4.0) * 0.01,
                                                            0.2 + ((0.0 + 0.0) + 2.0 / 4.0) * 0.01, 0.3 + ((0.0 + 0.0) + 2.0 / 4.0) * 0.01])))
    for name in SC.EMPTY:
        v, f, o = SC.spec(name)
        assert v.shape == (0, 3) and v.dtype == np.float64 and f.shape == (0, 3) and f.dtype == np.int32, name
        ins = SC.case(name)["data"] < 0  # a dim of 1: no cell, so every crossing edge of the slab is open
        crossing = sum(int((np.diff(ins.astype(np.int8), axis=a) != 0).sum()) for a in range(3))
        assert o == crossing and (o > 0) == name.startswith("dim1"), name
    v, f, o = SC.spec("z2")  # one layer of cells: vertices but no closed edge along x or y
    assert len(v) > 0 and o > 0
    # a sphere larger than its grid: faces only where the four cells exist, open edges where they do not
    v, f, o = SC.spec("leaves_grid")
    assert o > 0 and len(f) > 0 and SC.unpaired_directed_edges(f) > 0 and f.min() >= 0 and f.max() < len(v)
    # samples that are not finite next to the surface: NaN is outside, t falls back to 0.5, every vertex stays finite and in its cell
    for name in ("nan_inside", "nan_outside", "plus_inf", "minus_inf", "inf_both", "equal_to_level", "padded", "cloud"):
        v, f, o = SC.spec(name)
        c = SC.case(name)
        assert _closed(name) and np.isfinite(v).all() and SC.zero_area_faces(v, f) == 0, name
        u = (v - c["origin"]) / c["delta"] - SC.OFFSET[c["sample"]]
        assert u.min() >= -1e-9 and (u.max(0) <= np.array(c["data"].shape) - 1 + 1e-9).all(), name
    assert len(SC.spec("nan_inside")[0]) != len(SC.spec("nan_outside")[0])  # a NaN where an inside sample was is a hole in the solid
    assert not np.array_equal(SC.spec("plus_inf")[0], SC.spec("nan_outside")[0])  # +inf gives t = 0 or 1, NaN gives 0.5
    # the filler of the padded layout is outside: the mesh is that of the 10^3 volume alone
    c = SC.case("padded")
    alone = scenes.surface_nets(c["data"][:10, :10, :10], c["origin"], c["delta"], "centre", 0.0)
    assert np.array_equal(SC.bits(alone[0]), SC.bits(SC.spec("padded")[0])) and len(alone[1]) == len(SC.spec("padded")[1])
    # the cloud: a closed surface with every point inside or within one cell of it
    c = SC.case("cloud")
    v, f, o = SC.spec("cloud")
    assert SC.signed_volume(v, f) > 0 and (c["points"].min(0) > v.min(0) - c["delta"]).all() and (c["points"].max(0) < v.max(0) + c["delta"]).all()
    # an SdfGrid is taken with its own origin and delta; bad arguments are refused
    g = scenes.SdfGrid(c["data"], c["origin"], c["delta"])
    assert np.array_equal(SC.bits(scenes.surface_nets(g, sample="node", level=0.015)[0]), SC.bits(v))
    for bad in (dict(sample="corner"), dict(level=float("nan")), dict(delta=0.0), dict(delta=float("inf"))):
        with pytest.raises(ValueError):
            scenes.surface_nets(g, **bad)
    with pytest.raises(ValueError):
        scenes.surface_nets(c["data"])
    with pytest.raises(ValueError):
        scenes.surface_nets(c["data"][0], c["origin"], c["delta"])


def test_save_obj_is_read_back_by_load_obj(tmp_path):
    from omg_planner_amd import scene_io
    v, f, _ = SC.spec("252")
    scene_io.save_obj(tmp_path / "m.obj", v, f)
    rv, rf = scene_io.load_obj(tmp_path / "m.obj")
    assert np.array_equal(SC.bits(rv), SC.bits(v)) and np.array_equal(np.asarray(rf, np.int32), f)
    scene_io.save_obj(tmp_path / "e.obj", np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError):
        scene_io.save_obj(tmp_path / "b.obj", v, f + len(v))


# ---------------------------------------------------------------------------------------------------------------------
# csrc/omg_surface_body.h on the host
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include "omg_surface_body.h"
// One volume, sample by sample in x-major order, as the kernels visit them: vertices first (index: the vertex of every sample's
// cell or -1), then the faces.  counts = (vertices, faces, open edges).
extern "C" void host_surface(const float* vol, const int32_t* n, const double* origin, double delta, double sample_offset, float level,
                             double* verts, int32_t* faces, int32_t* index, int32_t* counts) {
    int32_t V = 0, F = 0, open = 0;
    int64_t id = 0;
    for (int i = 0; i < n[0]; ++i)
        for (int j = 0; j < n[1]; ++j)
            for (int k = 0; k < n[2]; ++k, ++id) {
                float v[8];
                surface_load_corners(vol, n, i, j, k, v);
                const unsigned mask = surface_corner_mask(v, level);
                index[id] = -1;
                if (surface_cell_active(mask, n, i, j, k)) {
                    surface_cell_vertex(v, mask, level, i, j, k, origin, delta, sample_offset, verts + 3 * V);
                    index[id] = V++;
                }
            }
    const int64_t step[3] = {(int64_t)n[1] * n[2], n[2], 1};
    id = 0;
    for (int i = 0; i < n[0]; ++i)
        for (int j = 0; j < n[1]; ++j)
            for (int k = 0; k < n[2]; ++k, ++id) {
                float v[8];
                surface_load_corners(vol, n, i, j, k, v);
                const unsigned mask = surface_corner_mask(v, level);
                const int a[3] = {i, j, k};
                for (int axis = 0; axis < 3; ++axis) {
                    if (!surface_edge_crosses(mask, axis)) continue;
                    if (!surface_edge_closed(n, a, axis)) { ++open; continue; }
                    const int64_t s1 = step[(axis + 1) % 3], s2 = step[(axis + 2) % 3];
                    surface_edge_triangles((mask & 1u) != 0u, index[id - s1 - s2], index[id - s2], index[id], index[id - s1], faces + 3 * F);
                    F += 2;
                }
            }
    counts[0] = V, counts[1] = F, counts[2] = open;
}
"""


@KB.requires_host_cxx
def test_kernel_body_compiled_for_the_host_equals_the_specification(tmp_path):
    """csrc/omg_surface_body.h is what a thread of the kernels does for its sample; compiled for the host without contraction and
    walked sample by sample it gives the specification's vertices as int64 bits, its faces and its open edges on every case."""
    vp = C.c_void_p
    lib = KB.host_harness(_HOST_HARNESS, tmp_path, {"host_surface": (None, [vp, vp, vp, C.c_double, C.c_double, C.c_float, vp, vp, vp, vp])})
    samples = 0
    for name in SC.ALL:
        c = SC.case(name)
        want_v, want_f, want_o = SC.spec(name)
        n = np.array(c["data"].shape, np.int32)
        total = int(n.prod())
        verts, faces = np.full((total, 3), 7.0), np.full((6 * total, 3), -7, np.int32)
        index, counts = np.zeros(total, np.int32), np.zeros(3, np.int32)
        lib.host_surface(c["data"].ctypes.data, n.ctypes.data, c["origin"].ctypes.data, c["delta"], SC.OFFSET[c["sample"]], c["level"],
                         verts.ctypes.data, faces.ctypes.data, index.ctypes.data, counts.ctypes.data)
        assert counts.tolist() == [len(want_v), len(want_f), want_o], name
        assert np.array_equal(SC.bits(verts[: counts[0]]), SC.bits(want_v)) and np.array_equal(faces[: counts[1]], want_f), name
        samples += total
    assert samples >= 100000


# ---------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _volumes(M=2, **over):
    from omg_planner_amd import _lib
    rec = (_lib.Mesh * M)()
    wg = 0
    for m in range(M):
        r = rec[m]
        r.origin[:], r.delta, r.sample_offset, r.dims[:] = [0.0, 0.0, 0.0], 0.01, 0.5, [4, 5, 6 + m]
        r.out_offset, r.first_workgroup = 1000 * m, wg
        wg += 1
        r.vert_begin, r.vert_count, r.face_begin, r.face_count = 10 * m, 10, 20 * m, 20
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
    assert _lib.SURFACE_NODES_PER_WORKGROUP == 256 == SC.BLOCK and lib.omgx_abi_version() == 14 and C.sizeof(_lib.Mesh) == 88
    INV, UNS, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED, _lib.OMGX_OK
    vpc = lambda x: C.cast(x, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    d = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first

    def nbytes(rec, M=None):
        return lib.omgx_surface_workspace_bytes(vpc(rec), len(rec) if M is None else M)

    # 16 bytes of totals and 256 one-byte ranks per workgroup of 256 samples
    assert nbytes(_volumes()) == 2 * (16 + 256)
    assert nbytes(_volumes(1, dims=[1, 1, 1])) == 272 and nbytes(_volumes(1, dims=[4, 8, 8])) == 272 and nbytes(_volumes(1, dims=[4, 8, 9])) == 2 * 272
    big = _volumes(2, dims=[64, 64, 64])
    assert nbytes(big) == (1 + 1024) * 272
    assert nbytes(_volumes(), M=0) == INV and lib.omgx_surface_workspace_bytes(None, 1) == INV and nbytes(_volumes(dims=[0, 4, 4])) == INV
    assert nbytes(_volumes(first_workgroup=2)) == INV and nbytes(_volumes(1, dims=[2048, 1024, 1024])) == UNS

    def count(rec=None, M=None, level=0.0, pool_elems=1 << 20, host=True, **ptr):
        rec = rec or _volumes()
        p = dict(pool=d, meshes=d, ws=d, counts=d)
        p.update(ptr)
        return lib.omgx_surface_count(p["pool"], pool_elems, p["meshes"], vpc(rec) if host else None, len(rec) if M is None else M, level, p["ws"],
                                      p["counts"], None)

    def gather(rec=None, M=None, level=0.0, pool_elems=1 << 20, host=True, vert_cap=100, face_cap=100, **ptr):
        rec = rec or _volumes()
        p = dict(pool=d, meshes=d, ws=d, verts=d, faces=d)
        p.update(ptr)
        return lib.omgx_surface_gather(p["pool"], pool_elems, p["meshes"], vpc(rec) if host else None, len(rec) if M is None else M, level, p["ws"],
                                       p["verts"], vert_cap, p["faces"], face_cap, None)

    for k in ("pool", "meshes", "ws", "counts"):
        assert count(**{k: None}) == INV, k
    for k in ("pool", "meshes", "ws", "verts", "faces"):
        assert gather(**{k: None}) == INV, k
    for fn in (count, gather):
        assert fn(host=False) == INV and fn(M=0) == INV and fn(M=-1) == INV and fn(level=nan) == INV and fn(pool_elems=-1) == INV, fn
        for dims in ([0, 4, 4], [4, -1, 4], [4, 4, 0]):
            assert fn(rec=_volumes(dims=dims)) == INV, dims
        for delta in (0.0, -0.01, nan, inf):
            assert fn(rec=_volumes(delta=delta)) == INV, delta
        for off in (0.25, 1.0, -0.5, nan):
            assert fn(rec=_volumes(sample_offset=off)) == INV, off
        for origin in ([nan, 0, 0], [0, inf, 0], [0, 0, -inf]):
            assert fn(rec=_volumes(origin=origin)) == INV, origin
        assert fn(rec=_volumes(out_offset=-1)) == INV
        assert fn(rec=_volumes(out_offset=(1 << 20) - 4 * 5 * 7 + 1)) == INV and fn(rec=_volumes(), pool_elems=1000 + 4 * 5 * 7 - 1) == INV
        assert fn(rec=_volumes(1, dims=[4, 4, 4]), pool_elems=63) == INV
        for wg in (0, 2, -1):
            assert fn(rec=_volumes(first_workgroup=wg)) == INV, wg
        # limits: an invalid record of any volume is reported first
        assert fn(rec=_volumes(1, dims=[2048, 1024, 1024]), pool_elems=1 << 40) == UNS  # 2^31 samples
        huge = _volumes(3, dims=[2048, 1024, 1024])
        huge[0].dims[:], huge[1].dims[:] = [2047, 1024, 1024], [1, 1, 1]
        huge[1].first_workgroup, huge[2].first_workgroup = 2047 * 4096, 2047 * 4096 + 1
        assert fn(rec=huge, pool_elems=1 << 40) == UNS
        huge[1].delta = 0.0
        assert fn(rec=huge, pool_elems=1 << 40) == INV
        # 257 volumes of 2047 * 2^20 samples, read from one place: 257 * 8 384 512 workgroups are more than 2^31 - 1 (256 are not)
        many = _volumes(257, dims=[2047, 1024, 1024])
        for m in range(257):
            many[m].dims[:], many[m].out_offset, many[m].first_workgroup = [2047, 1024, 1024], 0, m * 2047 * 4096
            many[m].vert_begin = many[m].vert_count = many[m].face_begin = many[m].face_count = 0
        assert fn(rec=many, pool_elems=1 << 40) == UNS
    for k in ("vert_begin", "vert_count", "face_begin", "face_count"):
        assert gather(rec=_volumes(**{k: -1})) == INV, k
    assert gather(vert_cap=-1) == INV and gather(face_cap=-1) == INV
    assert gather(rec=_volumes(vert_begin=9)) == INV and gather(rec=_volumes(face_begin=19)) == INV      # ranges of two meshes overlap
    # nothing to write: no launch
    assert gather(vert_cap=0, face_cap=0, verts=None, faces=None) == OK


def test_wrapper_checks_without_gpu():
    import torch
    from omg_planner_amd import _lib, ops
    E = _lib.OmgHipError
    rec = ops.surface_records([((0.0, 0.0, 0.0), 0.01, "centre", (4, 8, 9), 0), ((0.0, 0.0, 0.0), 0.02, "node", (2, 2, 2), 288)])
    assert [r.first_workgroup for r in rec] == [0, 2] and rec[1].sample_offset == 0.0 and rec[1].out_offset == 288 and list(rec[0].dims) == [4, 8, 9]
    again = ops.surface_records(rec)
    assert bytes(again) == bytes(rec) and again is not rec
    for bad in ([], [((0.0, 0.0), 0.01, "centre", (4, 4, 4), 0)], [((0.0, 0.0, 0.0), 0.0, "centre", (4, 4, 4), 0)],
                [((0.0, 0.0, 0.0), 0.01, "corner", (4, 4, 4), 0)], [((0.0, 0.0, 0.0), 0.01, "centre", (4, 0, 4), 0)],
                [((0.0, 0.0, 0.0), 0.01, "centre", (4, 4, 4), -1)], [((0.0, np.nan, 0.0), 0.01, "centre", (4, 4, 4), 0)]):
        with pytest.raises(E):
            ops.surface_records(bad)
    pool = torch.zeros(64, dtype=torch.float32)
    with pytest.raises(E, match="device tensor"):
        ops.surface_meshes(pool, [((0.0, 0.0, 0.0), 0.01, "centre", (4, 4, 4), 0)])
    with pytest.raises(E, match="tensor"):
        ops.surface_mesh(np.zeros((4, 4, 4), np.float32), (0.0, 0.0, 0.0), 0.01)
    with pytest.raises(E, match="device tensor"):
        ops.surface_mesh(torch.zeros((4, 4, 4)), (0.0, 0.0, 0.0), 0.01)


# ---------------------------------------------------------------------------------------------------------------------
# registers
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_surface_kernels_do_not_spill(tmp_path):
    """The compiler's resource remarks for csrc/omg_surface.hip: no kernel uses scratch (the eight corners and the twelve edges
    of a cell stay in registers)."""
    seen = KB.kernel_resources("omg_surface.hip", tmp_path)
    kernels = {k: KB.one(seen, k) for k in ("k_surface_count", "k_surface_scan", "k_surface_gather")}
    for k, v in kernels.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs"] <= 128, (k, v)
