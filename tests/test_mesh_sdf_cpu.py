"""Signed distance grids from triangle meshes, the parts that need no GPU: the host specification scenes.mesh_sdf
(closest point by the seven regions of a triangle, sign from the generalised winding number) against definitions that do not
share its code, the grid layout, the OBJ / text .sdf files, the argument checks of omgx_mesh_sdf (ABI 14) and of the wrappers,
and the compiled kernel's registers.  The device side is tests/test_gpu_mesh_sdf.py."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import kernel_build as KB
from tests import mesh_cases as MC


# ---------------------------------------------------------------------------------------------------------------------
# host specification against the exact box distance
# ---------------------------------------------------------------------------------------------------------------------
BOX_CASES = [  # half extents, pose, delta, padding
    (MC.BOX_HALF, MC.pose(), 0.01, 3),
    (MC.BOX_HALF, MC.pose(), 0.0125, 1),
    ((0.02, 0.02, 0.11), MC.pose((0.3, -0.5, 0.2)), 0.013, 2),
    ((0.10, 0.035, 0.06), MC.pose((0.0, 0.0, 0.9), (0.3, -0.2, 0.5)), 0.017, 4),
    (MC.BOX_HALF, MC.pose((0.0, 0.0, 0.0), (1.5, 0.0, 0.0)), 0.01, 3),
    (MC.BOX_HALF, MC.pose((1.1, 0.4, -0.7), (-0.4, 1.5, 0.25)), 0.009, 2),
]


@pytest.mark.parametrize("sample", ["centre", "node"])
@pytest.mark.parametrize("case", range(len(BOX_CASES)))
def test_host_spec_is_the_exact_box_distance(case, sample):
    """|scenes.mesh_sdf's float64 value - the formula of scenes.box_sdf in the box's frame| <= 1e-12 m on every node: coordinates
    below 2 m in float64 (ulp 2.2e-16) through a few dozen operations."""
    from omg_planner_amd import scenes as sc
    half, P, delta, padding = BOX_CASES[case]
    v, f = MC.box_mesh(half, P)
    origin, dims = sc.mesh_grid_layout(v, delta, padding)
    p = sc.mesh_nodes(origin, dims, delta, sample)
    assert np.abs(p).max() < 2.0
    d, w = sc.mesh_distance_winding(v, f, p)
    got = np.where(np.abs(w) > 0.5, -d, d)
    want = MC.box_distance(half, P, p)
    off = np.abs(want) > 1e-9  # a node ON the surface has distance 0 and no sign
    assert off.sum() > 0.5 * len(p) and (want < 0).sum() > 10
    err = np.abs(np.where(off, got, np.abs(got)) - np.where(off, want, np.abs(want))).max()
    print(f"case {case} {sample}: grid {tuple(int(x) for x in dims)}, max |diff| = {err:.3e}")
    assert err <= 1e-12
    # and the grid mesh_sdf returns is that value rounded once
    g = sc.mesh_sdf(v, f, delta, padding, sample)
    assert g.data.dtype == np.float32 and g.data.shape == tuple(dims) and g.delta == delta
    np.testing.assert_array_equal(g.origin, origin)
    np.testing.assert_array_equal(g.data.ravel(), got.astype(np.float32))


@pytest.mark.parametrize("half,shape,delta", [((0.05, 0.08, 0.03), (17, 24, 13), 0.011), ((0.031, 0.017, 0.052), (12, 10, 16), 0.013)])
def test_aligned_grid_equals_box_sdf_as_float32(half, shape, delta):
    """With box_sdf's own origin and dims the mesh grid IS box_sdf's grid, float32 for float32."""
    from omg_planner_amd import scenes as sc
    want = sc.box_sdf(half, shape, delta)
    x, y, z = sc._voxel_centres(shape, want.origin, delta)
    q = np.stack([np.abs(x) - half[0], np.abs(y) - half[1], np.abs(z) - half[2]], -1)
    assert np.abs(q).min() > 1e-6 and (want.data < 0).any() and (want.data > 0).any()  # no node on the surface (nor on a face's plane)
    v, f = MC.box_mesh(half)
    got = sc.mesh_sdf(v, f, delta, sample="centre", origin=want.origin, dims=shape)
    np.testing.assert_array_equal(got.data, want.data)
    np.testing.assert_array_equal(got.origin, want.origin)


# ---------------------------------------------------------------------------------------------------------------------
# closest point against an independent, exact definition
# ---------------------------------------------------------------------------------------------------------------------
def _exact_distance2(p, a, b, c):
    """|p - triangle|^2 in exact rational arithmetic: the projection onto the plane if it falls inside the triangle, otherwise the
    minimum over the three segments."""
    F = lambda x: [Fraction(float(t)) for t in x]
    p, a, b, c = F(p), F(a), F(b), F(c)
    sub = lambda u, v: [u[k] - v[k] for k in range(3)]
    dot = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    n = cross(sub(b, a), sub(c, a))
    nn = dot(n, n)
    s = dot(n, sub(p, a)) / nn
    proj = [p[k] - s * n[k] for k in range(3)]
    if all(dot(cross(sub(v, u), sub(proj, u)), n) >= 0 for u, v in ((a, b), (b, c), (c, a))):
        return s * s * nn
    best = None
    for u, v in ((a, b), (b, c), (c, a)):
        e = sub(v, u)
        t = min(max(dot(sub(p, u), e) / dot(e, e), Fraction(0)), Fraction(1))
        r = sub(p, [u[k] + t * e[k] for k in range(3)])
        best = dot(r, r) if best is None else min(best, dot(r, r))
    return best


def _triangles():
    """(kind, a, b, c) in the plane z = 0: acute, obtuse, needle-thin (aspect 1e4: two 0.1 m edges 1e-5 m apart at the far end)."""
    return [("acute", (0.0, 0.0), (0.11, 0.01), (0.05, 0.09)), ("acute", (0.02, -0.03), (0.12, 0.0), (0.06, 0.1)),
            ("obtuse", (0.0, 0.0), (0.2, 0.0), (0.1, 0.02)), ("obtuse", (0.0, 0.0), (0.05, 0.01), (-0.08, 0.07)),
            ("needle", (0.0, 0.0), (0.1, 0.0), (0.1, 1e-5)), ("needle", (0.0, 0.0), (0.1, 0.0), (0.05, 1e-5))]


def _points_by_region(a, b, c, rng, per_region=12):
    """Points built to lie in each of the seven regions (in the triangle's plane z = 0, lifted by O(0.1) along z afterwards):
    the interior by barycentric weights, an edge region from a point of the edge pushed along the edge's outward normal, a vertex
    region from the vertex pushed along a positive combination of its two edges' outward normals."""
    a, b, c = (np.array(x, np.float64) for x in (a, b, c))
    cen = (a + b + c) / 3

    def outward(u, v):
        e = v - u
        n = np.array([e[1], -e[0]]) / np.linalg.norm(e)
        return n if n @ (u - cen) > 0 else -n
    nab, nac, nbc = outward(a, b), outward(a, c), outward(b, c)
    pts, want = [], []
    for _ in range(per_region):
        s, t = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9)
        if s + t > 1:
            s, t = 1 - s, 1 - t
        r1, r2 = rng.uniform(0.2, 1.0, 2) * 0.05
        for region, xy in ((6, a + s * (b - a) + t * (c - a) * 0.98), (2, a + s * (b - a) + r1 * nab), (4, a + s * (c - a) + r1 * nac),
                           (5, b + s * (c - b) + r1 * nbc), (0, a + r1 * nab + r2 * nac), (1, b + r1 * nab + r2 * nbc),
                           (3, c + r1 * nac + r2 * nbc)):
            pts.append([xy[0], xy[1], rng.choice([-1, 1]) * rng.uniform(0.05, 0.15)])
            want.append(region)
    return np.array(pts), np.array(want)


@pytest.mark.parametrize("tri", range(6))
def test_closest_point_against_exact_definition(tri):
    from omg_planner_amd import scenes as sc
    kind, a2, b2, c2 = _triangles()[tri]
    rng = np.random.RandomState(100 + tri)
    p, want_region = _points_by_region(a2, b2, c2, rng)
    P = MC.pose(rng.uniform(-1, 1, 3), rng.uniform(-0.5, 0.5, 3))  # the triangle and the points anywhere in space
    mv = lambda x: np.asarray(x, np.float64) @ P[:3, :3].T + P[:3, 3]
    a, b, c = (mv([x[0], x[1], 0.0]) for x in (a2, b2, c2))
    p = mv(p)
    q, region = sc.closest_point_on_triangle(p, a, b, c)
    assert set(region.tolist()) == set(range(7)), f"{kind}: regions {sorted(set(region.tolist()))}"
    np.testing.assert_array_equal(region, want_region)
    d = np.sqrt(((p - q) ** 2).sum(-1))
    exact = np.array([float(_exact_distance2(p[i], a, b, c)) ** 0.5 for i in range(len(p))])
    assert 0.04 < exact.min() and exact.max() < 0.3
    rel = np.abs(d - exact) / exact
    print(f"{kind}: max relative error {rel.max():.3e} over {len(p)} points")
    assert rel.max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# sign
# ---------------------------------------------------------------------------------------------------------------------
def _closed_meshes():
    two = [MC.box_mesh((0.03, 0.02, 0.04), MC.pose((0, 0, 0.4), (-0.06, 0.0, 0.0))), MC.box_mesh((0.02, 0.05, 0.02), MC.pose((0.5, 0, 0), (0.07, 0.01, 0.0)))]
    return {
        "box": [MC.box_mesh(MC.BOX_HALF, MC.pose((0.2, 0.1, -0.3), (0.01, 0.0, 0.02)))],
        "flipped_box": [MC.box_mesh(MC.BOX_HALF, MC.pose((0.2, 0.1, -0.3), (0.01, 0.0, 0.02)), flip=True)],
        "ico80": [MC.icosphere(1, 0.06, (0.003, -0.002, 0.001))],
        "ico320": [MC.icosphere(2, 0.06, (0.003, -0.002, 0.001))],
        "two_boxes": two,
    }


@pytest.mark.parametrize("name", ["box", "flipped_box", "ico80", "ico320", "two_boxes"])
def test_sign_of_closed_meshes(name):
    """A closed mesh's winding number is 0 or +-1 up to rounding: every node is at least 0.4 from the threshold, and inside is
    the analytic inside (of the convex parts)."""
    from omg_planner_amd import scenes as sc
    parts = _closed_meshes()[name]
    v = np.concatenate([pv for pv, _ in parts])
    f = np.concatenate([pf + sum(len(q[0]) for q in parts[:i]) for i, (_, pf) in enumerate(parts)])
    delta = 0.012
    origin, dims = sc.mesh_grid_layout(v, delta, 2)
    p = sc.mesh_nodes(origin, dims, delta, "centre")
    d, w = sc.mesh_distance_winding(v, f, p)
    margin = np.abs(np.abs(w) - 0.5).min()
    print(f"{name}: grid {tuple(int(x) for x in dims)}, min | |w| - 0.5 | = {margin:.15f}")
    assert margin > 0.4
    inside = np.zeros(len(p), bool)
    for pv, pf in parts:
        ins, on = MC.inside_convex(pv, pf, p)
        assert not on.any()
        inside |= ins
    assert 10 < inside.sum() < len(p) - 10
    np.testing.assert_array_equal(np.abs(w) > 0.5, inside)
    if name == "flipped_box":
        # the same triangles with their corners in the other order: the same distances up to the last bits (a, b, c change
        # roles), the opposite winding number, the same volume
        d0, w0 = sc.mesh_distance_winding(v, f[:, ::-1].copy(), p)
        assert np.abs(d - d0).max() <= 1e-15
        np.testing.assert_allclose(w, -w0, rtol=0, atol=1e-12)
        g, g0 = sc.mesh_sdf(v, f, delta, 2), sc.mesh_sdf(v, f[:, ::-1].copy(), delta, 2)
        np.testing.assert_array_equal(g.data < 0, g0.data < 0)
        np.testing.assert_array_equal(g.data.ravel() < 0, inside)
        np.testing.assert_allclose(g.data, g0.data, rtol=0, atol=1e-8)


def test_sign_of_an_open_mesh():
    """A box without its last two triangles: w varies continuously through the hole, so some nodes come near the threshold —
    fewer than 0.5 % of them within 1e-3 (the band the device comparison leaves out)."""
    from omg_planner_amd import scenes as sc
    v, f = MC.box_mesh(MC.BOX_HALF)
    delta = 0.01
    origin, dims = sc.mesh_grid_layout(v, delta, 3)
    p = sc.mesh_nodes(origin, dims, delta, "centre")
    _, w = sc.mesh_distance_winding(v, f[:-2], p)
    gap = np.abs(np.abs(w) - 0.5)
    print(f"open box: grid {tuple(int(x) for x in dims)}, min | |w| - 0.5 | = {gap.min():.3e}, {int((gap <= 1e-3).sum())} of {len(p)} nodes within 1e-3")
    assert gap.min() < 0.4  # it IS open
    assert (gap <= 1e-3).sum() < 0.005 * len(p)


# ---------------------------------------------------------------------------------------------------------------------
# layout and files
# ---------------------------------------------------------------------------------------------------------------------
def test_mesh_grid_layout():
    from omg_planner_amd import scenes as sc
    v = np.array([[0.0, -0.1, 0.25], [0.1, 0.06, 0.31], [0.05, 0.0, 0.3]])
    origin, dims = sc.mesh_grid_layout(v, 0.02, 3)
    np.testing.assert_array_equal(origin, v.min(0) - 3 * 0.02)
    assert list(dims) == [int(np.ceil((0.1 - 0.0) / 0.02)) + 6, int(np.ceil((0.06 + 0.1) / 0.02)) + 6, int(np.ceil((0.31 - 0.25) / 0.02)) + 6]
    origin0, dims0 = sc.mesh_grid_layout(v, 0.03, 0)
    np.testing.assert_array_equal(origin0, v.min(0))
    assert list(dims0) == [4, 6, 2]
    # both conventions cover the mesh: the samples of "centre" straddle it, those of "node" start on lo
    pc, pn = sc.mesh_nodes(origin0, dims0, 0.03, "centre"), sc.mesh_nodes(origin0, dims0, 0.03, "node")
    np.testing.assert_array_equal(pn[0], v.min(0))
    np.testing.assert_allclose(pc[0], v.min(0) + 0.015, atol=1e-15)
    assert pn.shape == (48, 3) and np.array_equal(pn[1] - pn[0], [0, 0, (0.25 + 0.03) - 0.25])  # z runs fastest (x-major)


def test_sdf_text_round_trip(tmp_path):
    from omg_planner_amd import scene_io as io, scenes as sc
    rng = np.random.RandomState(3)
    g = sc.SdfGrid(rng.uniform(-0.1, 0.4, (3, 5, 2)).astype(np.float32), np.array([0.1, -0.2, 1.0 / 3.0]), 0.6 / 64)
    io.write_sdf_text(str(tmp_path / "a.sdf"), g)
    back = io.read_sdf_text(str(tmp_path / "a.sdf"))
    assert back.data.dtype == np.float32 and back.delta == g.delta
    np.testing.assert_array_equal(back.data, g.data)
    np.testing.assert_array_equal(back.origin, g.origin)
    lines = (tmp_path / "a.sdf").read_text().split("\n")
    assert lines[0] == "3 5 2" and float(lines[3]) == float(g.data[0, 0, 0]) and float(lines[4]) == float(g.data[1, 0, 0])  # x fastest
    (tmp_path / "short.sdf").write_text("2 2 2\n0 0 0\n0.1\n1\n2\n3\n")
    with pytest.raises(ValueError):
        io.read_sdf_text(str(tmp_path / "short.sdf"))


def test_read_sdf_text_reproduces_the_reference_reader(golden_dir):
    """sdf_text_ramp.npz is what SignedDensityField.from_sdf made of sdf_text_ramp.sdf (tests/golden/make_mesh_golden.py)."""
    from omg_planner_amd import scene_io as io
    rec = np.load(golden_dir / "sdf_text_ramp.npz")
    g = io.read_sdf_text(str(golden_dir / "sdf_text_ramp.sdf"))
    assert rec["data"].shape == (2, 3, 4) and len(np.unique(rec["data"])) == 24
    np.testing.assert_array_equal(g.data.astype(np.float64), rec["data"])
    np.testing.assert_array_equal(g.origin, rec["origin"])
    assert g.delta == float(rec["delta"])


def test_load_obj_box_with_quads_and_mixed_index_forms(golden_dir, tmp_path):
    from omg_planner_amd import scene_io as io, scenes as sc
    v, f = io.load_obj(str(golden_dir / "mesh_box_quads.obj"))
    assert v.shape == (8, 3) and v.dtype == np.float64 and f.shape == (12, 3) and f.dtype == np.int32
    wv, wf = MC.box_mesh(MC.BOX_HALF)
    np.testing.assert_array_equal(v, wv)
    np.testing.assert_array_equal(f, wf)  # fan triangulation of the same quads, the negative-index face included
    np.testing.assert_array_equal(sc.mesh_sdf(v, f, 0.02, 2).data, sc.mesh_sdf(wv, wf, 0.02, 2).data)
    (tmp_path / "bad.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError):
        io.load_obj(str(tmp_path / "bad.obj"))
    (tmp_path / "zero.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n")
    with pytest.raises(ValueError):
        io.load_obj(str(tmp_path / "zero.obj"))


# ---------------------------------------------------------------------------------------------------------------------
# arguments, without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def _records(M=2, **change):
    from omg_planner_amd import _lib
    rec = (_lib.Mesh * M)()
    wg = 0
    for m in range(M):
        r = rec[m]
        r.origin[:], r.delta, r.sample_offset, r.dims[:] = [0.0, 0.1, 0.2], 0.01, 0.5, [5, 6, 7 + m]
        r.vert_begin, r.vert_count, r.face_begin, r.face_count, r.out_offset, r.first_workgroup = 8 * m, 8, 12 * m, 12, 1000 * m, wg
        wg += -(-5 * 6 * (7 + m) // 256)
    for k, val in change.items():
        if k in ("origin", "dims"):
            getattr(rec[M - 1], k)[:] = val
        else:
            setattr(rec[M - 1], k, val)
    return rec


def test_c_abi_argument_checks_without_gpu():
    """Every OMGX_ERR_INVALID / OMGX_ERR_UNSUPPORTED case of omgx_mesh_sdf is decided on the host copy before any HIP call."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    assert lib.omgx_abi_version() == 14 == _lib.ABI_VERSION
    assert lib.omgx_mesh_sdf_tile() >= 64
    assert C.sizeof(_lib.Mesh) == 88 and _lib.Mesh.dims.offset == 56 and _lib.Mesh.first_workgroup.offset == 48
    d = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    INV, UNS = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED

    def call(rec=None, M=2, verts=d, faces=d, meshes=d, out=d, host=True):
        rec = _records(max(M, 1)) if rec is None else rec
        return lib.omgx_mesh_sdf(verts, faces, meshes, C.cast(rec, C.c_void_p) if host else None, M, out, None)
    assert call(verts=None) == INV and call(faces=None) == INV and call(meshes=None) == INV and call(out=None) == INV and call(host=False) == INV
    assert call(M=0) == INV and call(M=-1) == INV
    assert call(_records(face_count=0)) == INV and call(_records(vert_count=0)) == INV
    assert call(_records(vert_begin=-1)) == INV and call(_records(face_begin=-1)) == INV and call(_records(out_offset=-1)) == INV
    for bad in (0.0, -0.01, float("inf"), float("nan")):
        assert call(_records(delta=bad)) == INV, bad
    for bad in ([0, 6, 7], [5, -1, 7], [5, 6, 0]):
        assert call(_records(dims=bad)) == INV, bad
    for bad in (0.25, 1.0, -0.5, float("nan")):
        assert call(_records(sample_offset=bad)) == INV, bad
    assert call(_records(origin=[0.0, float("nan"), 0.0])) == INV
    assert call(_records(first_workgroup=0)) == INV and call(_records(first_workgroup=2)) == INV  # mesh 1 starts at workgroup 1
    assert call(_records(dims=[2048, 2048, 513])) == UNS            # more than 2^31 nodes in one mesh
    assert call(_records(dims=[2048, 2048, 513], delta=0.0)) == INV  # an invalid argument is reported first
    big = _records(1, dims=[2048, 2048, 513])
    assert call(big, M=1) == UNS
    mixed = _records(delta=0.0)                                      # mesh 0 too big, mesh 1 invalid: INVALID in any mesh comes first
    mixed[0].dims[:] = [2048, 2048, 513]
    mixed[1].first_workgroup = -(-2048 * 2048 * 513 // 256)
    assert call(mixed) == INV
    mixed[1].delta = 0.01                                            # (the delta alone made it invalid)
    assert call(mixed) == UNS


def test_wrapper_checks_without_gpu():
    from omg_planner_amd import _lib, ops, scenes as sc
    v, f = MC.box_mesh(MC.BOX_HALF)
    bad = f.copy()
    bad[3, 1] = 8
    with pytest.raises(_lib.OmgHipError, match="indices"):
        ops.mesh_sdf(v, bad, 0.01)
    bad[3, 1] = -1
    with pytest.raises(_lib.OmgHipError, match="indices"):
        ops.mesh_sdf_batch([(v, f), (v, bad)], 0.01)
    with pytest.raises(_lib.OmgHipError):
        ops.mesh_sdf(v, f, 0.0)
    with pytest.raises(_lib.OmgHipError):
        ops.mesh_sdf(v, f, 0.01, sample="corner")
    with pytest.raises(_lib.OmgHipError):
        ops.mesh_sdf(v, f, 0.01, origin=np.zeros(3))  # origin without dims
    with pytest.raises(_lib.OmgHipError, match="zero area"):
        ops.mesh_sdf(v, np.array([[0, 0, 1], [2, 2, 2]]), 0.01)
    # faces of zero area are dropped, and counted: a repeated vertex, three collinear vertices
    vv = np.concatenate([v, [[0.0, 0.0, 0.0], [0.01, 0.01, 0.01], [0.02, 0.02, 0.02]]])
    ff = np.concatenate([f, [[0, 0, 1], [8, 9, 10], [3, 5, 3]]]).astype(np.int64)
    cv, cf, dropped = sc.clean_mesh(vv, ff)
    assert dropped == 3 and cf.dtype == np.int32 and cv.dtype == np.float64
    np.testing.assert_array_equal(cf, f)
    np.testing.assert_array_equal(sc.mesh_sdf(vv, ff, 0.02, 2, origin=[-0.1, -0.1, -0.1], dims=(10, 10, 10)).data,
                                  sc.mesh_sdf(v, f, 0.02, 2, origin=[-0.1, -0.1, -0.1], dims=(10, 10, 10)).data)
    with pytest.raises(ValueError):
        sc.clean_mesh(v, f.astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# the compiled kernel
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include "omg_mesh_sdf_body.h"
#include <cstdint>
extern "C" void host_mesh(const double* verts, const int32_t* faces, int nf, const double* p, int n, double* d_out, double* w_out) {
    for (int i = 0; i < n; ++i) {
        double best = 1.0e300, wsum = 0.0;
        for (int q = 0; q < nf; ++q) {
            double T[9];
            for (int c = 0; c < 3; ++c)
                for (int a = 0; a < 3; ++a) T[c * 3 + a] = verts[faces[q * 3 + c] * 3 + a];
            mesh_sdf_pair(p[i * 3], p[i * 3 + 1], p[i * 3 + 2], T, best, wsum);
        }
        d_out[i] = sqrt(best);
        w_out[i] = wsum * 0.15915494309189535;
    }
}
"""


@KB.requires_host_cxx
def test_kernel_pair_body_compiled_for_the_host_equals_the_specification(tmp_path):
    """csrc/omg_mesh_sdf_body.h is what k_mesh_sdf does per (node, face) pair; compiled for the host without contraction it gives
    the specification's float64 distance bit for bit, and the same inside decision, on closed and open meshes."""
    from omg_planner_amd import scenes as sc
    lib = KB.host_harness(_HOST_HARNESS, tmp_path)
    lib.host_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    ico = MC.icosphere(2, 0.06, (0.003, -0.002, 0.001))
    for v, f, delta, sample in ((*MC.box_mesh(MC.BOX_HALF, MC.pose((1.1, 0.4, -0.7), (-0.4, 1.5, 0.25))), 0.011, "node"),
                                (*ico, 0.0123, "centre"), (ico[0], ico[1][:123], 0.02, "node")):
        v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int32)
        origin, dims = sc.mesh_grid_layout(v, delta, 2)
        p = np.ascontiguousarray(sc.mesh_nodes(origin, dims, delta, sample))
        d, w = sc.mesh_distance_winding(v, f, p)
        hd, hw = np.zeros(len(p)), np.zeros(len(p))
        lib.host_mesh(v.ctypes.data, f.ctypes.data, len(f), p.ctypes.data, len(p), hd.ctypes.data, hw.ctypes.data)
        np.testing.assert_array_equal(hd.view(np.uint64), d.view(np.uint64))
        decided = np.abs(np.abs(w) - 0.5) > 1e-3
        assert decided.mean() > 0.995
        np.testing.assert_array_equal((np.abs(hw) > 0.5)[decided], (np.abs(w) > 0.5)[decided])
        assert np.abs(hw - w).max() < 1e-12


@KB.requires_hipcc
def test_mesh_sdf_kernel_does_not_spill(tmp_path):
    """k_mesh_sdf keeps a node's whole state and a face's nine coordinates in registers: no scratch (128
    VGPRs, four waves per SIMD)."""
    v = KB.one(KB.kernel_resources("omg_mesh_sdf.hip", tmp_path), "k_mesh_sdf")
    assert v["ScratchSize [bytes/lane]"] == 0
    assert v["VGPRs"] <= 128
    assert v["Occupancy [waves/SIMD]"] >= 4
