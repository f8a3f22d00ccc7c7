"""Support-plane fitting without a GPU (omg-planner_amd/planes.py, csrc/omg_plane_body.h, include/omg_hip.h section 19): the
specification against analytic planes, every void branch, winding, ties, prior and skip, the observed scene of
tests/segment_cases.py with and without depth noise, the body header compiled for the host and walked in the kernels' order
against the specification bit for bit, every argument error of the entry points, and the kernels' resources."""
from __future__ import annotations

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import kernel_build as KB
from tests import plane_cases as PC
from tests import segment_cases as SC

INF, NAN = PC.INF, PC.NAN


def _fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_plane", Path(__file__).resolve().parent / "fuzz" / "fuzz_plane.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_constants_are_the_headers():
    from omg_planner_amd import _lib, planes, registration
    assert _lib.PLANE_PIXELS_PER_WORKGROUP == planes.PIXELS_PER_WORKGROUP == PC.CHUNK and _lib.PLANE_STAGE_HYPOTHESES == PC.STAGE
    assert registration.THREADS == 256 and PC.CHUNK % 256 == 0 and _lib.PLANE_NODES_PER_WORKGROUP == 256
    assert _lib.lib().omgx_abi_version() == 14 and len(_lib.STRUCTS) == 8


# ---------------------------------------------------------------------------------------------------------------------
# the specification against known answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tilted", "small"])
def test_every_live_hypothesis_of_an_analytic_plane_is_the_plane(name):
    """Depth images by ray-plane intersection in float64: every live hypothesis lies within 1e-12 of the truth in normal and
    offset, and with a tolerance far above the rounding its count is the number of valid pixels."""
    from omg_planner_amd import planes
    c = PC.cases()[name]
    a, kw = PC.arguments(c)
    hyp, live = planes.hypotheses(*a, **kw)
    counts = planes.score(c["intr"], c["depth"], hyp, live, c["tol"])
    _, valid = planes.pixel_points(c["intr"], c["depth"])
    assert live.sum() >= 1 and (name != "tilted" or live.sum() >= 32)
    assert np.abs(hyp[live] - PC.TILTED).max() <= 1e-12
    assert (counts[live] == valid.sum()).all() and (counts[~live] == -1).all() and valid.sum() == c["depth"].size
    fit = planes.fit_planes(*a, c["tol"], **kw)
    assert fit.status.tolist() == [planes.REFINED] and np.abs(fit.planes[0] - PC.TILTED).max() <= 1e-9 and fit.inliers.tolist() == [valid.sum()]
    assert planes.plane_mask(c["intr"], c["depth"], fit.planes, c["tol"]).all()


def _one(depth, triple, intr=PC.INTR, **kw):
    from omg_planner_amd import planes
    hyp, live = planes.hypotheses(np.array([intr]), depth[None], np.array([[triple]], np.int32), **kw)
    return hyp[0, 0], bool(live[0, 0])


def test_every_void_branch():
    from omg_planner_amd import planes
    H, W = 6, 8
    clean = PC.analytic_depth(PC.INTR, H, W, PC.TILTED)
    good = (0, 5, 40)
    plane, live = _one(clean, good)
    assert live and np.abs(plane - PC.TILTED).max() <= 1e-12
    for bad in (INF, NAN, 0.0, -0.7):  # each of the three pixels in turn
        for x in range(3):
            d = clean.copy()
            d.reshape(-1)[good[x]] = bad
            plane, live = _one(d, good)
            assert not live and (plane == 0).all(), (bad, x)
    for x in range(3):
        skip = np.zeros((1, H, W), bool)
        skip.reshape(-1)[good[x]] = True
        plane, live = _one(clean, good, skip=skip)
        assert not live and (plane == 0).all()
    # the same pixel three times, and twice: nn is exactly 0, void even with min_nn = 0
    for t in ((7, 7, 7), (7, 7, 9), (7, 9, 7)):
        assert not _one(clean, t, min_nn=0.0)[1]
    # three collinear points of a FLAT wall along an image row: the cross product is tiny, a positive min_nn voids it
    wall = PC.analytic_depth(PC.INTR, H, W, PC.WALL)
    assert not _one(wall, (0, 3, 6), min_nn=1e-10)[1]
    assert _one(wall, (0, 3, 14), min_nn=1e-10)[1]
    # the prior
    assert _one(clean, good, up=PC.TILTED[:3], cos_min=0.99)[1] and not _one(clean, good, up=-PC.TILTED[:3], cos_min=0.0)[1]
    assert not _one(clean, good, up=PC.WALL[:3], cos_min=0.99)[1]
    # every hypothesis void: best == -1, no plane, mask all False, count 0
    intr, depth = np.array([PC.INTR]), np.full((1, H, W), INF)
    tri = np.array([[good, (1, 2, 3)]], np.int32)
    fit = planes.fit_planes(intr, depth, tri, 0.01)
    assert fit.best.tolist() == [-1] and (fit.counts == -1).all() and fit.status.tolist() == [planes.NO_PLANE] and (fit.planes == 0).all()
    assert fit.inliers.tolist() == [0] and fit.ransac_counts.tolist() == [0]
    assert not planes.plane_mask(intr, clean[None], fit.planes, 0.01).any()
    count, sums = planes.moments(intr, clean[None], fit.planes, fit.anchors, 0.01)
    assert count.tolist() == [0] and (sums == 0).all()
    # arguments
    for change in (dict(tol=-1.0), dict(tol=NAN), dict(min_nn=-1e-3), dict(min_nn=INF), dict(cos_min=1.5), dict(cos_min=NAN)):
        with pytest.raises(ValueError):
            planes.fit_planes(intr, clean[None], tri, **{**dict(tol=0.01), **change})
    for bad_tri in (np.array([[(0, 1, H * W)]]), np.array([[(-1, 1, 2)]]), np.zeros((1, 0, 3), np.int32), np.zeros((2, 1, 3), np.int32)):
        with pytest.raises(ValueError):
            planes.fit_planes(intr, clean[None], bad_tri, 0.01)


def test_winding_and_ties():
    """Swapping b and c negates the cross product exactly and the orientation step undoes it: the same plane bit for bit.
    Duplicate triples have the same count: the smallest k wins."""
    from omg_planner_amd import planes
    rng = np.random.default_rng(5)
    c = PC.cases()["odd"]
    tri = c["triples"]
    swapped = tri[:, :, [0, 2, 1]]
    a, _ = planes.hypotheses(c["intr"], c["depth"], tri, c["min_nn"], c["skip"])
    b, _ = planes.hypotheses(c["intr"], c["depth"], swapped, c["min_nn"], c["skip"])
    assert np.array_equal(PC.bits(a), PC.bits(b)) and (a[..., :3] != 0).any()
    depth = PC.analytic_depth(PC.INTR, 48, 64, PC.TILTED)
    depth = np.where(rng.random(depth.shape) < 0.3, depth * 0.9, depth)[None]
    tri = rng.integers(0, 48 * 64, (1, 40, 3)).astype(np.int32)
    _, counts, best, _, _ = planes.ransac(np.array([PC.INTR]), depth, tri, 1e-9)
    k = int(best[0])
    assert counts[0, k] > 1000
    dup = tri.copy()
    dup[0, [3, 17, 31]] = tri[0, k]
    _, counts, best, _, _ = planes.ransac(np.array([PC.INTR]), depth, dup, 1e-9)
    assert int(best[0]) == min(3, k) and (counts[0, [3, 17, 31]] == counts[0, k]).all()


def test_prior_and_skip_with_a_floor_and_a_larger_wall():
    """Without a prior the wall wins; with up and cos_min the floor wins; with skip = plane_mask of the wall a second fit finds
    the floor."""
    from omg_planner_amd import planes
    depth, floor_px, wall_px = PC.floor_and_wall()
    assert wall_px.sum() > 2 * floor_px.sum() > 1000
    intr, depth = np.array([PC.INTR]), depth[None]
    tri = planes.draw_triples(48, 64, 256, np.random.default_rng(2))
    first = planes.fit_planes(intr, depth, tri, 0.001)
    assert np.abs(first.planes[0] - PC.WALL).max() < 1e-9 and first.inliers[0] >= wall_px.sum()
    with_prior = planes.fit_planes(intr, depth, tri, 0.001, up=PC.FLOOR[:3], cos_min=0.95)
    assert np.abs(with_prior.planes[0] - PC.FLOOR).max() < 1e-9 and with_prior.inliers[0] >= floor_px.sum()
    assert (with_prior.counts >= 0).sum() < (first.counts >= 0).sum()
    wall_mask = planes.plane_mask(intr, depth, first.planes, 0.001)
    assert wall_mask[0][wall_px].all() and not wall_mask[0][floor_px].all()  # (the floor's pixels are in front of the wall)
    second = planes.fit_planes(intr, depth, tri, 0.001, skip=wall_mask)
    assert np.abs(second.planes[0] - PC.FLOOR).max() < 1e-9 and second.inliers[0] == (floor_px & ~wall_mask[0]).sum()
    assert planes.plane_mask(intr, depth, second.planes, 0.001)[0][floor_px].all()


def test_observed_scene_without_noise_gives_the_known_tables_mask_and_segmentation():
    """The sphere and the box on the slab, 256 seeded triples per view: plane_mask equals explained_mask of the slab's own
    rendering pixel for pixel, and segment_views with it equals the segmentation with the known table array for array."""
    from omg_planner_amd import planes, fusion, segmentation as sg
    t, t_known, views = SC.observed_depth()
    intr, tri = PC.observed_intrinsics(), PC.observed_triples()
    fit = planes.fit_planes(intr, t, tri, SC.TOL)
    assert ((fit.counts >= 0).sum(1) >= 16).all(), "the test must not pass on luck"
    assert (fit.status == planes.REFINED).all()
    mask = planes.plane_mask(intr, t, fit.planes, SC.TOL)
    want = sg.explained_mask(t, t_known, SC.TOL)
    assert mask.sum((1, 2)).tolist() == [1720, 1586, 1586]
    assert np.array_equal(mask, want)
    for s in range(3):
        w = PC.plane_in_world(fit.planes[s], s)
        assert abs(w[3] + PC.SLAB_TOP) < 1e-4 and w[2] > 1 - 1e-8
    ref = SC.observed_segmentation()
    got = sg.segment_views(SC.LAYOUT, views, t, SC.BAND, SC.NEAR, fusion.obstacle_radius(SC.REACH, FC.DELTA), SC.SEED_POINT, SC.MIN_NODES, 6, free_mask=mask)
    for key in ("state", "labels", "comp_begin", "records", "record", "cropped"):
        assert np.array_equal(got[key], ref[key]), key
    assert got["rank"] == ref["rank"]
    for key in ("target", "obstacle"):
        assert np.array_equal(FC.bits(got[key].data), FC.bits(ref[key].data)) and np.array_equal(got[key].origin, ref[key].origin)


def noise_errors(seed):
    """Per view of the noisy observed scene: (offset error at the inliers' centroid, offset error at the world's origin, tilt in
    radians, N, rho) of the refined plane against the slab's top z = SLAB_TOP."""
    from omg_planner_amd import planes
    intr = PC.observed_intrinsics()
    depth = PC.noisy_depth(seed)
    fit = planes.fit_planes(intr, depth, PC.observed_triples(seed + 1), SC.TOL)
    p, valid = planes.pixel_points(intr, depth)
    cfw = FC.scene_cameras()[0]
    out = []
    for s in range(3):
        assert fit.status[s] == planes.REFINED
        with np.errstate(invalid="ignore"):
            inl = valid[s] & (np.abs(planes.residual(fit.planes[s], p[s])) <= SC.TOL)
        N = int(inl.sum())
        assert N == fit.inliers[s]
        wfc = np.linalg.inv(cfw[s])
        q = p[s][inl] @ wfc[:3, :3].T + wfc[:3, 3]
        c = q.mean(0)
        rho = float(np.sqrt(((q - c) ** 2).sum(1).mean()))
        w = PC.plane_in_world(fit.planes[s], s)
        at_centroid = abs(float(w[:3] @ np.array([c[0], c[1], PC.SLAB_TOP]) + w[3]))
        out.append((at_centroid, abs(float(w[3]) + PC.SLAB_TOP), float(np.arccos(min(1.0, abs(w[2])))), N, rho))
    return out


NOISE_SEEDS = tuple(range(8))


def test_observed_scene_with_depth_noise_is_refined_to_the_statistical_bound():
    """Gaussian depth noise of sigma = 1 mm on the finite pixels, 8 seeds x 3 views.  A least-squares plane through N points with
    noise sigma normal to it has a height of standard deviation sigma / sqrt(N) at the points' centroid and a slope of
    sigma / (sqrt(N) rho_axis) about each axis; the noise here is along the depth axis, whose component normal to the table is
    smaller than sigma.  The bounds are five of these standard deviations, with N the final inlier count and rho the RMS distance
    of the inliers from their centroid, both computed here: offset error <= 5 sigma / sqrt(N) (at the inliers' centroid, and
    also at the world's origin, where the slab's top is z = 0.01), tilt <= 5 sigma / (sqrt(N) rho).
    Worst seen over these 24 fits: 0.039 mm at the centroid, 0.044 mm at the origin (bounds 0.121 to 0.127 mm), tilt 0.0155 degrees
    (bounds 0.034 to 0.037 degrees)."""
    worst = np.zeros(3)
    for seed in NOISE_SEEDS:
        for s, (at_centroid, at_origin, tilt, N, rho) in enumerate(noise_errors(seed)):
            print(f"seed {seed} view {s}: N {N} rho {rho:.4f} offset {at_centroid:.3e} / {at_origin:.3e} (bound {5 * PC.SIGMA / np.sqrt(N):.3e}) "
                  f"tilt {tilt:.3e} (bound {5 * PC.SIGMA / (np.sqrt(N) * rho):.3e})")
            worst = np.maximum(worst, (at_centroid, at_origin, tilt))
            assert N > 1000
            assert at_centroid <= 5 * PC.SIGMA / np.sqrt(N) and at_origin <= 5 * PC.SIGMA / np.sqrt(N), (seed, s)
            assert tilt <= 5 * PC.SIGMA / (np.sqrt(N) * rho), (seed, s)
    print("worst offset at the centroid, at the origin [m], tilt [deg]:", worst[0], worst[1], np.degrees(worst[2]))


def test_helpers():
    from omg_planner_amd import planes
    rng = np.random.default_rng(0)
    tri = planes.draw_triples(48, 64, 500, rng, window=(10, 20, 30, 34), views=2)
    r, c = np.divmod(tri, 64)
    assert tri.shape == (2, 500, 3) and tri.dtype == np.int32 and r.min() == 10 and r.max() == 19 and c.min() == 30 and c.max() == 33
    with pytest.raises(ValueError):
        planes.draw_triples(48, 64, 5, rng, window=(10, 49, 0, 4))
    # a plane moved to another frame holds the moved points
    T = FC.look_at((0.6, 0.1, 0.5), (0.0, 0.0, 0.05))
    pts = rng.normal(size=(5, 3))
    pts[:, 2] = -(PC.TILTED[0] * pts[:, 0] + PC.TILTED[1] * pts[:, 1] + PC.TILTED[3]) / PC.TILTED[2]
    moved = planes.plane_to_frame(PC.TILTED, T)
    assert np.abs((pts @ T[:3, :3].T + T[:3, 3]) @ moved[:3] + moved[3]).max() < 1e-12 and abs(np.linalg.norm(moved[:3]) - 1) < 1e-12
    # refine_plane keeps its input where the fit means nothing
    plane = np.array([0.0, 0.0, -1.0, 1.0])
    for count, sums in ((2, np.zeros(9)), (5, np.full(9, NAN)), (5, np.array([1.0, 0, 0, 1.0, 0, 0, 0, 0, 0])), (4, np.zeros(9))):
        got, ok = planes.refine_plane(count, sums, np.zeros(3), plane)
        assert not ok and np.array_equal(got, plane)
    # the half-space volume against its formula, both sample kinds
    for v, p in zip(PC.VOLUMES, PC.VOLUME_PLANES):
        got = planes.halfspace_volume(v, p)
        i, j, k = np.meshgrid(*[np.arange(d) for d in v[3]], indexing="ij")
        o = 0.5 if v[2] == "centre" else 0.0
        x, y, z = (v[0][a] + (g + o) * v[1] for a, g in enumerate((i, j, k)))
        assert got.dtype == np.float32 and got.shape == v[3] and np.abs(got - (p[0] * x + p[1] * y + p[2] * z + p[3])).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the body header compiled for the host, walked in the kernels' order
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include <vector>
#include "omg_fusion_body.h"
#include "omg_plane_body.h"
// as pl_pixel of omg_plane.hip
static bool pixel(const double* intr, const double* depth, const uint8_t* skip, int v, int64_t N, int W, int64_t i, double* p) {
    const int64_t ic = i < N ? i : N - 1;
    const int64_t at = (int64_t)v * N + ic;
    const bool valid = plane_point(intr + (int64_t)v * 4, depth[at], skip ? skip[at] != 0 : false, (int)(ic / W), (int)(ic % W), p);
    return valid && i < N;
}
extern "C" void host_ransac(const double* intr, const double* depth, const uint8_t* skip, int V, int H, int W, const int32_t* triples, int K,
                            double tol, double min_nn, const double* up, double cos_min, int chunk_pixels, int stage, double* planes,
                            int32_t* counts, int32_t* best, double* best_planes, double* anchors) {
    const int64_t N = (int64_t)H * W;
    const int chunks = (int)((N + chunk_pixels - 1) / chunk_pixels), per_lane = chunk_pixels / PLANE_LANES;
    for (int64_t row = 0; row < (int64_t)V * K; ++row) {  // k_plane_hypotheses
        const int v = (int)(row / K);
        double p[3][3];
        bool valid = true;
        for (int x = 0; x < 3; ++x) valid = pixel(intr, depth, skip, v, N, W, triples[row * 3 + x], p[x]) && valid;
        counts[row] = plane_from_triple(p[0], p[1], p[2], valid, min_nn, up ? up + (int64_t)v * 3 : nullptr, cos_min, planes + row * 4) ? 0 : -1;
    }
    std::vector<double> px((size_t)chunk_pixels * 3);
    for (int v = 0; v < V; ++v)  // k_plane_score: a workgroup per (view, chunk), blocks of `stage` rows, one addition per workgroup and row
        for (int chunk = 0; chunk < chunks; ++chunk) {
            for (int lane = 0; lane < PLANE_LANES; ++lane)
                for (int j = 0; j < per_lane; ++j) {
                    double p[3];
                    const bool valid = pixel(intr, depth, skip, v, N, W, (int64_t)chunk * chunk_pixels + j * PLANE_LANES + lane, p);
                    for (int a = 0; a < 3; ++a) px[((size_t)lane * per_lane + j) * 3 + a] = valid ? p[a] : NAN;
                }
            for (int k0 = 0; k0 < K; k0 += stage)
                for (int j = 0; j < stage && k0 + j < K; ++j) {
                    const int64_t row = (int64_t)v * K + k0 + j;
                    if (counts[row] < 0) continue;
                    int c = 0;
                    for (int t = 0; t < chunk_pixels; ++t) c += fabs(plane_residual(planes + row * 4, &px[(size_t)t * 3])) <= tol ? 1 : 0;
                    counts[row] += c;
                }
        }
    for (int v = 0; v < V; ++v) {  // k_plane_select
        int count = -1, at = K;
        for (int k = 0; k < K; ++k)
            if (counts[(int64_t)v * K + k] > count) count = counts[(int64_t)v * K + k], at = k;
        const int b = count >= 0 ? at : -1;
        best[v] = b;
        double p[3] = {0.0, 0.0, 0.0};
        if (b >= 0) pixel(intr, depth, skip, v, N, W, triples[((int64_t)v * K + b) * 3], p);
        for (int a = 0; a < 4; ++a) best_planes[v * 4 + a] = b >= 0 ? planes[((int64_t)v * K + b) * 4 + a] : 0.0;
        for (int a = 0; a < 3; ++a) anchors[v * 3 + a] = b >= 0 ? p[a] : 0.0;
    }
}
extern "C" void host_moments(const double* intr, const double* depth, const uint8_t* skip, int V, int H, int W, const double* planes,
                             const double* anchors, double tol, int chunk_pixels, int32_t* count, double* sums) {
    const int64_t N = (int64_t)H * W;
    const int chunks = (int)((N + chunk_pixels - 1) / chunk_pixels), per_lane = chunk_pixels / PLANE_LANES;
    std::vector<double> lanes((size_t)PLANE_LANES * PLANE_SUMS);
    for (int v = 0; v < V; ++v) {
        const double* plane = planes + v * 4;
        const bool exists = plane_exists(plane);
        double total[PLANE_SUMS];
        for (int a = 0; a < PLANE_SUMS; ++a) total[a] = 0.0;
        int64_t n = 0;
        for (int chunk = 0; chunk < chunks; ++chunk) {  // k_plane_moments
            for (int lane = 0; lane < PLANE_LANES; ++lane) {
                double s[PLANE_SUMS];
                for (int a = 0; a < PLANE_SUMS; ++a) s[a] = 0.0;
                for (int j = 0; j < per_lane; ++j) {
                    double p[3], t[PLANE_SUMS];
                    const bool valid = pixel(intr, depth, skip, v, N, W, (int64_t)chunk * chunk_pixels + j * PLANE_LANES + lane, p);
                    const bool in = exists && plane_inlier(plane, p, valid, tol);
                    plane_terms(p, anchors + v * 3, t);
                    for (int a = 0; a < PLANE_SUMS; ++a) s[a] = s[a] + (in ? t[a] : 0.0);
                    n += in ? 1 : 0;
                }
                for (int a = 0; a < PLANE_SUMS; ++a) lanes[(size_t)lane * PLANE_SUMS + a] = s[a];
            }
            for (int a = 0; a < PLANE_SUMS; ++a) total[a] = total[a] + plane_tree(&lanes[a], PLANE_SUMS);  // k_plane_reduce: left to right
        }
        count[v] = (int32_t)n;
        for (int a = 0; a < PLANE_SUMS; ++a) sums[v * PLANE_SUMS + a] = total[a];
    }
}
extern "C" void host_mask(const double* intr, const double* depth, const uint8_t* skip, int V, int H, int W, const double* planes, double tol,
                          uint8_t* mask) {
    const int64_t N = (int64_t)H * W;
    for (int64_t id = 0; id < N * V; ++id) {
        const int v = (int)(id / N);
        double p[3];
        const bool valid = pixel(intr, depth, skip, v, N, W, id - v * N, p);
        mask[id] = plane_explains(planes + v * 4, p, valid, tol) ? 1 : 0;
    }
}
extern "C" void host_volume(const double* origin, double delta, double offset, const int32_t* n, const double* plane, float* out) {
    int64_t id = 0;
    for (int i = 0; i < n[0]; ++i)
        for (int j = 0; j < n[1]; ++j)
            for (int k = 0; k < n[2]; ++k) {
                double p[3];
                fusion_node_point(origin, delta, offset, i, j, k, p);
                out[id++] = plane_halfspace(plane, p);
            }
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if KB.host_compiler() is None:
        pytest.skip("no C++ compiler")
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    return KB.host_harness(_HOST_HARNESS, tmp_path_factory.mktemp("plane_host"),
                           {"host_ransac": (None, [vp, vp, vp, i, i, i, vp, i, d, d, vp, d, i, i, vp, vp, vp, vp, vp]),
                            "host_moments": (None, [vp, vp, vp, i, i, i, vp, vp, d, i, vp, vp]),
                            "host_mask": (None, [vp, vp, vp, i, i, i, vp, d, vp]), "host_volume": (None, [vp, d, d, vp, vp, vp])})


def host_outputs(lib, c, refine=1):
    """Everything fuzz_plane.specification returns, from the body header on the host (the host half of the fit is planes')."""
    from omg_planner_amd import planes, scenes as sc
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    intr, depth = np.ascontiguousarray(c["intr"], np.float64), np.ascontiguousarray(c["depth"], np.float64)
    V, H, W = depth.shape
    skip = None if c["skip"] is None else np.ascontiguousarray(c["skip"], np.uint8)
    up = None if c["up"] is None else np.ascontiguousarray(c["up"], np.float64)
    tri = np.ascontiguousarray(c["triples"], np.int32)
    K = tri.shape[1]
    hyp, counts, best = np.full((V, K, 4), 9.0), np.full((V, K), 77, np.int32), np.full(V, 77, np.int32)
    best_planes, anchors = np.full((V, 4), 9.0), np.full((V, 3), 9.0)
    lib.host_ransac(ptr(intr), ptr(depth), ptr(skip), V, H, W, ptr(tri), K, c["tol"], c["min_nn"], ptr(up), c["cos_min"], PC.CHUNK, PC.STAGE, ptr(hyp),
                    ptr(counts), ptr(best), ptr(best_planes), ptr(anchors))

    def moments_of(pl):
        pl = np.ascontiguousarray(pl, np.float64)
        count, sums = np.full(V, 77, np.int32), np.full((V, 9), 9.0)
        lib.host_moments(ptr(intr), ptr(depth), ptr(skip), V, H, W, ptr(pl), ptr(anchors), c["tol"], PC.CHUNK, ptr(count), ptr(sums))
        return count, sums

    count, sums = moments_of(best_planes)
    final, inliers, status = planes._fit_rounds(best, best_planes, anchors, refine, moments_of)
    mask = np.full((V, H, W), 77, np.uint8)
    lib.host_mask(ptr(intr), ptr(depth), ptr(skip), V, H, W, ptr(np.ascontiguousarray(final)), c["tol"], ptr(mask))
    out = dict(hyp=hyp, counts=counts, best=best, best_planes=best_planes, anchors=anchors, count=count, sums=sums, final=final, inliers=inliers,
               status=status, mask=mask.astype(bool))
    if "volumes" in c:
        pool = np.full(c["pool"], -123.0, np.float32)
        for v, p in zip(c["volumes"], c["volume_planes"]):
            dims, data = np.array(v[3], np.int32), np.zeros(int(np.prod(v[3])), np.float32)
            lib.host_volume(ptr(np.asarray(v[0], np.float64)), float(v[1]), sc.MESH_SAMPLE_OFFSET[v[2]], ptr(dims), ptr(np.ascontiguousarray(p, np.float64)), ptr(data))
            pool[v[4]: v[4] + data.size] = data
        out["pool"] = pool
    return out


def _same(got, want, what):
    for key, w in want.items():
        g = got[key]
        if w.dtype == np.float64:
            assert np.array_equal(PC.bits(g), PC.bits(w)), (what, key)
        elif w.dtype == np.float32:
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, key)
        else:
            assert np.array_equal(g, w), (what, key)


@KB.requires_host_cxx
@pytest.mark.parametrize("name", sorted(PC.cases()))
def test_body_header_on_the_host_equals_the_specification(host, name):
    """planes, counts, best, best planes, anchors, moments, the refined planes, masks and volumes, bit for bit, with the pixels in
    the kernels' chunks and the sums in their shape."""
    fuzz = _fuzz()
    c = dict(PC.cases()[name])
    volumes, size = PC.pool_layout()
    c.update(volumes=volumes, volume_planes=PC.VOLUME_PLANES, pool=size)
    want = fuzz.specification(c)
    _same(host_outputs(host, c), want, name)
    assert (want["counts"] >= 0).any() and (name != "odd" or (want["best"][1] == -1 and want["status"][1] == 0 and not want["mask"][1].any()))


@KB.requires_host_cxx
def test_body_header_on_the_host_equals_the_specification_on_the_fuzz_generators_draws(host):
    fuzz = _fuzz()
    rng = np.random.default_rng(fuzz.SMOKE_SEED)
    live = 0
    for k in range(40):
        c = fuzz.draw(rng)
        want = fuzz.specification(c)
        _same(host_outputs(host, c), want, k)
        live += int((want["counts"] >= 0).sum())
    assert live > 200


@KB.requires_host_cxx
def test_body_header_on_the_host_on_the_observed_scene(host):
    from omg_planner_amd import planes
    t = SC.observed_depth()[0]
    c = dict(intr=np.tile(PC.observed_intrinsics(), (3, 1)), depth=t, triples=PC.observed_triples(), tol=SC.TOL, min_nn=1e-10, skip=None, up=None, cos_min=-1.0)
    got = host_outputs(host, c, refine=2)
    fit = planes.fit_planes(c["intr"], t, c["triples"], SC.TOL)
    assert np.array_equal(PC.bits(got["final"]), PC.bits(fit.planes)) and np.array_equal(got["counts"], fit.counts) and np.array_equal(got["inliers"], fit.inliers)
    assert np.array_equal(got["mask"], planes.plane_mask(c["intr"], t, fit.planes, SC.TOL))


# ---------------------------------------------------------------------------------------------------------------------
# the library without a GPU: argument errors come before any HIP call
# ---------------------------------------------------------------------------------------------------------------------
def test_every_argument_error_of_section_19_without_a_gpu():
    from omg_planner_amd import _lib, ops
    l, vp = _lib.lib(), C.c_void_p
    OK, INVALID, UNSUPPORTED = _lib.OMGX_OK, _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED
    V, H, W, K = 2, 6, 8, 5
    intr = np.tile(np.array(PC.INTR), (V, 1))
    tri = np.random.default_rng(0).integers(0, H * W, (V, K, 3)).astype(np.int32)
    fake = np.zeros(64)  # stands for device memory: a refused call never touches it
    dp, hp = vp(fake.ctypes.data), lambda a: vp(a.ctypes.data)

    def ransac(**kw):
        a = dict(intrinsics=dp, h_intrinsics=hp(intr), depth=dp, skip=None, V=V, H=H, W=W, triples=dp, h_triples=hp(tri), K=K, tol=0.01, min_nn=1e-10,
                 up=None, cos_min=-1.0, planes=dp, counts=dp, best=dp, best_planes=dp, anchors=dp)
        a.update(kw)
        return l.omgx_plane_ransac(*a.values(), None)

    for name in ("intrinsics", "h_intrinsics", "depth", "triples", "h_triples", "planes", "counts", "best", "best_planes", "anchors"):
        assert ransac(**{name: None}) == INVALID, name
    for change in (dict(V=-1), dict(H=0), dict(W=0), dict(H=-3), dict(K=0), dict(K=-1), dict(K=_lib.PLANE_MAX_HYPOTHESES + 1), dict(tol=-1e-9), dict(tol=NAN),
                   dict(tol=INF), dict(min_nn=-1.0), dict(min_nn=NAN), dict(min_nn=INF), dict(cos_min=1.0001), dict(cos_min=-1.0001), dict(cos_min=NAN)):
        assert ransac(**change) == INVALID, change
    for x, bad in ((0, 0.0), (1, 0.0), (2, NAN), (7, INF), (4, NAN)):
        k = intr.copy()
        k.reshape(-1)[x] = bad
        assert ransac(h_intrinsics=hp(k)) == INVALID, (x, bad)
    for x, bad in ((0, -1), (V * K * 3 - 1, H * W), (7, 1 << 30)):
        t = tri.copy()
        t.reshape(-1)[x] = bad
        assert ransac(h_triples=hp(t)) == INVALID, (x, bad)
    assert ransac(V=0, intrinsics=None, h_intrinsics=None, depth=None, triples=None, h_triples=None, planes=None, counts=None, best=None, best_planes=None,
                  anchors=None) == OK
    assert ransac(V=0, K=0, intrinsics=None, h_intrinsics=None) == INVALID  # (K is checked whatever V is)
    big = np.tile(np.array(PC.INTR), (1, 1))
    # above 2^31 - 1 pixels: an invalid argument is still reported first
    assert ransac(V=1, H=1 << 16, W=1 << 15, h_intrinsics=hp(big), K=1) == UNSUPPORTED
    assert ransac(V=1, H=1 << 16, W=1 << 15, h_intrinsics=hp(big), K=1, tol=-1.0) == INVALID

    def images(fn, tail, **kw):
        a = dict(intrinsics=dp, h_intrinsics=hp(intr), depth=dp, skip=None, V=V, H=H, W=W)
        a.update(tail)
        a.update(kw)
        return fn(*a.values(), None)

    moments = dict(planes=dp, anchors=dp, tol=0.01, workspace=dp, count=dp, sums=dp)
    mask = dict(planes=dp, tol=0.01, mask=dp)
    for fn, tail in ((l.omgx_plane_moments, moments), (l.omgx_plane_mask, mask)):
        for name in ("intrinsics", "h_intrinsics", "depth") + tuple(n for n in tail if n != "tol"):
            assert images(fn, tail, **{name: None}) == INVALID, (fn.__name__, name)
        for change in (dict(V=-1), dict(H=0), dict(W=-1), dict(tol=-1.0), dict(tol=NAN), dict(tol=INF)):
            assert images(fn, tail, **change) == INVALID, (fn.__name__, change)
        k = intr.copy()
        k[1, 1] = 0.0
        assert images(fn, tail, h_intrinsics=hp(k)) == INVALID
        assert images(fn, tail, V=1, H=1 << 16, W=1 << 15) == UNSUPPORTED
        assert fn(None, None, None, None, 0, 0, 0, *([None if n != "tol" else 0.0 for n in tail]), None) == OK
    chunks = -(-H * W // PC.CHUNK)
    assert l.omgx_plane_workspace_bytes(V, H, W) == V * chunks * 80 and l.omgx_plane_workspace_bytes(3, 67, 131) == 3 * 5 * 80
    assert l.omgx_plane_workspace_bytes(0, 0, 0) == 0 and l.omgx_plane_workspace_bytes(-1, 4, 4) == INVALID and l.omgx_plane_workspace_bytes(1, 0, 4) == INVALID
    assert l.omgx_plane_workspace_bytes(1, 1 << 16, 1 << 15) == UNSUPPORTED

    layout, size = PC.pool_layout()
    M = len(layout)
    planes = np.ascontiguousarray(PC.VOLUME_PLANES)

    def volumes(records=None, **kw):
        rec = ops.surface_records(layout) if records is None else records
        a = dict(volumes=dp, h_volumes=C.cast(rec, vp), M=M, planes=dp, h_planes=hp(planes), pool=dp, pool_elems=size)
        a.update(kw)
        return l.omgx_plane_volumes(*a.values(), None)

    for name in ("volumes", "h_volumes", "planes", "h_planes", "pool"):
        assert volumes(**{name: None}) == INVALID, name
    assert volumes(M=-1) == INVALID and volumes(pool_elems=-1) == INVALID and volumes(pool_elems=size - POOL_TAIL - 1) == INVALID
    assert volumes(M=0, volumes=None, h_volumes=None, planes=None, h_planes=None, pool=None) == OK
    for field, bad in (("delta", 0.0), ("delta", NAN), ("delta", -0.01), ("sample_offset", 0.25), ("out_offset", -1), ("first_workgroup", 1)):
        rec = ops.surface_records(layout)
        setattr(rec[0], field, bad)
        assert volumes(rec) == INVALID, (field, bad)
    for a, bad in ((0, 0), (2, -4)):
        rec = ops.surface_records(layout)
        rec[1].dims[a] = bad
        assert volumes(rec) == INVALID
    rec = ops.surface_records(layout)
    rec[1].origin[2] = INF
    assert volumes(rec) == INVALID
    rec = ops.surface_records(layout)
    rec[1].out_offset = rec[0].out_offset + 5  # two volumes overlap in the pool
    assert volumes(rec) == INVALID
    rec = ops.surface_records(layout)
    rec[M - 1].out_offset = size  # outside the pool
    assert volumes(rec) == INVALID
    bad_planes = planes.copy()
    bad_planes[3, 1] = NAN
    assert volumes(h_planes=hp(bad_planes)) == INVALID
    huge = ops.surface_records([((0.0, 0.0, 0.0), 0.01, "centre", (1 << 11, 1 << 10, 1 << 10), 0)])
    assert l.omgx_plane_volumes(dp, C.cast(huge, vp), 1, dp, hp(planes), dp, 1 << 40, None) == UNSUPPORTED


POOL_TAIL = PC.POOL_GUARD  # the elements behind the last volume


def test_wrappers_refuse_bad_arguments_before_anything_touches_a_device():
    """The host halves of the ops wrappers (no GPU: a CPU tensor is refused only after every host argument has been checked)."""
    torch = pytest.importorskip("torch")
    from omg_planner_amd import _lib, ops
    depth = torch.zeros((2, 6, 8), dtype=torch.float64)
    tri = np.zeros((2, 4, 3), np.int32)
    good = dict(intrinsics=PC.INTR, depth=depth, triples=tri, tol=0.01)
    for what, change in (("intrinsics must be", dict(intrinsics=(80.0, 0.0, 1.0, 1.0))), ("intrinsics must be", dict(intrinsics=np.ones((3, 4)))),
                         ("tol must be finite", dict(tol=-1.0)), ("triples must be integers", dict(triples=np.zeros((2, 4, 3)))),
                         ("triples must be integers", dict(triples=np.zeros((1, 4, 3), np.int32))), ("K must lie in", dict(triples=np.zeros((2, 0, 3), np.int32))),
                         ("outside", dict(triples=np.full((2, 4, 3), 48, np.int32))), ("min_nn must be", dict(min_nn=-1.0)), ("min_nn must be", dict(cos_min=2.0)),
                         ("up must be", dict(up=np.ones((3, 3)))), ("up must be", dict(up=(0.0, NAN, 1.0))), ("depth must be a tensor", dict(depth=depth[0])),
                         ("skip must be a bool tensor", dict(skip=torch.zeros((2, 6, 8)))), ("refine must not be negative", dict(refine=-1)),
                         ("must be a device tensor", dict())):
        with pytest.raises(_lib.OmgHipError, match=what):
            ops.fit_planes(**{**good, **change})
    with pytest.raises(_lib.OmgHipError, match="tol must be finite"):
        ops.plane_mask(PC.INTR, depth, np.zeros((2, 4)), NAN)
    for what, vols, pls in (("need as many planes", PC.VOLUMES, PC.VOLUME_PLANES[:2]), ("need as many planes", PC.VOLUMES[:1], [(0.0, NAN, 1.0, 0.0)]),
                            ("three dims >= 1", [((0, 0, 0), 0.01, "centre", (4, 0, 4))], PC.VOLUME_PLANES[:1]),
                            ("sample must be", [((0, 0, 0), 0.01, "corner", (4, 4, 4))], PC.VOLUME_PLANES[:1])):
        with pytest.raises(_lib.OmgHipError, match=what):
            ops.plane_volumes(vols, pls, out=torch.zeros(10))


@KB.requires_hipcc
def test_plane_kernels_use_no_scratch_and_the_documented_lds(tmp_path):
    """No kernel of omg_plane.hip uses scratch or spills; the scoring kernel's LDS is the 3 328 bytes the header documents (64 rows
    of four doubles, 64 live flags, four waves' 64 counts).  Registers and occupancy are printed (DESIGN.md section 7k quotes
    them), not fixed."""
    seen = KB.kernel_resources("omg_plane.hip", tmp_path)
    assert len(seen) == 7
    for part in ("k_plane_hypotheses", "k_plane_score", "k_plane_select", "k_plane_moments", "k_plane_reduce", "k_plane_mask", "k_plane_volumes"):
        v = KB.one(seen, part)
        print(part, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, part
    assert KB.one(seen, "k_plane_score")["LDS Size [bytes/block]"] == PC.STAGE * 4 * 8 + PC.STAGE * 4 + 4 * PC.STAGE * 4 == 3328
    assert KB.one(seen, "k_plane_moments")["LDS Size [bytes/block]"] == 4 * 9 * 8 + 4 * 4
