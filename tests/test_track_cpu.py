"""Camera tracking without a GPU: answers worked by hand, the derivative, the kernels' body compiled for the host against the
specification (omg-planner_amd/tracking.py) bit for bit, track_turn against reg_iterate on recorded sums, argument errors of the
specification, the C ABI and the wrapper, the kernels' resources, and recovery on the slab, sphere and box scene."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import kernel_build as KB
from tests import track_cases as TC

K1 = np.array([[1.0, 1.0, 0.0, 0.0]])  # the identity camera
ID = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])


@pytest.fixture(scope="module")
def tr():
    from omg_planner_amd import tracking
    return tracking


def _pose(tx=0.0, ty=0.0, tz=0.0):
    p = ID.copy()
    p[3], p[7], p[11] = tx, ty, tz
    return p


def _sums(tr, zl, nl, zm, nm, pose, dist2=1.0, cos_min=0.7, k=K1, stride=1):
    cost, count, H, b = tr.one_pass(zl[0], None if nl is None else nl[0], zm[0], nm[0], k[0], pose, stride, dist2, cos_min)
    return cost, count, H, b


# ---------------------------------------------------------------------------------------------------------------------
# answers worked by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_residual_and_the_28_sums_of_a_2_x_2_image(tr):
    """Live plane z = 1.25, model plane z = 1 with n = (0, 0, -1), identity pose and camera: pixel (r, c) has P = (1.25c, 1.25r, 1.25),
    lands on model pixel (r, c), e = (0.25c, 0.25r, 0.25), res = -0.25, g = (0, 0, -1), j = (0, 0, -1, -1.25r, 1.25c, 0)."""
    zl, nl, zm, nm = TC.planes(2, 2)
    valid, inl, res, j, P = tr.pixel_terms(zl[0], nl[0], zm[0], nm[0], K1[0], ID, 1, 0.25, 0.7)
    assert valid.all() and inl.all() and (res == -0.25).all()
    want_j = np.array([[0, 0, -1, -1.25 * r, 1.25 * c, 0] for r in (0, 1) for c in (0, 1)])
    assert np.array_equal(j, want_j) and np.array_equal(P, [[1.25 * c, 1.25 * r, 1.25] for r in (0, 1) for c in (0, 1)])
    cost, count, H, b = _sums(tr, zl, nl, zm, nm, ID, dist2=0.25)
    from omg_planner_amd import registration as reg
    want_H = [sum(a[i] * a[k] for a in want_j) for i, k in reg._TRI]
    assert count == 4 and cost == 0.25 and H.tolist() == want_H and b.tolist() == [0.0, 0.0, 1.0, 0.625, -0.625, 0.0]
    assert H[reg._TRI.index((2, 2))] == 4.0 and H[reg._TRI.index((2, 3))] == 2.5 and H[reg._TRI.index((3, 4))] == -1.5625


def test_one_accepted_step_lands_on_the_model_plane(tr):
    """4 x 4 pixels of which the live frame has the upper left 3 x 3 (after the step pixel c lands on ua = 1.25c + 0.5 <= 3 < W), nine
    inliers (dd <= 0.0625 * 9 <= 1), a damping far below the floor: the first trial moves t_z by -0.25, where res == 0, and is
    accepted."""
    zl, nl, zm, nm = TC.planes(4, 4)
    zl[0, 3, :], zl[0, :, 3] = 0.0, 0.0
    poses, stats = tr.track_cameras(zl, nl, zm, nm, K1, None, dist_max=1.0, lambda0=2.0 ** -60, max_passes=1)
    assert np.abs(poses[0] - _pose(tz=-0.25)).max() < 1e-8
    assert stats[0, tr.COST0] == 9 * 0.0625 and stats[0, tr.COST] < 1e-14 and stats[0, [tr.COUNT0, tr.COUNT, tr.ACCEPTED, tr.TRIALS]].tolist() == [9, 9, 1, 1]


def test_the_edges_of_the_projection(tr):
    """H = 1, W = 2, both planes at z = 1: pixel c has ua = (c + tx) + 0.5.  ua == 0 is inside and one ulp below is outside; ua == W
    is outside and one ulp below is inside."""
    zl, nl, zm, nm = TC.planes(1, 2, z_live=1.0)
    inl = lambda tx: tr.pixel_terms(zl[0], nl[0], zm[0], nm[0], K1[0], _pose(tx=tx), 1, 4.0, 0.7)[1].tolist()
    assert inl(0.0) == [True, True]
    assert inl(-0.5) == [True, True]                       # pixel 0: ua == 0.0
    assert inl(-0.5 - 2.0 ** -53) == [False, True]         # ua == -2^-53
    assert inl(0.5) == [True, False]                       # pixel 1: ua == 2.0 == W
    assert inl(0.5 - 2.0 ** -52) == [True, True]           # ua == 2 - 2^-52
    for far in (1e300, -1e300, np.inf, np.nan):
        cost, count, _, _ = _sums(tr, zl, nl, zm, nm, _pose(tx=far), dist2=4.0)
        assert count == 0 and cost == 8.0


def test_the_edges_of_the_gates(tr):
    zl, nl, zm, nm = TC.planes(1, 1)                       # e = (0, 0, 0.25): dd = 0.0625
    inl = lambda dist2=0.25, cos_min=0.7, nl=nl: tr.pixel_terms(zl[0], None if nl is None else nl[0], zm[0], nm[0], K1[0], ID, 1, dist2, cos_min)[1][0]
    assert inl(dist2=0.0625) and not inl(dist2=float(np.nextafter(0.0625, 0.0)))
    assert inl(cos_min=1.0) and not inl(cos_min=float(np.nextafter(1.0, 2.0)))        # cs = 1.0
    tilted = nl.copy()
    tilted[0, 0, 0] = (0.6, 0.0, -0.8)                                                   # cs = 0.8
    assert inl(cos_min=0.8, nl=tilted) and not inl(cos_min=float(np.nextafter(0.8, 1.0)), nl=tilted)
    assert inl(cos_min=float(np.nextafter(0.8, 1.0)), nl=None)                         # without live normals there is no such test
    assert inl(cos_min=-np.inf) and not inl(cos_min=np.inf)


def test_what_a_pixel_adds(tr):
    """A live pixel without a normal adds nothing; the same pixel without live normals is VALID and adds dist2 when it is no inlier."""
    zl, nl, zm, nm = TC.planes(3, 3)                       # dd <= 0.0625 * 9 <= dist2 = 1: nine inliers of res = -0.25
    assert _sums(tr, zl, nl, zm, nm, ID)[:2] == (9 * 0.0625, 9)
    zl[0, 1, 1] = 3.0                                      # far behind the model: no inlier
    assert _sums(tr, zl, nl, zm, nm, ID)[:2] == (8 * 0.0625 + 1.0, 8)
    nl[0, 1, 1] = 0.0
    assert _sums(tr, zl, nl, zm, nm, ID)[:2] == (8 * 0.0625, 8)
    assert _sums(tr, zl, None, zm, nm, ID)[:2] == (8 * 0.0625 + 1.0, 8)
    zl, nl, zm, nm = TC.planes(3, 3)
    assert _sums(tr, zl, nl, zm, nm, _pose(tz=-1.25))[:2] == (9.0, 0)                     # Q2 == 0 is not in front
    assert _sums(tr, zl, nl, zm, nm, _pose(tz=-2.0))[:2] == (9.0, 0)
    zm[0, 0, 0], nm[0, 2, 2] = np.inf, 0.0                 # background, and a model pixel without a normal
    assert _sums(tr, zl, nl, zm, nm, ID)[:2] == (7 * 0.0625 + 2.0, 7)
    for bad in (0.0, -1.0, np.inf, -np.inf, np.nan):       # live depths that say nothing
        z2 = zl.copy()
        z2[0, 1, 1] = bad
        assert _sums(tr, z2, nl, zm, nm, ID)[:2] == (6 * 0.0625 + 2.0, 6), bad


def test_nan_in_every_input_in_turn(tr):
    for which in range(5):
        zl, nl, zm, nm = TC.planes(3, 3)
        pose = ID.copy()
        if which == 4:
            pose[6] = np.nan
        else:
            (zl, nl, zm, nm)[which].reshape(-1)[4 * (3 if which in (1, 3) else 1)] = np.nan   # pixel (1, 1)
        cost, count, H, b = _sums(tr, zl, nl, zm, nm, pose)
        assert np.isfinite([cost, *H, *b]).all(), which
        assert count == (0 if which == 4 else 8), which
        assert cost == (9.0 if which == 4 else 8 * 0.0625 + (0.0 if which in (0, 1) else 1.0)), which


def test_nothing_to_solve_leaves_the_pose_bits(tr):
    zl, nl, zm, nm = TC.planes(3, 3)
    p0 = TC.rows(TC.rigid((0.2, 0.5, 1.0), 0.01, (0.001, 0.002, -0.003)))[None]
    poses, stats = tr.track_cameras(np.zeros_like(zl), nl, zm, nm, K1, p0, dist_max=1.0)
    assert np.array_equal(TC.bits(poses), TC.bits(p0)) and stats[0].tolist() == [0, 0, 0, 0, 0, 0, 2.0 ** -10, tr.FEW_INLIERS]
    poses, stats = tr.track_cameras(zl, nl, zm, nm, K1, p0, dist_max=1.0, max_passes=0)
    assert np.array_equal(TC.bits(poses), TC.bits(p0)) and stats[0, tr.STATUS] == 0 and stats[0, tr.COUNT0] == 9 and stats[0, tr.TRIALS] == 0
    five = zl.copy()
    five.reshape(-1)[5:] = 0.0
    poses, stats = tr.track_cameras(five, nl, zm, nm, K1, p0, dist_max=1.0)
    assert np.array_equal(TC.bits(poses), TC.bits(p0)) and stats[0, tr.COUNT0] == 5 and stats[0, tr.STATUS] == tr.FEW_INLIERS


def test_a_negative_focal_length_mirrors_the_image(tr):
    """fx = -1 with cx = 2: dx = (c - 2) / -1, ua = -(Q0 / Q2) + 2 + 0.5 = c + 0.5: every pixel finds its own model pixel."""
    zl, nl, zm, nm = TC.planes(3, 3)
    k = np.array([[-1.0, 1.0, 2.0, 0.0]])
    valid, inl, res, j, P = tr.pixel_terms(zl[0], nl[0], zm[0], nm[0], k[0], ID, 1, 1.0, 0.7)
    assert inl.all() and (res == -0.25).all() and P[:3, 0].tolist() == [2.5, 1.25, 0.0]


def test_stride_numbers_the_used_grid(tr):
    zl, nl, zm, nm, intr, p0 = TC.synthetic(17, 33)
    for stride in (2, 3, 40):
        assert tr.used_grid(17, 33, stride) == zl[0, ::stride, ::stride].shape
        valid, _, _, _, P = tr.pixel_terms(zl[0], nl[0], zm[0], nm[0], intr[0], p0[0], stride, 0.0025, 0.7)
        assert np.array_equal(P[:, 2], zl[0, ::stride, ::stride].reshape(-1))            # row-major over the used grid
        assert tr.valid_pixels(zl[:1], nl[:1], stride)[0] == valid.sum()


def test_the_analytic_jacobian_against_central_differences(tr):
    """res as a function of xi under registration.step_pose, the pixel's model point and normal held: d res / d xi == j to 1e-6."""
    from omg_planner_amd import registration as reg
    zl, nl, zm, nm, intr, p0 = TC.synthetic(48, 64)
    fx, fy, cx, cy = intr[0]
    valid, inl, res, j, P = tr.pixel_terms(zl[0], nl[0], zm[0], nm[0], intr[0], p0[0], 1, 0.0025, 0.7)
    assert inl.sum() > 1000
    T = p0[0].reshape(3, 4)
    Q = P @ T[:, :3].T + T[:, 3]
    cm, rm = ((fx * (Q[:, 0] / Q[:, 2]) + cx) + 0.5).astype(int), ((fy * (Q[:, 1] / Q[:, 2]) + cy) + 0.5).astype(int)
    pick = np.nonzero(inl)[0][::37]
    n, zq = nm[0][rm[pick], cm[pick]], zm[0][rm[pick], cm[pick]]
    M = np.stack([(cm[pick] - cx) / fx * zq, (rm[pick] - cy) / fy * zq, zq], -1)

    def f(xi):
        S = reg.step_pose(p0[0], xi).reshape(3, 4)
        return ((P[pick] @ S[:, :3].T + S[:, 3] - M) * n).sum(1)

    assert np.abs(f(np.zeros(6)) - res[pick]).max() < 1e-14
    h = 1e-6
    for a in range(6):
        e = np.zeros(6)
        e[a] = h
        assert np.abs((f(e) - f(-e)) / (2 * h) - j[pick, a]).max() < 1e-6, a


def test_compose_and_accepted_mask(tr):
    T = TC.rigid((0.3, -1.0, 0.4), 0.2, (0.01, 0.02, -0.03))
    cfw0 = TC.look_at((0.5, -0.4, 0.5), (0.0, 0.0, 0.0))
    assert np.abs(tr.compose(TC.rows(T), cfw0) - np.linalg.inv(T) @ cfw0).max() < 1e-15
    assert np.array_equal(tr.compose(ID, cfw0), cfw0)
    stats = np.zeros((4, 8))
    stats[:, tr.COST0], stats[:, tr.COST], stats[:, tr.COUNT] = 2.0, (1.0, 2.0, 1.0, 1.0), (50, 50, 9, 50)
    assert tr.accepted_mask(stats, 10, 0.5, valid=[100, 100, 10, 101]).tolist() == [True, False, False, False]
    assert tr.accepted_mask(stats, 10, 0.5).tolist() == [True, False, False, True]


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' body compiled for the host, walked in the kernels' order
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include <vector>
#include "omg_track_body.h"
static void tree(reg_sums* lane, reg_sums& tot) {   // k_track_pass's sum, lane by lane
    for (int w = 0; w < 4; ++w)
        for (int s = 32; s >= 1; s >>= 1)
            for (int l = 0; l < s; ++l) {
                for (int i = 0; i < REG_NPART; ++i) lane[64 * w + l].x[i] = lane[64 * w + l].x[i] + lane[64 * w + l + s].x[i];
                lane[64 * w + l].count += lane[64 * w + l + s].count;
            }
    for (int i = 0; i < REG_NPART; ++i) tot.x[i] = ((lane[0].x[i] + lane[64].x[i]) + lane[128].x[i]) + lane[192].x[i];
    tot.count = ((lane[0].count + lane[64].count) + lane[128].count) + lane[192].count;
}
extern "C" void host_track(const double* intr, const double* zl, const double* nl, const double* zm, const double* nm, int V, int H, int W,
                           int stride, const double* poses0, double dist_max, double cos_min, double lambda0, double step_tol, int K,
                           double* poses_out, double* stats_out) {
    const int Hu = (H - 1) / stride + 1, Wu = (W - 1) / stride + 1;
    const int64_t used = (int64_t)Hu * Wu, chunks = (used + 2047) / 2048;
    const double dist2 = dist_max * dist_max;
    std::vector<track_state> states(V);
    std::vector<double> rows(V * chunks * TRACK_ROW, NAN);
    for (int v = 0; v < V; ++v) track_begin(states[v], poses0 + 12 * v, lambda0);                  // k_track_init
    for (int turn = 0; turn <= K; ++turn) {
        for (int v = 0; v < V; ++v) {                                                              // k_track_pass
            if (states[v].done) continue;
            const int64_t image = (int64_t)v * H * W;
            track_image I{zl + image, nl ? nl + image * 3 : nullptr, zm + image, nm + image * 3, intr[4 * v], intr[4 * v + 1], intr[4 * v + 2],
                          intr[4 * v + 3], H, W};
            for (int64_t q = 0; q < chunks; ++q) {
                static reg_sums lane[256];
                for (int l = 0; l < 256; ++l) {
                    reg_clear(lane[l]);
                    for (int j = 0; j < 8; ++j) {
                        const int64_t u = q * 2048 + j * 256 + l;
                        int r, c;
                        if (u < used) track_used_pixel(u, Wu, stride, &r, &c), track_pixel(I, states[v].trial, r, c, dist2, cos_min, lane[l]);
                    }
                }
                reg_sums tot;
                tree(lane, tot);
                double* out = rows.data() + (v * chunks + q) * TRACK_ROW;
                for (int i = 0; i < REG_NPART; ++i) out[i] = tot.x[i];
                out[REG_NPART] = (double)tot.count;
            }
        }
        for (int v = 0; v < V; ++v) {                                                              // k_track_step
            if (states[v].done) continue;
            reg_sums tri;
            double total[REG_NPART + 1];
            for (int i = 0; i <= REG_NPART; ++i) {
                total[i] = rows[v * chunks * TRACK_ROW + i];
                for (int64_t q = 1; q < chunks; ++q) total[i] = total[i] + rows[(v * chunks + q) * TRACK_ROW + i];
            }
            for (int i = 0; i < REG_NPART; ++i) tri.x[i] = total[i];
            tri.count = (int32_t)total[REG_NPART];
            if (track_turn(states[v], tri, step_tol, K)) {
                for (int i = 0; i < 12; ++i) poses_out[12 * v + i] = states[v].pose[i];
                track_stats(states[v], stats_out + 8 * v);
            }
        }
    }
}
// track_turn and reg_iterate on one recorded sequence of sums [n][29] (the last row again once it is used up) -> passes taken
extern "C" int host_turns(const double* seq, int n, const double* pose0, double lambda0, double step_tol, int K, double* pose, double* stats) {
    track_state s;
    track_begin(s, pose0, lambda0);
    int taken = 0;
    for (;;) {
        const double* row = seq + 29 * (taken < n ? taken : n - 1);
        reg_sums tri;
        for (int i = 0; i < REG_NPART; ++i) tri.x[i] = row[i];
        tri.count = (int32_t)row[28];
        ++taken;
        if (track_turn(s, tri, step_tol, K)) break;
    }
    for (int i = 0; i < 12; ++i) pose[i] = s.pose[i];
    track_stats(s, stats);
    return taken;
}
extern "C" int host_iterate(const double* seq, int n, const double* pose0, double lambda0, double step_tol, int K, double* pose, double* stats) {
    int taken = 0;
    auto pass = [&](const double*, reg_sums& tot) {
        const double* row = seq + 29 * (taken < n ? taken : n - 1);
        for (int i = 0; i < REG_NPART; ++i) tot.x[i] = row[i];
        tot.count = (int32_t)row[28];
        ++taken;
    };
    for (int i = 0; i < 12; ++i) pose[i] = pose0[i];
    reg_iterate(pass, pose, lambda0, step_tol, K, stats);
    return taken;
}
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    if KB.host_compiler() is None:
        pytest.skip("no C++ compiler")
    vp, dbl, i = C.c_void_p, C.c_double, C.c_int
    loop = (i, [vp, i, vp, dbl, dbl, i, vp, vp])
    return KB.host_harness(_HOST_HARNESS, tmp_path_factory.mktemp("track_host"),
                           {"host_track": (None, [vp] * 5 + [i] * 4 + [vp, dbl, dbl, dbl, dbl, i, vp, vp]), "host_turns": loop, "host_iterate": loop})


def host_track(lib, zl, nl, zm, nm, intr, p0, stride, dist_max, cos_min, lambda0, step_tol, max_passes):
    V, H, W = zl.shape
    arrs = [np.ascontiguousarray(a, np.float64) for a in (intr, zl, zm if nl is None else nl, zm, nm, p0)]
    poses, stats = np.full((V, 12), 7.0), np.full((V, 8), 7.0)
    lib.host_track(arrs[0].ctypes.data, arrs[1].ctypes.data, None if nl is None else arrs[2].ctypes.data, arrs[3].ctypes.data, arrs[4].ctypes.data, V, H, W,
                   int(stride), arrs[5].ctypes.data, float(dist_max), float(cos_min), float(lambda0), float(step_tol), int(max_passes), poses.ctypes.data,
                   stats.ctypes.data)
    return poses, stats


@pytest.mark.parametrize("H,W", TC.SHAPES)
def test_kernel_body_compiled_for_the_host_equals_the_specification(host_lib, tr, H, W):
    """csrc/omg_track_body.h walked as the kernels walk it (chunks of 2048 used pixels, 256 lanes of 8, the tree, the chunk rows
    left to right, turn by turn, a finished view skipped) gives the specification's poses and stats as bits: V = 3 views with three
    intrinsics, strides 1, 2, 3, with and without live normals, K in {0, 1, 2, 12}."""
    zl, nl, zm, nm, intr, p0 = TC.synthetic(H, W)
    seen = set()
    for stride in TC.STRIDES:
        for K in TC.PASSES:
            for with_normals in (True, False):
                if K in (1, 2) and (stride == 2) == with_normals:   # (every K with every stride; half the pairs with each kind of normals)
                    continue
                want = TC.synthetic_spec(H, W, stride, K, with_normals)
                got = host_track(host_lib, zl, nl if with_normals else None, zm, nm, intr, p0, **dict(TC.DEFAULT, stride=stride, max_passes=K))
                assert TC.same(got, want), (H, W, stride, K, with_normals)
                seen |= set(want[1][:, tr.STATUS].astype(int).tolist())
    if H * W >= 256:
        assert tr.CONVERGED in seen or 0 in seen


def test_kernel_body_on_dirty_images_and_on_the_views_that_stop_at_different_turns(host_lib, tr):
    for seed in range(4):
        zl, nl, zm, nm, intr, p0 = TC.synthetic(23, 89, 3, seed, dirty=True)
        args = dict(TC.DEFAULT, stride=1 + seed % 2, max_passes=6)
        assert TC.same(host_track(host_lib, zl, nl, zm, nm, intr, p0, **args), tr.track_cameras(zl, nl, zm, nm, intr, p0, **args)), seed
    args, want = TC.turns()
    assert TC.same(host_track(host_lib, *args, **TC.TURNS), want)
    stats = want[1]
    assert stats[0].tolist()[2:6] == [0, 0, 0, 0] and stats[0, tr.STATUS] == tr.FEW_INLIERS                       # stops at the first step
    assert stats[1, tr.TRIALS] == 1 and stats[1, tr.ACCEPTED] == 1 and int(stats[1, tr.STATUS]) == tr.CONVERGED    # one trial
    assert stats[2, tr.TRIALS] >= 3 and stats[2, tr.COST] < 0.5 * stats[2, tr.COST0]                               # the far one works longest
    assert stats[3, tr.COUNT0] == 0 and stats[3, tr.STATUS] == tr.FEW_INLIERS and np.isnan(want[0][3, 5])          # the NaN pose comes back
    assert len({int(s) for s in stats[:, tr.TRIALS]}) >= 3


def _sequence(costs, counts=None, bad_pivot=()):
    """Recorded sums [n][29]: H = J^T J + I of seeded j's (positive definite), b seeded, the given costs and counts."""
    rng = np.random.default_rng(len(costs))
    from omg_planner_amd import registration as reg
    seq = np.zeros((len(costs), 29))
    for i, cost in enumerate(costs):
        J = rng.normal(size=(12, 6))
        A = J.T @ J + np.eye(6)
        if i in bad_pivot:
            A[0, 0] = -1.0
        seq[i, :21] = [A[a, b] for a, b in reg._TRI]
        seq[i, 21:27] = 1e-3 * rng.normal(size=6)
        seq[i, 27], seq[i, 28] = cost, 100 if counts is None else counts[i]
    return seq


@pytest.mark.parametrize("name,seq,lambda0,step_tol,K", [
    ("rejected, accepted, K exhausted", _sequence([10.0, 12.0, 8.0, 9.0, 7.0, 7.5]), 2.0 ** -10, 1e-9, 4),
    ("an accepted trial converges", _sequence([10.0, 9.0, 8.0]), 2.0 ** -10, 1e9, 12),
    ("a singular solve, then lambda at its maximum", _sequence([10.0, 9.0], bad_pivot=(0,)), 2.0 ** 10, 1e-9, 12),
    ("a singular solve inside the loop", _sequence([10.0, 9.0, 8.5, 8.0], bad_pivot=(1,)), 2.0 ** -10, 1e-9, 5),
    ("rejections until lambda reaches its maximum", _sequence([10.0, 11.0, 12.0, 13.0]), 2.0 ** 14, 1e-9, 12),
    ("equal cost is a rejection", _sequence([10.0, 10.0, 10.0]), 2.0 ** -10, 1e-9, 2),
    ("NaN cost", _sequence([10.0, np.nan, 9.0]), 2.0 ** -10, 1e-9, 3),
    ("too few inliers after an accepted trial", _sequence([10.0, 9.0, 8.0], counts=[100, 5, 100]), 2.0 ** -10, 1e-9, 12),
    ("too few inliers at once", _sequence([10.0], counts=[5]), 2.0 ** -10, 1e-9, 12),
    ("K = 0", _sequence([10.0, 9.0]), 2.0 ** -10, 1e-9, 0),
])
def test_track_turn_and_reg_iterate_are_one_rule(host_lib, tr, name, seq, lambda0, step_tol, K):
    """track_turn driven with a recorded sequence of sums leaves the pose and stats bits, and takes as many passes, as reg_iterate
    whose pass returns the same sequence."""
    p0 = TC.rows(TC.rigid((0.1, 0.7, -0.3), 0.05, (0.01, -0.02, 0.03)))
    out = []
    for fn in (host_lib.host_turns, host_lib.host_iterate):
        pose, stats = np.full(12, 7.0), np.full(8, 7.0)
        taken = fn(seq.ctypes.data, len(seq), p0.ctypes.data, lambda0, step_tol, K, pose.ctypes.data, stats.ctypes.data)
        out.append((taken, pose, stats))
    (t1, p1, s1), (t2, p2, s2) = out
    print(name, "passes", t1, "stats", s1.tolist())
    assert t1 == t2 and TC.same((p1, s1), (p2, s2)), name
    assert t1 <= K + 1
    status = int(s1[tr.STATUS])
    want = {"rejected, accepted, K exhausted": (0, 4, None), "an accepted trial converges": (tr.CONVERGED, 1, 1),
            "a singular solve, then lambda at its maximum": (tr.SINGULAR | tr.LAMBDA_AT_MAX, None, 0),
            "rejections until lambda reaches its maximum": (tr.LAMBDA_AT_MAX, 2, 0), "equal cost is a rejection": (0, 2, 0),
            "too few inliers at once": (tr.FEW_INLIERS, 0, 0), "K = 0": (0, 0, 0)}.get(name)
    if want:
        assert status == want[0] and (want[1] is None or s1[tr.TRIALS] == want[1]) and (want[2] is None or s1[tr.ACCEPTED] == want[2]), (name, s1)
    if name == "rejected, accepted, K exhausted":
        assert 1 <= s1[tr.ACCEPTED] < 4
    if "singular" in name:
        assert status & tr.SINGULAR
    if name == "too few inliers after an accepted trial":
        assert status == tr.FEW_INLIERS and s1[tr.ACCEPTED] == 1 and s1[tr.COUNT] == 5


# ---------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_the_specification_refuses_bad_arguments(tr):
    zl, nl, zm, nm, intr, p0 = TC.synthetic(16, 16)
    ok = lambda zl=zl, nl=nl, zm=zm, nm=nm, intr=intr, p0=p0, **kw: tr.track_cameras(zl, nl, zm, nm, intr, p0, **dict(dict(max_passes=0), **kw))
    ok()
    ok(cos_min=-np.inf, stride=99, lambda0=1e300, dist_max=1e-300)
    bad = [dict(zl=zl[0]), dict(zl=zl.astype(np.float32)), dict(zm=zm[:2]), dict(nm=nm[..., :2]), dict(nl=nl[:, :8]), dict(intr=intr[:2]), dict(intr=intr[:, :3]),
           dict(p0=p0[:2]), dict(p0=p0[:, :11]), dict(stride=0), dict(stride=-1), dict(max_passes=-1), dict(max_passes=tr.MAX_PASSES + 1), dict(cos_min=np.nan)]
    for name in ("dist_max", "lambda0"):
        bad += [{name: x} for x in (0.0, -1.0, np.nan, np.inf, -np.inf)]
    for col, x in ((0, 0.0), (1, 0.0), (0, np.nan), (2, np.inf), (3, -np.inf)):
        k = intr.copy()
        k[1, col] = x
        bad.append(dict(intr=k))
    for kw in bad:
        with pytest.raises(ValueError):
            ok(**kw)
    k = intr.copy()
    k[:, 0] = -k[:, 0]                                       # a negative focal length is a camera
    ok(intr=k)


def test_c_abi_argument_checks_without_gpu(tr):
    """Every OMGX_ERR_INVALID and OMGX_ERR_UNSUPPORTED case of omgx_track_cameras is decided on the host before any HIP call."""
    from omg_planner_amd import _lib, registration as reg
    lib = _lib.lib()
    assert lib.omgx_abi_version() == 14 and (tr.PIXELS_PER_WORKGROUP, tr.MAX_PASSES, tr.STATS) == (2048, reg.MAX_PASSES, 8)
    INV, UNS, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED, _lib.OMGX_OK
    V, H, W = 2, 20, 30
    ws_bytes = lib.omgx_track_workspace_bytes(V, H, W, 1)
    assert ws_bytes == V * (512 + 1 * 32 * 8) and lib.omgx_track_workspace_bytes(1, 48, 64, 1) == 512 + 2 * 256
    assert lib.omgx_track_workspace_bytes(1, 48, 64, 2) == 512 + 256 and lib.omgx_track_workspace_bytes(0, 0, 0, 1) == 0
    assert lib.omgx_track_workspace_bytes(-1, 4, 4, 1) == INV and lib.omgx_track_workspace_bytes(1, 0, 4, 1) == INV and lib.omgx_track_workspace_bytes(1, 4, 4, 0) == INV
    assert lib.omgx_track_workspace_bytes(70000, 4, 4, 1) == UNS and lib.omgx_track_workspace_bytes(4, 1 << 15, 1 << 15, 1) == UNS
    k0 = np.array([[30.0, 31.0, 14.5, 9.5], [-30.0, 31.0, 14.5, 9.5]])
    # device pointers that are never dereferenced: every call below fails its checks first.  Far apart, so that nothing overlaps.
    base = dict(intr=1 << 30, zl=2 << 30, nl=3 << 30, zm=4 << 30, nm=5 << 30, p0=6 << 30, ws=7 << 30, poses=8 << 30, stats=9 << 30)

    def call(k=k0, V=V, H=H, W=W, stride=1, dist_max=0.05, cos_min=0.7, lambda0=1e-3, step_tol=1e-6, K=12, ws_bytes=ws_bytes, host=True, **ptr):
        p = dict(base, **ptr)
        vp = lambda x: None if x is None else C.c_void_p(x)
        k = np.ascontiguousarray(k, np.float64)
        return lib.omgx_track_cameras(vp(p["intr"]), C.c_void_p(k.ctypes.data) if host else None, vp(p["zl"]), vp(p["nl"]), vp(p["zm"]), vp(p["nm"]), V, H, W,
                                      stride, vp(p["p0"]), dist_max, cos_min, lambda0, step_tol, K, vp(p["ws"]), ws_bytes, vp(p["poses"]), vp(p["stats"]), None)

    for name in ("intr", "zl", "zm", "nm", "p0", "ws", "poses", "stats"):
        assert call(**{name: None}) == INV, name
    assert call(host=False) == INV
    assert call(V=-1) == INV and call(H=0) == INV and call(W=0) == INV and call(H=-3) == INV
    assert call(stride=0) == INV and call(stride=-2) == INV and call(K=-1) == INV and call(K=tr.MAX_PASSES + 1) == INV
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(dist_max=bad) == INV and call(lambda0=bad) == INV, bad
    assert call(cos_min=float("nan")) == INV
    for col, x in ((0, 0.0), (1, 0.0), (0, np.nan), (2, np.inf), (3, -np.inf)):
        k = k0.copy()
        k[1, col] = x
        assert call(k=k) == INV, (col, x)
    assert call(ws_bytes=ws_bytes - 1) == INV and call(ws_bytes=-1) == INV
    # an output that shares a byte with an input, or with another output; poses_out == poses0 alone is allowed
    pixels = V * H * W
    for out, size in (("poses", V * 96), ("stats", V * 64), ("ws", ws_bytes)):
        for inp, n in (("intr", V * 32), ("zl", pixels * 8), ("nl", pixels * 24), ("zm", pixels * 8), ("nm", pixels * 24), ("p0", V * 96)):
            assert call(**{out: base[inp] + n - 8}) == INV, (out, inp)
            assert call(**{out: base[inp] - size + 8}) == INV, (out, inp)
    assert call(poses=base["p0"] + 96) == INV and call(stats=base["p0"]) == INV and call(ws=base["p0"]) == INV
    assert call(stats=base["poses"] + 8) == INV and call(ws=base["poses"]) == INV and call(ws=base["stats"] - ws_bytes + 8) == INV
    many = np.tile(k0[:1], (70000, 1))
    assert call(k=many, V=70000, ws_bytes=1 << 40) == UNS and call(k=many, V=4, H=1 << 15, W=1 << 15, ws_bytes=1 << 40) == UNS
    # nothing to do: no view (everything per view may then be NULL), and nothing is launched
    assert call(V=0) == OK
    assert call(V=0, H=0, W=0, host=False, ws_bytes=0, **{n: None for n in base}) == OK


def test_wrapper_checks_without_gpu(tr):
    """Every argument error ops.track_cameras can see itself raises on host tensors, before anything asks where a tensor lies; with
    valid arguments the first complaint is that the tensors are not on a device."""
    import torch
    from omg_planner_amd import _lib, ops
    E = _lib.OmgHipError
    V, H, W = 2, 6, 7
    zl, zm = torch.ones((V, H, W), dtype=torch.float64), torch.ones((V, H, W), dtype=torch.float64)
    nl, nm = torch.zeros((V, H, W, 3), dtype=torch.float64), torch.zeros((V, H, W, 3), dtype=torch.float64)
    k = np.array([[30.0, 30.0, 3.0, 2.5]] * V)
    wrap = lambda zl=zl, nl=nl, zm=zm, nm=nm, k=k, **kw: ops.track_cameras(zl, nl, zm, nm, k, **kw)
    with pytest.raises(E, match="device tensor"):
        wrap()
    with pytest.raises(E, match="device tensor"):
        wrap(nl=None, stride=50, max_passes=0, cos_min=-np.inf, dist_max=1e-300, poses0=np.zeros((V, 12)))
    for kw in (dict(stride=0), dict(stride=-3)):
        with pytest.raises(E, match="stride must be"):
            wrap(**kw)
    for kw in (dict(max_passes=-1), dict(max_passes=tr.MAX_PASSES + 1)):
        with pytest.raises(E, match="max_passes must be"):
            wrap(**kw)
    for name in ("dist_max", "lambda0"):
        for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
            with pytest.raises(E, match="finite and positive"):
                wrap(**{name: bad})
    with pytest.raises(E, match="cos_min"):
        wrap(cos_min=np.nan)
    for kw in (dict(zl=zl[0]), dict(zl=zl.numpy()), dict(zm=zm[:1]), dict(nm=nm[..., :2]), dict(nl=nl[:, :3]), dict(nm=None)):
        with pytest.raises(E, match="must be a tensor"):
            wrap(**kw)
    for bad in (k[:1], k[:, :3], np.array([[0.0, 30.0, 3.0, 2.5]] * V), np.array([[30.0, np.nan, 3.0, 2.5]] * V)):
        with pytest.raises(E, match="intrinsics must be"):
            wrap(k=bad)
    for bad in (np.zeros((1, 12)), np.zeros((V, 16)), torch.zeros((V, 3, 4), dtype=torch.float64)):
        with pytest.raises(E, match="poses0 must be"):
            wrap(poses0=bad)
    with pytest.raises(E, match="H and W"):
        wrap(zl=torch.ones((V, 0, W), dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# resources
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_track_kernels_do_not_spill(tmp_path):
    """The compiler's resource remarks for csrc/omg_track.hip: no kernel uses scratch; k_track_pass keeps a lane's 28 partials in
    registers and its LDS is the four wave totals and counts."""
    res = KB.kernel_resources("omg_track.hip", tmp_path)
    for part in ("k_track_init", "k_track_pass", "k_track_step"):
        v = KB.one(res, part)
        print(part, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (part, v)
    assert KB.one(res, "k_track_pass")["SGPRs Spill"] == 0
    assert KB.one(res, "k_track_pass")["LDS Size [bytes/block]"] == 4 * (28 * 8 + 4)
    assert KB.one(res, "k_track_step")["LDS Size [bytes/block]"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# recovery, by the specification alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(TC.REC_SEEDS)))
def test_the_specification_recovers_the_camera_to_half_a_voxel(tr, i):
    """The slab, sphere and box scene at 1 cm seen by a 120 x 160 camera; the live frame is rendered at a camera moved by up to 30 mm
    and 8 degrees (seeded), its normals come from sensor.depth_normals.  From identity the camera of compose ends within half the
    model's voxel (5 mm) and 0.5 degree of the truth, with and without live normals, at stride 1 and 2.
    Reached by the committed specification on the five starts: 0.07 to 0.72 mm and 0.0006 to 0.062 degrees, in 5 to 30 trials."""
    R = TC.recovery()
    s = R["starts"][i]
    e0 = TC.camera_error(R["cfw"], s["truth"])
    for with_normals, stride in TC.REC_VARIANTS:
        poses, stats = TC.recovery_spec(i, with_normals, stride)
        e = TC.camera_error(tr.compose(poses[0], R["cfw"]), s["truth"])
        print(f"start {i} ({s['mm']:.1f} mm, {s['degrees']:.2f} deg), normals {with_normals}, stride {stride}: {e0[0] * 1e3:.2f} mm / {e0[1]:.3f} deg -> "
              f"{e[0] * 1e3:.3f} mm / {e[1]:.4f} deg, trials {int(stats[0, tr.TRIALS])}, inliers {int(stats[0, tr.COUNT0])} -> {int(stats[0, tr.COUNT])}")
        assert e[0] < 0.5 * TC.REC_DELTA and e[1] < 0.5, (i, with_normals, stride, e)
        valid = tr.valid_pixels(s["zl"], s["nl"] if with_normals else None, stride)
        assert tr.accepted_mask(stats, 100, 0.5, valid).all()
