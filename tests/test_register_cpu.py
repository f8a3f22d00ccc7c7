"""Registration of known volumes to observed clouds, without a GPU: the specification (omg-planner_amd/registration.py) recovers
poses, every special case holds what it is there for, the kernel's body compiled for the host has the specification's bits,
argument errors come back through the C ABI and the wrapper, and the kernel uses no scratch."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import kernel_build as KB
from tests import register_cases as RC


@pytest.fixture(scope="module")
def reg():
    from omg_planner_amd import registration
    return registration


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _rms_surface(c, row, m):
    pts = c["points"][c["ranges"][m, 0]: c["ranges"][m, 1]: c["stride"]]
    pts = pts[np.isfinite(pts).all(1) & (np.abs(pts) < 1e3).all(1)]
    return float(np.sqrt((RC.surface_distance(c["kind"], RC.to_object(row, pts)) ** 2).mean()))


# ---------------------------------------------------------------------------------------------------------------------
# recovery, by the specification alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,grid,delta,n", RC.RECOVERY)
def test_the_specification_recovers_poses_to_half_a_voxel(kind, grid, delta, n):
    """Full-surface clouds under random poses, starts 20 mm and 10 degrees away: the translation error and the RMS distance of
    the cloud to the true surface in the recovered frame (the measure that does not mind the box's own symmetries) end below
    half a voxel, the resolution of the data.  Both volumes, both grids, both cloud sizes.  Reached by the committed specification: <= 0.023 voxels on every case."""
    name = f"{kind}{grid}_{n}"
    c = RC.call(name)
    poses, stats = RC.spec(name)
    for m in range(len(poses)):
        terr = float(np.linalg.norm(poses[m].reshape(3, 4)[:, 3] - c["truth"][m][:3, 3]))
        rms0, rms = _rms_surface(c, c["poses0"][m], m), _rms_surface(c, poses[m], m)
        print(f"{name} instance {m}: translation error {terr * 1e3:.3f} mm = {terr / delta:.4f} voxels, rms {rms0 * 1e3:.2f} -> {rms * 1e3:.3f} mm, "
              f"trials {int(stats[m, 5])}, accepted {int(stats[m, 4])}")
        assert rms0 > 0.3 * delta                      # the start is away from the truth
        assert terr < 0.5 * delta and rms < 0.5 * delta, (name, m, terr, rms)
        assert stats[m, 1] < stats[m, 0] and stats[m, 3] >= 0.95 * n


def test_end_to_end_at_toy_size_by_the_specifications(reg):
    """scenes.mesh_sdf of a 12-face box and an 80-face ellipsoid, camera.render_depth and camera.pixel_clouds of two scenes at
    48 x 40 with the object index as label, starts 20 mm / 10 degrees away: the refined poses bring the one-sided clouds' RMS |v|
    below half a voxel and below a tenth of its starting value."""
    T = RC.toy()
    c = T["call"]
    poses, stats = RC.toy_spec()
    assert [g.data.shape for g in T["grids"]] == [(20, 16, 26), (23, 17, 26)] and len(T["meshes"][0][1]) == 12 and len(T["meshes"][1][1]) == 80
    for m in range(4):
        pts = c["points"][c["ranges"][m, 0]: c["ranges"][m, 1]]
        assert len(pts) >= 100 and np.array_equal(pts, T["clouds"][tuple(T["pairs"][m])])
        rms = []
        for row in (c["poses0"][m], poses[m]):
            inside, v, _ = reg.value_gradient(c["objects"][c["obj_index"][m]], c["pool"], RC.to_object(row, pts))
            assert inside.all()
            rms.append(float(np.sqrt((v ** 2).mean())))
        print(f"toy instance {m}: rms |v| {rms[0] * 1e3:.2f} -> {rms[1] * 1e3:.3f} mm")
        assert rms[1] < 0.5 * RC.TOY_DELTA and rms[1] < 0.1 * rms[0], (m, rms)
    # the far start on the same cloud ends where the near one does; the empty range is left alone
    assert abs(stats[4, reg.COST] - stats[0, reg.COST]) < 1e-9 and stats[5, reg.COUNT] == 0
    mask = reg.accepted_mask(stats, T["pairs"], RC.TOY_MIN_INLIERS)
    winner = reg.best_of(stats, [[0, 4]])[0]
    want = np.zeros(6, bool)
    want[[winner, 1, 2]] = True   # (scene 1, ellipsoid): the empty range has the lowest cost, 0, and does not pass: nothing accepted
    assert np.array_equal(mask, want)


# ---------------------------------------------------------------------------------------------------------------------
# each case holds what it is there for
# ---------------------------------------------------------------------------------------------------------------------
def test_a_rejected_and_an_accepted_trial(reg):
    _, stats = RC.spec("reject_accept")
    h = RC.history(RC.call("reject_accept"))
    accepted = int(stats[0, reg.ACCEPTED])
    assert 1 <= accepted < int(stats[0, reg.TRIALS]) == len(h) - 1
    costs = [x[0] for x in h]
    assert any(b >= min(costs[:k + 1]) for k, b in enumerate(costs[1:])) and costs[1] < costs[0]


def test_the_inlier_set_changes_between_passes(reg):
    _, stats = RC.spec("small_trunc")
    counts = [x[1] for x in RC.history(RC.call("small_trunc"))]
    assert len(set(counts)) >= 3 and counts[0] < 400 == counts[-1] and stats[0, reg.COUNT0] == counts[0] and stats[0, reg.COUNT] == 400


def test_sphere_centre_recovered_rotation_stays_orthogonal(reg):
    c = RC.call("sphere")
    poses, stats = RC.spec("sphere")
    P = poses[0].reshape(3, 4)
    assert np.linalg.norm(P[:, 3] - c["truth"][0][:3, 3]) < 0.5 * c["delta"]
    assert np.abs(P[:, :3].T @ P[:, :3] - np.eye(3)).max() < 1e-12 and np.isfinite(poses).all()
    # without the floor and the damping the rotations have no pivot worth dividing by
    H = reg.one_pass(c["objects"][0], c["pool"], poses[0], c["points"], c["trunc"])[2]
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(reg._TRI):
        A[i, j] = A[j, i] = H[k]
    assert np.linalg.eigvalsh(A)[0] < 1e-3 * np.linalg.eigvalsh(A)[3]


def test_one_face_has_exact_zeros_on_the_diagonal_and_the_floor_carries_them(reg, monkeypatch):
    c = RC.call("one_face")
    cost, count, H, b = reg.one_pass(c["objects"][0], c["pool"], c["poses0"][0], c["points"], c["trunc"])
    diag = [H[k] for k, (i, j) in enumerate(reg._TRI) if i == j]
    assert count == 200 and diag[0] > 0 and diag[1] == 0.0 and diag[2] == 0.0 and diag[3] == 0.0
    ok, xi = reg.solve6(H, b, c["lambda0"])
    assert ok and abs(xi[0] - 0.004) < 2e-4 and xi[1] == 0.0 and xi[2] == 0.0 and xi[3] == 0.0
    monkeypatch.setattr(reg, "FLOOR", 0.0)
    assert not reg.solve6(H, b, c["lambda0"])[0]
    monkeypatch.undo()
    poses, stats = RC.spec("one_face")
    assert not int(stats[0, reg.STATUS]) & reg.SINGULAR and stats[0, reg.COST] < 0.01 * stats[0, reg.COST0]
    assert abs(poses[0][3]) < 2e-4                                         # the face's own coordinate is found


def test_nothing_to_solve_leaves_the_pose_bits(reg):
    for name, count in (("all_outside", 0), ("few_inliers", 5), ("empty_range", 0)):
        c = RC.call(name)
        poses, stats = RC.spec(name)
        assert np.array_equal(_bits(poses), _bits(c["poses0"])), name
        assert stats[0, reg.COUNT0] == count == stats[0, reg.COUNT] and int(stats[0, reg.STATUS]) == reg.FEW_INLIERS, name
        assert stats[0, reg.TRIALS] == 0 and stats[0, reg.COST] == stats[0, reg.COST0], name
    n = 300
    assert RC.spec("all_outside")[1][0, reg.COST0] == pytest.approx(n * 0.03 ** 2, rel=1e-12)
    assert RC.spec("empty_range")[1][0, reg.COST0] == 0.0
    c = RC.call("k0")
    poses, stats = RC.spec("k0")
    assert np.array_equal(_bits(poses), _bits(c["poses0"])) and int(stats[0, reg.STATUS]) == 0 and stats[0, reg.COUNT0] == 300


def test_points_that_are_not_finite_are_outside(reg):
    c = RC.call("not_finite")
    poses, stats = RC.spec("not_finite")
    bad = ~np.isfinite(c["points"]).all(1) | (np.abs(c["points"]) > 1e10).any(1)
    assert bad.sum() == 6 and stats[0, reg.COUNT0] <= 294 and stats[0, reg.COUNT] == 294 and np.isfinite(poses).all() and np.isfinite(stats).all()
    assert np.linalg.norm(poses[0].reshape(3, 4)[:, 3] - c["truth"][0][:3, 3]) < 0.5 * c["delta"]
    good = dict(c, points=c["points"][~bad], ranges=np.array([[0, 294]], np.int32))
    assert reg.register_clouds(*RC.args(good))[1][0, reg.COST] == pytest.approx(stats[0, reg.COST] - 6 * c["trunc"] ** 2, rel=1e-9)


def test_ragged_pool_and_non_cubic_grid(reg):
    c = RC.call("ragged")
    assert c["objects"]["dim"][1].tolist() == [8, 9, 10] and c["objects"]["grid_offset"][1] == 3 + 16 ** 3 + 5 and np.isnan(c["pool"]).sum() == 9
    poses, stats = RC.spec("ragged")
    assert np.isfinite(stats).all() and np.linalg.norm(poses[0].reshape(3, 4)[:, 3] - c["truth"][0][:3, 3]) < 0.5 * c["delta"]
    # the same volume alone at offset 0 gives the same bits: only the record says where a grid lies
    rec, pool = RC.table([RC.volume("ellipsoid", (8, 9, 10), 0.03)])
    alone = reg.register_clouds(*RC.args(dict(c, objects=rec, pool=pool, obj_index=np.array([0], np.int32))))
    assert np.array_equal(_bits(alone[0]), _bits(poses)) and np.array_equal(_bits(alone[1]), _bits(stats))


def test_two_starts_on_one_range_and_best_of(reg):
    c = RC.call("shared_range")
    poses, stats = RC.spec("shared_range")
    assert c["ranges"][0].tolist() == c["ranges"][1].tolist() and stats[0, reg.COUNT0] < stats[1, reg.COUNT0]
    for m in range(3):
        assert np.linalg.norm(poses[m].reshape(3, 4)[:, 3] - c["truth"][m][:3, 3]) < 0.5 * c["delta"]
    best = reg.best_of(stats, [[0, 1], [2], [1, 0]])
    assert best[0] == best[2] == (0 if stats[0, reg.COST] <= stats[1, reg.COST] else 1) and best[1] == 2
    tie = np.zeros((3, 8))
    tie[:, reg.COST] = [2.0, 1.0, 1.0]
    assert reg.best_of(tie, [[2, 1, 0], [0, 2]]) == [1, 2]


def test_stride_takes_every_third_point(reg):
    c = RC.call("stride3")
    poses, stats = RC.spec("stride3")
    thinned = dict(c, points=c["points"][::3], ranges=np.array([[0, 300]], np.int32), stride=1)
    other = reg.register_clouds(*RC.args(thinned))
    assert stats[0, reg.COUNT] == 300 and np.array_equal(_bits(other[0]), _bits(poses)) and np.array_equal(_bits(other[1]), _bits(stats))


def test_cayley_is_a_rotation_and_matches_the_angle(reg):
    rng = np.random.default_rng(0)
    for _ in range(20):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        angle = rng.uniform(-3.0, 3.0)
        Cm = reg.cayley(np.tan(angle / 2) * axis)
        assert np.abs(Cm - RC.rotation(axis, angle)).max() < 1e-12 and abs(np.linalg.det(Cm) - 1) < 1e-12
    assert np.array_equal(reg.cayley([0.0, 0.0, 0.0]), np.eye(3))
    assert np.abs(reg.cayley([1e8, -3e7, 2e5]).T @ reg.cayley([1e8, -3e7, 2e5]) - np.eye(3)).max() < 1e-12


def test_the_analytic_gradient_is_the_interpolants_own(reg):
    rec, pool = RC.table([RC.volume("ellipsoid", (8, 9, 10), 0.03)], gaps=(7,))
    rng = np.random.default_rng(1)
    q = rng.uniform(-0.08, 0.08, (200, 3))
    inside, v, g = reg.value_gradient(rec[0], pool, q)
    assert inside.all()
    h = 1e-7
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        (ip, vp, _), (im, vm, _) = reg.value_gradient(rec[0], pool, q + e), reg.value_gradient(rec[0], pool, q - e)
        u = (q[:, a] - float(rec[0]["lo"][a])) / 0.03 - 0.5
        smooth = np.abs(u - np.round(u)) > 1e-4       # the interpolant has a kink on the cell faces
        assert np.abs((vp - vm) / (2 * h) - g[:, a])[smooth].max() < 1e-6
    assert not reg.value_gradient(rec[0], pool, [[np.nan, 0, 0], [0, np.inf, 0], [1e300, 0, 0], [0, 0, -1e300], [0.3, 0, 0]])[0].any()
    # the last sample of an axis is a corner, never a base: u = dim - 1 is outside, just below it is inside
    lo = rec[0]["lo"].astype(np.float64)
    edge = lo + (np.array([8, 9, 10]) - 0.5) / float(rec[0]["inv_delta"])
    assert not reg.value_gradient(rec[0], pool, [edge + 1e-7])[0][0] and reg.value_gradient(rec[0], pool, [edge - 1e-7])[0][0]
    for a in range(3):
        e = np.zeros(3)
        e[a] = 2e-7
        assert not reg.value_gradient(rec[0], pool, [edge - 1e-7 + e])[0][0]


# ---------------------------------------------------------------------------------------------------------------------
# the kernel body compiled for the host
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include "omg_register_body.h"
struct rec { float pose_inv[12], lo[3], hi[3]; int32_t dim[3]; float delta, epsilon, padding_scale, clearance; int32_t disabled;
             int64_t grid_offset; double inv_extent[3]; float rb_c[3], rb_h[3], rb_r, rb_r2; double inv_delta; float inv_2eps, inv_eps; };
static_assert(sizeof(rec) == 184, "omgx_object");
extern "C" void host_register(const rec* objects, const float* pool, const int32_t* obj_index, const double* poses0, const double* points,
                              const int32_t* ranges, int M, int stride, double trunc, double lambda0, double step_tol, int max_passes,
                              double* poses_out, double* stats_out) {
    for (int m = 0; m < M; ++m) {
        const rec& ob = objects[obj_index[m]];
        reg_grid G;
        for (int a = 0; a < 3; ++a) G.lo[a] = (double)ob.lo[a], G.dim[a] = ob.dim[a];
        G.inv_delta = ob.inv_delta, G.offset = ob.grid_offset;
        const int64_t begin = ranges[2 * m], end = ranges[2 * m + 1], used = (end - begin + stride - 1) / stride;
        const double tau2 = trunc * trunc;
        auto pass = [&](const double* P, reg_sums& tot) {   // the kernel's sum, lane by lane
            static reg_sums lane[256];
            for (int l = 0; l < 256; ++l) {
                reg_clear(lane[l]);
                for (int64_t j = l; j < used; j += 256) {
                    const double* p = points + (begin + j * stride) * 3;
                    reg_point(G, pool, P, p[0], p[1], p[2], trunc, tau2, lane[l]);
                }
            }
            for (int w = 0; w < 4; ++w)
                for (int s = 32; s >= 1; s >>= 1)
                    for (int l = 0; l < s; ++l) {
                        for (int i = 0; i < REG_NPART; ++i) lane[64 * w + l].x[i] = lane[64 * w + l].x[i] + lane[64 * w + l + s].x[i];
                        lane[64 * w + l].count += lane[64 * w + l + s].count;
                    }
            for (int i = 0; i < REG_NPART; ++i) tot.x[i] = ((lane[0].x[i] + lane[64].x[i]) + lane[128].x[i]) + lane[192].x[i];
            tot.count = ((lane[0].count + lane[64].count) + lane[128].count) + lane[192].count;
        };
        double pose[12];
        for (int i = 0; i < 12; ++i) pose[i] = poses0[12 * m + i];
        reg_iterate(pass, pose, lambda0, step_tol, max_passes, stats_out + 8 * m);
        for (int i = 0; i < 12; ++i) poses_out[12 * m + i] = pose[i];
    }
}
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    if KB.host_compiler() is None:
        pytest.skip("no C++ compiler")
    vp, dbl, i = C.c_void_p, C.c_double, C.c_int
    return KB.host_harness(_HOST_HARNESS, tmp_path_factory.mktemp("register_host"),
                           {"host_register": (None, [vp] * 6 + [i, i, dbl, dbl, dbl, i, vp, vp])})


def host_register(lib, c):
    objects, pool, index = np.ascontiguousarray(c["objects"]), np.ascontiguousarray(c["pool"], np.float32), np.ascontiguousarray(c["obj_index"], np.int32)
    poses0, points, ranges = np.ascontiguousarray(c["poses0"], np.float64), np.ascontiguousarray(c["points"], np.float64), np.ascontiguousarray(c["ranges"], np.int32)
    M = len(index)
    poses, stats = np.full((M, 12), 7.0), np.full((M, 8), 7.0)
    lib.host_register(objects.ctypes.data, pool.ctypes.data, index.ctypes.data, poses0.ctypes.data, points.ctypes.data, ranges.ctypes.data, M,
                      int(c["stride"]), float(c["trunc"]), float(c["lambda0"]), float(c["step_tol"]), int(c["max_passes"]), poses.ctypes.data,
                      stats.ctypes.data)
    return poses, stats


@pytest.mark.parametrize("name", RC.ALL + ["toy"])
def test_kernel_body_compiled_for_the_host_equals_the_specification(host_lib, name):
    """csrc/omg_register_body.h is the per-point pass, the 6 x 6 solve, the pose update and the accept / reject loop of
    k_register_clouds; compiled for the host without contraction, with the kernel's sum written as loops over 256 lanes, it gives
    the specification's poses and stats as int64 bits on every case of this file."""
    c, (poses, stats) = (RC.toy()["call"], RC.toy_spec()) if name == "toy" else (RC.call(name), RC.spec(name))
    got = host_register(host_lib, c)
    assert np.array_equal(_bits(got[0]), _bits(poses)) and np.array_equal(_bits(got[1]), _bits(stats)), name


def test_kernel_body_on_the_range_lengths_of_the_gpu_test(host_lib, reg):
    for K, stride in ((0, 1), (2, 3), (12, 1)):
        c = RC.lengths_call(K, stride)
        used = [len(range(b, e, stride)) for b, e in c["ranges"]]
        assert used == [0, 1, 5, 6, 63, 64, 65, 255, 256, 257, 513, 1025]
        poses, stats = reg.register_clouds(*RC.args(c))
        got = host_register(host_lib, c)
        assert np.array_equal(_bits(got[0]), _bits(poses)) and np.array_equal(_bits(got[1]), _bits(stats)), (K, stride)
        assert (stats[:3, reg.STATUS] == reg.FEW_INLIERS).all() and (stats[:3, reg.TRIALS] == 0).all()
        if K < 12:
            assert (stats[3:, reg.TRIALS] == K).all()


def test_fuzz_draws_without_a_gpu(host_lib, reg):
    """The generator of tests/fuzz/fuzz_register.py by the specification alone, and against the body compiled for the host: the
    draws reach short and empty ranges, aliased ranges, several strides and both ends of the loop."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_register", Path(__file__).resolve().parent / "fuzz" / "fuzz_register.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    rng = np.random.default_rng(20261)
    status, strides, aliased, instances = set(), set(), 0, 0
    for _ in range(12):
        c = fuzz.draw(rng)
        poses, stats = reg.register_clouds(*RC.args(c))
        got = host_register(host_lib, c)
        assert np.array_equal(_bits(got[0]), _bits(poses)) and np.array_equal(_bits(got[1]), _bits(stats))
        status |= set(stats[:, reg.STATUS].astype(int).tolist())
        strides.add(c["stride"])
        aliased += len(c["ranges"]) - len({tuple(r) for r in c["ranges"].tolist()})
        instances += len(poses)
    assert instances >= 40 and aliased >= 2 and len(strides) >= 2 and {0, reg.FEW_INLIERS, reg.CONVERGED} <= status, (instances, aliased, strides, status)


# ---------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_argument_checks_without_gpu(reg):
    """Every OMGX_ERR_INVALID case of omgx_register_clouds is decided on the host copies before any HIP call."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    assert lib.omgx_abi_version() == 14 and (reg.THREADS, reg.STATS) == (256, 8) and 30 <= reg.MAX_PASSES
    assert (reg.FEW_INLIERS, reg.SINGULAR, reg.LAMBDA_AT_MAX, reg.CONVERGED) == (1, 2, 4, 8)
    INV, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_OK
    d = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    rec0, pool0 = RC.table([RC.volume("box", (8, 9, 10), 0.03), RC.volume("sphere", (6, 6, 6), 0.04)], gaps=(2, 3))

    def call(rec=None, index=(0, 1, 1), ranges=((0, 10), (10, 10), (3, 50)), O=2, pool_elems=None, N=50, M=3, stride=1, trunc=0.03, lambda0=1e-3,
             step_tol=1e-6, K=30, host=(True, True, True), **ptr):
        rec = np.ascontiguousarray(rec0 if rec is None else rec)
        index, ranges = np.ascontiguousarray(index, np.int32), np.ascontiguousarray(ranges, np.int32)
        p = dict(objects=d, pool=d, d_index=d, poses0=d, points=d, d_ranges=d, poses=d, stats=d)
        p.update(ptr)
        h = [C.c_void_p(a.ctypes.data) if use else None for a, use in zip((rec, index, ranges), host)]
        return lib.omgx_register_clouds(p["objects"], h[0], O, p["pool"], len(pool0) if pool_elems is None else pool_elems, p["d_index"], h[1],
                                        p["poses0"], p["points"], N, p["d_ranges"], h[2], M, stride, trunc, lambda0, step_tol, K, p["poses"],
                                        p["stats"], None)

    for k in ("objects", "pool", "d_index", "poses0", "points", "d_ranges", "poses", "stats"):
        assert call(**{k: None}) == INV, k
    for k in range(3):
        assert call(host=tuple(j != k for j in range(3))) == INV, k
    assert call(O=-1) == INV and call(pool_elems=-1) == INV and call(N=-1) == INV and call(M=-1) == INV
    assert call(stride=0) == INV and call(stride=-2) == INV
    assert call(K=-1) == INV and call(K=reg.MAX_PASSES + 1) == INV
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(trunc=bad) == INV and call(lambda0=bad) == INV, bad
    for bad in ((0, 2, 1), (-1, 0, 0), (0, 1, 7)):
        assert call(index=bad) == INV, bad
    assert call(index=(0, 1, 1), O=1) == INV
    for bad in ((-1, 4), (0, 51), (5, 4), (51, 51), (-3, -2)):
        assert call(ranges=((0, 10), bad, (3, 50))) == INV, bad
    for axis in range(3):
        for dim in (1, 0, -4):
            r = rec0.copy()
            r["dim"][1][axis] = dim
            assert call(rec=r) == INV, (axis, dim)
    r = rec0.copy()
    r["grid_offset"][1] += 1                                   # the last voxel leaves the pool
    assert call(rec=r) == INV
    r["grid_offset"][1] = -1
    assert call(rec=r) == INV
    assert call(pool_elems=len(pool0) - 1) == INV
    r = rec0.copy()
    r["dim"][0] = (1 << 30, 1 << 30, 1 << 30)                  # a product beyond int64
    assert call(rec=r) == INV
    # nothing to do: no instance (everything per instance may then be NULL), and nothing is launched
    assert call(M=0) == OK
    assert call(M=0, N=0, objects=None, pool=None, d_index=None, poses0=None, points=None, d_ranges=None, poses=None, stats=None,
                host=(False, False, False)) == OK


def test_wrapper_checks_without_gpu(reg):
    """Every argument error of part 2 that ops.register_clouds can see itself (the scalars, the object indices, the ranges, the
    shapes) raises through the wrapper on a table held in host memory, before anything asks where a tensor lies; with valid
    arguments the first complaint is that the tensors are not on a device.  (Null pointers and negative sizes cannot be
    expressed through the wrapper; a record with a bad grid is the C ABI's to refuse: test_gpu_register.py.)  The specification
    refuses the same arguments with ValueError."""
    import torch
    from omg_planner_amd import _lib, ops, scenes as S
    E = _lib.OmgHipError
    scene = S.Scene([S.SceneObject("a", np.eye(4), RC.volume("box", (8, 9, 10), 0.03)), S.SceneObject("b", np.eye(4), RC.volume("sphere", (6, 6, 6), 0.04))], 0)
    ds = ops.DeviceScenes(S.pack_table([scene, scene], tight=False), device="cpu")
    pts, p0 = torch.zeros((20, 3), dtype=torch.float64), torch.zeros((2, 12), dtype=torch.float64)
    pairs, ranges = [(0, 1), (1, 0)], [(0, 10), (10, 20)]
    wrap = lambda pairs=pairs, p0=p0, pts=pts, ranges=ranges, **kw: ops.register_clouds(ds, pairs, p0, pts, ranges, **kw)
    with pytest.raises(E, match="device tensor"):
        wrap()
    with pytest.raises(E, match="device tensor"):
        wrap(ranges=[(0, 0), (20, 20)], stride=7, max_passes=0, trunc=1e-9, lambda0=1e300)     # the edges of what is valid
    for kw in (dict(stride=0), dict(stride=-3), dict(max_passes=-1), dict(max_passes=reg.MAX_PASSES + 1)):
        with pytest.raises(E, match="stride must be"):
            wrap(**kw)
    for name in ("trunc", "lambda0"):
        for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
            with pytest.raises(E, match="finite and positive"):
                wrap(**{name: bad})
    for bad in ([(0, 2), (1, 0)], [(2, 0), (1, 0)], [(0, -1), (1, 0)], [(0, 1), (-1, 0)]):
        with pytest.raises(IndexError):
            wrap(pairs=bad)
    for bad in (ranges[:1], ranges + [(0, 1)], []):
        with pytest.raises(E, match="ranges must be"):
            wrap(ranges=bad)
    for bad in ((-1, 4), (0, 21), (5, 4), (21, 21), (-3, -2), (0, 1 << 32), (1 << 32, (1 << 32) + 1), (-(1 << 32), 3)):   # the last three would wrap as int32
        with pytest.raises(E, match="a range is outside"):
            wrap(ranges=[(0, 10), bad])
    for bad in (pts.numpy(), torch.zeros((20, 4), dtype=torch.float64), torch.zeros(60, dtype=torch.float64), torch.zeros((2, 10, 3), dtype=torch.float64)):
        with pytest.raises(E, match="points must be a tensor"):
            wrap(pts=bad)
    for bad in (torch.zeros((3, 12), dtype=torch.float64), torch.zeros((2, 16), dtype=torch.float64), torch.zeros(24, dtype=torch.float64),
                np.zeros((2, 3, 4)), np.zeros((1, 12))):
        with pytest.raises(E, match="poses0 must be"):
            wrap(p0=bad)
    # the specification refuses the same
    spec = lambda index=(1, 2), ranges=ranges, pool=4000, **kw: reg.register_clouds(ds.host_objects, np.zeros(pool, np.float32), index, p0.numpy(),
                                                                                    pts.numpy(), ranges, **kw)
    for kw in (dict(stride=0), dict(max_passes=-1), dict(max_passes=reg.MAX_PASSES + 1)):
        with pytest.raises(ValueError):
            spec(**kw)
    for kw in (dict(trunc=0.0), dict(trunc=np.nan), dict(lambda0=-1.0), dict(lambda0=np.inf)):
        with pytest.raises(ValueError, match="finite"):
            spec(**kw)
    with pytest.raises(ValueError, match="index"):
        spec(index=(1, 4))
    with pytest.raises(ValueError, match="range"):
        spec(ranges=[(0, 10), (12, 11)])
    with pytest.raises(ValueError, match="pool"):
        spec(pool=100)


def test_set_object_poses_equals_set_object_pose_on_the_host(reg):
    """The batched form against one call per object on a table held in host memory: the record bytes and the host mirror."""
    import torch
    from omg_planner_amd import ops, scenes as S
    scenes = [S.make_tabletop_scene(s, num_objects=3, grid=8, table_grid=(8, 8, 4)) for s in range(3)]
    batch = S.pack_table(scenes, tight=False)
    one, many = ops.DeviceScenes(batch, device="cpu"), ops.DeviceScenes(batch, device="cpu")
    rng = np.random.default_rng(3)
    pairs = [(2, 1), (0, 0), (1, 3), (2, 0)]
    poses = np.stack([RC.random_pose(rng) for _ in pairs])
    for (s, o), P in zip(pairs, poses):
        one.set_object_pose(s, o, P)
    before = many.objects.clone()
    many.set_object_poses(pairs, poses)
    assert torch.equal(many.objects, one.objects) and not torch.equal(many.objects, before)
    assert many.host_objects.tobytes() == one.host_objects.tobytes()
    many.set_object_poses(np.zeros((0, 2), int), np.zeros((0, 4, 4)))
    assert torch.equal(many.objects, one.objects)
    with pytest.raises(ValueError, match="twice"):
        many.set_object_poses([(0, 0), (0, 0)], poses[:2])
    with pytest.raises(ValueError, match="poses"):
        many.set_object_poses(pairs, poses[:3])
    with pytest.raises(IndexError):
        many.set_object_poses([(0, 9)], poses[:1])
    rows = reg.pose_rows(poses)
    assert np.array_equal(reg.pose_mats(rows), poses) and rows.shape == (4, 12)


# ---------------------------------------------------------------------------------------------------------------------
# registers
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_register_kernel_does_not_spill(tmp_path):
    """The compiler's resource remarks for csrc/omg_register.hip: k_register_clouds keeps a lane's 28 partials, two sets of totals
    and two poses in registers, without scratch; its LDS is the two slots of four wave totals."""
    v = KB.one(KB.kernel_resources("omg_register.hip", tmp_path), "k_register_clouds")
    print(v)
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
    assert v["Occupancy [waves/SIMD]"] >= 1 and v["LDS Size [bytes/block]"] == 2 * 4 * (28 * 8 + 4), v
