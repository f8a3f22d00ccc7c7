"""CPU tests of depth conditioning (omg-planner_amd/sensor.py, csrc/omg_sensor.hip): the specification at
its edges as answers worked out by hand; csrc/omg_sensor_body.h compiled for the host equals the specification bit for bit; the
kernels' resources; every argument error of the specification, of the C ABI and of the wrappers; and the effect on the sphere
scene seen through a simulated sensor."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import kernel_build as KB
from tests import sensor_cases as SC

INF, NAN = SC.INF, SC.NAN
ONE = np.array([1.0])


def _condition(frames, R=0, table=ONE, min_support=0, tau=(0.5, 0.0, 0.0), scale=0.001, z_min=1.0, z_max=4.0, range_scale=1.0):
    from omg_planner_amd import sensor
    return sensor.condition_depth(np.asarray(frames)[None], scale, z_min, z_max, tau, min_support, R, table, range_scale)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the specification at its edges
# ---------------------------------------------------------------------------------------------------------------------
def test_returns_as_known_answers():
    """z_min = 1 and z_max = 4, both inclusive; uint16 at a scale of 2^-10 (exact), so that raw 1024 is z = 1 and 4096 is z = 4."""
    from omg_planner_amd import sensor
    s = 2.0 ** -10
    depth, flags = _condition(np.array([[2048]], np.uint16), scale=s)  # a 1 x 1 image: R = 0 returns z itself
    assert depth.tolist() == [[[2.0]]] and flags.tolist() == [[[sensor.KEPT]]] and depth.dtype == np.float64 and flags.dtype == np.uint8
    depth, flags = _condition(np.array([[0, 1023, 1024, 4096, 4097, 65535]], np.uint16), scale=s)
    assert depth.tolist() == [[[0.0, 0.0, 1.0, 4.0, 0.0, 0.0]]] and flags.tolist() == [[[1, 1, 0, 0, 1, 1]]]
    f = np.array([[NAN, INF, -INF, -2.0, 0.0, -0.0, 1.0, 4.0, np.nextafter(1.0, 0.0), np.nextafter(4.0, 5.0), 2.5]])
    depth, flags = _condition(f)
    assert depth.tolist() == [[[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 4.0, 0.0, 0.0, 2.5]]] and flags.tolist() == [[[1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0]]]
    # R = 0 returns the input's own bits, whatever the table's weight
    z = np.array([[1.0 + 2.0 ** -52, np.pi, 3.999999999999999]])
    assert _condition(z, table=np.array([0.3]))[0].tobytes() == z[None].tobytes()
    # V = 0: empty outputs
    depth, flags = sensor.condition_depth(np.zeros((0, 4, 5), np.uint16), s, 1.0, 4.0, (0.5, 0.0, 0.0), 3, 0, ONE, 1.0)
    assert depth.shape == (0, 4, 5) and flags.shape == (0, 4, 5)


def test_flying_pixels_and_support_as_known_answers():
    from omg_planner_amd import sensor
    K, F = sensor.KEPT, sensor.FLYING
    # a lone pixel at 2.5 between a plane at 2 (left) and a plane at 3 (right), tau = 0.25: nothing is near it
    f = np.tile([2.0, 2.0, 2.0, 3.0, 3.0, 3.0], (5, 1))
    f[2, 2] = 2.5
    depth, flags = _condition(f, min_support=3, tau=(0.25, 0.0, 0.0))
    assert flags[0, 2, 2] == F and depth[0, 2, 2] == 0.0 and (np.delete(flags.ravel(), 14) == K).all()
    depth, flags = _condition(f, min_support=0, tau=(0.25, 0.0, 0.0))
    assert (flags == K).all() and depth[0, 2, 2] == 2.5
    # |d| <= tau is inclusive: at tau = 0.5 the lone pixel has all 8 neighbours
    assert (_condition(f, min_support=8, tau=(0.5, 0.0, 0.0))[1][0, 2, 2]) == K
    # the noise scale grows with range and belongs to the pixel asked about: tau = (0 + 0*z) + 0.0625*z*z is 0.25 at z = 2,
    # 0.390625 at 2.5 and 0.5625 at 3; the steps are 0.5: only the pixel at 3 finds its neighbour near
    g = np.array([[2.0, 2.5, 3.0]])
    assert _condition(g, min_support=1, tau=(0.0, 0.0, 0.0625))[1].tolist() == [[[F, F, K]]]
    # a corner has 3 neighbours, an edge 5: what lies outside the image is no support
    flat = np.full((3, 3), 2.0)
    assert _condition(flat, min_support=3)[1].tolist() == [[[K] * 3] * 3]
    assert _condition(flat, min_support=4)[1].tolist() == [[[F, K, F], [K, K, K], [F, K, F]]]
    assert _condition(flat, min_support=6)[1].tolist() == [[[F, F, F], [F, K, F], [F, F, F]]]
    # a flying pixel still supports its neighbours (it has a return), but takes no part in the filter
    h = np.array([[2.0, 2.0, 2.25]])
    depth, flags = _condition(h, R=1, table=np.ones(9), min_support=2, tau=(0.25, 0.0, 0.0), range_scale=4.0)
    assert flags.tolist() == [[[F, K, F]]] and depth.tolist() == [[[0.0, 2.0, 0.0]]]


def test_biweight_as_known_answers():
    """A 3 x 3 step: the left two columns at 2, the right one at 3; rho = range_scale * tau = 1 * 1: across the step x = 1, u = 0
    and the weight is exactly nothing, so the centre's value is the mean of six equal values: 2, whatever the table."""
    from omg_planner_amd import sensor
    f = np.array([[2.0, 2.0, 3.0]] * 3)
    tab = np.arange(1.0, 10.0)
    depth, flags = _condition(f, R=1, table=tab, tau=(1.0, 0.0, 0.0))
    assert (flags == sensor.KEPT).all() and depth[0].tolist() == [[2.0, 2.0, 3.0]] * 3
    # half a step: the right column at 2.5, x = 0.5, u = 0.75, w_r = 0.5625; the centre with a table of ones:
    # num = 6 * 2 + 3 * 0.5625 * 2.5, den = 6 + 3 * 0.5625, in row-major order; every term is exact in binary
    g = np.array([[2.0, 2.0, 2.5]] * 3)
    depth, _ = _condition(g, R=1, table=np.ones(9), tau=(1.0, 0.0, 0.0))
    num = den = 0.0
    for row in range(3):
        for zq, w in ((2.0, 1.0), (2.0, 1.0), (2.5, 0.5625)):
            num, den = num + w * zq, den + w
    assert depth[0, 1, 1] == num / den == 16.21875 / 7.6875
    # the table is applied in row-major order, not transposed: weight only on the tap to the right (dr = 0, dc = +1) and the centre
    tab = np.zeros(9)
    tab[4], tab[5] = 1.0, 2.0
    h = np.array([[2.0, 2.0, 2.0], [2.0, 2.0, 2.5], [2.0, 2.0, 2.0]])
    depth, _ = _condition(h, R=1, table=tab, tau=(1.0, 0.0, 0.0))
    assert depth[0, 1, 1] == (2.0 + 2.0 * 0.5625 * 2.5) / (1.0 + 2.0 * 0.5625)
    # tau = 0 everywhere: rho = 0, the centre's own x is 0 / 0; the value falls back to z itself
    depth, flags = _condition(h, R=1, table=np.ones(9), tau=(0.0, 0.0, 0.0))
    assert depth[0].tolist() == h.tolist() and (flags == sensor.KEPT).all()


def _normals(depth, k=(2.0, 2.0, 1.0, 1.0), tau=(0.5, 0.0, 0.0), cos_min=0.0, flags=None):
    from omg_planner_amd import sensor
    depth = np.asarray(depth, np.float64)[None]
    return sensor.depth_normals(depth, [k], tau, cos_min, None if flags is None else np.asarray(flags, np.uint8)[None])


def test_normals_as_known_answers():
    from omg_planner_amd import sensor
    K, NN, G = sensor.KEPT, sensor.KEPT | sensor.NO_NORMAL, sensor.GRAZING
    # a fronto-parallel plane at z = 2, fx = fy = 2, cx = cy = 1: P = ((c - 1), (r - 1), 2); a = (2, 0, 0), b = (0, 2, 0) in the middle,
    # m = (0, 0, 4), s = 8 > 0: n = (0, 0, -1): towards the camera; cos = z / |P|
    n, d, f, cs = _normals(np.full((3, 3), 2.0))
    assert (f == K).all() and d.tolist() == [[[2.0] * 3] * 3]
    assert n.reshape(-1, 3).tolist() == [[-0.0, -0.0, -1.0]] * 9 or np.array_equal(n.reshape(-1, 3), np.tile([0.0, 0.0, -1.0], (9, 1)))
    r, c = np.meshgrid(np.arange(3.0), np.arange(3.0), indexing="ij")
    assert np.array_equal(cs[0], 2.0 / np.sqrt(((c - 1.0) * (c - 1.0) + (r - 1.0) * (r - 1.0)) + 4.0)) and cs[0, 1, 1] == 1.0
    # a one-sided difference at a depth step: the right column at 4 is not usable from the middle one (and the other way round)
    step = np.array([[2.0, 2.0, 4.0]] * 3)
    n, d, f, cs = _normals(step)
    assert (f == np.array([[K, K, NN]] * 3)).all()  # the right column has no horizontal neighbour at all
    assert np.array_equal(n[0, 1, 1], [0.0, 0.0, -1.0]) or n[0, 1, 1].tolist() == [-0.0, -0.0, -1.0]  # a = P(p) - P(left) = (1, 0, 0)
    assert n[0, :, 2].tolist() == [[0.0] * 3] * 3 and cs[0, :, 2].tolist() == [0.0] * 3 and d[0, :, 2].tolist() == [4.0] * 3
    # a plane tilted about the vertical axis: every row is (1, 4, 5), tau = 3.  Middle pixel: P = (0, 0, 4), P(left) = (-0.5, 0, 1),
    # P(right) = (2.5, 0, 5): a = (3, 0, 4); P(up) = (0, -2, 4), P(down) = (0, 2, 4): b = (0, 4, 0)
    # m = (0*0 - 4*4, 4*0 - 3*0, 3*4 - 0*0) = (-16, 0, 12), s = 48 > 0: m = (16, -0, -12), nn = 400, n = (0.8, -0, -0.6), cos = 2.4 / 4
    tilt = np.array([[1.0, 4.0, 5.0]] * 3)
    n, d, f, cs = _normals(tilt, tau=(3.0, 0.0, 0.0))
    assert n[0, 1, 1].tolist() == [0.8, 0.0, -0.6] and cs[0, 1, 1] == 0.6 and f[0, 1, 1] == K
    # grazing is decided by cos < cos_min exactly: at cos_min = 0.6 the pixel stays, one step above it goes
    assert _normals(tilt, tau=(3.0, 0.0, 0.0), cos_min=0.6)[2][0, 1, 1] == K
    n, d, f, cs = _normals(tilt, tau=(3.0, 0.0, 0.0), cos_min=np.nextafter(0.6, 1.0))
    assert f[0, 1, 1] == G and d[0, 1, 1] == 0.0 and n[0, 1, 1].tolist() == [0.0] * 3 and cs[0, 1, 1] == 0.0
    # no horizontal neighbour at all (a single column): kept, without a normal
    assert _normals(np.full((3, 1), 2.0), k=(2.0, 2.0, 0.0, 1.0))[2].tolist() == [[[NN], [NN], [NN]]]
    # s == 0 and nn == 0: focal lengths of 1e200 make a = (2e-200, 0, 0) and b = (0, 2e-200, 0); their product underflows, m = 0
    flat = np.full((3, 3), 2.0)
    n, d, f, cs = _normals(flat, k=(1e200, 1e200, 1.0, 1.0))
    assert f[0, 1, 1] == NN and d[0, 1, 1] == 2.0 and n[0, 1, 1].tolist() == [0.0] * 3 and cs[0, 1, 1] == 0.0  # kept, without a normal
    # nothing there: 0, NaN, negative and +inf's conditioned form (0.0); the flag that came in is kept, 0 becomes NO_RETURN
    holes = np.array([[0.0, NAN, -1.0], [2.0, 2.0, 2.0], [2.0, 2.0, 2.0]])
    n, d, f, cs = _normals(holes, flags=[[0, sensor.FLYING, sensor.NO_RETURN], [0, 0, 0], [0, 0, 0]])
    assert f[0, 0].tolist() == [sensor.NO_RETURN, sensor.FLYING, sensor.NO_RETURN] and d[0, 0].tolist() == [0.0] * 3
    assert f[0, 1].tolist() == [K] * 3  # one-sided downwards
    assert _normals(flat[:1, :1])[2].tolist() == [[[NN]]]  # a 1 x 1 image


# ---------------------------------------------------------------------------------------------------------------------
# 2. csrc/omg_sensor_body.h on the host
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include <vector>
#include "omg_sensor_body.h"
// One image as ONE staged tile with a halo of R + 1, in the kernel's three steps: stage the returns, test the halo-R region, mask,
// filter.  (The kernel does the same per 16 x 16 tile at the pitch SENSOR_PITCH; here the pitch is W + 2 (R + 1).)
extern "C" void host_condition(const void* in, int kind, double scale, int V, int H, int W, double z_min, double z_max, double t0, double t1,
                               double t2, int min_support, int R, const double* table, double range_scale, double* depth_out, uint8_t* flags) {
    const int halo = R + 1, pitch = W + 2 * halo, rows = H + 2 * halo;
    std::vector<double> z((size_t)pitch * rows), zs((size_t)pitch * rows);
    for (int v = 0; v < V; ++v) {
        const int64_t image = (int64_t)v * H * W;
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < pitch; ++x) {
                const int r = y - halo, c = x - halo;
                z[y * pitch + x] = r >= 0 && r < H && c >= 0 && c < W ? sensor_depth(in, kind, image + (int64_t)r * W + c, scale, z_min, z_max) : 0.0;
            }
        zs = z;
        for (int y = 1; y < rows - 1; ++y)
            for (int x = 1; x < pitch - 1; ++x)
                if (!sensor_survives(z.data(), pitch, y * pitch + x, t0, t1, t2, min_support)) zs[y * pitch + x] = 0.0;
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const int own = (r + halo) * pitch + c + halo;
                const bool kept = zs[own] > 0.0;
                depth_out[image + (int64_t)r * W + c] = kept ? sensor_filter(zs.data(), pitch, own, R, table, range_scale, t0, t1, t2) : 0.0;
                flags[image + (int64_t)r * W + c] = kept ? OMGX_SENSOR_KEPT : z[own] > 0.0 ? OMGX_SENSOR_FLYING : OMGX_SENSOR_NO_RETURN;
            }
    }
}
// staged != 0: every pixel through a tile of 3 x 3 around it at the pitch SENSOR_PITCH, as the kernel reads its staged tile;
// staged == 0: straight from the image, as the measurement variant reads.
extern "C" void host_normals(const double* depth, const uint8_t* flags_in, const double* k, int V, int H, int W, double t0, double t1, double t2,
                             double cos_min, int staged, double* normals, double* depth_out, uint8_t* flags_out, double* cosine) {
    for (int v = 0; v < V; ++v)
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const int64_t image = (int64_t)v * H * W, at = image + (int64_t)r * W + c;
                double tile[3 * SENSOR_PITCH];
                for (int y = 0; y < 3; ++y)
                    for (int x = 0; x < 3; ++x) {
                        const int rr = r - 1 + y, cc = c - 1 + x;
                        tile[y * SENSOR_PITCH + x] = rr >= 0 && rr < H && cc >= 0 && cc < W ? depth[image + (int64_t)rr * W + cc] : 0.0;
                    }
                const uint8_t f = flags_in ? flags_in[at] : (uint8_t)0;
                flags_out[at] = staged ? sensor_normal(tile, -((int64_t)(r - 1) * SENSOR_PITCH + (c - 1)), SENSOR_PITCH, H, W, r, c, k + 4 * v, t0, t1,
                                                       t2, cos_min, f, normals + at * 3, cosine + at, depth_out + at)
                                       : sensor_normal(depth + image, 0, W, H, W, r, c, k + 4 * v, t0, t1, t2, cos_min, f, normals + at * 3,
                                                       cosine + at, depth_out + at);
            }
}
extern "C" int host_lds_bytes(void) { return SENSOR_LDS_BYTES; }
"""


def _host_lib(tmp_path):
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    return KB.host_harness(_HOST_HARNESS, tmp_path, {"host_condition": (None, [vp, i, d, i, i, i, d, d, d, d, d, i, i, vp, d, vp, vp]),
                                                     "host_normals": (None, [vp, vp, vp, i, i, i, d, d, d, d, i, vp, vp, vp, vp]),
                                                     "host_lds_bytes": (i, [])})


def host_condition(lib, frames, scale, z_min, z_max, tau, min_support, R, table, range_scale):
    frames, table = np.ascontiguousarray(frames), np.ascontiguousarray(table, np.float64)
    V, H, W = frames.shape
    depth, flags = np.full((V, H, W), -7.0), np.full((V, H, W), 99, np.uint8)
    lib.host_condition(frames.ctypes.data, 0 if frames.dtype == np.uint16 else 1, scale, V, H, W, z_min, z_max, *tau, min_support, R, table.ctypes.data,
                       range_scale, depth.ctypes.data, flags.ctypes.data)
    return depth, flags


def host_normals(lib, depth, flags, k, tau, cos_min, staged=0):
    depth, k = np.ascontiguousarray(depth, np.float64), np.ascontiguousarray(k, np.float64)
    V, H, W = depth.shape
    out = np.full((V, H, W, 3), -7.0), np.full((V, H, W), -7.0), np.full((V, H, W), 99, np.uint8), np.full((V, H, W), -7.0)
    lib.host_normals(depth.ctypes.data, None if flags is None else np.ascontiguousarray(flags).ctypes.data, k.ctypes.data, V, H, W, *tau, cos_min,
                     staged, *(o.ctypes.data for o in out))
    return out


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@KB.requires_host_cxx
def test_kernel_body_compiled_for_the_host_equals_the_specification(tmp_path):
    """csrc/omg_sensor_body.h is what a thread of the two kernels does for its pixel; compiled for the host without contraction it
    gives the specification's bits on every shape, radius and input kind of sensor_cases (V = 3 with three intrinsics, a table
    that is not symmetric), read straight or through a staged tile; and on the fuzz generator's draws."""
    lib = _host_lib(tmp_path)
    seen = set()
    for H, W in SC.SHAPES:
        for R in SC.RADII:
            for kind in SC.KINDS:
                c = SC.bit_case(H, W, R, kind)
                depth, flags = host_condition(lib, c["frames"], SC.SCALE, SC.Z_MIN, SC.Z_MAX, SC.TAU, SC.MIN_SUPPORT, R, c["table"], SC.RANGE_SCALE)
                assert _same(depth, c["depth"]) and _same(flags, c["flags"]), (H, W, R, kind)
                for staged in (0, 1):
                    got = host_normals(lib, depth, flags, SC.INTRINSICS, SC.TAU, SC.COS_MIN, staged)
                    for g, name in zip(got, ("normals", "depth2", "flags2", "cosine")):
                        assert _same(g, c[name]), (H, W, R, kind, staged, name)
                seen |= set(np.unique(c["flags2"]).tolist())
                if R and H > 1:  # the filter does something, and a transposed table would do something else
                    kept = c["flags"] == 0
                    raw = c["frames"].astype(np.float64) * (SC.SCALE if kind == "uint16" else 1.0)
                    assert (c["depth"][kept] != raw[kept]).any()
                    side = 2 * R + 1
                    other = host_condition(lib, c["frames"], SC.SCALE, SC.Z_MIN, SC.Z_MAX, SC.TAU, SC.MIN_SUPPORT, R,
                                           c["table"].reshape(side, side).T.copy(), SC.RANGE_SCALE)[0]
                    assert not _same(other, c["depth"]), (H, W, R, kind)
    assert seen == {0, 1, 2, 3, 8}  # every flag occurs
    rng = np.random.default_rng(SC.FUZZ_SEED)
    for _ in range(SC.FUZZ_TRIALS):
        c = SC.draw(rng)
        want = SC.specification(c)
        depth, flags = host_condition(lib, c["frames"], c["scale"], c["z_min"], c["z_max"], c["tau"], c["min_support"], c["radius"], c["table"],
                                      c["range_scale"])
        got = (depth, flags) + host_normals(lib, depth, flags, c["intrinsics"], c["tau"], c["cos_min"])
        assert all(_same(g, w) for g, w in zip(got, want)), (c["frames"].shape, c["radius"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. resources
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_sensor_kernels_use_no_scratch_and_the_computed_lds(tmp_path):
    """The compiler's resource remarks for csrc/omg_sensor.hip: no scratch, no spills; k_depth_condition holds the staged tile, 32
    rows (16 + 2 * (7 + 1)) at a pitch of 48 doubles = 12 288 bytes, k_depth_normals its tile with a halo of 1: 18 rows at the same
    pitch = 6 912 bytes."""
    from omg_planner_amd import _lib
    seen = KB.kernel_resources("omg_sensor.hip", tmp_path)
    assert len(seen) == 2
    side = 16 + 2 * (_lib.CONSTANTS["OMGX_SENSOR_MAX_RADIUS"] + 1)
    for part, lds in (("k_depth_condition", side * 48 * 8), ("k_depth_normals", 18 * 48 * 8)):
        v = KB.one(seen, part)
        print(part, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (part, v)
        assert v["LDS Size [bytes/block]"] == lds, (part, v)
    assert side * 48 * 8 == 12288


@KB.requires_host_cxx
def test_the_headers_lds_figure_is_the_computed_one(tmp_path):
    assert _host_lib(tmp_path).host_lds_bytes() == 12288


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_specification_argument_errors():
    from omg_planner_amd import sensor
    good = dict(frames=np.full((1, 3, 3), 2000, np.uint16), scale=0.001, z_min=0.5, z_max=4.0, tau=(0.01, 0.0, 0.0), min_support=3, radius=1,
                table=np.ones(9), range_scale=2.0)
    sensor.condition_depth(**good)
    zero_centre, negative, nan_w = np.ones(9), np.ones(9), np.ones(9)
    zero_centre[4], negative[0], nan_w[8] = 0.0, -0.5, NAN
    for change in (dict(radius=8, table=np.ones(17 * 17)), dict(radius=-1), dict(table=zero_centre), dict(table=negative), dict(table=nan_w),
                   dict(table=np.ones(25)), dict(scale=NAN), dict(scale=0.0), dict(scale=-0.001), dict(z_min=NAN), dict(z_min=0.0), dict(z_min=-1.0),
                   dict(z_max=INF), dict(z_min=4.5), dict(range_scale=0.0), dict(range_scale=NAN), dict(tau=(NAN, 0.0, 0.0)), dict(tau=(0.0, INF, 0.0)),
                   dict(tau=(0.0, 0.0, -0.1)), dict(tau=(0.0, 0.0)), dict(min_support=-1), dict(min_support=9),
                   dict(frames=np.zeros((3, 3), np.uint16)), dict(frames=np.zeros((1, 3, 3), np.float32)), dict(frames=np.zeros((1, 0, 3)))):
        with pytest.raises(ValueError):
            sensor.condition_depth(**{**good, **change})
    ok = dict(depth=np.full((2, 3, 3), 2.0), intrinsics=[(2.0, 2.0, 1.0, 1.0)] * 2, tau=(0.01, 0.0, 0.0), cos_min=0.1)
    sensor.depth_normals(**ok)
    for change in (dict(intrinsics=[(2.0, 2.0, 1.0, 1.0)]), dict(intrinsics=[(0.0, 2.0, 1.0, 1.0)] * 2), dict(intrinsics=[(2.0, 2.0, NAN, 1.0)] * 2),
                   dict(cos_min=NAN), dict(tau=(-1.0, 0.0, 0.0)), dict(depth=np.zeros((3, 3))), dict(depth=np.zeros((2, 3, 3), np.float32)),
                   dict(flags=np.zeros((2, 3, 3))), dict(flags=np.zeros((1, 3, 3), np.uint8)), dict(depth=np.zeros((2, 3, 0)))):
        with pytest.raises(ValueError):
            sensor.depth_normals(**{**ok, **change})
    for bad in (dict(radius=8, sigma=1.0), dict(radius=1, sigma=0.0), dict(radius=1, sigma=NAN)):
        with pytest.raises(ValueError):
            sensor.gaussian_table(**bad)
    g = sensor.gaussian_table(2, 1.5)
    assert g.shape == (25,) and g[12] == 1.0 and g[0] == g[24] == np.exp(-8.0 / 4.5) and np.array_equal(g.reshape(5, 5), g.reshape(5, 5).T)


def test_c_abi_argument_checks_without_gpu():
    """Every OMGX_ERR_INVALID / OMGX_ERR_UNSUPPORTED case of the two entry points is decided on the host before any HIP call: the
    device pointers below are never dereferenced."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    assert lib.omgx_abi_version() == 14 and len(_lib.STRUCTS) == 8 and _lib.CONSTANTS["OMGX_SENSOR_MAX_RADIUS"] == 7
    INV, UNS, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED, _lib.OMGX_OK
    d, far = C.c_void_p(1 << 20), C.c_void_p(1 << 40)

    def cond(kind=0, scale=0.001, V=2, H=4, W=5, z_min=0.5, z_max=4.0, tau=(0.01, 0.0, 0.01), support=3, R=1, tab=None, rs=2.0, **ptr):
        tab = np.ones((2 * max(R, 0) + 1) ** 2) if tab is None else np.ascontiguousarray(tab, np.float64)
        p = dict(depth_in=d, table=d, h_table=C.c_void_p(tab.ctypes.data), depth_out=far, flags=far)
        p.update(ptr)
        return lib.omgx_depth_condition(p["depth_in"], kind, scale, V, H, W, z_min, z_max, *tau, support, R, p["table"], p["h_table"], rs,
                                        p["depth_out"], p["flags"], None)

    for k in ("depth_in", "table", "h_table", "depth_out", "flags"):
        assert cond(**{k: None}) == INV, k
    assert cond(V=0) == OK and cond(V=0, depth_in=None, depth_out=None, flags=None) == OK
    assert cond(V=-1) == INV and cond(H=0) == INV and cond(W=0) == INV and cond(kind=2) == INV and cond(kind=-1) == INV
    for bad in (NAN, INF, -INF, 0.0, -1.0):
        assert cond(scale=bad) == INV and cond(z_min=bad) == INV and cond(rs=bad) == INV, bad
    for bad in (NAN, INF, 0.25):  # (0.25: z_min > z_max)
        assert cond(z_max=bad) == INV, bad
    assert cond(z_min=2.0, z_max=2.0) != INV
    for i in range(3):
        for bad in (NAN, INF, -0.001):
            tau = [0.01, 0.0, 0.01]
            tau[i] = bad
            assert cond(tau=tau) == INV, (i, bad)
    assert cond(support=-1) == INV and cond(support=9) == INV and cond(R=-1) == INV
    for at, bad in ((4, 0.0), (0, -0.5), (8, NAN), (3, INF)):
        tab = np.ones(9)
        tab[at] = bad
        assert cond(tab=tab) == INV, (at, bad)
    assert cond(R=8, tab=np.ones(17 * 17)) == UNS and cond(R=8, tab=np.ones(17 * 17), scale=NAN) == INV  # limits after every invalid argument
    assert cond(V=65536, H=1, W=1) == UNS and cond(V=1, H=1 << 16, W=1 << 16) == UNS and cond(V=40000, H=300, W=300) == UNS
    # depth_out may not share a byte with the frames (2 x 4 x 5 pixels: 40 uint16 = 80 bytes, or 320 bytes of doubles)
    base = 1 << 20
    assert cond(depth_out=d) == INV and cond(depth_out=C.c_void_p(base + 72)) == INV and cond(depth_out=C.c_void_p(base + 80)) != INV
    assert cond(kind=1, depth_out=C.c_void_p(base + 312)) == INV and cond(kind=1, depth_out=C.c_void_p(base - 312)) == INV
    assert cond(kind=1, depth_out=C.c_void_p(base + 320)) != INV

    def norm(V=2, H=4, W=5, tau=(0.01, 0.0, 0.01), cos_min=0.1, k=None, **ptr):
        k = np.ascontiguousarray(np.tile((50.0, 50.0, 2.0, 2.0), (max(V, 1), 1)) if k is None else k, np.float64)
        p = dict(depth_in=d, flags_in=d, intrinsics=d, h_intrinsics=C.c_void_p(k.ctypes.data), normals=far, depth_out=C.c_void_p(1 << 41),
                 flags_out=d, cosine=C.c_void_p(1 << 42))
        p.update(ptr)
        return lib.omgx_depth_normals(p["depth_in"], p["flags_in"], p["intrinsics"], p["h_intrinsics"], V, H, W, *tau, cos_min, p["normals"],
                                      p["depth_out"], p["flags_out"], p["cosine"], None)

    for k in ("depth_in", "intrinsics", "h_intrinsics", "normals", "depth_out", "flags_out"):
        assert norm(**{k: None}) == INV, k
    assert norm(V=0) == OK and norm(V=0, depth_in=None, intrinsics=None, h_intrinsics=None, normals=None, depth_out=None, flags_out=None) == OK
    assert norm(V=-1) == INV and norm(H=0) == INV and norm(W=0) == INV
    for bad in (NAN, INF, -INF):
        assert norm(cos_min=bad) == INV and norm(tau=(bad, 0.0, 0.0)) == INV
    assert norm(tau=(0.0, -1.0, 0.0)) == INV
    for col in range(4):
        for bad in (NAN, INF) + ((0.0,) if col < 2 else ()):
            k = np.tile((50.0, 50.0, 2.0, 2.0), (2, 1))
            k[1, col] = bad
            assert norm(k=k) == INV, (col, bad)
    assert norm(depth_out=d) == INV and norm(normals=C.c_void_p(base + 8)) == INV and norm(cosine=C.c_void_p(base - 8)) == INV
    assert norm(depth_out=C.c_void_p(base + 312)) == INV
    assert norm(V=65536, H=1, W=1, k=np.tile((50.0, 50.0, 2.0, 2.0), (65536, 1))) == UNS and norm(V=1, H=1 << 16, W=1 << 16) == UNS


def test_wrapper_checks_without_gpu():
    """The wrappers' own refusals come before anything touches a device."""
    import torch
    from omg_planner_amd import _lib, camera, ops
    E = _lib.OmgHipError
    f = torch.zeros((1, 4, 4), dtype=torch.uint16)
    with pytest.raises(E, match="device tensor"):
        ops.condition_depth(f, 0.001, 0.5, 4.0, (0.01, 0.0, 0.0))
    with pytest.raises(E, match="uint16 or float64"):
        ops.condition_depth(torch.zeros((1, 4, 4), dtype=torch.float32), 0.001, 0.5, 4.0, (0.01, 0.0, 0.0))
    with pytest.raises(E, match="uint16 or float64"):
        ops.condition_depth(np.zeros((1, 4, 4), np.uint16), 0.001, 0.5, 4.0, (0.01, 0.0, 0.0))
    with pytest.raises(E, match="device tensor"):
        ops.depth_normals(torch.zeros((1, 4, 4), dtype=torch.float64), [(1.0, 1.0, 0.0, 0.0)], (0.01, 0.0, 0.0))
    with pytest.raises(E, match="must be a tensor"):
        ops.depth_normals(np.zeros((1, 4, 4)), [(1.0, 1.0, 0.0, 0.0)], (0.01, 0.0, 0.0))
    for fn in (camera.observe_frames, camera.Observation.conditioned, ops.condition_depth, ops.depth_normals, ops.FrameBatch):
        assert callable(fn)
    with pytest.raises(E, match="uint16 or float64"):
        camera.observe_frames(np.zeros((1, 4, 4), np.float32), 0.001, np.eye(4), (1.0, 1.0, 0.0, 0.0), (0.01, 0.0, 0.0), device="cpu")
    with pytest.raises(E, match=r"\[S,H,W\]"):
        camera.observe_frames(np.zeros((4, 4), np.uint16), 0.001, np.eye(4), (1.0, 1.0, 0.0, 0.0), (0.01, 0.0, 0.0), device="cpu")
    # an observation of frames alone has cameras and no instances; what needs an instance image says so
    batch = ops.FrameBatch(np.stack([camera.camera_rows((50.0, 50.0, 2.0, 2.0), np.eye(4))] * 2), device="cpu")
    assert batch.num_scenes == 2 and batch.num_instances == 0 and batch.h_inst_begin.tolist() == [0, 0, 0] and batch.frames_only
    assert batch.h_cameras["inst_count"].tolist() == [0, 0] and batch.h_cameras["fx"].tolist() == [50.0, 50.0]
    none = torch.full((2, 4, 4), -1, dtype=torch.int32)
    obs = camera.Observation(batch, torch.zeros((2, 4, 4), dtype=torch.float64), none, none)
    assert obs.flags is None and obs.normals is None and obs.intrinsics().tolist() == [[50.0, 50.0, 2.0, 2.0]] * 2
    with pytest.raises(E, match="needs an instance image"):
        obs.clouds(-1)
    with pytest.raises(E, match="needs an instance image"):
        obs._obstacle_views(None, np.zeros((0, 2)), True)
    with pytest.raises(E, match=r"frames must be \[2, 4, 4\]"):
        obs.conditioned((0.01, 0.0, 0.0), frames=torch.zeros((1, 4, 4), dtype=torch.uint16))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the effect, on the specification alone
# ---------------------------------------------------------------------------------------------------------------------
def test_conditioning_a_simulated_frame_of_the_sphere_scene():
    """fusion_cases' sphere on a slab, three cameras, through sensor.simulate at a committed seed (about 3 mm of noise at 0.8 m, 1 %
    dropout, flying pixels at the silhouettes where the gap exceeds 4 tau), conditioned with R = 2 and given normals.
    Reached at this seed: 36 of 36 flying pixels flagged, 0.46 % of the true-surface pixels dropped, rms 2.62 mm raw and 1.47 mm
    conditioned over 4 344 pixels (ratio 0.56).  Asserted: every flying pixel is flagged, at most 2 % dropped, the rms below the raw
    frame's."""
    from omg_planner_amd import sensor
    e = SC.effect()
    simulated, flagged, dropped_share, rms_raw, rms_out, count = SC.effect_figures(e)
    print("flying", simulated, "flagged", flagged, "dropped share", dropped_share, "rms raw", rms_raw, "conditioned", rms_out, "over", count)
    m = e["masks"]
    assert e["frame"].dtype == np.uint16 and (e["frame"][m["background"] | m["dropout"]] == 0).all() and m["dropout"].sum() > 10
    assert simulated >= 20 and flagged == simulated  # 1. every simulated flying pixel is flagged 2
    assert dropped_share <= SC.MAX_DROPPED_SHARE      # 2. the cap
    assert count > 3000 and rms_out < rms_raw         # 3. the direction
    # no flying pixel touches another, and each sits between a near and a far surface
    fly = m["flying"]
    touching = sum(sensor._shift(fly, dr, dc, False) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if dr or dc)
    assert not (fly & (touching > 0)).any()
    # the normals of the slab's pixels point along the world's +z, those of the sphere away from its centre
    cfw, _ = SC.FC.scene_cameras()
    kept = (e["flags2"] == sensor.KEPT) & np.isfinite(e["t"])
    sphere = SC.FC.scene_sphere_pixels() & kept
    for v in range(3):
        R = np.linalg.inv(cfw[v])[:3, :3]  # world_from_cam
        n_world = e["normals"][v] @ R.T
        slab = kept[v] & ~SC.FC.scene_sphere_pixels()[v]
        assert np.median(n_world[slab][:, 2]) > 0.95, v
        assert (np.einsum("ij,ij->i", e["normals"][v][kept[v]], _rays(e, v)[kept[v]]) < 0).all()  # every normal faces the camera
        assert sphere[v].sum() > 50


def test_flying_pixels_bridge_a_plate_to_the_wall_and_conditioning_parts_them():
    """The case the GPU test runs through segment_obstacles, built here with the specifications: in the raw frame the component
    picked at the plate reaches the wall's depth (its box spans the layout's z); in the conditioned one it is the plate alone."""
    p = SC.plate()
    raw, cond = p["picked"]["raw"], p["picked"]["conditioned"]
    print("flying", int(p["masks"]["flying"].sum()), "picked raw", raw.tolist(), "conditioned", cond.tolist())
    assert p["masks"]["flying"].sum() >= 30 and (p["flags2"][p["masks"]["flying"]] == 2).all()
    wall_k = int((SC.WALL_Z - SC.PLATE_LAYOUT[0][2]) / SC.PLATE_LAYOUT[1])  # the wall's layer of nodes
    assert raw[7] >= wall_k and cond[7] < wall_k - 1 and cond[0] > 1000 and raw[0] > 2 * cond[0]
    rows, cols = SC.PLATE_ROWS, SC.PLATE_COLS
    assert cond[5] - cond[2] <= (cols[1] - cols[0]) + 1 and cond[6] - cond[3] <= (rows[1] - rows[0]) + 1  # no wider than the plate (1 cm a pixel)


def _rays(e, v):
    k = e["intrinsics"][v]
    H, W = e["t"].shape[1:]
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([(c - k[2]) / k[0], (r - k[3]) / k[1], np.ones((H, W))], -1)
