"""CPU test of csrc/omg_image_body.h, what every kernel over images and its entry point do first: the header compiled for the
host, both tile maps run for every (tile, thread) of an image and compared with numpy, the pixel's ray compared with
camera.pixel_directions as bits, and the host checks of camera rows, grids and pixel counts at their edges."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import kernel_build as KB

BLOCK, TILE, WAVE_TILE = 256, 16, 8
CAMERA = (3.0, -7.0, 0.1, 16.5)  # fx, fy, cx, cy
NAN, INF = float("nan"), float("inf")
_HOST_HARNESS = r"""
#include <algorithm>
#include "omg_image_body.h"
extern "C" void host_constants(int64_t* out) { out[0] = IMAGE_TILE, out[1] = IMAGE_WAVE_TILE, out[2] = IMAGE_MAX_TILES, out[3] = IMAGE_MAX_VIEWS; }
extern "C" int64_t host_tile_grid(int H, int W, int* tiles_x) { return image_tile_grid(H, W, tiles_x); }
// Every (tile, thread) of an H x W image under the row map (which = 0) or the wave map (1): (pr, pc) as int32 [tiles][256][2] and
// the direction of the clamped pixel, as the kernels form it, as float64 [tiles][256][2].
extern "C" void host_map(int which, int H, int W, const double* k, int32_t* px, double* dir) {
    int tiles_x;
    const int64_t tiles = image_tile_grid(H, W, &tiles_x);
    for (int64_t t = 0; t < tiles; ++t)
        for (int tid = 0; tid < 256; ++tid) {
            int pr, pc;
            if (which) image_wave_pixel((uint32_t)t, tiles_x, tid, &pr, &pc); else image_row_pixel((uint32_t)t, tiles_x, tid, &pr, &pc);
            const int64_t at = (t * 256 + tid) * 2;
            px[at] = pr, px[at + 1] = pc;
            image_pixel_dir(std::min(pr, H - 1), std::min(pc, W - 1), k[0], k[1], k[2], k[3], dir[at], dir[at + 1]);
        }
}
extern "C" void host_dirs(int H, int W, const double* k, double* dx, double* dy) {
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) image_pixel_dir(r, c, k[0], k[1], k[2], k[3], dx[r * W + c], dy[r * W + c]);
}
extern "C" int host_all_finite(const double* x, int64_t n) { return image_all_finite(x, n) ? 1 : 0; }
extern "C" int host_check_rows(const double* h, int64_t rows, int stride) { return image_check_rows(h, rows, stride); }
extern "C" int host_check_camera(const double* row) {  // a row of 16 as an omgx_camera record with some instance range
    omgx_camera c = {};
    c.fx = row[0], c.fy = row[1], c.cx = row[2], c.cy = row[3], c.inst_begin = 0, c.inst_count = 0;
    for (int k = 0; k < 12; ++k) c.world_from_cam[k] = row[4 + k];
    return image_check_camera(c);
}
extern "C" int host_check_grid(int V, int H, int W) { return image_check_grid(V, H, W); }
extern "C" int host_pixels_fit(int V, int H, int W) { return image_pixels_fit(V, H, W) ? 1 : 0; }
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    return KB.host_harness(_HOST_HARNESS, tmp_path_factory.mktemp("image_body"), {
        "host_constants": (None, [vp]), "host_tile_grid": (i64, [i, i, vp]), "host_map": (None, [i, i, i, vp, vp, vp]),
        "host_dirs": (None, [i, i, vp, vp, vp]), "host_all_finite": (i, [vp, i64]), "host_check_rows": (i, [vp, i64, i]),
        "host_check_camera": (i, [vp]), "host_check_grid": (i, [i, i, i]), "host_pixels_fit": (i, [i, i, i])})


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


@KB.requires_host_cxx
@pytest.mark.parametrize("H,W", ((1, 1), (16, 16), (17, 33), (8, 40)))
def test_tile_maps_equal_numpy_for_every_tile_and_thread(host, H, W):
    """Both maps on every (tile, thread): the row map is the tile in row-major order; in the wave map wave w covers the 8 x 8 block
    (w >> 1, w & 1) of the tile and lane l the pixel (l >> 3, l & 7) of it.  Every pixel of the image comes from exactly one
    thread, a lane outside the image reports a pixel outside it, and its clamped direction is that of pixel (min(pr, H - 1),
    min(pc, W - 1)) as camera.pixel_directions gives it, bit for bit."""
    from omg_planner_amd import camera
    const = np.zeros(4, np.int64)
    host.host_constants(const.ctypes.data)
    assert const.tolist() == [TILE, WAVE_TILE, 1 << 23, 65535]
    tx = C.c_int(-1)
    tiles = host.host_tile_grid(H, W, C.byref(tx))
    tiles_x, tiles_y = -(-W // TILE), -(-H // TILE)
    assert (tiles, tx.value) == (tiles_x * tiles_y, tiles_x)
    k = np.array(CAMERA)
    dx, dy = camera.pixel_directions(k, H, W)
    ty, tix = np.divmod(np.arange(tiles), tiles_x)
    tid = np.arange(BLOCK)
    wave, lane = tid >> 6, tid & 63
    want = {0: (ty[:, None] * TILE + (tid >> 4), tix[:, None] * TILE + (tid & 15)),
            1: (ty[:, None] * TILE + (wave >> 1) * WAVE_TILE + (lane >> 3), tix[:, None] * TILE + (wave & 1) * WAVE_TILE + (lane & 7))}
    for which in (0, 1):
        px, d = np.full((tiles, BLOCK, 2), -9, np.int32), np.full((tiles, BLOCK, 2), np.nan)
        host.host_map(which, H, W, k.ctypes.data, px.ctypes.data, d.ctypes.data)
        pr, pc = px[..., 0].astype(np.int64), px[..., 1].astype(np.int64)
        assert np.array_equal(pr, want[which][0]) and np.array_equal(pc, want[which][1]), which
        inside = (pr < H) & (pc < W)
        assert (pr >= 0).all() and (pc >= 0).all() and inside.sum() == H * W
        assert np.array_equal(np.bincount((pr * W + pc)[inside], minlength=H * W), np.ones(H * W, np.int64)), which  # each pixel exactly once
        assert ((pr >= H) | (pc >= W))[~inside].all()
        at = np.minimum(pr, H - 1) * W + np.minimum(pc, W - 1)
        assert np.array_equal(_bits(d[..., 0]), _bits(dx[at])) and np.array_equal(_bits(d[..., 1]), _bits(dy[at])), which
    if (H, W) == (17, 33):
        assert tiles == 6 and not inside.all()  # 2 x 3 tiles, partial in both directions
        gx, gy = np.full(H * W, np.nan), np.full(H * W, np.nan)
        host.host_dirs(H, W, k.ctypes.data, gx.ctypes.data, gy.ctypes.data)
        assert np.array_equal(_bits(gx), _bits(dx)) and np.array_equal(_bits(gy), _bits(dy))


@KB.requires_host_cxx
@pytest.mark.parametrize("stride", (16, 4))
def test_row_and_camera_checks_refuse_every_bad_field(host, stride):
    """image_check_rows over rows of 16 (a view, a volume camera) and of 4 (plane intrinsics), from one valid row alone and as the
    last of three: NaN and both infinities are INVALID in every column, 0.0 in columns 0 and 1 only; no rows need no pointer.
    image_check_camera says the same of an omgx_camera record."""
    from omg_planner_amd import _lib
    OK, INV = _lib.OMGX_OK, _lib.OMGX_ERR_INVALID
    good = np.concatenate([CAMERA, np.arange(1.0, 13.0)])[:stride]
    rows = lambda h: host.host_check_rows(np.ascontiguousarray(h).ctypes.data, len(h), stride)
    assert rows(good[None]) == OK and rows(np.tile(good, (3, 1))) == OK
    assert host.host_check_rows(None, 0, stride) == OK and host.host_all_finite(None, 0) == 1
    if stride == 16:
        assert host.host_check_camera(good.ctypes.data) == OK
    for col in range(stride):
        for val in (NAN, INF, -INF, 0.0):
            want = INV if val != 0.0 or col < 2 else OK
            bad = good.copy()
            bad[col] = val
            three = np.tile(good, (3, 1))
            three[2] = bad
            assert rows(bad[None]) == want and rows(three) == want, (col, val)
            assert host.host_all_finite(bad.ctypes.data, stride) == (val == 0.0)
            if stride == 16:
                assert host.host_check_camera(bad.ctypes.data) == want, (col, val)


@KB.requires_host_cxx
def test_grid_and_pixel_limits_at_their_edges(host):
    """gridDim.y holds 65535 images and gridDim.x 2^23 tiles; V * H * W must fit int32 however the product is grouped, also
    where it leaves 32 bits only as a whole."""
    from omg_planner_amd import _lib
    OK, UNS = _lib.OMGX_OK, _lib.OMGX_ERR_UNSUPPORTED
    assert host.host_check_grid(65535, 16, 16) == OK and host.host_check_grid(65536, 16, 16) == UNS
    assert host.host_check_grid(1, 46336, 46336) == OK    # 2896^2 tiles = 8386816 <= 2^23
    assert host.host_check_grid(1, 46337, 46337) == UNS   # 2897^2 tiles = 8392609 > 2^23
    assert host.host_pixels_fit(1, 1, 2147483647) == 1 and host.host_pixels_fit(1, 32768, 65536) == 0
    # 3 x 26755^2 = 2147490075 is 6428 above 2^31 - 1 and needs 64-bit arithmetic: it does not fit, as every entry point has
    # answered so far (OMGX_ERR_UNSUPPORTED), whichever way the product is grouped; 3 x 26754^2 = 2147329548 is the last that does
    assert 3 * 26755 ** 2 == 2147490075 > 2 ** 31 - 1 > 3 * 26754 ** 2
    for a, b, c in ((3, 26755, 26755), (26755, 3, 26755), (26755, 26755, 3)):
        assert host.host_pixels_fit(a, b, c) == 0 and host.host_pixels_fit(*(x - (x > 3) for x in (a, b, c))) == 1
    assert host.host_pixels_fit(32768, 3, 32768) == 0     # V x H fits int32, the whole product does not
