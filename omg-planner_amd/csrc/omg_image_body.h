// omg_image_body.h — what every kernel over images and its entry point do first (omg_camera.hip, omg_volume_camera.hip,
// omg_robot_filter.hip; the host checks also serve omg_plane.hip and mesh_check_views): a thread's pixel of a 16 x 16 tile, the
// pixel's ray, and the checks of camera rows and of what the grids and the index types admit.  Functions of plain integers and
// doubles that also compile for the host (tests/test_image_body_cpu.py).  No HIP built-ins: the kernels pass blockIdx.x, threadIdx.x.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/omg_hip.h"

#if defined(__HIPCC__)
#define IMAGE_HD __host__ __device__ __forceinline__
#else
#define IMAGE_HD inline
#endif

#pragma clang fp contract(off)

// One workgroup of 256 threads per 16 x 16 pixels, a pixel per thread; a wave of the wave map owns 8 x 8 of them.
#define IMAGE_TILE 16
#define IMAGE_WAVE_TILE 8
static_assert(IMAGE_TILE * IMAGE_TILE == OMGX_CAMERA_PIXELS_PER_WORKGROUP && IMAGE_WAVE_TILE * IMAGE_WAVE_TILE == 64, "a wave is a quarter tile");
// Tiles of one image (gridDim.x; gridDim.x * 256 threads must stay below 2^32) and images of one launch (gridDim.y).
#define IMAGE_MAX_TILES (1 << 23)
#define IMAGE_MAX_VIEWS 65535

// The ray of pixel (row r, column c): direction (dx, dy, 1) from the camera origin.
IMAGE_HD void image_pixel_dir(int r, int c, double fx, double fy, double cx, double cy, double& dx, double& dy) {
    dx = ((double)c - cx) / fx;
    dy = ((double)r - cy) / fy;
}

// Thread tid of tile `tile` (row-major, tiles_x per row) -> its pixel.  A lane outside the image gets a pixel outside it: the
// kernels clamp it to the last row or column for the ray and store nothing.  The row map: the tile in row-major order.
IMAGE_HD void image_row_pixel(uint32_t tile, int tiles_x, int tid, int* pr, int* pc) {
    *pr = (int)(tile / tiles_x) * IMAGE_TILE + (tid >> 4);
    *pc = (int)(tile % tiles_x) * IMAGE_TILE + (tid & 15);
}
// The wave map: wave w on the 8 x 8 block (w >> 1, w & 1) of the tile, lane l on (l >> 3, l & 7) of it: 64 rays close together.
IMAGE_HD void image_wave_pixel(uint32_t tile, int tiles_x, int tid, int* pr, int* pc) {
    const int wave = tid >> 6, lane = tid & 63;
    *pr = (int)(tile / tiles_x) * IMAGE_TILE + (wave >> 1) * IMAGE_WAVE_TILE + (lane >> 3);
    *pc = (int)(tile % tiles_x) * IMAGE_TILE + (wave & 1) * IMAGE_WAVE_TILE + (lane & 7);
}

// On the host: the entry points' checks.
static inline bool image_all_finite(const double* x, int64_t count) {
    for (int64_t k = 0; k < count; ++k)
        if (!std::isfinite(x[k])) return false;
    return true;
}
// Rows of `stride` doubles that begin with fx, fy (a view or a volume camera: 16, plane intrinsics: 4): every field finite, no
// focal length of zero -> OMGX_OK or OMGX_ERR_INVALID.
static inline int image_check_rows(const double* h, int64_t rows, int stride) {
    if (!image_all_finite(h, rows * stride)) return OMGX_ERR_INVALID;
    for (int64_t r = 0; r < rows; ++r)
        if (h[r * stride] == 0.0 || h[r * stride + 1] == 0.0) return OMGX_ERR_INVALID;
    return OMGX_OK;
}
// The same for the intrinsics and the pose of one record (not its instance range).
static inline int image_check_camera(const omgx_camera& c) {
    const double k[4] = {c.fx, c.fy, c.cx, c.cy};
    return image_check_rows(k, 1, 4) != OMGX_OK || !image_all_finite(c.world_from_cam, 12) ? OMGX_ERR_INVALID : OMGX_OK;
}
// Tiles of an H x W image (H, W >= 1), *tiles_x of them per row.
static inline int64_t image_tile_grid(int32_t H, int32_t W, int* tiles_x) {
    *tiles_x = (W - 1) / IMAGE_TILE + 1;
    return (int64_t)*tiles_x * ((H - 1) / IMAGE_TILE + 1);
}
// What the grid of a kernel with a tile per workgroup admits (valid sizes) -> OMGX_OK or OMGX_ERR_UNSUPPORTED.
static inline int image_check_grid(int32_t V, int32_t H, int32_t W) {
    int tiles_x;
    return V > IMAGE_MAX_VIEWS || image_tile_grid(H, W, &tiles_x) > IMAGE_MAX_TILES ? OMGX_ERR_UNSUPPORTED : OMGX_OK;
}
// Do the pixels of V images fit int32 indices and counts: V * H * W <= 2^31 - 1?  (V > 0: H, W >= 1; the product may leave int64)
static inline bool image_pixels_fit(int32_t V, int32_t H, int32_t W) { return V < 1 || (int64_t)V * H <= 0x7fffffffll / W; }
