// omg_sensor.hip — depth conditioning: a sensor's frames to the clean depth images the other ops read, and the vertex and normal
// maps of such an image (include/omg_hip.h section 23).
//
// k_depth_condition: one workgroup of 256 threads per 16 x 16 pixel tile of ONE view (gridDim.y), one thread per pixel under the
//                    row map.  The tile's depths with a halo of R + 1 are staged in LDS (a pixel without a return, or outside the
//                    image, as 0.0), every thread taking up to four of the at most 32 x 32 values.  The flying-pixel test runs
//                    on the halo-R region there, its answers kept in registers over a barrier; then everything that does not
//                    survive is overwritten with 0.0, and after a second barrier a thread filters its pixel reading one double
//                    per tap: a tap takes part if it is > 0.  The spatial table's index is uniform: scalar loads.
// k_depth_normals:   the same grid; the tile's depths with a halo of 1 are staged in LDS (18 rows at the same pitch) and a pixel
//                    reads its own and its four neighbours' there.  OMGX_SENSOR_NORMALS_DIRECT builds the five reads straight
//                    from global memory instead: the same bits, measured a little slower.
// The arithmetic is omg_sensor_body.h: the bits of omg-planner_amd/sensor.py.  Plain loads and stores only.
#include "omg_mesh_common.h"
#include "omg_sensor_body.h"

#pragma clang fp contract(off)

#define SN_BLOCK 256
static_assert(SN_BLOCK == OMGX_CAMERA_PIXELS_PER_WORKGROUP, "a pixel per thread");
#define SN_STAGE_ROUNDS ((SENSOR_SIDE_MAX * SENSOR_SIDE_MAX + SN_BLOCK - 1) / SN_BLOCK)

namespace {

__global__ __launch_bounds__(SN_BLOCK) void k_depth_condition(const void* __restrict__ in, int kind, double scale, int H, int W, int tiles_x,
                                                              double z_min, double z_max, double t0, double t1, double t2, int min_support,
                                                              int R, const double* __restrict__ table, double range_scale,
                                                              double* __restrict__ depth_out, uint8_t* __restrict__ flags) {
    __shared__ double tile[SENSOR_SIDE_MAX * SENSOR_PITCH];
    const int tid = threadIdx.x;
    const int64_t image = (int64_t)blockIdx.y * H * W;
    int pr, pc;
    image_row_pixel(blockIdx.x, tiles_x, tid, &pr, &pc);
    const int halo = R + 1, side = IMAGE_TILE + 2 * halo;  // side <= SENSOR_SIDE_MAX: the entry point has checked R
    const int r0 = pr - (tid >> 4) - halo, c0 = pc - (tid & 15) - halo;  // the staged tile's corner in the image
    for (int k = 0; k < SN_STAGE_ROUNDS; ++k) {
        const int i = tid + k * SN_BLOCK;
        const int y = i / side, x = i - y * side;
        if (y < side) {
            const int r = r0 + y, c = c0 + x;
            const bool inside = r >= 0 && r < H && c >= 0 && c < W;
            tile[y * SENSOR_PITCH + x] = inside ? sensor_depth(in, kind, image + (int64_t)r * W + c, scale, z_min, z_max) : 0.0;
        }
    }
    __syncthreads();
    // the halo-R region: rows and columns 1 .. side - 2 of the staged tile
    const int inner = side - 2;
    unsigned dead = 0;
    for (int k = 0; k < SN_STAGE_ROUNDS; ++k) {
        const int i = tid + k * SN_BLOCK;
        const int y = i / inner, x = i - y * inner;
        if (y < inner && !sensor_survives(tile, SENSOR_PITCH, (y + 1) * SENSOR_PITCH + x + 1, t0, t1, t2, min_support)) dead |= 1u << k;
    }
    const int own = ((tid >> 4) + halo) * SENSOR_PITCH + (tid & 15) + halo;
    const double raw = tile[own];
    __syncthreads();  // every test has read the returns
    for (int k = 0; k < SN_STAGE_ROUNDS; ++k) {
        const int i = tid + k * SN_BLOCK;
        const int y = i / inner, x = i - y * inner;
        if (dead >> k & 1u) tile[(y + 1) * SENSOR_PITCH + x + 1] = 0.0;
    }
    __syncthreads();
    const bool kept = tile[own] > 0.0;
    const double out = kept ? sensor_filter(tile, SENSOR_PITCH, own, R, table, range_scale, t0, t1, t2) : 0.0;
    if (pr < H && pc < W) {
        const int64_t at = image + (int64_t)pr * W + pc;
        depth_out[at] = out;
        flags[at] = kept ? OMGX_SENSOR_KEPT : raw > 0.0 ? OMGX_SENSOR_FLYING : OMGX_SENSOR_NO_RETURN;
    }
}

__global__ __launch_bounds__(SN_BLOCK) void k_depth_normals(const double* __restrict__ depth_in, const uint8_t* __restrict__ flags_in,
                                                            const double* __restrict__ intrinsics, int H, int W, int tiles_x, double t0,
                                                            double t1, double t2, double cos_min, double* __restrict__ normals,
                                                            double* __restrict__ depth_out, uint8_t* __restrict__ flags_out,
                                                            double* __restrict__ cosine) {
    const double* __restrict__ k = intrinsics + (int64_t)blockIdx.y * 4;  // uniform: scalar loads
    const int64_t image = (int64_t)blockIdx.y * H * W;
    int pr, pc;
    image_row_pixel(blockIdx.x, tiles_x, threadIdx.x, &pr, &pc);
    const double kk[4] = {k[0], k[1], k[2], k[3]};
#if !defined(OMGX_SENSOR_NORMALS_DIRECT)
    // the tile with a halo of 1 through LDS, 18 rows at the pitch of k_depth_condition; what lies outside the image is never read
    __shared__ double tile[(IMAGE_TILE + 2) * SENSOR_PITCH];
    const int r0 = pr - (int)(threadIdx.x >> 4) - 1, c0 = pc - (int)(threadIdx.x & 15) - 1;
    for (int i = threadIdx.x; i < (IMAGE_TILE + 2) * (IMAGE_TILE + 2); i += SN_BLOCK) {
        const int y = i / (IMAGE_TILE + 2), x = i - y * (IMAGE_TILE + 2), r = r0 + y, c = c0 + x;
        tile[y * SENSOR_PITCH + x] = r >= 0 && r < H && c >= 0 && c < W ? depth_in[image + (int64_t)r * W + c] : 0.0;
    }
    __syncthreads();
    if (pr >= H || pc >= W) return;
    const int64_t at = image + (int64_t)pr * W + pc;
    double n[3], cs, z;
    const uint8_t flag = sensor_normal(tile, -((int64_t)r0 * SENSOR_PITCH + c0), SENSOR_PITCH, H, W, pr, pc, kk, t0, t1, t2, cos_min,
                                       flags_in ? flags_in[at] : (uint8_t)0, n, &cs, &z);
#else
    // the measurement variant: no LDS, no barrier
    if (pr >= H || pc >= W) return;
    const int64_t at = image + (int64_t)pr * W + pc;
    double n[3], cs, z;
    const uint8_t flag = sensor_normal(depth_in + image, 0, W, H, W, pr, pc, kk, t0, t1, t2, cos_min, flags_in ? flags_in[at] : (uint8_t)0, n, &cs, &z);
#endif
    normals[at * 3] = n[0], normals[at * 3 + 1] = n[1], normals[at * 3 + 2] = n[2];
    depth_out[at] = z;
    flags_out[at] = flag;
    if (cosine) cosine[at] = cs;
}

}  // namespace

extern "C" int omgx_depth_condition(const void* depth_in, int32_t in_kind, double scale, int32_t num_views, int32_t H, int32_t W, double z_min,
                                    double z_max, double t0, double t1, double t2, int32_t min_support, int32_t radius, const double* table,
                                    const double* h_table, double range_scale, double* depth_out, uint8_t* flags, void* stream) {
    const int32_t V = num_views, R = radius;
    if (V < 0 || R < 0 || min_support < 0 || min_support > 8) return OMGX_ERR_INVALID;
    if (in_kind != OMGX_SENSOR_UINT16 && in_kind != OMGX_SENSOR_FLOAT64) return OMGX_ERR_INVALID;
    const double s[4] = {scale, z_min, z_max, range_scale};
    if (!image_all_finite(s, 4) || !(scale > 0.0) || !(z_min > 0.0) || !(z_min <= z_max) || !(range_scale > 0.0)) return OMGX_ERR_INVALID;
    if (sensor_check_tau(t0, t1, t2) != OMGX_OK) return OMGX_ERR_INVALID;
    if (R <= OMGX_SENSOR_MAX_RADIUS && (!table || !h_table || sensor_check_table(h_table, R) != OMGX_OK)) return OMGX_ERR_INVALID;
    if (V > 0 && (!depth_in || !depth_out || !flags || H < 1 || W < 1)) return OMGX_ERR_INVALID;
    if (R > OMGX_SENSOR_MAX_RADIUS) return OMGX_ERR_UNSUPPORTED;
    if (V == 0) return OMGX_OK;
    if (image_check_grid(V, H, W) != OMGX_OK || !image_pixels_fit(V, H, W)) return OMGX_ERR_UNSUPPORTED;
    const int64_t pixels = (int64_t)V * H * W;
    if (sensor_overlap(depth_in, pixels * (in_kind == OMGX_SENSOR_UINT16 ? 2 : 8), depth_out, pixels * 8)) return OMGX_ERR_INVALID;
    int tiles_x;
    const int64_t tiles = image_tile_grid(H, W, &tiles_x);
    hipLaunchKernelGGL(k_depth_condition, dim3((unsigned)tiles, (unsigned)V), dim3(SN_BLOCK), 0, (hipStream_t)stream, depth_in, (int)in_kind, scale,
                       (int)H, (int)W, tiles_x, z_min, z_max, t0, t1, t2, (int)min_support, (int)R, table, range_scale, depth_out, flags);
    OMGX_CHECK_LAUNCH("k_depth_condition");
    return OMGX_OK;
}

extern "C" int omgx_depth_normals(const double* depth_in, const uint8_t* flags_in, const double* intrinsics, const double* h_intrinsics,
                                  int32_t num_views, int32_t H, int32_t W, double t0, double t1, double t2, double cos_min, double* normals,
                                  double* depth_out, uint8_t* flags_out, double* cosine, void* stream) {
    const int32_t V = num_views;
    if (V < 0 || sensor_check_tau(t0, t1, t2) != OMGX_OK || !std::isfinite(cos_min)) return OMGX_ERR_INVALID;
    if (V > 0 && (!depth_in || !intrinsics || !h_intrinsics || !normals || !depth_out || !flags_out || H < 1 || W < 1)) return OMGX_ERR_INVALID;
    if (V > 0 && image_check_rows(h_intrinsics, V, 4) != OMGX_OK) return OMGX_ERR_INVALID;
    if (V == 0) return OMGX_OK;
    if (image_check_grid(V, H, W) != OMGX_OK || !image_pixels_fit(V, H, W)) return OMGX_ERR_UNSUPPORTED;
    const int64_t pixels = (int64_t)V * H * W;
    if (sensor_overlap(depth_in, pixels * 8, depth_out, pixels * 8) || sensor_overlap(depth_in, pixels * 8, normals, pixels * 24) ||
        (cosine && sensor_overlap(depth_in, pixels * 8, cosine, pixels * 8)))
        return OMGX_ERR_INVALID;
    int tiles_x;
    const int64_t tiles = image_tile_grid(H, W, &tiles_x);
    hipLaunchKernelGGL(k_depth_normals, dim3((unsigned)tiles, (unsigned)V), dim3(SN_BLOCK), 0, (hipStream_t)stream, depth_in, flags_in, intrinsics,
                       (int)H, (int)W, tiles_x, t0, t1, t2, cos_min, normals, depth_out, flags_out, cosine);
    OMGX_CHECK_LAUNCH("k_depth_normals");
    return OMGX_OK;
}
