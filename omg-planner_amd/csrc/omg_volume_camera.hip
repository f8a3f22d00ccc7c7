// omg_volume_camera.hip — a depth camera on the SDF pool (include/omg_hip.h section 21).
//
// k_render_volumes: one workgroup of 256 threads per 16 x 16 pixel tile of ONE scene (gridDim.y), one thread per pixel, and each
// of the four waves on its own 8 x 8 block of the tile, so that its 64 rays walk neighbouring cells of a volume and their
// eight-corner gathers share cache lines.  The volumes stay in global memory (64^3 floats are 1 MB: the L2 serves them).  The
// object loop, the record, the camera and m = obj_from_cam depend on the scene and the object only: the record is read through
// uniform loads and m is formed by the same instructions in every lane, once per wave and object.  After the slab test a wave
// votes (one ballot) and skips the march of an object none of its rays can meet; waves do not wait for one another: no LDS,
// no barrier.  The march is a divergent loop: a lane that has hit or left idles until the wave's slowest ray is done.  The
// arithmetic is omg_volume_camera_body.h: the bits of volume_camera.render_volumes (omg-planner_amd/volume_camera.py).  Plain
// loads and stores only; every pixel of every image is written once.
#include "omg_host.h"
#include "omg_image_body.h"
#include "omg_volume_camera_body.h"

#pragma clang fp contract(off)

#define VCAM_BLOCK OMGX_CAMERA_PIXELS_PER_WORKGROUP
static_assert(VCAM_BLOCK == IMAGE_TILE * IMAGE_TILE, "a pixel of a tile per thread");
static_assert(sizeof(omgx_object) == 184, "records as include/omg_hip.h documents them");

namespace {

__global__ __launch_bounds__(VCAM_BLOCK) void k_render_volumes(const omgx_object* __restrict__ objects, int num_objects,
                                                               const int32_t* __restrict__ scene_begin, const float* __restrict__ pool,
                                                               int64_t pool_elems, const double* __restrict__ cameras,
                                                               const uint8_t* __restrict__ visible, int H, int W, int tiles_x, double level,
                                                               double t_min, double min_step, double relax, int max_steps,
                                                               double* __restrict__ t_out, int32_t* __restrict__ inst_out,
                                                               double* __restrict__ normal_out, int32_t* __restrict__ steps_out) {
    const double* __restrict__ cam = cameras + (int64_t)blockIdx.y * 16;  // uniform: scalar loads
    int pr, pc;
    image_wave_pixel(blockIdx.x, tiles_x, threadIdx.x, &pr, &pc);
    // lanes outside the image redo the last valid pixel of their row or column and store nothing
    double dx, dy;
    image_pixel_dir(min(pr, H - 1), min(pc, W - 1), cam[0], cam[1], cam[2], cam[3], dx, dy);

    double best = __builtin_inf(), n0 = 0.0, n1 = 0.0, n2 = 0.0;
    int32_t inst = -1, samples = 0;
    // the scene's records; the entry point has checked the host copy, and the range is cut to the buffer once more
    const int first = max(scene_begin[blockIdx.y], 0);
    const int count = min(scene_begin[blockIdx.y + 1], num_objects) - first;
    for (int k = 0; k < count; ++k) {
        if (visible && !visible[first + k]) continue;  // uniform
        const omgx_object* __restrict__ ob = objects + ((int64_t)first + k);
        if (!vcam_grid_usable(ob->dim, ob->grid_offset, pool_elems)) continue;  // uniform; never true after the host's checks
        vcam_grid G;
        vcam_set_grid(ob->lo, ob->dim, ob->inv_delta, ob->grid_offset, G);
        double m[12];
        vcam_object_from_camera(ob->pose_inv, cam + 4, m);
        vcam_ray R;
        vcam_make_ray(G, m, dx, dy, R);
        double t0, t1;
        const bool ok = vcam_slab(G, R, t_min, t0, t1);
        if (__ballot(ok) == 0ull) continue;  // no ray of this wave meets the box
        if (ok) {
            double th;
            if (vcam_march(G, pool, R, t0, t1, level, min_step, relax, max_steps, th, samples) && th < best) {
                best = th, inst = k;
                if (normal_out) {
                    double n[3];
                    vcam_normal(G, pool, R, m, th, n);
                    n0 = n[0], n1 = n[1], n2 = n[2];
                }
            }
        }
    }
    if (pr < H && pc < W) {
        const int64_t at = ((int64_t)blockIdx.y * H + pr) * W + pc;
        t_out[at] = best;
        inst_out[at] = inst;
        if (normal_out) normal_out[at * 3] = n0, normal_out[at * 3 + 1] = n1, normal_out[at * 3 + 2] = n2;
        if (steps_out) steps_out[at] = samples;
    }
}

}  // namespace

extern "C" int omgx_render_volumes(const omgx_object* objects, const omgx_object* h_objects, int32_t num_objects,
                                   const int32_t* scene_begin, const int32_t* h_scene_begin, int32_t num_scenes, const float* pool,
                                   int64_t pool_elems, const double* cameras, const double* h_cameras, const uint8_t* visible,
                                   const uint8_t* h_visible, int32_t H, int32_t W, double level, double t_min, double min_step, double relax,
                                   int32_t max_steps, double* t_out, int32_t* inst_out, double* normal_out, int32_t* steps_out, void* stream) {
    const int32_t S = num_scenes;
    if (num_objects < 0 || S < 0 || pool_elems < 0 || H < 1 || W < 1) return OMGX_ERR_INVALID;
    if (!std::isfinite(level) || !std::isfinite(t_min) || !std::isfinite(min_step) || !std::isfinite(relax)) return OMGX_ERR_INVALID;
    if (t_min < 0.0 || min_step <= 0.0 || relax <= 0.0 || relax > 1.0) return OMGX_ERR_INVALID;
    if (max_steps < 1 || max_steps > OMGX_VOLUME_CAMERA_MAX_STEPS) return OMGX_ERR_INVALID;
    if ((visible == nullptr) != (h_visible == nullptr)) return OMGX_ERR_INVALID;
    if (num_objects > 0 && (!objects || !h_objects)) return OMGX_ERR_INVALID;
    if (pool_elems > 0 && !pool) return OMGX_ERR_INVALID;
    if (S == 0) return OMGX_OK;
    if (!scene_begin || !h_scene_begin || !cameras || !h_cameras || !t_out || !inst_out) return OMGX_ERR_INVALID;
    if (h_scene_begin[0] < 0 || h_scene_begin[S] > num_objects) return OMGX_ERR_INVALID;
    for (int32_t s = 0; s < S; ++s)
        if (h_scene_begin[s + 1] < h_scene_begin[s]) return OMGX_ERR_INVALID;
    if (image_check_rows(h_cameras, S, 16) != OMGX_OK) return OMGX_ERR_INVALID;
    for (int32_t o = h_scene_begin[0]; o < h_scene_begin[S]; ++o) {
        if (h_visible && !h_visible[o]) continue;
        const omgx_object& r = h_objects[o];
        if (!std::isfinite(r.inv_delta) || !(r.inv_delta > 0.0) || !vcam_grid_usable(r.dim, r.grid_offset, pool_elems)) return OMGX_ERR_INVALID;
    }
    if (image_check_grid(S, H, W) != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    int tiles_x;
    const int64_t tiles = image_tile_grid(H, W, &tiles_x);
    hipLaunchKernelGGL(k_render_volumes, dim3((unsigned)tiles, (unsigned)S), dim3(VCAM_BLOCK), 0, (hipStream_t)stream, objects,
                       (int)num_objects, scene_begin, pool, pool_elems, cameras, visible, (int)H, (int)W, tiles_x, level, t_min, min_step, relax,
                       (int)max_steps, t_out, inst_out, normal_out, steps_out);
    OMGX_CHECK_LAUNCH("k_render_volumes");
    return OMGX_OK;
}
