// omg_camera.hip — a depth camera for the scenes' own meshes (include/omg_hip.h section 14).
//
// k_render_depth: one workgroup per 16 x 16 pixel tile of ONE scene, one thread per pixel.  It walks the scene's instances in
// order; every lane tests its ray against the instance's bounding ball, and only when some lane of the tile can hit it are the
// instance's faces streamed through LDS tile by tile as in k_mesh_raycast (mesh_stage_faces, omg_mesh_common.h) and cast with
// mesh_raycast_pair (omg_grasp_body.h).  The nearest hit per pixel is kept in registers and every pixel is written once.
// k_pixel_count / k_pixel_scan / k_pixel_gather: the hit pixels of one class as a packed list of world-frame points in pixel
// order: a count per group of 256 row-major pixels (ballot + popcount), an exclusive scan of all counts by one workgroup, and a
// gather that recomputes the mask and ranks the lanes inside their group.  All arithmetic is float64 with contraction off
// (omg_camera_body.h), one operation per operation of the specification camera.render_depth / camera.pixel_clouds
// (omg-planner_amd/camera.py).  Plain loads and stores only.
#include "omg_mesh_common.h"
#include "omg_camera_body.h"

#pragma clang fp contract(off)

#define CAM_BLOCK OMGX_CAMERA_PIXELS_PER_WORKGROUP
static_assert(CAM_BLOCK == IMAGE_TILE * IMAGE_TILE && CAM_BLOCK == OMGX_MESH_FACE_TILE, "mesh_stage_faces moves one face per thread");
static_assert(sizeof(omgx_camera) == 136 && sizeof(omgx_instance) == 136, "records as include/omg_hip.h documents them");

namespace {

__global__ __launch_bounds__(CAM_BLOCK) void k_render_depth(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                            const omgx_mesh* __restrict__ meshes,
                                                            const omgx_instance* __restrict__ instances,
                                                            const omgx_camera* __restrict__ cameras, int H, int W, int tiles_x, int cull,
                                                            double t_min, double neg_tol, double one_tol, double* __restrict__ t_out,
                                                            int32_t* __restrict__ inst_out, int32_t* __restrict__ face_out) {
    __shared__ double tile[OMGX_MESH_FACE_TILE * 9];
    __shared__ int wave_any[2][CAM_BLOCK / 64];
    const omgx_camera* __restrict__ cam = cameras + blockIdx.y;  // uniform: scalar loads
    const int tid = threadIdx.x;
    int pr, pc;
    image_row_pixel(blockIdx.x, tiles_x, tid, &pr, &pc);
    // lanes outside the image redo the last valid pixel of their row or column and store nothing
    double dx, dy;
    image_pixel_dir(min(pr, H - 1), min(pc, W - 1), cam->fx, cam->fy, cam->cx, cam->cy, dx, dy);

    double best = __builtin_inf();
    int32_t inst = -1, face = -1;
    const int n_inst = cam->inst_count;
    for (int i = 0; i < n_inst; ++i) {
        const omgx_instance* __restrict__ in = instances + ((int64_t)cam->inst_begin + i);  // uniform
        bool act = true;
        if (cull) {
            act = camera_instance_active(in->centre, in->q, dx, dy);
            // Workgroup-wide OR: a ballot per wave, one flag per wave in LDS.  Two sets of flags by the parity of i: a wave that
            // writes set i & 1 again (instance i + 2) has passed the barrier of instance i + 1, which every wave reaches only
            // after it has read the flags of instance i.
            const bool wave = __ballot(act) != 0ull;
            if ((tid & 63) == 0) wave_any[i & 1][tid >> 6] = wave;
            __syncthreads();
            const int any = wave_any[i & 1][0] | wave_any[i & 1][1] | wave_any[i & 1][2] | wave_any[i & 1][3];
            if (!any) continue;  // no pixel of the tile can hit this instance: its faces are not read at all
        }
        const omgx_mesh* __restrict__ ms = meshes + in->mesh;
        const double* __restrict__ mv = verts + (int64_t)ms->vert_begin * 3;
        const int32_t* __restrict__ mf = faces + (int64_t)ms->face_begin * 3;
        const int nv = ms->vert_count, nf = ms->face_count;
        double o[3], d[3];
        camera_object_ray(in->m, dx, dy, o, d);
        // The per-mesh loop starts from the running best, not from +inf.  The specification takes the instance's own nearest hit
        // (t_i, f_i) and commits it iff t_i < best.  A face with t >= best can never be that hit when t_i < best, and when
        // t_i >= best nothing is committed either way; among the faces with t < best the strict < still keeps the first face
        // that reaches the minimum.  So (b, f) below equals (t_i, f_i) whenever b < best, and is left at best otherwise.
        double b = best;
        int32_t f = -1;
        for (int t0 = 0; t0 < nf; t0 += OMGX_MESH_FACE_TILE) {
            const int cnt = min(OMGX_MESH_FACE_TILE, nf - t0);
            mesh_stage_faces(tile, mv, mf, nv, t0, cnt);
            if (act) {  // (no barrier inside)
                for (int q = 0; q < cnt; ++q) {
                    mesh_raycast_pair(o[0], o[1], o[2], d[0], d[1], d[2], tile + q * 9, t0 + q, t_min, neg_tol, one_tol, b, f);
                }
            }
        }
        const bool hit = act && (b < best);
        best = hit ? b : best;
        inst = hit ? i : inst;
        face = hit ? f : face;
    }
    if (pr < H && pc < W) {
        const int64_t at = ((int64_t)blockIdx.y * H + pr) * W + pc;
        t_out[at] = best;
        inst_out[at] = inst;
        if (face_out) face_out[at] = face;
    }
}

// Does the cloud of class cls keep pixel p of scene s?  (p < H * W)
__device__ __forceinline__ bool pixel_kept(const omgx_instance* __restrict__ instances, const omgx_camera* __restrict__ cam,
                                           const int32_t* __restrict__ inst_img, int64_t at, int32_t cls) {
    const int32_t inst = inst_img[at];
    const bool known = inst >= 0 && inst < cam->inst_count;  // anything else names no instance: not kept, no record read
    const int32_t label = known ? instances[(int64_t)cam->inst_begin + inst].label : -1;
    return camera_pixel_kept(inst, cam->inst_count, label, cls);
}

__global__ __launch_bounds__(CAM_BLOCK) void k_pixel_count(const omgx_instance* __restrict__ instances,
                                                           const omgx_camera* __restrict__ cameras, int64_t HW,
                                                           const int32_t* __restrict__ inst_img, int32_t cls,
                                                           int32_t* __restrict__ counts) {
    __shared__ int wave_count[CAM_BLOCK / 64];
    const omgx_camera* __restrict__ cam = cameras + blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * CAM_BLOCK + threadIdx.x;
    const bool keep = p < HW && pixel_kept(instances, cam, inst_img, (int64_t)blockIdx.y * HW + p, cls);
    const int n = __popcll(__ballot(keep));
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

// counts [n] (scene-major, `groups` per scene) -> exclusive offsets in place, scene_begin [S + 1].  ONE workgroup walks the list
// 256 entries at a time: a shuffle scan inside each wave, the four wave totals through LDS, a running carry in registers.
__global__ __launch_bounds__(CAM_BLOCK) void k_pixel_scan(int32_t* __restrict__ counts, int n, int groups, int num_scenes,
                                                          int32_t* __restrict__ scene_begin) {
    __shared__ int wave_total[CAM_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += CAM_BLOCK) {
        const int i = base + (int)threadIdx.x;
        const int v = i < n ? counts[i] : 0;
        int x = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(x, off, 64);
            x += lane >= off ? y : 0;
        }
        if (lane == 63) wave_total[wave] = x;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; ++w) before += wave_total[w];
        const int total = (wave_total[0] + wave_total[1]) + (wave_total[2] + wave_total[3]);
        const int exclusive = carry + before + (x - v);
        if (i < n) {
            counts[i] = exclusive;
            if (i % groups == 0) scene_begin[i / groups] = exclusive;
        }
        carry += total;
        __syncthreads();  // wave_total is written again
    }
    if (threadIdx.x == 0) scene_begin[num_scenes] = carry;
}

__global__ __launch_bounds__(CAM_BLOCK) void k_pixel_gather(const omgx_instance* __restrict__ instances,
                                                            const omgx_camera* __restrict__ cameras, int64_t HW, int W,
                                                            const double* __restrict__ t_img, const int32_t* __restrict__ inst_img,
                                                            int32_t cls, const int32_t* __restrict__ offsets,
                                                            double* __restrict__ points, int64_t cap) {
    __shared__ int wave_count[CAM_BLOCK / 64];
    const omgx_camera* __restrict__ cam = cameras + blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * CAM_BLOCK + threadIdx.x;
    const int64_t at = (int64_t)blockIdx.y * HW + p;
    const bool keep = p < HW && pixel_kept(instances, cam, inst_img, at, cls);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_count[w];
    const int64_t row = (int64_t)offsets[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] + before + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep && row >= 0 && row < cap) {
        double dx, dy, w[3];
        image_pixel_dir((int)(p / W), (int)(p % W), cam->fx, cam->fy, cam->cx, cam->cy, dx, dy);
        camera_world_point(cam->world_from_cam, t_img[at], dx, dy, w);
        points[row * 3] = w[0], points[row * 3 + 1] = w[1], points[row * 3 + 2] = w[2];
    }
}

// The host copies of the records and the image size -> OMGX_OK or OMGX_ERR_INVALID.  num_meshes < 0: the mesh indices are not checked (the cloud kernels do not read them).
int check_records(const omgx_instance* h_instances, int32_t num_instances, const omgx_camera* h_cameras, int32_t num_scenes, int32_t H,
                  int32_t W, int32_t num_meshes) {
    if (num_instances < 0 || num_scenes < 0 || H < 1 || W < 1) return OMGX_ERR_INVALID;
    if ((num_instances > 0 && !h_instances) || (num_scenes > 0 && !h_cameras)) return OMGX_ERR_INVALID;
    for (int32_t i = 0; i < num_instances; ++i) {
        const omgx_instance& in = h_instances[i];
        if (!image_all_finite(in.m, 12) || !image_all_finite(in.centre, 3) || !std::isfinite(in.q) || in.label < 0 || in.mesh < 0) return OMGX_ERR_INVALID;
        if (num_meshes >= 0 && in.mesh >= num_meshes) return OMGX_ERR_INVALID;
    }
    for (int32_t s = 0; s < num_scenes; ++s) {
        const omgx_camera& c = h_cameras[s];
        if (image_check_camera(c) != OMGX_OK) return OMGX_ERR_INVALID;
        if (c.inst_begin < 0 || c.inst_count < 0 || (int64_t)c.inst_begin + c.inst_count > num_instances) return OMGX_ERR_INVALID;
    }
    return OMGX_OK;
}

// What the cloud kernels admit (valid sizes) -> OMGX_OK or OMGX_ERR_UNSUPPORTED: scenes are gridDim.y, the offsets are int32.
int check_cloud_limits(int32_t num_scenes, int32_t H, int32_t W) {
    return num_scenes > IMAGE_MAX_VIEWS || !image_pixels_fit(num_scenes, H, W) ? OMGX_ERR_UNSUPPORTED : OMGX_OK;
}

int64_t pixel_groups(int32_t H, int32_t W) { return ((int64_t)H * W + CAM_BLOCK - 1) / CAM_BLOCK; }

}  // namespace

extern "C" int omgx_render_depth(const double* verts, const int32_t* faces, const omgx_mesh* meshes, const omgx_mesh* h_meshes,
                                 int32_t num_meshes, const omgx_instance* instances, const omgx_instance* h_instances,
                                 int32_t num_instances, const omgx_camera* cameras, const omgx_camera* h_cameras, int32_t num_scenes,
                                 int32_t H, int32_t W, int32_t cull, double t_min, double tol, double* t_out, int32_t* inst_out,
                                 int32_t* face_out, void* stream) {
    if (!verts || !faces || !meshes || !h_meshes || num_meshes < 1) return OMGX_ERR_INVALID;
    if (!(t_min >= 0.0) || !(tol >= 0.0) || !std::isfinite(t_min) || !std::isfinite(tol)) return OMGX_ERR_INVALID;
    if (num_instances > 0 && !instances) return OMGX_ERR_INVALID;
    if (num_scenes > 0 && (!cameras || !t_out || !inst_out)) return OMGX_ERR_INVALID;
    for (int32_t m = 0; m < num_meshes; ++m)
        if (mesh_check_ranges(h_meshes[m]) != OMGX_OK) return OMGX_ERR_INVALID;  // the volume fields are not read here
    int status = check_records(h_instances, num_instances, h_cameras, num_scenes, H, W, num_meshes);
    if (status == OMGX_OK) status = image_check_grid(num_scenes, H, W);
    if (status != OMGX_OK) return status;
    if (num_scenes == 0) return OMGX_OK;
    int tiles_x;
    const int64_t tiles = image_tile_grid(H, W, &tiles_x);
    hipLaunchKernelGGL(k_render_depth, dim3((unsigned)tiles, (unsigned)num_scenes), dim3(CAM_BLOCK), 0, (hipStream_t)stream, verts,
                       faces, meshes, instances, cameras, (int)H, (int)W, tiles_x, (int)(cull != 0), t_min, -tol, 1.0 + tol, t_out, inst_out,
                       face_out);
    OMGX_CHECK_LAUNCH("k_render_depth");
    return OMGX_OK;
}

extern "C" int64_t omgx_pixel_clouds_workspace_bytes(int32_t num_scenes, int32_t H, int32_t W) {
    if (num_scenes < 0 || H < 1 || W < 1) return OMGX_ERR_INVALID;
    return (int64_t)num_scenes * pixel_groups(H, W) * (int64_t)sizeof(int32_t);
}

extern "C" int omgx_pixel_count(const omgx_instance* instances, const omgx_instance* h_instances, int32_t num_instances,
                                const omgx_camera* cameras, const omgx_camera* h_cameras, int32_t num_scenes, int32_t H, int32_t W,
                                const int32_t* inst_img, int32_t cls, void* workspace, int32_t* scene_begin, void* stream) {
    if (!scene_begin) return OMGX_ERR_INVALID;
    if (num_instances > 0 && !instances) return OMGX_ERR_INVALID;
    if (num_scenes > 0 && (!cameras || !inst_img || !workspace)) return OMGX_ERR_INVALID;
    int status = check_records(h_instances, num_instances, h_cameras, num_scenes, H, W, -1);
    if (status == OMGX_OK) status = check_cloud_limits(num_scenes, H, W);
    if (status != OMGX_OK) return status;
    const int64_t groups = pixel_groups(H, W);
    if (num_scenes > 0) {
        hipLaunchKernelGGL(k_pixel_count, dim3((unsigned)groups, (unsigned)num_scenes), dim3(CAM_BLOCK), 0, (hipStream_t)stream, instances, cameras,
                           (int64_t)H * W, inst_img, cls, (int32_t*)workspace);
        OMGX_CHECK_LAUNCH("k_pixel_count");
    }
    // (with no scene: scene_begin[0] = 0)
    hipLaunchKernelGGL(k_pixel_scan, dim3(1), dim3(CAM_BLOCK), 0, (hipStream_t)stream, (int32_t*)workspace, (int)(groups * num_scenes), (int)groups,
                       (int)num_scenes, scene_begin);
    OMGX_CHECK_LAUNCH("k_pixel_scan");
    return OMGX_OK;
}

extern "C" int omgx_pixel_gather(const omgx_instance* instances, int32_t num_instances, const omgx_camera* cameras, int32_t num_scenes,
                                 int32_t H, int32_t W, const double* t_img, const int32_t* inst_img, int32_t cls, const void* workspace,
                                 double* points, int64_t cap, void* stream) {
    if (num_instances < 0 || num_scenes < 0 || H < 1 || W < 1 || cap < 0) return OMGX_ERR_INVALID;
    if (num_instances > 0 && !instances) return OMGX_ERR_INVALID;
    if (num_scenes > 0 && (!cameras || !t_img || !inst_img || !workspace)) return OMGX_ERR_INVALID;
    if (cap > 0 && !points) return OMGX_ERR_INVALID;
    if (check_cloud_limits(num_scenes, H, W) != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    if (num_scenes == 0 || cap == 0) return OMGX_OK;
    hipLaunchKernelGGL(k_pixel_gather, dim3((unsigned)pixel_groups(H, W), (unsigned)num_scenes), dim3(CAM_BLOCK), 0, (hipStream_t)stream, instances,
                       cameras, (int64_t)H * W, (int)W, t_img, inst_img, cls, (const int32_t*)workspace, points, cap);
    OMGX_CHECK_LAUNCH("k_pixel_gather");
    return OMGX_OK;
}
