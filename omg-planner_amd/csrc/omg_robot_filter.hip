// omg_robot_filter.hip — a robot self-filter: the arm's spheres in depth images and obstacle states (include/omg_hip.h section 22).
//
// k_render_spheres: one workgroup of 256 threads per 16 x 16 pixel tile of ONE view (gridDim.y), one thread per pixel, each of
//                   the four waves on its own 8 x 8 block of the tile (as k_render_volumes).  The workgroup moves the spheres into
//                   the view's camera frame a chunk of 256 at a time, one sphere per thread, into LDS (centre, radius and
//                   q = |centre|^2 - R^2: 5 doubles, read by all lanes at one address, a broadcast); the workgroups of tile 0 also
//                   write them to global memory.  Each wave then walks the chunk: one ballot of the cone test per sphere, and a
//                   sphere no ray of the wave can meet is skipped.
// k_clear_robot:    one thread per node in runs of 256 (volume_locate), the state byte read and written in place.  Per view of
//                   the node's volume: the node's point into the camera, the `front` test on the two images, and the view's
//                   spheres through LDS a chunk at a time.  With the cull a thread stages its sphere only if the ball around the
//                   run's nodes can reach it (robot_run_drops); the kept ones are packed by a ballot per wave and the waves'
//                   counts, so the walk is over the kept spheres only.  `inside` is an OR over spheres: their order is free.
// The arithmetic is omg_robot_filter_body.h: the bits of omg-planner_amd/robot_filter.py.  Plain loads and stores only.
#include "omg_mesh_common.h"
#include "omg_robot_filter_body.h"

#pragma clang fp contract(off)

#define RF_BLOCK 256
#define RF_CHUNK OMGX_ROBOT_SPHERE_CHUNK
static_assert(RF_BLOCK == OMGX_CAMERA_PIXELS_PER_WORKGROUP && RF_BLOCK == OMGX_FUSION_NODES_PER_WORKGROUP, "a pixel or a node per thread");
static_assert(RF_CHUNK == RF_BLOCK, "a sphere of a chunk per thread");
static_assert(OMGX_FUSION_FREE == ROBOT_FREE && OMGX_FUSION_UNKNOWN == ROBOT_UNKNOWN, "states");
static_assert(sizeof(omgx_camera) == 136, "records as include/omg_hip.h documents them");

namespace {

__global__ __launch_bounds__(RF_BLOCK) void k_render_spheres(const double* __restrict__ local, const int32_t* __restrict__ link, int N,
                                                             const double* __restrict__ link_poses, int num_configs,
                                                             const omgx_camera* __restrict__ cameras,
                                                             const int32_t* __restrict__ config_of_view, int H, int W, int tiles_x,
                                                             double pad, double t_min, int cull, double* __restrict__ cam_spheres,
                                                             double* __restrict__ t_out, int32_t* __restrict__ sphere_out) {
    __shared__ double tile[RF_CHUNK * 5];
    const omgx_camera* __restrict__ cam = cameras + blockIdx.y;  // uniform: scalar loads
    // (the entry point has checked the host copy; clamped once more so that no index can read outside the poses)
    const int cfg = min(max(config_of_view[blockIdx.y], 0), num_configs - 1);
    const int tid = threadIdx.x;
    int pr, pc;
    image_wave_pixel(blockIdx.x, tiles_x, tid, &pr, &pc);
    // lanes outside the image redo the last valid pixel of their row or column and store nothing
    double dx, dy;
    image_pixel_dir(min(pr, H - 1), min(pc, W - 1), cam->fx, cam->fy, cam->cx, cam->cy, dx, dy);
    const double dd = (dx * dx + dy * dy) + 1.0;

    double best = __builtin_inf();
    int32_t which = -1;
    for (int n0 = 0; n0 < N; n0 += RF_CHUNK) {
        const int cnt = min(RF_CHUNK, N - n0);
        __syncthreads();  // the walk of the chunk before is over
        if (tid < cnt) {
            const int n = n0 + tid;
            const int l = min(max(link[n], 0), OMGX_NUM_LINKS - 1);
            double s[4];
            robot_camera_sphere(link_poses + ((int64_t)cfg * OMGX_NUM_LINKS + l) * 16, local + (int64_t)n * 4, cam->world_from_cam, pad, s);
            for (int k = 0; k < 4; ++k) tile[tid * 5 + k] = s[k];
            tile[tid * 5 + 4] = robot_sphere_q(s);
            if (blockIdx.x == 0) {
                double* __restrict__ out = cam_spheres + ((int64_t)blockIdx.y * N + n) * 4;
                for (int k = 0; k < 4; ++k) out[k] = s[k];
            }
        }
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const double* s = tile + k * 5;
            const double q = s[4];
            if (cull && __ballot(robot_sphere_active(s, q, dx, dy, dd)) == 0ull) continue;  // no ray of this wave meets the sphere
            double entry;
            if (robot_sphere_entry(s, q, dx, dy, dd, t_min, &entry) && entry < best) best = entry, which = n0 + k;
        }
    }
    if (pr < H && pc < W) {
        const int64_t at = ((int64_t)blockIdx.y * H + pr) * W + pc;
        t_out[at] = best;
        sphere_out[at] = which;
    }
}

__global__ __launch_bounds__(RF_BLOCK) void k_clear_robot(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                          const double* __restrict__ views, const int32_t* __restrict__ view_range,
                                                          const int64_t* __restrict__ state_begin, const double* __restrict__ depth,
                                                          const double* __restrict__ t_near, int H, int W,
                                                          const double* __restrict__ cam_spheres, int N, double near, double tol, int cull,
                                                          uint8_t* __restrict__ state) {
    __shared__ double tile[RF_CHUNK * 4];
    __shared__ int counts[RF_BLOCK / 64];
    // (lanes past the last node of the volume repeat it and write nothing)
    const volume_node n = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, RF_BLOCK);
    const int m = n.m, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const omgx_mesh ms = meshes[m];
    double p[3];
    volume_node_point(ms, n.idc, p);
    uint8_t* __restrict__ mine = state + state_begin[m];  // (a 64-bit offset: the states may lie beyond 2^32 elements)
    const uint8_t old = mine[n.idc];
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (cull) robot_run_box(ms.dims, (uint32_t)n.id0, (uint32_t)min(n.id0 + RF_BLOCK - 1, n.total - 1), lo, hi);  // uniform
    bool inside = false, front = false;
    const int v0 = view_range[2 * m], v1 = v0 + view_range[2 * m + 1];
    const int64_t image = (int64_t)H * W;
    for (int v = v0; v < v1; ++v) {  // (uniform: the view row comes through scalar loads)
        const double* __restrict__ view = views + (int64_t)v * 16;
        double q[3], ball[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        bool f;
        robot_view_front(view, depth + v * image, t_near + v * image, H, W, p, near, tol, q, &f);
        front = front || f;
        if (cull) robot_run_ball(ms, lo, hi, view, ball);  // uniform
        const double* __restrict__ sv = cam_spheres + (int64_t)v * N * 4;
        for (int n0 = 0; n0 < N; n0 += RF_CHUNK) {
            const int cnt = min(RF_CHUNK, N - n0);
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            bool keep = false;
            if (tid < cnt) {
                for (int k = 0; k < 4; ++k) s[k] = sv[(int64_t)(n0 + tid) * 4 + k];
                keep = !(cull && robot_run_drops(ball, s));
            }
            const unsigned long long mask = __ballot(keep);
            __syncthreads();  // the walk of the chunk before is over
            if (lane == 0) counts[wave] = __popcll(mask);
            __syncthreads();
            int base = 0, kept = 0;
            for (int w = 0; w < RF_BLOCK / 64; ++w) {
                const int c = counts[w];
                base += w < wave ? c : 0, kept += c;
            }
            if (keep) {
                const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));  // slot < kept <= cnt <= RF_CHUNK
                tile[slot * 4] = s[0], tile[slot * 4 + 1] = s[1], tile[slot * 4 + 2] = s[2], tile[slot * 4 + 3] = s[3] * s[3];
            }
            __syncthreads();
            kept = __builtin_amdgcn_readfirstlane(kept);
            for (int k = 0; k < kept; ++k) inside = inside || robot_inside(q, tile[k * 4], tile[k * 4 + 1], tile[k * 4 + 2], tile[k * 4 + 3]);
        }
    }
    if (n.live) mine[n.id] = robot_new_state(old, inside, front);
}

// [count][4] spheres on the host: finite, radius >= 0.
bool spheres_valid(const double* h, int64_t count) {
    if (!image_all_finite(h, count * 4)) return false;
    for (int64_t k = 0; k < count; ++k)
        if (h[k * 4 + 3] < 0.0) return false;
    return true;
}

}  // namespace

extern "C" int omgx_render_spheres(const double* local, const double* h_local, const int32_t* link, const int32_t* h_link, int32_t num_spheres,
                                   const double* link_poses, const double* h_link_poses, int32_t num_configs, const omgx_camera* cameras,
                                   const omgx_camera* h_cameras, const int32_t* config_of_view, const int32_t* h_config_of_view,
                                   int32_t num_views, int32_t H, int32_t W, double pad, double t_min, int32_t cull, double* cam_spheres,
                                   double* t_near, int32_t* sphere, void* stream) {
    const int32_t N = num_spheres, C = num_configs, V = num_views;
    if (N < 0 || C < 0 || V < 0) return OMGX_ERR_INVALID;
    if (!std::isfinite(pad) || pad < 0.0 || !std::isfinite(t_min) || t_min < 0.0) return OMGX_ERR_INVALID;
    if (N > 0 && (!local || !h_local || !link || !h_link)) return OMGX_ERR_INVALID;
    if (C > 0 && (!link_poses || !h_link_poses)) return OMGX_ERR_INVALID;
    if (V > 0 && (!cameras || !h_cameras || !config_of_view || !h_config_of_view || !t_near || !sphere || H < 1 || W < 1)) return OMGX_ERR_INVALID;
    if (V > 0 && N > 0 && !cam_spheres) return OMGX_ERR_INVALID;
    if (!spheres_valid(h_local, N) || !image_all_finite(h_link_poses, (int64_t)C * OMGX_NUM_LINKS * 16)) return OMGX_ERR_INVALID;
    for (int32_t n = 0; n < N; ++n)
        if (h_link[n] < 0 || h_link[n] >= OMGX_NUM_LINKS) return OMGX_ERR_INVALID;
    for (int32_t v = 0; v < V; ++v) {
        if (image_check_camera(h_cameras[v]) != OMGX_OK || h_config_of_view[v] < 0 || h_config_of_view[v] >= C) return OMGX_ERR_INVALID;
    }
    if (V == 0) return OMGX_OK;
    if (N > OMGX_ROBOT_MAX_SPHERES || image_check_grid(V, H, W) != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    int tiles_x;
    const int64_t tiles = image_tile_grid(H, W, &tiles_x);
    hipLaunchKernelGGL(k_render_spheres, dim3((unsigned)tiles, (unsigned)V), dim3(RF_BLOCK), 0, (hipStream_t)stream, local, link,
                       (int)N, link_poses, (int)C, cameras, config_of_view, (int)H, (int)W, tiles_x, pad, t_min, (int)cull, cam_spheres, t_near,
                       sphere);
    OMGX_CHECK_LAUNCH("k_render_spheres");
    return OMGX_OK;
}

extern "C" int omgx_clear_robot(const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, const double* views,
                                const double* h_views, int32_t num_views, const int32_t* view_range, const int32_t* h_view_range,
                                const int64_t* state_begin, const int64_t* h_state_begin, const double* depth, const double* t_near, int32_t H,
                                int32_t W, const double* cam_spheres, const double* h_cam_spheres, int32_t num_spheres, double near, double tol,
                                int32_t cull, uint8_t* state, int64_t state_elems, void* stream) {
    const int32_t M = num_volumes, V = num_views, N = num_spheres;
    if (M < 0 || V < 0 || N < 0 || state_elems < 0 || !std::isfinite(near) || !std::isfinite(tol)) return OMGX_ERR_INVALID;
    if (M > 0 && (!volumes || !h_volumes || !view_range || !h_view_range || !state_begin || !h_state_begin || !state)) return OMGX_ERR_INVALID;
    if (V > 0 && (!views || !h_views || !depth || !t_near || H < 1 || W < 1)) return OMGX_ERR_INVALID;
    if (V > 0 && N > 0 && !cam_spheres) return OMGX_ERR_INVALID;
    if (h_cam_spheres && !spheres_valid(h_cam_spheres, (int64_t)V * N)) return OMGX_ERR_INVALID;
    const int images = mesh_check_views(h_views, V, H, W, h_view_range, M);
    if (images == OMGX_ERR_INVALID || M == 0) return images == OMGX_ERR_INVALID ? images : N > OMGX_ROBOT_MAX_SPHERES ? OMGX_ERR_UNSUPPORTED : images;
    int64_t wg = 0;
    const int status = mesh_check_batch(h_volumes, M, h_state_begin, state_elems, -1, RF_BLOCK, &wg);
    if (status == OMGX_ERR_INVALID) return status;
    if (status != OMGX_OK || images != OMGX_OK || N > OMGX_ROBOT_MAX_SPHERES) return OMGX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_clear_robot, dim3((unsigned)wg), dim3(RF_BLOCK), 0, (hipStream_t)stream, volumes, (int)M, views, view_range, state_begin,
                       depth, t_near, (int)H, (int)W, cam_spheres, (int)N, near, tol, (int)cull, state);
    OMGX_CHECK_LAUNCH("k_clear_robot");
    return OMGX_OK;
}
