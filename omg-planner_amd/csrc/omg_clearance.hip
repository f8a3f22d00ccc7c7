// omg_clearance.hip — plan clearance: the arm's spheres against a scene table's volumes and against one another
// (include/omg_hip.h section 24).
//
// k_sphere_clearance: one workgroup of 256 threads per run of CLR_CONFIGS = 4 configurations, one WAVE per configuration: its
//                     scene, the scene's records and the flags come through uniform loads.  The sphere table (local, link) is
//                     the same for every configuration: the workgroup stages it in LDS a chunk of OMGX_ROBOT_SPHERE_CHUNK at a
//                     time, once for its four configurations.  Lanes take the chunk's spheres lane, lane + 64, ...: the sphere
//                     into the world (and to world_out: each (configuration, sphere) has one wave, one lane), then the scene's
//                     records in order.  One ballot per (64 spheres, record) skips a record none of the lanes reaches
//                     (e <= beyond); a lane that does not reach contributes nothing either way, so the skip changes no bit.
//                     Each lane keeps its two best triples (clear, margin) in registers; the wave merges them by a butterfly
//                     of shuffles under the replace rule, which is a total order, so the order of the merge is free; lane 0
//                     writes the six outputs.
// k_self_clearance:   one workgroup per configuration.  The N <= OMGX_CLEARANCE_MAX_SELF world spheres (radius + pad) and their
//                     links go into LDS (32 KB + 1 KB + the pair table).  For i = 0, 1, ... thread t takes j = i + 1 + t,
//                     i + 1 + t + 256, ...; the four waves' results meet in LDS and thread 0 merges them in wave order.
// The arithmetic is omg_clearance_body.h: the bits of omg-planner_amd/clearance.py.  Plain loads and stores only, no atomics;
// every output element is written by exactly one thread.  Offsets into the pool are 64-bit (vcam_sample).
#include "omg_host.h"
#include "omg_image_body.h"
#include "omg_clearance_body.h"

#pragma clang fp contract(off)

#define CLR_BLOCK 256
#define CLR_CONFIGS (CLR_BLOCK / 64)
#define CLR_CHUNK OMGX_ROBOT_SPHERE_CHUNK
static_assert(CLR_CHUNK == CLR_BLOCK, "a sphere of a chunk per thread");
static_assert(sizeof(omgx_object) == 184, "records as include/omg_hip.h documents them");
static_assert(OMGX_CLEARANCE_MAX_SELF * 33 + 128 <= 64 * 1024, "the self op's spheres fit static LDS");

namespace {

// The replace rule across the wave: afterwards every lane holds the wave's best.
__device__ __forceinline__ void wave_best(clear_best& m) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double v = __shfl_xor(m.v, s);
        const int32_t a = __shfl_xor(m.a, s), b = __shfl_xor(m.b, s);
        clear_take(m, v, a, b);
    }
}

__global__ __launch_bounds__(CLR_BLOCK) void k_sphere_clearance(
    const omgx_object* __restrict__ objects, int num_objects, const int32_t* __restrict__ scene_begin, int num_scenes,
    const float* __restrict__ pool, int64_t pool_elems, const uint8_t* __restrict__ visible, const int32_t* __restrict__ scene_of_config,
    int B, const double* __restrict__ link_poses, const double* __restrict__ local, const int32_t* __restrict__ link, int N,
    const double* __restrict__ pad, double beyond, int cull, double* __restrict__ clear, int32_t* __restrict__ clear_sphere,
    int32_t* __restrict__ clear_object, double* __restrict__ margin, int32_t* __restrict__ margin_sphere,
    int32_t* __restrict__ margin_object, double* __restrict__ world_out) {
    __shared__ double tile[CLR_CHUNK * 4];
    __shared__ int32_t tile_link[CLR_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t mine = (int64_t)blockIdx.x * CLR_CONFIGS + wave;
    const bool live = mine < B;                           // (a wave past the last configuration redoes it and writes nothing)
    const int64_t b = live ? mine : (int64_t)B - 1;
    // (the entry point has checked the host copies; clamped once more so that no index can read outside the table)
    const int s = min(max(__builtin_amdgcn_readfirstlane(scene_of_config[b]), 0), num_scenes - 1);
    const int first = max(scene_begin[s], 0);
    const int count = min(scene_begin[s + 1], num_objects) - first;
    const double* __restrict__ poses = link_poses + b * (OMGX_NUM_LINKS * 16);

    clear_best bc = clear_none(), bm = clear_none();
    for (int n0 = 0; n0 < N; n0 += CLR_CHUNK) {
        const int cnt = min(CLR_CHUNK, N - n0);
        __syncthreads();  // the walk of the chunk before is over
        if (tid < cnt) {
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[tid * 4 + k] = local[(int64_t)(n0 + tid) * 4 + k];
            tile_link[tid] = min(max(link[n0 + tid], 0), OMGX_NUM_LINKS - 1);
        }
        __syncthreads();
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            const bool valid = j0 + lane < cnt;  // (a lane past the chunk's end redoes its last sphere and contributes nothing)
            const int at = min(j0 + lane, cnt - 1), n = n0 + at;
            const int l = tile_link[at];
            const double r = tile[at * 4 + 3];
            double w[3];
            clear_world(poses + l * 16, tile + at * 4, w);
            if (valid && live && world_out) {
                double* __restrict__ out = world_out + (b * N + n) * 4;
                out[0] = w[0], out[1] = w[1], out[2] = w[2], out[3] = r;
            }
            const double rm = pad ? r + pad[b * OMGX_NUM_LINKS + l] : r;
            for (int k = 0; k < count; ++k) {  // uniform: the record comes through scalar loads
                const omgx_object* __restrict__ ob = objects + ((int64_t)first + k);
                if (!clear_record_used(*ob, visible, (int64_t)first + k, pool_elems)) continue;
                vcam_grid G;
                vcam_set_grid(ob->lo, ob->dim, ob->inv_delta, ob->grid_offset, G);
                vcam_ray R;
                const double e = clear_reach(G, ob->pose_inv, w, R);
                const bool reach = valid && e <= beyond;
                if (cull && __ballot(reach) == 0ull) continue;  // no sphere of these 64 is within `beyond` of the grid
                const double d = vcam_sample<false>(G, pool, R, 0.0, nullptr) - e;  // (clamped: inside the grid for every lane)
                if (reach) {
                    clear_take(bc, d - r, n, k);
                    clear_take(bm, d - rm, n, k);
                }
            }
        }
    }
    wave_best(bc);
    wave_best(bm);
    if (live && lane == 0) {
        clear[b] = bc.v, clear_sphere[b] = bc.a, clear_object[b] = bc.b;
        if (margin) margin[b] = bm.v, margin_sphere[b] = bm.a, margin_object[b] = bm.b;
    }
}

__global__ __launch_bounds__(CLR_BLOCK) void k_self_clearance(const double* __restrict__ world, const int32_t* __restrict__ link, int N,
                                                              const uint8_t* __restrict__ pairs, const double* __restrict__ pad,
                                                              double* __restrict__ self_clear, int32_t* __restrict__ sphere_i,
                                                              int32_t* __restrict__ sphere_j) {
    __shared__ double sp[OMGX_CLEARANCE_MAX_SELF * 4];
    __shared__ uint8_t lk[OMGX_CLEARANCE_MAX_SELF];
    __shared__ uint8_t on[OMGX_NUM_LINKS * OMGX_NUM_LINKS];
    __shared__ double red_v[CLR_CONFIGS];
    __shared__ int32_t red_a[CLR_CONFIGS], red_b[CLR_CONFIGS];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int n = tid; n < N; n += CLR_BLOCK) {
        const double* __restrict__ c = world + (b * N + n) * 4;
        const int l = min(max(link[n], 0), OMGX_NUM_LINKS - 1);
        sp[n * 4] = c[0], sp[n * 4 + 1] = c[1], sp[n * 4 + 2] = c[2];
        sp[n * 4 + 3] = c[3] + (pad ? pad[b * OMGX_NUM_LINKS + l] : 0.0);
        lk[n] = (uint8_t)l;
    }
    if (tid < OMGX_NUM_LINKS * OMGX_NUM_LINKS) on[tid] = pairs[tid];
    __syncthreads();
    clear_best best = clear_none();
    for (int i = 0; i + 1 < N; ++i) {  // (sphere i is read by all lanes at one address: a broadcast)
        const uint8_t* __restrict__ row = on + lk[i] * OMGX_NUM_LINKS;
        for (int j = i + 1 + tid; j < N; j += CLR_BLOCK)
            if (row[lk[j]]) clear_take(best, clear_gap(sp + i * 4, sp + j * 4), i, j);
    }
    wave_best(best);
    if ((tid & 63) == 0) red_v[tid >> 6] = best.v, red_a[tid >> 6] = best.a, red_b[tid >> 6] = best.b;
    __syncthreads();
    if (tid == 0) {
        clear_best m = clear_none();
        for (int w = 0; w < CLR_CONFIGS; ++w) clear_take(m, red_v[w], red_a[w], red_b[w]);
        self_clear[b] = m.v, sphere_i[b] = m.a, sphere_j[b] = m.b;
    }
}

// [N] links on the host: inside [0, OMGX_NUM_LINKS).
bool links_valid(const int32_t* h_link, int32_t N) {
    for (int32_t n = 0; n < N; ++n)
        if (h_link[n] < 0 || h_link[n] >= OMGX_NUM_LINKS) return false;
    return true;
}

}  // namespace

extern "C" int omgx_sphere_clearance(const omgx_object* objects, const omgx_object* h_objects, int32_t num_objects, const int32_t* scene_begin,
                                     const int32_t* h_scene_begin, int32_t num_scenes, const float* pool, int64_t pool_elems,
                                     const uint8_t* visible, const uint8_t* h_visible, const int32_t* scene_of_config,
                                     const int32_t* h_scene_of_config, int32_t num_configs, const double* link_poses, const double* local,
                                     const double* h_local, const int32_t* link, const int32_t* h_link, int32_t num_spheres, const double* pad,
                                     double beyond, int32_t cull, double* clear, int32_t* clear_sphere, int32_t* clear_object, double* margin,
                                     int32_t* margin_sphere, int32_t* margin_object, double* world_out, void* stream) {
    const int32_t S = num_scenes, B = num_configs, N = num_spheres;
    if (num_objects < 0 || S < 0 || B < 0 || N < 0 || pool_elems < 0) return OMGX_ERR_INVALID;
    if (!std::isfinite(beyond) || beyond < 0.0) return OMGX_ERR_INVALID;
    if ((visible == nullptr) != (h_visible == nullptr)) return OMGX_ERR_INVALID;
    if (num_objects > 0 && (!objects || !h_objects)) return OMGX_ERR_INVALID;
    if (pool_elems > 0 && !pool) return OMGX_ERR_INVALID;
    if (S > 0 && (!scene_begin || !h_scene_begin)) return OMGX_ERR_INVALID;
    if (N > 0 && (!local || !h_local || !link || !h_link)) return OMGX_ERR_INVALID;
    if (B > 0 && (!scene_of_config || !h_scene_of_config || !link_poses || !clear || !clear_sphere || !clear_object)) return OMGX_ERR_INVALID;
    if (B > 0 && ((pad == nullptr) != (margin == nullptr) || (pad == nullptr) != (margin_sphere == nullptr) ||
                  (pad == nullptr) != (margin_object == nullptr)))
        return OMGX_ERR_INVALID;
    if (N > 0) {
        if (!image_all_finite(h_local, (int64_t)N * 4) || !links_valid(h_link, N)) return OMGX_ERR_INVALID;
        for (int32_t n = 0; n < N; ++n)
            if (h_local[(int64_t)n * 4 + 3] < 0.0) return OMGX_ERR_INVALID;
    }
    for (int32_t b = 0; b < B; ++b)
        if (h_scene_of_config[b] < 0 || h_scene_of_config[b] >= S) return OMGX_ERR_INVALID;
    if (S > 0) {
        if (h_scene_begin[0] < 0 || h_scene_begin[S] > num_objects) return OMGX_ERR_INVALID;
        for (int32_t s = 0; s < S; ++s)
            if (h_scene_begin[s + 1] < h_scene_begin[s]) return OMGX_ERR_INVALID;
        for (int32_t o = h_scene_begin[0]; o < h_scene_begin[S]; ++o) {
            const omgx_object& r = h_objects[o];
            if (h_visible ? h_visible[o] == 0 : r.disabled != 0) continue;
            if (!std::isfinite(r.inv_delta) || !(r.inv_delta > 0.0) || !vcam_grid_usable(r.dim, r.grid_offset, pool_elems)) return OMGX_ERR_INVALID;
        }
    }
    if (N > OMGX_ROBOT_MAX_SPHERES) return OMGX_ERR_UNSUPPORTED;
    if (B == 0) return OMGX_OK;
    const unsigned grid = (unsigned)(((int64_t)B + CLR_CONFIGS - 1) / CLR_CONFIGS);
    hipLaunchKernelGGL(k_sphere_clearance, dim3(grid), dim3(CLR_BLOCK), 0, (hipStream_t)stream, objects, (int)num_objects, scene_begin, (int)S, pool,
                       pool_elems, visible, scene_of_config, (int)B, link_poses, local, link, (int)N, pad, beyond, (int)cull, clear, clear_sphere,
                       clear_object, margin, margin_sphere, margin_object, world_out);
    OMGX_CHECK_LAUNCH("k_sphere_clearance");
    return OMGX_OK;
}

extern "C" int omgx_self_clearance(const double* world, int32_t num_configs, const int32_t* link, const int32_t* h_link, int32_t num_spheres,
                                   const uint8_t* pairs, const double* pad, double* self_clear, int32_t* sphere_i, int32_t* sphere_j,
                                   void* stream) {
    const int32_t B = num_configs, N = num_spheres;
    if (B < 0 || N < 0) return OMGX_ERR_INVALID;
    if (N > 0 && (!link || !h_link)) return OMGX_ERR_INVALID;
    if (B > 0 && (!pairs || !self_clear || !sphere_i || !sphere_j || (N > 0 && !world))) return OMGX_ERR_INVALID;
    if (N > 0 && !links_valid(h_link, N)) return OMGX_ERR_INVALID;
    if (N > OMGX_CLEARANCE_MAX_SELF) return OMGX_ERR_UNSUPPORTED;
    if (B == 0) return OMGX_OK;
    hipLaunchKernelGGL(k_self_clearance, dim3((unsigned)B), dim3(CLR_BLOCK), 0, (hipStream_t)stream, world, link, (int)N, pairs, pad, self_clear,
                       sphere_i, sphere_j);
    OMGX_CHECK_LAUNCH("k_self_clearance");
    return OMGX_OK;
}
