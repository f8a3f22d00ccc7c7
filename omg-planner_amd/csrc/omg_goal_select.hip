// omg_goal_select.hip — the selection of Planner.setup_goal_set on the device: omgx_select_goals (include/omg_hip.h, section 11).
//
// One workgroup (four waves) per scene.  The reference (omg/planner.py:526-575, goalset.select_goals) walks the collision-free
// goals in order and keeps a goal iff no goal kept before it lies closer than 0.5 (joint-space L2 over all nine entries); kept
// goal p >= 1 records the index of goal p - 1 (`indexes.append(j)`).  That greedy walk is sequential by definition; here it runs
// in blocks of 64 candidates, each block in three steps that give exactly the sequential result:
//   (a) all four waves test the block's candidates against the goals kept by earlier blocks (wave w takes kept goals w, w+4, ..);
//   (b) wave 0 resolves the block in order: lane l holds the mask of the earlier in-block candidates within 0.5 of candidate l,
//       and a 64-step scan over those masks decides which candidates survive (j is kept iff it passed (a) and no kept j' < j
//       of the block is near it);
//   (c) the kept goals join the kept set (LDS for the first SEL_LDS_KEPT, their rows in the workspace beyond) and emit their
//       predecessor's row.
// "Closer than 0.5" is decided without a square root: s < 0.25 for s = (((d0²+d1²)+(d2²+d3²))+((d4²+d5²)+(d6²+d7²)))+d8², the
// order in which numpy's linalg.norm(axis=-1) sums nine squares, and RN(sqrt(s)) < 0.5 <=> s < 0.25 for a correctly rounded
// sqrt.  The file is compiled with -ffp-contract=off: the squares and sums are plain IEEE double operations.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "omg_host.h"

namespace {

constexpr int SEL_THREADS = 256;   // four waves
constexpr int SEL_BLOCK = 64;      // candidates resolved per step (one wave)
constexpr int SEL_LDS_KEPT = 512;  // kept goals whose nine entries are cached in LDS (36 KB); later ones are read from `goals`

__device__ __forceinline__ double dist2(const double* a, const double* b) {
    double q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double d = a[k] - b[k];
        q[k] = d * d;
    }
    return (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) + q[8];
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int lane) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const int hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}

__global__ __launch_bounds__(SEL_THREADS) void k_select_goals(const double* __restrict__ goals, const int32_t* __restrict__ goal_count,
                                                             int32_t checked, const float* __restrict__ collides, int32_t G,
                                                             double allow, int32_t diversity, int32_t* __restrict__ candidates,
                                                             int32_t* __restrict__ num_candidates, int32_t* __restrict__ num_free,
                                                             int32_t* __restrict__ workspace) {
    __shared__ double s_kept[SEL_LDS_KEPT][9];
    __shared__ double s_block[SEL_BLOCK][9];
    __shared__ int s_near[4][SEL_BLOCK];
    __shared__ int s_wave[4];
    __shared__ unsigned long long s_keep;

    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = goal_count[s];
    if (n < 0 || n > G) {  // only without a host copy of the counts (checked == 0): reported, nothing read
        if (tid == 0 && !checked) num_free[s] = num_candidates[s] = -1;
        return;
    }
    const double* g = goals + (int64_t)s * G * 9;
    const float* col = collides ? collides + (int64_t)s * G : nullptr;
    int32_t* out = candidates + (int64_t)s * G;
    int32_t* fl = diversity ? workspace + (int64_t)s * G * 2 : out;  // the collision-free rows, in order
    int32_t* kept = diversity ? fl + G : nullptr;                    // the kept rows (read back beyond SEL_LDS_KEPT)
    const unsigned long long below = (1ull << lane) - 1ull;

    // the collision filter: an ordered compaction, 256 rows per step (ballot + popcount in the wave, wave totals through LDS)
    int nf = 0;
    for (int base = 0; base < n; base += SEL_THREADS) {
        const int i = base + tid;
        const bool f = i < n && (!col || (double)col[i] <= allow);
        const unsigned long long m = __ballot(f);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = nf;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        if (f) fl[off + __popcll(m & below)] = i;
        nf += (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        __syncthreads();
    }
    if (!diversity || nf == 0) {
        if (tid == 0) {
            num_free[s] = nf;
            num_candidates[s] = diversity ? 0 : nf;
        }
        return;
    }

    // the diversity filter: free[0] seeds the kept set
    if (tid < 9) s_kept[0][tid] = g[(int64_t)fl[0] * 9 + tid];
    if (tid == 0) kept[0] = fl[0];
    int nk = 1;
    __syncthreads();
    for (int p0 = 1; p0 < nf; p0 += SEL_BLOCK) {
        const int p = p0 + lane;
        const bool valid = p < nf;
        double c[9];
        const int64_t row = valid ? fl[p] : 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) c[k] = valid ? g[row * 9 + k] : 0.0;
        if (wave == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) s_block[lane][k] = c[k];
        }
        // (a) against the goals kept by earlier blocks
        bool near = false;
        if (valid) {
            const int lds_end = nk < SEL_LDS_KEPT ? nk : SEL_LDS_KEPT;
            for (int u = wave; u < lds_end && !near; u += 4) near = dist2(s_kept[u], c) < 0.25;
            for (int u = SEL_LDS_KEPT + wave; u < nk && !near; u += 4) {
                const double* kv = g + (int64_t)kept[u] * 9;
                double v[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) v[k] = kv[k];
                near = dist2(v, c) < 0.25;
            }
        }
        s_near[wave][lane] = near ? 1 : 0;
        __syncthreads();
        // (b) wave 0 resolves the block in order
        if (wave == 0) {
            const bool cand = valid && !(s_near[0][lane] | s_near[1][lane] | s_near[2][lane] | s_near[3][lane]);
            unsigned long long close = 0ull;  // earlier in-block candidates within 0.5 of this one
            for (int j = 0; j < SEL_BLOCK; ++j)
                if (j < lane && dist2(s_block[j], c) < 0.25) close |= 1ull << j;
            const unsigned long long alive = __ballot(cand);
            unsigned long long keep = 0ull;
            for (int j = 0; j < SEL_BLOCK; ++j) {
                const unsigned long long cj = readlane64(close, j);
                if (((alive >> j) & 1ull) && !(cj & keep)) keep |= 1ull << j;
            }
            if (lane == 0) s_keep = keep;
        }
        __syncthreads();
        // (c) append the kept goals; kept goal p emits row free[p - 1]
        const unsigned long long keep = s_keep;
        if (wave == 0 && ((keep >> lane) & 1ull)) {
            const int r = __popcll(keep & below);
            const int u = nk + r;
            kept[u] = (int32_t)row;
            if (u < SEL_LDS_KEPT) {
#pragma unroll
                for (int k = 0; k < 9; ++k) s_kept[u][k] = c[k];
            }
            out[u - 1] = fl[p - 1];
        }
        nk += __popcll(keep);
        __syncthreads();
    }
    if (tid == 0) {
        num_free[s] = nf;
        num_candidates[s] = nk - 1;
    }
}

}  // namespace

extern "C" int64_t omgx_select_goals_workspace_bytes(int32_t num_scenes, int32_t num_goals) {
    if (num_scenes <= 0 || num_goals <= 0) return 0;
    return (int64_t)num_scenes * num_goals * 2 * (int64_t)sizeof(int32_t);
}

extern "C" int omgx_select_goals(const double* goals, const int32_t* goal_count, const int32_t* h_goal_count, int32_t num_scenes,
                                 int32_t num_goals, const float* collides, double allow_collision_point, int32_t filter_diversity,
                                 int32_t* candidates, int32_t* num_candidates, int32_t* num_free, void* workspace, void* stream) {
    if (num_scenes < 0 || num_goals < 0 || num_goals > OMGX_SELECT_MAX_GOALS) return OMGX_ERR_INVALID;
    if (filter_diversity != 0 && filter_diversity != 1) return OMGX_ERR_INVALID;
    if (allow_collision_point != allow_collision_point) return OMGX_ERR_INVALID;  // NaN
    if (h_goal_count)
        for (int s = 0; s < num_scenes; ++s)
            if (h_goal_count[s] < 0 || h_goal_count[s] > num_goals) return OMGX_ERR_INVALID;
    if (num_scenes == 0) return OMGX_OK;
    if (!goal_count || !num_candidates || !num_free) return OMGX_ERR_INVALID;
    if (num_goals > 0 && (!goals || !candidates || (filter_diversity && !workspace))) return OMGX_ERR_INVALID;
    hipLaunchKernelGGL(k_select_goals, dim3((unsigned)num_scenes), dim3(SEL_THREADS), 0, (hipStream_t)stream, goals, goal_count,
                       h_goal_count ? 1 : 0, collides, num_goals, allow_collision_point, filter_diversity, candidates,
                       num_candidates, num_free, (int32_t*)workspace);
    OMGX_CHECK_LAUNCH("k_select_goals");
    return OMGX_OK;
}
