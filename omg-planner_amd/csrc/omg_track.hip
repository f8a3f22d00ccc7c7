// omg_track.hip — camera tracking: live depth frames aligned to the model's rendering by projective point-to-plane ICP
// (include/omg_hip.h section 25).
//
// One Levenberg-Marquardt loop per view cannot live in one workgroup as k_register_clouds' does: a frame has 10^5 pixels per pass,
// not 10^2 points.  So a pass is a launch of its own and the loop's variables (track_state, omg_track_body.h) live in the workspace:
//   k_track_init  one block per view: poses0 into the view's state
//   k_track_pass  grid (chunks, V), 256 threads, 8 used pixels per lane in the order l, l + 256, ...; the view's done word, trial
//                 pose and intrinsics are uniform: scalar loads, and a workgroup of a finished view returns at once.  A lane keeps
//                 the 28 float64 partials and a count in registers; they are summed by shuffles inside each wave (x[l] += x[l + s],
//                 s = 32 ... 1), the four wave totals go through LDS and are added as ((w0 + w1) + w2) + w3; one row of TRACK_ROW
//                 doubles per (view, chunk) goes to the workspace
//   k_track_step  one wave per view: lane k < 29 adds the view's chunk rows left to right (the loads issued ahead of the
//                 additions), the totals reach every lane by shuffles and every lane runs the same turn (track_turn), so control
//                 flow is uniform; lane 0 writes the state, and poses_out and stats_out at the turn the view stops
// The entry point enqueues init and max_passes + 1 times (pass, step) on one stream: the stream's order is the only barrier, no
// workgroup waits on another, and the host never learns when a view converged.  The arithmetic is omg_track_body.h and
// omg_register_body.h: the bits of omg-planner_amd/tracking.py.  Plain loads and stores only, no atomics.
#include "omg_host.h"
#include "omg_image_body.h"
#include "omg_track_body.h"

#pragma clang fp contract(off)

#define TR_BLOCK TRACK_LANES
#define TR_WAVES (TR_BLOCK / 64)
#define TR_CHUNK OMGX_TRACK_PIXELS_PER_WORKGROUP
#define TR_PER_LANE (TR_CHUNK / TR_BLOCK)
#define TR_AHEAD 8  // chunk rows whose loads k_track_step issues before it adds them
static_assert(TR_BLOCK == OMGX_REGISTER_THREADS && TR_CHUNK % TR_BLOCK == 0 && TR_PER_LANE == 8, "lane l takes the chunk's pixels l, l + 256, ...");
static_assert(OMGX_TRACK_STATS == OMGX_REGISTER_STATS && OMGX_TRACK_MAX_PASSES == OMGX_REGISTER_MAX_PASSES, "one loop, one stats row");
static_assert(REG_NPART + 1 <= TRACK_ROW, "28 sums and the count in a row");

namespace {

__global__ __launch_bounds__(64) void k_track_init(const double* __restrict__ poses0, double lambda0, track_state* __restrict__ states) {
    if (threadIdx.x != 0) return;
    track_state s;
    track_begin(s, poses0 + (int64_t)blockIdx.x * 12, lambda0);
    states[blockIdx.x] = s;
}

__global__ __launch_bounds__(TR_BLOCK) void k_track_pass(const track_state* __restrict__ states, const double* __restrict__ intrinsics,
                                                          const double* __restrict__ live_depth, const double* __restrict__ live_normals,
                                                          const double* __restrict__ model_depth, const double* __restrict__ model_normals,
                                                          int H, int W, int Wu, int64_t used, int stride, double dist2, double cos_min,
                                                          double* __restrict__ rows) {
    __shared__ double wave_sum[TR_WAVES][REG_NPART];
    __shared__ int32_t wave_count[TR_WAVES];
    const int v = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the view's done word, trial pose and intrinsics: uniform addresses, scalar loads
    const track_state* __restrict__ st = states + v;
    if (st->done) return;
    double P[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = st->trial[i];
    const double* __restrict__ k = intrinsics + (int64_t)v * 4;
    const int64_t image = (int64_t)v * H * W;
    track_image I;
    I.zl = live_depth + image, I.nl = live_normals ? live_normals + image * 3 : nullptr;
    I.zm = model_depth + image, I.nm = model_normals + image * 3;
    I.fx = k[0], I.fy = k[1], I.cx = k[2], I.cy = k[3], I.H = H, I.W = W;
    reg_sums acc;
    reg_clear(acc);
    const int64_t first = (int64_t)blockIdx.x * TR_CHUNK + tid;
#pragma unroll  // (kept as a loop the compiler holds 256 VGPRs; unrolled 150)
    for (int j = 0; j < TR_PER_LANE; ++j) {
        const int64_t u = first + j * TR_BLOCK;
        if (u < used) {
            int r, c;
            track_used_pixel(u, Wu, stride, &r, &c);  // r <= ((H - 1) / stride) * stride < H, c alike
            track_pixel(I, P, r, c, dist2, cos_min, acc);
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int i = 0; i < REG_NPART; ++i) acc.x[i] = acc.x[i] + __shfl_down(acc.x[i], s, 64);
        acc.count += __shfl_down(acc.count, s, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < REG_NPART; ++i) wave_sum[wave][i] = acc.x[i];
        wave_count[wave] = acc.count;
    }
    __syncthreads();
    double* __restrict__ out = rows + ((int64_t)v * gridDim.x + blockIdx.x) * TRACK_ROW;
    if (tid < REG_NPART)
        out[tid] = ((wave_sum[0][tid] + wave_sum[1][tid]) + wave_sum[2][tid]) + wave_sum[3][tid];
    else if (tid == REG_NPART)
        out[tid] = (double)(((wave_count[0] + wave_count[1]) + wave_count[2]) + wave_count[3]);  // (<= 2048: exact)
    else if (tid < TRACK_ROW)
        out[tid] = 0.0;
}

__global__ __launch_bounds__(64) void k_track_step(track_state* states, const double* __restrict__ rows, int chunks, double step_tol,
                                                   int max_passes, double* poses_out, double* stats_out) {
    const int v = blockIdx.x, lane = threadIdx.x;
    track_state* st = states + v;
    if (st->done) return;  // (uniform)
    // lane k adds column k of the view's chunk rows left to right, beginning with chunk 0's; the count (column 28) is a sum of
    // integers below 2^31 in doubles: exact
    const double* __restrict__ mine = rows + (int64_t)v * chunks * TRACK_ROW + (lane < TRACK_ROW ? lane : 0);
    double total = mine[0];
    for (int c0 = 1; c0 < chunks; c0 += TR_AHEAD) {
        double x[TR_AHEAD];
#pragma unroll
        for (int q = 0; q < TR_AHEAD; ++q) x[q] = mine[(int64_t)(c0 + q < chunks ? c0 + q : c0) * TRACK_ROW];
#pragma unroll
        for (int q = 0; q < TR_AHEAD; ++q)
            if (c0 + q < chunks) total = total + x[q];
    }
    reg_sums tri;
#pragma unroll
    for (int i = 0; i < REG_NPART; ++i) tri.x[i] = __shfl(total, i, 64);
    tri.count = (int32_t)__shfl(total, REG_NPART, 64);
    track_state s = *st;  // every lane the same values: the turn's control flow is uniform
    const bool stop = track_turn(s, tri, step_tol, max_passes);
    if (lane == 0) {
        *st = s;
        if (stop) {
            for (int i = 0; i < 12; ++i) poses_out[(int64_t)v * 12 + i] = s.pose[i];
            track_stats(s, stats_out + (int64_t)v * OMGX_TRACK_STATS);
        }
    }
}

bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

int64_t chunks_of(int32_t H, int32_t W, int32_t stride) {
    const int64_t used = (int64_t)((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    return (used + TR_CHUNK - 1) / TR_CHUNK;
}

}  // namespace

extern "C" int64_t omgx_track_workspace_bytes(int32_t num_views, int32_t H, int32_t W, int32_t stride) {
    if (num_views < 0 || stride < 1 || (num_views > 0 && (H < 1 || W < 1))) return OMGX_ERR_INVALID;
    if (num_views == 0) return 0;
    if (image_check_grid(num_views, H, W) != OMGX_OK || !image_pixels_fit(num_views, H, W)) return OMGX_ERR_UNSUPPORTED;
    return (int64_t)num_views * ((int64_t)sizeof(track_state) + chunks_of(H, W, stride) * TRACK_ROW * (int64_t)sizeof(double));
}

extern "C" int omgx_track_cameras(const double* intrinsics, const double* h_intrinsics, const double* live_depth, const double* live_normals,
                                  const double* model_depth, const double* model_normals, int32_t num_views, int32_t H, int32_t W,
                                  int32_t stride, const double* poses0, double dist_max, double cos_min, double lambda0, double step_tol,
                                  int32_t max_passes, void* workspace, int64_t workspace_bytes, double* poses_out, double* stats_out,
                                  void* stream) {
    const int32_t V = num_views;
    if (V < 0 || stride < 1 || workspace_bytes < 0) return OMGX_ERR_INVALID;
    if (max_passes < 0 || max_passes > OMGX_TRACK_MAX_PASSES) return OMGX_ERR_INVALID;
    if (!(dist_max > 0.0) || !std::isfinite(dist_max) || !(lambda0 > 0.0) || !std::isfinite(lambda0) || cos_min != cos_min) return OMGX_ERR_INVALID;
    if (V > 0 && (!intrinsics || !h_intrinsics || !live_depth || !model_depth || !model_normals || !poses0 || !workspace || !poses_out ||
                  !stats_out || H < 1 || W < 1))
        return OMGX_ERR_INVALID;
    if (V > 0 && image_check_rows(h_intrinsics, V, 4) != OMGX_OK) return OMGX_ERR_INVALID;
    if (V == 0) return OMGX_OK;
    if (image_check_grid(V, H, W) != OMGX_OK || !image_pixels_fit(V, H, W)) return OMGX_ERR_UNSUPPORTED;
    const int64_t need = omgx_track_workspace_bytes(V, H, W, stride);
    if (workspace_bytes < need) return OMGX_ERR_INVALID;
    const int64_t pixels = (int64_t)V * H * W;
    const struct { const void* p; int64_t n; } in[6] = {{intrinsics, (int64_t)V * 32}, {live_depth, pixels * 8}, {live_normals, pixels * 24},
                                                        {model_depth, pixels * 8}, {model_normals, pixels * 24}, {poses0, (int64_t)V * 96}},
                                               out[3] = {{poses_out, (int64_t)V * 96}, {stats_out, (int64_t)V * 64}, {workspace, need}};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 6; ++i)
            if (!(o == 0 && i == 5 && poses_out == poses0) && overlap(out[o].p, out[o].n, in[i].p, in[i].n)) return OMGX_ERR_INVALID;
        for (int q = o + 1; q < 3; ++q)
            if (overlap(out[o].p, out[o].n, out[q].p, out[q].n)) return OMGX_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const int Hu = (H - 1) / stride + 1, Wu = (W - 1) / stride + 1;
    const int64_t used = (int64_t)Hu * Wu;
    const int chunks = (int)chunks_of(H, W, stride);
    track_state* states = (track_state*)workspace;
    double* rows = (double*)((char*)workspace + (int64_t)V * (int64_t)sizeof(track_state));
    const double dist2 = dist_max * dist_max;
    hipLaunchKernelGGL(k_track_init, dim3((unsigned)V), dim3(64), 0, s, poses0, lambda0, states);
    OMGX_CHECK_LAUNCH("k_track_init");
    for (int32_t turn = 0; turn <= max_passes; ++turn) {
        hipLaunchKernelGGL(k_track_pass, dim3((unsigned)chunks, (unsigned)V), dim3(TR_BLOCK), 0, s, (const track_state*)states, intrinsics, live_depth,
                           live_normals, model_depth, model_normals, (int)H, (int)W, Wu, used, (int)stride, dist2, cos_min, rows);
        OMGX_CHECK_LAUNCH("k_track_pass");
        hipLaunchKernelGGL(k_track_step, dim3((unsigned)V), dim3(64), 0, s, states, (const double*)rows, chunks, step_tol, (int)max_passes, poses_out,
                           stats_out);
        OMGX_CHECK_LAUNCH("k_track_step");
    }
    return OMGX_OK;
}
