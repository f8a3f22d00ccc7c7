// omg_plane.hip — depth views to support planes, free masks and half-space volumes (include/omg_hip.h section 19).
//
// V depth images [H][W], pixels in row-major chunks of OMGX_PLANE_PIXELS_PER_WORKGROUP per workgroup, 256 lanes:
//   k_plane_hypotheses  one thread per (view, k): the plane of a pixel triple, counts = 0 for a live row and -1 for a void one
//   k_plane_score       one workgroup per (view, chunk): a lane computes the points of its pixels once and keeps them in registers
//                       (an invalid pixel as NaN: it is never an inlier); the view's planes pass through LDS in blocks of
//                       OMGX_PLANE_STAGE_HYPOTHESES, every lane reads the same row; per hypothesis a wave counts its inliers with
//                       __ballot and a population count, lane k % 64 keeps the count of hypothesis k, the four waves' counts meet in
//                       LDS and one integer atomicAdd per (workgroup, hypothesis) goes to `counts`
//   k_plane_select      one workgroup per view: the largest count, ties to the smallest k; the best plane and its anchor
//   k_plane_moments     one workgroup per (view, chunk): lane l adds its pixels l, l + 256, ... in order, the lanes are summed in
//                       the fixed shape of plane_tree, ten partials per chunk go to the workspace
//   k_plane_reduce      one workgroup per view adds the chunk partials left to right
//   k_plane_mask        one thread per pixel;  k_plane_volumes  one thread per node of a ragged batch of omgx_mesh records
// The arithmetic is omg_plane_body.h: the bits of planes.py.  Integer atomics only, so no result depends on the order of arrival;
// no spin-waits, no flags: the stream is the only barrier between the launches.
#include "omg_mesh_common.h"
#include "omg_plane_body.h"

#pragma clang fp contract(off)

#define PL_BLOCK 256
#define PL_CHUNK OMGX_PLANE_PIXELS_PER_WORKGROUP
#define PL_PER_LANE (PL_CHUNK / PL_BLOCK)
#define PL_STAGE OMGX_PLANE_STAGE_HYPOTHESES
#define PL_WAVES (PL_BLOCK / 64)
#define PL_PARTIALS (PLANE_SUMS + 1)  // nine sums and the count (an int64 in the tenth 8-byte cell)
#define PL_REDUCE_TILE 128            // chunks of a view in LDS at a time when their partials are added
static_assert(PL_BLOCK == PLANE_LANES && PL_CHUNK % PL_BLOCK == 0, "lane l takes the chunk's pixels l, l + 256, ...");
static_assert(PL_STAGE == 64 && PL_STAGE * 4 == PL_BLOCK, "a thread stages one double of a block of rows; lane k % 64 keeps hypothesis k");
static_assert(OMGX_PLANE_NODES_PER_WORKGROUP == PL_BLOCK, "one thread per node");

namespace {

// The point of pixel i (row-major, clamped into the image) of view v -> valid?
__device__ __forceinline__ bool pl_pixel(const double* __restrict__ intr, const double* __restrict__ depth, const uint8_t* __restrict__ skip, int v,
                                         int64_t N, int W, int64_t i, double* p) {
    const uint32_t ic = (uint32_t)(i < N ? i : N - 1);  // (N <= 2^31 - 1: 32-bit division)
    const int r = (int)(ic / (uint32_t)W), c = (int)(ic % (uint32_t)W);
    const int64_t at = (int64_t)v * N + ic;
    const bool valid = plane_point(intr + (int64_t)v * 4, depth[at], skip ? skip[at] != 0 : false, r, c, p);
    return valid && i < N;
}

__global__ __launch_bounds__(PL_BLOCK) void k_plane_hypotheses(const double* __restrict__ intr, const double* __restrict__ depth,
                                                               const uint8_t* __restrict__ skip, int64_t rows, int64_t N, int W, int K,
                                                               const int32_t* __restrict__ triples, double min_nn, const double* __restrict__ up,
                                                               double cos_min, double* __restrict__ planes, int32_t* __restrict__ counts) {
    const int64_t row = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (row >= rows) return;
    const int v = (int)(row / K);
    double p[3][3];
    bool valid = true;
    for (int x = 0; x < 3; ++x) {
        // the wrapper rejects indices outside the image; clamped here so that none can read outside it
        const int64_t i = min(max((int64_t)triples[row * 3 + x], (int64_t)0), N - 1);
        valid = pl_pixel(intr, depth, skip, v, N, W, i, p[x]) && valid;
    }
    const bool live = plane_from_triple(p[0], p[1], p[2], valid, min_nn, up ? up + (int64_t)v * 3 : nullptr, cos_min, planes + row * 4);
    counts[row] = live ? 0 : -1;
}

__global__ __launch_bounds__(PL_BLOCK) void k_plane_score(const double* __restrict__ intr, const double* __restrict__ depth,
                                                          const uint8_t* __restrict__ skip, int64_t N, int W, int chunks, int K,
                                                          const double* __restrict__ planes, double tol, int32_t* counts) {
    __shared__ double rows[PL_STAGE * 4];
    __shared__ int live[PL_STAGE];
    __shared__ int wave_counts[PL_WAVES][PL_STAGE];
    const int v = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double px[PL_PER_LANE], py[PL_PER_LANE], pz[PL_PER_LANE];
#pragma unroll
    for (int j = 0; j < PL_PER_LANE; ++j) {
        double p[3];
        const bool valid = pl_pixel(intr, depth, skip, v, N, W, (int64_t)chunk * PL_CHUNK + j * PL_BLOCK + (int)threadIdx.x, p);
        px[j] = valid ? p[0] : NAN, py[j] = valid ? p[1] : NAN, pz[j] = valid ? p[2] : NAN;  // (a NaN residual is no inlier)
    }
    const double* __restrict__ mine_planes = planes + (int64_t)v * K * 4;
    int32_t* mine_counts = counts + (int64_t)v * K;  // (other workgroups add to the same cells: a relaxed atomic load below)
    for (int k0 = 0; k0 < K; k0 += PL_STAGE) {
        __syncthreads();  // the block before has been read
        const int64_t cell = (int64_t)k0 * 4 + threadIdx.x;
        rows[threadIdx.x] = cell < (int64_t)K * 4 ? mine_planes[cell] : 0.0;
        // (a live row's count starts at 0 and only grows while this launch runs: its sign is the same whenever it is read)
        if (threadIdx.x < PL_STAGE) live[threadIdx.x] = k0 + (int)threadIdx.x < K && __atomic_load_n(mine_counts + k0 + threadIdx.x, __ATOMIC_RELAXED) >= 0;
        __syncthreads();
        int mine = 0;
        for (int j = 0; j < PL_STAGE; ++j) {
            if (!live[j]) continue;  // (uniform)
            const double n0 = rows[j * 4], n1 = rows[j * 4 + 1], n2 = rows[j * 4 + 2], off = rows[j * 4 + 3];
            int c = 0;
#pragma unroll
            for (int t = 0; t < PL_PER_LANE; ++t) c += __popcll(__ballot(fabs(((n0 * px[t] + n1 * py[t]) + n2 * pz[t]) + off) <= tol));
            mine = lane == j ? c : mine;
        }
        wave_counts[wave][lane] = mine;
        __syncthreads();
        if (threadIdx.x < PL_STAGE && live[threadIdx.x]) {
            const int total = (wave_counts[0][threadIdx.x] + wave_counts[1][threadIdx.x]) + (wave_counts[2][threadIdx.x] + wave_counts[3][threadIdx.x]);
            if (total > 0) atomicAdd(mine_counts + k0 + threadIdx.x, total);
        }
    }
}

__global__ __launch_bounds__(PL_BLOCK) void k_plane_select(const double* __restrict__ intr, const double* __restrict__ depth,
                                                           const uint8_t* __restrict__ skip, int64_t N, int W, int K,
                                                           const int32_t* __restrict__ triples, const double* __restrict__ planes,
                                                           const int32_t* __restrict__ counts, int32_t* __restrict__ best,
                                                           double* __restrict__ best_planes, double* __restrict__ anchors) {
    __shared__ int top_count[PL_BLOCK], top_k[PL_BLOCK];
    const int v = blockIdx.x, me = threadIdx.x;
    int count = -1, at = K;
    for (int k = me; k < K; k += PL_BLOCK) {  // (ascending: the strict > keeps the smallest k)
        const int c = counts[(int64_t)v * K + k];
        if (c > count) count = c, at = k;
    }
    top_count[me] = count, top_k[me] = at;
    __syncthreads();
    for (int s = PL_BLOCK / 2; s > 0; s >>= 1) {
        if (me < s) {
            const int c = top_count[me + s], k = top_k[me + s];
            if (c > top_count[me] || (c == top_count[me] && k < top_k[me])) top_count[me] = c, top_k[me] = k;
        }
        __syncthreads();
    }
    const int b = top_count[0] >= 0 ? top_k[0] : -1;
    if (me == 0) best[v] = b;
    if (me < 4) best_planes[(int64_t)v * 4 + me] = b >= 0 ? planes[((int64_t)v * K + b) * 4 + me] : 0.0;
    if (me == 4) {
        double p[3] = {0.0, 0.0, 0.0};
        if (b >= 0) pl_pixel(intr, depth, skip, v, N, W, min(max((int64_t)triples[((int64_t)v * K + b) * 3], (int64_t)0), N - 1), p);
        for (int a = 0; a < 3; ++a) anchors[(int64_t)v * 3 + a] = b >= 0 ? p[a] : 0.0;
    }
}

__global__ __launch_bounds__(PL_BLOCK) void k_plane_moments(const double* __restrict__ intr, const double* __restrict__ depth,
                                                            const uint8_t* __restrict__ skip, int64_t N, int W, int chunks,
                                                            const double* __restrict__ planes, const double* __restrict__ anchors, double tol,
                                                            double* __restrict__ partials) {
    __shared__ double wave_sums[PL_WAVES][PLANE_SUMS];
    __shared__ int wave_count[PL_WAVES];
    const int v = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double plane[4], anchor[3];
    for (int a = 0; a < 4; ++a) plane[a] = planes[(int64_t)v * 4 + a];
    for (int a = 0; a < 3; ++a) anchor[a] = anchors[(int64_t)v * 3 + a];
    const bool exists = plane_exists(plane);
    double s[PLANE_SUMS];
    for (int a = 0; a < PLANE_SUMS; ++a) s[a] = 0.0;
    int count = 0;
    for (int j = 0; j < PL_PER_LANE; ++j) {
        double p[3], t[PLANE_SUMS];
        const bool valid = pl_pixel(intr, depth, skip, v, N, W, (int64_t)chunk * PL_CHUNK + j * PL_BLOCK + (int)threadIdx.x, p);
        const bool in = exists && plane_inlier(plane, p, valid, tol);
        plane_terms(p, anchor, t);
        for (int a = 0; a < PLANE_SUMS; ++a) s[a] = s[a] + (in ? t[a] : 0.0);
        count += __popcll(__ballot(in));
    }
    // x[l] += x[l + s] for s = 32 ... 1: lane 0 ends with the wave's total (what lanes >= s read is never used)
    for (int a = 0; a < PLANE_SUMS; ++a)
        for (int off = 32; off > 0; off >>= 1) s[a] = s[a] + __shfl_down(s[a], off, 64);
    if (lane == 0) {
        for (int a = 0; a < PLANE_SUMS; ++a) wave_sums[wave][a] = s[a];
        wave_count[wave] = count;
    }
    __syncthreads();
    double* __restrict__ out = partials + (int64_t)blockIdx.x * PL_PARTIALS;
    if (threadIdx.x < PLANE_SUMS) {
        const int a = threadIdx.x;
        out[a] = ((wave_sums[0][a] + wave_sums[1][a]) + wave_sums[2][a]) + wave_sums[3][a];
    } else if (threadIdx.x == PLANE_SUMS) {
        ((int64_t*)out)[PLANE_SUMS] = (int64_t)((wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]));
    }
}

// One workgroup per view: the chunk partials pass through LDS PL_REDUCE_TILE chunks at a time (every thread loads, so that the
// loads do not wait for one another), and one thread per sum adds them left to right.
__global__ __launch_bounds__(PL_BLOCK) void k_plane_reduce(const double* __restrict__ partials, int chunks, int32_t* __restrict__ count,
                                                           double* __restrict__ sums) {
    __shared__ double tile[PL_REDUCE_TILE * PL_PARTIALS];
    const int v = blockIdx.x, a = threadIdx.x;
    const double* __restrict__ mine = partials + (int64_t)v * chunks * PL_PARTIALS;
    double total = 0.0;
    int64_t nodes = 0;
    for (int c0 = 0; c0 < chunks; c0 += PL_REDUCE_TILE) {
        const int n = min(PL_REDUCE_TILE, chunks - c0);
        __syncthreads();  // the tile before has been added
        for (int x = threadIdx.x; x < n * PL_PARTIALS; x += PL_BLOCK) tile[x] = mine[(int64_t)c0 * PL_PARTIALS + x];
        __syncthreads();
        if (a < PLANE_SUMS)
            for (int c = 0; c < n; ++c) total = total + tile[c * PL_PARTIALS + a];
        else if (a == PLANE_SUMS)
            for (int c = 0; c < n; ++c) nodes += ((const int64_t*)tile)[c * PL_PARTIALS + a];
    }
    if (a < PLANE_SUMS) sums[(int64_t)v * PLANE_SUMS + a] = total;
    else if (a == PLANE_SUMS) count[v] = (int32_t)nodes;  // (at most H * W <= 2^31 - 1)
}

__global__ __launch_bounds__(PL_BLOCK) void k_plane_mask(const double* __restrict__ intr, const double* __restrict__ depth,
                                                         const uint8_t* __restrict__ skip, int64_t pixels, int64_t N, int W,
                                                         const double* __restrict__ planes, double tol, uint8_t* __restrict__ mask) {
    const int64_t id = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (id >= pixels) return;
    const int v = (int)(id / N);
    double p[3];
    const bool valid = pl_pixel(intr, depth, skip, v, N, W, id - (int64_t)v * N, p);
    mask[id] = plane_explains(planes + (int64_t)v * 4, p, valid, tol) ? 1 : 0;
}

__global__ __launch_bounds__(PL_BLOCK) void k_plane_volumes(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                            const double* __restrict__ planes, float* __restrict__ pool) {
    const volume_node n = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, PL_BLOCK);
    if (!n.live) return;
    const omgx_mesh ms = meshes[n.m];
    double p[3];
    volume_node_point(ms, n.idc, p);
    pool[ms.out_offset + n.id] = plane_halfspace(planes + (int64_t)n.m * 4, p);
}

// What every entry point over images checks on the host -> OMGX_OK, OMGX_ERR_INVALID, or OMGX_ERR_UNSUPPORTED above 2^31 - 1
// pixels in all (an invalid argument is reported first: the caller returns UNSUPPORTED only after its own checks).
int check_images(const double* h_intrinsics, int32_t V, int32_t H, int32_t W, double tol) {
    if (V < 0 || !std::isfinite(tol) || tol < 0.0) return OMGX_ERR_INVALID;
    if (V == 0) return OMGX_OK;
    if (!h_intrinsics || H < 1 || W < 1) return OMGX_ERR_INVALID;
    if (image_check_rows(h_intrinsics, V, 4) != OMGX_OK) return OMGX_ERR_INVALID;
    return image_pixels_fit(V, H, W) ? OMGX_OK : OMGX_ERR_UNSUPPORTED;
}

int64_t chunks_of(int32_t H, int32_t W) { return ((int64_t)H * W + PL_CHUNK - 1) / PL_CHUNK; }

}  // namespace

extern "C" int omgx_plane_ransac(const double* intrinsics, const double* h_intrinsics, const double* depth, const uint8_t* skip, int32_t num_views,
                                 int32_t H, int32_t W, const int32_t* triples, const int32_t* h_triples, int32_t num_hypotheses, double tol,
                                 double min_nn, const double* up, double cos_min, double* planes, int32_t* counts, int32_t* best,
                                 double* best_planes, double* anchors, void* stream) {
    const int32_t V = num_views, K = num_hypotheses;
    const int images = check_images(h_intrinsics, V, H, W, tol);
    if (images == OMGX_ERR_INVALID || !std::isfinite(min_nn) || min_nn < 0.0 || !(cos_min >= -1.0 && cos_min <= 1.0)) return OMGX_ERR_INVALID;
    if (K < 1 || K > OMGX_PLANE_MAX_HYPOTHESES) return OMGX_ERR_INVALID;
    if (V == 0) return OMGX_OK;
    if (!intrinsics || !depth || !triples || !h_triples || !planes || !counts || !best || !best_planes || !anchors) return OMGX_ERR_INVALID;
    const int64_t N = (int64_t)H * W, rows = (int64_t)V * K;
    for (int64_t x = 0; x < rows * 3; ++x)
        if (h_triples[x] < 0 || h_triples[x] >= N) return OMGX_ERR_INVALID;
    if (images != OMGX_OK || rows > 0x7fffffffll) return OMGX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int chunks = (int)chunks_of(H, W);
    hipLaunchKernelGGL(k_plane_hypotheses, dim3((unsigned)((rows + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0, s, intrinsics, depth, skip, rows, N,
                       (int)W, (int)K, triples, min_nn, up, cos_min, planes, counts);
    OMGX_CHECK_LAUNCH("k_plane_hypotheses");
    hipLaunchKernelGGL(k_plane_score, dim3((unsigned)((int64_t)V * chunks)), dim3(PL_BLOCK), 0, s, intrinsics, depth, skip, N, (int)W, chunks, (int)K,
                       planes, tol, counts);
    OMGX_CHECK_LAUNCH("k_plane_score");
    hipLaunchKernelGGL(k_plane_select, dim3((unsigned)V), dim3(PL_BLOCK), 0, s, intrinsics, depth, skip, N, (int)W, (int)K, triples, planes, counts,
                       best, best_planes, anchors);
    OMGX_CHECK_LAUNCH("k_plane_select");
    return OMGX_OK;
}

extern "C" int64_t omgx_plane_workspace_bytes(int32_t num_views, int32_t H, int32_t W) {
    if (num_views < 0 || (num_views > 0 && (H < 1 || W < 1))) return OMGX_ERR_INVALID;
    if (num_views == 0) return 0;
    if (!image_pixels_fit(num_views, H, W)) return OMGX_ERR_UNSUPPORTED;
    return (int64_t)num_views * chunks_of(H, W) * PL_PARTIALS * (int64_t)sizeof(double);
}

extern "C" int omgx_plane_moments(const double* intrinsics, const double* h_intrinsics, const double* depth, const uint8_t* skip, int32_t num_views,
                                  int32_t H, int32_t W, const double* planes, const double* anchors, double tol, void* workspace, int32_t* count,
                                  double* sums, void* stream) {
    const int32_t V = num_views;
    const int images = check_images(h_intrinsics, V, H, W, tol);
    if (images == OMGX_ERR_INVALID) return images;
    if (V == 0) return OMGX_OK;
    if (!intrinsics || !depth || !planes || !anchors || !workspace || !count || !sums) return OMGX_ERR_INVALID;
    if (images != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int chunks = (int)chunks_of(H, W);
    hipLaunchKernelGGL(k_plane_moments, dim3((unsigned)((int64_t)V * chunks)), dim3(PL_BLOCK), 0, s, intrinsics, depth, skip, (int64_t)H * W, (int)W,
                       chunks, planes, anchors, tol, (double*)workspace);
    OMGX_CHECK_LAUNCH("k_plane_moments");
    hipLaunchKernelGGL(k_plane_reduce, dim3((unsigned)V), dim3(PL_BLOCK), 0, s, (const double*)workspace, chunks, count, sums);
    OMGX_CHECK_LAUNCH("k_plane_reduce");
    return OMGX_OK;
}

extern "C" int omgx_plane_mask(const double* intrinsics, const double* h_intrinsics, const double* depth, const uint8_t* skip, int32_t num_views,
                               int32_t H, int32_t W, const double* planes, double tol, uint8_t* mask, void* stream) {
    const int32_t V = num_views;
    const int images = check_images(h_intrinsics, V, H, W, tol);
    if (images == OMGX_ERR_INVALID) return images;
    if (V == 0) return OMGX_OK;
    if (!intrinsics || !depth || !planes || !mask) return OMGX_ERR_INVALID;
    if (images != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    const int64_t N = (int64_t)H * W, pixels = N * V;
    hipLaunchKernelGGL(k_plane_mask, dim3((unsigned)((pixels + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0, (hipStream_t)stream, intrinsics, depth, skip,
                       pixels, N, (int)W, planes, tol, mask);
    OMGX_CHECK_LAUNCH("k_plane_mask");
    return OMGX_OK;
}

extern "C" int omgx_plane_volumes(const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, const double* planes,
                                  const double* h_planes, float* pool, int64_t pool_elems, void* stream) {
    const int32_t M = num_volumes;
    if (M < 0 || pool_elems < 0) return OMGX_ERR_INVALID;
    if (M == 0) return OMGX_OK;
    if (!volumes || !h_volumes || !planes || !h_planes || !pool) return OMGX_ERR_INVALID;
    int64_t wg = 0;
    const int status = mesh_check_volumes(h_volumes, M, pool_elems, PL_BLOCK, &wg);
    if (status == OMGX_ERR_INVALID) return status;
    for (int64_t x = 0; x < (int64_t)M * 4; ++x)
        if (!std::isfinite(h_planes[x])) return OMGX_ERR_INVALID;
    if (mesh_pool_ranges_overlap(h_volumes, M)) return OMGX_ERR_INVALID;
    if (status != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_plane_volumes, dim3((unsigned)wg), dim3(PL_BLOCK), 0, (hipStream_t)stream, volumes, (int)M, planes, pool);
    OMGX_CHECK_LAUNCH("k_plane_volumes");
    return OMGX_OK;
}
