// omg_fusion.hip — depth views to signed obstacle volumes (include/omg_hip.h section 17).
//
// A ragged batch of volumes (omgx_mesh records), nodes in x-major groups of 256 per workgroup, workgroups mapped to volumes by the
// first_workgroup prefix table as in k_surface_count:
//   k_carve_views   one thread per node: the node's point through every view of its volume, the state byte
//   k_fusion_rows   the z pass of the distance transform: a workgroup stages its 256 nodes' states and `radius` more on either
//                   side (contiguous, clipped to the volume) in LDS as seeds and takes the windowed minimum inside each node's row
//   k_fusion_slab   the y and the x pass: a workgroup stages [OMGX_FUSION_CHUNK lines along the axis + a halo of radius][64
//                   consecutive elements] in LDS, a wave per line, so that global traffic runs along z; the x pass takes (y, z)
//                   flattened as its 64 elements.  The last pass turns the squared distances into the float32 value in the pool.
// Intermediates: one word per node and pass (two 16-bit channels) at workspace[first_workgroup * 256 + L], two buffers.
// The arithmetic is omg_fusion_body.h: the bits of fusion.py.  Plain loads and stores only; the stream orders the passes.
#include "omg_mesh_common.h"
#include "omg_fusion_body.h"

#pragma clang fp contract(off)

#define FUSE_BLOCK OMGX_FUSION_NODES_PER_WORKGROUP
#define FUSE_LANES 64
#define FUSE_WAVES (FUSE_BLOCK / FUSE_LANES)
static_assert(FUSE_BLOCK == 256 && OMGX_FUSION_CHUNK % FUSE_WAVES == 0, "four waves per workgroup, a line of a chunk per wave");
static_assert(OMGX_FUSION_MAX_RADIUS * OMGX_FUSION_MAX_RADIUS < (1 << 16), "a channel is 16 bits");
static_assert(OMGX_FUSION_FREE == FUSION_FREE && OMGX_FUSION_SURFACE == FUSION_SURFACE && OMGX_FUSION_UNKNOWN == FUSION_UNKNOWN, "states");
#define FUSE_MAX_GRID_Y 65535

namespace {

__global__ __launch_bounds__(FUSE_BLOCK) void k_carve_views(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                            const double* __restrict__ views, const int32_t* __restrict__ view_range,
                                                            const int64_t* __restrict__ state_begin, const double* __restrict__ depth,
                                                            int H, int W, double band, double near, int merge, uint8_t* __restrict__ state) {
    // (lanes past the last node of the volume repeat it and write nothing)
    const volume_node n = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, FUSE_BLOCK);
    const int m = n.m;
    const omgx_mesh ms = meshes[m];
    double p[3];
    volume_node_point(ms, n.idc, p);
    uint8_t* __restrict__ mine = state + state_begin[m];
    bool surface = false, free_ = false;
    if (merge) {
        const uint8_t s = mine[n.idc];
        surface = s == FUSION_SURFACE, free_ = s == FUSION_FREE;
    }
    const int v0 = view_range[2 * m], v1 = v0 + view_range[2 * m + 1];
    const int64_t image = (int64_t)H * W;
    for (int v = v0; v < v1; ++v) {  // (uniform: the view row comes through scalar loads)
        const int says = fusion_view_says(views + (int64_t)v * 16, depth + v * image, H, W, p, band, near);
        surface = surface || says == FUSION_SAYS_SURFACE, free_ = free_ || says == FUSION_SAYS_FREE;
    }
    if (n.live) mine[n.id] = fusion_state(surface, free_);
}

__global__ __launch_bounds__(FUSE_BLOCK) void k_fusion_rows(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                            const uint8_t* __restrict__ state, const int64_t* __restrict__ state_begin,
                                                            int radius, int unknown_occupied, uint32_t* __restrict__ dst) {
    __shared__ uint32_t seeds[FUSE_BLOCK + 2 * OMGX_FUSION_MAX_RADIUS];
    const volume_node n = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, FUSE_BLOCK);
    const int dz = meshes[n.m].dims[2];
    const int64_t wg0 = meshes[n.m].first_workgroup;
    const int64_t lo = max(n.id0 - radius, (int64_t)0), hi = min(n.id0 + FUSE_BLOCK + radius, n.total);  // hi - lo <= 256 + 2 * radius
    const uint32_t r2 = (uint32_t)(radius * radius);
    const uint8_t* __restrict__ mine = state + state_begin[n.m];
    for (int64_t t = lo + threadIdx.x; t < hi; t += FUSE_BLOCK) seeds[t - lo] = fusion_seed(fusion_occupied(mine[t], unknown_occupied), r2);
    __syncthreads();
    if (!n.live) return;
    // the window stays inside the node's row, so inside [lo, hi)
    dst[wg0 * FUSE_BLOCK + n.id] = fusion_line_pass(seeds + (n.id - lo), 1, (int)((uint32_t)n.id % (uint32_t)dz), dz, radius, r2);
}

// axis 1: lines along y, for every x the elements z; axis 0: lines along x, the elements (y, z) flattened.  blockIdx.y: the
// volume (from vol0); blockIdx.x: (outer, block of 64 elements, chunk of the axis), the chunk fastest; a workgroup past its
// volume's last leaves at once.
template <bool LAST>
__global__ __launch_bounds__(FUSE_BLOCK) void k_fusion_slab(const omgx_mesh* __restrict__ meshes, int vol0, int axis, int radius,
                                                            const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                            float* __restrict__ pool) {
    extern __shared__ uint32_t slab[];  // [hi - lo][64]
    const omgx_mesh* __restrict__ ms = meshes + (vol0 + (int)blockIdx.y);
    const int64_t nx = ms->dims[0], ny = ms->dims[1], nz = ms->dims[2];
    const int64_t outer = axis == 1 ? nx : 1, outer_stride = ny * nz, line_stride = axis == 1 ? nz : ny * nz, elems = line_stride;
    const int64_t n64 = axis == 1 ? ny : nx;  // (up to 2^31 - 1: the sums below are made in 64 bits, as launch_slab makes them)
    const int n = (int)n64;
    const int64_t chunks = (n64 + OMGX_FUSION_CHUNK - 1) / OMGX_FUSION_CHUNK, blocks = (elems + FUSE_LANES - 1) / FUSE_LANES;
    const int64_t w = blockIdx.x;
    if (w >= outer * blocks * chunks) return;
    const int64_t c0 = (w % chunks) * OMGX_FUSION_CHUNK, c1 = min(c0 + OMGX_FUSION_CHUNK, n64);
    const int a0 = (int)c0, count = (int)(c1 - c0);  // this chunk: positions a0 .. a0 + count of the axis
    const int lo = (int)max(c0 - radius, (int64_t)0), staged = (int)(min(c1 + radius, n64) - lo);  // staged <= min(chunk + 2 * radius, n): what the launch reserves
    const int lane = threadIdx.x & (FUSE_LANES - 1), wave = threadIdx.x / FUSE_LANES;
    const int64_t e = ((w / chunks) % blocks) * FUSE_LANES + lane;
    const bool live = e < elems;
    const int64_t node0 = (w / (chunks * blocks)) * outer_stride + (live ? e : 0);  // the line's node at position 0
    const uint32_t* __restrict__ from = src + ms->first_workgroup * FUSE_BLOCK + node0;
    for (int t = wave; t < staged; t += FUSE_WAVES) slab[t * FUSE_LANES + lane] = live ? from[(lo + t) * line_stride] : 0u;
    __syncthreads();
    if (!live) return;
    const uint32_t r2 = (uint32_t)(radius * radius);
    const double delta = ms->delta;
    for (int t = wave; t < count; t += FUSE_WAVES) {
        const int a = a0 + t;
        const uint32_t word = fusion_line_pass(slab + (a - lo) * FUSE_LANES + lane, FUSE_LANES, a, n, radius, r2);
        if (LAST) pool[ms->out_offset + node0 + a * line_stride] = fusion_value(word, delta);
        else dst[ms->first_workgroup * FUSE_BLOCK + node0 + a * line_stride] = word;
    }
}

int check_radius(int32_t radius) { return radius < 1 ? OMGX_ERR_INVALID : radius > OMGX_FUSION_MAX_RADIUS ? OMGX_ERR_UNSUPPORTED : OMGX_OK; }

// One of the y / x passes over all volumes: blockIdx.y holds at most 65535 volumes, so one launch per that many (one, in
// practice).  The grid's x is the largest workgroup count of the launch's volumes, the LDS its longest staged line.
template <bool LAST>
int launch_slab(const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t M, int axis, int radius, const uint32_t* src, uint32_t* dst,
                float* pool, hipStream_t stream) {
    for (int32_t vol0 = 0; vol0 < M; vol0 += FUSE_MAX_GRID_Y) {
        const int32_t count = std::min<int32_t>(M - vol0, FUSE_MAX_GRID_Y);
        int64_t grid = 0, lines = 0;
        for (int32_t m = vol0; m < vol0 + count; ++m) {
            const omgx_mesh& h = h_volumes[m];
            const int64_t n = axis == 1 ? h.dims[1] : h.dims[0], outer = axis == 1 ? h.dims[0] : 1;
            const int64_t elems = axis == 1 ? (int64_t)h.dims[2] : (int64_t)h.dims[1] * h.dims[2];
            grid = std::max(grid, outer * ((elems + FUSE_LANES - 1) / FUSE_LANES) * ((n + OMGX_FUSION_CHUNK - 1) / OMGX_FUSION_CHUNK));
            lines = std::max(lines, std::min<int64_t>(OMGX_FUSION_CHUNK + 2 * radius, n));
        }
        const size_t lds = (size_t)lines * FUSE_LANES * sizeof(uint32_t);  // at most 574 * 256 bytes
        if (lds > 64 * 1024) {
            const int rc = allow_big_lds<LAST ? 21 : 20>(k_fusion_slab<LAST>, "hipFuncSetAttribute(k_fusion_slab)");
            if (rc != OMGX_OK) return rc;
        }
        hipLaunchKernelGGL(k_fusion_slab<LAST>, dim3((unsigned)grid, (unsigned)count), dim3(FUSE_BLOCK), lds, stream, volumes, (int)vol0, axis,
                           radius, src, dst, pool);
        OMGX_CHECK_LAUNCH("k_fusion_slab");
    }
    return OMGX_OK;
}

}  // namespace

extern "C" int omgx_carve_views(const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, const double* views,
                                const double* h_views, int32_t num_views, const int32_t* view_range, const int32_t* h_view_range,
                                const int64_t* state_begin, const int64_t* h_state_begin, const double* depth, int32_t H, int32_t W,
                                double band, double near, int32_t merge, uint8_t* state, int64_t state_elems, void* stream) {
    const int32_t M = num_volumes, V = num_views;
    if (M < 0 || V < 0 || state_elems < 0 || !std::isfinite(band) || !std::isfinite(near)) return OMGX_ERR_INVALID;
    if (M > 0 && (!volumes || !h_volumes || !view_range || !h_view_range || !state_begin || !h_state_begin || !state)) return OMGX_ERR_INVALID;
    if (V > 0 && (!views || !h_views || !depth || H < 1 || W < 1)) return OMGX_ERR_INVALID;
    const int images = mesh_check_views(h_views, V, H, W, h_view_range, M);
    if (images == OMGX_ERR_INVALID || M == 0) return images;
    int64_t wg = 0;
    const int status = mesh_check_batch(h_volumes, M, h_state_begin, state_elems, -1, FUSE_BLOCK, &wg);
    if (status == OMGX_ERR_INVALID) return status;
    if (status != OMGX_OK || images != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_carve_views, dim3((unsigned)wg), dim3(FUSE_BLOCK), 0, (hipStream_t)stream, volumes, (int)M, views, view_range, state_begin,
                       depth, (int)H, (int)W, band, near, (int)merge, state);
    OMGX_CHECK_LAUNCH("k_carve_views");
    return OMGX_OK;
}

extern "C" int64_t omgx_distance_transform_workspace_bytes(const omgx_mesh* h_volumes, int32_t num_volumes, int32_t radius) {
    if (num_volumes < 0 || radius < 1) return OMGX_ERR_INVALID;
    int64_t wg = 0;
    const int status = num_volumes == 0 ? OMGX_OK : mesh_check_volumes(h_volumes, num_volumes, -1, FUSE_BLOCK, &wg);
    if (status == OMGX_ERR_INVALID) return status;
    if (status != OMGX_OK || check_radius(radius) != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    return wg * FUSE_BLOCK * 2 * (int64_t)sizeof(uint32_t);
}

extern "C" int omgx_distance_transform(const uint8_t* state, int64_t state_elems, const int64_t* state_begin, const int64_t* h_state_begin,
                                       const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, int32_t radius,
                                       int32_t unknown_occupied, void* workspace, float* pool, int64_t pool_elems, void* stream) {
    const int32_t M = num_volumes;
    if (M < 0 || state_elems < 0 || pool_elems < 0 || radius < 1) return OMGX_ERR_INVALID;
    if (M > 0 && (!state || !state_begin || !h_state_begin || !volumes || !h_volumes || !workspace || !pool)) return OMGX_ERR_INVALID;
    if (M == 0) return check_radius(radius);
    int64_t wg = 0;
    const int status = mesh_check_batch(h_volumes, M, h_state_begin, state_elems, pool_elems, FUSE_BLOCK, &wg);
    if (status == OMGX_ERR_INVALID || mesh_pool_ranges_overlap(h_volumes, M)) return OMGX_ERR_INVALID;
    if (status != OMGX_OK || check_radius(radius) != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    uint32_t* first = (uint32_t*)workspace;
    uint32_t* second = first + wg * FUSE_BLOCK;
    hipLaunchKernelGGL(k_fusion_rows, dim3((unsigned)wg), dim3(FUSE_BLOCK), 0, (hipStream_t)stream, volumes, (int)M, state, state_begin, (int)radius,
                       (int)unknown_occupied, first);
    OMGX_CHECK_LAUNCH("k_fusion_rows");
    int rc = launch_slab<false>(volumes, h_volumes, M, 1, radius, first, second, nullptr, (hipStream_t)stream);
    if (rc != OMGX_OK) return rc;
    return launch_slab<true>(volumes, h_volumes, M, 0, radius, second, nullptr, pool, (hipStream_t)stream);
}
