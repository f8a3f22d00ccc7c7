// omg_tsdf.hip — weighted TSDF fusion: depth views to sub-voxel obstacle volumes (include/omg_hip.h section 20).
//
// A ragged batch of volumes (omgx_mesh records), nodes in x-major groups of 256 per workgroup, workgroups mapped to volumes by the
// first_workgroup prefix table as in k_carve_views:
//   k_tsdf_integrate  one thread per node: the node's point through every view of its volume, the pair (D, W) averaged in
//                     float64 registers and written back as two float32: 16 bytes of coalesced traffic per node and call
//   k_tsdf_states     one thread per node: the pair's state byte (carve's layout)
//   k_tsdf_blend      one thread per node: the pair blended into the distance transform's value in the pool, in place
// The arithmetic is omg_tsdf_body.h: the bits of tsdf.py.  Plain loads and stores only; the stream is the only barrier.
#include "omg_mesh_common.h"
#include "omg_tsdf_body.h"

#pragma clang fp contract(off)

#define TSDF_BLOCK OMGX_TSDF_NODES_PER_WORKGROUP
static_assert(TSDF_BLOCK == 256 && TSDF_BLOCK == OMGX_FUSION_NODES_PER_WORKGROUP, "the prefix table of the fusion records");

namespace {

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_integrate(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                               const double* __restrict__ views, const int32_t* __restrict__ view_range,
                                                               const int64_t* __restrict__ state_begin, const double* __restrict__ depth,
                                                               int H, int W, const double* __restrict__ weights, double trunc, double near,
                                                               double wmax, int merge, float* __restrict__ tsdf, float* __restrict__ weight) {
    const volume_node n = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, TSDF_BLOCK);
    const omgx_mesh ms = meshes[n.m];
    double p[3];
    volume_node_point(ms, n.idc, p);
    const int64_t at = state_begin[n.m] + n.idc;
    double D, Wt;
    tsdf_start(merge != 0, merge ? tsdf[at] : 0.0f, merge ? weight[at] : 0.0f, &D, &Wt);
    const int v0 = view_range[2 * n.m], v1 = v0 + view_range[2 * n.m + 1];
    const int64_t image = (int64_t)H * W;
    for (int v = v0; v < v1; ++v) {  // (uniform: the view row and the weight come through scalar loads)
        const double w = weights ? weights[v] : 1.0;
        if (!(w > 0.0)) continue;
        double t;
        if (tsdf_view_updates(views + (int64_t)v * 16, depth + v * image, H, W, p, trunc, near, &t)) tsdf_update(&D, &Wt, t, w, wmax);
    }
    if (n.live) tsdf[at] = (float)D, weight[at] = (float)Wt;
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_states(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                            const int64_t* __restrict__ state_begin, const float* __restrict__ tsdf,
                                                            const float* __restrict__ weight, float min_weight, uint8_t* __restrict__ state) {
    const volume_node n = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, TSDF_BLOCK);
    const int64_t at = state_begin[n.m] + n.idc;
    const uint8_t s = tsdf_state(tsdf[at], weight[at], min_weight);
    if (n.live) state[at] = s;
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_blend(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                           const int64_t* __restrict__ state_begin, const float* __restrict__ tsdf,
                                                           const float* __restrict__ weight, double trunc, float min_weight,
                                                           float* __restrict__ pool) {
    const volume_node n = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, TSDF_BLOCK);
    const int64_t at = state_begin[n.m] + n.idc, out = meshes[n.m].out_offset + n.idc;
    const float v = tsdf_blend(tsdf[at], weight[at], pool[out], trunc, min_weight);
    if (n.live) pool[out] = v;
}

bool positive(double x, bool may_be_inf) { return x > 0.0 && (std::isfinite(x) || (may_be_inf && std::isinf(x))); }

}  // namespace

extern "C" int omgx_tsdf_integrate(const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, const double* views,
                                   const double* h_views, int32_t num_views, const int32_t* view_range, const int32_t* h_view_range,
                                   const int64_t* state_begin, const int64_t* h_state_begin, const double* depth, int32_t H, int32_t W,
                                   const double* weights, const double* h_weights, double trunc, double near, double wmax, int32_t merge,
                                   float* tsdf, float* weight, int64_t elems, void* stream) {
    const int32_t M = num_volumes, V = num_views;
    if (M < 0 || V < 0 || elems < 0 || !positive(trunc, false) || !positive(wmax, true) || !std::isfinite(near)) return OMGX_ERR_INVALID;
    if (M > 0 && (!volumes || !h_volumes || !view_range || !h_view_range || !state_begin || !h_state_begin || !tsdf || !weight)) return OMGX_ERR_INVALID;
    if (V > 0 && (!views || !h_views || !depth || H < 1 || W < 1)) return OMGX_ERR_INVALID;
    if ((weights != nullptr) != (h_weights != nullptr)) return OMGX_ERR_INVALID;
    const int images = mesh_check_views(h_views, V, H, W, h_view_range, M);
    if (images == OMGX_ERR_INVALID) return images;
    for (int32_t v = 0; h_weights && v < V; ++v)
        if (!std::isfinite(h_weights[v]) || h_weights[v] < 0.0) return OMGX_ERR_INVALID;
    if (M == 0) return images;
    int64_t wg = 0;
    const int status = mesh_check_batch(h_volumes, M, h_state_begin, elems, -1, TSDF_BLOCK, &wg);
    if (status == OMGX_ERR_INVALID) return status;
    if (status != OMGX_OK || images != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)wg), dim3(TSDF_BLOCK), 0, (hipStream_t)stream, volumes, (int)M, views, view_range,
                       state_begin, depth, (int)H, (int)W, weights, trunc, near, wmax, (int)merge, tsdf, weight);
    OMGX_CHECK_LAUNCH("k_tsdf_integrate");
    return OMGX_OK;
}

extern "C" int omgx_tsdf_states(const float* tsdf, const float* weight, int64_t elems, const int64_t* state_begin, const int64_t* h_state_begin,
                                const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, float min_weight, uint8_t* state,
                                void* stream) {
    const int32_t M = num_volumes;
    if (M < 0 || elems < 0 || !positive((double)min_weight, false)) return OMGX_ERR_INVALID;
    if (M > 0 && (!tsdf || !weight || !state_begin || !h_state_begin || !volumes || !h_volumes || !state)) return OMGX_ERR_INVALID;
    if (M == 0) return OMGX_OK;
    int64_t wg = 0;
    const int status = mesh_check_batch(h_volumes, M, h_state_begin, elems, -1, TSDF_BLOCK, &wg);
    if (status != OMGX_OK) return status;
    hipLaunchKernelGGL(k_tsdf_states, dim3((unsigned)wg), dim3(TSDF_BLOCK), 0, (hipStream_t)stream, volumes, (int)M, state_begin, tsdf, weight,
                       min_weight, state);
    OMGX_CHECK_LAUNCH("k_tsdf_states");
    return OMGX_OK;
}

extern "C" int omgx_tsdf_blend(const float* tsdf, const float* weight, int64_t elems, const int64_t* state_begin, const int64_t* h_state_begin,
                               const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, double trunc, float min_weight,
                               float* pool, int64_t pool_elems, void* stream) {
    const int32_t M = num_volumes;
    if (M < 0 || elems < 0 || pool_elems < 0 || !positive(trunc, false) || !positive((double)min_weight, false)) return OMGX_ERR_INVALID;
    if (M > 0 && (!tsdf || !weight || !state_begin || !h_state_begin || !volumes || !h_volumes || !pool)) return OMGX_ERR_INVALID;
    if (M == 0) return OMGX_OK;
    int64_t wg = 0;
    const int status = mesh_check_batch(h_volumes, M, h_state_begin, elems, pool_elems, TSDF_BLOCK, &wg);
    if (status == OMGX_ERR_INVALID || mesh_pool_ranges_overlap(h_volumes, M)) return OMGX_ERR_INVALID;
    if (status != OMGX_OK) return status;
    hipLaunchKernelGGL(k_tsdf_blend, dim3((unsigned)wg), dim3(TSDF_BLOCK), 0, (hipStream_t)stream, volumes, (int)M, state_begin, tsdf, weight,
                       trunc, min_weight, pool);
    OMGX_CHECK_LAUNCH("k_tsdf_blend");
    return OMGX_OK;
}
