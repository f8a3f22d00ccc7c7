// omg_register.hip — pose refinement of known objects against observed clouds (include/omg_hip.h section 15).
//
// k_register_clouds: one workgroup of 256 threads per instance (object, start pose, range of points), the whole
// Levenberg-Marquardt iteration inside one launch.  A pass streams the instance's points from global memory, lane l taking the
// used points l, l + 256, ...; each lane keeps the 21 + 6 + 1 float64 partials and the inlier count in registers; they are summed
// by shuffles inside each wave (x[l] += x[l + s], s = 32 ... 1) and the four wave totals go through LDS, added as
// ((w0 + w1) + w2) + w3.  Two LDS slots by the parity of the pass save the second barrier: a wave that writes slot p again has
// passed the barrier of the pass between, which every wave reaches only after it has read slot p.  Every lane then reads the
// totals and runs the same 6 x 6 solve and the same accept / reject decision (reg_iterate, omg_register_body.h), so control flow
// is uniform and nothing is broadcast.  All arithmetic is float64 with contraction off, one operation per operation of the
// specification registration.register_clouds (omg-planner_amd/registration.py).  Plain loads and stores only.
#include "omg_host.h"
#include "omg_register_body.h"

#pragma clang fp contract(off)

#define REG_BLOCK OMGX_REGISTER_THREADS
#define REG_WAVES (REG_BLOCK / 64)
static_assert(REG_BLOCK == 256 && OMGX_REGISTER_STATS == 8, "the shape of the sum and of a stats row as include/omg_hip.h documents them");
static_assert(REG_FEW_INLIERS == OMGX_REGISTER_FEW_INLIERS && REG_SINGULAR == OMGX_REGISTER_SINGULAR &&
                  REG_LAMBDA_AT_MAX == OMGX_REGISTER_LAMBDA_AT_MAX && REG_CONVERGED == OMGX_REGISTER_CONVERGED,
              "one status word");
static_assert(sizeof(omgx_object) == 184, "records as include/omg_hip.h documents them");

namespace {

__global__ __launch_bounds__(REG_BLOCK) void k_register_clouds(const omgx_object* __restrict__ objects, const float* __restrict__ pool,
                                                               const int32_t* __restrict__ obj_index, const double* __restrict__ poses0,
                                                               const double* __restrict__ points, const int32_t* __restrict__ ranges,
                                                               int stride, double trunc, double lambda0, double step_tol, int max_passes,
                                                               double* __restrict__ poses_out, double* __restrict__ stats_out) {
    __shared__ double wave_sum[2][REG_WAVES][REG_NPART];
    __shared__ int32_t wave_count[2][REG_WAVES];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the instance's record, pose and range: uniform addresses, scalar loads
    const omgx_object* __restrict__ ob = objects + obj_index[m];
    reg_grid G;
    for (int a = 0; a < 3; ++a) G.lo[a] = (double)ob->lo[a], G.dim[a] = ob->dim[a];
    G.inv_delta = ob->inv_delta, G.offset = ob->grid_offset;
    const int64_t begin = ranges[2 * m], end = ranges[2 * m + 1];
    const int64_t used = (end - begin + stride - 1) / stride;  // begin, begin + stride, ... < end
    const double tau2 = trunc * trunc;
    double pose[12], stats[OMGX_REGISTER_STATS];
    for (int i = 0; i < 12; ++i) pose[i] = poses0[(int64_t)m * 12 + i];
    int parity = 0;

    auto pass = [&](const double* P, reg_sums& tot) {
        reg_sums acc;
        reg_clear(acc);
        for (int64_t j = tid; j < used; j += REG_BLOCK) {
            const double* __restrict__ p = points + (begin + j * stride) * 3;
            reg_point(G, pool, P, p[0], p[1], p[2], trunc, tau2, acc);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (int i = 0; i < REG_NPART; ++i) acc.x[i] = acc.x[i] + __shfl_down(acc.x[i], s, 64);
            acc.count += __shfl_down(acc.count, s, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < REG_NPART; ++i) wave_sum[parity][wave][i] = acc.x[i];
            wave_count[parity][wave] = acc.count;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < REG_NPART; ++i)
            tot.x[i] = ((wave_sum[parity][0][i] + wave_sum[parity][1][i]) + wave_sum[parity][2][i]) + wave_sum[parity][3][i];
        tot.count = ((wave_count[parity][0] + wave_count[parity][1]) + wave_count[parity][2]) + wave_count[parity][3];
        parity ^= 1;
    };
    reg_iterate(pass, pose, lambda0, step_tol, max_passes, stats);

    if (tid == 0) {
        for (int i = 0; i < 12; ++i) poses_out[(int64_t)m * 12 + i] = pose[i];
        for (int i = 0; i < OMGX_REGISTER_STATS; ++i) stats_out[(int64_t)m * OMGX_REGISTER_STATS + i] = stats[i];
    }
}

}  // namespace

extern "C" int omgx_register_clouds(const omgx_object* objects, const omgx_object* h_objects, int32_t num_objects, const float* pool,
                                    int64_t pool_elems, const int32_t* obj_index, const int32_t* h_obj_index, const double* poses0,
                                    const double* points, int64_t num_points, const int32_t* ranges, const int32_t* h_ranges,
                                    int32_t num_instances, int32_t stride, double trunc, double lambda0, double step_tol, int32_t max_passes,
                                    double* poses_out, double* stats_out, void* stream) {
    if (num_objects < 0 || pool_elems < 0 || num_points < 0 || num_instances < 0 || stride < 1) return OMGX_ERR_INVALID;
    if (max_passes < 0 || max_passes > OMGX_REGISTER_MAX_PASSES) return OMGX_ERR_INVALID;
    if (!(trunc > 0.0) || !std::isfinite(trunc) || !(lambda0 > 0.0) || !std::isfinite(lambda0)) return OMGX_ERR_INVALID;
    if (num_instances > 0 && (!objects || !h_objects || !pool || !obj_index || !h_obj_index || !poses0 || !ranges || !h_ranges || !poses_out ||
                              !stats_out))
        return OMGX_ERR_INVALID;
    if (num_points > 0 && !points) return OMGX_ERR_INVALID;
    for (int32_t m = 0; m < num_instances; ++m) {
        const int32_t o = h_obj_index[m];
        if (o < 0 || o >= num_objects) return OMGX_ERR_INVALID;
        const int64_t b = h_ranges[2 * m], e = h_ranges[2 * m + 1];
        if (b < 0 || e < b || e > num_points) return OMGX_ERR_INVALID;
        const omgx_object& r = h_objects[o];
        if (r.dim[0] < 2 || r.dim[1] < 2 || r.dim[2] < 2 || r.grid_offset < 0) return OMGX_ERR_INVALID;
        const int64_t n = (int64_t)r.dim[0] * r.dim[1];  // < 2^62; times dim[2] could overflow: compare by division
        if (r.grid_offset > pool_elems || n > (pool_elems - r.grid_offset) / r.dim[2]) return OMGX_ERR_INVALID;
    }
    if (num_instances == 0) return OMGX_OK;
    hipLaunchKernelGGL(k_register_clouds, dim3((unsigned)num_instances), dim3(REG_BLOCK), 0, (hipStream_t)stream, objects, pool, obj_index, poses0,
                       points, ranges, (int)stride, trunc, lambda0, step_tol, (int)max_passes, poses_out, stats_out);
    OMGX_CHECK_LAUNCH("k_register_clouds");
    return OMGX_OK;
}
