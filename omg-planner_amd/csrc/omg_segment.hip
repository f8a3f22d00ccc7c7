// omg_segment.hip — carved states to objects: connected components and cropped state volumes (include/omg_hip.h section 18).
//
// A ragged batch of volumes (omgx_mesh records), nodes in x-major runs of 256 per workgroup, workgroups mapped to volumes by the
// first_workgroup prefix table as in omg_fusion.hip.  The labelling is a union by label equivalence on a table of parent links
// (one int32 per node, a node's linear index inside its volume, -1 for background), always the same launches:
//   k_label_local    a workgroup unions the backward neighbours that fall inside its own run in LDS and writes every node's
//                    root of the run
//   k_label_border   the backward neighbours that fall before the run, in global memory: atomics and relaxed agent-scope atomic
//                    loads only, because workgroups on other XCDs change the same cells
//   k_label_count    the nodes that are their own parent are the components' first nodes: their number per workgroup (ballot +
//                    popcount, the four waves summed in order) and every first node's rank inside its workgroup
//   k_label_scan     one workgroup per volume: the workgroup totals become exclusive offsets in place, the volume's total `counts`
//   k_label_write    every node follows its links to the root (nobody changes them any more: plain loads) and writes the root's
//                    rank; the pattern of omg_surface.hip, without atomics
// k_records_fill builds the components' records with integer atomics (add, min, max: the order of arrival changes nothing),
// lanes of a wave that share a component reduced first.  k_component_states: one thread per node of an output volume.
// The per-node rules are omg_segment_body.h.  No spin-waits, no flags: the stream is the only barrier between the launches.
#include <climits>

#include "omg_mesh_common.h"
#include "omg_segment_body.h"

#define SEG_BLOCK OMGX_SEGMENT_NODES_PER_WORKGROUP
static_assert(SEG_BLOCK == 256, "four waves per workgroup");
static_assert(OMGX_FUSION_FREE == SEG_FREE && OMGX_FUSION_SURFACE == SEG_SURFACE && OMGX_FUSION_UNKNOWN == SEG_UNKNOWN, "states");
// Workspace of WG workgroups: parent [WG * 256] int32, totals [WG] int32, ranks [WG * 256] uint8.
#define SEG_WORKSPACE_PER_WORKGROUP (SEG_BLOCK * 4 + 4 + SEG_BLOCK)
// Rounds in which k_records_fill reduces the lanes that share the first pending lane's component; what is left goes alone.
#define SEG_RECORD_ROUNDS 2

namespace {

// This thread's node (id0: the run's first node), its volume's record and its coordinates.  Lanes past the last node are not
// live and repeat it.
struct seg_node : volume_node {
    const omgx_mesh* ms;
    int i, j, k;
};

__device__ __forceinline__ seg_node seg_locate(const omgx_mesh* __restrict__ meshes, int num_meshes) {
    seg_node t;
    static_cast<volume_node&>(t) = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, SEG_BLOCK);
    t.ms = meshes + t.m;
    volume_decode(t.ms->dims, t.idc, &t.i, &t.j, &t.k);
    return t;
}

__global__ __launch_bounds__(SEG_BLOCK) void k_label_local(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                           const uint8_t* __restrict__ state, const int64_t* __restrict__ state_begin,
                                                           int select, int order, int32_t* __restrict__ parent) {
    __shared__ int32_t link[SEG_BLOCK];  // the run's links, as positions in the run
    const seg_node t = seg_locate(meshes, num_meshes);
    const int me = threadIdx.x;
    const bool fg = t.live && seg_foreground(state[state_begin[t.m] + t.id], select);
    link[me] = fg ? me : SEG_BACKGROUND;
    __syncthreads();
    if (fg) {
        for (int n = 0; n < SEG_BACKWARD; ++n) {
            int64_t q;
            if (!seg_neighbour(n, order, t.ms->dims, t.i, t.j, t.k, &q) || q < t.id0) continue;
            const int other = (int)(q - t.id0);  // 0 <= other < me
            if (seg_load<SEG_SCOPE_WORKGROUP>(link + other) != SEG_BACKGROUND) seg_union<SEG_SCOPE_WORKGROUP>(link, me, other);
        }
    }
    __syncthreads();
    // (every cell of the workgroup's 256 is written: those past the volume's last node are background)
    parent[(int64_t)blockIdx.x * SEG_BLOCK + me] = fg ? (int32_t)t.id0 + seg_find<SEG_SCOPE_WORKGROUP>(link, me) : SEG_BACKGROUND;
}

__global__ __launch_bounds__(SEG_BLOCK) void k_label_border(const omgx_mesh* __restrict__ meshes, int num_meshes, int order,
                                                            int32_t* __restrict__ parent) {
    const seg_node t = seg_locate(meshes, num_meshes);
    if (!t.live || t.id0 == 0) return;  // (the first run of a volume has nothing before it)
    int32_t* mine = parent + t.ms->first_workgroup * SEG_BLOCK;  // the volume's table, indexed by the linear index
    if (seg_load<SEG_SCOPE_AGENT>(mine + t.id) == SEG_BACKGROUND) return;
    for (int n = 0; n < SEG_BACKWARD; ++n) {
        int64_t q;
        if (!seg_neighbour(n, order, t.ms->dims, t.i, t.j, t.k, &q) || q >= t.id0) continue;
        if (seg_load<SEG_SCOPE_AGENT>(mine + q) != SEG_BACKGROUND) seg_union<SEG_SCOPE_AGENT>(mine, (int32_t)t.id, (int32_t)q);
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void k_label_count(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                           const int32_t* __restrict__ parent, int32_t* __restrict__ totals,
                                                           uint8_t* __restrict__ ranks) {
    __shared__ int wave_count[SEG_BLOCK / 64];
    const seg_node t = seg_locate(meshes, num_meshes);
    const int64_t cell = (int64_t)blockIdx.x * SEG_BLOCK + threadIdx.x;
    const bool first = t.live && (int64_t)parent[cell] == t.id;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long firsts = __ballot(first);
    if (lane == 0) wave_count[wave] = __popcll(firsts);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_count[w];
    ranks[cell] = (uint8_t)(before + __popcll(firsts & ((1ull << lane) - 1ull)));
    if (threadIdx.x == 0) totals[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

// One workgroup per volume walks the volume's workgroup totals 256 at a time, as k_surface_scan does.
__global__ __launch_bounds__(SEG_BLOCK) void k_label_scan(const omgx_mesh* __restrict__ meshes, int32_t* __restrict__ totals,
                                                          int32_t* __restrict__ counts) {
    __shared__ int wave_total[SEG_BLOCK / 64];
    const omgx_mesh* __restrict__ ms = meshes + blockIdx.x;
    const int64_t nodes = (int64_t)ms->dims[0] * ms->dims[1] * ms->dims[2];
    const int n = (int)((nodes + SEG_BLOCK - 1) / SEG_BLOCK);
    int32_t* __restrict__ mine = totals + ms->first_workgroup;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += SEG_BLOCK) {
        const int i = base + (int)threadIdx.x;
        const int v = i < n ? mine[i] : 0;
        int x = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(x, off, 64);
            x += lane >= off ? y : 0;
        }
        if (lane == 63) wave_total[wave] = x;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; ++w) before += wave_total[w];
        if (i < n) mine[i] = carry + before + (x - v);
        carry += (wave_total[0] + wave_total[1]) + (wave_total[2] + wave_total[3]);
        __syncthreads();  // wave_total is written again
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(SEG_BLOCK) void k_label_write(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                           const int32_t* __restrict__ parent, const int32_t* __restrict__ totals,
                                                           const uint8_t* __restrict__ ranks, const int64_t* __restrict__ state_begin,
                                                           int32_t* __restrict__ labels) {
    const seg_node t = seg_locate(meshes, num_meshes);
    if (!t.live) return;
    const int64_t wg0 = t.ms->first_workgroup;
    const int32_t* __restrict__ mine = parent + wg0 * SEG_BLOCK;
    int32_t label = SEG_BACKGROUND;
    if (mine[t.id] != SEG_BACKGROUND) {
        const int32_t root = seg_find<SEG_SCOPE_PLAIN>(mine, (int32_t)t.id);
        label = totals[wg0 + root / SEG_BLOCK] + (int32_t)ranks[wg0 * SEG_BLOCK + root];
    }
    labels[state_begin[t.m] + t.id] = label;
}

__global__ __launch_bounds__(SEG_BLOCK) void k_records_init(int32_t* __restrict__ records, int64_t rows) {
    const int64_t r = (int64_t)blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (r >= rows) return;
    int32_t* rec = records + r * SEG_RECORD;
    rec[0] = 0;
    for (int c = 1; c < 5; ++c) rec[c] = INT_MAX;
    for (int c = 5; c < 8; ++c) rec[c] = -1;
}

__device__ __forceinline__ void seg_record_add(int32_t* rec, int count, int32_t first, const int* lo, const int* hi) {
    atomicAdd(rec, count);
    atomicMin(rec + 1, first);
    for (int a = 0; a < 3; ++a) atomicMin(rec + 2 + a, lo[a]), atomicMax(rec + 5 + a, hi[a]);
}

// Integer add, min and max only: the records do not depend on the order in which the atomics arrive.  A solid component would
// send every node to the same eight words, so the lanes of a wave that share the first pending lane's component are reduced with
// shuffles and that lane sends one set of atomics, SEG_RECORD_ROUNDS times; lanes still pending then send their own.
__global__ __launch_bounds__(SEG_BLOCK) void k_records_fill(const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                            const int32_t* __restrict__ labels, const int64_t* __restrict__ state_begin,
                                                            const int64_t* __restrict__ comp_begin, int32_t* __restrict__ records,
                                                            int64_t record_cap) {
    const seg_node t = seg_locate(meshes, num_meshes);
    const int32_t label = t.live ? labels[state_begin[t.m] + t.id] : SEG_BACKGROUND;
    const int64_t c0 = comp_begin[t.m], c1 = comp_begin[t.m + 1];
    // (a label beyond the volume's rows or the cap writes nothing: no record row outside [0, record_cap) is ever formed)
    int64_t row = label >= 0 && c0 + label < c1 && c0 + label < record_cap ? c0 + label : -1;
    const int lane = threadIdx.x & 63;
    const int at[3] = {t.i, t.j, t.k};
    for (int round = 0; round < SEG_RECORD_ROUNDS; ++round) {
        const unsigned long long pending = __ballot(row >= 0);
        if (pending == 0ull) break;  // (uniform)
        const int leader = __ffsll((long long)pending) - 1;
        const int64_t shared = __shfl(row, leader, 64);
        const bool in = row == shared;
        int lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = in ? at[a] : INT_MAX, hi[a] = in ? at[a] : -1;
            for (int off = 32; off > 0; off >>= 1) {
                lo[a] = min(lo[a], __shfl_xor(lo[a], off, 64));
                hi[a] = max(hi[a], __shfl_xor(hi[a], off, 64));
            }
        }
        // (lanes hold ascending nodes: the leader's own is the smallest of the group)
        const int group = __popcll(__ballot(in));
        if (lane == leader) seg_record_add(records + shared * SEG_RECORD, group, (int32_t)t.id, lo, hi);
        if (in) row = -1;
    }
    if (row >= 0) seg_record_add(records + row * SEG_RECORD, 1, (int32_t)t.id, at, at);
}

__global__ __launch_bounds__(SEG_BLOCK) void k_component_states(const omgx_mesh* __restrict__ outs, int num_outs,
                                                                const int32_t* __restrict__ picks, const omgx_mesh* __restrict__ volumes,
                                                                const uint8_t* __restrict__ state, const int64_t* __restrict__ state_begin,
                                                                const int32_t* __restrict__ labels, const int64_t* __restrict__ comp_begin,
                                                                const int32_t* __restrict__ records, const int64_t* __restrict__ out_begin,
                                                                uint8_t* __restrict__ out_state) {
    const seg_node t = seg_locate(outs, num_outs);
    if (!t.live) return;
    const int32_t* __restrict__ pick = picks + (int64_t)t.m * 8;  // (uniform: volume, i0, j0, k0, component, mode)
    const int m = pick[0], c = pick[4];
    const omgx_mesh* __restrict__ src = volumes + m;
    // (the offsets are any int32: the sums are made in 64 bits and narrowed only where the node exists)
    const int64_t si = (int64_t)pick[1] + t.i, sj = (int64_t)pick[2] + t.j, sk = (int64_t)pick[3] + t.k;
    const bool in_grid = si >= 0 && si < src->dims[0] && sj >= 0 && sj < src->dims[1] && sk >= 0 && sk < src->dims[2];
    const int64_t at = state_begin[m] + (in_grid ? (si * src->dims[1] + sj) * src->dims[2] + sk : 0);
    const uint8_t s = in_grid ? state[at] : (uint8_t)SEG_FREE;
    const int32_t label = in_grid ? labels[at] : SEG_BACKGROUND;
    out_state[out_begin[t.m] + t.id] =
        seg_pick_state(in_grid, s, label, (int32_t)(c - comp_begin[m]), records + (int64_t)c * SEG_RECORD, (int)si, (int)sj, (int)sk, pick[5]);
}

// comp_begin [M+1] on the host: from 0, never decreasing, at most 2^31 - 1 rows -> OMGX_OK, OMGX_ERR_INVALID, OMGX_ERR_UNSUPPORTED.
int check_comp_begin(const int64_t* h_comp_begin, int32_t M) {
    if (h_comp_begin[0] != 0) return OMGX_ERR_INVALID;
    for (int32_t m = 0; m < M; ++m)
        if (h_comp_begin[m + 1] < h_comp_begin[m]) return OMGX_ERR_INVALID;
    return h_comp_begin[M] > 0x7fffffffll ? OMGX_ERR_UNSUPPORTED : OMGX_OK;
}

}  // namespace

extern "C" int64_t omgx_label_workspace_bytes(const omgx_mesh* h_volumes, int32_t num_volumes) {
    if (num_volumes < 0) return OMGX_ERR_INVALID;
    if (num_volumes == 0) return 0;
    int64_t wg = 0;
    const int status = mesh_check_volumes(h_volumes, num_volumes, -1, SEG_BLOCK, &wg);
    return status != OMGX_OK ? status : wg * (int64_t)SEG_WORKSPACE_PER_WORKGROUP;
}

extern "C" int omgx_label_components(const uint8_t* state, int64_t state_elems, const int64_t* state_begin, const int64_t* h_state_begin,
                                     const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, int32_t select,
                                     int32_t connectivity, void* workspace, int32_t* labels, int32_t* counts, void* stream) {
    const int32_t M = num_volumes;
    if (M < 0 || state_elems < 0 || select < 1 || select > 3) return OMGX_ERR_INVALID;
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return OMGX_ERR_INVALID;
    if (M == 0) return OMGX_OK;
    if (!state || !state_begin || !h_state_begin || !volumes || !h_volumes || !workspace || !labels || !counts) return OMGX_ERR_INVALID;
    int64_t wg = 0;
    const int status = mesh_check_batch(h_volumes, M, h_state_begin, state_elems, -1, SEG_BLOCK, &wg);
    if (status != OMGX_OK) return status;
    hipStream_t s = (hipStream_t)stream;
    int32_t* parent = (int32_t*)workspace;
    int32_t* totals = parent + wg * SEG_BLOCK;
    uint8_t* ranks = (uint8_t*)(totals + wg);
    const int order = seg_order(connectivity);
    // elements outside every volume's range: -1
    const hipError_t e = hipMemsetAsync(labels, 0xff, (size_t)state_elems * sizeof(int32_t), s);
    if (e != hipSuccess) return omgx_set_error("hipMemsetAsync(labels)", e);
    hipLaunchKernelGGL(k_label_local, dim3((unsigned)wg), dim3(SEG_BLOCK), 0, s, volumes, (int)M, state, state_begin, (int)select, order, parent);
    OMGX_CHECK_LAUNCH("k_label_local");
    hipLaunchKernelGGL(k_label_border, dim3((unsigned)wg), dim3(SEG_BLOCK), 0, s, volumes, (int)M, order, parent);
    OMGX_CHECK_LAUNCH("k_label_border");
    hipLaunchKernelGGL(k_label_count, dim3((unsigned)wg), dim3(SEG_BLOCK), 0, s, volumes, (int)M, parent, totals, ranks);
    OMGX_CHECK_LAUNCH("k_label_count");
    hipLaunchKernelGGL(k_label_scan, dim3((unsigned)M), dim3(SEG_BLOCK), 0, s, volumes, totals, counts);
    OMGX_CHECK_LAUNCH("k_label_scan");
    hipLaunchKernelGGL(k_label_write, dim3((unsigned)wg), dim3(SEG_BLOCK), 0, s, volumes, (int)M, parent, totals, ranks, state_begin, labels);
    OMGX_CHECK_LAUNCH("k_label_write");
    return OMGX_OK;
}

extern "C" int omgx_component_records(const int32_t* labels, int64_t state_elems, const int64_t* state_begin, const int64_t* h_state_begin,
                                      const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, const int64_t* comp_begin,
                                      const int64_t* h_comp_begin, int32_t* records, int64_t record_cap, void* stream) {
    const int32_t M = num_volumes;
    if (M < 0 || state_elems < 0 || record_cap < 0) return OMGX_ERR_INVALID;
    if (M == 0) return OMGX_OK;
    if (!labels || !state_begin || !h_state_begin || !volumes || !h_volumes || !comp_begin || !h_comp_begin) return OMGX_ERR_INVALID;
    int64_t wg = 0;
    const int status = mesh_check_batch(h_volumes, M, h_state_begin, state_elems, -1, SEG_BLOCK, &wg);
    if (status == OMGX_ERR_INVALID) return status;
    const int rows_status = check_comp_begin(h_comp_begin, M);
    if (rows_status == OMGX_ERR_INVALID || record_cap < h_comp_begin[M] || (h_comp_begin[M] > 0 && !records)) return OMGX_ERR_INVALID;
    if (status != OMGX_OK || rows_status != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    const int64_t rows = h_comp_begin[M];
    if (rows == 0) return OMGX_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_records_init, dim3((unsigned)((rows + SEG_BLOCK - 1) / SEG_BLOCK)), dim3(SEG_BLOCK), 0, s, records, rows);
    OMGX_CHECK_LAUNCH("k_records_init");
    hipLaunchKernelGGL(k_records_fill, dim3((unsigned)wg), dim3(SEG_BLOCK), 0, s, volumes, (int)M, labels, state_begin, comp_begin, records, rows);
    OMGX_CHECK_LAUNCH("k_records_fill");
    return OMGX_OK;
}

extern "C" int omgx_component_states(const uint8_t* state, int64_t state_elems, const int64_t* state_begin, const int64_t* h_state_begin,
                                     const omgx_mesh* volumes, const omgx_mesh* h_volumes, int32_t num_volumes, const int32_t* labels,
                                     const int64_t* comp_begin, const int64_t* h_comp_begin, const int32_t* records, int64_t num_records,
                                     const int32_t* picks, const int32_t* h_picks, const omgx_mesh* out_volumes,
                                     const omgx_mesh* h_out_volumes, int32_t num_picks, const int64_t* out_begin, const int64_t* h_out_begin,
                                     uint8_t* out_state, int64_t out_elems, void* stream) {
    const int32_t M = num_volumes, K = num_picks;
    if (M < 0 || K < 0 || state_elems < 0 || num_records < 0 || out_elems < 0) return OMGX_ERR_INVALID;
    if (K == 0) return OMGX_OK;
    if (M == 0) return OMGX_ERR_INVALID;  // a pick names a volume
    if (!state || !state_begin || !h_state_begin || !volumes || !h_volumes || !labels || !comp_begin || !h_comp_begin || !records) return OMGX_ERR_INVALID;
    if (!picks || !h_picks || !out_volumes || !h_out_volumes || !out_begin || !h_out_begin || !out_state) return OMGX_ERR_INVALID;
    int64_t wg = 0, out_wg = 0;
    const int status = mesh_check_batch(h_volumes, M, h_state_begin, state_elems, -1, SEG_BLOCK, &wg);
    const int out_status = mesh_check_batch(h_out_volumes, K, h_out_begin, out_elems, -1, SEG_BLOCK, &out_wg);
    if (status == OMGX_ERR_INVALID || out_status == OMGX_ERR_INVALID) return OMGX_ERR_INVALID;
    const int rows_status = check_comp_begin(h_comp_begin, M);
    if (rows_status == OMGX_ERR_INVALID || num_records < h_comp_begin[M]) return OMGX_ERR_INVALID;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t* p = h_picks + (int64_t)k * 8;
        if (p[0] < 0 || p[0] >= M || p[4] < h_comp_begin[p[0]] || p[4] >= h_comp_begin[p[0] + 1]) return OMGX_ERR_INVALID;
        if ((p[5] != 0 && p[5] != 1) || p[6] != 0 || p[7] != 0) return OMGX_ERR_INVALID;
    }
    if (status != OMGX_OK || out_status != OMGX_OK || rows_status != OMGX_OK) return OMGX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_component_states, dim3((unsigned)out_wg), dim3(SEG_BLOCK), 0, (hipStream_t)stream, out_volumes, (int)K, picks, volumes, state,
                       state_begin, labels, comp_begin, records, out_begin, out_state);
    OMGX_CHECK_LAUNCH("k_component_states");
    return OMGX_OK;
}
