// omg_surface.hip — triangle meshes from distance volumes by naive surface nets (include/omg_hip.h section 16).
//
// One thread per sample of ONE volume of a ragged batch, with the cell and the three sample edges anchored there; samples in
// x-major groups of 256 per workgroup, workgroups mapped to volumes by the first_workgroup prefix table as in k_mesh_sdf.  The
// count / scan / gather pattern of k_pixel_count / k_pixel_scan / k_pixel_gather (omg_camera.hip), without atomics:
//   k_surface_count   the cell's corner mask and the crossing edges; vertices, closed edges and open edges per workgroup (ballot +
//                     popcount per wave, the four waves summed in order) and every active cell's rank inside its workgroup
//   k_surface_scan    one workgroup per volume: the workgroup totals become exclusive offsets in place, the volume's totals `counts`
//   k_surface_gather  the flags again; a vertex goes to row offset + rank, a closed crossing edge reads the ranks of its four cells
//                     (and their workgroups' offsets) and writes its two triangles at twice its own scanned rank
// The arithmetic is omg_surface_body.h: float64, contraction off, the bits of scenes.surface_nets.  Plain loads and stores only.
#include <utility>
#include <vector>

#include "omg_mesh_common.h"
#include "omg_surface_body.h"

#pragma clang fp contract(off)

#define SURF_BLOCK OMGX_SURFACE_NODES_PER_WORKGROUP
static_assert(SURF_BLOCK == 256, "four waves per workgroup");
// Workspace: totals [WG][4] int32 (vertices, closed edges, open edges, 0; exclusive offsets per volume after the scan), then the
// rank of every sample's cell among the active cells of its workgroup, [WG * 256] uint8 (0..255; read only for active cells).
#define SURF_TOTALS 4

namespace {

struct surf_thread {
    omgx_mesh ms;
    int64_t id;         // this thread's sample of the volume
    int a[3];           // its coordinates (lanes past the volume's last sample: the last one's)
    unsigned mask;      // corners inside
    bool active;        // the cell exists and has a vertex
    bool closed[3], open[3];  // crossing edges with / without their four cells
    float v[8];
};

// The volume of this workgroup (uniform) and this thread's flags.  Lanes past the last sample of the volume flag nothing.
__device__ __forceinline__ void surf_flags(const float* __restrict__ pool, const omgx_mesh* __restrict__ meshes, int num_meshes,
                                           float level, surf_thread& t) {
    const volume_node n = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, SURF_BLOCK);
    t.ms = meshes[n.m];
    t.id = n.id;
    const bool live = n.live;
    volume_decode(t.ms.dims, n.idc, &t.a[0], &t.a[1], &t.a[2]);
    surface_load_corners(pool + t.ms.out_offset, t.ms.dims, t.a[0], t.a[1], t.a[2], t.v);
#if defined(OMGX_SURFACE_ONE_LOAD)  // measurement build (tools/surface_timing.py --one-load): what the count step costs without its
    for (int c = 1; c < 8; ++c) t.v[c] = t.v[0];  // neighbour loads, the most that staging a tile in LDS could save; wrong meshes
#endif
    t.mask = surface_corner_mask(t.v, level);
    t.active = live && surface_cell_active(t.mask, t.ms.dims, t.a[0], t.a[1], t.a[2]);
    for (int axis = 0; axis < 3; ++axis) {
        const bool cross = live && surface_edge_crosses(t.mask, axis);
        const bool closed = surface_edge_closed(t.ms.dims, t.a, axis);
        t.closed[axis] = cross && closed;
        t.open[axis] = cross && !closed;
    }
}

__device__ __forceinline__ int edges_in(const unsigned long long* b, unsigned long long lanes) {
    return (__popcll(b[0] & lanes) + __popcll(b[1] & lanes)) + __popcll(b[2] & lanes);
}

__global__ __launch_bounds__(SURF_BLOCK) void k_surface_count(const float* __restrict__ pool, const omgx_mesh* __restrict__ meshes,
                                                              int num_meshes, float level, int32_t* __restrict__ totals,
                                                              uint8_t* __restrict__ ranks) {
    __shared__ int wave_count[SURF_BLOCK / 64][3];
    surf_thread t;
    surf_flags(pool, meshes, num_meshes, level, t);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long all = ~0ull, before_me = (1ull << lane) - 1ull;
    const unsigned long long act = __ballot(t.active);
    unsigned long long closed[3], open[3];
    for (int axis = 0; axis < 3; ++axis) closed[axis] = __ballot(t.closed[axis]), open[axis] = __ballot(t.open[axis]);
    if (lane == 0) {
        wave_count[wave][0] = __popcll(act);
        wave_count[wave][1] = edges_in(closed, all);
        wave_count[wave][2] = edges_in(open, all);
    }
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_count[w][0];
    ranks[(int64_t)blockIdx.x * SURF_BLOCK + threadIdx.x] = (uint8_t)(before + __popcll(act & before_me));
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        totals[(int64_t)blockIdx.x * SURF_TOTALS + c] = (wave_count[0][c] + wave_count[1][c]) + (wave_count[2][c] + wave_count[3][c]);
    } else if (threadIdx.x == 3) {
        totals[(int64_t)blockIdx.x * SURF_TOTALS + 3] = 0;
    }
}

// One workgroup per volume walks the volume's workgroup totals 256 at a time, as k_pixel_scan does, for the three columns.
__global__ __launch_bounds__(SURF_BLOCK) void k_surface_scan(const omgx_mesh* __restrict__ meshes, int32_t* __restrict__ totals,
                                                             int32_t* __restrict__ counts) {
    __shared__ int wave_total[SURF_BLOCK / 64][3];
    const omgx_mesh* __restrict__ ms = meshes + blockIdx.x;
    const int64_t samples = (int64_t)ms->dims[0] * ms->dims[1] * ms->dims[2];
    const int n = (int)((samples + SURF_BLOCK - 1) / SURF_BLOCK);
    int32_t* __restrict__ mine = totals + ms->first_workgroup * SURF_TOTALS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry[3] = {0, 0, 0};
    for (int base = 0; base < n; base += SURF_BLOCK) {
        const int i = base + (int)threadIdx.x;
        int v[3], x[3];
        for (int c = 0; c < 3; ++c) {
            v[c] = i < n ? mine[(int64_t)i * SURF_TOTALS + c] : 0;
            x[c] = v[c];
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(x[c], off, 64);
                x[c] += lane >= off ? y : 0;
            }
            if (lane == 63) wave_total[wave][c] = x[c];
        }
        __syncthreads();
        for (int c = 0; c < 3; ++c) {
            int before = 0;
            for (int w = 0; w < wave; ++w) before += wave_total[w][c];
            if (i < n) mine[(int64_t)i * SURF_TOTALS + c] = carry[c] + before + (x[c] - v[c]);
            carry[c] += (wave_total[0][c] + wave_total[1][c]) + (wave_total[2][c] + wave_total[3][c]);
        }
        __syncthreads();  // wave_total is written again
    }
    if (threadIdx.x == 0) {
        int32_t* out = counts + (int64_t)blockIdx.x * 4;
        out[0] = carry[0], out[1] = 2 * carry[1], out[2] = carry[2], out[3] = 0;
    }
}

// The vertex index (local to the mesh) of the cell at sample `id` of the volume whose first workgroup is wg0: its workgroup's
// offset + its rank there.
__device__ __forceinline__ int32_t surf_vertex_index(const int32_t* __restrict__ totals, const uint8_t* __restrict__ ranks, int64_t wg0,
                                                     int64_t id) {
    return totals[(wg0 + id / SURF_BLOCK) * SURF_TOTALS] + (int32_t)ranks[wg0 * SURF_BLOCK + id];
}

__global__ __launch_bounds__(SURF_BLOCK) void k_surface_gather(const float* __restrict__ pool, const omgx_mesh* __restrict__ meshes,
                                                               int num_meshes, float level, const int32_t* __restrict__ totals,
                                                               const uint8_t* __restrict__ ranks, double* __restrict__ verts,
                                                               int64_t vert_cap, int32_t* __restrict__ faces, int64_t face_cap) {
    __shared__ int wave_count[SURF_BLOCK / 64];
    surf_thread t;
    surf_flags(pool, meshes, num_meshes, level, t);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long before_me = (1ull << lane) - 1ull;
    unsigned long long closed[3];
    for (int axis = 0; axis < 3; ++axis) closed[axis] = __ballot(t.closed[axis]);
    if (lane == 0) wave_count[wave] = edges_in(closed, ~0ull);
    __syncthreads();
    const int32_t* __restrict__ mine = totals + (int64_t)blockIdx.x * SURF_TOTALS;
    if (t.active) {
        const int64_t rank = (int64_t)mine[0] + ranks[(int64_t)blockIdx.x * SURF_BLOCK + threadIdx.x];
        const int64_t row = (int64_t)t.ms.vert_begin + rank;
        if (rank < t.ms.vert_count && row < vert_cap) {
            double p[3];
            surface_cell_vertex(t.v, t.mask, level, t.a[0], t.a[1], t.a[2], t.ms.origin, t.ms.delta, t.ms.sample_offset, p);
            verts[row * 3] = p[0], verts[row * 3 + 1] = p[1], verts[row * 3 + 2] = p[2];
        }
    }
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_count[w];
    int64_t edge = (int64_t)mine[1] + before + edges_in(closed, before_me);  // this thread's first closed edge of the volume
    const int64_t step[3] = {(int64_t)t.ms.dims[1] * t.ms.dims[2], (int64_t)t.ms.dims[2], 1};
    for (int axis = 0; axis < 3; ++axis) {
        if (!t.closed[axis]) continue;
        const int64_t tri = 2 * edge;
        ++edge;
        const int64_t row = (int64_t)t.ms.face_begin + tri;
        const bool first = tri < t.ms.face_count && row < face_cap, second = tri + 1 < t.ms.face_count && row + 1 < face_cap;
        if (!first) continue;
        const int64_t s1 = step[(axis + 1) % 3], s2 = step[(axis + 2) % 3], wg0 = t.ms.first_workgroup;
        const int32_t c0 = surf_vertex_index(totals, ranks, wg0, t.id - s1 - s2), c1 = surf_vertex_index(totals, ranks, wg0, t.id - s2);
        const int32_t c2 = surf_vertex_index(totals, ranks, wg0, t.id), c3 = surf_vertex_index(totals, ranks, wg0, t.id - s1);
        int32_t out[6];
        surface_edge_triangles((t.mask & 1u) != 0u, c0, c1, c2, c3, out);
        faces[row * 3] = out[0], faces[row * 3 + 1] = out[1], faces[row * 3 + 2] = out[2];
        if (second) faces[row * 3 + 3] = out[3], faces[row * 3 + 4] = out[4], faces[row * 3 + 5] = out[5];
    }
}

}  // namespace

extern "C" int64_t omgx_surface_workspace_bytes(const omgx_mesh* h_meshes, int32_t num_meshes) {
    int64_t wg = 0;
    const int status = mesh_check_volumes(h_meshes, num_meshes, -1, SURF_BLOCK, &wg);
    if (status != OMGX_OK) return status;
    return wg * (int64_t)(SURF_TOTALS * sizeof(int32_t)) + wg * SURF_BLOCK;
}

extern "C" int omgx_surface_count(const float* pool, int64_t pool_elems, const omgx_mesh* meshes, const omgx_mesh* h_meshes,
                                  int32_t num_meshes, float level, void* workspace, int32_t* counts, void* stream) {
    if (!pool || !meshes || !h_meshes || !workspace || !counts || pool_elems < 0 || std::isnan(level)) return OMGX_ERR_INVALID;
    int64_t wg = 0;
    const int status = mesh_check_volumes(h_meshes, num_meshes, pool_elems, SURF_BLOCK, &wg);
    if (status != OMGX_OK) return status;
    int32_t* totals = (int32_t*)workspace;
    hipLaunchKernelGGL(k_surface_count, dim3((unsigned)wg), dim3(SURF_BLOCK), 0, (hipStream_t)stream, pool, meshes, (int)num_meshes, level, totals,
                       (uint8_t*)(totals + wg * SURF_TOTALS));
    OMGX_CHECK_LAUNCH("k_surface_count");
    hipLaunchKernelGGL(k_surface_scan, dim3((unsigned)num_meshes), dim3(SURF_BLOCK), 0, (hipStream_t)stream, meshes, totals, counts);
    OMGX_CHECK_LAUNCH("k_surface_scan");
    return OMGX_OK;
}

extern "C" int omgx_surface_gather(const float* pool, int64_t pool_elems, const omgx_mesh* meshes, const omgx_mesh* h_meshes,
                                   int32_t num_meshes, float level, const void* workspace, double* verts, int64_t vert_cap,
                                   int32_t* faces, int64_t face_cap, void* stream) {
    if (!pool || !meshes || !h_meshes || !workspace || pool_elems < 0 || std::isnan(level) || vert_cap < 0 || face_cap < 0) return OMGX_ERR_INVALID;
    if ((vert_cap > 0 && !verts) || (face_cap > 0 && !faces)) return OMGX_ERR_INVALID;
    int64_t wg = 0;
    const int status = mesh_check_volumes(h_meshes, num_meshes, pool_elems, SURF_BLOCK, &wg);
    if (status == OMGX_ERR_INVALID) return status;
    std::vector<std::pair<int64_t, int64_t>> vr, fr;
    for (int32_t m = 0; m < num_meshes; ++m) {
        const omgx_mesh& h = h_meshes[m];
        if (h.vert_begin < 0 || h.vert_count < 0 || h.face_begin < 0 || h.face_count < 0) return OMGX_ERR_INVALID;
        vr.emplace_back(h.vert_begin, h.vert_count), fr.emplace_back(h.face_begin, h.face_count);
    }
    if (mesh_ranges_overlap(vr) || mesh_ranges_overlap(fr)) return OMGX_ERR_INVALID;
    if (status != OMGX_OK) return status;
    if (vert_cap == 0 && face_cap == 0) return OMGX_OK;
    const int32_t* totals = (const int32_t*)workspace;
    hipLaunchKernelGGL(k_surface_gather, dim3((unsigned)wg), dim3(SURF_BLOCK), 0, (hipStream_t)stream, pool, meshes, (int)num_meshes, level, totals,
                       (const uint8_t*)(totals + wg * SURF_TOTALS), verts, vert_cap, faces, face_cap);
    OMGX_CHECK_LAUNCH("k_surface_gather");
    return OMGX_OK;
}
