// omg_mesh_common.h — what the translation units that take omgx_mesh records share: the face tile that k_mesh_sdf and
// k_mesh_raycast stage in LDS (omg_mesh_sdf.hip, omg_grasp.hip), the checks on one host omgx_mesh record (include/omg_hip.h
// sections 12 and 13), on a batch of volumes and on a view table (omg_surface.hip, omg_fusion.hip, omg_segment.hip, omg_plane.hip,
// omg_tsdf.hip: sections 16 to 20), and through omg_volume_body.h the way a workgroup of their kernels finds its volume.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "omg_host.h"
#include "omg_image_body.h"   // the checks of camera rows and of the pixel count
#include "omg_volume_body.h"  // a workgroup's volume and a thread's node of it, on the device

// Faces of a mesh staged in LDS at a time (omgx_mesh_sdf_tile()), 9 doubles each: a, b, c.
#define OMGX_MESH_FACE_TILE 256
static_assert(OMGX_MESH_FACE_TILE == OMGX_MESH_SDF_NODES_PER_WORKGROUP && OMGX_MESH_FACE_TILE == OMGX_RAYCAST_RAYS_PER_WORKGROUP,
              "mesh_stage_faces moves one face per thread");

// The faces [t0, t0 + cnt) of a mesh (mv, mf: its rows of the vertex and face pools, nv vertices) into tile[cnt * 9], between two
// barriers: every thread of the workgroup must call it, with cnt <= OMGX_MESH_FACE_TILE.
__device__ __forceinline__ void mesh_stage_faces(double* tile, const double* __restrict__ mv, const int32_t* __restrict__ mf, int nv,
                                                 int t0, int cnt) {
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
        const int32_t* f = mf + (int64_t)(t0 + (int)threadIdx.x) * 3;
        for (int c = 0; c < 3; ++c) {
            // the wrappers reject indices outside the mesh; clamped here so that no index can read outside the pool
            const int v = min(max(f[c], 0), nv - 1);
            for (int a = 0; a < 3; ++a) tile[threadIdx.x * 9 + c * 3 + a] = mv[(int64_t)v * 3 + a];
        }
    }
    __syncthreads();
}

// One host record's rows of the vertex and face pools -> OMGX_OK or OMGX_ERR_INVALID.
static inline int mesh_check_ranges(const omgx_mesh& h) {
    return h.vert_begin < 0 || h.face_begin < 0 || h.vert_count < 1 || h.face_count < 1 ? OMGX_ERR_INVALID : OMGX_OK;
}

static inline int64_t mesh_node_count(const omgx_mesh& h) { return (int64_t)h.dims[0] * h.dims[1] * h.dims[2]; }
// One host record's volume -> OMGX_OK, OMGX_ERR_INVALID, or OMGX_ERR_UNSUPPORTED for more than 2^31 nodes (an invalid field is
// reported first).
static inline int mesh_check_volume(const omgx_mesh& h) {
    if (h.out_offset < 0) return OMGX_ERR_INVALID;
    if (!(h.delta > 0.0) || !std::isfinite(h.delta)) return OMGX_ERR_INVALID;
    if (h.dims[0] < 1 || h.dims[1] < 1 || h.dims[2] < 1) return OMGX_ERR_INVALID;
    if (!(h.sample_offset == 0.0 || h.sample_offset == 0.5)) return OMGX_ERR_INVALID;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(h.origin[a])) return OMGX_ERR_INVALID;
    return mesh_node_count(h) > (int64_t)1 << 31 ? OMGX_ERR_UNSUPPORTED : OMGX_OK;
}

// The host copies of a batch of volume records -> OMGX_OK, OMGX_ERR_INVALID or OMGX_ERR_UNSUPPORTED (an invalid field of any
// record first); first_workgroup must be the prefix table at `per_workgroup` nodes per workgroup; *workgroups: all of them.
// pool_elems < 0: the volumes' place in the pool is not checked.
static inline int mesh_check_volumes(const omgx_mesh* h_meshes, int32_t num_meshes, int64_t pool_elems, int per_workgroup,
                                     int64_t* workgroups) {
    if (!h_meshes || num_meshes < 1) return OMGX_ERR_INVALID;
    bool too_big = false;
    int64_t wg = 0;
    for (int32_t m = 0; m < num_meshes; ++m) {
        const omgx_mesh& h = h_meshes[m];
        const int volume = mesh_check_volume(h);
        if (volume == OMGX_ERR_INVALID || h.first_workgroup != wg) return OMGX_ERR_INVALID;
        const int64_t samples = mesh_node_count(h);
        if (samples > 0x7fffffffll) too_big = true;
        else if (pool_elems >= 0 && (samples > pool_elems || h.out_offset > pool_elems - samples)) return OMGX_ERR_INVALID;
        wg += (samples + per_workgroup - 1) / per_workgroup;
        if (wg > 0x7fffffffll) too_big = true;
    }
    *workgroups = wg;
    return too_big ? OMGX_ERR_UNSUPPORTED : OMGX_OK;
}

// Do two of the ranges [begin, begin + count) overlap?  (begins >= 0; empty ranges overlap nothing)
static inline bool mesh_ranges_overlap(std::vector<std::pair<int64_t, int64_t>>& r) {
    std::sort(r.begin(), r.end());
    int64_t end = 0;
    for (const auto& x : r) {
        if (x.second == 0) continue;
        if (x.first < end) return true;
        end = x.first + x.second;
    }
    return false;
}

// The state ranges of the volumes: inside [0, state_elems), no two overlapping -> OMGX_OK or OMGX_ERR_INVALID.  (node counts
// above 2^31 - 1 are the caller's OMGX_ERR_UNSUPPORTED; their ranges are checked all the same)
static inline int mesh_check_state_ranges(const omgx_mesh* h_volumes, int32_t M, const int64_t* h_state_begin, int64_t state_elems) {
    std::vector<std::pair<int64_t, int64_t>> r;
    for (int32_t m = 0; m < M; ++m) {
        const int64_t nodes = mesh_node_count(h_volumes[m]), begin = h_state_begin[m];
        if (begin < 0 || nodes > state_elems || begin > state_elems - nodes) return OMGX_ERR_INVALID;
        r.emplace_back(begin, nodes);
    }
    return mesh_ranges_overlap(r) ? OMGX_ERR_INVALID : OMGX_OK;
}

// mesh_check_volumes, then mesh_check_state_ranges -> OMGX_OK, OMGX_ERR_INVALID, or the records' OMGX_ERR_UNSUPPORTED, which
// comes last: the caller reports it only after the OMGX_ERR_INVALID of its own further checks.
static inline int mesh_check_batch(const omgx_mesh* h_volumes, int32_t M, const int64_t* h_state_begin, int64_t state_elems,
                                   int64_t pool_elems, int per_workgroup, int64_t* workgroups) {
    const int status = mesh_check_volumes(h_volumes, M, pool_elems, per_workgroup, workgroups);
    if (status == OMGX_ERR_INVALID) return status;
    return mesh_check_state_ranges(h_volumes, M, h_state_begin, state_elems) != OMGX_OK ? OMGX_ERR_INVALID : status;
}

// Do two of the volumes overlap in the pool they are written to (at out_offset)?
static inline bool mesh_pool_ranges_overlap(const omgx_mesh* h_volumes, int32_t M) {
    std::vector<std::pair<int64_t, int64_t>> in_pool;
    for (int32_t m = 0; m < M; ++m) in_pool.emplace_back(h_volumes[m].out_offset, mesh_node_count(h_volumes[m]));
    return mesh_ranges_overlap(in_pool);
}

// The host copies of a view table [V][16] (fx, fy, cx, cy, rows of cam_from_grid) and of the volumes' view ranges [M][2] (first,
// count) -> OMGX_ERR_INVALID for a field that is not finite, a focal length of zero or a range outside [0, V]; then
// OMGX_ERR_UNSUPPORTED for V * H * W > 2^31 - 1, which the caller reports after its other checks; OMGX_OK.  (V > 0: H, W >= 1)
static inline int mesh_check_views(const double* h_views, int32_t V, int32_t H, int32_t W, const int32_t* h_view_range, int32_t M) {
    if (image_check_rows(h_views, V, 16) != OMGX_OK) return OMGX_ERR_INVALID;
    for (int32_t m = 0; m < M; ++m) {
        const int64_t first = h_view_range[2 * m], count = h_view_range[2 * m + 1];
        if (first < 0 || count < 0 || first + count > V) return OMGX_ERR_INVALID;
    }
    return image_pixels_fit(V, H, W) ? OMGX_OK : OMGX_ERR_UNSUPPORTED;
}
