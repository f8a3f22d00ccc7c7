// omg_mesh_sdf.hip — signed distance grids from triangle meshes (include/omg_hip.h section 12, ABI 14).
//
// k_mesh_sdf: one thread per grid node, one workgroup per 256 nodes of ONE mesh of a ragged batch; the mesh's faces stream
// through LDS tile by tile (mesh_stage_faces, omg_mesh_common.h), every lane reading the same face at a time (LDS
// broadcast), like k_point_cloud_sdf (omg_kernels.hip).  All arithmetic is float64 with contraction off, one operation per
// line of the specification scenes.closest_point_on_triangle / scenes.mesh_sdf (omg-planner_amd/scenes.py), so the distance
// has the specification's bits; the sign is the generalised winding number's decision |w| > 0.5, summed in float64 with the
// device library's atan2 (the sum itself is not pinned, only the decision: DESIGN.md section 7d).
#include "omg_mesh_common.h"
#include "omg_mesh_sdf_body.h"

#pragma clang fp contract(off)

#define MSDF_BLOCK OMGX_MESH_SDF_NODES_PER_WORKGROUP

namespace {

__global__ __launch_bounds__(MSDF_BLOCK) void k_mesh_sdf(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                          const omgx_mesh* __restrict__ meshes, int num_meshes,
                                                          float* __restrict__ out) {
    __shared__ double tile[OMGX_MESH_FACE_TILE * 9];
    // the mesh of this workgroup (uniform: scalar loads); idle lanes of the last workgroup redo the last node and store nothing
    const volume_node n = volume_locate(meshes, num_meshes, blockIdx.x, threadIdx.x, MSDF_BLOCK);
    const omgx_mesh ms = meshes[n.m];
    double p[3];
    volume_node_point(ms, n.idc, p);  // (a mesh has at most 2^31 nodes: the index and the 32-bit division hold)
    const double px = p[0], py = p[1], pz = p[2];

    const double* __restrict__ mv = verts + (int64_t)ms.vert_begin * 3;
    const int32_t* __restrict__ mf = faces + (int64_t)ms.face_begin * 3;
    const int nv = ms.vert_count, nf = ms.face_count;

    double best = 1.0e300, wsum = 0.0;
    for (int t0 = 0; t0 < nf; t0 += OMGX_MESH_FACE_TILE) {
        const int cnt = min(OMGX_MESH_FACE_TILE, nf - t0);
        mesh_stage_faces(tile, mv, mf, nv, t0, cnt);
        for (int q = 0; q < cnt; ++q) {
            mesh_sdf_pair(px, py, pz, tile + q * 9, best, wsum);
        }
    }
    if (n.live) {
        const double w = wsum * 0.15915494309189535;  // (1 / 4 pi) * 2 * sum
        const double d = sqrt(best);
        out[ms.out_offset + n.id] = (float)(fabs(w) > 0.5 ? -d : d);
    }
}

}  // namespace

extern "C" int32_t omgx_mesh_sdf_tile(void) { return OMGX_MESH_FACE_TILE; }

extern "C" int omgx_mesh_sdf(const double* verts, const int32_t* faces, const omgx_mesh* meshes, const omgx_mesh* h_meshes,
                             int32_t num_meshes, float* out, void* stream) {
    if (!verts || !faces || !meshes || !h_meshes || !out || num_meshes < 1) return OMGX_ERR_INVALID;
    bool too_big = false;
    int64_t wg = 0;
    for (int32_t m = 0; m < num_meshes; ++m) {
        const omgx_mesh& h = h_meshes[m];
        const int volume = mesh_check_volume(h);
        if (mesh_check_ranges(h) != OMGX_OK || volume == OMGX_ERR_INVALID) return OMGX_ERR_INVALID;
        if (h.first_workgroup != wg) return OMGX_ERR_INVALID;  // the prefix table: workgroups of the meshes before this one
        if (volume != OMGX_OK) too_big = true;  // reported after an invalid record of any mesh
        wg += (mesh_node_count(h) + MSDF_BLOCK - 1) / MSDF_BLOCK;
    }
    if (too_big || wg > 0x7fffffffll) return OMGX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_mesh_sdf, dim3((unsigned)wg), dim3(MSDF_BLOCK), 0, (hipStream_t)stream, verts, faces, meshes, num_meshes, out);
    OMGX_CHECK_LAUNCH("k_mesh_sdf");
    return OMGX_OK;
}
