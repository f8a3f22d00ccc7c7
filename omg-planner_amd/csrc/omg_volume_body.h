// omg_volume_body.h — what every kernel over a ragged batch of volumes (omgx_mesh records) does first: find the volume of its
// workgroup in the first_workgroup prefix table, this thread's node of it, the node's coordinates and its point.  Functions of
// plain integers that also compile for the host, so that the search can be stepped through and compared with numpy without a GPU
// (tests/test_volume_locate_cpu.py).  No HIP built-ins here: the kernels pass blockIdx.x and threadIdx.x.
#pragma once
#include <cstdint>

#include "../../include/omg_hip.h"

#if defined(__HIPCC__)
#define VOLUME_HD __host__ __device__ __forceinline__
#else
#define VOLUME_HD inline
#endif

#pragma clang fp contract(off)

// One thread's node of a launch of `nodes_per_workgroup` consecutive nodes (x-major) per workgroup.
struct volume_node {
    int m;                   // the volume of the workgroup (uniform)
    int64_t id0, id, total;  // the workgroup's first node, this thread's node, the volume's nodes
    bool live;               // id < total; lanes past the last node of the volume repeat it and write nothing:
    uint32_t idc;            // min(id, total - 1)  (a volume has at most 2^31 nodes)
};

// The volume of workgroup `block` is the last one whose first_workgroup is <= block.
VOLUME_HD volume_node volume_locate(const omgx_mesh* __restrict__ meshes, int num_meshes, uint32_t block, uint32_t thread, int nodes_per_workgroup) {
    int lo = 0, hi = num_meshes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (meshes[mid].first_workgroup <= (int64_t)block) lo = mid; else hi = mid - 1;
    }
    const omgx_mesh* ms = meshes + lo;
    volume_node n;
    n.m = lo;
    n.total = (int64_t)ms->dims[0] * ms->dims[1] * ms->dims[2];
    n.id0 = ((int64_t)block - ms->first_workgroup) * nodes_per_workgroup;
    n.id = n.id0 + thread;
    n.live = n.id < n.total;
    n.idc = (uint32_t)(n.live ? n.id : n.total - 1);
    return n;
}

// idc = (i * dims[1] + j) * dims[2] + k, in 32-bit division: the index and dims[1] * dims[2] are at most 2^31.
VOLUME_HD void volume_decode(const int32_t* dims, uint32_t idc, int* i, int* j, int* k) {
    const uint32_t dz = (uint32_t)dims[2], plane = dz * (uint32_t)dims[1], rest = idc % plane;
    *i = (int)(idc / plane), *j = (int)(rest / dz), *k = (int)(rest % dz);
}

// p = origin + ((i, j, k) + sample_offset) * delta, per component.
VOLUME_HD void fusion_node_point(const double* origin, double delta, double sample_offset, int i, int j, int k, double* p) {
    p[0] = origin[0] + ((double)i + sample_offset) * delta;
    p[1] = origin[1] + ((double)j + sample_offset) * delta;
    p[2] = origin[2] + ((double)k + sample_offset) * delta;
}

// The point of node idc of the volume ms.
VOLUME_HD void volume_node_point(const omgx_mesh& ms, uint32_t idc, double* p) {
    int i, j, k;
    volume_decode(ms.dims, idc, &i, &j, &k);
    fusion_node_point(ms.origin, ms.delta, ms.sample_offset, i, j, k, p);
}
