// omg_fusion_body.h — what the kernels of omg_fusion.hip do for one node of a volume: what one depth view says about it, the
// state the views add up to, and one windowed-minimum step of the distance transform along a line, as functions that also
// compile for the host, so that the arithmetic can be stepped through and compared with omg-planner_amd/fusion.py without a GPU.
// float64 with + - * /, floor and sqrt only, one rounded operation per operation of the specification, in its order.  No HIP
// built-ins here.
#pragma once
#include <cmath>
#include <cstdint>

#include "omg_volume_body.h"  // fusion_node_point

#if defined(__HIPCC__)
#define FUSION_HD __host__ __device__ __forceinline__
#else
#define FUSION_HD inline
#endif

#pragma clang fp contract(off)

#define FUSION_FREE 0
#define FUSION_SURFACE 1
#define FUSION_UNKNOWN 2
// what fusion_view_says returns
#define FUSION_SAYS_NOTHING 0
#define FUSION_SAYS_FREE 1
#define FUSION_SAYS_SURFACE 2

// What the view (fx, fy, cx, cy, rows of cam_from_grid) with the image img [H][W] says about the point p.  The row and the
// column are 0 unless the pixel lies inside the image, so that no point can form an address outside it.
FUSION_HD int fusion_view_says(const double* view, const double* img, int H, int W, const double* p, double band, double near) {
    const double q0 = ((view[4] * p[0] + view[5] * p[1]) + view[6] * p[2]) + view[7];
    const double q1 = ((view[8] * p[0] + view[9] * p[1]) + view[10] * p[2]) + view[11];
    const double z = ((view[12] * p[0] + view[13] * p[1]) + view[14] * p[2]) + view[15];
    const double cf = floor((view[0] * (q0 / z) + view[2]) + 0.5), rf = floor((view[1] * (q1 / z) + view[3]) + 0.5);
    // (compared as doubles: NaN, inf and what no int holds are outside)
    const bool seen = z > near && cf >= 0.0 && cf <= (double)(W - 1) && rf >= 0.0 && rf <= (double)(H - 1);
    const int c = seen ? (int)cf : 0, r = seen ? (int)rf : 0;
    const double d = img[(int64_t)r * W + c];
    if (!(seen && d > 0.0)) return FUSION_SAYS_NOTHING;
    const double lo = d - band, hi = d + band;
    if (z < lo) return FUSION_SAYS_FREE;
    return lo <= z && z <= hi ? FUSION_SAYS_SURFACE : FUSION_SAYS_NOTHING;
}

FUSION_HD uint8_t fusion_state(bool surface, bool free_) { return surface ? FUSION_SURFACE : free_ ? FUSION_FREE : FUSION_UNKNOWN; }

FUSION_HD bool fusion_occupied(uint8_t state, int unknown_occupied) {
    return state == FUSION_SURFACE || (state != FUSION_FREE && unknown_occupied != 0);
}

// The two channels of a node in one word: the squared distance to the nearest occupied node in the low 16 bits, to the nearest
// free node in the high 16 bits, both saturated at r2 = radius^2 <= 65025.  Before the first pass: 0 to the node's own set.
FUSION_HD uint32_t fusion_seed(bool occupied, uint32_t r2) { return occupied ? r2 << 16 : r2; }

// One pass for the node at position a of a line of n nodes: both channels' min over the positions a + d, |d| <= radius, inside
// the line of value + d*d, saturated at r2.  at: the node's own word, its neighbours along the line `stride` words apart.
FUSION_HD uint32_t fusion_line_pass(const uint32_t* at, int64_t stride, int a, int n, int radius, uint32_t r2) {
    const int first = a < radius ? -a : -radius, last = n - 1 - a < radius ? n - 1 - a : radius;
    uint32_t occ = r2, fre = r2;
    for (int d = first; d <= last; ++d) {
        const uint32_t w = at[(int64_t)d * stride], dd = (uint32_t)(d * d);
        const uint32_t o = (w & 0xffffu) + dd, f = (w >> 16) + dd;
        occ = o < occ ? o : occ, fre = f < fre ? f : fre;
    }
    return occ | (fre << 16);
}

// The signed distance of a node after the last pass.  A node is occupied iff its distance to the occupied set is zero.
FUSION_HD float fusion_value(uint32_t w, double delta) {
    const uint32_t occ = w & 0xffffu, fre = w >> 16;
    const double inside = -((sqrt((double)fre) - 0.5) * delta), outside = (sqrt((double)occ) - 0.5) * delta;
    return (float)(occ == 0u ? inside : outside);
}
