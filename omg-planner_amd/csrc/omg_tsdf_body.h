// omg_tsdf_body.h — what the kernels of omg_tsdf.hip do for one node of a volume: what one depth view adds to its pair (D, the
// averaged truncated distance; W, the accumulated weight), the state byte of a pair, and the pair blended into the distance
// transform's value, as functions that also compile for the host, so that the arithmetic can be stepped through and compared
// with omg-planner_amd/tsdf.py without a GPU.  float64 with + - * /, floor, fabs and comparisons only, one rounded operation per
// operation of the specification, in its order.  No HIP built-ins here.  The node's point is omg_fusion_body.h's.
#pragma once
#include "omg_fusion_body.h"

#pragma clang fp contract(off)

// What the view (fx, fy, cx, cy, rows of cam_from_grid) with the image img [H][W] says about the point p: false for nothing,
// otherwise *t = the truncated distance along the optical axis.  The projection, the pixel and the depth are fusion_view_says's,
// operation for operation; the row and the column are 0 unless the pixel lies inside the image.
FUSION_HD bool tsdf_view_updates(const double* view, const double* img, int H, int W, const double* p, double trunc, double near, double* t) {
    const double q0 = ((view[4] * p[0] + view[5] * p[1]) + view[6] * p[2]) + view[7];
    const double q1 = ((view[8] * p[0] + view[9] * p[1]) + view[10] * p[2]) + view[11];
    const double z = ((view[12] * p[0] + view[13] * p[1]) + view[14] * p[2]) + view[15];
    const double cf = floor((view[0] * (q0 / z) + view[2]) + 0.5), rf = floor((view[1] * (q1 / z) + view[3]) + 0.5);
    const bool seen = z > near && cf >= 0.0 && cf <= (double)(W - 1) && rf >= 0.0 && rf <= (double)(H - 1);
    const int c = seen ? (int)cf : 0, r = seen ? (int)rf : 0;
    const double d = img[(int64_t)r * W + c];
    const double s = d - z;
    *t = s < trunc ? s : trunc;
    return seen && d > 0.0 && s >= -trunc;
}

// The pair a node starts from: (0, 0), or with merge the stored pair, (0, 0) if !(W > 0).
FUSION_HD void tsdf_start(bool merge, float stored_d, float stored_w, double* D, double* Wt) {
    const bool live = merge && stored_w > 0.0f;
    *D = live ? (double)stored_d : 0.0, *Wt = live ? (double)stored_w : 0.0;
}

// One update with the truncated distance t and the view's weight w > 0.
FUSION_HD void tsdf_update(double* D, double* Wt, double t, double w, double wmax) {
    const double wn = *Wt + w;
    *D = (*Wt * *D + w * t) / wn;
    *Wt = wn < wmax ? wn : wmax;
}

FUSION_HD uint8_t tsdf_state(float D, float Wt, float min_weight) {
    return !(Wt >= min_weight) ? FUSION_UNKNOWN : D < 0.0f ? FUSION_SURFACE : FUSION_FREE;
}

// E: the distance transform's value of the node.  a = |D| / trunc; a >= 1 ? E : D + a * (E - D) where W >= min_weight.
FUSION_HD float tsdf_blend(float D, float Wt, float E, double trunc, float min_weight) {
    if (!(Wt >= min_weight)) return E;
    const double d = (double)D, e = (double)E;
    const double a = fabs(d) / trunc;
    return a >= 1.0 ? E : (float)(d + a * (e - d));
}
