// omg_plane_body.h — what the kernels of omg_plane.hip do for one pixel, one hypothesis or one node: the pixel's point and whether
// it is valid, the plane of a pixel triple, the residual and the tests built on it, the terms of the moments and the half-space
// value, as functions that also compile for the host, so that the arithmetic can be stepped through and compared with
// omg-planner_amd/planes.py without a GPU.  float64 with + - * /, sqrt and comparisons only, one rounded operation per operation
// of the specification, in its order.  No HIP built-ins here.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PLANE_HD __host__ __device__ __forceinline__
#else
#define PLANE_HD inline
#endif

#pragma clang fp contract(off)

#define PLANE_LANES 256  // lanes that share a chunk of pixels: the shape of the moments' sums
#define PLANE_SUMS 9     // q0, q1, q2, q0q0, q0q1, q0q2, q1q1, q1q2, q2q2

// Pixel (r, c) with depth d of a camera k = (fx, fy, cx, cy): p = (d*dx, d*dy, d); valid if d > 0, d < +inf (NaN fails both) and
// the pixel is not skipped.
PLANE_HD bool plane_point(const double* k, double d, bool skipped, int r, int c, double* p) {
    const double dx = ((double)c - k[2]) / k[0], dy = ((double)r - k[3]) / k[1];
    p[0] = d * dx, p[1] = d * dy, p[2] = d;
    return d > 0.0 && d < INFINITY && !skipped;
}

// The plane through pa, pb, pc -> live?  A void hypothesis is four zeros.  up: the prior's direction or a null pointer.
PLANE_HD bool plane_from_triple(const double* pa, const double* pb, const double* pc, bool all_valid, double min_nn, const double* up,
                                double cos_min, double* plane) {
    const double e0 = pb[0] - pa[0], e1 = pb[1] - pa[1], e2 = pb[2] - pa[2];
    const double f0 = pc[0] - pa[0], f1 = pc[1] - pa[1], f2 = pc[2] - pa[2];
    double n0 = e1 * f2 - e2 * f1, n1 = e2 * f0 - e0 * f2, n2 = e0 * f1 - e1 * f0;
    const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
    bool live = all_valid && nn > min_nn;
    const double s = sqrt(nn);
    n0 = n0 / s, n1 = n1 / s, n2 = n2 / s;
    double off = -((n0 * pa[0] + n1 * pa[1]) + n2 * pa[2]);
    if (off < 0.0) n0 = -n0, n1 = -n1, n2 = -n2, off = -off;
    if (up) live = live && (n0 * up[0] + n1 * up[1]) + n2 * up[2] >= cos_min;
    plane[0] = live ? n0 : 0.0, plane[1] = live ? n1 : 0.0, plane[2] = live ? n2 : 0.0, plane[3] = live ? off : 0.0;
    return live;
}

PLANE_HD double plane_residual(const double* plane, const double* p) {
    return ((plane[0] * p[0] + plane[1] * p[1]) + plane[2] * p[2]) + plane[3];
}

// Four zeros stand for "no plane": a row is a plane if its normal is not (0, 0, 0).
PLANE_HD bool plane_exists(const double* plane) { return plane[0] != 0.0 || plane[1] != 0.0 || plane[2] != 0.0; }

PLANE_HD bool plane_inlier(const double* plane, const double* p, bool valid, double tol) {
    return valid && fabs(plane_residual(plane, p)) <= tol;
}

// On the plane or behind it: the mask.
PLANE_HD bool plane_explains(const double* plane, const double* p, bool valid, double tol) {
    return valid && plane_exists(plane) && plane_residual(plane, p) <= tol;
}

// The nine terms of one inlier about the anchor.
PLANE_HD void plane_terms(const double* p, const double* anchor, double* t) {
    const double q0 = p[0] - anchor[0], q1 = p[1] - anchor[1], q2 = p[2] - anchor[2];
    t[0] = q0, t[1] = q1, t[2] = q2;
    t[3] = q0 * q0, t[4] = q0 * q1, t[5] = q0 * q2, t[6] = q1 * q1, t[7] = q1 * q2, t[8] = q2 * q2;
}

// The 256 lane partials x[l * stride] of one sum -> the chunk's total, the shape of registration._tree: inside each group of 64
// lanes x[l] += x[l + s] for s = 32 ... 1, then the four group totals left to right.  x is overwritten.
PLANE_HD double plane_tree(double* x, int stride) {
    for (int g = 0; g < PLANE_LANES; g += 64)
        for (int s = 32; s > 0; s >>= 1)
            for (int l = 0; l < s; ++l) x[(g + l) * stride] = x[(g + l) * stride] + x[(g + l + s) * stride];
    return ((x[0] + x[64 * stride]) + x[128 * stride]) + x[192 * stride];
}

// The half-space value of a node at p: positive on the camera's side of the plane, rounded to float32 once.
PLANE_HD float plane_halfspace(const double* plane, const double* p) { return (float)plane_residual(plane, p); }
