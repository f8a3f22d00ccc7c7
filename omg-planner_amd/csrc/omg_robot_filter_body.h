// omg_robot_filter_body.h — what the kernels of omg_robot_filter.hip do for one sphere, one pixel and one node: a sphere of the
// arm into a camera's frame, a pixel's ray against it, what one view says about a node, and the rule by which a run of nodes
// drops a sphere it cannot reach, as functions that also compile for the host, so that the arithmetic can be stepped through and
// compared with omg-planner_amd/robot_filter.py without a GPU.  float64 with + - * /, floor and sqrt only, one rounded
// operation per operation of the specification, in its order: dot products as (a*x + b*y) + c*z, rejections as negated
// comparisons (NaN falls on the "no" side).  No HIP built-ins here.
#pragma once
#include <cmath>
#include <cstdint>

#include "omg_volume_body.h"

#if defined(__HIPCC__)
#define ROBOT_HD __host__ __device__ __forceinline__
#else
#define ROBOT_HD inline
#endif

#pragma clang fp contract(off)

#define ROBOT_FREE 0
#define ROBOT_UNKNOWN 2

// Sphere (centre in its link's frame, radius) -> out[0..2]: the centre in the camera's frame, out[3]: r + pad.
// pose: the link's [4][4] row-major; wfc: the rows of world_from_cam [3][4] = (R, t).  w = P p + t_l, u = w - t, c = R^T u.
ROBOT_HD void robot_camera_sphere(const double* pose, const double* local, const double* wfc, double pad, double* out) {
    const double w0 = ((pose[0] * local[0] + pose[1] * local[1]) + pose[2] * local[2]) + pose[3];
    const double w1 = ((pose[4] * local[0] + pose[5] * local[1]) + pose[6] * local[2]) + pose[7];
    const double w2 = ((pose[8] * local[0] + pose[9] * local[1]) + pose[10] * local[2]) + pose[11];
    const double u0 = w0 - wfc[3], u1 = w1 - wfc[7], u2 = w2 - wfc[11];
    out[0] = (wfc[0] * u0 + wfc[4] * u1) + wfc[8] * u2;
    out[1] = (wfc[1] * u0 + wfc[5] * u1) + wfc[9] * u2;
    out[2] = (wfc[2] * u0 + wfc[6] * u1) + wfc[10] * u2;
    out[3] = local[3] + pad;
}

// q = |centre|^2 - R^2 of a sphere in the camera's frame: the same for every pixel.
ROBOT_HD double robot_sphere_q(const double* s) { return ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) - s[3] * s[3]; }

// camera.instance_active's test on q and the centre: can the ray (dx, dy, 1) meet the sphere beyond the camera?  Where it says
// no the ray misses (robot_sphere_entry returns false, for every t_min >= 0): with q > 0, b*b >= q*dd is disc >= 0 (a difference
// of two doubles is >= 0 exactly when the first is >= the second), and with b <= 0, s = sqrt(disc) <= |b| gives t1 <= 0.
ROBOT_HD bool robot_sphere_active(const double* s, double q, double dx, double dy, double dd) {
    const double cd = (s[0] * dx + s[1] * dy) + s[2];
    return q <= 0.0 || (cd > 0.0 && cd * cd >= q * dd);
}

// The ray (dx, dy, 1), dd = (dx*dx + dy*dy) + 1, against the sphere s with q = robot_sphere_q(s): false on a miss, otherwise
// *entry = t0 if t0 > t_min, else t_min.
ROBOT_HD bool robot_sphere_entry(const double* s, double q, double dx, double dy, double dd, double t_min, double* entry) {
    const double b = (s[0] * dx + s[1] * dy) + s[2];
    const double disc = b * b - q * dd;
    if (!(disc >= 0.0)) return false;
    const double root = sqrt(disc);
    const double t0 = (b - root) / dd, t1 = (b + root) / dd;
    if (!(t1 > t_min)) return false;
    *entry = t0 > t_min ? t0 : t_min;
    return true;
}

// t_near < inf and depth >= t_near - tol.
ROBOT_HD bool robot_explained(double depth, double t_near, double tol) { return t_near < __builtin_inf() && depth >= t_near - tol; }

// q = cam_from_grid p of the view (fx, fy, cx, cy, rows of cam_from_grid), and *front: the view sees p (z > near, the pixel
// inside the image), the pixel is explained and z < t_near there.  The row and the column are 0 unless the pixel lies inside the
// image, so that no point can form an address outside it (fusion_view_says's projection, operation for operation).
ROBOT_HD void robot_view_front(const double* view, const double* img, const double* t_img, int H, int W, const double* p, double near,
                               double tol, double* q, bool* front) {
    q[0] = ((view[4] * p[0] + view[5] * p[1]) + view[6] * p[2]) + view[7];
    q[1] = ((view[8] * p[0] + view[9] * p[1]) + view[10] * p[2]) + view[11];
    q[2] = ((view[12] * p[0] + view[13] * p[1]) + view[14] * p[2]) + view[15];
    const double z = q[2];
    const double cf = floor((view[0] * (q[0] / z) + view[2]) + 0.5), rf = floor((view[1] * (q[1] / z) + view[3]) + 0.5);
    const bool seen = z > near && cf >= 0.0 && cf <= (double)(W - 1) && rf >= 0.0 && rf <= (double)(H - 1);
    const int c = seen ? (int)cf : 0, r = seen ? (int)rf : 0;
    const int64_t at = (int64_t)r * W + c;
    const double tn = t_img[at];
    *front = seen && robot_explained(img[at], tn, tol) && z < tn;
}

// Is the camera-frame point q inside the sphere (x, y, z; rr = R*R)?
ROBOT_HD bool robot_inside(const double* q, double x, double y, double z, double rr) {
    const double e0 = q[0] - x, e1 = q[1] - y, e2 = q[2] - z;
    return (e0 * e0 + e1 * e1) + e2 * e2 <= rr;
}

ROBOT_HD uint8_t robot_new_state(uint8_t old, bool inside, bool front) {
    return inside || (old == ROBOT_UNKNOWN && front) ? (uint8_t)ROBOT_FREE : old;
}

// The nodes [id0, id1] (id1 >= id0, both inside the volume) of a volume lie in the index box lo..hi: one row of z, or whole rows
// of one slab of x, or whole slabs.
ROBOT_HD void robot_run_box(const int32_t* dims, uint32_t id0, uint32_t id1, int* lo, int* hi) {
    int a[3], b[3];
    volume_decode(dims, id0, &a[0], &a[1], &a[2]);
    volume_decode(dims, id1, &b[0], &b[1], &b[2]);
    lo[0] = a[0], hi[0] = b[0];
    if (a[0] != b[0]) lo[1] = 0, hi[1] = dims[1] - 1, lo[2] = 0, hi[2] = dims[2] - 1;
    else if (a[1] != b[1]) lo[1] = a[1], hi[1] = b[1], lo[2] = 0, hi[2] = dims[2] - 1;
    else lo[1] = hi[1] = a[1], lo[2] = a[2], hi[2] = b[2];
}

// A ball in the view's camera frame that holds the image of the index box lo..hi of the volume ms, and the size of the numbers
// that went into it: ball[0..2] the image of the box's centre, ball[3] a radius >= the distance of any node's image from it
// (sum over the axes of the half extent times the length of the matrix's column: right for any affine cam_from_grid),
// ball[4] = scale: over the three rows, the sum of |coefficient| times (|origin| + |offset of the centre| + half extent) and the
// |translation|: an upper bound of the absolute terms in the image of every node of the box.
ROBOT_HD void robot_run_ball(const omgx_mesh& ms, const int* lo, const int* hi, const double* view, double* ball) {
    double pc[3], h[3], ext[3];
    for (int a = 0; a < 3; ++a) {
        const double x = (0.5 * ((double)lo[a] + (double)hi[a]) + ms.sample_offset) * ms.delta;
        pc[a] = ms.origin[a] + x;
        h[a] = 0.5 * ((double)hi[a] - (double)lo[a]) * ms.delta;
        ext[a] = (fabs(ms.origin[a]) + fabs(x)) + h[a];
    }
    double rad = 0.0, scale = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double c0 = view[4 + a], c1 = view[8 + a], c2 = view[12 + a];
        rad += h[a] * sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    }
    for (int k = 0; k < 3; ++k) {
        const double* row = view + 4 + 4 * k;
        ball[k] = ((row[0] * pc[0] + row[1] * pc[1]) + row[2] * pc[2]) + row[3];
        scale += ((fabs(row[0]) * ext[0] + fabs(row[1]) * ext[1]) + fabs(row[2]) * ext[2]) + fabs(row[3]);
    }
    ball[3] = rad;
    ball[4] = scale;
}

// May the run whose ball is `ball` drop the sphere s = (x, y, z, R) of the same frame?  Only if the distance of the centres
// exceeds R + the ball's radius by more than 1e-9 of the scale of the numbers involved: the rounding of a node's image, of the
// ball and of robot_inside's sum is below 1e-14 of that scale, so no node of the run can be inside a dropped sphere.  Anything
// that is not finite keeps the sphere.
ROBOT_HD bool robot_run_drops(const double* ball, const double* s) {
    const double e0 = ball[0] - s[0], e1 = ball[1] - s[1], e2 = ball[2] - s[2];
    const double d = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    const double scale = ball[4] + (((fabs(s[0]) + fabs(s[1])) + fabs(s[2])) + s[3]);
    return d > (s[3] + ball[3]) + 1e-9 * scale;
}
