// omg_clearance_body.h — what the kernels of omg_clearance.hip do for one sphere, one (sphere, record) pair and one pair of
// spheres, and the rule by which two results are merged, as functions that also compile for the host, so that the arithmetic can
// be stepped through and compared with omg-planner_amd/clearance.py without a GPU.  float64 with + - * / and sqrt only, one
// rounded operation per operation of the specification, in its order: dot products as (a*x + b*y) + c*z, rejections as negated
// comparisons (NaN falls on the "no" side).  The volume is read by omg_volume_camera_body.h's vcam_sample and nothing else.
// No HIP built-ins here.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/omg_hip.h"
#include "omg_volume_camera_body.h"

#pragma clang fp contract(off)

struct clear_best {  // a result of the replace rule: the value and who gave it ((-1, -1): nobody)
    double v;
    int32_t a, b;
};

GRASP_HD clear_best clear_none() { return clear_best{__builtin_inf(), -1, -1}; }

// Does the candidate (v, a, b) replace `best`?  It is < the best, or == the best with a smaller (a, b).  NaN never does, and
// +inf never does either: nobody's (a, b) is below (-1, -1).
GRASP_HD bool clear_replaces(double v, int32_t a, int32_t b, const clear_best& best) {
    return v < best.v || (v == best.v && (a < best.a || (a == best.a && b < best.b)));
}

GRASP_HD void clear_take(clear_best& best, double v, int32_t a, int32_t b) {
    if (clear_replaces(v, a, b, best)) best.v = v, best.a = a, best.b = b;
}

// Sphere centre p (in its link's frame) -> w: the centre in the world.  pose: the link's [4][4] row-major.
GRASP_HD void clear_world(const double* pose, const double* p, double* w) {
    w[0] = ((pose[0] * p[0] + pose[1] * p[1]) + pose[2] * p[2]) + pose[3];
    w[1] = ((pose[4] * p[0] + pose[5] * p[1]) + pose[6] * p[2]) + pose[7];
    w[2] = ((pose[8] * p[0] + pose[9] * p[1]) + pose[10] * p[2]) + pose[11];
}

// Is the record one the op reads?  visible (or NULL: the record's own `disabled`), and a grid a kernel can read.
GRASP_HD bool clear_record_used(const omgx_object& ob, const uint8_t* visible, int64_t index, int64_t pool_elems) {
    if (visible ? visible[index] == 0 : ob.disabled != 0) return false;
    return ob.inv_delta > 0.0 && ob.inv_delta < __builtin_inf() && vcam_grid_usable(ob.dim, ob.grid_offset, pool_elems);
}

// The world point w against the record whose grid is G -> R.uo = u (grid coordinates, not clamped; R.ud = 0) and e: the distance
// from w to the box of the grid's samples.  vcam_sample<false>(G, pool, R, 0.0, nullptr) is then v at the nearest point of it.
GRASP_HD double clear_reach(const vcam_grid& G, const float* pose_inv, const double* w, vcam_ray& R) {
    double x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double q = (((double)pose_inv[4 * a] * w[0] + (double)pose_inv[4 * a + 1] * w[1]) + (double)pose_inv[4 * a + 2] * w[2]) +
                         (double)pose_inv[4 * a + 3];
        const double u = (q - G.lo[a]) * G.inv_delta - 0.5;
        double c = u >= 0.0 ? u : 0.0;  // vcam_cell's clamp
        c = c > G.hi[a] ? G.hi[a] : c;
        R.uo[a] = u, R.ud[a] = 0.0;
        x[a] = u - c;
    }
    R.nrm = 0.0;
    return sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) / G.inv_delta;
}

// One pair of spheres (centre, radius + pad): dist - (rp_i + rp_j).
GRASP_HD double clear_gap(const double* si, const double* sj) {
    const double d0 = si[0] - sj[0], d1 = si[1] - sj[1], d2 = si[2] - sj[2];
    return sqrt((d0 * d0 + d1 * d1) + d2 * d2) - (si[3] + sj[3]);
}
