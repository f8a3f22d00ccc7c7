// omg_track_body.h — what k_track_pass (omg_track.hip) does for one used pixel and what k_track_step does between two passes, as
// functions that also compile for the host, so that the arithmetic can be stepped through and compared with
// tracking.track_cameras (omg-planner_amd/tracking.py) without a GPU.  float64, one rounded operation per operation of the
// specification, in its order.  The 6 x 6 solve, the pose update, the constants and the partials are omg_register_body.h's, called:
// track_turn is everything reg_iterate does between one pass(...) and the next, with the loop's variables in a record that
// lives in device memory between the launches.  How a chunk's lanes and a view's chunk rows are summed is left to the caller:
// shuffles, LDS and a wave in the kernels, plain loops in a host harness.
#pragma once
#include <cmath>
#include <cstdint>

#include "omg_register_body.h"

#pragma clang fp contract(off)

#define TRACK_LANES 256
#define TRACK_ROW 32  // doubles of one (view, chunk) row of the workspace: 28 sums, the count, padding

// The loop's variables of one view (reg_iterate's locals), 512 bytes.
struct track_state {
    double pose[12], trial[12];
    reg_sums cur;  // the sums at `pose` (x [28], count)
    double xi[6], cost0, lam;
    int32_t count0, status, accepted, trials, first, done;
};
static_assert(sizeof(track_state) == 512, "one view's row of the workspace");

struct track_image {  // what a pass reads of one view
    const double* zl;  // [H][W]
    const double* nl;  // [H][W][3] or null
    const double* zm;  // [H][W]
    const double* nm;  // [H][W][3]
    double fx, fy, cx, cy;
    int32_t H, W;
};

// tracking.pixel_terms and one_pass's contribution for the used pixel (r, c) at the pose P = rows of [R t], added to a lane's partials.
GRASP_HD void track_pixel(const track_image& I, const double* P, int r, int c, double dist2, double cos_min, reg_sums& acc) {
    const int64_t at = (int64_t)r * I.W + c;
    const double z = I.zl[at];
    bool valid = (z > 0.0) && (z < (double)INFINITY);
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    if (I.nl) {
        m0 = I.nl[at * 3], m1 = I.nl[at * 3 + 1], m2 = I.nl[at * 3 + 2];
        valid = valid && ((m0 * m0 + m1 * m1) + m2 * m2 > 0.0);
    }
    if (!valid) return;
    const double dx = ((double)c - I.cx) / I.fx, dy = ((double)r - I.cy) / I.fy;
    const double P0 = dx * z, P1 = dy * z, P2 = z;
    const double Q0 = ((P[0] * P0 + P[1] * P1) + P[2] * P2) + P[3];
    const double Q1 = ((P[4] * P0 + P[5] * P1) + P[6] * P2) + P[7];
    const double Q2 = ((P[8] * P0 + P[9] * P1) + P[10] * P2) + P[11];
    bool inlier = false;
    if (Q2 > 0.0) {
        const double ua = (I.fx * (Q0 / Q2) + I.cx) + 0.5, ub = (I.fy * (Q1 / Q2) + I.cy) + 0.5;
        // in double, before any conversion: NaN, +-inf and 1e300 fail a comparison and are outside
        if ((ua >= 0.0) && (ua < (double)I.W) && (ub >= 0.0) && (ub < (double)I.H)) {
            const int cm = (int)ua, rm = (int)ub;
            const int64_t am = (int64_t)rm * I.W + cm;
            const double zq = I.zm[am];
            const double n0 = I.nm[am * 3], n1 = I.nm[am * 3 + 1], n2 = I.nm[am * 3 + 2];
            if ((zq > 0.0) && (zq < (double)INFINITY) && ((n0 * n0 + n1 * n1) + n2 * n2 > 0.0)) {
                const double dxm = ((double)cm - I.cx) / I.fx, dym = ((double)rm - I.cy) / I.fy;
                const double e0 = Q0 - dxm * zq, e1 = Q1 - dym * zq, e2 = Q2 - zq;
                const double dd = (e0 * e0 + e1 * e1) + e2 * e2;
                bool ok = dd <= dist2;
                if (I.nl) {
                    const double r0 = (P[0] * m0 + P[1] * m1) + P[2] * m2;
                    const double r1 = (P[4] * m0 + P[5] * m1) + P[6] * m2;
                    const double r2 = (P[8] * m0 + P[9] * m1) + P[10] * m2;
                    ok = ok && ((r0 * n0 + r1 * n1) + r2 * n2 >= cos_min);
                }
                if (ok) {
                    inlier = true;
                    const double res = (n0 * e0 + n1 * e1) + n2 * e2;
                    const double g0 = (P[0] * n0 + P[4] * n1) + P[8] * n2;
                    const double g1 = (P[1] * n0 + P[5] * n1) + P[9] * n2;
                    const double g2 = (P[2] * n0 + P[6] * n1) + P[10] * n2;
                    double j[6];
                    j[0] = g0, j[1] = g1, j[2] = g2;
                    j[3] = P1 * g2 - P2 * g1, j[4] = P2 * g0 - P0 * g2, j[5] = P0 * g1 - P1 * g0;
                    int k = 0;
#pragma unroll
                    for (int a = 0; a < 6; ++a) {
#pragma unroll
                        for (int b = a; b < 6; ++b) acc.x[k] = acc.x[k] + j[a] * j[b], ++k;
                    }
#pragma unroll
                    for (int a = 0; a < 6; ++a) acc.x[21 + a] = acc.x[21 + a] + j[a] * res;
                    acc.x[27] = acc.x[27] + res * res;
                    acc.count += 1;
                }
            }
        }
    }
    if (!inlier) acc.x[27] = acc.x[27] + dist2;
}

// The used pixel u (row-major over the used grid of Wu columns) -> its pixel.
GRASP_HD void track_used_pixel(int64_t u, int Wu, int stride, int* r, int* c) {
    const uint32_t ru = (uint32_t)u / (uint32_t)Wu, cu = (uint32_t)u % (uint32_t)Wu;  // (u < H * W <= 2^31 - 1: 32-bit division)
    *r = (int)ru * stride, *c = (int)cu * stride;
}

// What k_track_init writes: reg_iterate's state before its first pass.
GRASP_HD void track_begin(track_state& s, const double* pose0, double lambda0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) s.pose[i] = pose0[i], s.trial[i] = pose0[i];
    reg_clear(s.cur);
#pragma unroll
    for (int i = 0; i < 6; ++i) s.xi[i] = 0.0;
    s.count0 = 0, s.cost0 = 0.0, s.lam = lambda0;
    s.status = 0, s.accepted = 0, s.trials = 0, s.first = 1, s.done = 0;
}

// reg_iterate between one pass(...) and the next: `tri` holds the sums at s.trial.  -> true when the view stops; otherwise
// s.trial is the next pose to evaluate.  The order of the tests and every operation are reg_iterate's.
GRASP_HD bool track_turn(track_state& s, const reg_sums& tri, double step_tol, int max_passes) {
    bool stop = false;
    if (s.first || tri.x[27] < s.cur.x[27]) {
#pragma unroll
        for (int i = 0; i < 12; ++i) s.pose[i] = s.trial[i];
#pragma unroll
        for (int i = 0; i < REG_NPART; ++i) s.cur.x[i] = tri.x[i];
        s.cur.count = tri.count;
        if (s.first) {
            s.cost0 = s.cur.x[27], s.count0 = s.cur.count;
        } else {
            ++s.accepted;
            s.lam = s.lam / 8.0 > REG_LAMBDA_MIN ? s.lam / 8.0 : REG_LAMBDA_MIN;
            bool small = true;
#pragma unroll
            for (int i = 0; i < 6; ++i) small = small && ((s.xi[i] < 0.0 ? -s.xi[i] : s.xi[i]) < step_tol);
            if (small) s.status |= REG_CONVERGED, stop = true;
        }
    } else {
        s.lam = 8.0 * s.lam < REG_LAMBDA_MAX ? 8.0 * s.lam : REG_LAMBDA_MAX;
    }
    s.first = 0;
    // the next trial: the first one whose solve succeeds
    bool have = false;
    while (!stop && !have) {
        if (s.cur.count < REG_MIN_INLIERS) {
            s.status |= REG_FEW_INLIERS, stop = true;
        } else if (s.lam >= REG_LAMBDA_MAX) {
            s.status |= REG_LAMBDA_AT_MAX, stop = true;
        } else if (s.trials >= max_passes) {
            stop = true;
        } else {
            ++s.trials;
            have = reg_solve6(s.cur, s.lam, s.xi);
            if (!have) {
                s.status |= REG_SINGULAR;
                s.lam = 8.0 * s.lam < REG_LAMBDA_MAX ? 8.0 * s.lam : REG_LAMBDA_MAX;
            }
        }
    }
    if (!stop) reg_step_pose(s.pose, s.xi, s.trial);
    s.done = stop ? 1 : 0;
    return stop;
}

// The stats row of a view that has stopped: reg_iterate's.
GRASP_HD void track_stats(const track_state& s, double* stats) {
    stats[0] = s.cost0, stats[1] = s.cur.x[27], stats[2] = (double)s.count0, stats[3] = (double)s.cur.count;
    stats[4] = (double)s.accepted, stats[5] = (double)s.trials, stats[6] = s.lam, stats[7] = (double)s.status;
}
