// omg_ik.hip — goal-set IK on the device: omgx_goal_ik (include/omg_hip.h, section 10).
//
// One lane per chain (grasp n, seed k): the reference's solve_one_pose_ik (omg/planner.py:17-86) in float64 registers, every
// solve a KDL ChainIkSolverPos_NR_JL::CartToJnt over ChainIkSolverVel_pinv (robot_pykdl.py:118-146), restated:
//   for i < max_iter:  f = FK(q);  d = diff(f, target);  stop if every |d_j| <= eps;  q += J^+ d;  clamp q to [lo, hi].
// FK: panda_link0 -> panda_hand = robot_pykdl output_pose[:, 7] before center_offset, from the blob's derived chain constants
// (UVW, TP, H) with the angle in radians (no degree round trip: that belongs to the CHOMP path's kinematics only).
// J: 6x7, base frame, reference point at the hand origin; joint i turns about the z axis of cur_{i-1} . pose_0[i] through that
// frame's origin (the true derivative, not the CHOMP point Jacobian's joint origins).
// J^+ d: one-sided (Hestenes) Jacobi on the six rows of J — Givens rotations V of the rows until they are orthogonal, applied to
// d as well: J = V W^T with W's columns w_a orthogonal, so J^+ d = sum_a w_a (V^T d)_a / |w_a|^2 over |w_a| = sigma_a >= pinv_eps,
// the truncated SVD pseudo-inverse of KDL (which drops the same singular values).  Only W [6][7] and V^T d [6] are kept.
// The file is compiled with -ffp-contract=off: no fused multiply-adds, as in the numpy restatement (tests/ik_restatement.py).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "omg_device.h"
#include "omg_host.h"

namespace {
using namespace omg;

constexpr double KDL_EPSILON = 1e-6;  // KDL::epsilon, Rotation::GetRotAngle's margins
constexpr int IK_MAX_SWEEPS = 32;     // Jacobi sweeps (a 6-row problem converges in 5-8)

typedef const OMG_CONST_AS double* CD;

// sin / cos / atan2 from fdlibm's kernels (range reduction by a three-part pi/2, the minimax polynomials of k_sin.c / k_cos.c /
// s_atan.c), written with + - * / and rint only: under -ffp-contract=off every operation is an IEEE double operation, so the numpy
// restatement (tests/ik_restatement.py: ik_sincos, ik_atan2) reproduces them bit for bit where the vendor libraries' last bits
// differ — a Newton step near a singular configuration amplifies a one-ulp difference by 1e5 and more.  Accuracy ~1 ulp on the
// angles a solve sees (|q| well below 2^20).
__device__ __forceinline__ void ik_sincos(double x, double* sn, double* cs) {
    const double n = rint(x * 6.36619772367581382433e-01);
    const double r = ((x - n * 1.57079632673412561417e+00) - n * 6.07710050630396597660e-11) - n * 2.02226624871116645580e-21;
    const double z = r * r;
    const double ps = r + r * z * (-1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
    const double hz = 0.5 * z, w = 1.0 - hz;
    const double rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const double pc = w + (((1.0 - w) - hz) + z * rc);
    const int qd = ((int)(long long)n) & 3;
    *sn = qd == 0 ? ps : qd == 1 ? pc : qd == 2 ? -ps : -pc;
    *cs = qd == 0 ? pc : qd == 1 ? -ps : qd == 2 ? -pc : ps;
}

__device__ __forceinline__ double ik_atan_nonneg(double x) {  // fdlibm atan for x >= 0
    const double hi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
    const double lo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
    int id;
    if (x < 0.4375) {
        id = -1;
    } else if (x < 1.1875) {
        if (x < 0.6875) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); } else { id = 1; x = (x - 1.0) / (x + 1.0); }
    } else {
        if (x < 2.4375) { id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); } else { id = 3; x = -1.0 / x; }
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                      w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                      w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (id < 0) return x - x * (s1 + s2);
    double h = 0.0, l = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k == id) { h = hi[k]; l = lo[k]; }
    return h - ((x * (s1 + s2) - l) - x);
}

// atan2(y, x) for y >= 0 (GetRotAngle's |axis| / 2, cos angle)
__device__ __forceinline__ double ik_atan2_ynonneg(double y, double x) {
    if (x == 0.0) return y == 0.0 ? 0.0 : 1.57079632679489655800e+00;
    if (y == 0.0) return x > 0.0 ? 0.0 : 3.14159265358979311600e+00;
    const double a = ik_atan_nonneg(y / fabs(x));
    return x > 0.0 ? a : 3.14159265358979311600e+00 - (a - 1.22464679914735320717e-16);
}

struct IkTarget { double R[9]; double t[3]; };

// hand frame (R, t) of q and the Jacobian's rows W[6][7]
__device__ __forceinline__ void ik_fk_jacobian(const RobotViewS& rv, CD pose0, const double* q, double* R, double* t,
                                               double W[6][7]) {
    double cR[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double ct[3] = {0.0, 0.0, 0.0};
    double z[7][3], p[7][3];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        CD P0 = pose0 + 16 * i;  // pose_0[i], row-major 4x4: column 2 = (P0[2], P0[6], P0[10])
#pragma unroll
        for (int r = 0; r < 3; ++r) z[i][r] = cR[3 * r] * P0[2] + cR[3 * r + 1] * P0[6] + cR[3 * r + 2] * P0[10];
        double s, c;
        ik_sincos(q[i], &s, &c);
        const auto uvw = rv.uvw(i);
        const auto tp = rv.tp(i);
        double B[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) B[k] = c * uvw[k] + s * uvw[9 + k] + uvw[18 + k];
        double nR[9], nt[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) nR[3 * r + cc] = cR[3 * r] * B[cc] + cR[3 * r + 1] * B[3 + cc] + cR[3 * r + 2] * B[6 + cc];
            nt[r] = cR[3 * r] * tp[0] + cR[3 * r + 1] * tp[1] + cR[3 * r + 2] * tp[2] + ct[r];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) cR[k] = nR[k];
#pragma unroll
        for (int r = 0; r < 3; ++r) p[i][r] = ct[r] = nt[r];  // the joint frame's origin: Rz, Rx leave the translation alone
    }
    const auto H = rv.hand();  // rows of pose_0[7]
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) R[3 * r + cc] = cR[3 * r] * H[cc] + cR[3 * r + 1] * H[4 + cc] + cR[3 * r + 2] * H[8 + cc];
        t[r] = cR[3 * r] * H[3] + cR[3 * r + 1] * H[7] + cR[3 * r + 2] * H[11] + ct[r];
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double ex = t[0] - p[i][0], ey = t[1] - p[i][1], ez = t[2] - p[i][2];
        W[0][i] = z[i][1] * ez - z[i][2] * ey;
        W[1][i] = z[i][2] * ex - z[i][0] * ez;
        W[2][i] = z[i][0] * ey - z[i][1] * ex;
        W[3][i] = z[i][0];
        W[4][i] = z[i][1];
        W[5][i] = z[i][2];
    }
}

// KDL Rotation::GetRot = axis * angle of Rotation::GetRotAngle(axis, KDL::epsilon), with its branches at angle 0 and pi.
__device__ __forceinline__ void kdl_rotvec(const double* d, double* out) {
    const double e = KDL_EPSILON, e2 = 10.0 * KDL_EPSILON;
    if (fabs(d[1] - d[3]) < e && fabs(d[2] - d[6]) < e && fabs(d[5] - d[7]) < e) {
        if (fabs(d[1] + d[3]) < e2 && fabs(d[2] + d[6]) < e2 && fabs(d[5] + d[7]) < e2 && fabs(d[0] + d[4] + d[8] - 3) < e2) {
            out[0] = out[1] = out[2] = 0.0;  // identity: angle 0
            return;
        }
        const double xx = (d[0] + 1) / 2, yy = (d[4] + 1) / 2, zz = (d[8] + 1) / 2;
        const double xy = (d[1] + d[3]) / 4, xz = (d[2] + d[6]) / 4, yz = (d[5] + d[7]) / 4;
        double x, y, z;
        if (xx > yy && xx > zz) {
            x = sqrt(xx); y = xy / x; z = xz / x;
        } else if (yy > zz) {
            y = sqrt(yy); x = xy / y; z = yz / y;
        } else {
            z = sqrt(zz); x = xz / z; y = yz / z;
        }
        out[0] = x * M_PI; out[1] = y * M_PI; out[2] = z * M_PI;
        return;
    }
    const double f = (d[0] + d[4] + d[8] - 1) / 2;
    double x = d[7] - d[5], y = d[2] - d[6], z = d[3] - d[1];
    const double n = sqrt(x * x + y * y + z * z);
    const double ang = ik_atan2_ynonneg(n / 2, f);
    if (n < e) {  // Vector::Normalize below its eps: (1, 0, 0)
        x = 1.0; y = 0.0; z = 0.0;
    } else {
        x /= n; y /= n; z /= n;
    }
    out[0] = x * ang; out[1] = y * ang; out[2] = z * ang;
}

// one NR_JL solve; q in/out; returns the number of updates made (max_iter: failed)
__device__ int ik_solve(const RobotViewS& rv, CD pose0, CD lo, CD hi, const IkTarget& T, double* q, int max_iter, double eps,
                        double pinv_eps) {
    for (int it = 0; it < max_iter; ++it) {
        double R[9], t[3], W[6][7];
        ik_fk_jacobian(rv, pose0, q, R, t, W);
        // d = diff(f, target): (target.p - f.p, f.M . rotvec(f.M^T . target.M))
        double d[6];
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = T.t[r] - t[r];
        double rel[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) rel[3 * r + c] = R[r] * T.R[c] + R[3 + r] * T.R[3 + c] + R[6 + r] * T.R[6 + c];
        }
        double w[3];
        kdl_rotvec(rel, w);
#pragma unroll
        for (int r = 0; r < 3; ++r) d[3 + r] = R[3 * r] * w[0] + R[3 * r + 1] * w[1] + R[3 * r + 2] * w[2];
        bool conv = true;
#pragma unroll
        for (int j = 0; j < 6; ++j) conv = conv && fabs(d[j]) <= eps;
        if (conv) return it;
        // Hestenes: orthogonalise the rows of J, rotating d alongside
        for (int sweep = 0; sweep < IK_MAX_SWEEPS; ++sweep) {
            bool rotated = false;
#pragma unroll
            for (int a = 0; a < 5; ++a) {
#pragma unroll
                for (int b = a + 1; b < 6; ++b) {
                    double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                    for (int j = 0; j < 7; ++j) {
                        al += W[a][j] * W[a][j];
                        be += W[b][j] * W[b][j];
                        ga += W[a][j] * W[b][j];
                    }
                    if (fabs(ga) > 1e-15 * sqrt(al * be) && ga != 0.0) {
                        const double zeta = (be - al) / (2.0 * ga);
                        const double az = fabs(zeta);
                        const double tn = (az > 1e100 ? 0.5 / az : 1.0 / (az + sqrt(1.0 + zeta * zeta))) * (zeta < 0.0 ? -1.0 : 1.0);
                        const double c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
#pragma unroll
                        for (int j = 0; j < 7; ++j) {
                            const double wa = W[a][j], wb = W[b][j];
                            W[a][j] = c * wa - s * wb;
                            W[b][j] = s * wa + c * wb;
                        }
                        const double da = d[a], db = d[b];
                        d[a] = c * da - s * db;
                        d[b] = s * da + c * db;
                        rotated = true;
                    }
                }
            }
            if (!rotated) break;
        }
        double dq[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double s2 = 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) s2 += W[a][j] * W[a][j];
            if (sqrt(s2) >= pinv_eps) {  // KDL: |S(i)| < eps -> 0 (truncated SVD)
                const double f = d[a] / s2;
#pragma unroll
                for (int j = 0; j < 7; ++j) dq[j] += W[a][j] * f;
            }
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            double v = q[j] + dq[j];
            v = v < lo[j] ? lo[j] : v;
            q[j] = v > hi[j] ? hi[j] : v;
        }
    }
    return max_iter;
}

__device__ __forceinline__ IkTarget load_target(const double* __restrict__ p) {
    IkTarget T;
#pragma unroll
    for (int k = 0; k < 9; ++k) T.R[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) T.t[k] = p[9 + k];
    return T;
}

__global__ void __launch_bounds__(64) k_goal_ik(const double* __restrict__ robot, int P, const double* __restrict__ targets,
                                                const int32_t* __restrict__ grasp_begin, int S, int N, const double* __restrict__ seeds,
                                                int K, int T, int use_standoff, int max_iter, double eps, double pinv_eps,
                                                double accept_diff, int32_t* __restrict__ status, double* __restrict__ solutions,
                                                int32_t* __restrict__ iterations) {
    const int64_t chain = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (chain >= (int64_t)N * K) return;
    const int n = (int)(chain / K), k = (int)(chain % K);
    int lo_s = 0, hi_s = S - 1;  // scene s: grasp_begin[s] <= n < grasp_begin[s + 1] (the last scene on bad input: in range)
    while (lo_s < hi_s) {
        const int mid = (lo_s + hi_s + 1) >> 1;
        if (grasp_begin[mid] <= n) lo_s = mid; else hi_s = mid - 1;
    }
    const RobotViewS rv(robot, P);
    CD raw = (CD)(uintptr_t)robot;
    CD pose0 = raw + OMGX_ROBOT_POSE0, lo = raw + OMGX_ROBOT_LOWER, hi = raw + OMGX_ROBOT_UPPER;
    double q[7];
    const double* sd = seeds + ((int64_t)lo_s * K + k) * 7;
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = sd[j];
    const double* tg = targets + (int64_t)n * T * 12;
    double* sol = solutions + chain * T * 7;
    const int ni = use_standoff ? 1 + T : 1;
    int32_t* its = iterations ? iterations + chain * ni : nullptr;
    for (int s = 0; s < T * 7; ++s) sol[s] = 0.0;
    if (its)
        for (int s = 0; s < ni; ++s) its[s] = -1;
    int32_t st = 0;
    int it = ik_solve(rv, pose0, lo, hi, load_target(tg + (use_standoff ? (T - 1) * 12 : 0)), q, max_iter, eps, pinv_eps);
    if (its) its[0] = it;
    if (!use_standoff) {
#pragma unroll
        for (int j = 0; j < 7; ++j) sol[j] = q[j];
        st = it < max_iter ? 0 : 1;
    } else if (it >= max_iter) {
        st = 1;
    } else {
        double frob = 0.0;  // np.linalg.norm(np.diff(reach_traj, axis=0)) squared (the order of the rows does not matter)
        double prev[7];
        for (int t = 0; t < T; ++t) {
#pragma unroll
            for (int j = 0; j < 7; ++j) prev[j] = q[j];
            it = ik_solve(rv, pose0, lo, hi, load_target(tg + t * 12), q, max_iter, eps, pinv_eps);
            if (its) its[1 + t] = it;
#pragma unroll
            for (int j = 0; j < 7; ++j) sol[t * 7 + j] = q[j];
            if (it >= max_iter) {
                st = 2 + t;
                break;
            }
            if (t > 0) {
#pragma unroll
                for (int j = 0; j < 7; ++j) frob += (q[j] - prev[j]) * (q[j] - prev[j]);
            }
        }
        if (st == 0 && !(sqrt(frob) < accept_diff)) st = -1;
    }
    status[chain] = st;
}

}  // namespace

extern "C" int omgx_goal_ik(const double* robot, int32_t n_points, const double* targets, const int32_t* grasp_begin,
                            const int32_t* h_grasp_begin, int32_t num_scenes, int32_t num_grasps, const double* seeds,
                            int32_t num_seeds, int32_t T, int32_t use_standoff, int32_t attached, int32_t max_iter, double eps,
                            double pinv_eps, double accept_diff, int32_t* status, double* solutions, int32_t* iterations,
                            void* stream) {
    if (num_scenes < 0 || num_grasps < 0) return OMGX_ERR_INVALID;
    if (T < 1 || T > OMGX_IK_MAX_TAIL || (!use_standoff && T != 1)) return OMGX_ERR_INVALID;
    if (num_seeds < 1 || num_seeds > OMGX_IK_MAX_SEEDS) return OMGX_ERR_INVALID;
    if ((use_standoff != 0 && use_standoff != 1) || (attached != 0 && attached != 1)) return OMGX_ERR_INVALID;
    if (max_iter < 1 || max_iter > 100000 || !(eps >= 0.0) || !(pinv_eps >= 0.0) || !(accept_diff >= 0.0)) return OMGX_ERR_INVALID;
    if (!h_grasp_begin) return OMGX_ERR_INVALID;
    if (h_grasp_begin[0] != 0 || h_grasp_begin[num_scenes] != num_grasps) return OMGX_ERR_INVALID;
    for (int s = 0; s < num_scenes; ++s)
        if (h_grasp_begin[s + 1] < h_grasp_begin[s]) return OMGX_ERR_INVALID;
    if (num_grasps == 0) return OMGX_OK;
    if (!robot || !targets || !grasp_begin || !seeds || !status || !solutions) return OMGX_ERR_INVALID;
    if (n_points < 1 || n_points > OMGX_MAX_POINTS) return OMGX_ERR_UNSUPPORTED;
    if ((int64_t)num_grasps * num_seeds > ((int64_t)1 << 31) - 64) return OMGX_ERR_UNSUPPORTED;
    const int64_t chains = (int64_t)num_grasps * num_seeds;
    hipLaunchKernelGGL(k_goal_ik, dim3((unsigned)((chains + 63) / 64)), dim3(64), 0, (hipStream_t)stream, robot, n_points, targets,
                       grasp_begin, num_scenes, num_grasps, seeds, num_seeds, T, use_standoff, max_iter, eps, pinv_eps, accept_diff,
                       status, solutions, iterations);
    OMGX_CHECK_LAUNCH("k_goal_ik");
    return OMGX_OK;
}
