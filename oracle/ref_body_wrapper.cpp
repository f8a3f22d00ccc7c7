// ref_body_wrapper.cpp — the REFERENCE's own SDF kernel body, compiled for the host and run serially.
//
// TEST INFRASTRUCTURE ONLY.  The file REF_BODY_INC is produced at build time by oracle/Makefile (`make ref`) as lines
// 11-13 (the grid-stride loop macro), 15-86 (the interpolation helpers) and 96-195 (SDFdistanceForward and
// sum_gradients) of the reference's layers/sdf_matching_loss_kernel.cu, cut out of the file where it lies into a
// temporary that is deleted after the compile.  Nothing of it is stored in the repository; only the resulting
// oracle/_ref/libsdf_ref_body.so exists (git-ignored).  This file holds only our own code:
//   - the CUDA qualifiers defined empty, float3 / int3, and threadIdx = blockIdx = 0, blockDim = gridDim = 1, so that the
//     grid-stride loop visits every index once, in order; atomicAdd as a plain add, so that sum_gradients adds the objects of
//     a point in index order (like orc_sdf_loss_forward);
//   - stand-ins for the few Eigen / Sophus types the body names: a fixed-size Matrix with the comma initialiser,
//     operator(), transpose() and the 3x3 by 3x1 product; SO3::matrix(); SE3(Matrix4), so3() and SE3 * Vec3;
//   - ref_sdf_loss_forward, which restates the launcher's data flow (.cu:204-262): zeroed per-pair and per-point outputs
//     (at::zeros — the body `continue`s without writing), one run of the body, three sum_gradients runs.
//
// The stand-ins have two arithmetic modes, chosen per call:
//   mode 0 (matrix):     SE3 * p = R p + t and R^T v as the fma chains of orc_sdf_pair's default path and of the HIP kernels;
//   mode 1 (quaternion): Eigen's matrix -> quaternion assignment, QuaternionBase::_transformVector and toRotationMatrix in
//                        float32, and Eigen's plain sum of products for R^T v: the oracle's SOPHUS MODE.
//
// WHAT THIS PINS: the body's text — every index, cast, literal promotion, comparison, branch, `continue` and operand order
// of .cu:96-195 — because that text itself is what runs.
// WHAT IT CANNOT PIN: Eigen's and Sophus' own arithmetic (the two modes are our restatement of the published algorithms);
// whatever nvcc would contract inside them; and the order of the atomic reduction over objects (serial here).
//
// Floating point: compile with -ffp-contract=off (the stand-ins' arithmetic must not fuse: only the explicit fma()s do);
// contraction is switched to `fast` by pragma around the included text only, which is what nvcc does to `a + t*(b-a)`.
// The fourth row of the pose is read by the comma initialiser and never used, like the matrix path of the kernels.
#include <cmath>
#include <cstring>

#define __global__
#define __device__
#define __host__
struct float3 { float x, y, z; };
struct int3 { int x, y, z; };
static inline float3 make_float3(float x, float y, float z) { return {x, y, z}; }
static inline int3 make_int3(int x, int y, int z) { return {x, y, z}; }
struct serial_dim { int x; };
static const serial_dim threadIdx = {0}, blockIdx = {0}, blockDim = {1}, gridDim = {1};
template <typename T> static inline void atomicAdd(T* p, T v) { *p += v; }

static thread_local int t_mode = 0;  // set by ref_sdf_loss_forward for the duration of one call

namespace Eigen {
enum { DontAlign = 2 };
template <typename T, int R, int C, int Opt = 0> struct Matrix {
    T m[R * C];  // row-major
    struct Comma {
        Matrix& M; int k;
        Comma& operator,(T v) { M.m[k++] = v; return *this; }
    };
    Comma operator<<(T v) { m[0] = v; return Comma{*this, 1}; }
    T& operator()(int i) { return m[i]; }
    const T& operator()(int i) const { return m[i]; }
    T& operator()(int r, int c) { return m[r * C + c]; }
    const T& operator()(int r, int c) const { return m[r * C + c]; }
    Matrix<T, C, R, Opt> transpose() const {
        Matrix<T, C, R, Opt> t;
        for (int r = 0; r < R; ++r) for (int c = 0; c < C; ++c) t.m[c * R + r] = m[r * C + c];
        return t;
    }
};
template <typename T, int O1, int O2> Matrix<T, 3, 1, O2> operator*(const Matrix<T, 3, 3, O1>& A, const Matrix<T, 3, 1, O2>& v) {
    Matrix<T, 3, 1, O2> o;
    for (int r = 0; r < 3; ++r) {
        if (t_mode == 0) o.m[r] = std::fma(A(r, 2), v(2), std::fma(A(r, 1), v(1), A(r, 0) * v(0)));
        else o.m[r] = (A(r, 0) * v(0) + A(r, 1) * v(1)) + A(r, 2) * v(2);
    }
    return o;
}
}  // namespace Eigen

namespace Sophus {
template <typename T> struct SO3 {
    T R[9];  // the matrix as given (mode 0)
    T q[4];  // x y z w (mode 1)
    int branch;  // which branch of the matrix -> quaternion assignment was taken: 3 = trace > 0, else the pivot i
    Eigen::Matrix<T, 3, 3, Eigen::DontAlign> matrix() const {
        Eigen::Matrix<T, 3, 3, Eigen::DontAlign> M;
        if (t_mode == 0) { for (int i = 0; i < 9; ++i) M.m[i] = R[i]; return M; }
        const T x = q[0], y = q[1], z = q[2], w = q[3];  // QuaternionBase::toRotationMatrix
        const T tx = 2 * x, ty = 2 * y, tz = 2 * z;
        const T twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
        M.m[0] = 1 - (tyy + tzz); M.m[1] = txy - twz; M.m[2] = txz + twy;
        M.m[3] = txy + twz; M.m[4] = 1 - (txx + tzz); M.m[5] = tyz - twx;
        M.m[6] = txz - twy; M.m[7] = tyz + twx; M.m[8] = 1 - (txx + tyy);
        return M;
    }
};
template <typename T> struct SE3 {
    SO3<T> rot; T t[3];
    SE3() {}
    explicit SE3(const Eigen::Matrix<T, 4, 4>& P) {
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) rot.R[3 * r + c] = P(r, c); t[r] = P(r, 3); }
        T* q = rot.q;  // quaternionbase_assign_impl<.., 3, 3>
        T s = P(0, 0) + P(1, 1) + P(2, 2);
        if (s > 0) {
            rot.branch = 3;
            s = std::sqrt(s + T(1)); q[3] = T(0.5) * s; s = T(0.5) / s;
            q[0] = (P(2, 1) - P(1, 2)) * s; q[1] = (P(0, 2) - P(2, 0)) * s; q[2] = (P(1, 0) - P(0, 1)) * s;
        } else {
            int i = 0;
            if (P(1, 1) > P(0, 0)) i = 1;
            if (P(2, 2) > P(i, i)) i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            rot.branch = i;
            s = std::sqrt(P(i, i) - P(j, j) - P(k, k) + T(1)); q[i] = T(0.5) * s; s = T(0.5) / s;
            q[3] = (P(k, j) - P(j, k)) * s; q[j] = (P(j, i) + P(i, j)) * s; q[k] = (P(k, i) + P(i, k)) * s;
        }
    }
    const SO3<T>& so3() const { return rot; }
    template <int O> Eigen::Matrix<T, 3, 1, O> operator*(const Eigen::Matrix<T, 3, 1, O>& p) const {
        Eigen::Matrix<T, 3, 1, O> o;
        if (t_mode == 0) {
            for (int r = 0; r < 3; ++r)
                o.m[r] = std::fma(rot.R[3 * r + 2], p(2), std::fma(rot.R[3 * r + 1], p(1), std::fma(rot.R[3 * r], p(0), t[r])));
            return o;
        }
        const T* q = rot.q;  // _transformVector: uv = 2 q.vec x p;  p + w uv + q.vec x uv;  then the translation
        T uv[3], c2[3];
        uv[0] = q[1] * p(2) - q[2] * p(1); uv[1] = q[2] * p(0) - q[0] * p(2); uv[2] = q[0] * p(1) - q[1] * p(0);
        for (int i = 0; i < 3; ++i) uv[i] += uv[i];
        c2[0] = q[1] * uv[2] - q[2] * uv[1]; c2[1] = q[2] * uv[0] - q[0] * uv[2]; c2[2] = q[0] * uv[1] - q[1] * uv[0];
        for (int i = 0; i < 3; ++i) o.m[i] = ((p(i) + q[3] * uv[i]) + c2[i]) + t[i];
        return o;
    }
};
}  // namespace Sophus

#pragma clang fp contract(fast)
#include REF_BODY_INC
#pragma clang fp contract(off)

// mode: 0 matrix, 1 quaternion.  Per-point outputs pot [N], grad [N,3], col [N]; per-pair outputs pair_pot [N,O],
// pair_grad [N,O,3], pair_col [N,O].  Returns 0, or -1 for a mode it does not know.
extern "C" int ref_sdf_loss_forward(int mode, const float* pose_init, const float* grids, const float* limits, const float* points,
                                    const float* eps, const float* pad, const float* clr, const float* dis, int N, int O, float* pot,
                                    float* grad, float* col, float* pair_pot, float* pair_grad, float* pair_col) {
    if (mode != 0 && mode != 1) return -1;
    t_mode = mode;
    const int n = N * O;
    std::memset(pair_pot, 0, sizeof(float) * n); std::memset(pair_col, 0, sizeof(float) * n); std::memset(pair_grad, 0, sizeof(float) * n * 3);
    std::memset(pot, 0, sizeof(float) * N); std::memset(col, 0, sizeof(float) * N); std::memset(grad, 0, sizeof(float) * N * 3);
    SDFdistanceForward<float>(n, pose_init, grids, limits, points, eps, pad, clr, dis, N, O, pair_pot, pair_col, pair_grad);
    sum_gradients<float>(n, pair_pot, O, 1, pot);
    sum_gradients<float>(n, pair_col, O, 1, col);
    sum_gradients<float>(n * 3, pair_grad, O, 3, grad);
    t_mode = 0;
    return 0;
}

// Which branch of the matrix -> quaternion assignment pose [16] takes: 3 = trace > 0, else the pivot index 0 / 1 / 2.
extern "C" int ref_quaternion_branch(const float* pose) {
    Eigen::Matrix<float, 4, 4> P;
    for (int i = 0; i < 16; ++i) P.m[i] = pose[i];
    return Sophus::SE3<float>(P).so3().branch;
}
