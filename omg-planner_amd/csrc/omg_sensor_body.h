// omg_sensor_body.h — what the kernels of omg_sensor.hip do for one pixel: a sensor's raw value as a depth, the noise scale, the
// flying-pixel test, the bilateral filter over the survivors, and the vertex, normal and cosine of a pixel of a conditioned image,
// as functions that also compile for the host, so that the arithmetic can be stepped through and compared with
// omg-planner_amd/sensor.py without a GPU.  float64 with + - * /, sqrt (normals only) and comparisons, one rounded operation per
// operation of the specification, in its order; rejections as negated comparisons (NaN falls on the "no" side).  The functions
// read a STAGED image: doubles at a pitch, with a halo around the pixels asked about, in which a pixel without a return (or
// outside the image) is 0.0.  No HIP built-ins here.
#pragma once
#include <cmath>
#include <cstdint>

#include "omg_image_body.h"

#if defined(__HIPCC__)
#define SENSOR_HD __host__ __device__ __forceinline__
#else
#define SENSOR_HD inline
#endif

#pragma clang fp contract(off)

// The staged tile of k_depth_condition: 16 x 16 pixels with a halo of OMGX_SENSOR_MAX_RADIUS + 1 at most, 32 rows of 32 doubles
// used, at a pitch of 48 doubles.  ds_read_b64 banks by (byte / 4) % 64 within each half of a wave; under the row map a half
// wave reads 16 consecutive doubles of two consecutive rows, 32 banks each, and a pitch of 48 doubles (96 dwords = 32 mod 64) puts
// the second row on the other 32 banks, whatever the tap and the radius.  A pitch of 32 would put both rows on the same banks.
#define SENSOR_HALO_MAX (OMGX_SENSOR_MAX_RADIUS + 1)
#define SENSOR_SIDE_MAX (IMAGE_TILE + 2 * SENSOR_HALO_MAX)
#define SENSOR_PITCH 48
#define SENSOR_LDS_BYTES (SENSOR_SIDE_MAX * SENSOR_PITCH * 8)
static_assert(SENSOR_PITCH >= SENSOR_SIDE_MAX && (2 * SENSOR_PITCH) % 64 == 32, "two rows of 16 doubles on disjoint banks");

// Element `at` of the input images as a depth: uint16 times scale, or the double as given; 0.0 unless it is a return, which is
// finite and inside [z_min, z_max] (z_min > 0, so 0.0 is never one).
SENSOR_HD double sensor_depth(const void* in, int kind, int64_t at, double scale, double z_min, double z_max) {
    const double z = kind == OMGX_SENSOR_UINT16 ? (double)((const uint16_t*)in)[at] * scale : ((const double*)in)[at];
    return z >= z_min && z <= z_max ? z : 0.0;  // (NaN and the infinities fail a comparison)
}

SENSOR_HD double sensor_tau(double z, double t0, double t1, double t2) { return (t0 + t1 * z) + t2 * (z * z); }

// |zq - zp| <= tau, for a neighbour with a return.
SENSOR_HD bool sensor_near(double zq, double zp, double tau) {
    const double d = zq - zp;
    return zq > 0.0 && d <= tau && -d <= tau;
}

// Does the staged pixel z[at] (returns, not yet masked) survive: a return with at least min_support of its 8 neighbours near it?
SENSOR_HD bool sensor_survives(const double* z, int pitch, int at, double t0, double t1, double t2, int min_support) {
    const double zp = z[at];
    const double tau = sensor_tau(zp, t0, t1, t2);
    int n = 0;
    for (int dr = -1; dr <= 1; ++dr)
        for (int dc = -1; dc <= 1; ++dc)
            if (dr != 0 || dc != 0) n += sensor_near(z[at + dr * pitch + dc], zp, tau) ? 1 : 0;
    return zp > 0.0 && n >= min_support;
}

// The filtered depth of the survivor z[at] of a staged image in which everything but the survivors is 0.0.  table: (2R+1)^2
// spatial weights, row-major.  The taps one after the other in the table's order; Tukey's biweight on d / rho.
SENSOR_HD double sensor_filter(const double* z, int pitch, int at, int R, const double* table, double range_scale, double t0, double t1,
                               double t2) {
    const double zp = z[at];
    if (R == 0) return zp;
    const double rho = range_scale * sensor_tau(zp, t0, t1, t2);
    double num = 0.0, den = 0.0;
    int k = 0;
    for (int dr = -R; dr <= R; ++dr)
        for (int dc = -R; dc <= R; ++dc, ++k) {
            const double zq = z[at + dr * pitch + dc];
            const double x = (zq - zp) / rho;
            const double u = 1.0 - x * x;
            const double w = zq > 0.0 && u > 0.0 ? table[k] * (u * u) : 0.0;
            num = num + w * zq;
            den = den + w;
        }
    return den > 0.0 ? num / den : zp;
}

// ---- normals --------------------------------------------------------------------------------------------------------------
// Pixel (r, c) of ONE conditioned image of H x W (0.0 or less, or NaN: nothing there) with the intrinsics k = fx, fy, cx, cy; the
// pixel lies at img[base + r * pitch + c]: the image itself (base 0, pitch W), or a staged tile of it (base: minus its corner).
// -> the flag: OMGX_SENSOR_KEPT, | OMGX_SENSOR_NO_NORMAL, OMGX_SENSOR_GRAZING, or `flag` (OMGX_SENSOR_NO_RETURN if that is 0) where
// the image has nothing; n[3]: the unit normal in the camera's frame, facing the camera, or zeros; *cosine: of the angle between
// the normal and the ray back to the camera, or 0.0; *depth: the pixel's depth, 0.0 if grazing or nothing.
SENSOR_HD void sensor_vertex(const double* img, int64_t base, int pitch, int r, int c, const double* k, double* P) {
    double dx, dy;
    image_pixel_dir(r, c, k[0], k[1], k[2], k[3], dx, dy);
    const double z = img[base + (int64_t)r * pitch + c];
    P[0] = dx * z, P[1] = dy * z, P[2] = z;
}

// One difference: after minus before if both are usable, else the one-sided difference to the usable one -> false if neither.
// (r0, c0) before and (r1, c1) after the pixel with the vertex P; a neighbour outside the image is not usable (and not read).
SENSOR_HD bool sensor_difference(const double* img, int64_t base, int pitch, int H, int W, int r0, int c0, int r1, int c1, const double* k,
                                 const double* P, double tau, double* out) {
    const bool before = r0 >= 0 && c0 >= 0 && sensor_near(img[base + (int64_t)r0 * pitch + c0], P[2], tau);
    const bool after = r1 < H && c1 < W && sensor_near(img[base + (int64_t)r1 * pitch + c1], P[2], tau);
    if (!before && !after) return false;
    double A[3] = {P[0], P[1], P[2]}, B[3] = {P[0], P[1], P[2]};
    if (before) sensor_vertex(img, base, pitch, r0, c0, k, A);
    if (after) sensor_vertex(img, base, pitch, r1, c1, k, B);
    out[0] = B[0] - A[0], out[1] = B[1] - A[1], out[2] = B[2] - A[2];
    return true;
}

SENSOR_HD uint8_t sensor_normal(const double* img, int64_t base, int pitch, int H, int W, int r, int c, const double* k, double t0, double t1,
                                double t2, double cos_min, uint8_t flag, double* n, double* cosine, double* depth) {
    n[0] = n[1] = n[2] = 0.0, *cosine = 0.0, *depth = 0.0;
    const double z = img[base + (int64_t)r * pitch + c];
    if (!(z > 0.0)) return flag != 0 ? flag : (uint8_t)OMGX_SENSOR_NO_RETURN;
    *depth = z;
    double P[3], a[3], b[3];
    sensor_vertex(img, base, pitch, r, c, k, P);
    const double tau = sensor_tau(z, t0, t1, t2);
    const bool ha = sensor_difference(img, base, pitch, H, W, r, c - 1, r, c + 1, k, P, tau, a);
    const bool hb = sensor_difference(img, base, pitch, H, W, r - 1, c, r + 1, c, k, P, tau, b);
    if (!ha || !hb) return OMGX_SENSOR_KEPT | OMGX_SENSOR_NO_NORMAL;
    double m0 = a[1] * b[2] - a[2] * b[1], m1 = a[2] * b[0] - a[0] * b[2], m2 = a[0] * b[1] - a[1] * b[0];
    const double s = (m0 * P[0] + m1 * P[1]) + m2 * P[2];
    const double nn = (m0 * m0 + m1 * m1) + m2 * m2;
    if (!(s > 0.0 || s < 0.0) || !(nn > 0.0)) return OMGX_SENSOR_KEPT | OMGX_SENSOR_NO_NORMAL;
    if (s > 0.0) m0 = -m0, m1 = -m1, m2 = -m2;
    const double len = sqrt(nn);
    const double n0 = m0 / len, n1 = m1 / len, n2 = m2 / len;
    const double cs = -((n0 * P[0] + n1 * P[1]) + n2 * P[2]) / sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]);
    if (cs < cos_min) {
        *depth = 0.0;
        return OMGX_SENSOR_GRAZING;
    }
    n[0] = n0, n[1] = n1, n[2] = n2, *cosine = cs;
    return OMGX_SENSOR_KEPT;
}

// On the host: the entry points' checks of the scalars -> OMGX_OK or OMGX_ERR_INVALID.
static inline int sensor_check_tau(double t0, double t1, double t2) {
    const double t[3] = {t0, t1, t2};
    return image_all_finite(t, 3) && t0 >= 0.0 && t1 >= 0.0 && t2 >= 0.0 ? OMGX_OK : OMGX_ERR_INVALID;
}
// The spatial table of radius R (0 <= R <= OMGX_SENSOR_MAX_RADIUS): finite, >= 0, the centre > 0.
static inline int sensor_check_table(const double* h_table, int R) {
    const int side = 2 * R + 1;
    if (!image_all_finite(h_table, (int64_t)side * side)) return OMGX_ERR_INVALID;
    for (int k = 0; k < side * side; ++k)
        if (h_table[k] < 0.0) return OMGX_ERR_INVALID;
    return h_table[(side * side) / 2] > 0.0 ? OMGX_OK : OMGX_ERR_INVALID;
}
// Do the byte ranges [a, a + na) and [b, b + nb) share a byte?
static inline bool sensor_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}
