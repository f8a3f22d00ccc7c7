// omg_mesh_sdf_body.h — what k_mesh_sdf (omg_mesh_sdf.hip) does for one (node, face) pair, as a function that also compiles for
// the host, so that the arithmetic can be stepped through and compared with scenes.mesh_sdf without a GPU.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSDF_HD __host__ __device__ __forceinline__
#else
#define MSDF_HD inline
#endif

#pragma clang fp contract(off)

MSDF_HD double msdf_dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}

// node p against the face T = {a, b, c} (nine doubles): `best` keeps the smallest squared distance, `wsum` adds the face's
// atan2 term of the winding number (half its solid angle seen from p)
MSDF_HD void mesh_sdf_pair(double px, double py, double pz, const double* T, double& best, double& wsum) {
    const double ax = T[0], ay = T[1], az = T[2], bx = T[3], by = T[4], bz = T[5], cx = T[6], cy = T[7], cz = T[8];
    // ---- closest point on the triangle (scenes.closest_point_on_triangle, the same operations in the same order) ----
    const double abx = bx - ax, aby = by - ay, abz = bz - az;
    const double acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const double d1 = msdf_dot3(abx, aby, abz, apx, apy, apz), d2 = msdf_dot3(acx, acy, acz, apx, apy, apz);
    const double d3 = msdf_dot3(abx, aby, abz, bpx, bpy, bpz), d4 = msdf_dot3(acx, acy, acz, bpx, bpy, bpz);
    const double d5 = msdf_dot3(abx, aby, abz, cpx, cpy, cpz), d6 = msdf_dot3(acx, acy, acz, cpx, cpy, cpz);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double e1 = d4 - d3, e2 = d5 - d6;
    const bool rA = d1 <= 0.0 && d2 <= 0.0, rB = d3 >= 0.0 && d4 <= d3, rC = d6 >= 0.0 && d5 <= d6;
    const bool rAB = vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0, rAC = vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0;
    const bool rBC = va <= 0.0 && e1 >= 0.0 && e2 >= 0.0;
    // the first region that holds, in the order A, B, AB, C, AC, BC; none: the interior.  Vertex and edge regions are
    // base + (num / den) * dir with num = 0, den = 1 at a vertex
    const bool vertex = rA || rB || (!rAB && rC);
    const bool fromB = !rA && (rB || (!rAB && !rC && !rAC));                      // B, BC
    const bool fromC = !rA && !rB && !rAB && rC;                                   // C
    const bool dirAB = rAB, dirAC = !rAB && rAC;                                   // (only read when not a vertex)
    const double num = vertex ? 0.0 : (dirAB ? d1 : (dirAC ? d2 : e1));
    const double den = vertex ? 1.0 : (dirAB ? d1 - d3 : (dirAC ? d2 - d6 : e1 + e2));
    const double t = num / den;
    const double ox = fromB ? bx : (fromC ? cx : ax), oy = fromB ? by : (fromC ? cy : ay), oz = fromB ? bz : (fromC ? cz : az);
    const double ex = dirAB ? abx : (dirAC ? acx : cx - bx), ey = dirAB ? aby : (dirAC ? acy : cy - by),
                 ez = dirAB ? abz : (dirAC ? acz : cz - bz);
    const double qex = ox + t * ex, qey = oy + t * ey, qez = oz + t * ez;
    const double inv = 1.0 / ((va + vb) + vc);
    const double bv = vb * inv, bw = vc * inv;
    const double qix = (ax + abx * bv) + acx * bw, qiy = (ay + aby * bv) + acy * bw, qiz = (az + abz * bv) + acz * bw;
    const bool interior = !(rA || rB || rAB || rC || rAC || rBC);
    const double rx = px - (interior ? qix : qex), ry = py - (interior ? qiy : qey), rz = pz - (interior ? qiz : qez);
    const double dd = (rx * rx + ry * ry) + rz * rz;
    best = dd < best ? dd : best;
    // ---- solid angle of the face seen from the node (A = a - p = -ap, B, C alike: all three negated) ----
    const double la = sqrt(msdf_dot3(apx, apy, apz, apx, apy, apz)), lb = sqrt(msdf_dot3(bpx, bpy, bpz, bpx, bpy, bpz)),
                 lc = sqrt(msdf_dot3(cpx, cpy, cpz, cpx, cpy, cpz));
    const double nx = bpy * cpz - bpz * cpy, ny = bpz * cpx - bpx * cpz, nz = bpx * cpy - bpy * cpx;
    const double det = -msdf_dot3(apx, apy, apz, nx, ny, nz);
    const double den2 = ((la * lb) * lc + msdf_dot3(apx, apy, apz, bpx, bpy, bpz) * lc) +
                        (msdf_dot3(bpx, bpy, bpz, cpx, cpy, cpz) * la + msdf_dot3(cpx, cpy, cpz, apx, apy, apz) * lb);
    wsum += atan2(det, den2);
}
