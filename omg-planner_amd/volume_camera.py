"""A depth camera on the SDF pool: the specification of omgx_render_volumes (csrc/omg_volume_camera.hip and
csrc/omg_volume_camera_body.h follow it operation by operation).

camera.render_depth casts rays at triangle meshes.  The objects of a scene table (scenes.OBJECT_DTYPE records plus float32
volumes in one pool) have no meshes: fused and TSDF-blended obstacles, segmented targets and plane half-spaces exist as volumes
only.  Here one ray per pixel is sphere-traced through the trilinear interpolant of every object's volume, the interpolant
registration.value_gradient reads, and the nearest crossing of `level` gives depth, object index and surface normal.  Every TSDF
stack pairs "integrate" with "ray-cast the volume"; this is the second half.

The camera is camera.py's: pixel (r, c) is the ray from the camera origin with dx = (c - cx) / fx, dy = (r - cy) / fy, dz = 1,
so t is the depth along the optical axis and the images go into camera.pixel_clouds, the fusion, the TSDF and the plane ops as
render_depth's do.

Everything is plain numpy float64, every operation rounded on its own, dot products written (a*x + b*y) + c*z, and nothing but
+ - * /, sqrt, comparisons and float-to-int truncation, so that the device can equal the bits.  Not part of the contract: colour,
a far plane, shadows, anti-aliasing, noise, the TSDF pair arrays themselves, empty-space skipping structures.
"""
from __future__ import annotations

import numpy as np

from . import _lib, registration as _reg

MAX_STEPS = _lib.CONSTANTS["OMGX_VOLUME_CAMERA_MAX_STEPS"]  # the largest max_steps a call may ask for
MIN_STEP = 1e-4      # default shortest step along the ray's direction, in metres
DEFAULT_STEPS = 512  # default max_steps


def _finite(x) -> bool:
    return bool(np.isfinite(float(x)))


def check_scalars(level, t_min, min_step, relax, max_steps) -> None:
    """The scalar arguments of render_volumes (ValueError)."""
    if not (_finite(level) and _finite(t_min) and _finite(min_step) and _finite(relax)):
        raise ValueError("level, t_min, min_step and relax must be finite")
    if float(t_min) < 0 or float(min_step) <= 0 or not 0 < float(relax) <= 1:
        raise ValueError("t_min must be >= 0, min_step > 0 and relax in (0, 1]")
    if not 1 <= int(max_steps) <= MAX_STEPS:
        raise ValueError(f"max_steps must be in [1, {MAX_STEPS}]")


def check_table(objects, scene_begin, pool_elems: int, cameras, visible):
    """The records, ranges, cameras and flags of render_volumes (ValueError) -> (objects, scene_begin int64 [S+1], cameras
    [S,16], visible bool [n]).  Only the visible objects of the scenes' ranges are looked at."""
    from . import camera as _cam, scenes as _sc
    objects = np.asarray(objects)
    if objects.dtype != _sc.OBJECT_DTYPE or objects.ndim != 1:
        raise ValueError("objects must be a 1-d array of scenes.OBJECT_DTYPE records")
    cameras = _cam.check_camera_rows(cameras)
    begin = np.asarray(scene_begin, np.int64).reshape(-1)
    S, n = len(cameras), len(objects)
    if len(begin) != S + 1 or begin[0] < 0 or (np.diff(begin) < 0).any() or begin[-1] > n:
        raise ValueError(f"scene_begin must be [S+1] = [{S + 1}], ascending, inside the {n} records")
    if visible is None:
        vis = np.ones(n, bool)
    else:
        vis = np.asarray(visible).reshape(-1) != 0
        if len(vis) != n:
            raise ValueError(f"visible must have one flag per record ({n}), got {len(vis)}")
    at = np.arange(int(begin[0]), int(begin[-1]))
    at = at[vis[at]]  # the visible records of the scenes, all at once: a table has hundreds
    r = objects[at]
    dims, off = r["dim"].astype(np.int64), r["grid_offset"].astype(np.int64)
    with np.errstate(invalid="ignore"):
        bad = (dims < 2).any(axis=1) | ~(np.isfinite(r["inv_delta"]) & (r["inv_delta"] > 0))
    if bad.any():
        raise ValueError(f"object {int(at[bad][0])}: every axis needs two samples and inv_delta must be finite and positive")
    bad = (off < 0) | (off + dims.prod(axis=1) > int(pool_elems))
    if bad.any():
        raise ValueError(f"object {int(at[bad][0])}: the grid leaves the pool of {int(pool_elems)} elements")
    return objects, begin, cameras, vis


def object_from_camera(pose_inv, Wc) -> np.ndarray:
    """m [12]: the rows of obj_from_cam = pose_inv (the record's float32 rows, widened) times world_from_cam (Wc [12]).
    m[4i+j] = (P[4i]*Wc[j] + P[4i+1]*Wc[4+j]) + P[4i+2]*Wc[8+j];  m[4i+3] = ((P[4i]*Wc[3] + P[4i+1]*Wc[7]) + P[4i+2]*Wc[11]) + P[4i+3]."""
    P = np.asarray(pose_inv, np.float32).astype(np.float64).reshape(12)
    Wc = np.asarray(Wc, np.float64).reshape(12)
    m = np.zeros(12)
    for i in range(3):
        for j in range(3):
            m[4 * i + j] = (P[4 * i] * Wc[j] + P[4 * i + 1] * Wc[4 + j]) + P[4 * i + 2] * Wc[8 + j]
        m[4 * i + 3] = ((P[4 * i] * Wc[3] + P[4 * i + 1] * Wc[7]) + P[4 * i + 2] * Wc[11]) + P[4 * i + 3]
    return m


class _Grid:
    """What a ray reads of one record."""

    def __init__(self, obj):
        self.lo = np.asarray(obj["lo"], np.float32).astype(np.float64)
        self.dim = [int(d) for d in obj["dim"]]
        self.hi = [float(d - 1) for d in self.dim]
        self.inv_delta, self.offset = float(obj["inv_delta"]), int(obj["grid_offset"])


def sample(grid: _Grid, pool, uo, ud, t):
    """The interpolant at parameter t of rays in grid coordinates (uo, ud: lists of three [n]) -> (v [n], g [n,3]).
    u_a = uo_a + t*ud_a; clamped by comparisons: !(u_a >= 0) -> 0, u_a > hi_a -> hi_a; i_a = min(int(u_a), dim_a - 2);
    f_a = u_a - i_a (exactly 1.0 on the far face); then registration.trilinear."""
    i, f = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            u = uo[a] + t * ud[a]
            u = np.where(u >= 0.0, u, 0.0)
            u = np.where(u > grid.hi[a], grid.hi[a], u)
            k = np.minimum(u.astype(np.int64), grid.dim[a] - 2)
            i.append(k), f.append(u - k.astype(np.float64))
        base = grid.offset + (i[0] * grid.dim[1] + i[1]) * grid.dim[2] + i[2]
        v, gx, gy, gz = _reg.trilinear(pool, base, grid.dim[1] * grid.dim[2], grid.dim[2], f[0], f[1], f[2], grid.inv_delta)
    return v, np.stack([gx, gy, gz], -1)


def slab(grid: _Grid, uo, ud, t_min: float):
    """The ray's interval inside the box [0, hi] of grid coordinates -> (ok, t0, t1) [n].  From t0 = t_min, t1 = +inf, per axis:
    ud_a == 0: ok &= 0 <= uo_a <= hi_a; otherwise ta = (0.0 - uo_a) / ud_a, tb = (hi_a - uo_a) / ud_a, (l, h) = (ta, tb) if
    ta <= tb else (tb, ta); l > t0: t0 = l; h < t1: t1 = h.  Finally ok &= (t0 <= t1) & (t1 < +inf)."""
    n = len(uo[0])
    t0, t1, ok = np.full(n, float(t_min)), np.full(n, np.inf), np.ones(n, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(3):
            zero = ud[a] == 0.0
            ok &= ~zero | ((uo[a] >= 0.0) & (uo[a] <= grid.hi[a]))
            den = np.where(zero, 1.0, ud[a])
            ta, tb = (0.0 - uo[a]) / den, (grid.hi[a] - uo[a]) / den
            first = ta <= tb
            l, h = np.where(first, ta, tb), np.where(first, tb, ta)
            t0 = np.where(~zero & (l > t0), l, t0)
            t1 = np.where(~zero & (h < t1), h, t1)
        ok &= (t0 <= t1) & (t1 < np.inf)
    return ok, t0, t1


def march(grid: _Grid, pool, uo, ud, nrm, t0, t1, level: float, min_step: float, relax: float, max_steps: int):
    """Sphere tracing of rays that passed the slab test -> (hit [n] bool, th [n], samples [n] int32).

    t = t0, v = sample(t0); v <= level: a hit at t0 (the ray starts inside: the box face counts as surface).  Otherwise at most
    max_steps times: s = (v - level) * relax, !(s >= min_step): s = min_step; tn = t + s / nrm, !(tn <= t1): tn = t1;
    vn = sample(tn); vn <= level: th = t + (tn - t) * ((v - level) / (v - vn)), !(th >= t): th = t, !(th <= tn): th = tn, a hit;
    else tn >= t1: a miss; else (t, v) = (tn, vn).  Running out of steps is a miss."""
    n = len(t0)
    hit, th, count = np.zeros(n, bool), np.full(n, np.inf), np.zeros(n, np.int32)
    if n == 0:
        return hit, th, count
    t = t0.copy()
    v, _ = sample(grid, pool, uo, ud, t)
    count += 1
    hit = v <= level
    th = np.where(hit, t0, th)
    live = np.flatnonzero(~hit)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _ in range(int(max_steps)):
            if not len(live):
                break
            tl, vl = t[live], v[live]
            s = (vl - level) * relax
            s = np.where(s >= min_step, s, min_step)
            tn = tl + s / nrm[live]
            tn = np.where(tn <= t1[live], tn, t1[live])
            vn, _ = sample(grid, pool, [x[live] for x in uo], [x[live] for x in ud], tn)
            count[live] += 1
            crossed = vn <= level
            x = tl + (tn - tl) * ((vl - level) / (vl - vn))
            x = np.where(x >= tl, x, tl)
            x = np.where(x <= tn, x, tn)
            hit[live[crossed]] = True
            th[live[crossed]] = x[crossed]
            t[live], v[live] = tn, vn
            live = live[~crossed & ~(tn >= t1[live])]
    return hit, th, count


def render_volumes(objects, scene_begin, pool, cameras, H: int, W: int, visible=None, level: float = 0.0, t_min: float = 1e-6,
                   min_step: float = MIN_STEP, relax: float = 1.0, max_steps: int = DEFAULT_STEPS):
    """Depth, object and normal images of S scenes of a scene table -> (t [S,H,W] float64, inst [S,H,W] int32, normal [S,H,W,3]
    float64, steps [S,H,W] int32); background: (+inf, -1, (0,0,0)).  The specification of omgx_render_volumes.

    objects: scenes.OBJECT_DTYPE records (pose_inv, lo, dim, inv_delta and grid_offset are read; `disabled` is ignored: a camera
    sees the floor); scene s owns the records [scene_begin[s], scene_begin[s+1]) and inst is local to the scene; pool: the float32
    volume pool; cameras [S,16] (camera.camera_rows: fx, fy, cx, cy, Wc = the rows of world_from_cam); visible: uint8 per record or
    None (all).  Per pixel, from best = +inf, inst = -1, for the scene's objects k = 0, 1, ... in order, invisible ones skipped:

      m = object_from_camera(pose_inv, Wc);  o_a = m[4a+3];  d_a = (m[4a]*dx + m[4a+1]*dy) + m[4a+2];
      nrm = sqrt((d0*d0 + d1*d1) + d2*d2);  uo_a = (o_a - float64(lo_a)) * inv_delta - 0.5;  ud_a = d_a * inv_delta  (the
      cell-centre convention of registration.value_gradient);  (ok, t0, t1) = slab: not ok, the object takes no sample;
      (hit, th) = march;  hit and th < best (strict: the lowest index wins a tie): best = th, inst = k, and with g the gradient of
      sample(th): n_j = (m[j]*g0 + m[4+j]*g1) + m[8+j]*g2, nn = (n0*n0 + n1*n1) + n2*n2, normal = n / sqrt(nn) if nn > 0 else 0.

    steps: the samples the marches of all objects of the pixel took (the normal's sample is not counted).  The negated comparisons
    make NaN and +-inf voxels harmless: t stays finite inside [t0, t1]; such a ray leaves through the far face or runs out of steps."""
    from . import camera as _cam
    check_scalars(level, t_min, min_step, relax, max_steps)
    pool = np.asarray(pool)
    if pool.dtype != np.float32 or pool.ndim != 1:
        raise ValueError("pool must be a 1-d float32 array")
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"H and W must be >= 1, got {H} and {W}")
    objects, begin, cameras, vis = check_table(objects, scene_begin, len(pool), cameras, visible)
    level, t_min, min_step, relax = float(level), float(t_min), float(min_step), float(relax)
    S, N = len(cameras), H * W
    t_img, inst_img = np.full((S, N), np.inf), np.full((S, N), -1, np.int32)
    n_img, steps = np.zeros((S, N, 3)), np.zeros((S, N), np.int32)
    for s in range(S):
        dx, dy = _cam.pixel_directions(cameras[s], H, W)
        for k, o in enumerate(range(int(begin[s]), int(begin[s + 1]))):
            if not vis[o]:
                continue
            grid = _Grid(objects[o])
            m = object_from_camera(objects[o]["pose_inv"], cameras[s, 4:])
            with np.errstate(invalid="ignore", over="ignore"):
                d = [(m[4 * a] * dx + m[4 * a + 1] * dy) + m[4 * a + 2] for a in range(3)]
                nrm = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                uo = [np.full(N, (m[4 * a + 3] - grid.lo[a]) * grid.inv_delta - 0.5) for a in range(3)]
                ud = [d[a] * grid.inv_delta for a in range(3)]
            ok, t0, t1 = slab(grid, uo, ud, t_min)
            at = np.flatnonzero(ok)
            cut = lambda xs: [x[at] for x in xs]
            hit, th, count = march(grid, pool, cut(uo), cut(ud), nrm[at], t0[at], t1[at], level, min_step, relax, max_steps)
            steps[s, at] += count
            take = hit & (th < t_img[s, at])
            w = at[take]
            if not len(w):
                continue
            t_img[s, w], inst_img[s, w] = th[take], k
            _, g = sample(grid, pool, [x[w] for x in uo], [x[w] for x in ud], th[take])
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                nv = [(m[j] * g[:, 0] + m[4 + j] * g[:, 1]) + m[8 + j] * g[:, 2] for j in range(3)]
                nn = (nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]
                root = np.sqrt(nn)
                n_img[s, w] = np.stack([np.where(nn > 0.0, x / root, 0.0) for x in nv], -1)
    return t_img.reshape(S, H, W), inst_img.reshape(S, H, W), n_img.reshape(S, H, W, 3), steps.reshape(S, H, W)
