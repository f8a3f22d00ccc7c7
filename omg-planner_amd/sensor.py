"""Depth conditioning: a depth sensor's frames to the clean depth images every other perception op reads, and the vertex and
normal maps of such an image.  The specification of omgx_depth_condition / omgx_depth_normals (include/omg_hip.h section 23;
csrc/omg_sensor_body.h follows it operation by operation) in plain numpy, and `simulate`, a host-only sensor model for tests and
timing.

A real sensor hands over uint16 millimetres in which 0 means "no return"; its axial noise grows with range; between foreground
and background it invents flying pixels at every silhouette; surfaces seen at grazing angles come back as junk.  The images
camera.py and volume_camera.py render have none of that, and fusion.py, tsdf.py, segmentation.py and planes.py were specified
on them.  condition_depth turns frames [V,H,W] into such images: 0.0 ("no information", what every reader already takes:
!(d > 0)) where there is no return or a flying pixel, a bilateral filter over the rest.  depth_normals adds what a rendered
observation has and an observed one lacked: unit normals in the camera's frame that face the camera (volume_camera.py's
convention for render_volumes: the outward normal of a surface the camera sees), and drops the pixels seen at a grazing angle.

condition_depth, per pixel p:
  z = float64(raw) * scale for uint16 frames, the value itself for float64 frames (a rendered image can go in: +inf is no return)
  RETURN: z_min <= z <= z_max, both inclusive (NaN, +-inf, 0 and negatives fail; z_min > 0)
  tau(z) = (t0 + t1*z) + t2*(z*z)                     the noise scale; structured light and stereo go quadratic in range
  NEAR(q, p): q has a return, and with d = z(q) - z(p): d <= tau(z(p)) and -d <= tau(z(p))
  FLYING: p has a return and fewer than min_support of its 8 neighbours (those inside the image) are NEAR it
  SURVIVOR: a return that is not flying.  Over the (2R+1)^2 window, the taps q in row-major order with the spatial weight
  table[k], k = 0, 1, ... (a tap outside the image or not a survivor weighs 0):
      rho = range_scale * tau(z(p));  x = (z(q) - z(p)) / rho;  u = 1 - x*x;  w = table[k] * (u*u) if u > 0 else 0
      num = num + w * z(q);  den = den + w
  out = num / den if den > 0 else z(p); with R == 0 out = z(p).  Tukey's biweight has compact support: a tap across a depth step
  of rho or more weighs exactly nothing, so the filter does not round silhouettes.  The spatial weights are a table because exp
  on the device cannot equal numpy's bits; gaussian_table fills one.
  depth = out for survivors, else 0.0;  flags = KEPT (0), NO_RETURN (1) or FLYING (2).

depth_normals, per pixel p of a conditioned image (THERE: z > 0) with the intrinsics fx, fy, cx, cy:
  P = (dx*z, dy*z, z) with camera.py's ray dx = (c - cx) / fx, dy = (r - cy) / fy
  USABLE(q): inside the image, there, and NEAR(q, p) with the same tau
  a = P(right) - P(left) if both are usable, else P(right) - P(p) or P(p) - P(left), whichever is usable; b alike with down
  minus up; without a usable neighbour in either direction there is NO NORMAL
  m = a x b = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0);  s = (m0*P0 + m1*P1) + m2*P2;  nn = (m0*m0 + m1*m1) + m2*m2
  NO NORMAL unless (s > 0 or s < 0) and nn > 0;  m = -m if s > 0 (towards the camera);  n = m / sqrt(nn)
  cos = -((n0*P0 + n1*P1) + n2*P2) / sqrt((P0*P0 + P1*P1) + P2*P2);  GRAZING (3) if cos < cos_min: depth 0.0, normal zeros
  flags: KEPT, KEPT | NO_NORMAL (8), GRAZING; where nothing is there the flag that came in, or NO_RETURN if that is 0.

Everything is float64, every operation rounded on its own, with + - * /, comparisons and (in the normals) sqrt only, so that
the device can equal the bits.  Not part of the contract: lens distortion, registration of depth to colour, multi-path and
motion blur, temporal filtering, hole filling (a dropped pixel stays dropped), the sensor's own confidence image, and `simulate`.
"""
from __future__ import annotations

import numpy as np

MAX_RADIUS = 7
KEPT, NO_RETURN, FLYING, GRAZING, NO_NORMAL = 0, 1, 2, 3, 8
UINT16, FLOAT64 = 0, 1


def gaussian_table(radius: int, sigma: float) -> np.ndarray:
    """[(2R+1)^2] float64 spatial weights exp(-(dr*dr + dc*dc) / (2 sigma^2)), row-major; on the host, through numpy."""
    R = int(radius)
    if not 0 <= R <= MAX_RADIUS or not (np.isfinite(float(sigma)) and float(sigma) > 0):
        raise ValueError(f"radius must lie in [0, {MAX_RADIUS}] and sigma be finite and positive")
    d = np.arange(-R, R + 1, dtype=np.float64)
    return np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * float(sigma) ** 2)).reshape(-1)


def check_tau(tau):
    t = np.asarray(tau, np.float64).reshape(-1)
    if len(t) != 3 or not np.isfinite(t).all() or (t < 0).any():
        raise ValueError("tau must be three finite doubles >= 0: t0, t1, t2")
    return float(t[0]), float(t[1]), float(t[2])


def check_table(table, radius):
    R = int(radius)
    if not 0 <= R <= MAX_RADIUS:
        raise ValueError(f"radius must lie in [0, {MAX_RADIUS}], got {R}")
    table = np.asarray(table, np.float64).reshape(-1)
    n = (2 * R + 1) ** 2
    if len(table) != n or not np.isfinite(table).all() or (table < 0).any() or not table[n // 2] > 0:
        raise ValueError(f"table must be {n} finite weights >= 0 with a centre > 0")
    return R, np.ascontiguousarray(table)


def check_condition(frames, scale, z_min, z_max, tau, min_support, radius, table, range_scale):
    """The argument checks of condition_depth (the wrapper makes the same) -> (frames, kind, scale, z_min, z_max, (t0, t1, t2),
    min_support, R, table, range_scale)."""
    frames = np.asarray(frames)
    if frames.ndim != 3 or frames.dtype not in (np.uint16, np.float64):
        raise ValueError(f"frames must be [V,H,W] uint16 or float64, got {frames.shape} {frames.dtype}")
    if len(frames) and (frames.shape[1] < 1 or frames.shape[2] < 1):
        raise ValueError("H and W must be >= 1")
    scale, z_min, z_max, range_scale = float(scale), float(z_min), float(z_max), float(range_scale)
    if not (np.isfinite([scale, z_min, z_max, range_scale]).all() and scale > 0 and z_min > 0 and z_min <= z_max and range_scale > 0):
        raise ValueError("scale, z_min, z_max and range_scale must be finite, scale, z_min and range_scale > 0, z_min <= z_max")
    if not 0 <= int(min_support) <= 8:
        raise ValueError(f"min_support must lie in [0, 8], got {min_support}")
    R, table = check_table(table, radius)
    return frames, UINT16 if frames.dtype == np.uint16 else FLOAT64, scale, z_min, z_max, check_tau(tau), int(min_support), R, table, range_scale


def _shift(a, dr, dc, fill=0.0):
    """b[r, c] = a[r + dr, c + dc] over the last two axes, `fill` outside."""
    H, W = a.shape[-2:]
    out = np.full_like(a, fill)
    r0, r1, c0, c1 = max(0, -dr), min(H, H - dr), max(0, -dc), min(W, W - dc)
    if r0 < r1 and c0 < c1:
        out[..., r0:r1, c0:c1] = a[..., r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def _tau(z, t):
    return (t[0] + t[1] * z) + t[2] * (z * z)


def _near(zq, zp, tau):
    d = zq - zp
    return (zq > 0.0) & (d <= tau) & (-d <= tau)


def condition_depth(frames, scale: float, z_min: float, z_max: float, tau, min_support: int, radius: int, table, range_scale: float):
    """Frames [V,H,W] uint16 or float64 -> (depth [V,H,W] float64, flags [V,H,W] uint8): the module docstring, operation by
    operation.  tau = (t0, t1, t2); table: (2*radius+1)^2 spatial weights (gaussian_table)."""
    frames, kind, scale, z_min, z_max, t, min_support, R, table, range_scale = check_condition(frames, scale, z_min, z_max, tau, min_support, radius,
                                                                                               table, range_scale)
    with np.errstate(all="ignore"):
        z = frames.astype(np.float64) * scale if kind == UINT16 else frames
        ret = (z >= z_min) & (z <= z_max)
        z = np.where(ret, z, 0.0)
        tz = _tau(z, t)
        count = np.zeros(z.shape, np.int64)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if dr or dc:
                    count += _near(_shift(z, dr, dc), z, tz)
        keep = ret & (count >= min_support)
        zs = np.where(keep, z, 0.0)
        out = zs
        if R > 0:
            rho = range_scale * tz
            num, den, k = np.zeros(z.shape), np.zeros(z.shape), 0
            for dr in range(-R, R + 1):
                for dc in range(-R, R + 1):
                    zq = _shift(zs, dr, dc)
                    x = (zq - zs) / rho
                    u = 1.0 - x * x
                    w = np.where((zq > 0.0) & (u > 0.0), table[k] * (u * u), 0.0)
                    num, den, k = num + w * zq, den + w, k + 1
            out = np.where(den > 0.0, num / den, zs)
        depth = np.where(keep, out, 0.0)
    flags = np.where(keep, KEPT, np.where(ret, FLYING, NO_RETURN)).astype(np.uint8)
    return depth, flags


def check_normals(depth, intrinsics, tau, cos_min, flags):
    depth = np.asarray(depth)
    if depth.ndim != 3 or depth.dtype != np.float64:
        raise ValueError(f"depth must be [V,H,W] float64, got {depth.shape} {depth.dtype}")
    V = len(depth)
    if V and (depth.shape[1] < 1 or depth.shape[2] < 1):
        raise ValueError("H and W must be >= 1")
    k = np.asarray(intrinsics, np.float64)
    if k.shape != (V, 4) or not np.isfinite(k).all() or (k[:, :2] == 0).any():
        raise ValueError(f"intrinsics must be [{V},4], finite, with no focal length of zero")
    if not np.isfinite(float(cos_min)):
        raise ValueError("cos_min must be finite")
    if flags is not None:
        flags = np.asarray(flags)
        if flags.shape != depth.shape or flags.dtype != np.uint8:
            raise ValueError(f"flags must be uint8 {depth.shape}")
    return depth, np.ascontiguousarray(k), check_tau(tau), float(cos_min), flags


def depth_normals(depth, intrinsics, tau, cos_min: float, flags=None):
    """Conditioned images [V,H,W] float64 and intrinsics [V,4] -> (normals [V,H,W,3], depth_out [V,H,W], flags [V,H,W] uint8, cosine
    [V,H,W]): the module docstring, operation by operation.  flags: condition_depth's, or None."""
    depth, K, t, cos_min, flags = check_normals(depth, intrinsics, tau, cos_min, flags)
    V, H, W = depth.shape
    normals, depth_out, cosine = np.zeros((V, H, W, 3)), np.zeros((V, H, W)), np.zeros((V, H, W))
    flags_out = np.zeros((V, H, W), np.uint8)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        for v in range(V):
            z = depth[v]
            there = z > 0.0
            dx, dy = (c - K[v, 2]) / K[v, 0], (r - K[v, 3]) / K[v, 1]
            P = [dx * z, dy * z, z]
            tz = _tau(z, t)

            def difference(dr, dc):
                before, after = _near(_shift(z, -dr, -dc), z, tz), _near(_shift(z, dr, dc), z, tz)
                A = [np.where(before, _shift(P[j], -dr, -dc), P[j]) for j in range(3)]
                B = [np.where(after, _shift(P[j], dr, dc), P[j]) for j in range(3)]
                return [B[j] - A[j] for j in range(3)], before | after

            a, ha = difference(0, 1)
            b, hb = difference(1, 0)
            m = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            s = (m[0] * P[0] + m[1] * P[1]) + m[2] * P[2]
            nn = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
            has = there & ha & hb & ((s > 0.0) | (s < 0.0)) & (nn > 0.0)
            m = [np.where(s > 0.0, -x, x) for x in m]
            length = np.sqrt(nn)
            n = [x / length for x in m]
            cs = -((n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]) / np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2])
            grazing = has & (cs < cos_min)
            good = has & ~grazing
            for j in range(3):
                normals[v, :, :, j] = np.where(good, n[j], 0.0)
            cosine[v] = np.where(good, cs, 0.0)
            depth_out[v] = np.where(there & ~grazing, z, 0.0)
            base = np.zeros((H, W), np.uint8) if flags is None else flags[v]
            flags_out[v] = np.where(~there, np.where(base != 0, base, NO_RETURN), np.where(grazing, GRAZING, np.where(has, KEPT, KEPT | NO_NORMAL)))
    return normals, depth_out, flags_out, cosine


def simulate(t, rng, scale: float = 0.001, sigma=(0.0, 0.0), dropout: float = 0.0, flying=None):
    """A sensor's frame of the rendered images t [V,H,W] float64 (+inf: background) -> (frame [V,H,W] uint16, masks: a dict of bool
    [V,H,W] arrays "background", "dropout", "flying").  On the host, for tests and timing; no bit contract.
    sigma = (s0, s2): Gaussian axial noise of standard deviation s0 + s2*z^2.  flying: None, or (t0, t1, t2): a pixel on the far
    side of a step to a 4-neighbour that is nearer by more than 4 tau(its own depth) becomes a flying pixel at the mid depth of
    the two, every second one along the edge (none of them touches another, diagonals included).  Background and a `dropout`
    share of the pixels read 0.  The value is round(z / scale), cut to uint16."""
    t = np.asarray(t, np.float64)
    V, H, W = t.shape
    background = ~np.isfinite(t)
    clean = np.where(background, 0.0, t)
    z = clean + (float(sigma[0]) + float(sigma[1]) * clean * clean) * rng.standard_normal(t.shape)
    fly = np.zeros(t.shape, bool)
    if flying is not None:
        tau4 = 4.0 * _tau(clean, check_tau(flying))
        mid = np.zeros(t.shape)
        for dr, dc in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            q = _shift(clean, dr, dc)
            edge = ~background & (q > 0.0) & (clean - q > tau4) & (mid == 0.0)
            mid = np.where(edge, 0.5 * (clean + q), mid)
        for v, r, c in zip(*np.nonzero(mid)):  # row-major: a candidate next to a chosen one is passed over
            if not fly[v, max(r - 1, 0): r + 2, max(c - 1, 0): c + 2].any():
                fly[v, r, c] = True
        z = np.where(fly, mid, z)
    drop = ~background & ~fly & (rng.random(t.shape) < float(dropout))
    z = np.where(background | drop, 0.0, z)
    frame = np.clip(np.rint(z / float(scale)), 0, 65535).astype(np.uint16)
    return frame, {"background": background, "dropout": drop, "flying": fly}
