"""Weighted TSDF fusion: depth views to sub-voxel obstacle volumes.  The specification of omgx_tsdf_integrate / omgx_tsdf_states /
omgx_tsdf_blend (include/omg_hip.h section 20; csrc/omg_tsdf_body.h follows it operation by operation) in plain numpy.

fusion.carve_views labels a node FREE, SURFACE or UNKNOWN and fusion.distance_transform puts the zero level on voxel faces: the
observed surface is inflated by the band, every noisy frame thickens it, and a node once SURFACE stays SURFACE.  Here a node
keeps KinectFusion's pair instead: D, the truncated signed distance along the optical axis averaged over the views with
weights, and W, the accumulated weight (integrate).  The sign of D and a threshold on W give carve's three states (states), so
that fusion.distance_transform, segmentation.label_components and component_states take them as they are, and near the
surface the distance transform's value is replaced by D, blended over the truncation (blend): the zero level of the result
is the TSDF's, between the nodes, and everything further away is the distance transform's bit for bit.

Volumes, views, view_range, state_begin, the depth [V,H,W] layout and the nodes' points are fusion.py's.  The pair of node L of
volume m sits at state_begin[m] + L of two float32 arrays, tsdf and weight.  Everything is float64, every operation rounded on
its own, dot products written ((a*x + b*y) + c*z) + d, with + - * /, floor and comparisons only; the pair is rounded to float32
once, after the last view of a call.  Not part of the contract: along-ray distances, bilinear depth lookup, colour, noise
models beyond the per-view weights.
"""
from __future__ import annotations

import numpy as np

from . import fusion as _fu
from . import scenes as _sc
from .fusion import FREE, SURFACE, UNKNOWN, node_points, state_offsets, view_rows  # noqa: F401  (the same layout, by import)

INF = float("inf")


def _positive(name: str, x, may_be_inf: bool = False) -> float:
    x = float(x)
    if not (x > 0.0) or not (np.isfinite(x) or (may_be_inf and x == INF)):
        raise ValueError(f"{name} must be positive and finite{' (or +inf)' if may_be_inf else ''}, got {x}")
    return x


def view_updates(view, image, p, trunc: float, near: float):
    """What one view says about the points p [N,3] -> (updates [N] bool, t [N] float64).  The projection, the pixel and the depth
    d are fusion.view_says's, operation for operation: nothing if !(z > near), if the pixel is outside the image or if !(d > 0).
    Then s = d - z: nothing if !(s >= -trunc) (the node lies behind the surface by more than the truncation), otherwise
    t = s < trunc ? s : trunc (a depth of +inf gives trunc: background frees, as it does in carve)."""
    H, W = image.shape
    x, y, zc = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        q = [((view[4 + 4 * k] * x + view[5 + 4 * k] * y) + view[6 + 4 * k] * zc) + view[7 + 4 * k] for k in range(3)]
        z = q[2]
        cf = np.floor((view[0] * (q[0] / z) + view[2]) + 0.5)
        rf = np.floor((view[1] * (q[1] / z) + view[3]) + 0.5)
        seen = (z > near) & (cf >= 0.0) & (cf <= float(W - 1)) & (rf >= 0.0) & (rf <= float(H - 1))
        c, r = np.where(seen, cf, 0.0).astype(np.int64), np.where(seen, rf, 0.0).astype(np.int64)
        d = image[r, c]
        seen = seen & (d > 0.0)
        s = d - z
        return seen & (s >= -trunc), np.where(s < trunc, s, trunc)


def integrate(volumes, views, view_range, depth, trunc: float, near: float, weights=None, wmax: float = INF, tsdf=None, weight=None,
              state_begin=None):
    """The pairs (D, W) of the nodes of M volumes after V depth views -> (tsdf, weight) float32, volume m's node L at
    state_begin[m] + L (default: back to back, fusion.state_offsets).  A node starts from (0, 0), or with tsdf / weight (what an
    earlier call returned: merge) from the stored pair widened to float64, (0, 0) if !(W > 0).  Volume m's views
    view_range[m][0] .. + view_range[m][1] are applied in order; a view that updates (view_updates) with the weight
    w = weights[v] (1.0 without weights; a view with !(w > 0) says nothing) gives
        Wn = W + w,   D = (W*D + w*t) / Wn,   W = Wn < wmax ? Wn : wmax,
    and after the last view the pair is rounded to float32 once.  Elements outside every volume's range keep what they hold
    (zeros without merge).  Two calls (A, then B with merge) round in between, so they equal one call over A + B to float32
    rounding only, not bit for bit."""
    vols = _fu._volumes(volumes)
    views = np.asarray(views, np.float64).reshape(-1, 16)
    depth = np.asarray(depth, np.float64)
    depth = depth.reshape((-1,) + depth.shape[-2:]) if depth.ndim >= 2 else depth.reshape(0, 1, 1)
    view_range = np.asarray(view_range, np.int64).reshape(-1, 2)
    trunc, wmax, near = _positive("trunc", trunc), _positive("wmax", wmax, True), float(near)
    if not np.isfinite(near):
        raise ValueError("near must be finite")
    if not np.isfinite(views).all() or (views[:, :2] == 0).any():
        raise ValueError("a view is not finite or has a focal length of zero")
    if len(depth) != len(views) or len(view_range) != len(vols):
        raise ValueError(f"{len(views)} views need as many images and {len(vols)} volumes as many view ranges")
    if (view_range < 0).any() or (view_range.sum(1) > len(views)).any():
        raise ValueError(f"a view range leaves [0, {len(views)}]")
    w = np.ones(len(views)) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    if len(w) != len(views) or not np.isfinite(w).all() or (w < 0).any():
        raise ValueError(f"weights must be {len(views)} finite numbers >= 0")
    if (tsdf is None) != (weight is None):
        raise ValueError("merge needs both tsdf and weight")
    begin = state_offsets(volumes) if state_begin is None else np.asarray(state_begin, np.int64).reshape(-1)
    sizes = [int(np.prod(v[3])) for v in vols]
    need = max([int(begin[m]) + sizes[m] for m in range(len(vols))], default=0)
    merge = tsdf is not None
    out_d = np.array(tsdf, np.float32).reshape(-1) if merge else np.zeros(need, np.float32)
    out_w = np.array(weight, np.float32).reshape(-1) if merge else np.zeros(need, np.float32)
    if len(out_d) != len(out_w) or len(out_d) < need or (len(vols) and min(int(b) for b in begin[: len(vols)]) < 0):
        raise ValueError(f"tsdf and weight need {need} elements each from offsets >= 0")
    for m, (origin, delta, offset, dims) in enumerate(vols):
        at = slice(int(begin[m]), int(begin[m]) + sizes[m])
        D, W = out_d[at].astype(np.float64), out_w[at].astype(np.float64)
        live = W > 0.0
        D, W = np.where(live, D, 0.0), np.where(live, W, 0.0)
        p = node_points(origin, delta, offset, dims)
        for v in range(int(view_range[m, 0]), int(view_range[m, 0] + view_range[m, 1])):
            if not (w[v] > 0.0):
                continue
            upd, t = view_updates(views[v], depth[v], p, trunc, near)
            with np.errstate(all="ignore"):
                Wn = W + w[v]
                D = np.where(upd, (W * D + w[v] * t) / Wn, D)
                W = np.where(upd, np.where(Wn < wmax, Wn, wmax), W)
        out_d[at], out_w[at] = D.astype(np.float32), W.astype(np.float32)
    return out_d, out_w


def states(tsdf, weight, min_weight: float = 1.0) -> np.ndarray:
    """Carve's state bytes from the pairs, compared in float32: UNKNOWN (2) if !(W >= min_weight), else SURFACE (1) if D < 0,
    else FREE (0).  A NaN weight is unknown, a NaN distance with enough weight is free.  The layout is the pairs', so it is
    carve's: fusion.distance_transform, segmentation.label_components and component_states take the result as it is."""
    mw = np.float32(_positive("min_weight", min_weight))
    D, W = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(~(W >= mw), UNKNOWN, np.where(D < np.float32(0.0), SURFACE, FREE)).astype(np.uint8)


def blend(volume, tsdf, weight, trunc: float, min_weight: float = 1.0) -> np.ndarray:
    """The distance transform's values E (`volume`, float32: what fusion.distance_transform made of states(...)) with the TSDF
    blended in near the surface -> float32 of volume's shape.  Per node with W >= min_weight (float32): D and E widened to
    float64, a = |D| / trunc, out = a >= 1.0 ? E : D + a * (E - D), rounded once; every other node keeps E.
      - Where the TSDF is saturated (|D| >= trunc) or unobserved, the volume is the distance transform's bit for bit.
      - out has the sign of D wherever W >= min_weight and D != 0: a FREE node has E >= delta/2 and an occupied one
        E <= -delta/2, so out lies between D and E on D's side of zero, and the zero level of the result is the TSDF's.
      - |out - E| <= (1 - a) * |E - D| (out - E = (1 - a) * (D - E) before rounding): the correction fades out towards the
        truncation, where the result joins the distance transform continuously."""
    trunc, mw = _positive("trunc", trunc), np.float32(_positive("min_weight", min_weight))
    E32 = np.asarray(volume, np.float32)
    D32, W = np.asarray(tsdf, np.float32).reshape(E32.shape), np.asarray(weight, np.float32).reshape(E32.shape)
    D, E = D32.astype(np.float64), E32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        a = np.abs(D) / trunc
        mixed = np.where(a >= 1.0, E, D + a * (E - D))
        return np.where(W >= mw, mixed, E).astype(np.float32)


def fuse(volumes, views, view_range, depth, trunc: float, near: float, radius: int, unknown_occupied: bool = True, min_weight: float = 1.0,
         weights=None, wmax: float = INF, tsdf=None, weight=None):
    """integrate, states, fusion.distance_transform and blend -> M scenes.SdfGrid (data float32 [X,Y,Z], the volume's origin and
    delta).  tsdf / weight: an earlier integrate's arrays (back to back), merged into."""
    vols = _fu._volumes(volumes)
    _positive("min_weight", min_weight)
    if not 1 <= int(radius) <= _fu.MAX_RADIUS:
        raise ValueError(f"radius must lie in [1, {_fu.MAX_RADIUS}], got {radius}")
    D, W = integrate(volumes, views, view_range, depth, trunc, near, weights, wmax, tsdf, weight)
    E = _fu.distance_transform(states(D, W, min_weight), volumes, radius, unknown_occupied)
    at = state_offsets(volumes)
    return [_sc.SdfGrid(blend(E[m], D[at[m]: at[m + 1]], W[at[m]: at[m + 1]], trunc, min_weight), vols[m][0].copy(), vols[m][1])
            for m in range(len(vols))]
