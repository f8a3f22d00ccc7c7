"""Depth fusion: depth views to signed obstacle volumes.  The specification of omgx_carve_views / omgx_distance_transform
(include/omg_hip.h section 17; csrc/omg_fusion_body.h follows it operation by operation) in plain numpy.

The reference's obstacle volume from observation (PointEnv.compute_sdf_from_points, omg/core.py:426-457; here
ops.point_cloud_sdf) is unsigned, reads space no camera has seen as free, and tests every node against every point.  Here the
nodes of M volumes are classified FREE, SURFACE or UNKNOWN from V depth images (carve_views), and an exact Euclidean distance
transform of that classification is the signed float32 volume (distance_transform): the zero level lies on the faces between
occupied and free voxels, unknown space can count as occupied, and the cost does not depend on the number of pixels.

A volume is (origin [3], delta, "centre" or "node", dims [3][, ...]) as ops.surface_records takes it; node (i,j,k) has the linear
index L = (i * dims[1] + j) * dims[2] + k (x-major, as the SDF pool).  A view is one row of 16 doubles: fx, fy, cx, cy and the
rows of cam_from_grid [3,4] (view_rows); the camera convention is camera.py's: optical axis +z, rows downwards, depth along
the axis.  View v reads image v of depth [V,H,W] float64, the layout camera.render_depth writes, +inf as background.

Everything is float64, every operation rounded on its own, dot products written ((a*x + b*y) + c*z) + d, with + - * /, floor
and sqrt only, so that the device can equal the bits.  Distances are to voxel centres: the fused value is at most
(sqrt(3)/2) * delta coarser than the distance to the true surface points (plus the band on the free side).  Not part of the
contract: sub-voxel surfaces, weighted averaging and sensor noise (tsdf.py adds them on these states and volumes), colour.
"""
from __future__ import annotations

import numpy as np

from . import scenes as _sc

FREE, SURFACE, UNKNOWN = 0, 1, 2
MAX_RADIUS = 255  # radius^2 fits the 16 bits of a channel


def view_rows(intrinsics, cam_from_grid) -> np.ndarray:
    """One row of `views` [16]: fx, fy, cx, cy and the rows of cam_from_grid [3,4] (a [4,4] or [3,4] matrix: the camera's
    cam_from_world times the pose of the grid's frame in the world).  How the host multiplies or inverts matrices to get there is
    not part of the contract, which starts at the row."""
    k = np.asarray(intrinsics, np.float64).reshape(4)
    m = np.asarray(cam_from_grid, np.float64)
    return np.concatenate([k, m.reshape(-1, 4)[:3].ravel()])


def _volumes(volumes):
    out = []
    for m, v in enumerate(volumes):
        origin, delta, sample, dims = v[0], v[1], v[2], v[3]
        if sample not in _sc.MESH_SAMPLE_OFFSET:
            raise ValueError(f"volume {m}: sample must be 'centre' or 'node', got {sample!r}")
        origin, dims = np.asarray(origin, np.float64).reshape(-1), tuple(int(d) for d in np.asarray(dims).reshape(-1))
        if len(origin) != 3 or len(dims) != 3 or min(dims) < 1 or not np.isfinite(origin).all() or not (float(delta) > 0 and np.isfinite(float(delta))):
            raise ValueError(f"volume {m}: origin [3] finite, delta positive and finite, three dims >= 1; got {origin}, {delta}, {dims}")
        out.append((origin, float(delta), _sc.MESH_SAMPLE_OFFSET[sample], dims))
    return out


def state_offsets(volumes) -> np.ndarray:
    """state_begin [M] int64 of the volumes' states laid back to back, and their total as element M."""
    n = [int(np.prod([int(d) for d in np.asarray(v[3]).reshape(-1)])) for v in volumes]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def node_points(origin, delta, offset, dims):
    """p [N,3] of the nodes in x-major order: origin + ((i,j,k) + offset) * delta, per component."""
    idx = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    return origin + (idx + offset) * delta


def view_says(view, image, p, band: float, near: float):
    """What one view says about the points p [N,3] -> (free [N], surface [N]) bool.  q = cam_from_grid p, z = q[2]; no
    information if !(z > near), or the pixel c = floor((fx*(q0/z) + cx) + 0.5), r = floor((fy*(q1/z) + cy) + 0.5) is outside the
    image, or !(d > 0) with d = image[r, c]; otherwise free if z < d - band, surface if d - band <= z <= d + band."""
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
        lo, hi = d - band, d + band
        return seen & (z < lo), seen & (lo <= z) & (z <= hi)


def carve_views(volumes, views, view_range, depth, band: float, near: float, state=None, state_begin=None) -> np.ndarray:
    """The states of the nodes of M volumes from V depth views -> uint8, volume m's node L at state_begin[m] + L (default: back
    to back, state_offsets).  Volume m runs over the views view_range[m][0] .. + view_range[m][1] in order (ranges of two volumes
    may overlap): SURFACE if any view says surface, otherwise FREE if any says free, otherwise UNKNOWN.  state: what an earlier
    call returned (merge): the flags start from it, 1 as surface and 0 as free, so that carving the views A and merging the
    views B equals carving A and B together.  Elements outside every volume's range keep what `state` holds (UNKNOWN without)."""
    vols = _volumes(volumes)
    views = np.asarray(views, np.float64).reshape(-1, 16)
    depth = np.asarray(depth, np.float64)
    depth = depth.reshape((-1,) + depth.shape[-2:]) if depth.ndim >= 2 else depth.reshape(0, 1, 1)
    view_range = np.asarray(view_range, np.int64).reshape(-1, 2)
    band, near = float(band), float(near)
    if not (np.isfinite(band) and np.isfinite(near)):
        raise ValueError("band and near must be finite")
    if not np.isfinite(views).all() or (views[:, :2] == 0).any():
        raise ValueError("a view is not finite or has a focal length of zero")
    if len(depth) != len(views) or len(view_range) != len(vols):
        raise ValueError(f"{len(views)} views need as many images and {len(vols)} volumes as many view ranges")
    if (view_range < 0).any() or (view_range.sum(1) > len(views)).any():
        raise ValueError(f"a view range leaves [0, {len(views)}]")
    begin = state_offsets(volumes) if state_begin is None else np.asarray(state_begin, np.int64).reshape(-1)
    sizes = [int(np.prod(v[3])) for v in vols]
    need = max([int(begin[m]) + sizes[m] for m in range(len(vols))], default=0)
    out = np.full(need, UNKNOWN, np.uint8) if state is None else np.array(state, np.uint8).reshape(-1)
    if len(out) < need or (len(vols) and min(int(b) for b in begin[: len(vols)]) < 0):
        raise ValueError(f"the states need {need} elements from offsets >= 0")
    for m, (origin, delta, offset, dims) in enumerate(vols):
        mine = out[int(begin[m]): int(begin[m]) + sizes[m]]
        surface, free = (mine == SURFACE, mine == FREE) if state is not None else (np.zeros(sizes[m], bool), np.zeros(sizes[m], bool))
        p = node_points(origin, delta, offset, dims)
        for v in range(int(view_range[m, 0]), int(view_range[m, 0] + view_range[m, 1])):
            f, s = view_says(views[v], depth[v], p, band, near)
            surface, free = surface | s, free | f
        mine[:] = np.where(surface, SURFACE, np.where(free, FREE, UNKNOWN))
    return out


def occupied(state, unknown_occupied: bool) -> np.ndarray:
    """A node is occupied if its state is 1, or if it is neither 0 nor 1 and unknown_occupied is set; every other node is free."""
    state = np.asarray(state)
    return (state == SURFACE) | ((state != FREE) & bool(unknown_occupied))


def _line_pass(g: np.ndarray, axis: int, radius: int, r2: int) -> np.ndarray:
    """min over |d| <= radius, inside the grid, of g shifted by d along `axis` + d*d, saturated at r2."""
    n = g.shape[axis]
    out = np.minimum(g, r2)
    for d in range(1, min(radius, n - 1) + 1):
        near_, far_ = [slice(None)] * 3, [slice(None)] * 3
        near_[axis], far_[axis] = slice(0, n - d), slice(d, n)
        near_, far_ = tuple(near_), tuple(far_)
        out[near_] = np.minimum(out[near_], g[far_] + d * d)
        out[far_] = np.minimum(out[far_], g[near_] + d * d)
    return out


def squared_distances(mask, radius: int) -> np.ndarray:
    """d2(p, X) = min(radius^2, min over the nodes q of X = {mask} of |p - q|^2) in index units for every node p of the grid
    [X,Y,Z] -> int64: three windowed passes of +-radius along z, y, x, saturated at radius^2 after each (which keeps the result
    exact: a term that saturates could only have given radius^2 or more)."""
    r2 = int(radius) * int(radius)
    g = np.where(np.asarray(mask, bool), 0, r2).astype(np.int64)
    for axis in (2, 1, 0):
        g = _line_pass(g, axis, int(radius), r2)
    return g


def signed_volume(state, delta: float, radius: int, unknown_occupied: bool) -> np.ndarray:
    """One volume's states [X,Y,Z] -> float32 [X,Y,Z]:
    occupied ? -((sqrt(d2(p, free)) - 0.5) * delta) : (sqrt(d2(p, occupied)) - 0.5) * delta, in float64, rounded once."""
    occ = occupied(state, unknown_occupied)
    to_occ, to_free = squared_distances(occ, radius), squared_distances(~occ, radius)
    inside, outside = -((np.sqrt(to_free.astype(np.float64)) - 0.5) * float(delta)), (np.sqrt(to_occ.astype(np.float64)) - 0.5) * float(delta)
    return np.where(occ, inside, outside).astype(np.float32)


def distance_transform(state, volumes, radius: int, unknown_occupied: bool = True, state_begin=None):
    """The signed float32 volumes [X,Y,Z] of M volumes' states (carve_views' array and offsets) -> a list of M arrays.
    Distances saturate at (radius - 0.5) * delta; a volume with no occupied node, or with no free node, is constant."""
    radius = int(radius)
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must lie in [1, {MAX_RADIUS}], got {radius}")
    vols = _volumes(volumes)
    state = np.asarray(state, np.uint8).reshape(-1)
    begin = state_offsets(volumes) if state_begin is None else np.asarray(state_begin, np.int64).reshape(-1)
    out = []
    for m, (origin, delta, offset, dims) in enumerate(vols):
        n = int(np.prod(dims))
        if begin[m] < 0 or begin[m] + n > len(state):
            raise ValueError(f"volume {m}: its states [{begin[m]}, {begin[m] + n}) leave the {len(state)} given")
        out.append(signed_volume(state[int(begin[m]): int(begin[m]) + n].reshape(dims), delta, radius, unknown_occupied))
    return out


def obstacle_radius(reach: float, delta: float) -> int:
    """The radius at which the saturation lies beyond `reach` (epsilon + clearance of the cost): ceil(reach / delta + 0.5) + 1."""
    return int(np.ceil(float(reach) / float(delta) + 0.5)) + 1


def fuse_views(volumes, views, view_range, depth, band: float, near: float, radius: int, unknown_occupied: bool = True):
    """carve_views, then distance_transform -> M scenes.SdfGrid (data float32 [X,Y,Z], the volume's origin and delta)."""
    vols = _volumes(volumes)
    data = distance_transform(carve_views(volumes, views, view_range, depth, band, near), volumes, radius, unknown_occupied)
    return [_sc.SdfGrid(data[m], vols[m][0].copy(), vols[m][1]) for m in range(len(vols))]
