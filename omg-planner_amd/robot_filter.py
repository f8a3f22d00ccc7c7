"""A robot self-filter: which pixels of a depth image show the arm, and which nodes of an obstacle volume the arm occupies.  The
specification of omgx_render_spheres / omgx_clear_robot (include/omg_hip.h section 22; csrc/omg_robot_filter_body.h follows it
operation by operation) in plain numpy.

A camera beside or on the arm sees the arm.  Fed such an image, fusion carves the arm into the obstacle volume, segmentation
labels it as a component and the support vote counts its pixels.  Here the arm is N padded spheres, each fixed in the frame of
one of the 10 links of omgx_forward_kinematics (link_poses [C,10,4,4], center_offset applied: the frame of
PandaModel.collision_points).  The spheres are moved into every camera's frame (camera_spheres) and ray-cast (render_spheres:
the nearest entry depth per pixel).  A pixel whose depth is at or behind that entry (explained) shows the arm, or something the
arm hides: it is set to 0.0, which every reader of a depth image takes as "no information" (filter_depth; +inf would carve the
whole ray free, and behind the arm the space is occluded, not free).  clear_states then frees, in the states that
fusion.carve_views or tsdf.tsdf_states wrote, the nodes inside a sphere and the unknown nodes between the camera and the arm.

Everything is float64, every operation rounded on its own, dot products written (a*x + b*y) + c*z, with + - * /, sqrt,
comparisons and float-to-int conversion only, so that the device can equal the bits.  Rejections are negated comparisons: NaN
falls on the "no" side.  Not part of the contract: link meshes and capsules, the arm's shadow on the scene, exit depths (space
behind the arm stays UNKNOWN), self-collision, attached objects, other chains than the 10 links.
"""
from __future__ import annotations

import numpy as np

from . import fusion as _fu

NUM_LINKS = 10


def _spheres(local, link):
    local, link = np.asarray(local, np.float64).reshape(-1, 4), np.asarray(link, np.int64).reshape(-1)
    if len(link) != len(local):
        raise ValueError(f"{len(local)} spheres need as many links, got {len(link)}")
    if not np.isfinite(local).all() or (local[:, 3] < 0).any():
        raise ValueError("a sphere is not finite or has a negative radius")
    if len(link) and (link.min() < 0 or link.max() >= NUM_LINKS):
        raise ValueError(f"a sphere's link leaves [0, {NUM_LINKS - 1}]")
    return local, link


def _cameras(cameras):
    from . import camera as _cam
    cameras = np.asarray(cameras)
    if cameras.dtype != _cam.CAMERA_DTYPE:
        raise ValueError("cameras must be camera.CAMERA_DTYPE records")
    cameras = cameras.reshape(-1)
    k = np.stack([cameras[n] for n in ("fx", "fy", "cx", "cy")], -1).reshape(-1, 4)
    _cam.check_camera_rows(np.concatenate([k, cameras["world_from_cam"].reshape(-1, 12)], 1))
    return cameras, k


def camera_spheres(link_poses, local, link, cameras, config_of_view, pad: float) -> np.ndarray:
    """The spheres in every view's camera frame -> [V,N,4]: centre and padded radius.  link_poses [C,10,4,4]; local [N,4]: a
    centre in the frame of link[n] and a radius (finite, >= 0); cameras: V camera.CAMERA_DTYPE records (the intrinsics and
    world_from_cam = (R, t) are read); config_of_view [V] in 0..C-1; pad finite, >= 0.  With P = link_poses[config, link]:
    w_k = ((P[k,0]*p0 + P[k,1]*p1) + P[k,2]*p2) + P[k,3];  u = w - t;  c_k = (R[0,k]*u0 + R[1,k]*u1) + R[2,k]*u2;  r + pad."""
    local, link = _spheres(local, link)
    cameras, _ = _cameras(cameras)
    poses = np.asarray(link_poses, np.float64)
    if poses.ndim != 4 or poses.shape[1:] != (NUM_LINKS, 4, 4):
        raise ValueError(f"link_poses must be [C,{NUM_LINKS},4,4], got {poses.shape}")
    if not np.isfinite(poses).all():
        raise ValueError("a link pose is not finite")
    cfg = np.asarray(config_of_view, np.int64).reshape(-1)
    if len(cfg) != len(cameras):
        raise ValueError(f"{len(cameras)} views need as many configurations, got {len(cfg)}")
    if len(cfg) and (cfg.min() < 0 or cfg.max() >= len(poses)):
        raise ValueError(f"a view's configuration leaves [0, {len(poses) - 1}]")
    pad = float(pad)
    if not (np.isfinite(pad) and pad >= 0):
        raise ValueError("pad must be finite and not negative")
    out = np.zeros((len(cameras), len(local), 4))
    p = local[:, :3]
    for v in range(len(cameras)):
        P = poses[cfg[v], link]  # [N,4,4]
        w = [((P[:, k, 0] * p[:, 0] + P[:, k, 1] * p[:, 1]) + P[:, k, 2] * p[:, 2]) + P[:, k, 3] for k in range(3)]
        m = cameras["world_from_cam"][v].reshape(3, 4)
        u = [w[k] - m[k, 3] for k in range(3)]
        for k in range(3):
            out[v, :, k] = (m[0, k] * u[0] + m[1, k] * u[1]) + m[2, k] * u[2]
        out[v, :, 3] = local[:, 3] + pad
    return out


def _cam_spheres(cam_spheres, V):
    s = np.asarray(cam_spheres, np.float64)
    if s.ndim != 3 or s.shape[2] != 4 or len(s) != V:
        raise ValueError(f"cam_spheres must be [{V},N,4], got {s.shape}")
    if not np.isfinite(s).all() or (s[:, :, 3] < 0).any():
        raise ValueError("a sphere is not finite or has a negative radius")
    return s


def render_spheres(cam_spheres, cameras, H: int, W: int, t_min: float = 1e-6):
    """The nearest sphere per pixel -> (t_near [V,H,W] float64, +inf on a miss; sphere [V,H,W] int32, -1 on a miss).  Pixel (r, c)
    is camera.py's ray: dx = (c - cx) / fx, dy = (r - cy) / fy, dz = 1, so t is depth along the axis.  Per sphere (x, y, z, R):
    dd = (dx*dx + dy*dy) + 1;  b = (x*dx + y*dy) + z;  q = ((x*x + y*y) + z*z) - R*R;  disc = b*b - q*dd;  a miss if
    !(disc >= 0);  s = sqrt(disc), t0 = (b - s) / dd, t1 = (b + s) / dd;  a miss if !(t1 > t_min);  the entry is t0 if
    t0 > t_min, else t_min (a camera inside a sphere sees it at t_min).  The smallest entry wins, the lowest index on a tie."""
    cameras, k = _cameras(cameras)
    V, H, W, t_min = len(cameras), int(H), int(W), float(t_min)
    if H < 1 or W < 1:
        raise ValueError(f"H and W must be >= 1, got {H} and {W}")
    if not (np.isfinite(t_min) and t_min >= 0):
        raise ValueError("t_min must be finite and not negative")
    s = _cam_spheres(cam_spheres, V)
    t_near, which = np.full((V, H, W), np.inf), np.full((V, H, W), -1, np.int32)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        for v in range(V):
            dx, dy = (c - k[v, 2]) / k[v, 0], (r - k[v, 3]) / k[v, 1]
            dd = (dx * dx + dy * dy) + 1.0
            for n, (x, y, z, R) in enumerate(s[v]):
                b = (x * dx + y * dy) + z
                q = ((x * x + y * y) + z * z) - R * R
                disc = b * b - q * dd
                hit = disc >= 0.0
                root = np.sqrt(np.where(hit, disc, 0.0))
                t0, t1 = (b - root) / dd, (b + root) / dd
                hit = hit & (t1 > t_min)
                entry = np.where(t0 > t_min, t0, t_min)
                take = hit & (entry < t_near[v])
                t_near[v] = np.where(take, entry, t_near[v])
                which[v] = np.where(take, np.int32(n), which[v])
    return t_near, which


def explained(depth, t_near, tol: float) -> np.ndarray:
    """The pixels the arm explains: t_near < inf and depth >= t_near - tol.  A NaN depth is not explained, +inf (background
    behind the arm) is; a surface in front of the arm by more than tol is not."""
    with np.errstate(all="ignore"):
        return (np.asarray(t_near) < np.inf) & (np.asarray(depth) >= np.asarray(t_near) - float(tol))


def filter_depth(depth, t_near, tol: float) -> np.ndarray:
    """A copy of depth with the explained pixels set to 0.0: no information."""
    return np.where(explained(depth, t_near, tol), 0.0, np.asarray(depth, np.float64))


def view_clears(view, image, t_image, spheres, p, near: float, tol: float):
    """What one view says about the points p [N,3] -> (inside [N], front [N]) bool.  q = cam_from_grid p and the pixel (r, c) are
    fusion.view_says's; seen = z > near and the pixel is inside the image.  inside: ((q0-x)^2 + (q1-y)^2) + (q2-z)^2 <= R*R for
    some sphere (x, y, z, R) of `spheres`, whether seen or not.  front: seen, the pixel is explained, and z < t_image[r, c]."""
    H, W = image.shape
    x, y, zc = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        q = [((view[4 + 4 * k] * x + view[5 + 4 * k] * y) + view[6 + 4 * k] * zc) + view[7 + 4 * k] for k in range(3)]
        z = q[2]
        cf = np.floor((view[0] * (q[0] / z) + view[2]) + 0.5)
        rf = np.floor((view[1] * (q[1] / z) + view[3]) + 0.5)
        seen = (z > near) & (cf >= 0.0) & (cf <= float(W - 1)) & (rf >= 0.0) & (rf <= float(H - 1))
        c, r = np.where(seen, cf, 0.0).astype(np.int64), np.where(seen, rf, 0.0).astype(np.int64)
        tn = t_image[r, c]
        front = seen & explained(image[r, c], tn, tol) & (z < tn)
        inside = np.zeros(len(p), bool)
        for sx, sy, sz, R in spheres:
            e0, e1, e2 = q[0] - sx, q[1] - sy, q[2] - sz
            inside |= ((e0 * e0 + e1 * e1) + e2 * e2) <= R * R
    return inside, front


def clear_states(state, volumes, views, view_range, depth, near: float, t_near, cam_spheres, tol: float, state_begin=None) -> np.ndarray:
    """The states with the arm taken out -> a new uint8 array.  state, volumes, views, view_range and state_begin are
    fusion.carve_views's own (the layout and the projection are exactly view_says's); depth, t_near [V,H,W] and cam_spheres
    [V,N,4] belong to the views.  For the node of volume m at p, over the views of the volume's range (view_clears): FREE if
    inside held in any view; otherwise FREE if the old state is UNKNOWN and front held in any view; otherwise the old byte.
    A SURFACE node in front of the arm stays (another view saw it: surface wins, as in carve); a SURFACE or UNKNOWN node inside
    a sphere becomes FREE.  Bytes outside every volume's range are untouched."""
    vols = _fu._volumes(volumes)
    views = np.asarray(views, np.float64).reshape(-1, 16)
    V = len(views)
    depth, t_near = np.asarray(depth, np.float64), np.asarray(t_near, np.float64)
    if depth.ndim != 3 or t_near.ndim != 3 or len(depth) != V or len(t_near) != V:
        raise ValueError(f"{V} views need as many images and as many images of the arm")
    if depth.shape != t_near.shape:
        raise ValueError(f"the images {depth.shape[1:]} and the images of the arm {t_near.shape[1:]} differ in size")
    spheres = _cam_spheres(cam_spheres, V)
    view_range = np.asarray(view_range, np.int64).reshape(-1, 2)
    near, tol = float(near), float(tol)
    if not (np.isfinite(near) and np.isfinite(tol)):
        raise ValueError("near and tol must be finite")
    if not np.isfinite(views).all() or (views[:, :2] == 0).any():
        raise ValueError("a view is not finite or has a focal length of zero")
    if len(view_range) != len(vols):
        raise ValueError(f"{len(vols)} volumes need as many view ranges")
    if (view_range < 0).any() or (view_range.sum(1) > V).any():
        raise ValueError(f"a view range leaves [0, {V}]")
    begin = _fu.state_offsets(volumes) if state_begin is None else np.asarray(state_begin, np.int64).reshape(-1)
    sizes = [int(np.prod(v[3])) for v in vols]
    need = max([int(begin[m]) + sizes[m] for m in range(len(vols))], default=0)
    out = np.array(state, np.uint8).reshape(-1)
    if len(out) < need or (len(vols) and min(int(b) for b in begin[: len(vols)]) < 0):
        raise ValueError(f"the states need {need} elements from offsets >= 0")
    for m, (origin, delta, offset, dims) in enumerate(vols):
        mine = out[int(begin[m]): int(begin[m]) + sizes[m]]
        p = _fu.node_points(origin, delta, offset, dims)
        inside, front = np.zeros(sizes[m], bool), np.zeros(sizes[m], bool)
        for v in range(int(view_range[m, 0]), int(view_range[m, 0] + view_range[m, 1])):
            i, f = view_clears(views[v], depth[v], t_near[v], spheres[v], p, near, tol)
            inside, front = inside | i, front | f
        mine[:] = np.where(inside | ((mine == _fu.UNKNOWN) & front), _fu.FREE, mine)
    return out
