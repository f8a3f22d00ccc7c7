"""Support-plane fitting: depth views to the plane of an unknown support, the free mask that takes it out before carving, and the
half-space volume that puts it back as an obstacle.  The specification of omgx_plane_ransac / omgx_plane_moments /
omgx_plane_mask / omgx_plane_volumes (include/omg_hip.h section 19; csrc/omg_plane_body.h holds the per-pixel and per-hypothesis
rules) in plain numpy.

Objects standing on a table are one connected component with it, so segmentation.segment_views needs the table's pixels masked
out; camera.explained_mask gets them from a rendering of a table that is already known.  Here the dominant plane of every depth
view is found by RANSAC over pixel triples that the host draws, refined by a least-squares fit to its inliers, and the pixels
on or behind it are the mask.

Everything is in the camera frame of its view, the camera convention is camera.py's: pixel (r, c) with depth d is the point
p = (d*dx, d*dy, d), dx = (c - cx) / fx, dy = (r - cy) / fy.  A plane is (n0, n1, n2, off): n.p + off = 0, |n| = 1, off >= 0, so
that the normal faces the camera and the residual r = ((n0*x + n1*y) + n2*z) + off is positive on the camera's side.

Everything specified is float64, every operation rounded on its own, dot products written ((a*x + b*y) + c*z) + d, with
+ - * /, sqrt and comparisons only, so that the device can equal the bits.  refine_plane (an eigenvector) and the helpers
draw_triples and plane_to_frame run on the host in both paths and are not part of the bit contract.  Not part of the contract:
curved supports, several supports at once, weighted fits, sensor noise models.
"""
from __future__ import annotations

import numpy as np

from . import fusion as _fu
from .registration import THREADS, _tree

PIXELS_PER_WORKGROUP = 2048  # OMGX_PLANE_PIXELS_PER_WORKGROUP (the tests assert that it is the header's)
NO_PLANE, RANSAC_ONLY, REFINED = 0, 1, 2  # fit_planes' status of a view
SUMS = ("q0", "q1", "q2", "q0q0", "q0q1", "q0q2", "q1q1", "q1q2", "q2q2")


def _images(intrinsics, depth, skip):
    depth = np.asarray(depth, np.float64)
    if depth.ndim != 3:
        raise ValueError("depth must be [V,H,W]")
    V = depth.shape[0]
    k = np.asarray(intrinsics, np.float64)
    k = np.broadcast_to(k, (V, 4)) if k.ndim == 1 else k.reshape(-1, 4)
    if len(k) != V or not np.isfinite(k).all() or (k[:, :2] == 0).any():
        raise ValueError(f"intrinsics must be [{V},4] (fx, fy, cx, cy), finite, the focal lengths not zero")
    if skip is not None:
        skip = np.asarray(skip)
        if skip.shape != depth.shape:
            raise ValueError("skip must have depth's shape")
        skip = skip.astype(bool)
    return np.ascontiguousarray(k), depth, skip


def _scalars(tol=0.0, min_nn=0.0, cos_min=-1.0):
    tol, min_nn, cos_min = float(tol), float(min_nn), float(cos_min)
    if not (np.isfinite(tol) and tol >= 0 and np.isfinite(min_nn) and min_nn >= 0):
        raise ValueError("tol and min_nn must be finite and not negative")
    if not -1.0 <= cos_min <= 1.0:
        raise ValueError("cos_min must lie in [-1, 1]")
    return tol, min_nn, cos_min


def pixel_points(intrinsics, depth, skip=None):
    """(p [V,H*W,3], valid [V,H*W]) of the pixels in row-major order.  Pixel (r, c) is valid if d > 0, d < +inf (NaN fails both)
    and skip is not set there; p = (d*dx, d*dy, d) with camera.pixel_directions' dx = (c - cx) / fx, dy = (r - cy) / fy."""
    k, depth, skip = _images(intrinsics, depth, skip)
    V, H, W = depth.shape
    r, c = np.divmod(np.arange(H * W, dtype=np.int64), W)
    d = depth.reshape(V, H * W)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (d > 0.0) & (d < np.inf)
        if skip is not None:
            valid &= ~skip.reshape(V, H * W)
        dx = (c.astype(np.float64)[None] - k[:, 2:3]) / k[:, 0:1]
        dy = (r.astype(np.float64)[None] - k[:, 3:4]) / k[:, 1:2]
        return np.stack([d * dx, d * dy, d], -1), valid


def _triples(triples, V, pixels):
    t = np.asarray(triples)
    if t.ndim != 3 or t.shape[0] != V or t.shape[2] != 3 or t.shape[1] < 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"triples must be integers [{V},K,3] with K >= 1")
    if V and (t.min() < 0 or t.max() >= pixels):
        raise ValueError(f"a triple names a pixel outside [0, {pixels})")
    return np.ascontiguousarray(t, np.int32)


def _up(up, V):
    if up is None:
        return None
    up = np.asarray(up, np.float64)
    up = np.broadcast_to(up, (V, 3)) if up.ndim == 1 else up.reshape(-1, 3)
    if len(up) != V or not np.isfinite(up).all():
        raise ValueError(f"up must be [{V},3] and finite")
    return np.ascontiguousarray(up)


def residual(plane, p):
    """r = ((n0*x + n1*y) + n2*z) + off for planes [...,4] and points [...,3] that broadcast."""
    return ((plane[..., 0] * p[..., 0] + plane[..., 1] * p[..., 1]) + plane[..., 2] * p[..., 2]) + plane[..., 3]


def hypotheses(intrinsics, depth, triples, min_nn: float = 0.0, skip=None, up=None, cos_min: float = -1.0):
    """One plane per pixel triple -> (planes [V,K,4], live [V,K] bool); void rows are four zeros.  triples [V,K,3]: row-major
    pixel indices (a, b, c).  With pa, pb, pc the pixels' points:
      1. void if any of the three pixels is invalid
      2. e = pb - pa, f = pc - pa
      3. n = (e1*f2 - e2*f1, e2*f0 - e0*f2, e0*f1 - e1*f0): two rounded products, one subtraction
      4. nn = (n0*n0 + n1*n1) + n2*n2 (four times the squared area of the triangle); void unless nn > min_nn
      5. s = sqrt(nn), n = n / s per component, off = -((n0*a0 + n1*a1) + n2*a2)
      6. if off < 0: n = -n, off = -off (the normal faces the camera)
      7. with up [V,3] given: void unless (n0*u0 + n1*u1) + n2*u2 >= cos_min"""
    _, min_nn, cos_min = _scalars(0.0, min_nn, cos_min)
    p, valid = pixel_points(intrinsics, depth, skip)
    V, N = valid.shape
    t, up = _triples(triples, V, N), _up(up, V)
    v = np.arange(V)[:, None]
    pa, pb, pc = (p[v, t[:, :, x]] for x in range(3))
    live = valid[v, t[:, :, 0]] & valid[v, t[:, :, 1]] & valid[v, t[:, :, 2]]
    with np.errstate(all="ignore"):
        e, f = pb - pa, pc - pa
        n = np.stack([e[..., 1] * f[..., 2] - e[..., 2] * f[..., 1], e[..., 2] * f[..., 0] - e[..., 0] * f[..., 2],
                      e[..., 0] * f[..., 1] - e[..., 1] * f[..., 0]], -1)
        nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        live &= nn > min_nn
        n = n / np.sqrt(nn)[..., None]
        off = -((n[..., 0] * pa[..., 0] + n[..., 1] * pa[..., 1]) + n[..., 2] * pa[..., 2])
        flip = off < 0.0
        n, off = np.where(flip[..., None], -n, n), np.where(flip, -off, off)
        if up is not None:
            u = up[:, None, :]
            live &= ((n[..., 0] * u[..., 0] + n[..., 1] * u[..., 1]) + n[..., 2] * u[..., 2]) >= cos_min
    planes = np.concatenate([n, off[..., None]], -1)
    return np.where(live[..., None], planes, 0.0), live


def score(intrinsics, depth, planes, live, tol: float, skip=None) -> np.ndarray:
    """counts [V,K] int32: per live hypothesis the number of valid pixels with |r| <= tol; -1 for a void row."""
    tol, _, _ = _scalars(tol)
    p, valid = pixel_points(intrinsics, depth, skip)
    planes, live = np.asarray(planes, np.float64), np.asarray(live, bool)
    counts = np.full(live.shape, -1, np.int32)
    with np.errstate(all="ignore"):
        for v, k in zip(*np.nonzero(live)):
            counts[v, k] = int((valid[v] & (np.abs(residual(planes[v, k], p[v])) <= tol)).sum())
    return counts


def select(counts) -> np.ndarray:
    """best [V] int32: the smallest k with the largest count, -1 if every row is void."""
    counts = np.asarray(counts, np.int32)
    best = np.argmax(counts, 1).astype(np.int32) if counts.shape[1] else np.full(len(counts), -1, np.int32)  # (argmax: the first of equals)
    return np.where(counts.max(1, initial=-1) < 0, np.int32(-1), best).astype(np.int32)


def ransac(intrinsics, depth, triples, tol: float, min_nn: float = 0.0, skip=None, up=None, cos_min: float = -1.0):
    """hypotheses, score, select -> (planes [V,K,4], counts [V,K] int32, best [V] int32, best_planes [V,4], anchors [V,3]):
    the best hypothesis' plane and the point pa of its triple; zeros for a view whose best is -1."""
    planes, live = hypotheses(intrinsics, depth, triples, min_nn, skip, up, cos_min)
    counts = score(intrinsics, depth, planes, live, tol, skip)
    best = select(counts)
    p, _ = pixel_points(intrinsics, depth, skip)
    V = len(best)
    t = _triples(triples, V, p.shape[1])
    best_planes, anchors = np.zeros((V, 4)), np.zeros((V, 3))
    for v in np.flatnonzero(best >= 0):
        best_planes[v], anchors[v] = planes[v, best[v]], p[v, t[v, best[v], 0]]
    return planes, counts, best, best_planes, anchors


def has_plane(planes) -> np.ndarray:
    """A row (n, off) is a plane if its normal is not (0, 0, 0): four zeros stand for "no plane"."""
    planes = np.asarray(planes, np.float64)
    return (planes[..., 0] != 0.0) | (planes[..., 1] != 0.0) | (planes[..., 2] != 0.0)


def moments(intrinsics, depth, planes, anchors, tol: float, skip=None):
    """(count [V] int32, sums [V,9]) over the inliers (valid, |r| <= tol) of planes [V,4]: the nine sums SUMS of q = p - anchor
    per component, about anchors [V,3] so that the covariance does not cancel.  A view without a plane (has_plane) has no inlier.

    The shape of the sum: a view's pixels lie in chunks of PIXELS_PER_WORKGROUP; lane l of 256 adds its chunk's pixels l,
    l + 256, ... in order from +0.0 (a pixel that is no inlier adds +0.0); the lanes are summed by registration._tree (inside
    each group of 64 lanes x[l] += x[l + s] for s = 32 ... 1, then the four group totals left to right); the chunk totals of a
    view are added left to right from +0.0."""
    tol, _, _ = _scalars(tol)
    p, valid = pixel_points(intrinsics, depth, skip)
    V, N = valid.shape
    planes, anchors = np.asarray(planes, np.float64).reshape(V, 4), np.asarray(anchors, np.float64).reshape(V, 3)
    count, sums = np.zeros(V, np.int32), np.zeros((V, 9))
    for v in range(V):
        with np.errstate(all="ignore"):
            inl = valid[v] & (np.abs(residual(planes[v], p[v])) <= tol) & bool(has_plane(planes[v]))
            q = [p[v, :, a] - anchors[v, a] for a in range(3)]
            terms = np.stack([q[0], q[1], q[2], q[0] * q[0], q[0] * q[1], q[0] * q[2], q[1] * q[1], q[1] * q[2], q[2] * q[2]], -1)
        terms = np.where(inl[:, None], terms, 0.0)
        count[v] = int(inl.sum())
        total = np.zeros(9)
        for c0 in range(0, N, PIXELS_PER_WORKGROUP):
            chunk = terms[c0: c0 + PIXELS_PER_WORKGROUP]
            rows = -(-len(chunk) // THREADS)
            chunk = np.concatenate([chunk, np.zeros((rows * THREADS - len(chunk), 9))]).reshape(rows, THREADS, 9)
            acc = np.zeros((THREADS, 9))
            for row in chunk:
                acc = acc + row
            total = total + _tree(acc)
        sums[v] = total
    return count, sums


def refine_plane(count, sums, anchor, plane):
    """The least-squares plane of the inliers whose moments are (count, sums) about `anchor` -> (plane [4], refined): the
    centroid anchor + S1 / count, the covariance S2 / count - m m^T, the eigenvector of its smallest eigenvalue (np.linalg.eigh),
    oriented towards the camera (off >= 0).  The input plane comes back, with refined False, when fewer than three inliers or a
    covariance that is not finite or has no two directions of spread (collinear inliers) make the fit meaningless.  On the host
    in every path; not part of the bit contract."""
    plane = np.asarray(plane, np.float64).reshape(4).copy()
    s = np.asarray(sums, np.float64).reshape(9)
    if int(count) < 3 or not np.isfinite(s).all():
        return plane, False
    m = s[:3] / float(count)
    S2 = np.array([[s[3], s[4], s[5]], [s[4], s[6], s[7]], [s[5], s[7], s[8]]]) / float(count)
    cov = S2 - np.outer(m, m)
    w, vec = np.linalg.eigh(cov)
    if not np.isfinite(w).all() or not w[1] > 1e-12 * max(w[2], 0.0) or not w[2] > 0.0:
        return plane, False
    n = vec[:, 0] / np.sqrt(vec[:, 0] @ vec[:, 0])
    off = -float(n @ (np.asarray(anchor, np.float64).reshape(3) + m))
    if off < 0:
        n, off = -n, -off
    return np.array([n[0], n[1], n[2], off]), True


class PlaneFit:
    """What fit_planes returns: planes [V,4] (four zeros without a plane), hypotheses [V,K,4], counts [V,K] int32 (-1: void),
    best [V] int32, ransac_counts [V] (the best hypothesis' count, 0 without), inliers [V] int32 (at the final plane), status [V]
    (NO_PLANE, RANSAC_ONLY, REFINED), anchors [V,3]."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _fit_rounds(best, best_planes, anchors, refine: int, moments_of):
    """The host half of fit_planes, shared with ops.fit_planes: `refine` rounds of (moments at the current planes, refine_plane),
    then the inlier counts at the final planes.  moments_of(planes [V,4]) -> (count [V], sums [V,9]) on the host."""
    refine = int(refine)
    if refine < 0:
        raise ValueError("refine must not be negative")
    planes = np.array(best_planes, np.float64).reshape(-1, 4)
    status = np.where(np.asarray(best) >= 0, RANSAC_ONLY, NO_PLANE).astype(np.int32)
    for _ in range(refine):
        count, sums = moments_of(planes)
        for v in np.flatnonzero(status != NO_PLANE):
            new, ok = refine_plane(count[v], sums[v], anchors[v], planes[v])
            planes[v] = new
            status[v] = REFINED if ok else status[v]
    count, _ = moments_of(planes)
    return planes, np.asarray(count, np.int32).copy(), status


def fit_planes(intrinsics, depth, triples, tol: float, skip=None, up=None, cos_min: float = -1.0, min_nn: float = 1e-10, refine: int = 2) -> PlaneFit:
    """The dominant plane of every view: ransac, then `refine` rounds of moments at the current plane followed by refine_plane,
    then the inliers of the final plane (refine + 1 moment passes) -> PlaneFit.  intrinsics [4] or [V,4], depth [V,H,W], triples
    [V,K,3] (draw_triples); skip: bool [V,H,W], pixels that do not exist for this fit (plane_mask of an earlier fit: the next
    plane); up [3] or [V,3] with cos_min: only hypotheses whose normal has n.up >= cos_min count.  min_nn: the smallest
    4 * area^2 of a triple's triangle (the default is a triangle of 5 mm^2)."""
    planes, counts, best, best_planes, anchors = ransac(intrinsics, depth, triples, tol, min_nn, skip, up, cos_min)
    final, inliers, status = _fit_rounds(best, best_planes, anchors, refine, lambda pl: moments(intrinsics, depth, pl, anchors, tol, skip))
    ransac_counts = np.array([counts[v, best[v]] if best[v] >= 0 else 0 for v in range(len(best))], np.int32)
    return PlaneFit(planes=final, hypotheses=planes, counts=counts, best=best, ransac_counts=ransac_counts, inliers=inliers, status=status,
                    anchors=anchors)


def plane_mask(intrinsics, depth, planes, tol: float, skip=None) -> np.ndarray:
    """bool [V,H,W]: valid and r <= tol, the pixels on the plane or behind it (what segmentation.explained_mask means by
    t >= t_known - tol); a view without a plane (has_plane) gives all False.  As segment_views' free_mask it takes the support
    out before carving; as the skip of another fit it lets the next plane be found."""
    tol, _, _ = _scalars(tol)
    p, valid = pixel_points(intrinsics, depth, skip)
    V, N = valid.shape
    planes = np.asarray(planes, np.float64).reshape(V, 4)
    with np.errstate(all="ignore"):
        mask = valid & (residual(planes[:, None, :], p) <= tol) & has_plane(planes)[:, None]
    return mask.reshape(np.asarray(depth).shape)


def halfspace_volume(volume, plane) -> np.ndarray:
    """float32 [X,Y,Z]: float32(((n0*x + n1*y) + n2*z) + off) at the nodes of `volume` (origin, delta, "centre" / "node", dims:
    fusion.py's record, the points fusion.node_points'), positive on the camera's side; plane [4] in the grid's frame."""
    (origin, delta, offset, dims), = _fu._volumes([volume])
    plane = np.asarray(plane, np.float64).reshape(4)
    if not np.isfinite(plane).all():
        raise ValueError("the plane is not finite")
    p = _fu.node_points(origin, delta, offset, dims)
    return residual(plane, p).astype(np.float32).reshape(dims)


def draw_triples(H: int, W: int, K: int, rng, window=None, views: int = 1) -> np.ndarray:
    """int32 [views,K,3] of uniform row-major pixel indices, optionally inside the pixel rectangle window = (r0, r1, c0, c1)
    (half open).  The three pixels of a triple are drawn independently.  Void hypotheses simply cost a slot: with a valid
    fraction g of the image about K * g^3 triples stay live, so K is sized for the background, not the draw repeated.  rng: a
    numpy Generator.  On the host; the contract starts at the array."""
    r0, r1, c0, c1 = (0, int(H), 0, int(W)) if window is None else (int(x) for x in window)
    if not (0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W) or K < 1:
        raise ValueError(f"the window must lie inside the {H} x {W} image and K be at least 1")
    r, c = rng.integers(r0, r1, (int(views), int(K), 3)), rng.integers(c0, c1, (int(views), int(K), 3))
    return (r * int(W) + c).astype(np.int32)


def plane_to_frame(plane, frame_from_cam) -> np.ndarray:
    """The plane [4] of the camera frame in another frame, frame_from_cam [4,4] rigid: n' = R n, off' = off - n'.t.  On the host."""
    plane, T = np.asarray(plane, np.float64).reshape(4), np.asarray(frame_from_cam, np.float64).reshape(4, 4)
    n = T[:3, :3] @ plane[:3]
    return np.array([n[0], n[1], n[2], plane[3] - float(n @ T[:3, 3])])
