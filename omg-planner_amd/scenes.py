"""Scene data for the CHOMP engine: SDF volumes, object tables, synthetic table-top scenes.

Two HBM layouts of the same information:

* the **reference boundary layout** of ``Env.combine_sdfs`` (omg/core.py:366-411): every grid padded
  with 1.0 to the per-scene max shape, ``sdf_torch[O,X,Y,Z]`` float32 + ``sdf_limits[O,10]`` with the
  max coordinate *stretched* to the padded shape -> :func:`pack_padded`;
* the **engine layout** of ``include/omg_hip.h``: one ragged float32 pool holding every grid of every
  scene back to back + a 128-byte ``omgx_object`` record per object + ``scene_begin[S+1]``
  -> :func:`pack_table` / :class:`SceneBatch`.

The reference's ``data/`` (YCB SDFs, scene .mat files) is a 600 MB download that is not available
offline, so benchmark and test scenes are synthetic: analytic spheres / boxes sampled at
voxel centres, a table slab, table-top poses.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import _lib

OBJECT_DTYPE = np.dtype(_lib.Object)  # records of `omgx_object` (include/omg_hip.h explains the fields), 184 bytes


def finish_records(rec: np.ndarray) -> np.ndarray:
    """Fill the derived fields (include/omg_hip.h): inv_extent = 1 / float64(float32(hi) - float32(lo)) and the default
    influence region — a rounded box  sum_k max(|t_k - c_k| - h_k, 0)^2 <= R^2  in offset-from-lo coordinates — as the plain
    box (R = 0) [-1.5 voxel, extent + 1.5 voxel].  A lookup is in range only for grid coordinates in (-0.5, dim - 0.5), so
    1.5 voxels of slack absorb every rounding; degenerate extents get an infinite box (never reject)."""
    w = (rec["hi"].astype(np.float32) - rec["lo"].astype(np.float32)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rec["inv_extent"] = 1.0 / w.astype(np.float64)
        vox = w / np.maximum(rec["dim"], 1).astype(np.float32)
    ok = (w > 0) & (rec["dim"] > 0)
    with np.errstate(invalid="ignore"):
        rec["rb_c"] = np.where(ok, 0.5 * w, 0.0).astype(np.float32)
        rec["rb_h"] = np.where(ok, 0.5 * w + 1.5 * vox, np.inf).astype(np.float32)
    rec["rb_r"] = 0.0
    rec["rb_r2"] = 0.0
    with np.errstate(divide="ignore"):
        rec["inv_delta"] = 1.0 / rec["delta"].astype(np.float64)
        eps = rec["epsilon"].astype(np.float32)
        rec["inv_2eps"] = np.float32(1.0) / (np.float32(2.0) * eps)   # float32 arithmetic like the kernel's literals
        rec["inv_eps"] = np.float32(1.0) / eps
    return rec


def _needed_windows(grid: np.ndarray, epsilon: float, clearance: float):
    """(need, ge, margin): `need[w]` (shape = grid dims) says whether a lookup through WINDOW w can return a value <= max(epsilon, 0)
    or < clearance (anything else adds neither potential, gradient nor collision, .cu:150-173; a value <= 0 takes the first hinge
    branch whatever epsilon is, .cu:158).

    Window w = (wx, wy, wz) is the trilinear polynomial of voxels w-1 .. w per axis, evaluated at fractions in [0, 1]; voxel -1 is
    the linear extension 2 v[0] - v[1].  A lookup with base index b and fractions f in [0,1)^3 uses window b + 1; on an axis
    where b == 0 the reference's trunc-toward-zero also lets f run through (-1, 0) (.cu:39-48), which is window 0 of that
    axis.  In grid coordinates g (the kernels' `gx`), window w covers g_k in [w_k - 0.5, w_k + 0.5).  A multilinear function
    takes its extrema at the vertices of a box, so the minimum over a window is the minimum of its 8 corner voxels.  A relative
    margin absorbs the float32 rounding of the lerp chain; non-finite voxels count as reachable.  `ge` = the grid in float64
    with the extension layer prepended on every axis (ge index = voxel index + 1), non-finite entries as -inf."""
    g = np.asarray(grid, np.float32).astype(np.float64)
    finite = np.isfinite(g)
    margin = 1e-5 * max(1.0, float(np.abs(g[finite]).max(initial=1.0)))
    for ax in range(3):  # prepend the extended layer on every axis
        with np.errstate(invalid="ignore"):  # inf - inf of non-finite voxels: NaN, counted as reachable below
            first = np.take(g, [0], axis=ax) * 2.0 - np.take(g, [1], axis=ax)
        g = np.concatenate([first, g], axis=ax)
    ge = np.where(np.isfinite(g), g, -np.inf)
    m = ge
    for ax in range(3):
        n = m.shape[ax]
        m = np.minimum(np.take(m, range(0, n - 1), axis=ax), np.take(m, range(1, n), axis=ax))
    need = (m <= max(float(np.float32(epsilon)), 0.0) + margin) | (m < float(np.float32(clearance)) + margin)
    return need, ge, margin


def influence_range(grid: np.ndarray, epsilon: float, clearance: float):
    """Per-axis range [bmin, bmax] of the lookup BASE indices whose trilinear value can be <= epsilon or < clearance, or None
    when no base index can (the bounding box of the needed windows, see _needed_windows)."""
    if min(np.asarray(grid).shape) < 2:
        return None
    need, _, _ = _needed_windows(grid, epsilon, clearance)
    if not need.any():
        return None
    lo, hi = [], []
    for ax in range(3):
        idx = np.flatnonzero(need.any(axis=tuple(a for a in range(3) if a != ax)))
        lo.append(max(int(idx[0]) - 1, 0)); hi.append(max(int(idx[-1]) - 1, 0))  # window w <-> base w - 1 (window 0 belongs to base 0)
    return np.array(lo), np.array(hi)


RBOX_REFINE = 4  # sub-cells per axis the boundary windows are split into when the region is fitted


def influence_rbox(grid: np.ndarray, epsilon: float, clearance: float, vox: np.ndarray):
    """A rounded box (c, h, R) — in the kernels' offset coordinates t = R_obj p + t_obj - lo, metres — that contains every
    point whose lookup can add anything:  sum_k max(|t_k - c_k| - h_k, 0)^2 <= R^2.  None when nothing can.

    The set to cover is the union of the needed windows (_needed_windows), boxes g in [w - 0.5, w + 0.5] in grid coordinates;
    windows on its boundary are split RBOX_REFINE times per axis and only the sub-boxes that can still reach the thresholds are
    kept — then merged into one bounding box per window — (the interpolant restricted to a sub-box is multilinear too: its minimum sits at a sub-box vertex).  For a given inner
    box the smallest admissible R is the largest distance from the inner box to the far corner of any kept box — the distance
    to a box is convex, so its maximum over the union is attained at such a corner.  The inner box is chosen among a small
    family (the bounding box of the needed windows eroded by 0 .. its smallest half-width; the bounding box of the non-positive
    voxels shrunk towards its centre) for the smallest volume of the resulting rounded box: a sphere-like object gets a ball, a
    box-like object its own box grown by epsilon with rounded edges, a volume that fills its grid the plain grid box (R = 0).
    Conservative for ANY volume — a field that is no distance field just gets a large R.  `vox` = voxel extents per axis."""
    dim = np.array(np.asarray(grid).shape)
    if dim.min() < 2:
        return None
    vox = np.asarray(vox, np.float64)
    need, ge, margin = _needed_windows(grid, epsilon, clearance)
    if not need.any():
        return None
    eps_t, clr_t = max(float(np.float32(epsilon)), 0.0) + margin, float(np.float32(clearance)) + margin
    # boundary windows: needed, with a face neighbour that is not (windows on the grid's faces: the outside is not needed)
    pad = np.pad(need, 1, constant_values=False)
    inner = pad[1:-1, 1:-1, 1:-1].copy()
    for ax in range(3):
        for sh in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[ax] = slice(sh, sh + need.shape[ax])
            inner &= pad[tuple(sl)]
    bidx = np.argwhere(need & ~inner)
    # kept boxes of the boundary windows in grid coordinates
    r = RBOX_REFINE
    fr = np.arange(r + 1) / r
    lo_list, hi_list = [], []
    for k0 in range(0, len(bidx), 20000):  # chunks keep the lattice arrays small
        w = bidx[k0: k0 + 20000]
        c = [[[ge[w[:, 0] + a, w[:, 1] + b, w[:, 2] + cc] for cc in (0, 1)] for b in (0, 1)] for a in (0, 1)]
        fx, fy, fz = fr[None, :, None, None], fr[None, None, :, None], fr[None, None, None, :]
        e = lambda a: a[:, None, None, None]
        lerp = lambda a, b, t: a + (b - a) * t
        with np.errstate(invalid="ignore"):
            v = lerp(lerp(lerp(e(c[0][0][0]), e(c[1][0][0]), fx), lerp(e(c[0][1][0]), e(c[1][1][0]), fx), fy),
                     lerp(lerp(e(c[0][0][1]), e(c[1][0][1]), fx), lerp(e(c[0][1][1]), e(c[1][1][1]), fx), fy), fz)
        v = np.where(np.isfinite(v), v, -np.inf)  # -inf corners: inf - inf along the way
        for ax in (1, 2, 3):
            nn = v.shape[ax]
            v = np.minimum(np.take(v, range(0, nn - 1), axis=ax), np.take(v, range(1, nn), axis=ax))
        kept = (v <= eps_t) | (v < clr_t)  # [windows, r, r, r]
        # one box per window: the bounding box of its kept sub-boxes (keeps the windows' count small for the fit below)
        lo_w, hi_w = np.empty((len(w), 3)), np.empty((len(w), 3))
        for ax in range(3):
            along = kept.any(axis=tuple(a for a in (1, 2, 3) if a != ax + 1))  # [windows, r]
            first = along.argmax(1)
            last = r - 1 - along[:, ::-1].argmax(1)
            lo_w[:, ax] = w[:, ax] - 0.5 + first / r
            hi_w[:, ax] = w[:, ax] - 0.5 + (last + 1) / r
        some = kept.reshape(len(w), -1).any(1)  # (every needed window keeps at least the sub-box of its minimal corner)
        lo_list.append(lo_w[some]); hi_list.append(hi_w[some])
    # ... and, whole, the needed windows NEXT to the boundary (inner windows with a boundary window as a face neighbour).  Once the
    # boundary windows have been shrunk to their kept sub-boxes they no longer enclose what lies behind them, and a far corner of
    # such an inner window can be the farthest point of the union.  Deeper windows cannot: along every axis a deeper window lies
    # between two windows of this layer, so none of its corners is an extreme point of the union (omgx_fit_influence_region,
    # the device version of this fit, simply feeds every inner window: the same maximum).
    bnd = need & ~inner
    padb = np.pad(bnd, 1, constant_values=False)
    adj = np.zeros_like(need)
    for ax in range(3):
        for sh in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[ax] = slice(sh, sh + need.shape[ax])
            adj |= padb[tuple(sl)]
    sidx = np.argwhere(inner & adj).astype(np.float64)
    if len(sidx):
        lo_list.append(sidx - 0.5); hi_list.append(sidx + 0.5)
    blo, bhi = np.concatenate(lo_list), np.concatenate(hi_list)
    if len(blo) == 0:  # cannot happen (a needed window keeps the sub-box of its minimal corner); stay safe
        widx = np.argwhere(need)
        blo, bhi = widx - 0.5, widx + 0.5
    # candidate inner boxes (centre, half-widths) in grid coordinates
    allw = np.argwhere(need)
    nlo, nhi = allw.min(0) - 0.5, allw.max(0) + 0.5
    bc, bh = (nlo + nhi) / 2, (nhi - nlo) / 2
    cands = []
    rmax = float((bh * vox).min())
    for k in range(9):
        cands.append((bc, np.maximum(bh - (rmax * k / 8.0) / vox, 0.0)))
    neg = np.argwhere(np.asarray(grid) <= 0)
    if len(neg):
        qlo, qhi = neg.min(0) + 0.5, neg.max(0) + 0.5  # voxel i sits at grid coordinate i + 0.5
        for sh in (0.0, 0.25, 0.5, 0.75, 1.0):
            cands.append(((qlo + qhi) / 2, (qhi - qlo) / 2 * (1.0 - sh)))
    best = None
    for ctr, h in cands:
        d = np.maximum(np.maximum(np.abs(blo - ctr), np.abs(bhi - ctr)) - h, 0.0) * vox
        R = float(np.sqrt((d * d).sum(1).max()))
        hm = h * vox
        vol = 8 * hm.prod() + 8 * R * (hm[0] * hm[1] + hm[1] * hm[2] + hm[0] * hm[2]) + 2 * np.pi * R * R * hm.sum() + 4.0 / 3.0 * np.pi * R ** 3
        if best is None or vol < best[0]:
            best = (vol, ctr * vox, hm, R)
    return best[1], best[2], best[3]


def culled(rec: np.ndarray) -> np.ndarray:
    """bool [n]: the records the kernels cull for, the ones whose influence region is worth fitting — a positive extent, more than
    one voxel along every axis, and thresholds an out-of-range lookup (which returns 1.0) cannot reach: epsilon < 1, clearance <= 1."""
    w = (rec["hi"].astype(np.float32) - rec["lo"].astype(np.float32)).astype(np.float32)
    return (w > 0).all(axis=-1) & (rec["dim"] > 1).all(axis=-1) & (rec["epsilon"] < 1.0) & (rec["clearance"] <= 1.0)


def tighten_far_boxes(rec: np.ndarray, pool: np.ndarray, cache: dict | None = None) -> np.ndarray:
    """Replace the default influence region of every record (the whole grid) by the fitted rounded box (influence_rbox) of
    the lookups that can matter, grown by 1 % of a voxel + 1e-6 m for the float32 rounding of the kernels' coordinates.
    Only meaningful where the kernels cull at all (`culled`).
    A record nothing can reach gets R^2 = -1 (every point is rejected).
    `cache` (optional dict) keeps the fits between calls (key: the volume's CONTENT, voxel sizes, epsilon, clearance — scenes
    with private copies of one model share the fit)."""
    import hashlib
    cache = {} if cache is None else cache
    for o in np.flatnonzero(culled(rec)):
        r = rec[o]
        d = r["dim"].astype(np.int64)
        w = (r["hi"].astype(np.float32) - r["lo"].astype(np.float32)).astype(np.float32)
        g = pool[int(r["grid_offset"]): int(r["grid_offset"]) + int(d.prod())]
        vox = (w / d.astype(np.float32)).astype(np.float64)
        key = (hashlib.blake2b(np.ascontiguousarray(g).tobytes(), digest_size=12).digest(), tuple(d), tuple(vox), float(r["epsilon"]), float(r["clearance"]))
        if key not in cache:
            cache[key] = influence_rbox(g.reshape(tuple(d)), key[3], key[4], vox)
        fit = cache[key]
        if fit is None:  # nothing reachable: an empty region rejects every point
            r["rb_c"] = 0.0
            r["rb_h"] = 0.0
            r["rb_r"] = 0.0
            r["rb_r2"] = -1.0
            continue
        c, h, R = fit
        R = R + 0.01 * float(vox.min()) + 1e-6
        r["rb_c"] = c.astype(np.float32)
        r["rb_h"] = np.nextafter(h.astype(np.float32), np.float32(np.inf))  # rounded up
        r["rb_r"] = np.nextafter(np.float32(R), np.float32(np.inf))
        r["rb_r2"] = np.nextafter(np.float32(float(r["rb_r"]) ** 2), np.float32(np.inf))
    return rec


@dataclass
class SdfGrid:
    """What the path reads of SignedDensityField (omg/sdf_tools.py:17-35): data[x,y,z], origin, delta."""
    data: np.ndarray  # [X,Y,Z] float32
    origin: np.ndarray  # min_coords [3]
    delta: float

    @property
    def min_coords(self) -> np.ndarray:
        return np.asarray(self.origin, dtype=np.float64)

    @property
    def max_coords(self) -> np.ndarray:  # sdf_tools.py:30
        return self.min_coords + self.delta * np.array(self.data.shape)


@dataclass
class SceneObject:
    """What the path reads of Model (omg/core.py:83-141): name, pose_mat, sdf, attached."""
    name: str
    pose_mat: np.ndarray  # [4,4] object -> world
    sdf: SdfGrid
    attached: bool = False


@dataclass
class Scene:
    objects: list = field(default_factory=list)
    target_idx: int = 0


def scene_from_env(env) -> Scene:
    """The `Scene` of a reference `Env` (omg/core.py:239-411), for `pack_table` / `ChompEngine`: every object's name, pose and
    attached flag and the volume the reference itself puts on the GPU — `obj.sdf.data_torch` (core.py:381), NOT `obj.sdf.data`,
    whose negative values `Model` has multiplied by cfg.penalize_constant on the numpy copy only (core.py:110) — with origin
    `sdf.min_coords` and voxel size `sdf.delta`."""
    objs = []
    for o in env.objects:
        vol = getattr(o.sdf, "data_torch", None)
        vol = np.asarray(o.sdf.data, np.float32) if vol is None else vol.detach().cpu().numpy().astype(np.float32)
        objs.append(SceneObject(str(o.name), np.array(o.pose_mat, np.float64), SdfGrid(np.ascontiguousarray(vol), np.array(o.sdf.min_coords, np.float64),
                                                                                   float(o.sdf.delta)), bool(getattr(o, "attached", False))))
    return Scene(objs, int(env.target_idx))


def se3_inverse(pose: np.ndarray) -> np.ndarray:
    """[R t]^-1 = [R^T, -R^T t] as float32 (omg/util.py:129-135)."""
    out = np.eye(4, dtype=np.float32)
    R = pose[:3, :3]
    out[:3, :3] = R.T
    out[:3, 3] = -(R.T @ pose[:3, 3])
    return out


# ------------------------------------------------------------------------------------------------
# analytic SDFs
# ------------------------------------------------------------------------------------------------
def _voxel_centres(shape, origin, delta):
    ax = [origin[i] + (np.arange(shape[i]) + 0.5) * delta for i in range(3)]
    return np.meshgrid(*ax, indexing="ij")


def sphere_sdf(radius: float, shape=(64, 64, 64), delta: float = 0.6 / 64) -> SdfGrid:
    origin = -0.5 * delta * np.array(shape, dtype=np.float64)
    x, y, z = _voxel_centres(shape, origin, delta)
    return SdfGrid((np.sqrt(x * x + y * y + z * z) - radius).astype(np.float32), origin, float(delta))


def box_sdf(half_extents, shape=(64, 64, 64), delta: float = 0.6 / 64) -> SdfGrid:
    origin = -0.5 * delta * np.array(shape, dtype=np.float64)
    x, y, z = _voxel_centres(shape, origin, delta)
    q = np.stack([np.abs(x) - half_extents[0], np.abs(y) - half_extents[1], np.abs(z) - half_extents[2]], -1)
    outside = np.linalg.norm(np.maximum(q, 0.0), axis=-1)
    inside = np.minimum(q.max(-1), 0.0)
    return SdfGrid((outside + inside).astype(np.float32), origin, float(delta))


def point_cloud_sdf(points: np.ndarray, grid_resolution: float = 0.02, margin: float = 0.24) -> SdfGrid:
    """Unsigned nearest-point distance grid like PointEnv.compute_sdf_from_points (omg/core.py:426-457):
    grid nodes at arange(min - margin, max + margin, res) per axis, value = distance to nearest point."""
    from scipy.spatial import cKDTree

    lo, hi = points.min(0), points.max(0)
    ax = [np.arange(lo[i] - margin, hi[i] + margin, grid_resolution) for i in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), 0)
    d, _ = cKDTree(points).query(g.reshape(3, -1).T)
    return SdfGrid(d.reshape(g.shape[1:]).astype(np.float32), (lo - margin).astype(np.float64), float(grid_resolution))


# ------------------------------------------------------------------------------------------------
# signed distance grids from triangle meshes: the specification of omgx_mesh_sdf (csrc/omg_mesh_sdf.hip follows it operation by
# operation) and the CPU path.  The reference has no counterpart in the planner: it runs a mesh through the external SDFGen binary
# (real_world/gen_sdf.py:13-37) and reads the text file that comes out (omg/sdf_tools.py:169-185).
# ------------------------------------------------------------------------------------------------
MESH_SAMPLE_OFFSET = {"centre": 0.5, "node": 0.0}
REGION_NAMES = ("a", "b", "ab", "c", "ac", "bc", "interior")  # closest_point_on_triangle's region numbers


def _dot3(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def closest_point_on_triangle(p, a, b, c):
    """The point of triangle (a, b, c) closest to each row of p [N,3], by the seven regions of the triangle's plane: the first
    that holds of vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, else the interior -> (q [N,3], region [N] indexing
    REGION_NAMES).  float64, every operation rounded on its own, in the order the kernel keeps: dot products as (x*x' + y*y') + z*z',
    an edge point as base + (num / den) * dir, the interior as (a + ab * v) + ac * w with v = vb * inv, w = vc * inv,
    inv = 1 / ((va + vb) + vc)."""
    p = np.asarray(p, np.float64)
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    P = (p[..., 0], p[..., 1], p[..., 2])
    ab, ac, bc = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)], [c[k] - b[k] for k in range(3)]
    ap, bp, cp = [P[k] - a[k] for k in range(3)], [P[k] - b[k] for k in range(3)], [P[k] - c[k] for k in range(3)]
    d1, d2 = _dot3(ab, ap), _dot3(ac, ap)
    d3, d4 = _dot3(ab, bp), _dot3(ac, bp)
    d5, d6 = _dot3(ab, cp), _dot3(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    region = np.select([(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                        (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e1 >= 0) & (e2 >= 0)], [0, 1, 2, 3, 4, 5], 6)
    on_ab, on_ac, on_bc = region == 2, region == 4, region == 5
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):  # the quotients of the regions that do not hold
        t = np.select([on_ab, on_ac, on_bc], [d1, d2, e1], 0.0) / np.select([on_ab, on_ac, on_bc], [d1 - d3, d2 - d6, e1 + e2], 1.0)
        inv = 1.0 / ((va + vb) + vc)
        v, w = vb * inv, vc * inv
        q = []
        for k in range(3):
            base = np.where((region == 1) | on_bc, b[k], np.where(region == 3, c[k], a[k]))
            edge = base + t * np.where(on_ab, ab[k], np.where(on_ac, ac[k], bc[k]))
            q.append(np.where(region == 6, (a[k] + ab[k] * v) + ac[k] * w, edge))
    return np.stack(q, -1), region


def clean_mesh(verts, faces):
    """(verts [V,3] float64, faces [F',3] int32, dropped): the mesh as omgx_mesh_sdf takes it.  Face indices must lie in [0, V)
    (ValueError otherwise); faces whose normal (b - a) x (c - a) is exactly zero in float64 have no closest-point regions and
    no solid angle, and are dropped (`dropped` of them)."""
    verts = np.ascontiguousarray(verts, np.float64)
    faces = np.asarray(faces)
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"a mesh is verts [V,3] and faces [F,3], got {verts.shape} and {faces.shape}")
    if not np.issubdtype(faces.dtype, np.integer):
        raise ValueError(f"face indices must be integers, got {faces.dtype}")
    if not np.isfinite(verts).all():
        raise ValueError("a vertex is not finite")
    if len(verts) < 1 or len(faces) < 1:
        raise ValueError("a mesh needs at least one vertex and one face")
    if faces.min() < 0 or faces.max() >= len(verts):
        raise ValueError(f"face indices must lie in [0, {len(verts)}): found {int(faces.min())} .. {int(faces.max())}")
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    u, v = b - a, c - a
    keep = ~((u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1] == 0) & (u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2] == 0) &
             (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0] == 0))
    if not keep.any():
        raise ValueError("every face of the mesh has zero area")
    return verts, np.ascontiguousarray(faces[keep], np.int32), int((~keep).sum())


def mesh_grid_layout(verts, delta: float, padding: int):
    """(origin [3] float64, dims [3] int) of a grid around a mesh: `padding` voxels on every side of the vertices' bounding box
    [lo, hi]: origin = lo - padding * delta, dims = ceil((hi - lo) / delta) + 2 * padding (float64)."""
    verts = np.asarray(verts, np.float64)
    lo, hi = verts.min(0), verts.max(0)
    dims = np.array([int(np.ceil((hi[a] - lo[a]) / delta)) + 2 * int(padding) for a in range(3)], np.int64)
    return lo - int(padding) * float(delta), dims


def mesh_nodes(origin, dims, delta: float, sample: str = "centre") -> np.ndarray:
    """The sample positions [X*Y*Z, 3] (x-major) of a grid: origin + ((i, j, k) + offset) * delta, offset 0.5 for "centre" and 0.0 for
    "node" (see mesh_sdf)."""
    off = MESH_SAMPLE_OFFSET[sample]
    ax = [origin[a] + (np.arange(int(dims[a])).astype(np.float64) + off) * float(delta) for a in range(3)]
    return np.stack([g.ravel() for g in np.meshgrid(*ax, indexing="ij")], -1)


def mesh_distance_winding(verts, faces, p):
    """(d [N], w [N]) float64 for the points p [N,3]: d = sqrt(min over faces |p - closest_point_on_triangle(p, face)|^2) with
    |r|^2 = (rx*rx + ry*ry) + rz*rz, and the generalised winding number
    w = (1 / 4 pi) sum over faces 2 atan2(A.(BxC), |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|), A, B, C = a - p, b - p, c - p.
    verts / faces as clean_mesh returns them.  Vectorised over the points with a loop over the faces."""
    p = np.asarray(p, np.float64)
    best = np.full(len(p), 1.0e300)
    wsum = np.zeros(len(p))
    for f in faces:
        a, b, c = verts[f[0]], verts[f[1]], verts[f[2]]
        q, _ = closest_point_on_triangle(p, a, b, c)
        r = [p[:, k] - q[:, k] for k in range(3)]
        dd = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
        best = np.where(dd < best, dd, best)
        A, B, C = [a[k] - p[:, k] for k in range(3)], [b[k] - p[:, k] for k in range(3)], [c[k] - p[:, k] for k in range(3)]
        la, lb, lc = np.sqrt(_dot3(A, A)), np.sqrt(_dot3(B, B)), np.sqrt(_dot3(C, C))
        n = [B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0]]
        wsum += np.arctan2(_dot3(A, n), ((la * lb) * lc + _dot3(A, B) * lc) + (_dot3(B, C) * la + _dot3(C, A) * lb))
    return np.sqrt(best), wsum * (2.0 / (4.0 * np.pi))


def mesh_sdf(verts, faces, delta: float, padding: int = 4, sample: str = "centre", origin=None, dims=None) -> SdfGrid:
    """Signed distance grid of a triangle mesh -> SdfGrid (float32 data[x, y, z], origin, delta).  Sample i of an axis sits at
    origin + (i + offset) * delta:

    * sample="centre" (offset 0.5, the default) is where the SDF op reads a grid: it interpolates at p / delta - 0.5
      (layers/sdf_matching_loss_kernel.cu:36-41; `_voxel_centres`, what sphere_sdf / box_sdf fill), so this is the
      convention that makes the looked-up distance right;
    * sample="node" (offset 0.0) is the convention of the text .sdf files the reference consumes as far as its reader shows
      (sdf_tools.py:169-185 takes origin and delta from the header and keeps them as min_coords and voxel size).  The program
      that writes those files, SDFGen, is not part of the reference and nothing here pins where it samples.

    origin / dims default to mesh_grid_layout(verts, delta, padding); given explicitly they align the grid with another one.
    Value: mesh_distance_winding's d, negated where |w| > 0.5 (inside; |w| so that a mesh whose faces all point inwards gives the
    same volume), rounded to float32 once.  Faces of zero area are dropped (clean_mesh).  Plain numpy float64: the specification
    of omgx_mesh_sdf (ops.mesh_sdf gives the same float32 magnitudes bit for bit) and the CPU path; it may be slow."""
    verts, faces, _ = clean_mesh(verts, faces)
    if sample not in MESH_SAMPLE_OFFSET:
        raise ValueError(f"sample must be 'centre' or 'node', got {sample!r}")
    delta = float(delta)
    if not (delta > 0 and np.isfinite(delta)):
        raise ValueError("delta must be positive and finite")
    if (origin is None) != (dims is None):
        raise ValueError("give origin and dims together")
    if origin is None:
        origin, dims = mesh_grid_layout(verts, delta, padding)
    origin = np.asarray(origin, np.float64).copy()
    dims = tuple(int(d) for d in dims)
    if min(dims) < 1:
        raise ValueError(f"dims must be >= 1, got {dims}")
    d, w = mesh_distance_winding(verts, faces, mesh_nodes(origin, dims, delta, sample))
    return SdfGrid(np.where(np.abs(w) > 0.5, -d, d).astype(np.float32).reshape(dims), origin, delta)


# ------------------------------------------------------------------------------------------------
# triangle meshes from distance volumes (naive surface nets): the specification of omgx_surface_count / omgx_surface_gather
# (csrc/omg_surface_body.h follows it operation by operation) and the CPU path.  The reference has no counterpart: its data set keeps
# a mesh file beside every volume file (omg/core.py:86-127 loads the volume, ycb_render the mesh), and an object it has no mesh of
# gets its grasps from an outside detector (omg/planner.py:176-186).
# ------------------------------------------------------------------------------------------------
def _surface_edges():
    """The 12 edges of a cell in the order the vertex sums them: axis x, y, z; the offsets (u, w) on the two other axes, taken
    cyclically (x -> (y, z), y -> (z, x), z -> (x, y)), through 00, 01, 10, 11 -> [(axis, o1, o2, u, w)]."""
    return [(ax, (ax + 1) % 3, (ax + 2) % 3, u, w) for ax in range(3) for u in (0, 1) for w in (0, 1)]


def surface_nets(grid, origin=None, delta=None, sample: str = "centre", level: float = 0.0):
    """The level set {v = level} of a distance volume as a triangle mesh -> (verts [V,3] float64, faces [F,3] int32, open_edges).
    grid: an SdfGrid (origin and delta default to its own) or an array [X,Y,Z]; sample (i,j,k) sits at
    origin + ((i,j,k) + offset) * delta, offset 0.5 for "centre" and 0.0 for "node", as in mesh_sdf.

    * inside(i,j,k) = v[i,j,k] < float32(level), a float32 compare: NaN is outside.
    * Cell (i,j,k), 0 <= i < X-1 and so on, has the corners (i+dx, j+dy, k+dz); it is active iff they are neither all inside nor
      all outside.  An active cell has ONE vertex: over its 12 edges in _surface_edges' order, an edge from corner a to
      b = a + e_axis crosses iff inside(a) != inside(b), at t = (L - va) / (vb - va) with L = float64(float32(level)) and the
      samples widened to float64 (t outside [0,1], i.e. from samples that are not finite: t = 0.5); the crossing point has t on the
      axis and the edge's offsets (u, w) on the two others; local = (sum of the crossing points, in that order, component by
      component, from +0.0) / count, and vertex = origin + (((i,j,k) + offset) + local) * delta.  + - * / only, each rounded once.
    * Vertices are numbered by their cell's x-major index, ascending.
    * Every sample edge a -> a + e_axis with inside(a) != inside(b) has four cells around it, with (o1, o2) the cyclic other axes:
      c0 = a - e_o1 - e_o2, c1 = a - e_o2, c2 = a, c3 = a - e_o1.  If one of them is outside the grid the edge gives nothing and
      counts as an open edge; otherwise two triangles split along c0-c2, turned so that the normal points from inside to outside:
      (c0,c1,c2), (c0,c2,c3) if inside(a), else (c0,c2,c1), (c0,c3,c2).  Faces are ordered by 3 * linear(a) + axis, ascending.
    * A volume with a dim below 2 has no cells: an empty mesh (V = F = 0) whose crossing edges are all open.  All inside or all
      outside: an empty mesh without open edges.

    The surface is closed iff open_edges == 0.  Plain numpy float64, vectorised over the cells."""
    if isinstance(grid, SdfGrid):
        origin = grid.min_coords if origin is None else origin
        delta = grid.delta if delta is None else delta
        grid = grid.data
    if origin is None or delta is None:
        raise ValueError("an array needs origin and delta")
    if sample not in MESH_SAMPLE_OFFSET:
        raise ValueError(f"sample must be 'centre' or 'node', got {sample!r}")
    delta, off = float(delta), MESH_SAMPLE_OFFSET[sample]
    if not (delta > 0 and np.isfinite(delta)):
        raise ValueError("delta must be positive and finite")
    origin = np.asarray(origin, np.float64).reshape(3)
    v32 = np.ascontiguousarray(grid, np.float32)
    if v32.ndim != 3 or min(v32.shape) < 1:
        raise ValueError(f"a volume is [X,Y,Z] with every dim >= 1, got {v32.shape}")
    L32 = np.float32(level)
    if np.isnan(L32):
        raise ValueError("level is NaN")
    empty = (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int32), 0)
    n = v32.shape
    inside = v32 < L32
    v, L = v32.astype(np.float64), float(L32)
    c = tuple(d - 1 for d in n)  # cells per axis

    def corner(a, d):  # the corner (dx, dy, dz) = d of every cell
        return a[d[0]: d[0] + c[0], d[1]: d[1] + c[1], d[2]: d[2] + c[2]]
    n_in = sum(corner(inside, (dx, dy, dz)).astype(np.int32) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    active = (n_in > 0) & (n_in < 8)
    sums, count = [np.zeros(c), np.zeros(c), np.zeros(c)], np.zeros(c)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for ax, o1, o2, u, w in _surface_edges():
            da, db = [0, 0, 0], [0, 0, 0]
            da[o1] = db[o1] = u
            da[o2] = db[o2] = w
            db[ax] = 1
            cross = corner(inside, da) != corner(inside, db)
            va, vb = corner(v, da), corner(v, db)
            t = (L - va) / (vb - va)
            t = np.where((t >= 0.0) & (t <= 1.0), t, 0.5)
            p = [None, None, None]
            p[ax], p[o1], p[o2] = t, float(u), float(w)
            for k in range(3):
                sums[k] = sums[k] + np.where(cross, p[k], 0.0)
            count = count + np.where(cross, 1.0, 0.0)
        ijk = np.nonzero(active)  # x-major, ascending
        verts = np.stack([origin[k] + ((ijk[k].astype(np.float64) + off) + sums[k][ijk] / count[ijk]) * delta for k in range(3)], -1)
    index = np.full(c, -1, np.int64)
    index[ijk] = np.arange(len(ijk[0]))
    keys, tris, open_edges = [], [], 0
    lin = np.arange(int(np.prod(n)), dtype=np.int64).reshape(n)
    for ax in range(3):
        o1, o2 = (ax + 1) % 3, (ax + 2) % 3
        sl_a, sl_b = [slice(None)] * 3, [slice(None)] * 3
        sl_a[ax], sl_b[ax] = slice(0, n[ax] - 1), slice(1, n[ax])
        ia = inside[tuple(sl_a)]
        a = np.stack(np.nonzero(ia != inside[tuple(sl_b)]), -1)  # the samples a of the crossing edges of this axis
        if not len(a):
            continue
        closed = (a[:, o1] >= 1) & (a[:, o1] <= n[o1] - 2) & (a[:, o2] >= 1) & (a[:, o2] <= n[o2] - 2)
        open_edges += int((~closed).sum())
        a = a[closed]
        e1, e2 = np.zeros(3, np.int64), np.zeros(3, np.int64)
        e1[o1], e2[o2] = 1, 1
        cell = lambda q: index[q[:, 0], q[:, 1], q[:, 2]]
        c0, c1, c2, c3 = cell(a - e1 - e2), cell(a - e2), cell(a), cell(a - e1)
        a_in = inside[a[:, 0], a[:, 1], a[:, 2]]
        first = np.where(a_in[:, None], np.stack([c0, c1, c2], -1), np.stack([c0, c2, c1], -1))
        second = np.where(a_in[:, None], np.stack([c0, c2, c3], -1), np.stack([c0, c3, c2], -1))
        keys.append(3 * lin[a[:, 0], a[:, 1], a[:, 2]] + ax)
        tris.append(np.stack([first, second], 1))
    if not keys:
        return (verts, empty[1], open_edges) if len(verts) else (empty[0], empty[1], open_edges)
    order = np.argsort(np.concatenate(keys), kind="stable")
    faces = np.concatenate(tris)[order].reshape(-1, 3)
    assert faces.min(initial=0) >= 0  # the four cells of a crossing edge each have a crossing edge: they are active
    return verts, np.ascontiguousarray(faces, np.int32), open_edges


# ------------------------------------------------------------------------------------------------
# per-object SDF-layer parameters (Cost.compute_obstacle_cost_layer, omg/cost.py:303-328)
# ------------------------------------------------------------------------------------------------
def layer_params(scene: Scene, epsilon=0.2, target_epsilon=0.1, clearance=0.01, target_clearance=0.0,
                 disable_collision_set=(), special_check_id=None):
    """-> poses_inv [O,4,4] f32, epsilons, padding_scales, clearances, disables [O] f32.

    ``special_check_id`` is accepted for signature parity; like the reference, the target is taken from
    ``scene.target_idx`` (cost.py:321 compares against ``self.env.target_idx``).
    """
    O = len(scene.objects)
    poses = np.zeros((O, 4, 4), np.float32)
    eps = np.full(O, epsilon, np.float32)
    pad = np.ones(O, np.float32)
    clr = np.full(O, clearance, np.float32)
    dis = np.zeros(O, np.float32)
    for i, ob in enumerate(scene.objects):
        if ob.name == "floor" or ob.name in disable_collision_set:
            dis[i] = 1
        poses[i] = se3_inverse(ob.pose_mat)
        if i == scene.target_idx:
            clr[i] = target_clearance
            eps[i] = target_epsilon
    if O > 0 and scene.objects[scene.target_idx].attached:  # cost.py:325-328 (table is last)
        clr[-1] = 0.0
        eps[-1] = 0.05
        pad[-1] = 0.5
    return poses, eps, pad, clr, dis


# ------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------
def pack_padded(objects) -> tuple[np.ndarray, np.ndarray]:
    """Env.combine_sdfs (omg/core.py:366-411): -> sdf [O,X,Y,Z] f32 (pad value 1.0), limits [O,10] f32."""
    shapes = np.array([o.sdf.data.shape for o in objects])
    mx = shapes.max(0)
    sdf = np.ones((len(objects), mx[0], mx[1], mx[2]), np.float32)
    lim = np.zeros((len(objects), 10), np.float32)
    for i, o in enumerate(objects):
        sz = o.sdf.data.shape
        sdf[i, : sz[0], : sz[1], : sz[2]] = o.sdf.data.astype(np.float32)
        mn, mxc = o.sdf.min_coords, o.sdf.max_coords
        lim[i, 0:3] = mn
        for a in range(3):
            lim[i, 3 + a] = mn[a] + (mxc[a] - mn[a]) * mx[a] / sz[a]
        lim[i, 6:9] = mx
        lim[i, 9] = o.sdf.delta
    return sdf, lim


def table_from_padded(poses_inv, limits, eps, pad, clr, dis, grid_elems_per_object=None) -> np.ndarray:
    """omgx_object records that address the reference's padded [O,X,Y,Z] tensor in place."""
    O = limits.shape[0]
    rec = np.zeros(O, OBJECT_DTYPE)
    for o in range(O):
        rec[o]["pose_inv"] = np.asarray(poses_inv[o], np.float32)[:3, :4].ravel()
        rec[o]["lo"] = limits[o, 0:3]
        rec[o]["hi"] = limits[o, 3:6]
        rec[o]["dim"] = limits[o, 6:9].astype(np.int32)
        rec[o]["delta"] = limits[o, 9]
        rec[o]["epsilon"] = eps[o]
        rec[o]["padding_scale"] = pad[o]
        rec[o]["clearance"] = clr[o]
        rec[o]["disabled"] = 1 if dis[o] > 0 else 0
        d = rec[o]["dim"].astype(np.int64)
        rec[o]["grid_offset"] = o * int(d[0] * d[1] * d[2]) if grid_elems_per_object is None else o * grid_elems_per_object
    return finish_records(rec)


@dataclass
class SceneBatch:
    """Engine layout for S scenes: object records, scene_begin[S+1], one ragged float32 pool."""
    objects: np.ndarray  # OBJECT_DTYPE [sum O_s]
    scene_begin: np.ndarray  # int32 [S+1]
    pool: np.ndarray  # float32 [sum voxels]

    @property
    def num_scenes(self) -> int:
        return len(self.scene_begin) - 1

    def subset(self, first: int, last: int) -> "SceneBatch":
        """Scenes [first, last) as their own batch: records copied, scene_begin rebased, and the pool cut to
        the range those records address (grid offsets rebased)."""
        lo_o, hi_o = int(self.scene_begin[first]), int(self.scene_begin[last])
        rec = self.objects[lo_o:hi_o].copy()
        sizes = rec["dim"].astype(np.int64).prod(axis=1)
        p0 = int(rec["grid_offset"].min()) if len(rec) else 0
        p1 = int((rec["grid_offset"] + sizes).max()) if len(rec) else 0
        rec["grid_offset"] -= p0
        return SceneBatch(rec, (self.scene_begin[first:last + 1] - lo_o).astype(np.int32), self.pool[p0:p1])


def grid_limits(origin, shape, delta):
    """(lo, hi) float32 [3] a record keeps of a grid of `shape` voxels of size `delta` with its min corner at `origin`: hi is
    combine_sdfs' stretched max coordinate with max_shape == size (omg/core.py:366-411), float64 arithmetic rounded to float32 ONCE."""
    mn = np.asarray(origin, np.float64)
    mxc = mn + float(delta) * np.array(shape)
    return mn.astype(np.float32), np.array([mn[a] + (mxc[a] - mn[a]) * 1.0 for a in range(3)], np.float32)


def ragged_records(scenes, cfg_kwargs=None, share_grids: bool = True):
    """The records of `scenes` in the ragged engine layout, without touching a voxel -> (rec after finish_records, scene_begin
    int32 [S+1], chunks = [(offset, ndarray)] of the distinct volumes in pool order, the elements they take).  share_grids: a
    volume several objects reference (the same ndarray) once.  pack_table concatenates the chunks, DeviceScenes.from_scenes uploads them."""
    cfg_kwargs = cfg_kwargs or {}
    rec = np.zeros(sum(len(s.objects) for s in scenes), OBJECT_DTYPE)
    begins, chunks, seen, offset, k = [0], [], {}, 0, 0
    for s in scenes:
        poses, eps, pad, clr, dis = layer_params(s, **cfg_kwargs)
        m = len(s.objects)
        rec["pose_inv"][k: k + m] = poses[:, :3, :4].reshape(m, 12)
        rec["epsilon"][k: k + m], rec["padding_scale"][k: k + m], rec["clearance"][k: k + m] = eps, pad, clr
        rec["disabled"][k: k + m] = dis > 0
        for i, ob in enumerate(s.objects):
            rec["lo"][k + i], rec["hi"][k + i] = grid_limits(ob.sdf.min_coords, ob.sdf.data.shape, ob.sdf.delta)
            rec["dim"][k + i] = ob.sdf.data.shape
            rec["delta"][k + i] = ob.sdf.delta
            key = id(ob.sdf.data)
            if not (share_grids and key in seen):
                seen[key] = offset
                chunks.append((offset, ob.sdf.data))
                offset += int(ob.sdf.data.size)
            rec["grid_offset"][k + i] = seen[key]
        k += m
        begins.append(k)
    return finish_records(rec), np.array(begins, np.int32), chunks, offset


def pack_table(scenes, cfg_kwargs=None, ragged: bool = True, share_grids: bool = True, tight: bool = True) -> SceneBatch:
    """Pack scenes into the engine layout.

    ragged=True keeps every grid at its own shape (true limits); ragged=False reproduces the
    reference's pad-to-max + stretched-limits layout per scene.  The two agree up to the float32
    rounding of the grid coordinate (u-lo)/(hi-lo)*dim; inside the stretched box the padded layout reads
    the 1.0 padding value where the ragged one returns the out-of-range 1.0 — the same number.
    share_grids=True stores a grid referenced by several scenes once (same ndarray object).
    tight=True shrinks each record's far box to the voxels that can contribute (tighten_far_boxes): same results,
    fewer exact lookups.
    """
    if ragged:
        rec, begins, chunks, _ = ragged_records(scenes, cfg_kwargs, share_grids)
        chunks = [np.ascontiguousarray(data, np.float32).ravel() for _, data in chunks]
    else:
        recs, begins, chunks, offset = [], [0], [], 0
        for sc in scenes:
            poses, eps, pad, clr, dis = layer_params(sc, **(cfg_kwargs or {}))
            sdf, lim = pack_padded(sc.objects)
            t = table_from_padded(poses, lim, eps, pad, clr, dis)
            t["grid_offset"] += offset
            chunks.append(sdf.ravel())
            offset += sdf.size
            recs.extend(list(t))
            begins.append(len(recs))
        rec, begins = finish_records(np.array(recs, OBJECT_DTYPE)), np.array(begins, np.int32)
    pool = np.concatenate(chunks) if chunks else np.zeros(0, np.float32)
    if tight:
        tighten_far_boxes(rec, pool)
    return SceneBatch(rec, begins, pool)


# ------------------------------------------------------------------------------------------------
# synthetic table-top scenes
# ------------------------------------------------------------------------------------------------
_SHAPE_CACHE: dict = {}


def _shape(kind: str, key, grid: int) -> SdfGrid:
    k = (kind, key, grid)
    if k not in _SHAPE_CACHE:
        delta = 0.6 / grid
        if kind == "sphere":
            _SHAPE_CACHE[k] = sphere_sdf(key, (grid,) * 3, delta)
        else:
            _SHAPE_CACHE[k] = box_sdf(key, (grid,) * 3, delta)
    return _SHAPE_CACHE[k]


def _yaw_pose(x, y, z, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [x, y, z]
    return T


def make_tabletop_scene(seed: int, num_objects: int = 4, grid: int = 64, table_grid=(128, 96, 32)) -> Scene:
    """`num_objects` YCB-like shapes (spheres r 6-9 cm, boxes 5-20 cm) on `grid`^3 volumes with
    delta = 0.6/grid m, plus a table slab 1.2 x 0.8 x 0.04 m as the LAST object (cost.py:325-328 treats
    objects[-1] as the table).  Object 0 is the grasp target.  A small palette of shapes is shared
    between scenes (like the 21 YCB models are shared between the reference's 100 scenes)."""
    rng = np.random.RandomState(seed)
    radii = (0.06, 0.07, 0.08, 0.09)
    boxes = ((0.025, 0.05, 0.10), (0.05, 0.05, 0.05), (0.04, 0.08, 0.03), (0.03, 0.03, 0.09))
    objs = []
    for i in range(num_objects):
        if rng.rand() < 0.5:
            sdf = _shape("sphere", radii[rng.randint(len(radii))], grid)
        else:
            sdf = _shape("box", boxes[rng.randint(len(boxes))], grid)
        pose = _yaw_pose(rng.uniform(0.3, 0.7), rng.uniform(-0.3, 0.3), 0.15 + rng.uniform(-0.02, 0.02),
                         rng.uniform(-np.pi, np.pi))
        objs.append(SceneObject(f"obj_{i}", pose, sdf))
    tk = ("table", tuple(table_grid))
    if tk not in _SHAPE_CACHE:
        tdelta = 1.5 / table_grid[0]
        _SHAPE_CACHE[tk] = box_sdf((0.6, 0.4, 0.02), table_grid, tdelta)
    objs.append(SceneObject("table", _yaw_pose(0.5, 0.0, 0.02, 0.0), _SHAPE_CACHE[tk]))
    return Scene(objs, target_idx=0)


def make_goal_set(seed: int, num_goals: int) -> np.ndarray:
    """Reach configurations near a table-top pre-grasp + N(0, 0.05^2) on the arm joints."""
    rng = np.random.RandomState(10_000 + seed)
    base = np.array([0.3, 0.2, 0.1, -1.6, 0.1, 1.9, 1.0, 0.04, 0.04])
    g = np.tile(base, (num_goals, 1))
    g[:, :7] += rng.normal(0.0, 0.05, size=(num_goals, 7))
    return g


_REACH_POOL: dict = {}


def _reach_pool(model, count: int = 400_000, seed: int = 1234):
    """Random arm configurations within the soft joint limits with their hand pose (numpy FK), cached."""
    key = (count, seed)
    if key not in _REACH_POOL:
        from scipy.spatial import cKDTree
        rng = np.random.RandomState(seed)
        lo, hi = model.joint_lower_limit[0], model.joint_upper_limit[0]
        q = rng.uniform(lo, hi, size=(count, 9))
        q[:, 7:] = 0.04
        pos, zax = hand_pose(model, q)
        keep = pos[:, 2] > 0.10
        q, pos, zax = q[keep], pos[keep], zax[keep]
        _REACH_POOL[key] = (q, pos, zax, cKDTree(pos))
    return _REACH_POOL[key]


def hand_pose(model, q: np.ndarray):
    """Position and approach (z) axis of the hand link for configurations q [B,9]: the first 8 frames of
    robot_pykdl.py:148-215 in plain numpy (host-side scene synthesis only, not on the hot path)."""
    offs = [0.0, -np.pi, np.pi, np.pi, -np.pi, np.pi, np.pi]
    B = q.shape[0]
    cur = np.tile(np.eye(4), (B, 1, 1))
    for i in range(7):
        c, s = np.cos(q[:, i]), np.sin(q[:, i])
        Rz = np.tile(np.eye(4), (B, 1, 1))
        Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1] = c, -s, s, c
        co, so = np.cos(offs[i]), np.sin(offs[i])
        Rx = np.array([[1, 0, 0, 0], [0, co, -so, 0], [0, so, co, 0], [0, 0, 0, 1.0]])
        b = model.pose_0[i] @ (Rz @ Rx)
        if i > 0:
            b[..., [1, 2]] *= -1
        cur = cur @ b
    hand = cur @ model.pose_0[7]
    return hand[:, :3, 3].copy(), hand[:, :3, 2].copy()


def make_reach_goals(scene: "Scene", model, num_goals: int, seed: int = 0) -> np.ndarray:
    """Grasp-like goal set for the scene's target: configurations whose hand sits 10-16 cm from the
    target's centre, above it, with the approach axis pointing at it — a stand-in for the IK'd grasp
    set of Planner.solve_goal_set_ik (omg/planner.py:296-455; IK itself is out of scope)."""
    q, pos, zax, tree = _reach_pool(model)
    ctr = scene.objects[scene.target_idx].pose_mat[:3, 3]
    rng = np.random.RandomState(20_000 + seed)
    radius = 0.16
    while True:
        idx = np.array(tree.query_ball_point(ctr, radius), dtype=np.int64)
        if idx.size:
            d = ctr[None] - pos[idx]
            dist = np.linalg.norm(d, axis=1)
            good = (dist > 0.10) & (np.einsum("ij,ij->i", d / dist[:, None], zax[idx]) > 0.8) & (pos[idx, 2] > ctr[2] + 0.02)
            idx = idx[good]
        if idx.size >= num_goals or radius > 0.4:
            break
        radius += 0.02
    if idx.size == 0:
        return make_goal_set(seed, num_goals)
    pick = rng.choice(idx, size=num_goals, replace=idx.size < num_goals)
    return q[pick].copy()


def linear_init(start: np.ndarray, end: np.ndarray, n: int) -> np.ndarray:
    """Interior waypoints linspace(0,1,n+2)[1:-1] between start and end (util.py:238-258, "linear"): bit-identical to
    the reference's interp1d result (linspace is i * step with step = fl(1 / (n + 1)))."""
    t = np.linspace(0, 1, n + 2)[1:-1, None]
    return start[None] + t * (end - start)[None]


def cubic_init(start: np.ndarray, end: np.ndarray, n: int) -> np.ndarray:
    """Clamped cubic spline through (0,start),(1,end) with zero end slopes = 3t^2-2t^3 blend
    (closed form of scipy CubicSpline(bc_type="clamped") on two knots, util.py:252)."""
    t = (np.arange(1, n + 1) / (n + 1.0))[:, None]
    h = 3.0 * t * t - 2.0 * t * t * t
    return start[None] + h * (end - start)[None]
