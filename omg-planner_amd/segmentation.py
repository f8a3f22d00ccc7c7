"""Object segmentation of carved states: connected components of the SURFACE nodes, and per component a cropped state volume
that fusion.distance_transform turns into a signed volume.  The specification of omgx_label_components /
omgx_component_records / omgx_component_states (include/omg_hip.h section 18; csrc/omg_segment_body.h holds the per-node rules)
in plain numpy.  Integers only: the kernels equal every array here exactly.

The reference splits an observed cloud into target and obstacles by the simulator's instance labels ("non-target points
only", omg/core.py:849-851).  A depth sensor gives no labels; here the carved states (fusion.carve_views) are split into
objects by connectivity, the target is the component nearest to a seed point, and the obstacle volume is the whole layout with
the target taken out.

Volumes, state_begin and the linear index L = (i * dims[1] + j) * dims[2] + k are fusion.py's.  Not part of the contract:
splitting objects that touch, colour, tracking labels from frame to frame.  (Unknown supports: planes.py.)
"""
from __future__ import annotations

import numpy as np

from . import fusion as _fu
from . import scenes as _sc

FREE, SURFACE, UNKNOWN = _fu.FREE, _fu.SURFACE, _fu.UNKNOWN
CONNECTIVITIES = (6, 18, 26)
RECORD_FIELDS = ("count", "first_L", "lo_i", "lo_j", "lo_k", "hi_i", "hi_j", "hi_k")
# The backward neighbours (di, dj, dk): the 13 offsets before (0, 0, 0) in x-major order, with the number of axes they move
# along.  Connectivity 6 takes those that move along one axis, 18 along at most two, 26 all.  The other half of a node's
# neighbours are these, negated.
BACKWARD = [(di, dj, dk) for di in (-1, 0) for dj in (-1, 0, 1) for dk in (-1, 0, 1) if (di, dj, dk) < (0, 0, 0)]


def backward_neighbours(connectivity: int):
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    order = {6: 1, 18: 2, 26: 3}[connectivity]
    return [o for o in BACKWARD if sum(1 for d in o if d) <= order]


def foreground(state, select: int = 1) -> np.ndarray:
    """bool per state: bit 0 of `select` selects SURFACE nodes, bit 1 nodes that are neither FREE nor SURFACE."""
    if select not in (1, 2, 3):
        raise ValueError(f"select must be 1, 2 or 3, got {select!r}")
    state = np.asarray(state)
    return ((state == SURFACE) & bool(select & 1)) | ((state != FREE) & (state != SURFACE) & bool(select & 2))


def _ranges(state_len, volumes, state_begin):
    vols = _fu._volumes(volumes)
    begin = _fu.state_offsets(volumes) if state_begin is None else np.asarray(state_begin, np.int64).reshape(-1)
    if len(begin) < len(vols):
        raise ValueError(f"state_begin must have one offset per volume ({len(vols)}), got {len(begin)}")
    sizes = [int(np.prod(v[3])) for v in vols]
    for m, n in enumerate(sizes):
        if begin[m] < 0 or begin[m] + n > state_len:
            raise ValueError(f"volume {m}: its states [{begin[m]}, {begin[m] + n}) leave the {state_len} given")
    return vols, begin, sizes


def _label_volume(fg: np.ndarray, offsets) -> np.ndarray:
    """Ranks of the components of one bool grid [X,Y,Z] -> int32 [X,Y,Z], -1 for background: every foreground node takes the
    smallest linear index it can reach (neighbour minimum and pointer jumping in turn, until nothing changes), the nodes that
    keep their own index are the components' first nodes, and a component's rank is the number of first nodes before its own."""
    n = fg.size
    own = np.arange(n, dtype=np.int64).reshape(fg.shape)
    lab = np.where(fg, own, n)
    both = [tuple(o) for o in offsets] + [tuple(-d for d in o) for o in offsets]
    while True:
        new = lab.copy()
        for o in both:
            a = tuple(slice(max(0, -d), fg.shape[x] - max(0, d)) for x, d in enumerate(o))   # the node
            b = tuple(slice(max(0, d), fg.shape[x] - max(0, -d)) for x, d in enumerate(o))   # its neighbour at + o
            new[a] = np.where(fg[a] & fg[b], np.minimum(new[a], lab[b]), new[a])
        flat, idx = new.reshape(-1), np.flatnonzero(fg.reshape(-1))
        while True:  # a node's value is the index of a node of its own component: follow it
            nxt = flat[flat[idx]]
            if np.array_equal(nxt, flat[idx]):
                break
            flat[idx] = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    first = fg & (lab == own)
    rank = np.cumsum(first.reshape(-1)) - 1
    out = np.full(n, -1, np.int32)
    idx = np.flatnonzero(fg.reshape(-1))
    out[idx] = rank[lab.reshape(-1)[idx]]
    return out.reshape(fg.shape)


def label_components(state, volumes, select: int = 1, connectivity: int = 6, state_begin=None) -> np.ndarray:
    """labels int32, one per state element: -1 for background nodes and for elements outside every volume's range, otherwise the
    rank 0, 1, ... of the node's component among the components of its own volume, ordered by their smallest linear index.
    Components never join across volumes."""
    offsets = backward_neighbours(connectivity)
    state = np.asarray(state, np.uint8).reshape(-1)
    fg = foreground(state, select)
    vols, begin, sizes = _ranges(len(state), volumes, state_begin)
    labels = np.full(len(state), -1, np.int32)
    for m, (_, _, _, dims) in enumerate(vols):
        b = int(begin[m])
        labels[b: b + sizes[m]] = _label_volume(fg[b: b + sizes[m]].reshape(dims), offsets).reshape(-1)
    return labels


def component_records(labels, volumes, state_begin=None):
    """(comp_begin [M+1] int64, records [C,8] int32): the components volume by volume in rank order, a row
    (count, first_L, lo_i, lo_j, lo_k, hi_i, hi_j, hi_k) with the box inclusive; volume m's rows are
    comp_begin[m] .. comp_begin[m+1]."""
    labels = np.asarray(labels, np.int32).reshape(-1)
    vols, begin, sizes = _ranges(len(labels), volumes, state_begin)
    comp_begin, rows = [0], []
    for m, (_, _, _, dims) in enumerate(vols):
        lab = labels[int(begin[m]): int(begin[m]) + sizes[m]]
        L = np.flatnonzero(lab >= 0)
        c = lab[L].astype(np.int64)
        n = int(c.max()) + 1 if len(c) else 0
        rec = np.zeros((n, 8), np.int64)
        if n:
            ijk = np.stack(np.unravel_index(L, dims), -1)
            rec[:, 0] = np.bincount(c, minlength=n)
            rec[:, 1:5], rec[:, 5:] = np.iinfo(np.int64).max, -1
            np.minimum.at(rec[:, 1], c, L)
            for a in range(3):
                np.minimum.at(rec[:, 2 + a], c, ijk[:, a])
                np.maximum.at(rec[:, 5 + a], c, ijk[:, a])
        rows.append(rec)
        comp_begin.append(comp_begin[-1] + n)
    records = np.concatenate(rows) if rows else np.zeros((0, 8), np.int64)
    return np.array(comp_begin, np.int64), records.astype(np.int32)


def check_picks(picks, num_volumes: int, comp_begin) -> np.ndarray:
    """picks [K,8] int32 = (source volume m, i0, j0, k0, component c as a row of records, mode, 0, 0), checked."""
    picks = np.asarray(picks, np.int64).reshape(-1, 8)
    comp_begin = np.asarray(comp_begin, np.int64).reshape(-1)
    for k, (m, _, _, _, c, mode, p0, p1) in enumerate(picks):
        if not 0 <= m < num_volumes:
            raise ValueError(f"pick {k}: volume {m} is not one of {num_volumes}")
        if not comp_begin[m] <= c < comp_begin[m + 1]:
            raise ValueError(f"pick {k}: component {c} is not a row of volume {m} ([{comp_begin[m]}, {comp_begin[m + 1]}))")
        if mode not in (0, 1) or p0 or p1:
            raise ValueError(f"pick {k}: mode must be 0 or 1 and the padding zero, got {mode}, {p0}, {p1}")
    return picks.astype(np.int32)


def component_states(state, volumes, state_begin, labels, comp_begin, records, picks, out_volumes, out_begin=None) -> np.ndarray:
    """uint8 states of K cropped output volumes, output k's node L at out_begin[k] + L (default: back to back); elements outside
    every output's range are UNKNOWN.  Output node (a,b,c) of pick (m, i0, j0, k0, c, mode) reads source node
    (i0+a, j0+b, k0+c) of volume m; outside the source grid: FREE.
    mode 0, the target alone: SURFACE if the source's label is component c; UNKNOWN if the source is neither FREE nor SURFACE
      and lies inside component c's box; FREE otherwise.
    mode 1, everything but the target: FREE if the source's label is component c, or if the source is neither FREE nor SURFACE
      and lies inside component c's box; otherwise the source state, unchanged."""
    state, labels = np.asarray(state, np.uint8).reshape(-1), np.asarray(labels, np.int32).reshape(-1)
    vols, begin, _ = _ranges(len(state), volumes, state_begin)
    if len(labels) != len(state):
        raise ValueError(f"{len(state)} states need as many labels, got {len(labels)}")
    comp_begin, records = np.asarray(comp_begin, np.int64).reshape(-1), np.asarray(records, np.int32).reshape(-1, 8)
    picks = check_picks(picks, len(vols), comp_begin)
    if comp_begin[-1] > len(records):
        raise ValueError(f"comp_begin names {comp_begin[-1]} records, {len(records)} given")
    outs = _fu._volumes(out_volumes)
    if len(outs) != len(picks):
        raise ValueError(f"{len(picks)} picks need as many output volumes, got {len(outs)}")
    ob = _fu.state_offsets(out_volumes) if out_begin is None else np.asarray(out_begin, np.int64).reshape(-1)
    sizes = [int(np.prod(v[3])) for v in outs]
    out = np.full(max([int(ob[k]) + sizes[k] for k in range(len(outs))], default=0), UNKNOWN, np.uint8)
    for k, (m, i0, j0, k0, c, mode, _, _) in enumerate(picks.tolist()):
        dims, odims = vols[m][3], outs[k][3]
        src = [np.arange(odims[a], dtype=np.int64) + (i0, j0, k0)[a] for a in range(3)]
        I, J, K = np.meshgrid(*src, indexing="ij")
        inside = (I >= 0) & (I < dims[0]) & (J >= 0) & (J < dims[1]) & (K >= 0) & (K < dims[2])
        L = np.where(inside, (I * dims[1] + J) * dims[2] + K, 0) + int(begin[m])
        s, lab = np.where(inside, state[L], FREE).astype(np.uint8), np.where(inside, labels[L], -1)
        r = records[c]
        box = inside & (I >= r[2]) & (I <= r[5]) & (J >= r[3]) & (J <= r[6]) & (K >= r[4]) & (K <= r[7])
        mine = lab == c - comp_begin[m]
        hidden = (s != FREE) & (s != SURFACE) & box
        if mode == 0:
            res = np.where(mine, SURFACE, np.where(hidden, UNKNOWN, FREE))
        else:
            res = np.where(mine | hidden, FREE, s)
        out[int(ob[k]): int(ob[k]) + sizes[k]] = res.astype(np.uint8).reshape(-1)
    return out


def crop_layout(volume, record, margin: int):
    """(origin [3], delta, dims [3], (i0, j0, k0)) of the record's box grown by `margin` nodes on every side: output node 0 sits
    where the source's node (i0, j0, k0) sits, with the source's sample position, so origin = source origin + (i0, j0, k0) * delta
    per component."""
    origin, delta = np.asarray(volume[0], np.float64).reshape(3), float(volume[1])
    r, margin = [int(x) for x in np.asarray(record).reshape(8)], int(margin)
    if margin < 0:
        raise ValueError("margin must not be negative")
    first = np.array([r[2] - margin, r[3] - margin, r[4] - margin], np.int64)
    dims = tuple(int(r[5 + a] - r[2 + a] + 1 + 2 * margin) for a in range(3))
    return origin + first.astype(np.float64) * delta, delta, dims, tuple(int(x) for x in first)


def pick_component(records, point_ijk, min_nodes: int = 1) -> int:
    """The rank of the component of ONE volume (records: its rows) with count >= min_nodes whose box is nearest to the point
    (index units; the squared distance in float64, 0 inside the box); ties go to the smaller rank."""
    records = np.asarray(records, np.int64).reshape(-1, 8)
    p = np.asarray(point_ijk, np.float64).reshape(3)
    if not np.isfinite(p).all():
        raise ValueError("the seed point is not finite")
    ok = np.flatnonzero(records[:, 0] >= int(min_nodes))
    if not len(ok):
        raise ValueError(f"no component has {int(min_nodes)} nodes or more ({len(records)} components)")
    lo, hi = records[ok, 2:5].astype(np.float64), records[ok, 5:8].astype(np.float64)
    gap = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    d2 = (gap[:, 0] * gap[:, 0] + gap[:, 1] * gap[:, 1]) + gap[:, 2] * gap[:, 2]
    return int(ok[int(np.argmin(d2))])  # (argmin: the first of equals)


def point_to_index(volume, point) -> np.ndarray:
    """A point of the layout's frame in index units: (point - origin) / delta - sample offset, float64."""
    origin, delta, sample = np.asarray(volume[0], np.float64).reshape(3), float(volume[1]), volume[2]
    return (np.asarray(point, np.float64).reshape(3) - origin) / delta - _sc.MESH_SAMPLE_OFFSET[sample]


def explained_mask(t, t_known, tol: float) -> np.ndarray:
    """The pixels that the known objects explain: t_known finite and t >= t_known - tol (camera.explained_mask in numpy)."""
    t, t_known = np.asarray(t, np.float64), np.asarray(t_known, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(t_known) & (t >= t_known - float(tol))


def segment_views(layout, views, depth, band: float, near: float, radius: int, seed, min_nodes: int, connectivity: int = 6,
                  margin=None, free_mask=None):
    """What DeviceScenes.segment_obstacles does for one scene, on the host: carve `layout` (origin, delta, dims: voxel centres)
    from the views, label the SURFACE nodes, pick the component nearest to `seed` (a point of the layout's frame) among those
    with at least min_nodes nodes, and transform its crop (mode 0) and the whole layout without it (mode 1) ->
    dict(state, labels, comp_begin, records, rank, record, target: SdfGrid, obstacle: SdfGrid, crop: crop_layout's tuple)."""
    origin, delta, dims = layout
    volume = (np.asarray(origin, np.float64), float(delta), "centre", tuple(int(d) for d in dims))
    depth = np.asarray(depth, np.float64)
    if free_mask is not None:
        depth = np.where(np.asarray(free_mask, bool), np.inf, depth)
    views = np.asarray(views, np.float64).reshape(-1, 16)
    state = _fu.carve_views([volume], views, [(0, len(views))], depth, band, near)
    labels = label_components(state, [volume], 1, connectivity)
    comp_begin, records = component_records(labels, [volume])
    rank = pick_component(records, point_to_index(volume, seed), min_nodes)
    margin = int(radius) + 1 if margin is None else int(margin)
    crop = crop_layout(volume, records[rank], margin)
    outs = [(crop[0], crop[1], "centre", crop[2]), volume]
    picks = [(0,) + crop[3] + (rank, 0, 0, 0), (0, 0, 0, 0, rank, 1, 0, 0)]
    cropped = component_states(state, [volume], None, labels, comp_begin, records, picks, outs)
    data = _fu.distance_transform(cropped, outs, radius, True)
    grids = [_sc.SdfGrid(data[k], np.asarray(outs[k][0], np.float64).copy(), outs[k][1]) for k in range(2)]
    return dict(state=state, labels=labels, comp_begin=comp_begin, records=records, rank=rank, record=records[rank].copy(),
                target=grids[0], obstacle=grids[1], crop=crop, cropped=cropped)
