"""Cases shared by the CPU and the GPU tests of object segmentation (omg-planner_amd/segmentation.py, csrc/omg_segment.hip):
named state grids with their known numbers of components, the ragged batch they form between guard bytes, picks for the cropped
volumes, scipy's labelling made canonical, and the observed scene of a sphere and a box on a slab."""
from __future__ import annotations

import functools

import numpy as np

from tests import fusion_cases as FC
from tests import mesh_cases as MC

N = 256  # OMGX_SEGMENT_NODES_PER_WORKGROUP (test_segment_cpu.py asserts it is the header's)
LONG = 2 * N + 44
CONNECTIVITIES = (6, 18, 26)
GUARD = 1  # the bytes between the volumes' states are SURFACE: they must come back -1 all the same


def _serpentine():
    """One 6-connected path through every other row of a 12 x 12 x 12 grid: the even planes i hold rows j = 0, 2, .. 10 along k,
    joined at alternating ends by a node of the odd rows; the odd planes hold one node that joins two even planes, alternately
    at (10, 0) and (0, 0).  6 * (72 + 5) + 5 = 467 nodes in a chain."""
    s = np.zeros((12, 12, 12), np.uint8)
    for i in range(0, 12, 2):
        s[i, 0::2, :] = 1
        for n, j in enumerate(range(1, 11, 2)):
            s[i, j, 11 if n % 2 == 0 else 0] = 1
        if i + 1 < 11:
            s[i + 1, 10 if (i // 2) % 2 == 0 else 0, 0] = 1
    return s


def _comb(spine: bool):
    """Teeth along x at every even (j, k) of a 40 x 7 x 5 grid; with the spine they join in the last plane only."""
    s = np.zeros((40, 7, 5), np.uint8)
    s[:, 0::2, 0::2] = 1
    if spine:
        s[-1] = 1
    else:
        s[-1] = 0
    return s


def _checkerboard():
    i, j, k = np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij")
    return ((i + j + k) % 2 == 0).astype(np.uint8)


def _cubes(corner: bool):
    s = np.zeros((5, 5, 5), np.uint8)
    s[0:2, 0:2, 0:2] = 1
    if corner:
        s[2:4, 2:4, 2:4] = 1
    else:
        s[2:4, 2:4, 0:2] = 1
    return s


def _random(dims, density, seed, values=(0, 2)):
    """Foreground (1) with this density; the background drawn from `values`."""
    rng = np.random.default_rng(seed)
    fg = rng.random(dims) < density
    return np.where(fg, 1, rng.choice(np.array(values, np.uint8), size=dims)).astype(np.uint8)


# name -> (states [X,Y,Z] uint8, the numbers of components of the SURFACE nodes under 6 / 18 / 26, or None where not written out)
@functools.lru_cache(maxsize=None)
def cases():
    c = {
        "serpentine": (_serpentine(), (1, 1, 1)),
        "comb": (_comb(True), (1, 1, 1)),
        "teeth": (_comb(False), (12, 12, 12)),
        "checkerboard": (_checkerboard(), (105, 1, 1)),
        "cubes_edge": (_cubes(False), (2, 1, 1)),
        "cubes_corner": (_cubes(True), (2, 2, 1)),
        "bar": (np.ones((3, LONG, 3), np.uint8), (1, 1, 1)),
        "line": (np.ones((LONG, 1, 1), np.uint8), (1, 1, 1)),
        "one_fg": (np.ones((1, 1, 1), np.uint8), (1, 1, 1)),
        "one_bg": (np.full((1, 1, 1), 2, np.uint8), (0, 0, 0)),
        "none": (_random((4, 5, 6), 0.0, 1), (0, 0, 0)),
        "all": (np.ones((4, 5, 6), np.uint8), (1, 1, 1)),
        "random15": (_random((20, 17, 23), 0.15, 15), None),
        "random31": (_random((20, 17, 23), 0.31, 31), None),
        "random60": (_random((20, 17, 23), 0.60, 60), None),
        "values": (_random((9, 10, 11), 0.3, 7, values=(0, 2, 3, 200, 255)), None),
        "big": (_random((64, 64, 40), 0.31, 64), None),
    }
    for n, dims in enumerate(((1, 1, 9), (1, 9, 1), (9, 1, 1), (1, 5, 6), (5, 1, 6), (5, 6, 1))):
        c["ones" + "x".join(map(str, dims))] = (_random(dims, 0.5, 100 + n), None)
    return c


SMALL = tuple(n for n in cases() if n != "big")
# the order of the ragged batch: "all" and then "bar" with no gap, so that a foreground last node is followed in the array by a
# foreground first node of another volume
BATCH = ("serpentine", "all", "bar", "comb", "teeth", "checkerboard", "cubes_edge", "cubes_corner", "line", "one_fg", "one_bg", "none",
         "random15", "random31", "random60", "values", "ones1x1x9", "ones1x9x1", "ones9x1x1", "ones1x5x6", "ones5x1x6", "ones5x6x1", "big")
GAPS = {"all": 0, "one_fg": 0, "one_bg": 1}  # elements after a volume's states (default 5)


def volume_of(state, m=0):
    return ((0.01 * m, -0.02, 0.0), 0.01, "centre" if m % 2 == 0 else "node", tuple(state.shape))


@functools.lru_cache(maxsize=None)
def batch():
    """(volumes, state with GUARD between and around the volumes' states, state_begin int64 [M])"""
    grids = [cases()[n][0] for n in BATCH]
    volumes = [volume_of(g, m) for m, g in enumerate(grids)]
    begin, parts, at = [], [np.full(3, GUARD, np.uint8)], 3
    for n, g in zip(BATCH, grids):
        begin.append(at)
        gap = GAPS.get(n, 5)
        parts += [g.ravel(), np.full(gap, GUARD, np.uint8)]
        at += g.size + gap
    state = np.concatenate(parts)
    a, b = BATCH.index("all"), BATCH.index("bar")
    assert begin[a] + grids[a].size == begin[b] and state[begin[b] - 1] == 1 and state[begin[b]] == 1
    return volumes, state, np.array(begin, np.int64)


def picks_for(volumes, comp_begin, records, seed=0, per_volume=2, margin=2):
    """Picks over a labelled batch -> (picks [K,8] int32, out_volumes, out_begin with gaps): per volume that has a component, the
    crop of a drawn component grown by `margin` (negative offsets, crops that hang over the grid) in mode 0 and in mode 1, and a
    pick at drawn offsets with drawn dims."""
    from omg_planner_amd import segmentation as sg
    rng = np.random.default_rng(seed)
    picks, outs = [], []
    for m, v in enumerate(volumes):
        n = int(comp_begin[m + 1] - comp_begin[m])
        if n == 0:
            continue
        for _ in range(per_volume):
            c = int(comp_begin[m]) + int(rng.integers(n))
            origin, delta, dims, first = sg.crop_layout(v, records[c], margin)
            for mode in (0, 1):
                picks.append((m,) + first + (c, mode, 0, 0))
                outs.append((origin, delta, "centre", dims))
        dims = tuple(int(x) for x in rng.integers(1, 7, 3))
        first = tuple(int(x) for x in rng.integers(-3, 4, 3))
        picks.append((m,) + first + (int(comp_begin[m]) + int(rng.integers(n)), int(rng.integers(2)), 0, 0))
        outs.append(((0.0, 0.0, 0.0), 0.01, "node", dims))
    sizes = [int(np.prod(o[3])) for o in outs]
    begin = np.cumsum([2] + [s + 3 for s in sizes])[:-1].astype(np.int64)
    return np.array(picks, np.int32).reshape(-1, 8), outs, begin


def structure(connectivity):
    """scipy's structuring element of a connectivity."""
    from scipy import ndimage
    return ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])


def scipy_labels(fg, connectivity):
    """scipy.ndimage.label made canonical: components renumbered by their smallest linear index -> (int32 [X,Y,Z] with -1 as
    background, count).  scipy's own numbering is not relied on."""
    from scipy import ndimage
    lab, n = ndimage.label(fg, structure(connectivity))
    flat = lab.ravel()
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    order = np.argsort(first[1:], kind="stable")
    rank = np.empty(n + 1, np.int64)
    rank[0] = -1
    rank[1 + order] = np.arange(n)
    return rank[lab].astype(np.int32), n


def scipy_records(fg, connectivity):
    """records [C,8] from scipy.ndimage.find_objects and bincount, in canonical order."""
    from scipy import ndimage
    lab, n = ndimage.label(fg, structure(connectivity))
    canon, _ = scipy_labels(fg, connectivity)
    rec = np.zeros((n, 8), np.int32)
    counts = np.bincount(lab.ravel(), minlength=n + 1)
    for c, sl in enumerate(ndimage.find_objects(lab), 1):
        where = np.flatnonzero(lab.ravel() == c)
        r = canon.ravel()[where[0]]
        rec[r] = (counts[c], where[0], sl[0].start, sl[1].start, sl[2].start, sl[0].stop - 1, sl[1].stop - 1, sl[2].stop - 1)
    return rec


# ---------------------------------------------------------------------------------------------------------------------
# the observed scene: a sphere and a box standing on a slab, FC's three cameras, FC's grid
# ---------------------------------------------------------------------------------------------------------------------
SLAB_HALF = (0.25, 0.25, 0.01)
SPHERE_R, SPHERE_C = 0.04, (-0.06, 0.0, 0.05)
BOX_HALF, BOX_C = (0.03, 0.03, 0.04), (0.07, 0.0, 0.05)
LAYOUT = (FC.ORIGIN, FC.DELTA, FC.DIMS)
BAND, NEAR, REACH, TOL, MIN_NODES = FC.BAND, FC.NEAR, 0.1, 0.004, 100
SEED_POINT = (-0.06, 0.0, 0.06)  # somewhere in the sphere


@functools.lru_cache(maxsize=None)
def observed_meshes():
    return [MC.icosphere(2, SPHERE_R, SPHERE_C), MC.box_mesh(BOX_HALF, MC.pose(t=BOX_C)), MC.box_mesh(SLAB_HALF)]


@functools.lru_cache(maxsize=None)
def observed_records(which=(0, 1, 2)):
    """What camera.render_depth / ops.CameraBatch take for FC's three cameras as three `scenes` of the instances `which`."""
    from omg_planner_amd import camera
    cfw, intr = FC.scene_cameras()
    meshes = observed_meshes()
    n = len(which)
    recs = [camera.instance_records(meshes, list(which), [np.eye(4)] * n, [1] * n, cfw[s]) for s in range(3)]
    cams = np.stack([camera.camera_rows(intr, cfw[s]) for s in range(3)])
    return meshes, np.concatenate(recs), np.arange(4, dtype=np.int64) * n, cams


@functools.lru_cache(maxsize=None)
def observed_depth():
    """(t [3,H,W] of the whole scene, t_known [3,H,W] of the slab alone, view rows [3,16]): camera.render_depth, the
    specification."""
    from omg_planner_amd import camera, fusion
    out = []
    for which in ((0, 1, 2), (2,)):
        meshes, inst, begin, cams = observed_records(which)
        out.append(camera.render_depth(meshes, inst, begin, cams, FC.H, FC.W)[0])
    cfw, intr = FC.scene_cameras()
    return out[0], out[1], np.stack([fusion.view_rows(intr, cfw[s]) for s in range(3)])


@functools.lru_cache(maxsize=None)
def observed_segmentation(connectivity=6):
    """segmentation.segment_views of the observed scene with the slab's pixels masked out."""
    from omg_planner_amd import fusion, segmentation as sg
    t, t_known, views = observed_depth()
    radius = fusion.obstacle_radius(REACH, FC.DELTA)
    return sg.segment_views(LAYOUT, views, t, BAND, NEAR, radius, SEED_POINT, MIN_NODES, connectivity, free_mask=sg.explained_mask(t, t_known, TOL))
