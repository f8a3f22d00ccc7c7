"""CPU tests of object segmentation (omg-planner_amd/segmentation.py, csrc/omg_segment.hip): the
specification against scipy.ndimage and against the answers written out; the cropped states as known answers; the observed scene
of a sphere and a box on a slab; csrc/omg_segment_body.h compiled for the host and walked in the kernels' order equals the
specification; every argument error of the C ABI and of the wrappers; the kernels use no scratch."""
from __future__ import annotations

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import kernel_build as KB
from tests import segment_cases as SC


# ---------------------------------------------------------------------------------------------------------------------
# 1. the specification: scipy, known answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.cases()))
def test_labels_and_records_against_scipy(name):
    """Labels equal scipy.ndimage.label's components renumbered by smallest linear index, records equal find_objects and
    bincount, for the three structuring elements and the three select values."""
    pytest.importorskip("scipy.ndimage")
    from omg_planner_amd import segmentation as sg
    s, _ = SC.cases()[name]
    vol = [SC.volume_of(s)]
    for conn in SC.CONNECTIVITIES:
        for select in (1, 2, 3):
            fg = sg.foreground(s, select)
            assert np.array_equal(fg, ((s == 1) & bool(select & 1)) | ((s >= 2) & bool(select & 2)))
            want, n = SC.scipy_labels(fg, conn)
            got = sg.label_components(s.ravel(), vol, select, conn)
            assert got.dtype == np.int32 and np.array_equal(got.reshape(s.shape), want), (name, conn, select)
            comp_begin, records = sg.component_records(got, vol)
            assert comp_begin.tolist() == [0, n] and records.dtype == np.int32
            assert np.array_equal(records, SC.scipy_records(fg, conn)), (name, conn, select)


def test_known_numbers_of_components():
    """The answers written out in tests/segment_cases.py, and the structure of the serpentine: one chain of 467 links whose
    nodes have at most two neighbours."""
    from omg_planner_amd import segmentation as sg
    seen = 0
    for name, (s, known) in SC.cases().items():
        if known is None:
            continue
        for conn, want in zip(SC.CONNECTIVITIES, known):
            lab = sg.label_components(s.ravel(), [SC.volume_of(s)], 1, conn)
            assert (lab.max() + 1 if (lab >= 0).any() else 0) == want, (name, conn)
            assert ((lab >= 0) == (s.ravel() == 1)).all()
            seen += 1
    assert seen == 36
    snake = SC.cases()["serpentine"][0]
    assert snake.sum() == 467
    pad = np.pad(snake.astype(np.int64), 1)
    nb = sum(np.roll(pad, sh, ax) for ax in range(3) for sh in (-1, 1))[1:-1, 1:-1, 1:-1]
    assert sorted(np.bincount(nb[snake == 1]).tolist()) == [0, 2, 465]  # two ends, everything else has two neighbours
    assert SC.cases()["checkerboard"][0].sum() == 105
    # components never join across volumes; elements outside every range are -1 whatever they hold
    volumes, state, begin = SC.batch()
    for conn in (6, 26):
        lab = sg.label_components(state, volumes, 1, conn, state_begin=begin)
        inside = np.zeros(len(state), bool)
        for m, v in enumerate(volumes):
            n = int(np.prod(v[3]))
            inside[begin[m]: begin[m] + n] = True
            assert np.array_equal(lab[begin[m]: begin[m] + n], sg.label_components(state[begin[m]: begin[m] + n], [v], 1, conn)), (m, conn)
        assert (~inside).sum() > 50 and (state[~inside] == SC.GUARD).all() and (lab[~inside] == -1).all()
        a = SC.BATCH.index("all")
        assert lab[begin[a + 1] - 1] == 0 and lab[begin[a + 1]] == 0  # the last node of one volume, the first of the next: rank 0 of each
    for bad in (dict(select=0), dict(select=4), dict(connectivity=8), dict(connectivity=4)):
        with pytest.raises(ValueError):
            sg.label_components(np.zeros(8, np.uint8), [((0, 0, 0), 0.01, "centre", (2, 2, 2))], **bad)
    with pytest.raises(ValueError):
        sg.label_components(np.zeros(7, np.uint8), [((0, 0, 0), 0.01, "centre", (2, 2, 2))])


def test_component_states_known_answers():
    """Both modes, negative offsets, crops that hang over the grid, the box rule for UNKNOWN, and in mode 1 a neighbour's SURFACE
    nodes inside the target's box, which stay."""
    from omg_planner_amd import segmentation as sg
    F, S, U = sg.FREE, sg.SURFACE, sg.UNKNOWN
    # one row of 8 nodes along z: component 0 = nodes 1..2, UNKNOWN behind it at 3 (outside its box), component 1 = 5..6
    row = np.array([F, S, S, U, F, S, S, U], np.uint8)
    vol = [((0.0, 0.0, 0.0), 0.01, "node", (1, 1, 8))]
    lab = sg.label_components(row, vol)
    cb, rec = sg.component_records(lab, vol)
    assert lab.tolist() == [-1, 0, 0, -1, -1, 1, 1, -1] and cb.tolist() == [0, 2]
    assert rec.tolist() == [[2, 1, 0, 0, 1, 0, 0, 2], [2, 5, 0, 0, 5, 0, 0, 6]]

    def crop(pick, dims):
        return sg.component_states(row, vol, None, lab, cb, rec, [pick], [((0.0, 0.0, 0.0), 0.01, "node", dims)]).tolist()

    assert crop((0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 8)) == [F, S, S, F, F, F, F, F]     # the target alone; UNKNOWN outside the box: FREE
    assert crop((0, 0, 0, 0, 1, 0, 0, 0), (1, 1, 8)) == [F, F, F, F, F, S, S, F]
    assert crop((0, 0, 0, 0, 0, 1, 0, 0), (1, 1, 8)) == [F, F, F, U, F, S, S, U]     # everything but the target
    assert crop((0, 0, 0, -2, 0, 0, 0, 0), (1, 1, 5)) == [F, F, F, S, S]             # a negative offset: outside is FREE
    assert crop((0, 0, 0, 6, 1, 1, 0, 0), (1, 1, 4)) == [F, U, F, F]                 # hangs over the end: FREE in mode 1 as well
    assert crop((0, -1, 0, 0, 0, 1, 0, 0), (3, 1, 2)) == [F, F, F, F, F, F]          # the rows beside the grid
    # a shell: SURFACE around an UNKNOWN core, and a second object's SURFACE inside the first one's box
    g = np.zeros((5, 5, 5), np.uint8)
    g[0:4, 0:4, 0:4] = S
    g[1:3, 1:3, 1:3] = U
    g[4, 4, 4] = U            # unknown space outside the box
    g[3, 3, 3] = F            # a corner of the shell is missing
    vol3 = [((0.0, 0.0, 0.0), 0.01, "centre", (5, 5, 5))]
    lab3 = sg.label_components(g.ravel(), vol3)
    cb3, rec3 = sg.component_records(lab3, vol3)
    assert cb3.tolist() == [0, 1] and rec3[0].tolist() == [4 * 4 * 4 - 8 - 1, 0, 0, 0, 0, 3, 3, 3]
    whole = ((0.0, 0.0, 0.0), 0.01, "centre", (5, 5, 5))
    t = sg.component_states(g.ravel(), vol3, None, lab3, cb3, rec3, [(0, 0, 0, 0, 0, 0, 0, 0)], [whole]).reshape(5, 5, 5)
    assert (t[1:3, 1:3, 1:3] == U).all() and t[4, 4, 4] == F and t[3, 3, 3] == F and (t == S).sum() == 55
    o = sg.component_states(g.ravel(), vol3, None, lab3, cb3, rec3, [(0, 0, 0, 0, 0, 1, 0, 0)], [whole]).reshape(5, 5, 5)
    assert (o[0:4, 0:4, 0:4] == F).all() and o[4, 4, 4] == U and (o == U).sum() == 1
    # an L-shaped target whose box holds a neighbour: the neighbour's SURFACE stays in mode 1, its UNKNOWN inside the box goes
    e = np.zeros((1, 4, 4), np.uint8)
    e[0, 0, :] = S
    e[0, :, 0] = S
    e[0, 2, 2] = S            # the neighbour, inside the L's box
    e[0, 3, 3] = U
    e[0, 2, 3] = 7            # neither FREE nor SURFACE: hidden as UNKNOWN is
    vole = [((0.0, 0.0, 0.0), 0.01, "centre", (1, 4, 4))]
    labe = sg.label_components(e.ravel(), vole)
    cbe, rece = sg.component_records(labe, vole)
    assert cbe.tolist() == [0, 2] and rece.tolist() == [[7, 0, 0, 0, 0, 0, 3, 3], [1, 10, 0, 2, 2, 0, 2, 2]]
    out = ((0.0, 0.0, 0.0), 0.01, "centre", (1, 4, 4))
    m1 = sg.component_states(e.ravel(), vole, None, labe, cbe, rece, [(0, 0, 0, 0, 0, 1, 0, 0)], [out]).reshape(4, 4)
    assert m1.tolist() == [[F, F, F, F], [F, F, F, F], [F, F, S, F], [F, F, F, F]]
    m0 = sg.component_states(e.ravel(), vole, None, labe, cbe, rece, [(0, 0, 0, 0, 0, 0, 0, 0)], [out]).reshape(4, 4)
    assert m0.tolist() == [[S, S, S, S], [S, F, F, F], [S, F, F, U], [S, F, F, U]]
    m1b = sg.component_states(e.ravel(), vole, None, labe, cbe, rece, [(0, 0, 0, 0, 1, 1, 0, 0)], [out]).reshape(4, 4)
    assert m1b.tolist() == [[S, S, S, S], [S, F, F, F], [S, F, F, 7], [S, F, F, U]]  # the neighbour's box is one node
    # two outputs at the caller's offsets; what lies between is UNKNOWN
    two = sg.component_states(row, vol, None, lab, cb, rec, [(0, 0, 0, 1, 0, 0, 0, 0), (0, 0, 0, 5, 1, 0, 0, 0)],
                              [((0.0, 0.0, 0.0), 0.01, "node", (1, 1, 2))] * 2, [1, 4])
    assert two.tolist() == [U, S, S, U, S, S]
    for bad in ((1, 0, 0, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 2, 0, 0, 0), (0, 0, 0, 0, -1, 0, 0, 0), (0, 0, 0, 0, 0, 2, 0, 0),
                (0, 0, 0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 0, 0, 1)):
        with pytest.raises(ValueError):
            crop(bad, (1, 1, 2))
    # a component of another volume
    two_vols = vol + [((0.0, 0.0, 0.0), 0.01, "node", (1, 1, 2))]
    st = np.concatenate([row, [S, S]]).astype(np.uint8)
    lab2 = sg.label_components(st, two_vols)
    cb2, rec2 = sg.component_records(lab2, two_vols)
    assert cb2.tolist() == [0, 2, 3]
    with pytest.raises(ValueError):
        sg.component_states(st, two_vols, None, lab2, cb2, rec2, [(0, 0, 0, 0, 2, 0, 0, 0)], [out])
    with pytest.raises(ValueError):
        sg.component_states(st, two_vols, None, lab2, cb2, rec2, [(1, 0, 0, 0, 1, 0, 0, 0)], [out])


def test_crop_layout_and_pick_component():
    from omg_planner_amd import segmentation as sg
    vol = ((0.1, -0.2, 0.3), 0.5, "centre", (10, 10, 10))
    origin, delta, dims, first = sg.crop_layout(vol, (5, 123, 2, 3, 4, 4, 3, 9), 2)
    assert first == (0, 1, 2) and dims == (7, 5, 10) and delta == 0.5 and origin.tolist() == [0.1, -0.2 + 1 * 0.5, 0.3 + 2 * 0.5]
    origin, _, dims, first = sg.crop_layout(vol, (5, 123, 0, 0, 0, 0, 0, 0), 3)
    assert first == (-3, -3, -3) and dims == (7, 7, 7) and origin.tolist() == [0.1 + -3.0 * 0.5, -0.2 + -3.0 * 0.5, 0.3 + -3.0 * 0.5]
    assert sg.crop_layout(vol, (1, 0, 1, 1, 1, 1, 1, 1), 0)[2:] == ((1, 1, 1), (1, 1, 1))
    with pytest.raises(ValueError):
        sg.crop_layout(vol, (1, 0, 1, 1, 1, 1, 1, 1), -1)
    recs = np.array([[50, 0, 0, 0, 0, 2, 2, 2], [3, 9, 4, 4, 4, 5, 5, 5], [60, 20, 8, 0, 0, 9, 2, 2], [70, 30, 0, 6, 0, 2, 9, 2]], np.int32)
    assert sg.pick_component(recs, (1.0, 1.0, 1.0), 1) == 0      # inside a box: distance 0
    assert sg.pick_component(recs, (4.5, 4.5, 4.5), 1) == 1
    assert sg.pick_component(recs, (4.5, 4.5, 4.5), 4) == 3      # the small one is not considered: 18.75 to box 0, 24.75 to box 2, 14.75 to box 3
    assert sg.pick_component(recs, (5.0, 1.0, 1.0), 4) == 0      # 3 to box 0 and 3 to box 2: the smaller rank
    assert sg.pick_component(recs, (5.5, 1.0, 1.0), 4) == 2
    assert sg.pick_component(recs, (1.0, 4.0, 1.0), 60) == 3 and sg.pick_component(recs, (100.0, -100.0, 7.0), 70) == 3
    with pytest.raises(ValueError):
        sg.pick_component(recs, (1.0, 1.0, 1.0), 71)
    with pytest.raises(ValueError):
        sg.pick_component(recs[:0], (1.0, 1.0, 1.0), 1)
    with pytest.raises(ValueError):
        sg.pick_component(recs, (1.0, float("nan"), 1.0), 1)
    assert np.allclose(sg.point_to_index(vol, (0.1 + 0.75, -0.2 + 0.25, 0.3 + 2.25)), [1.0, 0.0, 4.0], rtol=0, atol=1e-12)
    assert np.allclose(sg.point_to_index(vol[:2] + ("node",), (0.1 + 0.75, -0.2, 0.3)), [1.5, 0.0, 0.0], rtol=0, atol=1e-12)
    t, k = np.array([1.0, 2.0, np.inf, 0.5, np.nan]), np.array([1.003, np.inf, 3.0, 1.0, 1.0])
    assert sg.explained_mask(t, k, 0.004).tolist() == [True, False, True, False, False]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the observed scene
# ---------------------------------------------------------------------------------------------------------------------
def test_observed_scene_of_a_sphere_and_a_box_on_a_slab():
    """icosphere(2, 0.04) at (-0.06, 0, 0.05) and a box of 6 x 6 x 8 cm at (0.07, 0, 0.05) on the slab of fusion's scene, its three
    64 x 48 cameras and its 32 x 32 x 24 grid of 1 cm; the slab's pixels taken out by explained_mask of the slab's own rendering.
    The specification gives exactly two components of at least MIN_NODES = 100 nodes (measured: 416, the box, and 286, the
    sphere) and everything else below it (measured: two single nodes); the seeded pick is the sphere; its mode-0 volume has a
    closed, non-empty zero level; the mode-1 volume is positive at the sphere's centre and negative in the box."""
    from omg_planner_amd import fusion, scenes, segmentation as sg
    t, t_known, views = SC.observed_depth()
    mask = sg.explained_mask(t, t_known, SC.TOL)
    assert 0.2 < mask.mean() < 0.9 and (np.isfinite(t) & ~mask).mean() > 0.03  # the slab is seen and goes; the objects stay
    unmasked = fusion.carve_views([SC.LAYOUT[:2] + ("centre", SC.LAYOUT[2])], views, [(0, 3)], t, SC.BAND, SC.NEAR)
    welded = sg.component_records(sg.label_components(unmasked, [SC.LAYOUT[:2] + ("centre", SC.LAYOUT[2])]), [SC.LAYOUT[:2] + ("centre", SC.LAYOUT[2])])[1]
    slab = welded[np.argmax(welded[:, 0])]  # without the mask the slab is the largest component and holds the box that stands on it
    top_of_box = sg.point_to_index((SC.LAYOUT[0], SC.LAYOUT[1], "centre"), (SC.BOX_C[0], SC.BOX_C[1], SC.BOX_C[2] + SC.BOX_HALF[2]))
    assert slab[2] == 0 and slab[5] == FC.DIMS[0] - 1 and slab[3] == 0 and slab[6] == FC.DIMS[1] - 1 and slab[7] >= np.floor(top_of_box[2])
    for conn in SC.CONNECTIVITIES:
        r = SC.observed_segmentation(conn)
        counts = np.sort(r["records"][:, 0])[::-1]
        print(conn, "components", counts.tolist(), "picked", r["rank"], r["record"].tolist(), "crop", r["crop"][2])
        assert (counts >= SC.MIN_NODES).sum() == 2 and (counts[2:] < SC.MIN_NODES // 10).all()
        lo, hi = r["record"][2:5], r["record"][5:8]
        centre = sg.point_to_index((SC.LAYOUT[0], SC.LAYOUT[1], "centre"), SC.SPHERE_C)
        box_centre = sg.point_to_index((SC.LAYOUT[0], SC.LAYOUT[1], "centre"), SC.BOX_C)
        assert (lo <= centre).all() and (centre <= hi).all() and not ((lo <= box_centre).all() and (box_centre <= hi).all())
        assert np.abs((hi - lo + 1) * FC.DELTA - 2 * SC.SPHERE_R).max() <= 3 * FC.DELTA
        radius = fusion.obstacle_radius(SC.REACH, FC.DELTA)
        assert r["crop"][2] == tuple(int(h - l + 1 + 2 * (radius + 1)) for l, h in zip(lo, hi))
        v, f, open_edges = scenes.surface_nets(r["target"].data, r["target"].origin, r["target"].delta, "centre", 0.0)
        assert open_edges == 0 and len(v) > 100 and len(f) > 200
        assert np.abs(v - np.array(SC.SPHERE_C)).max() < SC.SPHERE_R + 3 * FC.DELTA   # the mesh is the sphere, nothing else
        at = lambda g, p: g.data[tuple(np.floor((np.array(p) - g.origin) / g.delta).astype(int))]
        assert at(r["obstacle"], SC.SPHERE_C) > 0 and at(r["obstacle"], SC.BOX_C) < 0 and at(r["target"], SC.SPHERE_C) < 0
        assert r["obstacle"].data.shape == FC.DIMS and np.array_equal(r["obstacle"].origin, FC.ORIGIN)


# ---------------------------------------------------------------------------------------------------------------------
# 3. csrc/omg_segment_body.h on the host
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include <vector>
#include "omg_segment_body.h"
static void node_of(int64_t id, const int32_t* n, int* i, int* j, int* k) {
    *i = (int)(id / ((int64_t)n[1] * n[2])), *j = (int)(id / n[2] % n[1]), *k = (int)(id % n[2]);
}
// One volume in the kernels' order, run by run of `block` nodes: k_label_local (links in a table of the run's own), k_label_border
// (the volume's table), then the first nodes counted run by run, scanned, and every node's root's rank written.  Returns the
// number of components.
extern "C" int host_label(const uint8_t* state, const int32_t* n, int select, int connectivity, int block, int32_t* parent, int32_t* labels) {
    const int64_t total = (int64_t)n[0] * n[1] * n[2], runs = (total + block - 1) / block;
    const int order = seg_order(connectivity);
    std::vector<int32_t> link(block);
    for (int64_t r = 0; r < runs; ++r) {
        const int64_t id0 = r * block;
        for (int me = 0; me < block; ++me) link[me] = id0 + me < total && seg_foreground(state[id0 + me], select) ? me : SEG_BACKGROUND;
        for (int me = 0; me < block; ++me) {
            if (link[me] == SEG_BACKGROUND) continue;
            int i, j, k;
            node_of(id0 + me, n, &i, &j, &k);
            for (int b = 0; b < SEG_BACKWARD; ++b) {
                int64_t q;
                if (!seg_neighbour(b, order, n, i, j, k, &q) || q < id0) continue;
                if (seg_load<SEG_SCOPE_WORKGROUP>(&link[q - id0]) != SEG_BACKGROUND) seg_union<SEG_SCOPE_WORKGROUP>(link.data(), me, (int)(q - id0));
            }
        }
        for (int me = 0; me < block && id0 + me < total; ++me)
            parent[id0 + me] = link[me] == SEG_BACKGROUND ? SEG_BACKGROUND : (int32_t)id0 + seg_find<SEG_SCOPE_WORKGROUP>(link.data(), me);
    }
    for (int64_t r = 1; r < runs; ++r)
        for (int64_t id = r * block; id < total && id < (r + 1) * block; ++id) {
            if (seg_load<SEG_SCOPE_AGENT>(parent + id) == SEG_BACKGROUND) continue;
            int i, j, k;
            node_of(id, n, &i, &j, &k);
            for (int b = 0; b < SEG_BACKWARD; ++b) {
                int64_t q;
                if (!seg_neighbour(b, order, n, i, j, k, &q) || q >= r * block) continue;
                if (seg_load<SEG_SCOPE_AGENT>(parent + q) != SEG_BACKGROUND) seg_union<SEG_SCOPE_AGENT>(parent, (int32_t)id, (int32_t)q);
            }
        }
    std::vector<int32_t> before(runs + 1, 0), rank(total, 0);
    for (int64_t r = 0; r < runs; ++r) {
        int firsts = 0;
        for (int64_t id = r * block; id < total && id < (r + 1) * block; ++id)
            if (parent[id] == id) rank[id] = firsts++;
        before[r + 1] = before[r] + firsts;
    }
    for (int64_t id = 0; id < total; ++id) {
        if (parent[id] == SEG_BACKGROUND) { labels[id] = SEG_BACKGROUND; continue; }
        const int32_t root = seg_find<SEG_SCOPE_PLAIN>(parent, (int32_t)id);
        labels[id] = before[root / block] + rank[root];
    }
    return before[runs];
}
// k_records_init and k_records_fill, node by node.
extern "C" void host_records(const int32_t* labels, const int32_t* n, int rows, int32_t* rec) {
    for (int r = 0; r < rows; ++r) {
        rec[r * 8] = 0;
        for (int c = 1; c < 5; ++c) rec[r * 8 + c] = 0x7fffffff;
        for (int c = 5; c < 8; ++c) rec[r * 8 + c] = -1;
    }
    const int64_t total = (int64_t)n[0] * n[1] * n[2];
    for (int64_t id = 0; id < total; ++id) {
        if (labels[id] < 0 || labels[id] >= rows) continue;
        int at[3];
        node_of(id, n, at, at + 1, at + 2);
        int32_t* r = rec + labels[id] * 8;
        r[0] += 1;
        if (id < r[1]) r[1] = (int32_t)id;
        for (int a = 0; a < 3; ++a) {
            if (at[a] < r[2 + a]) r[2 + a] = at[a];
            if (at[a] > r[5 + a]) r[5 + a] = at[a];
        }
    }
}
// k_component_states for one output volume whose source is one volume with ranks `labels` and the records `rec` of its own.
extern "C" void host_states(const uint8_t* state, const int32_t* labels, const int32_t* n, const int32_t* rec, const int32_t* pick,
                            const int32_t* on, uint8_t* out) {
    int64_t id = 0;
    for (int a = 0; a < on[0]; ++a)
        for (int b = 0; b < on[1]; ++b)
            for (int c = 0; c < on[2]; ++c, ++id) {
                const int64_t si = (int64_t)pick[1] + a, sj = (int64_t)pick[2] + b, sk = (int64_t)pick[3] + c;
                const bool in_grid = si >= 0 && si < n[0] && sj >= 0 && sj < n[1] && sk >= 0 && sk < n[2];
                const int64_t at = in_grid ? (si * n[1] + sj) * n[2] + sk : 0;
                out[id] = seg_pick_state(in_grid, in_grid ? state[at] : (uint8_t)SEG_FREE, in_grid ? labels[at] : SEG_BACKGROUND, pick[4],
                                         rec + (int64_t)pick[4] * 8, (int)si, (int)sj, (int)sk, pick[5]);
            }
}
"""


def _host_lib(tmp_path):
    vp, i = C.c_void_p, C.c_int
    return KB.host_harness(_HOST_HARNESS, tmp_path, {"host_label": (i, [vp, vp, i, i, i, vp, vp]), "host_records": (None, [vp, vp, i, vp]),
                                                     "host_states": (None, [vp, vp, vp, vp, vp, vp, vp])})


def host_segment(lib, state, select, connectivity, block=SC.N):
    """(labels [n] int32, records [C,8] int32) of one volume's states [X,Y,Z] through the body header."""
    state = np.ascontiguousarray(state, np.uint8)
    n = np.array(state.shape, np.int32)
    parent, labels = np.full(state.size, -9, np.int32), np.full(state.size, -9, np.int32)
    count = lib.host_label(state.ctypes.data, n.ctypes.data, select, connectivity, block, parent.ctypes.data, labels.ctypes.data)
    rec = np.full((count, 8), -9, np.int32)
    lib.host_records(labels.ctypes.data, n.ctypes.data, count, rec.ctypes.data)
    return labels, rec


def host_states(lib, state, labels, rec, pick, out_dims):
    """One output volume; pick = (_, i0, j0, k0, the component's LOCAL rank, mode, 0, 0)."""
    state, labels, rec = np.ascontiguousarray(state, np.uint8), np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(rec, np.int32)
    n, on, pick = np.array(state.shape, np.int32), np.array(out_dims, np.int32), np.array(pick, np.int32)
    out = np.full(int(on.prod()), 9, np.uint8)
    lib.host_states(state.ctypes.data, labels.ctypes.data, n.ctypes.data, rec.ctypes.data if len(rec) else None, pick.ctypes.data, on.ctypes.data,
                    out.ctypes.data)
    return out


def _against_the_specification(lib, volumes, state, begin, select, conn, pick_seed):
    """Every volume of a batch through the host harness against the specification of the whole batch -> nodes compared."""
    from omg_planner_amd import segmentation as sg
    want = sg.label_components(state, volumes, select, conn, state_begin=begin)
    comp_begin, records = sg.component_records(want, volumes, begin)
    picks, outs, ob = SC.picks_for(volumes, comp_begin, records, seed=pick_seed)
    cropped = sg.component_states(state, volumes, begin, want, comp_begin, records, picks, outs, ob)
    got = {}
    for m, v in enumerate(volumes):
        n, b = int(np.prod(v[3])), int(begin[m])
        got[m] = host_segment(lib, state[b: b + n].reshape(v[3]), select, conn)
        assert np.array_equal(got[m][0], want[b: b + n]), (m, v[3], select, conn)
        assert np.array_equal(got[m][1], records[comp_begin[m]: comp_begin[m + 1]]), (m, v[3], select, conn)
    for k, p in enumerate(picks.tolist()):
        m, b = p[0], int(begin[p[0]])
        local = p[:4] + [p[4] - int(comp_begin[m])] + p[5:]
        out = host_states(lib, state[b: b + int(np.prod(volumes[m][3]))].reshape(volumes[m][3]), got[m][0], got[m][1], local, outs[k][3])
        assert np.array_equal(out, cropped[int(ob[k]): int(ob[k]) + out.size]), (k, p)
    return int(sum(np.prod(v[3]) for v in volumes)), len(picks)


@KB.requires_host_cxx
def test_kernel_body_compiled_for_the_host_equals_the_specification(tmp_path):
    """csrc/omg_segment_body.h holds what a thread of the kernels does for its node; compiled for the host and walked in the
    kernels' order (run by run of N = 256 nodes: links inside the run, then across the borders, then the ranks) it gives the
    specification's labels, records and cropped states on every case, for the three connectivities and select values; a run of 7
    nodes gives the same (more borders)."""
    from omg_planner_amd import _lib, segmentation as sg
    assert _lib.SEGMENT_NODES_PER_WORKGROUP == SC.N
    lib = _host_lib(tmp_path)
    volumes, state, begin = SC.batch()
    nodes = picks = 0
    for conn in SC.CONNECTIVITIES:
        a, b = _against_the_specification(lib, volumes, state, begin, 1, conn, conn)
        nodes, picks = nodes + a, picks + b
    small = [m for m, n in enumerate(SC.BATCH) if n != "big"]
    vs, bs = [volumes[m] for m in small], begin[small]
    for select in (2, 3):
        for conn in SC.CONNECTIVITIES:
            a, b = _against_the_specification(lib, vs, state, bs, select, conn, 10 * select + conn)
            nodes, picks = nodes + a, picks + b
    assert nodes > 500000 and picks > 300
    for name in ("serpentine", "comb", "random31", "checkerboard"):
        s = SC.cases()[name][0]
        for conn in SC.CONNECTIVITIES:
            want = sg.label_components(s.ravel(), [SC.volume_of(s)], 1, conn)
            for block in (7, 64):
                assert np.array_equal(host_segment(lib, s, 1, conn, block)[0], want), (name, conn, block)


@KB.requires_host_cxx
def test_fuzz_generator_against_the_body_compiled_for_the_host(tmp_path):
    """The generator of tests/fuzz/fuzz_segment.py without a GPU: the draws of the GPU test's seed through the body header on the
    host equal the specification, and between them they reach every connectivity and select value, both modes, a volume without
    foreground and a volume of more than 4 N nodes."""
    from omg_planner_amd import segmentation as sg
    spec = importlib.util.spec_from_file_location("fuzz_segment", Path(__file__).resolve().parent / "fuzz" / "fuzz_segment.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    lib = _host_lib(tmp_path)
    rng = np.random.default_rng(fuzz.SMOKE_SEED)
    conns, selects, modes, empty, large, ones, hanging = set(), set(), set(), 0, 0, 0, 0
    for _ in range(fuzz.SMOKE_TRIALS):
        c = fuzz.draw(rng)
        labels, comp_begin, records, picks, outs, ob, want = fuzz.specification(c)
        got = {}
        for m, v in enumerate(c["volumes"]):
            n, b = int(np.prod(v[3])), int(c["begin"][m])
            got[m] = host_segment(lib, c["state"][b: b + n].reshape(v[3]), c["select"], c["connectivity"])
            assert np.array_equal(got[m][0], labels[b: b + n]) and np.array_equal(got[m][1], records[comp_begin[m]: comp_begin[m + 1]]), (v[3], c["select"])
            empty += not sg.foreground(c["state"][b: b + n], c["select"]).any()
            large += n > 4 * SC.N
            ones += 1 in v[3]
        for k, p in enumerate(picks.tolist()):
            m, b = p[0], int(c["begin"][p[0]])
            dims = c["volumes"][m][3]
            out = host_states(lib, c["state"][b: b + int(np.prod(dims))].reshape(dims), got[m][0], got[m][1], p[:4] + [p[4] - int(comp_begin[m])] + p[5:], outs[k][3])
            assert np.array_equal(out, want[int(ob[k]): int(ob[k]) + out.size]), (k, p)
            modes.add(p[5])
            hanging += any(p[1 + a] < 0 or p[1 + a] + outs[k][3][a] > dims[a] for a in range(3))
        inside = np.zeros(len(labels), bool)
        for m, v in enumerate(c["volumes"]):
            inside[int(c["begin"][m]): int(c["begin"][m]) + int(np.prod(v[3]))] = True
        assert (labels[~inside] == -1).all() and (c["state"][~inside] == fuzz.GUARD_STATE).all()
        conns.add(c["connectivity"]), selects.add(c["select"])
    print("empty volumes", empty, "large", large, "with a dim of one", ones, "picks that hang over", hanging)
    assert conns == {6, 18, 26} and selects == {1, 2, 3} and modes == {0, 1} and empty > 0 and large > 0 and ones > 0 and hanging > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _volumes(M=2, **over):
    from omg_planner_amd import _lib
    rec = (_lib.Mesh * M)()
    for m in range(M):
        r = rec[m]
        r.origin[:], r.delta, r.sample_offset, r.dims[:] = [0.0, 0.0, 0.0], 0.01, 0.5, [4, 5, 6 + m]
        r.out_offset, r.first_workgroup = 1000 * m, m
    for k, val in over.items():
        if k in ("origin", "dims"):
            getattr(rec[M - 1], k)[:] = val
        else:
            setattr(rec[M - 1], k, val)
    return rec


def test_c_abi_argument_checks_without_gpu():
    """Every OMGX_ERR_INVALID / OMGX_ERR_UNSUPPORTED case of the four entry points is decided on the host copies before any HIP
    call: the device pointers below are never dereferenced."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    assert lib.omgx_abi_version() == 14 and _lib.SEGMENT_NODES_PER_WORKGROUP == 256 and len(_lib.STRUCTS) == 8
    INV, UNS, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED, _lib.OMGX_OK
    NAN, INF = float("nan"), float("inf")
    vpc = lambda x: C.cast(x, C.c_void_p)
    arr = lambda a: C.c_void_p(a.ctypes.data)
    d = C.c_void_p(4096)

    def nbytes(rec, M=None):
        return lib.omgx_label_workspace_bytes(vpc(rec), len(rec) if M is None else M)

    # per workgroup of 256 nodes: 256 links of 4 bytes, one total of 4 bytes, 256 ranks of 1 byte
    assert nbytes(_volumes()) == 2 * 1284 and nbytes(_volumes(1, dims=[64, 64, 64])) == 1024 * 1284
    assert nbytes(_volumes(), M=0) == 0 and lib.omgx_label_workspace_bytes(None, 0) == 0 and nbytes(_volumes(), M=-1) == INV
    assert lib.omgx_label_workspace_bytes(None, 1) == INV and nbytes(_volumes(dims=[0, 4, 4])) == INV and nbytes(_volumes(first_workgroup=2)) == INV
    assert nbytes(_volumes(1, dims=[2048, 1024, 1024])) == UNS

    def label(rec=None, M=None, begin=(0, 120), select=1, connectivity=6, state_elems=1 << 20, host=True, **ptr):
        rec = _volumes() if rec is None else rec
        begin = np.ascontiguousarray(begin, np.int64)
        p = dict(state=d, state_begin=d, volumes=d, workspace=d, labels=d, counts=d, h_state_begin=arr(begin), h_volumes=vpc(rec) if host else None)
        p.update(ptr)
        return lib.omgx_label_components(p["state"], state_elems, p["state_begin"], p["h_state_begin"], p["volumes"], p["h_volumes"],
                                         len(rec) if M is None else M, select, connectivity, p["workspace"], p["labels"], p["counts"], None)

    def records(rec=None, M=None, begin=(0, 120), comp=(0, 2, 5), cap=5, state_elems=1 << 20, **ptr):
        rec = _volumes() if rec is None else rec
        begin, comp = np.ascontiguousarray(begin, np.int64), np.ascontiguousarray(comp, np.int64)
        p = dict(labels=d, state_begin=d, volumes=d, comp_begin=d, records=d, h_state_begin=arr(begin), h_volumes=vpc(rec), h_comp_begin=arr(comp))
        p.update(ptr)
        return lib.omgx_component_records(p["labels"], state_elems, p["state_begin"], p["h_state_begin"], p["volumes"], p["h_volumes"],
                                          len(rec) if M is None else M, p["comp_begin"], p["h_comp_begin"], p["records"], cap, None)

    def outs(K=2, **over):
        rec = _volumes(K, **over)
        for k in range(K):
            rec[k].dims[:] = [3, 3, 3 + k]
        for key, val in over.items():
            if key == "dims":
                rec[K - 1].dims[:] = val
        return rec

    def states(rec=None, M=None, begin=(0, 120), comp=(0, 2, 5), C_=5, rows=((0, 0, 0, 0, 1, 0, 0, 0), (1, -2, 3, 0, 4, 1, 0, 0)), out=None, K=None,
               out_at=(0, 30), state_elems=1 << 20, out_elems=1 << 20, **ptr):
        rec, out = _volumes() if rec is None else rec, outs() if out is None else out
        begin, comp = np.ascontiguousarray(begin, np.int64), np.ascontiguousarray(comp, np.int64)
        rows, out_at = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(out_at, np.int64)
        p = dict(state=d, state_begin=d, volumes=d, labels=d, comp_begin=d, records=d, picks=d, out_volumes=d, out_begin=d, out_state=d,
                 h_state_begin=arr(begin), h_volumes=vpc(rec), h_comp_begin=arr(comp), h_picks=arr(rows), h_out_volumes=vpc(out), h_out_begin=arr(out_at))
        p.update(ptr)
        return lib.omgx_component_states(p["state"], state_elems, p["state_begin"], p["h_state_begin"], p["volumes"], p["h_volumes"],
                                         len(rec) if M is None else M, p["labels"], p["comp_begin"], p["h_comp_begin"], p["records"], C_, p["picks"],
                                         p["h_picks"], p["out_volumes"], p["h_out_volumes"], len(out) if K is None else K, p["out_begin"],
                                         p["h_out_begin"], p["out_state"], out_elems, None)

    good = [(0, 0, 0, 0, 1, 0, 0, 0), (1, -2, 3, 0, 4, 1, 0, 0)]
    for k in ("state", "state_begin", "h_state_begin", "volumes", "h_volumes", "workspace", "labels", "counts"):
        assert label(**{k: None}) == INV, k
    for k in ("labels", "state_begin", "h_state_begin", "volumes", "h_volumes", "comp_begin", "h_comp_begin", "records"):
        assert records(**{k: None}) == INV, k
    for k in ("state", "state_begin", "h_state_begin", "volumes", "h_volumes", "labels", "comp_begin", "h_comp_begin", "records", "picks", "h_picks",
              "out_volumes", "h_out_volumes", "out_begin", "h_out_begin", "out_state"):
        assert states(**{k: None}) == INV, k
    # nothing to do: OK before any pointer is looked at
    none = {k: None for k in ("state", "state_begin", "h_state_begin", "volumes", "h_volumes", "workspace", "labels", "counts")}
    assert label(M=0) == OK and label(M=0, **none) == OK and records(M=0) == OK and states(K=0) == OK and states(K=0, M=0) == OK
    assert records(M=0, labels=None, volumes=None, h_volumes=None, records=None) == OK and states(K=0, state=None, picks=None, out_state=None) == OK
    assert records(comp=(0, 0, 0), cap=0, records=None) == OK  # no component: no row, nothing launched
    assert states(M=0) == INV  # picks without volumes
    assert label(M=-1) == INV and records(M=-1) == INV and states(M=-1) == INV and states(K=-1) == INV
    assert label(state_elems=-1) == INV and records(state_elems=-1) == INV and states(state_elems=-1) == INV and states(out_elems=-1) == INV
    assert records(cap=-1) == INV and states(C_=-1) == INV
    for select in (0, 4, -1, 7):
        assert label(select=select) == INV and label(M=0, select=select) == INV
    for conn in (0, 4, 8, 7, 27, -6):
        assert label(connectivity=conn) == INV and label(M=0, connectivity=conn) == INV
    assert all(label(select=s, connectivity=c, M=0) == OK for s in (1, 2, 3) for c in (6, 18, 26))
    for fn in (label, records, states):
        for dims in ([0, 4, 4], [4, -1, 4], [4, 4, 0]):
            assert fn(rec=_volumes(dims=dims)) == INV, dims
        for delta in (0.0, -0.01, NAN, INF):
            assert fn(rec=_volumes(delta=delta)) == INV, delta
        for off in (0.25, 1.0, -0.5, NAN):
            assert fn(rec=_volumes(sample_offset=off)) == INV, off
        for origin in ([NAN, 0, 0], [0, INF, 0], [0, 0, -INF]):
            assert fn(rec=_volumes(origin=origin)) == INV, origin
        for wg in (0, 2, -1):
            assert fn(rec=_volumes(first_workgroup=wg)) == INV, wg
        assert fn(begin=(-1, 120)) == INV and fn(begin=(0, (1 << 20) - 139)) == INV and fn(state_elems=120 + 139) == INV
        assert fn(begin=(0, 119)) == INV and fn(begin=(100, 0)) == INV and fn(begin=(139, 0)) == INV
        one = {} if fn is label else {"comp": (0, 5)} if fn is records else dict(comp=(0, 5), rows=good[:1], out=outs(1), out_at=(0,))
        assert fn(rec=_volumes(1, dims=[2048, 1024, 1024]), begin=(0,), state_elems=1 << 40, **one) == UNS
        huge = _volumes(3, dims=[2048, 1024, 1024])
        huge[0].dims[:], huge[1].dims[:] = [2047, 1024, 1024], [1, 1, 1]
        huge[1].first_workgroup, huge[2].first_workgroup = 2047 * 4096, 2047 * 4096 + 1
        extra = {} if fn is label else {"comp": (0, 2, 5, 5)}
        assert fn(rec=huge, begin=(0, 1 << 32, 1 << 33), state_elems=1 << 40, **extra) == UNS
        huge[1].delta = 0.0
        assert fn(rec=huge, begin=(0, 1 << 32, 1 << 33), state_elems=1 << 40, **extra) == INV
    # the rows of the records
    for fn in (records, states):
        assert fn(comp=(1, 2, 5)) == INV and fn(comp=(0, 3, 2)) == INV and fn(comp=(0, -1, 5)) == INV
    assert records(cap=4) == INV and records(comp=(0, 2, 6)) == INV and states(C_=4) == INV
    assert records(comp=(0, 2, 1 << 31), cap=1 << 32) == UNS and states(comp=(0, 2, 1 << 31), C_=1 << 32) == UNS
    assert records(comp=(0, 2, (1 << 31) - 1), cap=(1 << 31) - 2) == INV
    # the picks: the volume, a component of another volume, the mode, the padding
    for k, col, val in ((0, 0, 2), (0, 0, -1), (1, 0, 2), (0, 4, 2), (0, 4, -1), (1, 4, 1), (1, 4, 5), (0, 5, 2), (1, 5, -1), (0, 6, 1), (1, 7, -3)):
        bad = [list(p) for p in good]
        bad[k][col] = val
        assert states(rows=bad) == INV, (k, col, val)
    assert states(comp=(0, 0, 5)) == INV  # volume 0 has no component: pick 0 names none of its rows
    # the outputs: records, ranges
    for dims in ([0, 3, 3], [3, 3, -1]):
        assert states(out=outs(dims=dims)) == INV
    assert states(out=outs(delta=0.0)) == INV and states(out=outs(first_workgroup=3)) == INV and states(out=outs(sample_offset=0.3)) == INV
    assert states(out_at=(0, 26)) == INV and states(out_at=(-1, 30)) == INV and states(out_elems=65) == INV and states(out_at=(35, 0)) == INV
    assert states(out_at=(0, 27), out_elems=62) == INV and states(out=outs(1, dims=[2048, 1024, 1024]), rows=good[:1], out_at=(0,), out_elems=1 << 40) == UNS


def test_wrapper_checks_without_gpu():
    """The host arguments are checked before the tensors, so every one of these is refused without a GPU."""
    import torch
    from omg_planner_amd import _lib, camera, ops, pipeline
    E = _lib.OmgHipError
    vols = [((0.0, 0.0, 0.0), 0.01, "centre", (4, 4, 4))]
    state = torch.zeros(64, dtype=torch.uint8)
    for what, kw in (("select must be 1, 2 or 3", dict(select=0)), ("select must be 1, 2 or 3", dict(select=4)),
                     ("connectivity must be 6, 18 or 26", dict(connectivity=8)), ("connectivity must be 6, 18 or 26", dict(connectivity=0))):
        with pytest.raises(E, match=what):
            ops.label_components(state, None, vols, **kw)
    with pytest.raises(E, match="one offset per volume"):
        ops.label_components(state, [0, 64], vols)
    with pytest.raises(E, match="dims >= 1"):
        ops.label_components(state, None, [vols[0][:3] + ((4, 0, 4),)])
    with pytest.raises(E, match="device tensor"):
        ops.label_components(state, None, vols)
    with pytest.raises(E, match="components must be"):
        ops.component_states(state, None, [], [])
    batch = ops._VolumeBatch(vols, None)
    rec, begin = batch.rec, batch.begin
    comps = ops.Components(torch.zeros(64, dtype=torch.int32), np.array([2]), np.array([0, 2]), np.zeros((2, 8), np.int32),
                           torch.zeros((2, 8), dtype=torch.int32), rec, begin, 1, 6)
    assert comps.of(0).shape == (2, 8)
    out = [((0.0, 0.0, 0.0), 0.01, "centre", (2, 2, 2))]
    for what, picks, outs_ in (("volume 1 is not one of 1", [(1, 0, 0, 0, 0, 0, 0, 0)], out), ("component 2 is not a row", [(0, 0, 0, 0, 2, 0, 0, 0)], out),
                               ("component -1 is not a row", [(0, 0, 0, 0, -1, 0, 0, 0)], out), ("mode must be 0 or 1", [(0, 0, 0, 0, 0, 2, 0, 0)], out),
                               ("padding zero", [(0, 0, 0, 0, 0, 0, 0, 1)], out), ("1 picks need as many output volumes", [(0, 0, 0, 0, 0, 0, 0, 0)], out * 2),
                               ("dims >= 1", [(0, 0, 0, 0, 0, 0, 0, 0)], [out[0][:3] + ((2, 0, 2),)])):
        with pytest.raises(E, match=what):
            ops.component_states(state, comps, picks, outs_)
        with pytest.raises(E, match=what):
            ops.component_volumes(state, comps, picks, outs_, 3)
    for radius in (0, 256):
        with pytest.raises(E, match=r"radius must lie in \[1, 255\]"):
            ops.component_volumes(state, comps, [(0, 0, 0, 0, 0, 0, 0, 0)], out, radius)
    with pytest.raises(E, match="device tensor"):
        ops.component_states(state, comps, [(0, 0, 0, 0, 0, 0, 0, 0)], out)
    assert hasattr(ops.DeviceScenes, "segment_obstacles") and hasattr(camera.Observation, "segment_obstacles") and hasattr(pipeline, "plan_observed")
    t, k = torch.tensor([1.0, 2.0, float("inf"), 0.5, float("nan")], dtype=torch.float64), torch.tensor([1.003, float("inf"), 3.0, 1.0, 1.0], dtype=torch.float64)
    assert camera.explained_mask(t, k, 0.004).tolist() == [True, False, True, False, False]


# ---------------------------------------------------------------------------------------------------------------------
# 5. registers
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_segment_kernels_do_not_spill(tmp_path):
    """The compiler's resource remarks for csrc/omg_segment.hip: no kernel uses scratch or spills, every one leaves room for eight
    waves per SIMD, and the static LDS is what the text states: the 256 links of a run (1 024 bytes) in k_label_local, one
    count per wave (16 bytes) in k_label_count and k_label_scan, none elsewhere."""
    seen = KB.kernel_resources("omg_segment.hip", tmp_path)
    lds = {"k_label_local": 1024, "k_label_border": 0, "k_label_count": 16, "k_label_scan": 16, "k_label_write": 0, "k_records_init": 0,
           "k_records_fill": 0, "k_component_states": 0}
    assert len(seen) == len(lds)
    for part, want in lds.items():
        v = KB.one(seen, part)
        print(part, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs"] <= 64, (part, v)
        assert v["LDS Size [bytes/block]"] == want, (part, v)
