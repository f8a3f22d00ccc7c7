"""Weighted TSDF fusion on the MI355X (csrc/omg_tsdf.hip): omgx_tsdf_integrate / omgx_tsdf_states /
omgx_tsdf_blend against tsdf.py bit for bit: a ragged batch between guard values against single calls, the rule's edges as one
batch of written answers, merge over two calls, ops.fuse_tsdf, the rendered scene integrated into a scene table frame after
frame and read back as a mesh, the target's pixels masked out, every refused argument, the states through the labelling, and a
short seeded fuzz run.  Every launch is followed by a checked synchronise."""
from __future__ import annotations

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import tsdf_cases as TC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _spec_volumes(volumes, D, W, begin, trunc, min_weight, radius, uo):
    """tsdf.states, fusion.distance_transform and tsdf.blend of pairs laid back to back -> (states, [volume])."""
    from omg_planner_amd import fusion, tsdf
    st = tsdf.states(D, W, min_weight)
    E = fusion.distance_transform(st, volumes, radius, uo)
    return st, [tsdf.blend(E[m], D[begin[m]: begin[m + 1]], W[begin[m]: begin[m + 1]], trunc, min_weight) for m in range(len(volumes))]


def test_ragged_batch_between_guards_against_the_specification_and_single_calls(dev):
    """Three volumes of 3 072, 765 and 910 nodes (a partial workgroup, both sample kinds) in ONE set of launches through the C
    ABI, view ranges that overlap, weights and a cap, pairs, states and volumes at offsets that are neither zero nor in order,
    guard values everywhere else: everything equals the specification and the single calls, and nothing outside the ranges is
    written."""
    from omg_planner_amd import _lib, tsdf, ops
    t, views = FC.scene_depth()
    depth = torch.from_numpy(t).to(dev)
    nodes = [int(np.prod(v[3])) for v in TC.RAGGED]
    assert nodes == [3072, 765, 910]
    begin = np.array([nodes[2] + 9, 5, nodes[2] + nodes[0] + 20], np.int64)          # volume 1 first, then 0, then 2
    offsets = [nodes[1] + nodes[2] + 11, 3, nodes[1] + 7]                             # in the pool: 1, 2, 0
    volumes = [v + (o,) for v, o in zip(TC.RAGGED, offsets)]
    elems, pool_elems = int(begin[2]) + nodes[2] + 6, offsets[0] + nodes[0] + 5
    weights, mw = np.array(TC.RAGGED_WEIGHTS), 1.5
    want_d, want_w = tsdf.integrate(TC.RAGGED, views, TC.RAGGED_RANGES, t, TC.TRUNC, FC.NEAR, weights, TC.RAGGED_WMAX)
    at = tsdf.state_offsets(TC.RAGGED)
    want = {uo: _spec_volumes(TC.RAGGED, want_d, want_w, at, TC.TRUNC, mw, TC.RAGGED_RADIUS, uo) for uo in (False, True)}
    want_state = want[True][0]
    assert all((want_state[at[m]: at[m + 1]] == k).any() for m in range(3) for k in (0, 1, 2)) and want_w.max() == TC.RAGGED_WMAX

    rec = ops.surface_records(volumes)
    l, vp, M = _lib.lib(), C.c_void_p, 3
    ptr = lambda x: vp(x.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    h_views, h_ranges = np.ascontiguousarray(views), np.ascontiguousarray(TC.RAGGED_RANGES, np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_rec = up(np.frombuffer(rec, np.uint8).copy())
    d_views, d_ranges, d_begin, d_weights = up(h_views), up(h_ranges), up(begin), up(weights)
    d, w = torch.full((elems,), 0.125, dtype=torch.float32, device=dev), torch.full((elems,), 3.25, dtype=torch.float32, device=dev)
    assert l.omgx_tsdf_integrate(ptr(d_rec), C.cast(rec, vp), M, ptr(d_views), vp(h_views.ctypes.data), 3, ptr(d_ranges), vp(h_ranges.ctypes.data),
                                 ptr(d_begin), vp(begin.ctypes.data), ptr(depth), FC.H, FC.W, ptr(d_weights), vp(weights.ctypes.data), TC.TRUNC, FC.NEAR,
                                 TC.RAGGED_WMAX, 0, ptr(d), ptr(w), elems, stream) == 0
    torch.cuda.synchronize()
    state = torch.full((elems,), 0xAB, dtype=torch.uint8, device=dev)
    assert l.omgx_tsdf_states(ptr(d), ptr(w), elems, ptr(d_begin), vp(begin.ctypes.data), ptr(d_rec), C.cast(rec, vp), M, mw, ptr(state), stream) == 0
    torch.cuda.synchronize()
    hd, hw, hs, untouched = d.cpu().numpy(), w.cpu().numpy(), state.cpu().numpy(), np.ones(elems, bool)
    for m in range(M):
        mine, spec = slice(begin[m], begin[m] + nodes[m]), slice(at[m], at[m + 1])
        assert np.array_equal(TC.bits(hd[mine]), TC.bits(want_d[spec])) and np.array_equal(TC.bits(hw[mine]), TC.bits(want_w[spec])), m
        assert np.array_equal(hs[mine], want_state[spec]), m
        untouched[mine] = False
    assert untouched.sum() == elems - sum(nodes) >= 20
    assert (hd[untouched] == 0.125).all() and (hw[untouched] == 3.25).all() and (hs[untouched] == 0xAB).all()
    ws = torch.empty(int(l.omgx_distance_transform_workspace_bytes(C.cast(rec, vp), M, TC.RAGGED_RADIUS)), dtype=torch.uint8, device=dev)
    for uo in (False, True):
        pool = torch.full((pool_elems,), -7.5, dtype=torch.float32, device=dev)
        assert l.omgx_distance_transform(ptr(state), elems, ptr(d_begin), vp(begin.ctypes.data), ptr(d_rec), C.cast(rec, vp), M, TC.RAGGED_RADIUS,
                                         int(uo), ptr(ws), ptr(pool), pool_elems, stream) == 0
        assert l.omgx_tsdf_blend(ptr(d), ptr(w), elems, ptr(d_begin), vp(begin.ctypes.data), ptr(d_rec), C.cast(rec, vp), M, TC.TRUNC, mw, ptr(pool),
                                 pool_elems, stream) == 0
        torch.cuda.synchronize()
        hp, untouched = pool.cpu().numpy(), np.ones(pool_elems, bool)
        for m in range(M):
            assert np.array_equal(TC.bits(hp[offsets[m]: offsets[m] + nodes[m]]), TC.bits(want[uo][1][m].ravel())), (m, uo)
            untouched[offsets[m]: offsets[m] + nodes[m]] = False
        assert untouched.sum() == pool_elems - sum(nodes) >= 15 and (hp[untouched] == -7.5).all()
        assert np.array_equal(d.cpu().numpy(), hd) and np.array_equal(w.cpu().numpy(), hw)  # the blend reads the pairs only
        # the single calls, through the wrappers: back to back from offset 0
        for m in range(M):
            single = ops.fuse_tsdf([TC.RAGGED[m]], views, [TC.RAGGED_RANGES[m]], depth, TC.TRUNC, FC.NEAR, TC.RAGGED_RADIUS, uo, mw, weights, TC.RAGGED_WMAX)
            torch.cuda.synchronize()
            assert single.numel() == nodes[m] and np.array_equal(_bits(single), TC.bits(want[uo][1][m].ravel())), (m, uo)
    # the wrappers on the whole batch: new buffers, zero (and unknown) where no volume lies
    got_d, got_w, got_begin = ops.tsdf_integrate(TC.RAGGED, views, TC.RAGGED_RANGES, depth, TC.TRUNC, FC.NEAR, weights, TC.RAGGED_WMAX)
    got_state = ops.tsdf_states(got_d, got_w, got_begin, TC.RAGGED, mw)
    torch.cuda.synchronize()
    assert np.array_equal(got_begin, at[:-1]) and np.array_equal(_bits(got_d), TC.bits(want_d)) and np.array_equal(_bits(got_w), TC.bits(want_w))
    assert np.array_equal(got_state.cpu().numpy(), want_state)
    # an empty batch launches nothing
    assert l.omgx_tsdf_integrate(None, None, 0, ptr(d_views), vp(h_views.ctypes.data), 3, None, None, None, None, ptr(depth), FC.H, FC.W, None, None,
                                 TC.TRUNC, FC.NEAR, float("inf"), 0, None, None, 0, stream) == 0
    assert l.omgx_tsdf_states(None, None, 0, None, None, None, None, 0, 1.0, None, stream) == 0
    assert l.omgx_tsdf_blend(None, None, 0, None, None, None, None, 0, TC.TRUNC, 1.0, None, 0, stream) == 0
    torch.cuda.synchronize()


def test_edges_as_one_ragged_batch_against_the_written_answers(dev):
    """The edges of the rule (TC.EDGE_CASES) through ONE launch, at offsets that are neither zero nor in order, between guard
    values: the device gives the pairs written out in tests/tsdf_cases.py."""
    from omg_planner_amd import ops
    volumes, ranges, _, _ = TC.edge_batch()
    nodes = [len(c[3]) for c in TC.EDGE_CASES]
    order = [4, 0, 11, 7, 2, 9, 8, 1, 6, 10, 3, 5]  # the volumes' order in the buffers, three guard elements before each
    begin, at = np.zeros(len(volumes), np.int64), 0
    for m in order:
        begin[m] = at + 3
        at += 3 + nodes[m]
    depth = torch.from_numpy(TC.EDGE_DEPTH).to(dev)
    d, w = torch.full((at + 3,), 0.125, dtype=torch.float32, device=dev), torch.full((at + 3,), 3.25, dtype=torch.float32, device=dev)
    got_d, got_w, got_begin = ops.tsdf_integrate(volumes, TC.edge_views(), ranges, depth, TC.EDGE_TRUNC, TC.EDGE_NEAR, TC.EDGE_WEIGHTS, TC.EDGE_WMAX, d, w, begin)
    torch.cuda.synchronize()
    assert got_d.data_ptr() == d.data_ptr() and got_w.data_ptr() == w.data_ptr() and np.array_equal(got_begin, begin)
    hd, hw, untouched = d.cpu().numpy(), w.cpu().numpy(), np.ones(at + 3, bool)
    for m, (what, _, _, want_d, want_w) in enumerate(TC.EDGE_CASES):
        assert hd[begin[m]: begin[m] + nodes[m]].tolist() == want_d and hw[begin[m]: begin[m] + nodes[m]].tolist() == want_w, what
        untouched[begin[m]: begin[m] + nodes[m]] = False
    assert untouched.sum() == 3 * (len(volumes) + 1) and (hd[untouched] == 0.125).all() and (hw[untouched] == 3.25).all()


def test_merge_over_two_calls(dev):
    """View 0, then views 1 and 2 merged in: the device equals the specification's own two calls bit for bit and one call over
    all three to within 2^-22 * trunc; a TsdfVolumes does the same frame after frame."""
    from omg_planner_amd import ops, tsdf
    t, views = FC.scene_depth()
    depth = torch.from_numpy(t).to(dev)
    vols = [FC.SCENE_VOLUME]
    a = tsdf.integrate(vols, views, [(0, 1)], t, TC.TRUNC, FC.NEAR)
    both = tsdf.integrate(vols, views, [(1, 2)], t, TC.TRUNC, FC.NEAR, tsdf=a[0], weight=a[1])
    d, w, begin = ops.tsdf_integrate(vols, views, [(0, 1)], depth, TC.TRUNC, FC.NEAR)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d), TC.bits(a[0])) and np.array_equal(_bits(w), TC.bits(a[1]))
    d2, w2, _ = ops.tsdf_integrate(vols, views, [(1, 2)], depth, TC.TRUNC, FC.NEAR, tsdf=d, weight=w, merge=True)
    torch.cuda.synchronize()
    assert d2.data_ptr() == d.data_ptr() and np.array_equal(_bits(d), TC.bits(both[0])) and np.array_equal(_bits(w), TC.bits(both[1]))
    one = TC.scene_pairs()
    assert np.abs(d.cpu().numpy().astype(np.float64) - one[0]).max() <= 2.0 ** -22 * TC.TRUNC and np.array_equal(w.cpu().numpy(), one[1])
    # without merge the same buffers start from (0, 0) again
    ops.tsdf_integrate(vols, views, [(0, 1)], depth, TC.TRUNC, FC.NEAR, tsdf=d, weight=w)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d), TC.bits(a[0])) and np.array_equal(_bits(w), TC.bits(a[1]))
    held = ops.TsdfVolumes(vols, TC.TRUNC, FC.NEAR, device=dev)
    held.integrate(depth[:1], views[:1], [(0, 1)]).integrate(depth[1:].contiguous(), views[1:], [(0, 2)])
    torch.cuda.synchronize()
    assert held.frames == 2 and np.array_equal(_bits(held.tsdf), TC.bits(both[0])) and np.array_equal(_bits(held.weight), TC.bits(both[1]))
    assert np.array_equal(held.states(TC.MIN_WEIGHT).cpu().numpy(), tsdf.states(both[0], both[1], TC.MIN_WEIGHT))


def test_fuse_tsdf_against_the_specification(dev):
    """ops.fuse_tsdf on the scene: a new buffer, and in place into a pool at an offset between guard values; both flags."""
    from omg_planner_amd import ops, tsdf
    t, views = FC.scene_depth()
    depth = torch.from_numpy(t).to(dev)
    n = int(np.prod(FC.DIMS))
    for uo in (False, True):
        out = ops.fuse_tsdf([FC.SCENE_VOLUME], views, [(0, 3)], depth, TC.TRUNC, FC.NEAR, FC.RADIUS, uo, TC.MIN_WEIGHT)
        torch.cuda.synchronize()
        assert out.numel() == n and np.array_equal(_bits(out), TC.bits(TC.scene_volume(uo)).ravel()), uo
    pool = torch.full((n + 11,), -7.5, dtype=torch.float32, device=dev)
    weights = [2.0, 0.0, 0.5]
    got = ops.fuse_tsdf([FC.SCENE_VOLUME[:4] + (7,)], views, [(0, 3)], depth, TC.TRUNC, FC.NEAR, FC.RADIUS, True, 2.0, weights, 2.25, out=pool)
    torch.cuda.synchronize()
    want = tsdf.fuse([FC.SCENE_VOLUME], views, [(0, 3)], t, TC.TRUNC, FC.NEAR, FC.RADIUS, True, 2.0, weights, 2.25)[0].data
    hp = pool.cpu().numpy()
    assert got.data_ptr() == pool.data_ptr() and np.array_equal(TC.bits(hp[7: 7 + n]), TC.bits(want).ravel()) and (hp[:7] == -7.5).all() and (hp[7 + n:] == -7.5).all()
    assert not np.array_equal(TC.bits(want), TC.bits(TC.scene_volume(True)))


def _table(dev, grid, scenes_n=1, reserve=0, pose=np.eye(4)):
    from omg_planner_amd import ops, scenes as sc
    slab = sc.box_sdf((0.6, 0.4, 0.02), (24, 16, 8), 1.5 / 24)
    made = [sc.Scene([sc.SceneObject("obstacles", pose, grid), sc.SceneObject("table", sc._yaw_pose(0.5, 0.0, -0.3, 0.0), slab)], 1)
            for _ in range(scenes_n)]
    return ops.DeviceScenes.from_scenes(made, device=dev, share_grids=False, reserve_voxels=reserve)


def _pool_bits(table, s, nodes):
    off = int(table.sync_host()[int(table.host_scene_begin[s])]["grid_offset"])
    return _bits(table.pool[off: off + nodes])


def test_render_integrate_into_a_table_and_a_second_frame(dev):
    """The scene rendered by ops.render_depth and integrated by DeviceScenes.integrate_obstacles into a table: the pool holds the
    specification's volume, the record has the limits and the region of a table built on the host from that volume,
    object_surfaces gives scenes.surface_nets of it; a second frame (two of the views again, with weights) through the returned
    TsdfVolumes gives the specification's merged volume in a new slot."""
    from omg_planner_amd import ops, scenes as sc, tsdf
    meshes, inst, begin, cams = FC.scene_records()
    batch = ops.CameraBatch(meshes, inst, begin, cams, device=dev)
    t, _, _ = ops.render_depth(batch, FC.H, FC.W)
    torch.cuda.synchronize()
    want_t, views = FC.scene_depth()
    assert np.array_equal(t.cpu().numpy().view(np.int64), want_t.view(np.int64))
    want = sc.SdfGrid(TC.scene_volume(True), np.array(FC.ORIGIN), FC.DELTA)
    n = want.data.size
    lifted = sc._yaw_pose(0.0, 0.0, 0.3, 0.0)
    host_table = _table(dev, want, pose=lifted)
    table = _table(dev, sc.sphere_sdf(0.05, (8, 8, 8), 0.05), reserve=2 * n, pose=lifted)
    layout = (FC.ORIGIN, FC.DELTA, FC.DIMS)
    radius, held = table.integrate_obstacles([(0, 0)], None, t, views, [(0, 3)], [layout], TC.TRUNC, FC.NEAR, reach=0.1)
    torch.cuda.synchronize()
    assert radius == FC.RADIUS and isinstance(held, ops.TsdfVolumes) and held.frames == 1 and not table._slots.pending
    rec, want_rec = table.sync_host()[0], host_table.sync_host()[0]
    assert tuple(rec["dim"]) == FC.DIMS and np.array_equal(_pool_bits(table, 0, n), TC.bits(want.data).ravel())
    for name in ("lo", "hi", "dim", "delta", "inv_delta", "pose_inv", "rb_c", "rb_h", "rb_r"):
        assert np.array_equal(rec[name], want_rec[name]), name
    verts, faces, vrows, frows, _ = table.object_surfaces([(0, 0)])
    torch.cuda.synchronize()
    wv, wf, _ = sc.surface_nets(want.data, rec["lo"].astype(np.float64), float(rec["delta"]), "centre", 0.0)
    assert len(wf) > 1000 and vrows[0].tolist() == [0, len(wv)] and frows[0].tolist() == [0, len(wf)]
    assert np.array_equal(verts.cpu().numpy().view(np.int64), wv.view(np.int64)) and np.array_equal(faces.cpu().numpy(), wf)
    # a second frame into the same pairs
    weights = [0.5, 2.0]
    radius2, again = table.integrate_obstacles([(0, 0)], held, t[1:].contiguous(), views[1:], [(0, 2)], [layout], TC.TRUNC, FC.NEAR, reach=0.1, weights=weights)
    torch.cuda.synchronize()
    assert again is held and held.frames == 2 and radius2 == FC.RADIUS and not table._slots.pending
    D, W = tsdf.integrate([FC.SCENE_VOLUME], views[1:], [(0, 2)], want_t[1:], TC.TRUNC, FC.NEAR, weights, tsdf=TC.scene_pairs()[0], weight=TC.scene_pairs()[1])
    assert np.array_equal(_bits(held.tsdf), TC.bits(D)) and np.array_equal(_bits(held.weight), TC.bits(W))
    _, vols = _spec_volumes([FC.SCENE_VOLUME], D, W, [0, n], TC.TRUNC, 1.0, FC.RADIUS, True)
    assert np.array_equal(_pool_bits(table, 0, n), TC.bits(vols[0]).ravel()) and not np.array_equal(TC.bits(vols[0]), TC.bits(want.data))


def test_observation_integrate_obstacles_with_the_targets_pixels_free(dev):
    """The sphere as the target (label 0): camera.Observation.integrate_obstacles(target_free=True) gives, per scene's camera,
    the volume the specification makes of the images with the sphere's pixels set to +inf, which is not the volume of the
    unmasked images; target_free=False gives that one."""
    from omg_planner_amd import camera, ops, scenes as sc, tsdf
    meshes, inst, begin, cams = FC.scene_records((0, 1))
    batch = ops.CameraBatch(meshes, inst, begin, cams, device=dev)
    t, inst_img, face_img = ops.render_depth(batch, FC.H, FC.W)
    torch.cuda.synchronize()
    want_t, _ = FC.scene_depth()
    sphere = FC.scene_sphere_pixels()
    assert np.array_equal(t.cpu().numpy().view(np.int64), want_t.view(np.int64)) and np.array_equal(inst_img.cpu().numpy() == 0, sphere)
    masked = np.where(sphere, np.inf, want_t)
    n = int(np.prod(FC.DIMS))
    three = _table(dev, sc.sphere_sdf(0.05, (8, 8, 8), 0.05), scenes_n=3, reserve=3 * n)
    obs = camera.Observation(batch, t, inst_img, face_img)
    pairs = [(s, 0) for s in range(3)]
    own_views = obs.view_rows(three, pairs)
    spec = lambda images, s: tsdf.fuse([FC.SCENE_VOLUME], own_views, [(s, 1)], images, TC.TRUNC, FC.NEAR, FC.RADIUS)[0].data
    for target_free, images in ((True, masked), (False, want_t)):
        radius, held = obs.integrate_obstacles(three, pairs, [(FC.ORIGIN, FC.DELTA, FC.DIMS)] * 3, TC.TRUNC, FC.NEAR, reach=0.1, target_free=target_free)
        torch.cuda.synchronize()
        assert radius == FC.RADIUS and len(held.rec) == 3
        for s in range(3):
            want = TC.bits(spec(images, s)).ravel()
            assert np.array_equal(_pool_bits(three, s, n), want), (target_free, s)
            assert not target_free or not np.array_equal(want, TC.bits(spec(want_t, s)).ravel()), s
    assert np.array_equal(t.cpu().numpy().view(np.int64), want_t.view(np.int64))  # the caller's images are not changed


def test_integrate_obstacles_refuses_bad_arguments_before_it_takes_a_slot(dev):
    """Every error of DeviceScenes.integrate_obstacles is raised before grid_slot has offered a slot (nothing pending afterwards),
    and the table still takes a good call; the wrappers' checks of their tensors."""
    from omg_planner_amd import _lib, ops, scenes as sc, tsdf
    E = _lib.OmgHipError
    want_t, views = FC.scene_depth()
    t = torch.from_numpy(want_t).to(dev)
    n = int(np.prod(FC.DIMS))
    table = _table(dev, sc.sphere_sdf(0.05, (8, 8, 8), 0.05), scenes_n=2, reserve=4 * n)
    layout = (FC.ORIGIN, FC.DELTA, FC.DIMS)
    good = dict(pairs=[(0, 0), (1, 0)], tsdf_volumes=None, depth=t, views=views, view_range=[(0, 3), (1, 2)], layouts=[layout, layout], trunc=TC.TRUNC,
                near=FC.NEAR, reach=0.1)
    nan_view = views.copy()
    nan_view[1, 9] = np.nan
    other = ops.TsdfVolumes([(FC.ORIGIN, FC.DELTA, "centre", FC.DIMS)] * 2, 0.02, FC.NEAR, device=dev)
    moved = ops.TsdfVolumes([(FC.ORIGIN, FC.DELTA, "centre", FC.DIMS), ((0.0, 0.0, 0.0), FC.DELTA, "centre", FC.DIMS)], TC.TRUNC, FC.NEAR, device=dev)
    for what, change in (("pairs need as many layouts", dict(layouts=[layout])), ("pairs need as many layouts", dict(pairs=[], layouts=[])),
                         ("named twice", dict(pairs=[(1, 0), (1, 0)])), ("reach must be finite", dict(reach=-0.01)), ("reach must be finite", dict(reach=float("nan"))),
                         ("radius must lie in", dict(reach=2.6)), ("trunc must be positive", dict(trunc=0.0)), ("trunc must be positive", dict(trunc=float("inf"))),
                         ("wmax must be positive", dict(wmax=0.0)), ("wmax must be positive", dict(wmax=float("nan"))),
                         ("min_weight must be positive", dict(min_weight=0.0)), ("min_weight must be positive", dict(min_weight=float("inf"))),
                         ("weights must be 3 finite", dict(weights=[1.0, -1.0, 1.0])), ("weights must be 3 finite", dict(weights=[1.0, 1.0])),
                         ("view_range", dict(view_range=[(0, 3), (2, 2)])), ("view_range", dict(view_range=[(0, 3)])), ("2 views but 3 images", dict(views=views[:2])),
                         ("not finite or has a focal length of zero", dict(views=nan_view)), ("band and near must be finite", dict(near=float("inf"))),
                         ("dims >= 1", dict(layouts=[layout, (FC.ORIGIN, FC.DELTA, (32, 0, 24))])),
                         ("delta must be positive", dict(layouts=[layout, (FC.ORIGIN, -0.01, FC.DIMS)])),
                         ("depth must be a tensor", dict(depth=t[0])), ("depth must be torch.float64", dict(depth=t.float())),
                         ("depth must be a device tensor", dict(depth=t.cpu())),
                         ("free_mask must be a bool tensor", dict(free_mask=torch.zeros_like(t))),
                         ("free_mask must be a bool tensor", dict(free_mask=torch.zeros(t.shape, dtype=torch.bool))),
                         ("started with other layouts", dict(tsdf_volumes=other)), ("started with other layouts", dict(tsdf_volumes=moved)),
                         ("started with other layouts", dict(tsdf_volumes="volumes"))):
        with pytest.raises(E, match=what):
            table.integrate_obstacles(**{**good, **change})
        assert not table._slots.pending, what
    with pytest.raises(IndexError):
        table.integrate_obstacles(**{**good, "pairs": [(0, 0), (2, 0)]})
    assert not table._slots.pending
    radius, held = table.integrate_obstacles(**good)
    torch.cuda.synchronize()
    assert radius == FC.RADIUS and not table._slots.pending
    with pytest.raises(E, match="started with other layouts"):  # the cap is the volumes', not the call's
        table.integrate_obstacles(**{**good, "tsdf_volumes": held, "wmax": 4.0})
    assert not table._slots.pending and held.frames == 1
    for s, rng_ in enumerate(good["view_range"]):
        want = tsdf.fuse([FC.SCENE_VOLUME], views, [rng_], want_t, TC.TRUNC, FC.NEAR, FC.RADIUS)[0].data
        assert np.array_equal(_pool_bits(table, s, n), TC.bits(want).ravel()), s
    # the wrappers' checks of their tensors
    vols = [FC.SCENE_VOLUME]
    d, w, _ = ops.tsdf_integrate(vols, views, [(0, 3)], t, TC.TRUNC, FC.NEAR)
    torch.cuda.synchronize()
    integrate = lambda **kw: ops.tsdf_integrate(vols, views, [(0, 3)], t, TC.TRUNC, FC.NEAR, **kw)
    for what, call in (("tsdf must be torch.float32", lambda: integrate(tsdf=d.double(), weight=w)), ("weight must be a device tensor", lambda: integrate(tsdf=d, weight=w.cpu())),
                       ("same number of elements", lambda: integrate(tsdf=d, weight=w[:-1])), ("omgx_tsdf_integrate", lambda: integrate(tsdf=d[:-1], weight=w[:-1])),
                       ("state must be torch.uint8", lambda: ops.tsdf_states(d, w, None, vols, 1.0, torch.zeros(n, dtype=torch.int32, device=dev))),
                       ("state must have the pairs'", lambda: ops.tsdf_states(d, w, None, vols, 1.0, torch.zeros(n + 1, dtype=torch.uint8, device=dev))),
                       ("out must be torch.float32", lambda: ops.tsdf_blend(d, w, None, vols, TC.TRUNC, 1.0, torch.zeros(n, dtype=torch.float64, device=dev))),
                       ("out must be a device tensor", lambda: ops.tsdf_blend(d, w, None, vols, TC.TRUNC, 1.0, torch.zeros(n))),
                       ("omgx_tsdf_blend", lambda: ops.tsdf_blend(d, w, None, vols, TC.TRUNC, 1.0, torch.zeros(n - 1, device=dev)))):
        with pytest.raises(E, match=what):
            call()
    torch.cuda.synchronize()


def test_label_components_on_the_states_of_the_pairs(dev):
    """ops.tsdf_states writes carve's layout: ops.label_components on its bytes gives the labels and records segmentation.py
    gives on the specification's states, and the sphere and the slab are two of the components."""
    from omg_planner_amd import ops, segmentation as sg, tsdf
    t, views = FC.scene_depth()
    depth = torch.from_numpy(t).to(dev)
    vols = [FC.SCENE_VOLUME]
    d, w, begin = ops.tsdf_integrate(vols, views, [(0, 3)], depth, TC.TRUNC, FC.NEAR)
    state = ops.tsdf_states(d, w, begin, vols, TC.MIN_WEIGHT)
    comps = ops.label_components(state, begin, vols, 1, 6)
    torch.cuda.synchronize()
    want_state = tsdf.states(*TC.scene_pairs(), TC.MIN_WEIGHT)
    want = sg.label_components(want_state, vols, 1, 6)
    comp_begin, records = sg.component_records(want, vols)
    assert np.array_equal(state.cpu().numpy(), want_state) and np.array_equal(comps.labels.cpu().numpy(), want)
    assert np.array_equal(comps.comp_begin, comp_begin) and np.array_equal(comps.records, records) and (records[:, 0] > 100).sum() >= 2


def test_a_short_seeded_fuzz_run(dev):
    spec = importlib.util.spec_from_file_location("fuzz_tsdf", Path(__file__).resolve().parent / "fuzz" / "fuzz_tsdf.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    assert fuzz.main(trials=fuzz.SMOKE_TRIALS, seed=fuzz.SMOKE_SEED) == 0
