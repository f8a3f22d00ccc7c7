"""Depth fusion on the MI355X (csrc/omg_fusion.hip): omgx_carve_views / omgx_distance_transform against
fusion.py bit for bit: a ragged batch between guard values against single calls, merge against the union, the transform grids,
the carve rule's edges as one batch of known answers, the shapes that straddle a chunk at the radius extremes, the rendered
scene fused into a scene table and read by the SDF kernel, the target's pixels masked out, every refused argument, and a short
seeded fuzz run.  Every launch is followed by a checked synchronise."""
from __future__ import annotations

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import fusion_cases as FC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def test_ragged_batch_between_guards_against_the_specification_and_single_calls(dev):
    """Three volumes of different dims and sample offsets in ONE set of launches through the C ABI, view ranges that overlap,
    states and volumes at offsets that are neither zero nor in order, guard values everywhere else: states and volumes equal the
    specification and the single calls, nothing outside the ranges is written, and merge on the device equals the union."""
    from omg_planner_amd import _lib, fusion, ops
    t, views = FC.scene_depth()
    depth = torch.from_numpy(t).to(dev)
    nodes = [int(np.prod(v[3])) for v in FC.RAGGED]
    begin = np.array([nodes[2] + 9, 5, nodes[2] + nodes[0] + 20], np.int64)          # volume 1 first, then 0, then 2
    offsets = [nodes[1] + nodes[2] + 11, 3, nodes[1] + 7]                             # in the pool: 1, 2, 0
    volumes = [v + (o,) for v, o in zip(FC.RAGGED, offsets)]
    state_elems, pool_elems = int(begin[2]) + nodes[2] + 6, offsets[0] + nodes[0] + 5
    want_state = fusion.carve_views(FC.RAGGED, views, FC.RAGGED_RANGES, t, FC.BAND, FC.NEAR)
    want = {uo: fusion.distance_transform(want_state, FC.RAGGED, FC.RAGGED_RADIUS, uo) for uo in (False, True)}
    at = fusion.state_offsets(FC.RAGGED)
    assert all((want_state[at[m]: at[m + 1]] == k).any() for m in range(3) for k in (0, 1, 2))

    rec = ops.surface_records(volumes)
    l, vp, M = _lib.lib(), C.c_void_p, 3
    ptr = lambda x: vp(x.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    h_views, h_ranges = np.ascontiguousarray(views), np.ascontiguousarray(FC.RAGGED_RANGES, np.int32)
    d_rec = torch.from_numpy(np.frombuffer(rec, np.uint8).copy()).to(dev)
    d_views, d_ranges, d_begin = torch.from_numpy(h_views).to(dev), torch.from_numpy(h_ranges).to(dev), torch.from_numpy(begin).to(dev)
    state = torch.full((state_elems,), 0xAB, dtype=torch.uint8, device=dev)
    assert l.omgx_carve_views(ptr(d_rec), C.cast(rec, vp), M, ptr(d_views), vp(h_views.ctypes.data), 3, ptr(d_ranges), vp(h_ranges.ctypes.data),
                              ptr(d_begin), vp(begin.ctypes.data), ptr(depth), FC.H, FC.W, FC.BAND, FC.NEAR, 0, ptr(state), state_elems, stream) == 0
    torch.cuda.synchronize()
    hs, untouched = state.cpu().numpy(), np.ones(state_elems, bool)
    for m in range(M):
        assert np.array_equal(hs[begin[m]: begin[m] + nodes[m]], want_state[at[m]: at[m + 1]]), m
        untouched[begin[m]: begin[m] + nodes[m]] = False
    assert untouched.sum() == state_elems - sum(nodes) >= 20 and (hs[untouched] == 0xAB).all()
    ws = torch.empty(int(l.omgx_distance_transform_workspace_bytes(C.cast(rec, vp), M, FC.RAGGED_RADIUS)), dtype=torch.uint8, device=dev)
    for uo in (False, True):
        pool = torch.full((pool_elems,), -7.5, dtype=torch.float32, device=dev)
        assert l.omgx_distance_transform(ptr(state), state_elems, ptr(d_begin), vp(begin.ctypes.data), ptr(d_rec), C.cast(rec, vp), M, FC.RAGGED_RADIUS,
                                         int(uo), ptr(ws), ptr(pool), pool_elems, stream) == 0
        torch.cuda.synchronize()
        hp, untouched = pool.cpu().numpy(), np.ones(pool_elems, bool)
        for m in range(M):
            assert np.array_equal(FC.bits(hp[offsets[m]: offsets[m] + nodes[m]]), FC.bits(want[uo][m].ravel())), (m, uo)
            untouched[offsets[m]: offsets[m] + nodes[m]] = False
        assert untouched.sum() == pool_elems - sum(nodes) >= 15 and (hp[untouched] == -7.5).all()
        assert np.array_equal(state.cpu().numpy(), hs)  # the transform reads the states only
        # the single calls, through the wrappers: back to back from offset 0
        for m in range(M):
            single = ops.fuse_views([FC.RAGGED[m]], views, [FC.RAGGED_RANGES[m]], depth, FC.BAND, FC.NEAR, FC.RAGGED_RADIUS, uo)
            torch.cuda.synchronize()
            assert single.numel() == nodes[m] and np.array_equal(_bits(single), FC.bits(want[uo][m].ravel())), (m, uo)
    # the wrapper on the whole batch, and merge: views [first] and then the rest equals all of them
    got_state, got_begin = ops.carve_views(FC.RAGGED, views, FC.RAGGED_RANGES, depth, FC.BAND, FC.NEAR)
    torch.cuda.synchronize()
    assert np.array_equal(got_begin, at[:-1]) and np.array_equal(got_state.cpu().numpy(), want_state)
    first = [(a, min(n, 1)) for a, n in FC.RAGGED_RANGES]
    rest = [(a + min(n, 1), n - min(n, 1)) for a, n in FC.RAGGED_RANGES]
    part, _ = ops.carve_views(FC.RAGGED, views, first, depth, FC.BAND, FC.NEAR)
    torch.cuda.synchronize()
    assert np.array_equal(part.cpu().numpy(), fusion.carve_views(FC.RAGGED, views, first, t, FC.BAND, FC.NEAR)) and not np.array_equal(part.cpu().numpy(), want_state)
    merged, _ = ops.carve_views(FC.RAGGED, views, rest, depth, FC.BAND, FC.NEAR, state=part, merge=True)
    torch.cuda.synchronize()
    assert merged.data_ptr() == part.data_ptr() and np.array_equal(merged.cpu().numpy(), want_state)
    # an empty batch launches nothing
    assert l.omgx_carve_views(None, None, 0, ptr(d_views), vp(h_views.ctypes.data), 3, None, None, None, None, ptr(depth), FC.H, FC.W, FC.BAND, FC.NEAR,
                              0, None, 0, stream) == 0
    torch.cuda.synchronize()


def test_carve_edges_as_one_ragged_batch_against_the_written_answers(dev):
    """The edges of the carve rule (FC.EDGE_CASES: z at near, pixels -0.5 and W - 0.5 / H - 0.5, depths NaN / 0 / negative /
    +inf, z at d - band and d + band, surface against free, a moved camera with its own intrinsics, no views, both sample
    offsets) through ONE launch, at state offsets that are neither zero nor in order, between guard values: the device gives
    the answers written out in tests/fusion_cases.py and the specification's bytes, and the transform of those states its bits."""
    from omg_planner_amd import fusion, ops
    volumes, ranges = [c[1] for c in FC.EDGE_CASES], [c[2] for c in FC.EDGE_CASES]
    nodes = [len(c[3]) for c in FC.EDGE_CASES]
    order = [4, 0, 7, 2, 8, 1, 6, 3, 5]  # the volumes' order in the state buffer, three guard bytes before each
    begin, at = np.zeros(len(volumes), np.int64), 0
    for m in order:
        begin[m] = at + 3
        at += 3 + nodes[m]
    depth = torch.from_numpy(FC.EDGE_DEPTH).to(dev)
    state = torch.full((at + 3,), 0xAB, dtype=torch.uint8, device=dev)
    got, got_begin = ops.carve_views(volumes, FC.edge_views(), ranges, depth, FC.EDGE_BAND, FC.EDGE_NEAR, state=state, state_begin=begin)
    torch.cuda.synchronize()
    assert got.data_ptr() == state.data_ptr() and np.array_equal(got_begin, begin)
    hs, untouched = state.cpu().numpy(), np.ones(at + 3, bool)
    want = fusion.carve_views(volumes, FC.edge_views(), ranges, FC.EDGE_DEPTH, FC.EDGE_BAND, FC.EDGE_NEAR, state=np.full(at + 3, 0xAB, np.uint8),
                              state_begin=begin)
    for m, (what, _, _, answer) in enumerate(FC.EDGE_CASES):
        assert hs[begin[m]: begin[m] + nodes[m]].tolist() == answer, what
        untouched[begin[m]: begin[m] + nodes[m]] = False
    assert np.array_equal(hs, want) and untouched.sum() == 3 * (len(volumes) + 1) and (hs[untouched] == 0xAB).all()
    # a buffer of the wrapper's own at the caller's offsets: unknown where no volume lies, as the specification's
    own, _ = ops.carve_views(volumes, FC.edge_views(), ranges, depth, FC.EDGE_BAND, FC.EDGE_NEAR, state_begin=begin)
    torch.cuda.synchronize()
    assert np.array_equal(own.cpu().numpy(), fusion.carve_views(volumes, FC.edge_views(), ranges, FC.EDGE_DEPTH, FC.EDGE_BAND, FC.EDGE_NEAR,
                                                                state_begin=begin))
    assert own.numel() == at and (own.cpu().numpy()[untouched[:at]] == fusion.UNKNOWN).all()
    # merge: view 1 alone, then view 0 merged in, on the volume that sees both
    both = FC.EDGE_CASES[6]
    part, _ = ops.carve_views([both[1]], FC.edge_views(), [(1, 1)], depth, FC.EDGE_BAND, FC.EDGE_NEAR)
    torch.cuda.synchronize()
    assert part.cpu().numpy().tolist() == [fusion.SURFACE, fusion.UNKNOWN]
    merged, _ = ops.carve_views([both[1]], FC.edge_views(), [(0, 1)], depth, FC.EDGE_BAND, FC.EDGE_NEAR, state=part, merge=True)
    torch.cuda.synchronize()
    assert merged.cpu().numpy().tolist() == both[3]
    for uo in (False, True):
        out = ops.distance_transform(state, begin, volumes, 3, uo)
        torch.cuda.synchronize()
        spec = fusion.distance_transform(want, volumes, 3, uo, state_begin=begin)
        off = fusion.state_offsets(volumes)
        assert out.numel() == off[-1]  # (layouts without a pool offset lie back to back)
        for m in range(len(volumes)):
            assert np.array_equal(_bits(out[off[m]: off[m + 1]]), FC.bits(spec[m]).ravel()), (FC.EDGE_CASES[m][0], uo)


@pytest.mark.parametrize("radius", FC.RADII)
def test_transform_grids_as_one_batch(dev, radius):
    """The grids of the CPU test (random states with bytes that are neither 0, 1 nor 2; a dim of 1; all free; all occupied) as one
    ragged batch per radius and flag."""
    from omg_planner_amd import fusion, ops
    grids = [FC.states(n) for n in FC.TRANSFORM]
    volumes, at = [], 0
    for s in grids:
        volumes.append(((0.0, 0.0, 0.0), 0.0125, "centre", s.shape, at))
        at += s.size
    state = torch.from_numpy(np.concatenate([s.ravel() for s in grids])).to(dev)
    for uo in (False, True):
        out = ops.distance_transform(state, None, volumes, radius, uo)
        torch.cuda.synchronize()
        got = _bits(out)
        for v, s in zip(volumes, grids):
            assert np.array_equal(got[v[4]: v[4] + s.size], FC.bits(fusion.signed_volume(s, 0.0125, radius, uo)).ravel()), (s.shape, radius, uo)


@pytest.mark.parametrize("radius", FC.STRADDLE_RADII)
def test_chunk_straddling_shapes_and_radius_extremes(dev, radius):
    """One axis of 2 * OMGX_FUSION_CHUNK + 3 = 131 nodes, for each axis in turn, and an x and a y axis of 261, at radius 1, 5, 70 (a
    halo longer than a chunk) and 255 (the largest: longer than the axis of 131, and 261 staged lines, more than 64 KB of LDS)."""
    from omg_planner_amd import _lib, fusion, ops
    assert _lib.FUSION_CHUNK == FC.CHUNK
    grids = [FC.states(n) for n in FC.STRADDLE]
    volumes, at = [], 0
    for s in grids:
        volumes.append(((0.0, 0.0, 0.0), 0.01, "node", s.shape, at))
        at += s.size
    state = torch.from_numpy(np.concatenate([s.ravel() for s in grids])).to(dev)
    for uo in (False, True):
        out = ops.distance_transform(state, None, volumes, radius, uo)
        torch.cuda.synchronize()
        got = _bits(out)
        for v, s in zip(volumes, grids):
            assert np.array_equal(got[v[4]: v[4] + s.size], FC.bits(fusion.signed_volume(s, 0.01, radius, uo)).ravel()), (s.shape, radius, uo)


def _table(dev, grid, scenes_n=1, reserve=0, pose=np.eye(4)):
    from omg_planner_amd import ops, scenes as sc
    slab = sc.box_sdf((0.6, 0.4, 0.02), (24, 16, 8), 1.5 / 24)
    made = [sc.Scene([sc.SceneObject("obstacles", pose, grid), sc.SceneObject("table", sc._yaw_pose(0.5, 0.0, -0.3, 0.0), slab)], 1)
            for _ in range(scenes_n)]
    return ops.DeviceScenes.from_scenes(made, device=dev, share_grids=False, reserve_voxels=reserve)


def test_end_to_end_render_fuse_into_a_table_and_read_by_the_sdf_kernel(dev):
    """The scene of the CPU test rendered by ops.render_depth and fused by DeviceScenes.fuse_obstacles into a table: the pool holds
    the specification's volume, and ops.fk_sdf gives on that table the potentials it gives on a table built on the host from the
    specification's volume, bit for bit.  Then camera.Observation.fuse_obstacles: one volume per camera's scene in one set of launches."""
    from omg_planner_amd import camera, fusion, ops, robot as rb, scenes as sc
    meshes, inst, begin, cams = FC.scene_records()
    batch = ops.CameraBatch(meshes, inst, begin, cams, device=dev)
    t, inst_img, face_img = ops.render_depth(batch, FC.H, FC.W)
    torch.cuda.synchronize()
    want_t, views = FC.scene_depth()
    assert np.array_equal(t.cpu().numpy().view(np.int64), want_t.view(np.int64))
    want = sc.SdfGrid(FC.scene_volume(3), np.array(FC.ORIGIN), FC.DELTA)
    lifted = sc._yaw_pose(0.0, 0.0, 0.3, 0.0)  # the grid's frame in the world: the observed sphere around the arm's first links
    host_table = _table(dev, want, pose=lifted)
    placeholder = sc.sphere_sdf(0.05, (8, 8, 8), 0.05)
    table = _table(dev, placeholder, reserve=want.data.size, pose=lifted)
    radius = table.fuse_obstacles([(0, 0)], t, views, [(0, 3)], [(FC.ORIGIN, FC.DELTA, FC.DIMS)], FC.BAND, FC.NEAR, reach=0.1)
    torch.cuda.synchronize()
    assert radius == FC.RADIUS
    rec = table.sync_host()[0]
    off = int(rec["grid_offset"])
    assert tuple(rec["dim"]) == FC.DIMS and np.array_equal(_bits(table.pool[off: off + want.data.size]), FC.bits(want.data).ravel())
    want_rec = host_table.sync_host()[0]
    for name in ("lo", "hi", "dim", "delta", "inv_delta", "pose_inv", "rb_c", "rb_h", "rb_r"):
        assert np.array_equal(rec[name], want_rec[name]), name
    model = rb.PandaModel(seed=0)
    robot = ops.robot_blob(model, dev)
    rng = np.random.default_rng(5)
    joints = torch.from_numpy(np.stack([rb.HOME_CONFIG] + [rb.HOME_CONFIG + rng.normal(scale=0.4, size=9) for _ in range(7)])[None]).to(dev)
    pots = []
    for tab in (table, host_table):
        pot, grad, _ = ops.fk_sdf(robot, model.points_per_link, tab, joints)
        torch.cuda.synchronize()
        pots.append((pot.clone(), grad.clone()))
    assert float(pots[0][0].abs().sum()) > 0  # the arm's first links stand inside the observed volume
    assert np.array_equal(_bits(pots[0][0]), _bits(pots[1][0])) and np.array_equal(_bits(pots[0][1]), _bits(pots[1][1]))
    # one obstacle volume per scene, each seen by its own scene's camera, in one set of launches
    three = _table(dev, placeholder, scenes_n=3, reserve=3 * want.data.size)
    obs = camera.Observation(batch, t, inst_img, face_img)
    assert obs.fuse_obstacles(three, [(s, 0) for s in range(3)], [(FC.ORIGIN, FC.DELTA, FC.DIMS)] * 3, FC.BAND, FC.NEAR, reach=0.1) == FC.RADIUS
    torch.cuda.synchronize()
    recs = three.sync_host()
    own_views = obs.view_rows(three, [(s, 0) for s in range(3)])  # (the camera records' inverse, inverted back: the last bits may differ)
    assert np.abs(own_views - views).max() < 1e-12
    for s in range(3):
        r = recs[int(three.host_scene_begin[s])]
        single = fusion.signed_volume(fusion.carve_views([FC.SCENE_VOLUME], own_views, [(s, 1)], want_t, FC.BAND, FC.NEAR).reshape(FC.DIMS), FC.DELTA,
                                      FC.RADIUS, True)
        off = int(r["grid_offset"])
        assert np.array_equal(_bits(three.pool[off: off + single.size]), FC.bits(single).ravel()), s


def test_free_mask_turns_the_targets_pixels_into_background(dev):
    """The sphere as the target (label 0), the slab not: camera.Observation.fuse_obstacles(target_free=True) and
    DeviceScenes.fuse_obstacles(free_mask=...) give the volume the specification carves from the depth images with the sphere's
    pixels set to +inf, which is not the volume of the unmasked images (a wrong label, a wrong instance index or a wrong
    selection would give that one, or another)."""
    from omg_planner_amd import camera, fusion, ops, scenes as sc
    meshes, inst, begin, cams = FC.scene_records((0, 1))
    batch = ops.CameraBatch(meshes, inst, begin, cams, device=dev)
    t, inst_img, face_img = ops.render_depth(batch, FC.H, FC.W)
    torch.cuda.synchronize()
    want_t, views = FC.scene_depth()
    sphere = FC.scene_sphere_pixels()
    assert np.array_equal(t.cpu().numpy().view(np.int64), want_t.view(np.int64)) and np.array_equal(inst_img.cpu().numpy() == 0, sphere)
    assert all(100 < sphere[s].sum() < FC.H * FC.W // 2 for s in range(3))
    masked = np.where(sphere, np.inf, want_t)
    placeholder = sc.sphere_sdf(0.05, (8, 8, 8), 0.05)
    nodes = int(np.prod(FC.DIMS))
    three = _table(dev, placeholder, scenes_n=3, reserve=3 * nodes)
    obs = camera.Observation(batch, t, inst_img, face_img)
    pairs = [(s, 0) for s in range(3)]
    own_views = obs.view_rows(three, pairs)

    def spec(images, s):
        return fusion.signed_volume(fusion.carve_views([FC.SCENE_VOLUME], own_views, [(s, 1)], images, FC.BAND, FC.NEAR).reshape(FC.DIMS), FC.DELTA,
                                    FC.RADIUS, True)

    def pool_bits(table, s):
        off = int(table.sync_host()[int(table.host_scene_begin[s])]["grid_offset"])
        return _bits(table.pool[off: off + nodes])

    assert obs.fuse_obstacles(three, pairs, [(FC.ORIGIN, FC.DELTA, FC.DIMS)] * 3, FC.BAND, FC.NEAR, reach=0.1, target_free=True) == FC.RADIUS
    torch.cuda.synchronize()
    for s in range(3):
        want = FC.bits(spec(masked, s)).ravel()
        assert np.array_equal(pool_bits(three, s), want) and not np.array_equal(want, FC.bits(spec(want_t, s)).ravel()), s
    assert obs.fuse_obstacles(three, pairs, [(FC.ORIGIN, FC.DELTA, FC.DIMS)] * 3, FC.BAND, FC.NEAR, reach=0.1, target_free=False) == FC.RADIUS
    torch.cuda.synchronize()
    for s in range(3):
        assert np.array_equal(pool_bits(three, s), FC.bits(spec(want_t, s)).ravel()), s
    # the mask handed over directly: any pixels, here the left half of image 0 and the sphere in image 2, three views on one volume
    mask = np.zeros(want_t.shape, bool)
    mask[0, :, : FC.W // 2], mask[2] = True, sphere[2]
    one = _table(dev, placeholder, reserve=nodes)
    one.fuse_obstacles([(0, 0)], t, views, [(0, 3)], [(FC.ORIGIN, FC.DELTA, FC.DIMS)], FC.BAND, FC.NEAR, reach=0.1, free_mask=torch.from_numpy(mask).to(dev))
    torch.cuda.synchronize()
    want = fusion.signed_volume(fusion.carve_views([FC.SCENE_VOLUME], views, [(0, 3)], np.where(mask, np.inf, want_t), FC.BAND, FC.NEAR).reshape(FC.DIMS),
                                FC.DELTA, FC.RADIUS, True)
    assert np.array_equal(pool_bits(one, 0), FC.bits(want).ravel()) and not np.array_equal(FC.bits(want), FC.bits(FC.scene_volume(3)))
    assert np.array_equal(t.cpu().numpy().view(np.int64), want_t.view(np.int64))  # the caller's images are not changed


def test_fuse_obstacles_refuses_bad_arguments_before_it_takes_a_slot(dev):
    """Every error of DeviceScenes.fuse_obstacles, and those of the wrappers that need device tensors: raised before grid_slot has
    offered a slot (nothing pending afterwards), and the table still takes a good call."""
    from omg_planner_amd import _lib, fusion, ops, scenes as sc
    E = _lib.OmgHipError
    want_t, views = FC.scene_depth()
    t = torch.from_numpy(want_t).to(dev)
    nodes = int(np.prod(FC.DIMS))
    table = _table(dev, sc.sphere_sdf(0.05, (8, 8, 8), 0.05), scenes_n=2, reserve=2 * nodes)
    layout = (FC.ORIGIN, FC.DELTA, FC.DIMS)
    good = dict(pairs=[(0, 0), (1, 0)], depth=t, views=views, view_range=[(0, 3), (1, 2)], layouts=[layout, layout], band=FC.BAND, near=FC.NEAR, reach=0.1)
    nan_view = views.copy()
    nan_view[1, 9] = np.nan
    no_focal = views.copy()
    no_focal[2, 1] = 0.0
    for what, change in (("pairs need as many layouts", dict(layouts=[layout])), ("pairs need as many layouts", dict(pairs=[], layouts=[])),
                         ("named twice", dict(pairs=[(1, 0), (1, 0)])), ("reach must be finite", dict(reach=-0.01)),
                         ("reach must be finite", dict(reach=float("inf"))), ("reach must be finite", dict(reach=float("nan"))),
                         ("radius must lie in", dict(reach=2.6)),  # ceil(2.6 / 0.01 + 0.5) + 1 = 262
                         ("radius must lie in", dict(layouts=[layout, (FC.ORIGIN, 0.0003, FC.DIMS)])),  # a fine delta
                         ("view_range", dict(view_range=[(0, 3), (2, 2)])), ("view_range", dict(view_range=[(0, 3)])),
                         ("view_range", dict(view_range=[(0, 3), (-1, 2)])), ("2 views but 3 images", dict(views=views[:2])),
                         ("not finite or has a focal length of zero", dict(views=nan_view)),
                         ("not finite or has a focal length of zero", dict(views=no_focal)),
                         ("band and near must be finite", dict(band=float("nan"))), ("band and near must be finite", dict(near=float("inf"))),
                         ("dims >= 1", dict(layouts=[layout, (FC.ORIGIN, FC.DELTA, (32, 0, 24))])),
                         ("delta must be positive", dict(layouts=[layout, (FC.ORIGIN, -0.01, FC.DIMS)])),
                         ("depth must be a tensor", dict(depth=t[0])), ("depth must be torch.float64", dict(depth=t.float())),
                         ("depth must be a device tensor", dict(depth=t.cpu())),
                         ("free_mask must be a bool tensor", dict(free_mask=torch.zeros_like(t))),
                         ("free_mask must be a bool tensor", dict(free_mask=torch.zeros(t.shape[1:], dtype=torch.bool, device=dev))),
                         ("free_mask must be a bool tensor", dict(free_mask=torch.zeros(t.shape, dtype=torch.bool))),
                         ("free_mask must be a bool tensor", dict(free_mask=np.zeros(t.shape, bool)))):
        with pytest.raises(E, match=what):
            table.fuse_obstacles(**{**good, **change})
        assert not table._slots.pending, what
    with pytest.raises(IndexError):
        table.fuse_obstacles(**{**good, "pairs": [(0, 0), (2, 0)]})
    assert not table._slots.pending
    assert table.fuse_obstacles(**good) == FC.RADIUS
    torch.cuda.synchronize()
    assert not table._slots.pending
    for s, rng_ in enumerate(good["view_range"]):
        want = fusion.signed_volume(fusion.carve_views([FC.SCENE_VOLUME], views, [rng_], want_t, FC.BAND, FC.NEAR).reshape(FC.DIMS), FC.DELTA, FC.RADIUS, True)
        off = int(table.sync_host()[int(table.host_scene_begin[s])]["grid_offset"])
        assert np.array_equal(_bits(table.pool[off: off + nodes]), FC.bits(want).ravel()), s
    # the wrappers' checks of their tensors
    vols = [FC.SCENE_VOLUME]
    state, _ = ops.carve_views(vols, views, [(0, 3)], t, FC.BAND, FC.NEAR)
    torch.cuda.synchronize()
    for what, call in (("state must be torch.uint8", lambda: ops.carve_views(vols, views, [(0, 3)], t, FC.BAND, FC.NEAR, state=state.float(), merge=True)),
                       ("state must be a device tensor", lambda: ops.carve_views(vols, views, [(0, 3)], t, FC.BAND, FC.NEAR, state=state.cpu())),
                       ("state must be torch.uint8", lambda: ops.distance_transform(state.int(), None, vols, 3)),
                       ("out must be torch.float32", lambda: ops.distance_transform(state, None, vols, 3, out=torch.zeros(nodes, dtype=torch.float64, device=dev))),
                       ("out must be a device tensor", lambda: ops.distance_transform(state, None, vols, 3, out=torch.zeros(nodes))),
                       ("omgx_carve_views", lambda: ops.carve_views(vols, views, [(0, 3)], t, FC.BAND, FC.NEAR, state=state[:-1])),  # too short
                       ("omgx_distance_transform", lambda: ops.distance_transform(state, None, vols, 3, out=torch.zeros(nodes - 1, device=dev)))):
        with pytest.raises(E, match=what):
            call()
    torch.cuda.synchronize()


def test_a_short_seeded_fuzz_run(dev):
    spec = importlib.util.spec_from_file_location("fuzz_fusion", Path(__file__).resolve().parent / "fuzz" / "fuzz_fusion.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    assert fuzz.main(trials=fuzz.SMOKE_TRIALS, seed=fuzz.SMOKE_SEED) == 0


def test_every_volume_op_finds_the_volumes_of_one_ragged_batch(dev):
    """The six volumes of fusion_cases.LOCATE (1, 1, 1, 2, 3 and 2 workgroups: a single node, a full workgroup, one node past a
    full one, a long thin row; both sample offsets) as ONE batch through every op that maps workgroups to volumes by the
    first_workgroup prefix table: mesh SDF, carve and transform, the three TSDF steps, labelling, half-space volumes and surface
    extraction, each bit for bit what its specification gives."""
    from omg_planner_amd import fusion, ops, planes, scenes as sc, segmentation as sg, tsdf
    from tests import mesh_cases as MC
    vols, M = FC.LOCATE, len(FC.LOCATE)
    nodes = [int(np.prod(v[3])) for v in vols]
    at = fusion.state_offsets(vols)
    assert [-(-n // 256) for n in nodes] == list(np.diff(FC.LOCATE_FIRST_WORKGROUP)) and {v[2] for v in vols} == {"centre", "node"}
    t, views = FC.locate_views()
    depth = torch.from_numpy(t).to(dev)
    # carve and transform
    want_state = fusion.carve_views(vols, views, FC.LOCATE_RANGES, t, FC.LOCATE_BAND, FC.LOCATE_NEAR)
    want_vol = fusion.distance_transform(want_state, vols, FC.LOCATE_RADIUS, True)
    assert {0, 1, 2} <= set(want_state.tolist())
    state, begin = ops.carve_views(vols, views, FC.LOCATE_RANGES, depth, FC.LOCATE_BAND, FC.LOCATE_NEAR)
    pool = ops.distance_transform(state, begin, vols, FC.LOCATE_RADIUS, True)
    torch.cuda.synchronize()
    assert np.array_equal(begin, at[:-1]) and np.array_equal(state.cpu().numpy(), want_state)
    assert np.array_equal(_bits(pool), np.concatenate([FC.bits(v).ravel() for v in want_vol]))
    # the three TSDF steps
    trunc, mw = 0.03, 1.0
    want_d, want_w = tsdf.integrate(vols, views, FC.LOCATE_RANGES, t, trunc, FC.LOCATE_NEAR)
    want_ts = tsdf.states(want_d, want_w, mw)
    want_e = fusion.distance_transform(want_ts, vols, FC.LOCATE_RADIUS, True)
    want_blend = [tsdf.blend(want_e[m], want_d[at[m]: at[m + 1]], want_w[at[m]: at[m + 1]], trunc, mw) for m in range(M)]
    got_d, got_w, got_begin = ops.tsdf_integrate(vols, views, FC.LOCATE_RANGES, depth, trunc, FC.LOCATE_NEAR)
    got_ts = ops.tsdf_states(got_d, got_w, got_begin, vols, mw)
    blended = ops.tsdf_blend(got_d, got_w, got_begin, vols, trunc, mw, ops.distance_transform(got_ts, got_begin, vols, FC.LOCATE_RADIUS, True))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got_d), FC.bits(want_d)) and np.array_equal(_bits(got_w), FC.bits(want_w)) and (want_w > 0).any()
    assert np.array_equal(got_ts.cpu().numpy(), want_ts)
    assert np.array_equal(_bits(blended), np.concatenate([FC.bits(v).ravel() for v in want_blend]))
    # labelling: the nodes that are not free
    comps = ops.label_components(state, begin, vols, 3, 26)
    torch.cuda.synchronize()
    want_labels = sg.label_components(want_state, vols, 3, 26)
    comp_begin, records = sg.component_records(want_labels, vols)
    assert np.array_equal(comps.labels.cpu().numpy(), want_labels) and np.array_equal(comps.records, records) and np.array_equal(comps.comp_begin, comp_begin)
    assert (np.diff(comp_begin) > 0).sum() >= M - 1
    # half-space volumes
    pls = [(0.6, 0.0, 0.8, -0.01 * m) for m in range(M)]
    got_planes = ops.plane_volumes(vols, pls, device=dev)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got_planes), np.concatenate([planes.halfspace_volume(v, p).ravel() for v, p in zip(vols, pls)]).view(np.uint32))
    # surface extraction: the planes' zero level
    v, f, vrows, frows, o = ops.surface_meshes(got_planes, [vol + (int(a),) for vol, a in zip(vols, at)], 0.0)
    torch.cuda.synchronize()
    want_surf = [sc.surface_nets(planes.halfspace_volume(vol, p), np.array(vol[0]), vol[1], vol[2], 0.0) for vol, p in zip(vols, pls)]
    assert vrows[:, 1].tolist() == [len(w[0]) for w in want_surf] and frows[:, 1].tolist() == [len(w[1]) for w in want_surf]
    assert o.tolist() == [w[2] for w in want_surf] and sum(len(w[0]) for w in want_surf) > 0
    assert np.array_equal(v.cpu().numpy().view(np.uint64), np.concatenate([w[0] for w in want_surf]).view(np.uint64))
    assert np.array_equal(f.cpu().numpy(), np.concatenate([w[1] for w in want_surf]))
    # mesh SDF: a closed box about the middle of every volume, the magnitudes bit for bit and the sign by the winding number's decision
    origins, dims, boxes = [np.array(vol[0]) for vol in vols], [vol[3] for vol in vols], []
    for origin, delta, sample, d in vols:
        pose = np.eye(4)
        pose[:3, 3] = origin + ((np.array(d) - 1) / 2 + {"centre": 0.5, "node": 0.0}[sample]) * delta
        boxes.append(MC.box_mesh(np.maximum(0.3 * np.array(d) * delta, 0.75 * delta), pose)[:2])
    grids, _, _, dropped = ops.mesh_sdf_batch(boxes, [vol[1] for vol in vols], 0, [vol[2] for vol in vols], origins, dims, device=dev)
    torch.cuda.synchronize()
    assert dropped == [0] * M
    for m, vol in enumerate(vols):
        want_sdf = sc.mesh_sdf(boxes[m][0], boxes[m][1], vol[1], 0, vol[2], origins[m], dims[m]).data
        got_sdf = grids[m].cpu().numpy()
        assert (want_sdf < 0).any() and np.array_equal(FC.bits(np.abs(got_sdf)), FC.bits(np.abs(want_sdf))) and np.array_equal(got_sdf < 0, want_sdf < 0), m
