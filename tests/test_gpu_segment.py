"""Object segmentation on the MI355X (csrc/omg_segment.hip): omgx_label_components /
omgx_component_records / omgx_component_states against segmentation.py, integer for integer: every case as one ragged launch set
per connectivity between guard bytes, the same batch as single calls, the observed scene segmented into a scene table's pool,
plan_observed against plan_volumes on the specification's volumes, and a short seeded fuzz run.  Every launch is followed by a
checked synchronise.  The labelling's launches do not depend on the data and hold no loop that waits, so a step that does not
return is a hang: run the tests one by one under a time limit where that matters."""
from __future__ import annotations

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import segment_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("connectivity,select", [(6, 1), (18, 1), (26, 1), (6, 2), (18, 3)])
def test_every_case_as_one_ragged_launch_set_through_the_c_abi(dev, connectivity, select):
    """All the cases of tests/segment_cases.py (the serpentine, the combs, the checkerboard, the cubes, the bar and the line over
    several workgroups, dims of one, empty and full volumes, the random fields, 64 x 64 x 40) as ONE batch between SURFACE guard
    bytes: labels (the guards -1), counts, records and the cropped states of the picks equal the specification."""
    from omg_planner_amd import _lib, ops, segmentation as sg
    volumes, state, begin = SC.batch()
    want = sg.label_components(state, volumes, select, connectivity, state_begin=begin)
    comp_begin, records = sg.component_records(want, volumes, begin)
    picks, outs, ob = SC.picks_for(volumes, comp_begin, records, seed=connectivity + select)
    cropped = sg.component_states(state, volumes, begin, want, comp_begin, records, picks, outs, ob)
    if select == 1:
        for m, name in enumerate(SC.BATCH):
            known = SC.cases()[name][1]
            assert known is None or comp_begin[m + 1] - comp_begin[m] == known[SC.CONNECTIVITIES.index(connectivity)], name

    l, vp, M, K = _lib.lib(), C.c_void_p, len(volumes), len(picks)
    assert _lib.SEGMENT_NODES_PER_WORKGROUP == SC.N
    ptr = lambda x: vp(x.data_ptr())
    up = lambda a: torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy() if isinstance(a, C.Array) else np.ascontiguousarray(a)).to(dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    rec, out_rec = ops.surface_records([v + (0,) for v in volumes]), ops.surface_records([o + (0,) for o in outs])
    elems = len(state)
    d_state, d_rec, d_begin = up(state), up(rec), up(begin)
    ws = torch.empty(int(l.omgx_label_workspace_bytes(C.cast(rec, vp), M)), dtype=torch.uint8, device=dev)
    labels = torch.full((elems,), 12345, dtype=torch.int32, device=dev)
    counts = torch.full((M,), -5, dtype=torch.int32, device=dev)
    assert l.omgx_label_components(ptr(d_state), elems, ptr(d_begin), vp(begin.ctypes.data), ptr(d_rec), C.cast(rec, vp), M, select, connectivity,
                                   ptr(ws), ptr(labels), ptr(counts), stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(counts.cpu().numpy(), np.diff(comp_begin))
    assert np.array_equal(d_state.cpu().numpy(), state)  # the states are only read
    total = int(comp_begin[-1])
    d_comp = up(comp_begin)
    d_records = torch.full((total + 3, 8), -77, dtype=torch.int32, device=dev)
    assert l.omgx_component_records(ptr(labels), elems, ptr(d_begin), vp(begin.ctypes.data), ptr(d_rec), C.cast(rec, vp), M, ptr(d_comp),
                                    vp(comp_begin.ctypes.data), ptr(d_records), total + 3, stream) == 0
    torch.cuda.synchronize()
    got = d_records.cpu().numpy()
    assert np.array_equal(got[:total], records) and (got[total:] == -77).all()
    out_elems = int(ob[-1]) + int(np.prod(outs[-1][3])) + 4
    out = torch.full((out_elems,), 0xAB, dtype=torch.uint8, device=dev)
    h_picks = np.ascontiguousarray(picks, np.int32)
    d_picks, d_out_rec, d_ob = up(h_picks), up(out_rec), up(ob)
    assert l.omgx_component_states(ptr(d_state), elems, ptr(d_begin), vp(begin.ctypes.data), ptr(d_rec), C.cast(rec, vp), M, ptr(labels), ptr(d_comp),
                                   vp(comp_begin.ctypes.data), ptr(d_records), total, ptr(d_picks), vp(h_picks.ctypes.data), ptr(d_out_rec),
                                   C.cast(out_rec, vp), K, ptr(d_ob), vp(ob.ctypes.data), ptr(out), out_elems, stream) == 0
    torch.cuda.synchronize()
    got, written = out.cpu().numpy(), np.zeros(out_elems, bool)
    for k, o in enumerate(outs):
        n = int(np.prod(o[3]))
        assert np.array_equal(got[ob[k]: ob[k] + n], cropped[ob[k]: ob[k] + n]), (k, picks[k].tolist())
        written[ob[k]: ob[k] + n] = True
    assert K > 60 and (~written).sum() > K and (got[~written] == 0xAB).all()
    # an empty batch launches nothing
    assert l.omgx_label_components(None, 0, None, None, None, None, 0, select, connectivity, None, None, None, stream) == 0
    assert l.omgx_component_states(ptr(d_state), elems, ptr(d_begin), vp(begin.ctypes.data), ptr(d_rec), C.cast(rec, vp), M, ptr(labels), ptr(d_comp),
                                   vp(comp_begin.ctypes.data), ptr(d_records), total, None, None, None, None, 0, None, None, None, 0, stream) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("connectivity", SC.CONNECTIVITIES)
def test_the_same_batch_as_single_calls(dev, connectivity):
    """Every volume of the batch on its own through ops.label_components and ops.component_states: the same labels, records and
    cropped states as the specification gives for it (so: as the batch gives)."""
    from omg_planner_amd import ops, segmentation as sg
    volumes, state, begin = SC.batch()
    for m, (name, v) in enumerate(zip(SC.BATCH, volumes)):
        if name == "big" and connectivity != 6:
            continue
        n = int(np.prod(v[3]))
        s = state[begin[m]: begin[m] + n]
        want = sg.label_components(s, [v], 1, connectivity)
        comp_begin, records = sg.component_records(want, [v])
        comps = ops.label_components(torch.from_numpy(s.copy()).to(dev), None, [v], 1, connectivity)
        torch.cuda.synchronize()
        assert np.array_equal(comps.labels.cpu().numpy(), want), name
        assert np.array_equal(comps.comp_begin, comp_begin) and np.array_equal(comps.records, records) and comps.counts.tolist() == [len(records)], name
        assert np.array_equal(comps.d_records.cpu().numpy(), records)
        picks, outs, ob = SC.picks_for([v], comp_begin, records, seed=m, per_volume=1)
        if len(picks):
            got, got_begin = ops.component_states(torch.from_numpy(s.copy()).to(dev), comps, picks, outs)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), sg.component_states(s, [v], None, want, comp_begin, records, picks, outs)), name
    # the wrapper on the whole batch at the caller's offsets, and component_volumes into a pool
    d_state = torch.from_numpy(state).to(dev)
    comps = ops.label_components(d_state, begin, volumes, 1, connectivity)
    torch.cuda.synchronize()
    want = sg.label_components(state, volumes, 1, connectivity, state_begin=begin)
    comp_begin, records = sg.component_records(want, volumes, begin)
    assert np.array_equal(comps.labels.cpu().numpy(), want) and np.array_equal(comps.records, records) and np.array_equal(comps.comp_begin, comp_begin)
    from omg_planner_amd import fusion
    picks, outs, _ = SC.picks_for(volumes[:6], comp_begin[:7], records, seed=3, per_volume=1)
    pool = ops.component_volumes(d_state, comps, picks, outs, 4, True)
    torch.cuda.synchronize()
    cropped = sg.component_states(state, volumes, begin, want, comp_begin, records, picks, outs)
    vols = fusion.distance_transform(cropped, outs, 4, True)
    assert np.array_equal(_bits(pool), np.concatenate([FC.bits(v).ravel() for v in vols]))


def _scene(pose, n=1):
    """n scenes of a target and an obstacle object (placeholders) at `pose` and a table slab; the target is object 0."""
    from omg_planner_amd import scenes as sc
    slab = sc.box_sdf((0.6, 0.4, 0.02), (24, 16, 8), 1.5 / 24)
    return [sc.Scene([sc.SceneObject("target", pose, sc.sphere_sdf(0.05, (8, 8, 8), 0.05)), sc.SceneObject("obstacles", pose, sc.sphere_sdf(0.04, (8, 8, 8), 0.05)),
                      sc.SceneObject("table", sc._yaw_pose(0.5, 0.0, -0.3, 0.0), slab)], 0) for _ in range(n)]


def _render(dev, which):
    from omg_planner_amd import ops
    meshes, inst, begin, cams = SC.observed_records(which)
    batch = ops.CameraBatch(meshes, inst, begin, cams, device=dev)
    return (batch,) + tuple(ops.render_depth(batch, FC.H, FC.W))


def _check_pool(table, scene, obj, grid, pose):
    """The object's volume in the pool has the specification's bits, and its record the limits of a table built on the host."""
    from omg_planner_amd import ops, scenes as sc
    rec = table.sync_host()[table._index(scene, obj)]
    off = int(rec["grid_offset"])
    assert tuple(rec["dim"]) == grid.data.shape and np.array_equal(_bits(table.pool[off: off + grid.data.size]), FC.bits(grid.data).ravel()), (scene, obj)
    host = ops.DeviceScenes.from_scenes([sc.Scene([sc.SceneObject("x", pose, grid)], 0)], device=table.device).sync_host()[0]
    for name in ("lo", "hi", "dim", "delta", "inv_delta", "pose_inv"):
        assert np.array_equal(rec[name], host[name]), (scene, obj, name)


def test_observed_scene_segmented_into_a_scene_table(dev):
    """The sphere and the box on the slab rendered by ops.render_depth, the slab's pixels taken out by camera.explained_mask of
    the slab's own rendering, segmented by DeviceScenes.segment_obstacles from the three views: the pool holds the
    specification's target crop and its obstacle volume bit for bit, the records have the limits replace_grid writes, the chosen
    record is the specification's.  Then camera.Observation.segment_obstacles: three scenes, each seen by its own camera, with the
    box as the target, in one set of launches."""
    from omg_planner_amd import camera, fusion, ops, scenes as sc, segmentation as sg
    batch, t, inst_img, face_img = _render(dev, (0, 1, 2))
    _, t_known, _, _ = _render(dev, (2,))
    torch.cuda.synchronize()
    want_t, want_known, views = SC.observed_depth()
    assert np.array_equal(t.cpu().numpy().view(np.int64), want_t.view(np.int64)) and np.array_equal(t_known.cpu().numpy().view(np.int64), want_known.view(np.int64))
    mask = camera.explained_mask(t, t_known, SC.TOL)
    assert np.array_equal(mask.cpu().numpy(), sg.explained_mask(want_t, want_known, SC.TOL))
    lifted = sc._yaw_pose(0.0, 0.0, 0.3, 0.0)
    nodes = int(np.prod(FC.DIMS))
    table = ops.DeviceScenes.from_scenes(_scene(lifted), device=dev, share_grids=False, reserve_voxels=8 * nodes)  # (two calls, a larger crop in the second)
    for conn in (6, 26):
        want = SC.observed_segmentation(conn)
        radius, records, comps = table.segment_obstacles([(0, 0)], [(0, 1)], t, views, [(0, 3)], [SC.LAYOUT], SC.BAND, SC.NEAR, SC.REACH, [SC.SEED_POINT],
                                                         SC.MIN_NODES, connectivity=conn, free_mask=mask)
        torch.cuda.synchronize()
        assert radius == fusion.obstacle_radius(SC.REACH, FC.DELTA) and not table._slots.pending
        assert np.array_equal(records, want["record"][None]) and np.array_equal(comps.records, want["records"])
        assert np.array_equal(comps.labels.cpu().numpy(), want["labels"])
        _check_pool(table, 0, 0, want["target"], lifted)
        _check_pool(table, 0, 1, want["obstacle"], lifted)
    assert np.array_equal(t.cpu().numpy().view(np.int64), want_t.view(np.int64))  # the caller's images are not changed
    # a scene without a component of min_nodes nodes is refused before a slot is offered
    with pytest.raises(Exception, match="no component has"):
        table.segment_obstacles([(0, 0)], [(0, 1)], t, views, [(0, 3)], [SC.LAYOUT], SC.BAND, SC.NEAR, SC.REACH, [SC.SEED_POINT], 5000, free_mask=mask)
    assert not table._slots.pending
    # every other refusal comes before a slot is offered as well, and the table still takes a good call
    good = dict(target_pairs=[(0, 0)], obstacle_pairs=[(0, 1)], depth=t, views=views, view_range=[(0, 3)], layouts=[SC.LAYOUT], band=SC.BAND, near=SC.NEAR,
                reach=SC.REACH, seeds=[SC.SEED_POINT], min_nodes=SC.MIN_NODES, free_mask=mask)
    for what, change in (("layouts need as many", dict(layouts=[SC.LAYOUT] * 2)), ("layouts need as many", dict(seeds=[SC.SEED_POINT] * 2)),
                         ("layouts need as many", dict(target_pairs=[], obstacle_pairs=[], layouts=[], seeds=[])),
                         ("named twice", dict(target_pairs=[(0, 1)])), ("reach must be finite", dict(reach=float("nan"))),
                         ("seeds must be finite", dict(seeds=[(0.0, float("nan"), 0.0)])), ("seeds must be finite", dict(min_nodes=0)),
                         ("seeds must be finite", dict(margin=-1)), ("connectivity must be 6, 18 or 26", dict(connectivity=8)),
                         ("radius must lie in", dict(reach=2.6)), ("view_range", dict(view_range=[(1, 3)])), ("band and near must be finite", dict(band=float("inf"))),
                         ("dims >= 1", dict(layouts=[(FC.ORIGIN, FC.DELTA, (32, 0, 24))])), ("depth must be torch.float64", dict(depth=t.float())),
                         ("free_mask must be a bool tensor", dict(free_mask=torch.zeros_like(t)))):
        with pytest.raises(Exception, match=what):
            table.segment_obstacles(**{**good, **change})
        assert not table._slots.pending, what
    with pytest.raises(IndexError):
        table.segment_obstacles(**{**good, "obstacle_pairs": [(1, 1)]})
    assert table.segment_obstacles(**good)[0] == fusion.obstacle_radius(SC.REACH, FC.DELTA) and not table._slots.pending
    torch.cuda.synchronize()
    _check_pool(table, 0, 0, SC.observed_segmentation(6)["target"], lifted)
    # one camera per scene, no instance image
    eye = np.eye(4)  # (the images were rendered with the objects in the world's frame: the layout's frame is the world's here)
    three = ops.DeviceScenes.from_scenes(_scene(eye, 3), device=dev, share_grids=False, reserve_voxels=3 * 4 * nodes)
    obs = camera.Observation(batch, t, None, None)
    tp, op = [(s, 0) for s in range(3)], [(s, 1) for s in range(3)]
    own_views = obs.view_rows(three, op)
    radius, records, comps = obs.segment_obstacles(three, tp, op, [SC.LAYOUT] * 3, SC.BAND, SC.NEAR, SC.REACH, [SC.BOX_C] * 3, 40, free_mask=mask)
    torch.cuda.synchronize()
    h_mask = mask.cpu().numpy()
    for s in range(3):
        want = sg.segment_views(SC.LAYOUT, own_views[s: s + 1], want_t[s: s + 1], SC.BAND, SC.NEAR, radius, SC.BOX_C, 40, 6, free_mask=h_mask[s: s + 1])
        assert np.array_equal(records[s], want["record"]) and np.array_equal(comps.of(s), want["records"]), s
        _check_pool(three, s, 0, want["target"], eye)
        _check_pool(three, s, 1, want["obstacle"], eye)


def test_plan_observed_against_plan_volumes_on_the_specifications_volumes(dev):
    """Two tabletop scenes whose target (the box) and obstacles exist only in the depth image of the scene's camera: plan_observed
    gives the planned flags, the goal counts and the grasp sets of plan_volumes run on scenes that hold the specification's two
    volumes (segmentation.segment_views)."""
    from omg_planner_amd import camera, ops, pipeline, robot as rb, scenes as sc, segmentation as sg
    from omg_planner_amd.config import Config
    cfg = Config(use_standoff=True, timeout=-1, silent=True)
    model = rb.PandaModel()
    poses = [sc._yaw_pose(0.5, 0.0, 0.125, 0.4 + 0.5 * k) for k in range(2)]

    def make():
        out = []
        for k, seed in enumerate((3, 4)):
            scene = sc.make_tabletop_scene(seed, num_objects=1, grid=32, table_grid=(48, 32, 16))
            scene.objects[0] = sc.SceneObject("target", poses[k], sc.sphere_sdf(0.05, (8, 8, 8), 0.05))
            scene.objects.append(sc.SceneObject("obstacles", poses[k], sc.sphere_sdf(0.04, (8, 8, 8), 0.05)))
            assert scene.target_idx == 0
            out.append(scene)
        return out

    scenes = make()
    obstacle_idx = [len(s.objects) - 1 for s in scenes]
    # the observed objects stand at the scenes' poses; scene k is seen by camera k of the three, moved with the pose
    cfw, intr = FC.scene_cameras()
    meshes = SC.observed_meshes()
    recs = [camera.instance_records(meshes, [0, 1, 2], [poses[k]] * 3, [1, 1, 1], cfw[k] @ np.linalg.inv(poses[k])) for k in range(2)]
    known = [camera.instance_records(meshes, [2], [poses[k]], [1], cfw[k] @ np.linalg.inv(poses[k])) for k in range(2)]
    cams = np.stack([camera.camera_rows(intr, cfw[k] @ np.linalg.inv(poses[k])) for k in range(2)])
    batch = ops.CameraBatch(meshes, np.concatenate(recs), np.array([0, 3, 6], np.int64), cams, device=dev)
    t = ops.render_depth(batch, FC.H, FC.W)[0]
    t_known = ops.render_depth(ops.CameraBatch(meshes, np.concatenate(known), np.array([0, 1, 2], np.int64), cams, device=dev), FC.H, FC.W)[0]
    torch.cuda.synchronize()
    mask = camera.explained_mask(t, t_known, SC.TOL)
    obs = camera.Observation(batch, t, None, None)
    start = np.tile(np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785, 0.04, 0.04]), (2, 1))
    rngs = lambda: [np.random.RandomState(7), np.random.RandomState(8)]
    kw = dict(n_rays=256, n_angles=8, ol_alg="MD", max_grasps=64, cone=np.deg2rad(15.0))
    res, sets, found, records = pipeline.plan_observed(model, scenes, obs, obstacle_idx, [SC.LAYOUT] * 2, SC.BAND, SC.NEAR, SC.REACH, [SC.BOX_C] * 2, 40,
                                                       start, cfg, free_mask=mask, device=dev, rng=np.random.RandomState(0), grasp_rng=rngs(), **kw)
    torch.cuda.synchronize()
    # the specification: the same images and view rows on the host, the volumes put into fresh scenes
    ref_scenes = make()
    table = ops.DeviceScenes.from_scenes(ref_scenes, cfg.layer_kwargs(), device=dev, share_grids=False)
    views = obs.view_rows(table, [(k, obstacle_idx[k]) for k in range(2)])
    h_t, h_mask = t.cpu().numpy(), mask.cpu().numpy()
    from omg_planner_amd import fusion
    radius = fusion.obstacle_radius(SC.REACH, FC.DELTA)
    for k in range(2):
        want = sg.segment_views(SC.LAYOUT, views[k: k + 1], h_t[k: k + 1], SC.BAND, SC.NEAR, radius, SC.BOX_C, 40, 6, free_mask=h_mask[k: k + 1])
        assert np.array_equal(records[k], want["record"]), k
        ref_scenes[k].objects[0].sdf, ref_scenes[k].objects[obstacle_idx[k]].sdf = want["target"], want["obstacle"]
        for o, g in ((0, want["target"]), (obstacle_idx[k], want["obstacle"])):
            assert np.array_equal(FC.bits(scenes[k].objects[o].sdf.data), FC.bits(g.data)) and np.array_equal(scenes[k].objects[o].sdf.origin, g.origin), (k, o)
    ref, ref_sets, ref_found = pipeline.plan_volumes(model, ref_scenes, start, cfg, device=dev, rng=np.random.RandomState(0), grasp_rng=rngs(), **kw)
    print("grasps", [len(s) for s in sets], "goals", res.goal_counts.tolist(), "planned", res.planned.tolist())
    assert all(len(s) > 0 for s in sets) and all(np.array_equal(a, b) for a, b in zip(sets, ref_sets))
    assert np.array_equal(res.planned, ref.planned) and np.array_equal(res.goal_counts, ref.goal_counts)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(found, ref_found))


def test_a_short_seeded_fuzz_run(dev):
    spec = importlib.util.spec_from_file_location("fuzz_segment", Path(__file__).resolve().parent / "fuzz" / "fuzz_segment.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    assert fuzz.main(trials=fuzz.SMOKE_TRIALS, seed=fuzz.SMOKE_SEED) == 0
