"""Surface extraction on the MI355X (csrc/omg_surface.hip): omgx_surface_count / omgx_surface_gather against
scenes.surface_nets bit for bit around the 256-sample workgroup and the 64-lane wave; a ragged batch between sentinel rows against
single launches; the caller's pools with a cap; a scene table read in place; and the chains volume -> depth image and
volume -> grasps -> plans."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import mesh_cases as MC
from tests import surface_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _layout(c, offset=0):
    return (c["origin"], c["delta"], c["sample"], c["data"].shape, offset)


def _same(verts, faces, want_v, want_f):
    """verts as int64 bits and faces, device against specification."""
    return (torch.equal(verts.cpu().view(torch.int64), torch.from_numpy(np.array(want_v, np.float64)).view(torch.int64).reshape(-1, 3)) and
            torch.equal(faces.cpu(), torch.from_numpy(np.array(want_f, np.int32)).reshape(-1, 3)))


@pytest.mark.parametrize("name", SC.N24 + SC.EDGE + SC.GROUPS)
def test_device_equals_specification(dev, name):
    """One volume per launch: the 24^3 shapes (both sample offsets, levels 0, 0.01, -0.005), the edge cases of the text (NaN, inf,
    a sample equal to the level, no cells, all inside, a surface that leaves the grid), and volumes of 252, 256 and 294 samples,
    of several workgroups, and of z-extent 1, 2 and 65."""
    from omg_planner_amd import ops
    c = SC.case(name)
    want_v, want_f, want_o = SC.spec(name)
    verts, faces, open_edges = ops.surface_mesh(torch.from_numpy(c["data"]).to(dev), c["origin"], c["delta"], c["sample"], c["level"])
    assert verts.dtype == torch.float64 and faces.dtype == torch.int32 and tuple(verts.shape) == (len(want_v), 3) and tuple(faces.shape) == (len(want_f), 3)
    assert open_edges == want_o and _same(verts, faces, want_v, want_f)


RAGGED = ("17x9x5", "all_outside", "sphere_node_0.01")  # different sizes and sample offsets, one of them empty; one level per launch


def _pool_of(names, dev, gap=3):
    """The volumes back to back with `gap` elements of NaN between them -> (pool, layouts)."""
    parts, layouts, at = [], [], gap
    for n in names:
        c = SC.case(n)
        parts += [np.full(gap, np.nan, np.float32), c["data"].ravel()]
        layouts.append(_layout(c, at))
        at += c["data"].size + gap
    return torch.from_numpy(np.concatenate(parts + [np.full(gap, np.nan, np.float32)])).to(dev), layouts


def test_ragged_batch_between_sentinels_against_single_launches(dev):
    """Three volumes of different sizes in ONE launch through the C ABI, with host-assigned ranges that are neither contiguous nor
    in order, sentinel rows everywhere else in both output pools and around `counts`: every mesh equals its single launch (and
    the specification), and nothing outside the ranges is written."""
    from omg_planner_amd import _lib, ops
    level = 0.01
    cases = [dict(SC.case(n), level=level) for n in RAGGED]
    from omg_planner_amd import scenes
    want = [scenes.surface_nets(c["data"], c["origin"], c["delta"], c["sample"], level) for c in cases]
    assert len(want[1][1]) == 0 and len(want[0][1]) > 0 and len(want[2][1]) > 0
    pool, layouts = _pool_of(RAGGED, dev)
    for m, c in enumerate(cases):  # the single launches
        v, f, o = ops.surface_mesh(torch.from_numpy(c["data"]).to(dev), c["origin"], c["delta"], c["sample"], level)
        assert o == want[m][2] and _same(v, f, want[m][0], want[m][1]), m
    rec = ops.surface_records(layouts)
    l, vp, M = _lib.lib(), C.c_void_p, 3
    ptr = lambda t: vp(t.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(int(l.omgx_surface_workspace_bytes(C.cast(rec, vp), M)), dtype=torch.uint8, device=dev)
    counts = torch.full((M + 2, 4), -77, dtype=torch.int32, device=dev)
    up = lambda: torch.from_numpy(np.frombuffer(rec, np.uint8).copy()).to(dev)
    d_rec = up()
    assert l.omgx_surface_count(ptr(pool), pool.numel(), ptr(d_rec), C.cast(rec, vp), M, level, ptr(ws), vp(counts.data_ptr() + 16), stream) == 0
    h = counts.cpu().numpy()
    assert (h[0] == -77).all() and (h[-1] == -77).all()
    assert h[1:-1].tolist() == [[len(w[0]), len(w[1]), w[2], 0] for w in want]
    # mesh 2 first, then a hole, then mesh 0; the empty mesh 1 gets rows in the middle of the hole that must stay untouched
    nv, nf = [len(w[0]) for w in want], [len(w[1]) for w in want]
    vb, fb = [nv[2] + 7, nv[2] + 3, 2], [nf[2] + 11, nf[2] + 5, 1]
    for m in range(M):
        rec[m].vert_begin, rec[m].vert_count, rec[m].face_begin, rec[m].face_count = vb[m], nv[m], fb[m], nf[m]
    verts = torch.full((vb[0] + nv[0] + 5, 3), -7.5, dtype=torch.float64, device=dev)
    faces = torch.full((fb[0] + nf[0] + 5, 3), -7, dtype=torch.int32, device=dev)
    d_rec = up()
    assert l.omgx_surface_gather(ptr(pool), pool.numel(), ptr(d_rec), C.cast(rec, vp), M, level, ptr(ws), ptr(verts), verts.shape[0], ptr(faces),
                                 faces.shape[0], stream) == 0
    torch.cuda.synchronize()
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    untouched_v, untouched_f = np.ones(len(hv), bool), np.ones(len(hf), bool)
    for m in (0, 2):
        assert np.array_equal(SC.bits(hv[vb[m]: vb[m] + nv[m]]), SC.bits(want[m][0])) and np.array_equal(hf[fb[m]: fb[m] + nf[m]], want[m][1]), m
        untouched_v[vb[m]: vb[m] + nv[m]] = False
        untouched_f[fb[m]: fb[m] + nf[m]] = False
    assert untouched_v.sum() == len(hv) - nv[0] - nv[2] >= 12 and (hv[untouched_v] == -7.5).all()
    assert untouched_f.sum() == len(hf) - nf[0] - nf[2] >= 16 and (hf[untouched_f] == -7).all()
    # the same batch through the wrapper: back to back, in order
    v, f, vrows, frows, o = ops.surface_meshes(pool, layouts, level)
    assert vrows.tolist() == [[0, nv[0]], [nv[0], 0], [nv[0], nv[2]]] and frows.tolist() == [[0, nf[0]], [nf[0], 0], [nf[0], nf[2]]]
    assert o.tolist() == [w[2] for w in want] and _same(v, f, np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want]))


def test_callers_pools_with_a_cap_smaller_than_needed(dev):
    """out= with fewer rows than the meshes have: the rows that fit equal the specification, the tables still say what each mesh
    has, and nothing else changes (the tensors are larger than the `out` views handed over)."""
    from omg_planner_amd import ops
    names = ("252", "17x9x5_node")
    pool, layouts = _pool_of(names, dev)
    level = 0.0
    want = [SC.spec(n) for n in names]
    all_v, all_f = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    cap_v, cap_f = len(want[0][0]) + 9, len(want[0][1]) + 5   # cuts mesh 1; an odd face cap cuts the two triangles of one edge apart
    assert cap_f % 2 == 1 and cap_v < len(all_v) and cap_f < len(all_f)
    verts = torch.full((len(all_v) + 4, 3), -7.5, dtype=torch.float64, device=dev)
    faces = torch.full((len(all_f) + 4, 3), -7, dtype=torch.int32, device=dev)
    v, f, vrows, frows, o = ops.surface_meshes(pool, layouts, level, out=(verts[:cap_v], faces[:cap_f]))
    torch.cuda.synchronize()
    assert vrows[:, 1].tolist() == [len(w[0]) for w in want] and frows[:, 1].tolist() == [len(w[1]) for w in want] and o.tolist() == [w[2] for w in want]
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    assert np.array_equal(SC.bits(hv[:cap_v]), SC.bits(all_v[:cap_v])) and np.array_equal(hf[:cap_f], all_f[:cap_f])
    assert (hv[cap_v:] == -7.5).all() and (hf[cap_f:] == -7).all()


def _table_scenes():
    """2 scenes x 3 objects: a sphere, a box and a second sphere; the box's volume is one ndarray shared by both scenes."""
    from omg_planner_amd import scenes as sc
    box = sc.box_sdf(MC.BOX_HALF, shape=(32, 32, 32), delta=1.0 / 128)   # origin -0.125 and delta are exact in float32
    out = []
    for s in range(2):
        objs = [sc.SceneObject("ball", MC.pose((0.0, 0.0, 0.3 * s), (0.4, 0.1 * s, 0.2)), sc.sphere_sdf(0.05 + 0.01 * s, shape=(20, 18, 22), delta=1.0 / 128)),
                sc.SceneObject("box", MC.pose((0.1, 0.0, 0.2), (0.5, -0.2, 0.1 + 0.1 * s)), box),
                sc.SceneObject("ball2", MC.pose(t=(0.6, 0.2, 0.3)), sc.sphere_sdf(0.03, shape=(12, 12, 12), delta=0.01))]
        out.append(sc.Scene(objs, target_idx=1))
    return out


def _spec_of_record(table, k, grid, level=0.0):
    from omg_planner_amd import scenes as sc
    rec = table.host_objects[k]
    return sc.surface_nets(grid.data, rec["lo"].astype(np.float64), float(rec["delta"]), "centre", level)


def test_object_surfaces_of_a_scene_table_read_in_place(dev):
    from omg_planner_amd import ops
    from omg_planner_amd.config import Config
    scenes = _table_scenes()
    table = ops.DeviceScenes.from_scenes(scenes, Config().layer_kwargs(), device=dev)
    assert table.host_objects["grid_offset"][1] == table.host_objects["grid_offset"][4]  # the shared grid
    before = table.pool.cpu().numpy().tobytes()
    verts, faces, vrows, frows, open_edges = table.object_surfaces()
    torch.cuda.synchronize()
    assert table.pool.cpu().numpy().tobytes() == before
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    assert vrows[1].tolist() == vrows[4].tolist() and frows[1].tolist() == frows[4].tolist()  # extracted once
    assert vrows[:, 1].sum() - vrows[4, 1] == len(hv) and frows[:, 1].sum() - frows[4, 1] == len(hf)
    for s in range(2):
        for o in range(3):
            k = 3 * s + o
            wv, wf, wo = _spec_of_record(table, k, scenes[s].objects[o].sdf)
            assert len(wf) > 0 and wo == 0 == open_edges[k]
            assert np.array_equal(SC.bits(hv[vrows[k, 0]: vrows[k, 0] + vrows[k, 1]]), SC.bits(wv)), (s, o)
            assert np.array_equal(hf[frows[k, 0]: frows[k, 0] + frows[k, 1]], wf), (s, o)
    # named pairs, at another level, in the caller's order
    v2, f2, vr2, fr2, o2 = table.object_surfaces([(1, 2), (0, 0)], level=0.004)
    for row, (s, o) in enumerate([(1, 2), (0, 0)]):
        wv, wf, wo = _spec_of_record(table, 3 * s + o, scenes[s].objects[o].sdf, 0.004)
        assert _same(v2[vr2[row, 0]: vr2[row, 0] + vr2[row, 1]], f2[fr2[row, 0]: fr2[row, 0] + fr2[row, 1]], wv, wf) and o2[row] == wo


def test_observe_table_equals_the_depth_image_of_the_specifications_mesh(dev):
    """A one-box scene: the depth, instance and face images of observe_table equal camera.render_depth of the mesh
    scenes.surface_nets gives for the record's volume, at the record's pose, bit for bit."""
    from omg_planner_amd import camera as cam, ops, scenes as sc
    from omg_planner_amd.config import Config
    box = sc.box_sdf(MC.BOX_HALF, shape=(32, 32, 32), delta=1.0 / 128)
    scene = sc.Scene([sc.SceneObject("box", MC.pose((0.2, 0.1, -0.3), (0.02, -0.01, 0.5)), box)], target_idx=0)
    table = ops.DeviceScenes.from_scenes([scene], Config().layer_kwargs(), device=dev)
    H, W, intr, cfw = 40, 32, (100.0, 100.0, 15.5, 19.5), np.eye(4)
    obs = cam.observe_table(table, cfw, intr, H, W)
    torch.cuda.synchronize()
    wv, wf, wo = _spec_of_record(table, 0, box)
    pose = cam.table_object_poses(table)[0]
    assert np.abs(pose - scene.objects[0].pose_mat).max() < 1e-6
    inst = cam.instance_records([(wv, wf)], [0], [pose], [0], cfw)
    t, ii, ff = cam.render_depth([(wv, wf)], inst, [0, 1], cam.camera_rows(intr, cfw)[None], H, W)
    assert np.isfinite(t).sum() > 50 and (ii == -1).sum() > 50
    assert np.array_equal(SC.bits(obs.t.cpu().numpy()), SC.bits(t)) and np.array_equal(obs.inst.cpu().numpy(), ii) and np.array_equal(obs.face.cpu().numpy(), ff)
    cloud = obs.clouds(0)[0]
    assert cloud.shape[0] == int(np.isfinite(t).sum())


def _plan_scenes(grid):
    """Two tabletop scenes whose target is `grid`'s object standing on its 0.10 x 0.06 side (test_gpu_grasp_sampling.py's scenes)."""
    from omg_planner_amd import scenes as sc
    stand = MC.pose((np.pi / 2, 0.0, 0.0))
    out = []
    for seed in (3, 4):
        scene = sc.make_tabletop_scene(seed, num_objects=1, grid=32, table_grid=(48, 32, 16))
        scene.objects[0] = sc.SceneObject("box", sc._yaw_pose(0.5, 0.0, 0.125, 0.4 + 0.5 * (seed - 3)) @ stand, grid)
        out.append(scene)
    return out


def test_plan_volumes_equals_plan_meshes_on_the_specifications_meshes(dev):
    """plan_volumes on two tabletop scenes whose box target exists only as a volume: the extracted meshes equal the specification's,
    and the grasp sets, trajectories and goals equal plan_meshes fed with the specification's meshes and the same streams.  A target
    whose surface leaves its grid is refused, and so is one without a surface."""
    from omg_planner_amd import pipeline, robot as rb, scenes as sc
    from omg_planner_amd.config import Config
    cfg = Config(use_standoff=True, timeout=-1, silent=True)
    model = rb.PandaModel()
    box = sc.box_sdf(MC.BOX_HALF, shape=(32, 32, 32), delta=1.0 / 128)
    scenes = _plan_scenes(box)
    assert scenes[0].target_idx == 0
    start = np.tile(np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785, 0.04, 0.04]), (2, 1))
    rngs = lambda: [np.random.RandomState(7), np.random.RandomState(8)]
    kw = dict(n_rays=256, n_angles=8, ol_alg="MD", max_grasps=64, device=dev, cone=np.deg2rad(15.0))
    res, sets, meshes = pipeline.plan_volumes(model, scenes, start, cfg, rng=np.random.RandomState(0), grasp_rng=rngs(), **kw)
    wv, wf, wo = sc.surface_nets(box)
    assert wo == 0
    for v, f in meshes:
        assert np.array_equal(SC.bits(v), SC.bits(wv)) and np.array_equal(f, wf)
    ref, ref_sets = pipeline.plan_meshes(model, scenes, [(wv, wf)] * 2, start, cfg, rng=np.random.RandomState(0), grasp_rng=rngs(), **kw)
    print("grasps", [len(s) for s in sets], "goals", res.goal_counts.tolist(), "planned", res.planned.tolist())
    assert all(np.array_equal(a, b) for a, b in zip(sets, ref_sets)) and all(len(s) > 0 for s in sets)
    assert res.planned.any() and np.array_equal(res.planned, ref.planned)
    assert torch.equal(res.traj, ref.traj) and torch.equal(res.goal_idx, ref.goal_idx) and torch.equal(res.goal_set, ref.goal_set)
    cut = sc.SdfGrid(np.ascontiguousarray(box.data[:, :, :16]), box.origin, box.delta)  # the box sticks out of its grid
    with pytest.raises(ValueError, match=r"scene 1: .*open edges"):
        pipeline.plan_volumes(model, [scenes[0]] + _plan_scenes(cut)[1:], start, cfg, **kw)
    with pytest.raises(ValueError, match=r"scene 0: .*empty"):
        pipeline.plan_volumes(model, scenes, start, cfg, level=-1.0, **kw)


def test_random_volumes_levels_and_batches(dev):
    """Random smooth volumes with dims 2..20 per axis and a random level each, in random batch compositions (one launch takes one
    level: the volumes of a batch are extracted at the level of its first), device against specification."""
    from omg_planner_amd import ops, scenes as sc
    rng = np.random.default_rng(11)
    for _ in range(6):
        names = [SC.SMOOTH[i] for i in rng.choice(len(SC.SMOOTH), int(rng.integers(1, 6)), replace=False)]
        level = SC.case(names[0])["level"]
        pool, layouts = _pool_of(names, dev, gap=int(rng.integers(0, 5)))
        v, f, vrows, frows, o = ops.surface_meshes(pool, layouts, level)
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        for m, n in enumerate(names):
            c = SC.case(n)
            wv, wf, wo = SC.spec(n) if m == 0 else sc.surface_nets(c["data"], c["origin"], c["delta"], c["sample"], level)
            assert o[m] == wo and np.array_equal(SC.bits(hv[vrows[m, 0]: vrows[m, 0] + vrows[m, 1]]), SC.bits(wv)), (names, m)
            assert np.array_equal(hf[frows[m, 0]: frows[m, 0] + frows[m, 1]], wf), (names, m)
