"""Support-plane fitting on the MI355X (csrc/omg_plane.hip): omgx_plane_ransac / omgx_plane_moments /
omgx_plane_mask / omgx_plane_volumes against planes.py, bit for bit: every case of tests/plane_cases.py as one batch of views
between guard values and as single-view calls, the wrappers, the observed scene segmented with the fitted support in place of the
known one, the half-space volume in a scene table, plan_on_unknown_support against plan_observed, and a short seeded fuzz run.
Every launch is followed by a checked synchronise.  The launches do not depend on the data and hold no loop that waits, so a step
that does not return is a hang: run the tests one by one under a time limit where that matters."""
from __future__ import annotations

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import plane_cases as PC
from tests import segment_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD_F, GUARD_I, GUARD_B = -7.25, -77, 0xAB


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_plane", Path(__file__).resolve().parent / "fuzz" / "fuzz_plane.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz


def _abi(dev, c, want):
    """One case through the four image entry points between guard values -> nothing; asserts."""
    from omg_planner_amd import _lib
    l, vp = _lib.lib(), C.c_void_p
    ptr = lambda x: None if x is None else vp(x.data_ptr())
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    intr, tri = np.ascontiguousarray(c["intr"], np.float64), np.ascontiguousarray(c["triples"], np.int32)
    V, H, W = c["depth"].shape
    K, PAD = tri.shape[1], 5
    d_intr, d_depth, d_tri = up(intr), up(c["depth"]), up(tri)
    d_skip = None if c["skip"] is None else up(c["skip"].astype(np.uint8))
    d_up = None if c["up"] is None else up(np.ascontiguousarray(c["up"], np.float64))
    f64 = lambda n: torch.full((n + PAD,), GUARD_F, dtype=torch.float64, device=dev)
    i32 = lambda n: torch.full((n + PAD,), GUARD_I, dtype=torch.int32, device=dev)
    planes, counts, best, best_planes, anchors = f64(V * K * 4), i32(V * K), i32(V), f64(V * 4), f64(V * 3)
    assert l.omgx_plane_ransac(ptr(d_intr), vp(intr.ctypes.data), ptr(d_depth), ptr(d_skip), V, H, W, ptr(d_tri), vp(tri.ctypes.data), K, c["tol"],
                               c["min_nn"], ptr(d_up), c["cos_min"], ptr(planes), ptr(counts), ptr(best), ptr(best_planes), ptr(anchors), stream) == 0
    torch.cuda.synchronize()

    def same(t, w, what):
        g, w = t.cpu().numpy(), np.ascontiguousarray(w).reshape(-1)
        n = w.size
        if w.dtype == np.float64:
            assert np.array_equal(g[:n].view(np.uint64), w.view(np.uint64)), what
            assert (g[n:] == GUARD_F).all(), what
        else:
            assert np.array_equal(g[:n], w), what
            assert (g[n:] == (GUARD_I if w.dtype == np.int32 else GUARD_B)).all(), what

    same(planes, want["hyp"], "planes"), same(counts, want["counts"], "counts"), same(best, want["best"], "best")
    same(best_planes, want["best_planes"], "best planes"), same(anchors, want["anchors"], "anchors")
    ws = torch.empty(int(l.omgx_plane_workspace_bytes(V, H, W)) + 8, dtype=torch.uint8, device=dev)
    count, sums = i32(V), f64(V * 9)
    assert l.omgx_plane_moments(ptr(d_intr), vp(intr.ctypes.data), ptr(d_depth), ptr(d_skip), V, H, W, ptr(best_planes), ptr(anchors), c["tol"], ptr(ws),
                                ptr(count), ptr(sums), stream) == 0
    torch.cuda.synchronize()
    same(count, want["count"], "count"), same(sums, want["sums"], "sums")
    d_final = up(np.ascontiguousarray(want["final"]))
    mask = torch.full((V * H * W + PAD,), GUARD_B, dtype=torch.uint8, device=dev)
    assert l.omgx_plane_mask(ptr(d_intr), vp(intr.ctypes.data), ptr(d_depth), ptr(d_skip), V, H, W, ptr(d_final), c["tol"], ptr(mask), stream) == 0
    torch.cuda.synchronize()
    same(mask, want["mask"].astype(np.uint8), "mask")
    assert np.array_equal(d_depth.cpu().numpy().view(np.uint64), c["depth"].view(np.uint64))  # the images are only read


@pytest.mark.parametrize("name", sorted(PC.cases()))
def test_every_case_through_the_c_abi_as_one_batch_and_as_single_views(dev, name):
    """Planes as uint64 bits, counts and best integer for integer, sums as bits, masks byte for byte, all between guard values;
    then every view of the batch as a call of its own."""
    fuzz = _fuzz()
    c = dict(PC.cases()[name])
    c.update(volumes=[], volume_planes=np.zeros((0, 4)), pool=0)
    want = fuzz.specification(c)
    _abi(dev, c, want)
    V = c["depth"].shape[0]
    for v in range(V if V > 1 else 0):
        one = dict(c)
        for key in ("intr", "depth", "triples", "skip", "up"):
            one[key] = None if c[key] is None else np.ascontiguousarray(c[key][v: v + 1])
        _abi(dev, one, {k: w[v: v + 1] for k, w in want.items() if k != "pool"})
    from omg_planner_amd import _lib
    assert _lib.lib().omgx_plane_ransac(None, None, None, None, 0, 0, 0, None, None, 1, 0.0, 0.0, None, -1.0, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()


def test_volumes_through_the_c_abi_as_a_ragged_batch_and_as_single_calls(dev):
    """The half-space volumes as uint32 bits, written into a pool between guards as ONE launch, then volume by volume."""
    from omg_planner_amd import _lib, ops, planes
    l, vp = _lib.lib(), C.c_void_p
    layout, size = PC.pool_layout()
    want = np.full(size, GUARD_F, np.float32)
    for v, p in zip(layout, PC.VOLUME_PLANES):
        want[v[4]: v[4] + int(np.prod(v[3]))] = planes.halfspace_volume(v[:4], p).ravel()
    stream = vp(torch.cuda.current_stream().cuda_stream)
    up = lambda a: torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy() if isinstance(a, C.Array) else np.ascontiguousarray(a)).to(dev)

    def run(vols, pls, pool):
        rec, h = ops.surface_records(vols), np.ascontiguousarray(pls, np.float64)
        d_rec, d_pl = up(rec), up(h)
        assert l.omgx_plane_volumes(vp(d_rec.data_ptr()), C.cast(rec, vp), len(vols), vp(d_pl.data_ptr()), vp(h.ctypes.data), vp(pool.data_ptr()),
                                    int(pool.numel()), stream) == 0
        torch.cuda.synchronize()

    pool = torch.full((size,), GUARD_F, dtype=torch.float32, device=dev)
    run(layout, PC.VOLUME_PLANES, pool)
    assert np.array_equal(_bits(pool), want.view(np.uint32)) and (want == np.float32(GUARD_F)).sum() == (len(layout) + 1) * PC.POOL_GUARD
    pool = torch.full((size,), GUARD_F, dtype=torch.float32, device=dev)
    for v, p in zip(layout, PC.VOLUME_PLANES):
        run([v], [p], pool)
    assert np.array_equal(_bits(pool), want.view(np.uint32))
    got = ops.plane_volumes(PC.VOLUMES, PC.VOLUME_PLANES, device=dev)  # back to back in a new buffer
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got), np.concatenate([planes.halfspace_volume(v, p).ravel() for v, p in zip(PC.VOLUMES, PC.VOLUME_PLANES)]).view(np.uint32))


def _observed_case():
    return dict(intr=np.tile(PC.observed_intrinsics(), (3, 1)), depth=SC.observed_depth()[0], triples=PC.observed_triples(), tol=SC.TOL, min_nn=1e-10,
                skip=None, up=None, cos_min=-1.0)


@pytest.mark.parametrize("name", sorted(PC.cases()) + ["observed", "noisy"])
def test_ops_fit_planes_and_plane_mask_equal_the_specification(dev, name):
    """ops.fit_planes against planes.fit_planes: the same host code refines the same moments, so the planes are equal bit for
    bit, with the counts, the inliers and the status; ops.plane_mask is the specification's mask; skip = that mask gives the
    specification's next plane."""
    from omg_planner_amd import ops, planes
    c = PC.cases()[name] if name in PC.cases() else _observed_case()
    if name == "noisy":
        c = dict(c, depth=PC.noisy_depth(3))
    depth = torch.from_numpy(c["depth"]).to(dev)
    skip = None if c["skip"] is None else torch.from_numpy(c["skip"]).to(dev)
    kw = dict(up=c["up"], cos_min=c["cos_min"], min_nn=c["min_nn"])
    want = planes.fit_planes(c["intr"], c["depth"], c["triples"], c["tol"], skip=c["skip"], **kw)
    got = ops.fit_planes(c["intr"], depth, c["triples"], c["tol"], skip=skip, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(PC.bits(got.h_planes), PC.bits(want.planes)) and np.array_equal(PC.bits(got.planes.cpu().numpy()), PC.bits(want.planes))
    assert np.array_equal(PC.bits(got.hypotheses.cpu().numpy()), PC.bits(want.hypotheses)) and np.array_equal(got.counts.cpu().numpy(), want.counts)
    assert np.array_equal(got.best.cpu().numpy(), want.best) and np.array_equal(got.h_best, want.best) and np.array_equal(got.ransac_counts, want.ransac_counts)
    assert np.array_equal(got.inliers, want.inliers) and np.array_equal(got.status, want.status) and np.array_equal(PC.bits(got.anchors), PC.bits(want.anchors))
    mask = ops.plane_mask(c["intr"], depth, got.planes, c["tol"], skip)
    torch.cuda.synchronize()
    want_mask = planes.plane_mask(c["intr"], c["depth"], want.planes, c["tol"], c["skip"])
    assert mask.dtype == torch.bool and mask.shape == depth.shape and np.array_equal(mask.cpu().numpy(), want_mask)
    if c["skip"] is None:
        again = ops.fit_planes(c["intr"], depth, c["triples"], c["tol"], skip=mask, **kw)
        torch.cuda.synchronize()
        want_again = planes.fit_planes(c["intr"], c["depth"], c["triples"], c["tol"], skip=want_mask, **kw)
        assert np.array_equal(PC.bits(again.h_planes), PC.bits(want_again.planes)) and np.array_equal(again.counts.cpu().numpy(), want_again.counts)


def _scene(pose, n=1):
    """n scenes of a target, an obstacle object and a support (placeholders) at `pose`; the target is object 0."""
    from omg_planner_amd import scenes as sc
    ball = lambda r: sc.sphere_sdf(r, (8, 8, 8), 0.05)
    return [sc.Scene([sc.SceneObject("target", pose, ball(0.05)), sc.SceneObject("obstacles", pose, ball(0.04)), sc.SceneObject("support", pose, ball(0.03))], 0)
            for _ in range(n)]


def _render(dev, which):
    from omg_planner_amd import ops
    meshes, inst, begin, cams = SC.observed_records(which)
    batch = ops.CameraBatch(meshes, inst, begin, cams, device=dev)
    return (batch,) + tuple(ops.render_depth(batch, FC.H, FC.W))


def _up_in_cameras(batch, up_world):
    """A direction of the world in every camera's frame, from the batch's records as Observation.fit_supports turns it."""
    return np.stack([np.asarray(w, np.float64).reshape(3, 4)[:, :3].T @ np.asarray(up_world, np.float64) for w in batch.h_cameras["world_from_cam"]])


SUPPORT_LAYOUT = ((-0.26, -0.26, -0.07), 0.02, (26, 26, 6))  # in the layout's frame: the slab's top z = 0.01 passes through it


def test_observed_scene_segmented_with_the_fitted_support(dev):
    """Three scenes, each seen by its own camera: Observation.fit_supports gives the mask that camera.explained_mask gives from
    the slab's own rendering, and Observation.segment_obstacles with it leaves the same pool bits and records as the existing
    path.  Then DeviceScenes.plane_obstacles: the pool holds the specification's half-space volume, the record has the limits
    and the region of a table built from a host SdfGrid of the same volume, and a refused argument offers no slot."""
    from omg_planner_amd import camera, ops, planes, scenes as sc
    batch, t, _, _ = _render(dev, (0, 1, 2))
    _, t_known, _, _ = _render(dev, (2,))
    torch.cuda.synchronize()
    known = camera.explained_mask(t, t_known, SC.TOL)
    obs = camera.Observation(batch, t, None, None)
    up_world = (0.0, 0.0, 1.0)
    fit, mask = obs.fit_supports(PC.observed_triples(), SC.TOL, up_world=up_world, cos_min=0.9)
    torch.cuda.synchronize()
    assert (fit.status == planes.REFINED).all() and ((fit.counts.cpu().numpy() >= 0).sum(1) >= 16).all()
    assert torch.equal(mask, known) and mask.sum().item() == 1720 + 1586 + 1586
    # the specification with the prior turned into the cameras' frames
    want = planes.fit_planes(PC.observed_intrinsics(), SC.observed_depth()[0], PC.observed_triples(), SC.TOL, up=_up_in_cameras(batch, up_world),
                             cos_min=0.9)
    assert np.array_equal(PC.bits(fit.h_planes), PC.bits(want.planes)) and np.array_equal(fit.inliers, want.inliers)
    eye = np.eye(4)
    nodes = int(np.prod(FC.DIMS))
    tp, op, sp = [(s, 0) for s in range(3)], [(s, 1) for s in range(3)], [(s, 2) for s in range(3)]
    tables = []
    for m in (mask, known):
        table = ops.DeviceScenes.from_scenes(_scene(eye, 3), device=dev, share_grids=False, reserve_voxels=3 * 4 * nodes + 3 * int(np.prod(SUPPORT_LAYOUT[2])))
        radius, records, comps = obs.segment_obstacles(table, tp, op, [SC.LAYOUT] * 3, SC.BAND, SC.NEAR, SC.REACH, [SC.BOX_C] * 3, 40, free_mask=m)
        torch.cuda.synchronize()
        tables.append((table, records, comps.records.copy(), comps.labels.cpu().numpy()))
    (a, ra, ca, la), (b, rb_, cb, lb) = tables
    assert np.array_equal(ra, rb_) and np.array_equal(ca, cb) and np.array_equal(la, lb)
    assert np.array_equal(a.sync_host(), b.sync_host()) and a.pool_used == b.pool_used
    assert np.array_equal(_bits(a.pool[: a.pool_used]), _bits(b.pool[: b.pool_used]))
    # the supports as obstacles
    table = a
    in_frames = obs.support_planes(table, sp, fit)
    for s in range(3):  # (the objects stand in the world's frame here: the slab's top)
        assert abs(in_frames[s][3] + PC.SLAB_TOP) < 1e-4 and in_frames[s][2] > 1 - 1e-8
    table.plane_obstacles(sp, in_frames, [SUPPORT_LAYOUT] * 3)
    torch.cuda.synchronize()
    assert not table._slots.pending
    volume = (SUPPORT_LAYOUT[0], SUPPORT_LAYOUT[1], "centre", SUPPORT_LAYOUT[2])
    host = table.sync_host()
    for s in range(3):
        grid = sc.SdfGrid(planes.halfspace_volume(volume, in_frames[s]), np.array(SUPPORT_LAYOUT[0]), SUPPORT_LAYOUT[1])
        assert (grid.data > 0).any() and (grid.data < 0).any()
        rec = host[table._index(s, 2)]
        off = int(rec["grid_offset"])
        assert tuple(rec["dim"]) == grid.data.shape and np.array_equal(_bits(table.pool[off: off + grid.data.size]), FC.bits(grid.data).ravel()), s
        ref = ops.DeviceScenes.from_scenes([sc.Scene([sc.SceneObject("x", eye, grid)], 0)], device=dev).sync_host()[0]
        for name in ("lo", "hi", "dim", "delta", "inv_delta", "pose_inv", "rb_c", "rb_h", "rb_r"):
            assert np.array_equal(rec[name], ref[name]), (s, name)
    # refusals come before a slot is offered, and the table still takes a good call
    good = dict(pairs=sp, planes=in_frames, layouts=[SUPPORT_LAYOUT] * 3)
    for what, change in (("pairs need as many", dict(layouts=[SUPPORT_LAYOUT] * 2)), ("pairs need as many", dict(pairs=[], planes=np.zeros((0, 4)), layouts=[])),
                         ("named twice", dict(pairs=[(0, 2), (0, 2), (1, 2)])), ("need as many planes", dict(planes=in_frames[:2])),
                         ("need as many planes", dict(planes=np.where(np.arange(12).reshape(3, 4) == 5, np.nan, in_frames))),
                         ("dims >= 1", dict(layouts=[SUPPORT_LAYOUT, SUPPORT_LAYOUT, (SUPPORT_LAYOUT[0], 0.02, (26, 0, 6))])),
                         ("delta must be positive", dict(layouts=[SUPPORT_LAYOUT, SUPPORT_LAYOUT, (SUPPORT_LAYOUT[0], -0.02, (26, 26, 6))]))):
        with pytest.raises(Exception, match=what):
            table.plane_obstacles(**{**good, **change})
        assert not table._slots.pending, what
    with pytest.raises(IndexError):
        table.plane_obstacles(**{**good, "pairs": [(0, 2), (1, 2), (3, 2)]})
    assert not table._slots.pending
    with pytest.raises(ValueError, match="no fitted plane"):
        obs.support_planes(table, sp, ops.PlaneFit(h_planes=np.zeros((3, 4))))
    table.plane_obstacles(**good)
    torch.cuda.synchronize()
    assert not table._slots.pending


def test_plan_on_unknown_support_against_plan_observed_with_the_known_support(dev):
    """Two tabletop scenes whose target, obstacles AND support exist only in the depth image of the scene's camera:
    plan_on_unknown_support gives the plans, grasp sets and records of plan_observed run with explained_mask of the slab's own
    rendering and the specification's half-space volume in the support object."""
    from omg_planner_amd import camera, ops, pipeline, planes, robot as rb, scenes as sc
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
            scene.objects.append(sc.SceneObject("support", poses[k], sc.sphere_sdf(0.03, (8, 8, 8), 0.05)))
            assert scene.target_idx == 0
            out.append(scene)
        return out

    scenes = make()
    obstacle_idx, support_idx = [len(s.objects) - 2 for s in scenes], [len(s.objects) - 1 for s in scenes]
    cfw, intr = FC.scene_cameras()
    meshes = SC.observed_meshes()
    cam_k = [cfw[k] @ np.linalg.inv(poses[k]) for k in range(2)]  # scene k is seen by camera k, moved with the pose
    recs = [camera.instance_records(meshes, [0, 1, 2], [poses[k]] * 3, [1, 1, 1], cam_k[k]) for k in range(2)]
    known = [camera.instance_records(meshes, [2], [poses[k]], [1], cam_k[k]) for k in range(2)]
    cams = np.stack([camera.camera_rows(intr, cam_k[k]) for k in range(2)])
    batch = ops.CameraBatch(meshes, np.concatenate(recs), np.array([0, 3, 6], np.int64), cams, device=dev)
    t = ops.render_depth(batch, FC.H, FC.W)[0]
    t_known = ops.render_depth(ops.CameraBatch(meshes, np.concatenate(known), np.array([0, 1, 2], np.int64), cams, device=dev), FC.H, FC.W)[0]
    torch.cuda.synchronize()
    explained = camera.explained_mask(t, t_known, SC.TOL)
    obs = camera.Observation(batch, t, None, None)
    start = np.tile(np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785, 0.04, 0.04]), (2, 1))
    rngs = lambda: [np.random.RandomState(7), np.random.RandomState(8)]
    kw = dict(n_rays=256, n_angles=8, ol_alg="MD", max_grasps=64, cone=np.deg2rad(15.0))
    triples = PC.observed_triples()[:2]
    res, sets, found, records, fit = pipeline.plan_on_unknown_support(
        model, scenes, obs, obstacle_idx, support_idx, [SC.LAYOUT] * 2, [SUPPORT_LAYOUT] * 2, SC.BAND, SC.NEAR, SC.REACH, [SC.BOX_C] * 2, 40, start, cfg,
        triples, SC.TOL, up_world=(0.0, 0.0, 1.0), cos_min=0.9, device=dev, rng=np.random.RandomState(0), grasp_rng=rngs(), **kw)
    torch.cuda.synchronize()
    assert (fit.status == planes.REFINED).all()
    assert torch.equal(ops.plane_mask(obs.intrinsics(), t, fit.planes, SC.TOL), explained)
    # the existing path: the known slab's mask, and the specification's half-space volume in the support object
    ref_scenes = make()
    table = ops.DeviceScenes.from_scenes(ref_scenes, cfg.layer_kwargs(), device=dev, share_grids=False)
    sp = [(k, support_idx[k]) for k in range(2)]
    want_fit = planes.fit_planes(obs.intrinsics(), t.cpu().numpy(), triples, SC.TOL, up=_up_in_cameras(batch, (0.0, 0.0, 1.0)), cos_min=0.9)
    in_frames = obs.support_planes(table, sp, want_fit)
    volume = (SUPPORT_LAYOUT[0], SUPPORT_LAYOUT[1], "centre", SUPPORT_LAYOUT[2])
    for k in range(2):
        assert abs(in_frames[k][3] + PC.SLAB_TOP) < 1e-4 and in_frames[k][2] > 1 - 1e-7
        grid = sc.SdfGrid(planes.halfspace_volume(volume, in_frames[k]), np.array(SUPPORT_LAYOUT[0]), SUPPORT_LAYOUT[1])
        ref_scenes[k].objects[support_idx[k]].sdf = grid
        got = scenes[k].objects[support_idx[k]].sdf
        assert np.array_equal(FC.bits(got.data), FC.bits(grid.data)) and np.array_equal(got.origin, grid.origin) and got.delta == grid.delta, k
    ref, ref_sets, ref_found, ref_records = pipeline.plan_observed(model, ref_scenes, obs, obstacle_idx, [SC.LAYOUT] * 2, SC.BAND, SC.NEAR, SC.REACH,
                                                                   [SC.BOX_C] * 2, 40, start, cfg, free_mask=explained, device=dev,
                                                                   rng=np.random.RandomState(0), grasp_rng=rngs(), **kw)
    print("grasps", [len(s) for s in sets], "goals", res.goal_counts.tolist(), "planned", res.planned.tolist())
    assert np.array_equal(records, ref_records)
    assert all(len(s) > 0 for s in sets) and all(np.array_equal(a, b) for a, b in zip(sets, ref_sets))
    assert np.array_equal(res.planned, ref.planned) and np.array_equal(res.goal_counts, ref.goal_counts)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(found, ref_found))


def test_a_short_seeded_fuzz_run(dev):
    fuzz = _fuzz()
    assert fuzz.main(trials=fuzz.SMOKE_TRIALS, seed=fuzz.SMOKE_SEED) == 0
