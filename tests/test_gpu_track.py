"""Camera tracking on the MI355X (csrc/omg_track.hip): omgx_track_cameras against tracking.py bit for bit
between guard values on every shape, stride and K of tests/track_cases.py, V = 0, 1, 3 and 70, in place, with a dirty and a reused
workspace, on a side stream, on views that stop at different turns of one launch, a short seeded fuzz run, the wrapper's refusals,
and camera.Observation.tracked against the two-step specification chain.  Every call is followed by a checked synchronise."""
from __future__ import annotations

import numpy as np
import pytest

from tests import track_cases as TC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD, PAD = -7.5, 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), GUARD, dtype=torch.float64, device=dev)
    return buf, buf[:n].view(shape)


def _track(dev, zl, nl, zm, nm, intr, p0, in_place=False, workspace=None, **kw):
    """ops.track_cameras into guarded buffers, a checked synchronise -> (poses, stats) as numpy; the guards must hold."""
    from omg_planner_amd import ops
    V = len(zl)
    b0, poses = _guarded((V, 12), dev)
    b1, stats = _guarded((V, 8), dev)
    d_p0 = _up(p0, dev)
    if in_place and d_p0 is not None:
        poses.copy_(d_p0)
        d_p0 = poses
    got = ops.track_cameras(_up(zl, dev), _up(nl, dev), _up(zm, dev), _up(nm, dev), intr, d_p0, workspace=workspace, out=(poses, stats), **kw)
    torch.cuda.synchronize()
    assert got[0] is poses and got[1] is stats
    assert bool((b0[-PAD:] == GUARD).all()) and bool((b1[-PAD:] == GUARD).all())
    return poses.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("H,W", TC.SHAPES)
def test_device_equals_the_specification_bit_for_bit(dev, H, W):
    """V = 3 with three intrinsics, strides 1, 2, 3, K in {0, 1, 2, 12}, with and without live normals: poses and stats have the
    specification's bits and nothing is written past their last element; V = 1 alike."""
    from omg_planner_amd import tracking
    zl, nl, zm, nm, intr, p0 = TC.synthetic(H, W)
    for stride in TC.STRIDES:
        for K in TC.PASSES:
            for with_normals in (True, False):
                if K in (1, 2) and (stride == 2) == with_normals:
                    continue
                want = TC.synthetic_spec(H, W, stride, K, with_normals)
                got = _track(dev, zl, nl if with_normals else None, zm, nm, intr, p0, **dict(TC.DEFAULT, stride=stride, max_passes=K))
                assert TC.same(got, want), (H, W, stride, K, with_normals)
    one = TC.synthetic(H, W, 1)
    assert TC.same(_track(dev, *one, **TC.DEFAULT), tracking.track_cameras(*one, **TC.DEFAULT)), (H, W)


def test_no_views_in_place_workspaces_and_a_side_stream(dev):
    from omg_planner_amd import ops
    poses, stats = ops.track_cameras(torch.empty((0, 5, 7), dtype=torch.float64, device=dev), None, torch.empty((0, 5, 7), dtype=torch.float64, device=dev),
                                     torch.empty((0, 5, 7, 3), dtype=torch.float64, device=dev), np.zeros((0, 4)))
    torch.cuda.synchronize()
    assert poses.shape == (0, 12) and stats.shape == (0, 8)
    H, W = 48, 64
    args, want = TC.synthetic(H, W), TC.synthetic_spec(H, W, 1, 12, True)
    assert TC.same(_track(dev, *args, in_place=True, **TC.DEFAULT), want)                       # poses_out in place of poses0
    need = ops.track_workspace_bytes(3, H, W, 1)
    ws = torch.full((need // 8,), float("nan"), dtype=torch.float64, device=dev).view(torch.uint8)
    assert TC.same(_track(dev, *args, workspace=ws, **TC.DEFAULT), want)                         # a workspace full of NaN
    other = TC.synthetic(H, W, 3, seed=2)
    assert TC.same(_track(dev, *other, workspace=ws, **dict(TC.DEFAULT, max_passes=3)),        # used a second time, by other views
                   TC.synthetic_spec(H, W, 1, 3, True, 3, 2))
    assert TC.same(_track(dev, *args, workspace=ws, **TC.DEFAULT), want)
    # a side stream: inputs made on it, two calls and a copy back to back, no host sync in between
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        d = [_up(a, dev) for a in args[:4]]
        p1, s1 = ops.track_cameras(*d, args[4], _up(args[5], dev), **TC.DEFAULT)
        p2, s2 = ops.track_cameras(*d, args[4], p1, **dict(TC.DEFAULT, max_passes=2))           # starts where the first call ended
        both = torch.cat([p1, s1, p2, s2], 1)
    side.synchronize()
    torch.cuda.synchronize()
    from omg_planner_amd import tracking
    both = both.cpu().numpy()
    assert TC.same((both[:, :12], both[:, 12:20]), want)
    assert TC.same((both[:, 20:32], both[:, 32:]), tracking.track_cameras(*args[:5], want[0], **dict(TC.DEFAULT, max_passes=2)))


@pytest.mark.parametrize("i", range(len(TC.REC_SEEDS)))
def test_recovery_has_the_specifications_bits(dev, i):
    """The recovery scene at 120 x 160, K = 30: the same bits, and therefore the same errors, as tests/test_track_cpu.py asserts."""
    from omg_planner_amd import tracking
    R = TC.recovery()
    s = R["starts"][i]
    for with_normals, stride in TC.REC_VARIANTS:
        want = TC.recovery_spec(i, with_normals, stride)
        got = _track(dev, s["zl"], s["nl"] if with_normals else None, R["zm"], R["nm"], R["k"], None, **dict(TC.REC_ARGS, stride=stride))
        assert TC.same(got, want), (i, with_normals, stride)
        e = TC.camera_error(tracking.compose(got[0][0], R["cfw"]), s["truth"])
        assert e[0] < 0.5 * TC.REC_DELTA and e[1] < 0.5, (i, with_normals, stride, e)


def test_views_that_stop_at_different_turns_of_one_launch(dev):
    """Every pixel invalid (stops at the first step), at the optimum (one trial), far away (works on), a NaN pose: each view
    equals the same view launched alone and the specification."""
    args, want = TC.turns()
    got = _track(dev, *args, **TC.TURNS)
    assert TC.same(got, want)
    assert len({int(x) for x in want[1][:, 5]}) >= 3
    for v in range(4):
        alone = _track(dev, *(a[v: v + 1] for a in args), **TC.TURNS)
        assert TC.same(alone, (want[0][v: v + 1], want[1][v: v + 1])), v


def test_seventy_views_in_one_launch(dev):
    from omg_planner_amd import tracking
    base = TC.synthetic(17, 33)
    rng = np.random.default_rng(70)
    pick = rng.integers(0, 3, 70)
    zl, nl, zm, nm, intr = (np.ascontiguousarray(a[pick]) for a in base[:5])
    p0 = np.stack([TC.rows(TC.rigid(rng.normal(size=3), np.deg2rad(rng.uniform(0.0, 2.0)), rng.uniform(-0.006, 0.006, 3))) for _ in range(70)])
    args = (zl, nl, zm, nm, intr, p0)
    kw = dict(TC.DEFAULT, max_passes=8)
    got = _track(dev, *args, **kw)
    assert TC.same(got, tracking.track_cameras(*args, **kw))
    assert len({int(x) for x in got[1][:, 5]}) >= 3                                             # they stop at different turns
    for v in range(0, 70, 7):
        assert TC.same(_track(dev, *(a[v: v + 1] for a in args), **kw), (got[0][v: v + 1], got[1][v: v + 1])), v


def test_seeded_fuzz(dev):
    """20 draws: H, W <= 70, V <= 5, random stride, gates, K and poses, NaN and infinities sprinkled in."""
    from omg_planner_amd import tracking
    rng = np.random.default_rng(2026)
    status = set()
    for draw in range(20):
        H, W, V = int(rng.integers(1, 71)), int(rng.integers(1, 71)), int(rng.integers(1, 6))
        zl, nl, zm, nm, intr, p0 = TC.synthetic(H, W, V, seed=100 + draw, dirty=True)
        kw = dict(stride=int(rng.integers(1, 5)), dist_max=float(rng.choice([0.005, 0.02, 0.05, 1.0])), cos_min=float(rng.choice([-1.0, 0.5, 0.7, 0.95])),
                  lambda0=float(2.0 ** rng.integers(-14, 4)), step_tol=float(rng.choice([1e-9, 1e-6, 1e-3])), max_passes=int(rng.integers(0, 13)))
        with_normals = bool(rng.random() < 0.6)
        args = (zl, nl if with_normals else None, zm, nm, intr, p0)
        want = tracking.track_cameras(*args, **kw)
        assert TC.same(_track(dev, *args, **kw), want), (draw, H, W, V, kw)
        status |= {int(x) for x in want[1][:, 7]}
    assert len(status) >= 3, status


def test_the_wrappers_refusals_on_the_device(dev):
    from omg_planner_amd import _lib, ops
    E = _lib.OmgHipError
    zl, nl, zm, nm, intr, p0 = TC.synthetic(16, 16)
    d = dict(zl=_up(zl, dev), nl=_up(nl, dev), zm=_up(zm, dev), nm=_up(nm, dev), p0=_up(p0, dev))
    call = lambda intr=intr, **kw: ops.track_cameras(kw.pop("zl", d["zl"]), kw.pop("nl", d["nl"]), kw.pop("zm", d["zm"]), kw.pop("nm", d["nm"]), intr,
                                                     kw.pop("p0", d["p0"]), **kw)
    call(max_passes=1)
    torch.cuda.synchronize()
    for kw, match in ((dict(zl=d["zl"].float()), "float64"), (dict(nm=d["nm"].cpu()), "device tensor"), (dict(zm=d["zm"].transpose(1, 2)), "contiguous"),
                      (dict(p0=d["p0"].float()), "float64"), (dict(nl=d["nl"].cpu()), "device tensor"),
                      (dict(workspace=torch.empty(100, dtype=torch.uint8, device=dev)), "workspace has"),
                      (dict(workspace=torch.empty(4096, dtype=torch.float64, device=dev)), "uint8"),
                      (dict(out=(torch.empty((3, 12), dtype=torch.float64, device=dev), torch.empty((3, 9), dtype=torch.float64, device=dev))), r"out\[1\]")):
        with pytest.raises(E, match=match):
            call(**kw)
    # an output that shares bytes with an input is the C ABI's to refuse; poses_out == poses0 is allowed
    shared = torch.empty((3, 20), dtype=torch.float64, device=dev)
    with pytest.raises(E, match="invalid argument"):
        call(p0=shared.view(-1)[:36].view(3, 12), out=(shared.view(-1)[12:48].view(3, 12), torch.empty((3, 8), dtype=torch.float64, device=dev)))
    with pytest.raises(E, match="invalid argument"):
        call(out=(torch.empty((3, 12), dtype=torch.float64, device=dev), d["zl"].view(-1)[:24].view(3, 8)))
    call(out=(d["p0"], torch.empty((3, 8), dtype=torch.float64, device=dev)), max_passes=1)
    torch.cuda.synchronize()


def test_observation_tracked_equals_the_two_step_specification(dev):
    """Frames of the recovery scene rendered at the true cameras and announced with cameras 20 mm / 3 degrees off, tracked against
    the table: the corrected cameras, the accepted mask, poses and stats equal the chain volume_camera.render_volumes ->
    tracking.track_cameras -> accepted_mask -> compose on the observation's own images, the view that looks away from the scene
    is rejected and keeps its camera, and the accepted views end within half a voxel and half a degree of the truth."""
    from omg_planner_amd import _lib, camera, ops, scenes as sc, tracking, volume_camera as vc
    A = TC.announced()
    objects, begin, pool = TC.scene_table(3)
    table = ops.DeviceScenes(sc.SceneBatch(objects, begin, pool), device=dev)
    intr = np.array([TC.REC_INTRINSICS] * 3)
    obs = camera.observe_frames(A["frames"], 1.0, A["announced"], intr, TC.TAU, TC.NORMAL_COS, device=dev)
    new, res = obs.tracked(table, **TC.REC_ARGS)  # (min_inliers = 100, min_share = 0.5)
    torch.cuda.synchronize()
    # the specification chain on the observation's images
    zl, nl = obs.t.cpu().numpy(), obs.normals.cpu().numpy()
    rows = np.stack([camera.camera_rows(intr[s], A["announced"][s]) for s in range(3)])
    cfw0 = np.stack([np.linalg.inv(np.vstack([r[4:].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])) for r in rows])
    model_rows = np.stack([camera.camera_rows(intr[s], cfw0[s]) for s in range(3)])     # the model is rendered at the cameras compose starts from
    zm, _, nm, _ = vc.render_volumes(objects, begin, pool, model_rows, TC.REC_H, TC.REC_W)
    poses, stats = tracking.track_cameras(zl, nl, zm, nm, intr, None, **TC.REC_ARGS)
    mask = tracking.accepted_mask(stats, 100, 0.5, tracking.valid_pixels(zl, nl, 1))
    want = np.stack([tracking.compose(poses[s], cfw0[s]) if mask[s] else cfw0[s] for s in range(3)])
    assert mask.tolist() == [True, True, False] and res.accepted.tolist() == mask.tolist()
    assert TC.same((res.poses, res.stats), (poses, stats))
    assert np.array_equal(TC.bits(res.cam_from_world), TC.bits(want)) and np.array_equal(TC.bits(res.cam_from_world[2]), TC.bits(cfw0[2]))
    assert getattr(new.batch, "frames_only", False) and new.t is obs.t and new.normals is obs.normals
    assert np.array_equal(TC.bits(new.batch.h_cameras["world_from_cam"]), TC.bits(np.stack([camera.camera_rows(intr[s], want[s])[4:] for s in range(3)])))
    for s in range(2):
        before, after = TC.camera_error(A["announced"][s], A["truth"][s]), TC.camera_error(res.cam_from_world[s], A["truth"][s])
        print(f"view {s}: {before[0] * 1e3:.2f} mm / {before[1]:.3f} deg -> {after[0] * 1e3:.3f} mm / {after[1]:.4f} deg")
        assert after[0] < 0.5 * TC.REC_DELTA and after[1] < 0.5
    # two rounds: the model is rendered again at the corrected cameras; a rendered observation is refused
    again, res2 = obs.tracked(table, rounds=2, **TC.REC_ARGS)
    torch.cuda.synchronize()
    assert res2.accepted.tolist() == [True, True, False] and np.array_equal(TC.bits(res2.cam_from_world[2]), TC.bits(cfw0[2]))
    for s in range(2):
        after = TC.camera_error(res2.cam_from_world[s], A["truth"][s])
        assert after[0] < 0.5 * TC.REC_DELTA and after[1] < 0.5
    rendered = camera.observe_volumes(table, A["announced"], intr, TC.REC_H, TC.REC_W)
    with pytest.raises(_lib.OmgHipError, match="sensor frames"):
        rendered.tracked(table)


def _sphere_rms_of_integrated(dev, obs):
    """The three images of `obs` integrated as three views into ONE volume of a scene table (Observation.view_rows for the views,
    DeviceScenes.integrate_obstacles, unknown nodes counted as free), the volume read back from the pool -> tsdf_cases.sphere_rms."""
    from omg_planner_amd import ops, scenes as sc
    from tests import fusion_cases as FC, tsdf_cases as TS
    n = int(np.prod(FC.DIMS))
    slab = sc.box_sdf((0.6, 0.4, 0.02), (24, 16, 8), 1.5 / 24)
    made = [sc.Scene([sc.SceneObject("obstacles", np.eye(4), sc.sphere_sdf(0.05, (8, 8, 8), 0.05)),
                      sc.SceneObject("table", sc._yaw_pose(0.5, 0.0, -0.3, 0.0), slab)], 1) for _ in range(3)]
    three = ops.DeviceScenes.from_scenes(made, device=dev, share_grids=False, reserve_voxels=n)
    views = obs.view_rows(three, [(s, 0) for s in range(3)])
    three.integrate_obstacles([(0, 0)], None, obs.t, views, [(0, 3)], [(FC.ORIGIN, FC.DELTA, FC.DIMS)], TS.TRUNC, FC.NEAR, reach=0.1, unknown_occupied=False)
    torch.cuda.synchronize()
    off = int(three.sync_host()[0]["grid_offset"])
    return TS.sphere_rms(three.pool[off: off + n].cpu().numpy().reshape(FC.DIMS))


def test_tracked_cameras_sharpen_the_fused_sphere(dev):
    """Three frames of the sphere scene integrated into one TSDF volume with the true cameras, with cameras 20 mm / 3 degrees off,
    and with those cameras tracked against the scene's volumes: the rms distance of the extracted surface from the analytic sphere
    (tsdf_cases.sphere_rms) is smaller with the tracked cameras than with the wrong ones.  All three are printed."""
    from omg_planner_amd import camera, ops, scenes as sc
    E = TC.effect()
    k = np.array([E["intrinsics"]] * 3)
    table = ops.DeviceScenes(sc.SceneBatch(*E["table"]), device=dev)
    observe = lambda cams: camera.observe_frames(E["frames"], 1.0, cams, k, TC.TAU, TC.NORMAL_COS, device=dev)
    true, wrong = observe(E["truth"]), observe(E["announced"])
    tracked, res = wrong.tracked(table, **TC.REC_ARGS)
    torch.cuda.synchronize()
    rms = {name: _sphere_rms_of_integrated(dev, obs) for name, obs in (("true", true), ("wrong", wrong), ("tracked", tracked))}
    for s in range(3):
        before, after = TC.camera_error(E["announced"][s], E["truth"][s]), TC.camera_error(res.cam_from_world[s], E["truth"][s])
        print(f"view {s}: {before[0] * 1e3:.2f} mm / {before[1]:.3f} deg -> {after[0] * 1e3:.3f} mm / {after[1]:.4f} deg, accepted {bool(res.accepted[s])}, "
              f"trials {int(res.stats[s, 5])}, inliers {int(res.stats[s, 3])}")
    print("sphere rms (m, vertices): " + ", ".join(f"{name} {v[0]:.5f} ({v[1]})" for name, v in rms.items()))
    assert rms["tracked"][0] < rms["wrong"][0]
