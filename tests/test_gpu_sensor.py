"""Depth conditioning on the MI355X (csrc/omg_sensor.hip): omgx_depth_condition / omgx_depth_normals against
sensor.py bit for bit between guard values on every shape, radius and input kind of tests/sensor_cases.py, V = 0, a short seeded
fuzz run, both ops back to back on one stream, and camera.Observation.conditioned / camera.observe_frames on the simulated frames of
the sphere scene (into TSDF volumes, into clouds) and of a plate in front of a wall (into segmentation).  Every launch is followed by a checked synchronise."""
from __future__ import annotations

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import sensor_cases as SC
from tests import tsdf_cases as TC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD_F, GUARD_B, PAD = -7.5, 0xA5, 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _same(t, want):
    got = t.detach().cpu().numpy()
    want = np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _guarded(shape, dtype, dev):
    """(a flat buffer filled with the guard value, its first prod(shape) elements as a tensor of `shape`)"""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), GUARD_B if dtype == torch.uint8 else GUARD_F, dtype=dtype, device=dev)
    return buf, buf[:n].view(shape)


def _guards_hold(*bufs):
    return all(bool((b[-PAD:] == (GUARD_B if b.dtype == torch.uint8 else GUARD_F)).all()) for b in bufs)


def _run(dev, frames, scale, z_min, z_max, tau, min_support, R, table, range_scale, intrinsics, cos_min):
    """Both ops into guarded buffers -> ((depth, flags, normals, depth2, flags2, cosine), guards hold)."""
    from omg_planner_amd import ops
    f = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    shape = tuple(f.shape)
    b0, depth = _guarded(shape, torch.float64, dev)
    b1, flags = _guarded(shape, torch.uint8, dev)
    b2, normals = _guarded(shape + (3,), torch.float64, dev)
    b3, depth2 = _guarded(shape, torch.float64, dev)
    b4, flags2 = _guarded(shape, torch.uint8, dev)
    b5, cosine = _guarded(shape, torch.float64, dev)
    ops.condition_depth(f, scale, z_min, z_max, tau, min_support, R, table=table, range_scale=range_scale, out=(depth, flags))
    ops.depth_normals(depth, intrinsics, tau, cos_min, flags=flags, out=(normals, depth2, flags2, cosine))
    torch.cuda.synchronize()
    return (depth, flags, normals, depth2, flags2, cosine), _guards_hold(b0, b1, b2, b3, b4, b5)


@pytest.mark.parametrize("kind", SC.KINDS)
def test_device_equals_the_specification_bit_for_bit(dev, kind):
    """1 x 1, one tile, partial tiles both ways and several tiles; R = 0, 1, 3, 7; V = 3 with three intrinsics; a table that is not
    symmetric: every output array has the specification's bytes and nothing is written past its last element."""
    for H, W in SC.SHAPES:
        for R in SC.RADII:
            c = SC.bit_case(H, W, R, kind)
            got, guards = _run(dev, c["frames"], SC.SCALE, SC.Z_MIN, SC.Z_MAX, SC.TAU, SC.MIN_SUPPORT, R, c["table"], SC.RANGE_SCALE, SC.INTRINSICS,
                               SC.COS_MIN)
            for g, name in zip(got, ("depth", "flags", "normals", "depth2", "flags2", "cosine")):
                assert _same(g, c[name]), (H, W, R, kind, name)
            assert guards, (H, W, R, kind)


def test_no_views_is_a_no_op_and_flags_may_be_updated_in_place(dev):
    from omg_planner_amd import ops
    for dtype in (torch.uint16, torch.float64):
        depth, flags = ops.condition_depth(torch.empty((0, 5, 7), dtype=dtype, device=dev), SC.SCALE, SC.Z_MIN, SC.Z_MAX, SC.TAU)
        normals, depth2, flags2, cosine = ops.depth_normals(depth, np.zeros((0, 4)), SC.TAU, want_cosine=True)
        torch.cuda.synchronize()
        assert depth.shape == (0, 5, 7) and flags.shape == (0, 5, 7) and normals.shape == (0, 5, 7, 3) and cosine.shape == (0, 5, 7)
    c = SC.bit_case(17, 33, 3, "uint16")
    depth, flags = (torch.from_numpy(c[k]).to(dev) for k in ("depth", "flags"))
    normals, depth2, flags2, cosine = ops.depth_normals(depth, SC.INTRINSICS, SC.TAU, SC.COS_MIN, flags=flags,
                                                        out=(torch.empty((3, 17, 33, 3), dtype=torch.float64, device=dev), torch.empty_like(depth), flags, None))
    torch.cuda.synchronize()
    assert flags2 is flags and cosine is None and _same(flags, c["flags2"]) and _same(normals, c["normals"]) and _same(depth2, c["depth2"])
    from omg_planner_amd import _lib
    with pytest.raises(_lib.OmgHipError, match="invalid argument"):  # depth_out may not be the input
        ops.depth_normals(depth, SC.INTRINSICS, SC.TAU, SC.COS_MIN, out=(normals, depth, flags, None))
    with pytest.raises(_lib.OmgHipError, match="invalid argument"):
        ops.condition_depth(depth, 1.0, SC.Z_MIN, SC.Z_MAX, SC.TAU, out=(depth, flags))
    with pytest.raises(_lib.OmgHipError, match=r"radius must lie in \[0, 7\]"):
        ops.condition_depth(depth, 1.0, SC.Z_MIN, SC.Z_MAX, SC.TAU, radius=8, table=np.ones(17 * 17))


def test_a_short_seeded_fuzz_run(dev):
    """Random H, W <= 70, V <= 5, R, tables, thresholds and both input kinds; NaN and the infinities in the float64 frames."""
    rng = np.random.default_rng(SC.FUZZ_SEED)
    kinds, radii = set(), set()
    for _ in range(SC.FUZZ_TRIALS):
        c = SC.draw(rng)
        got, guards = _run(dev, c["frames"], c["scale"], c["z_min"], c["z_max"], c["tau"], c["min_support"], c["radius"], c["table"], c["range_scale"],
                           c["intrinsics"], c["cos_min"])
        for g, w in zip(got, SC.specification(c)):
            assert _same(g, w), (c["frames"].shape, c["frames"].dtype, c["radius"])
        assert guards
        kinds.add(str(c["frames"].dtype)), radii.add(c["radius"])
    assert kinds == {"uint16", "float64"} and len(radii) >= 4 and 0 in radii and 7 in radii


def test_both_ops_on_one_stream_without_a_host_sync(dev):
    """The two launches enqueued on a side stream one after the other, nothing waited for in between: the second reads what the
    first wrote, and the result is the two-step specification."""
    from omg_planner_amd import ops
    c = SC.bit_case(40, 50, 3, "uint16")
    frames = torch.from_numpy(c["frames"]).to(dev)
    d_table = c["table"]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        depth, flags = ops.condition_depth(frames, SC.SCALE, SC.Z_MIN, SC.Z_MAX, SC.TAU, SC.MIN_SUPPORT, 3, table=d_table, range_scale=SC.RANGE_SCALE)
        normals, depth2, flags2, cosine = ops.depth_normals(depth, SC.INTRINSICS, SC.TAU, SC.COS_MIN, flags=flags, want_cosine=True)
    side.synchronize()
    for g, name in zip((depth, flags, normals, depth2, flags2, cosine), ("depth", "flags", "normals", "depth2", "flags2", "cosine")):
        assert _same(g, c[name]), name


# ---------------------------------------------------------------------------------------------------------------------
# Observation.conditioned and observe_frames on the simulated frames of the sphere scene
# ---------------------------------------------------------------------------------------------------------------------
def _frames_observation(dev, **over):
    from omg_planner_amd import camera
    e = SC.effect()
    cfw, intr = FC.scene_cameras()
    args = dict(frames=torch.from_numpy(e["frame"]).to(dev), scale=SC.EFFECT_SCALE, cam_from_world=cfw, intrinsics=intr, cos_min=SC.EFFECT_COS_MIN,
                table=e["table"], **SC.EFFECT)
    args.update(over)
    return camera.observe_frames(**args), e


def test_observe_frames_equals_the_specification(dev):
    from omg_planner_amd import sensor
    obs, e = _frames_observation(dev)
    torch.cuda.synchronize()
    assert _same(obs.t, e["depth2"]) and _same(obs.flags, e["flags2"]) and _same(obs.normals, e["normals"])
    assert bool((obs.inst == -1).all()) and bool((obs.face == -1).all()) and obs.batch.num_instances == 0 and obs.batch.num_scenes == 3
    assert (e["flags2"] == sensor.KEPT).sum() > 4000
    # a host array goes in as well, and a float64 frame of metres
    metres = e["frame"].astype(np.float64) * SC.EFFECT_SCALE
    again, _ = _frames_observation(dev, frames=metres, scale=1.0)
    torch.cuda.synchronize()
    assert _same(again.t, e["depth2"]) and _same(again.normals, e["normals"])


def _table(dev, scenes_n, reserve):
    from omg_planner_amd import ops, scenes as sc
    slab = sc.box_sdf((0.6, 0.4, 0.02), (24, 16, 8), 1.5 / 24)
    made = [sc.Scene([sc.SceneObject("obstacles", np.eye(4), sc.sphere_sdf(0.05, (8, 8, 8), 0.05)),
                      sc.SceneObject("table", sc._yaw_pose(0.5, 0.0, -0.3, 0.0), slab)], 1) for _ in range(scenes_n)]
    return ops.DeviceScenes.from_scenes(made, device=dev, share_grids=False, reserve_voxels=reserve)


def _sphere_rms_of_integrated(dev, obs, unknown_occupied):
    """The three images of `obs` integrated as three views into ONE volume of a scene table (Observation.view_rows for the views,
    DeviceScenes.integrate_obstacles), the surface extracted on the device, the volume read back from the pool ->
    tsdf_cases.sphere_rms of it."""
    n = int(np.prod(FC.DIMS))
    three = _table(dev, 3, n)
    views = obs.view_rows(three, [(s, 0) for s in range(3)])  # (the object stands at the same pose in every scene)
    radius, held = three.integrate_obstacles([(0, 0)], None, obs.t, views, [(0, 3)], [(FC.ORIGIN, FC.DELTA, FC.DIMS)], TC.TRUNC, FC.NEAR, reach=0.1,
                                             unknown_occupied=unknown_occupied)
    torch.cuda.synchronize()
    assert radius == FC.RADIUS and len(held.rec) == 1
    verts, faces, vrows, frows, _ = three.object_surfaces([(0, 0)])  # the surface comes out on the device too
    torch.cuda.synchronize()
    assert frows[0, 1] > 500
    off = int(three.sync_host()[0]["grid_offset"])
    return TC.sphere_rms(three.pool[off: off + n].cpu().numpy().reshape(FC.DIMS))


def test_integrating_conditioned_frames_gives_no_worse_a_sphere(dev):
    """The simulated frames integrated as they are (raw * scale, 0 where there is no return, flying pixels and all) and after
    observe_frames, three views into one volume, unknown nodes counted as free: the rms distance of the extracted surface from the
    analytic sphere (tsdf_cases.sphere_rms) is no larger with conditioning.  The specification on the CPU gives 2.68 mm with and
    7.03 mm without (the noise-free images: 4.51 mm).  With unknown nodes counted as occupied the order turns round, 5.43 mm with and
    2.81 mm without: a dropped pixel says nothing, so the nodes along its ray stay unknown, while a raw flying pixel still carves
    the free space in front of it; that figure is printed, not asserted."""
    from omg_planner_amd import camera
    obs, e = _frames_observation(dev)
    raw = camera.Observation(obs.batch, torch.from_numpy(e["frame"].astype(np.float64) * SC.EFFECT_SCALE).to(dev), obs.inst, obs.face)
    (with_c, n_with), (without, n_without) = _sphere_rms_of_integrated(dev, obs, False), _sphere_rms_of_integrated(dev, raw, False)
    print("sphere rms, unknown free: conditioned", with_c, n_with, "raw", without, n_without)
    print("sphere rms, unknown occupied: conditioned", _sphere_rms_of_integrated(dev, obs, True), "raw", _sphere_rms_of_integrated(dev, raw, True))
    assert n_with > 200 and n_without > 200 and with_c <= without


def test_frames_observation_serves_the_depth_only_calls_and_refuses_the_rest(dev):
    """fit_supports and support_planes find the slab in the conditioned frames; robot_view renders on the batch's cameras; what needs
    an instance image raises."""
    from omg_planner_amd import _lib, ops, planes
    obs, e = _frames_observation(dev)
    triples = planes.draw_triples(FC.H, FC.W, 128, np.random.default_rng(3), views=3)
    fit, mask = obs.fit_supports(triples, 0.01, up_world=(0.0, 0.0, 1.0), cos_min=0.9)
    torch.cuda.synchronize()
    slab = np.isfinite(e["t"]) & ~FC.scene_sphere_pixels() & (e["depth2"] > 0)
    assert mask.shape == obs.t.shape and (mask.cpu().numpy()[slab]).mean() > 0.9  # the slab's kept pixels lie on the fitted plane
    table = _table(dev, 3, 0)
    moved = obs.support_planes(table, [(s, 0) for s in range(3)], fit)
    assert moved.shape == (3, 4) and (np.abs(moved[:, 2]) > 0.99).all()  # the slab's top: a plane of constant z in the world
    view = obs.robot_view(ops.RobotSpheres([(0.0, 0.0, 0.0, 0.05)], [9], device=dev), *_robot(dev), pad=0.01, tol=0.01)
    torch.cuda.synchronize()
    assert view.t_near.shape == obs.t.shape and view.mask.shape == obs.t.shape
    with pytest.raises(_lib.OmgHipError, match="needs an instance image"):
        obs.clouds(-1)
    with pytest.raises(_lib.OmgHipError, match="needs an instance image"):
        obs.integrate_obstacles(_table(dev, 3, 0), [(0, 0)], [(FC.ORIGIN, FC.DELTA, FC.DIMS)], TC.TRUNC, FC.NEAR, reach=0.1)


def test_segmentation_finds_the_plate_on_conditioned_frames_only(dev):
    """sensor_cases' plate 5 cm in front of a wall: through Observation.segment_obstacles the component picked at the plate is the
    CPU construction's record: in the raw frame it is joined to the wall by the flying pixels, from observe_frames it is the
    plate alone."""
    from omg_planner_amd import camera, ops, scenes as sc
    p = SC.plate()
    n = int(np.prod(SC.PLATE_LAYOUT[2]))
    made = [sc.Scene([sc.SceneObject("target", np.eye(4), sc.sphere_sdf(0.05, (8, 8, 8), 0.05)),
                      sc.SceneObject("obstacles", np.eye(4), sc.sphere_sdf(0.05, (8, 8, 8), 0.05))], 0)]
    filt = {k: v for k, v in SC.PLATE.items()}
    obs = camera.observe_frames(torch.from_numpy(p["frame"]).to(dev), 0.001, np.eye(4), SC.PLATE_K, cos_min=SC.PLATE_COS_MIN, table=p["table"], **filt)
    raw = camera.Observation(obs.batch, torch.from_numpy(p["frame"].astype(np.float64) * 0.001).to(dev), obs.inst, obs.face)
    torch.cuda.synchronize()
    assert _same(obs.t, p["depth2"])
    for name, o in (("conditioned", obs), ("raw", raw)):
        table = ops.DeviceScenes.from_scenes(made, device=dev, share_grids=False, reserve_voxels=12 * n)
        radius, records, comps = o.segment_obstacles(table, [(0, 0)], [(0, 1)], [SC.PLATE_LAYOUT], SC.PLATE_BAND, SC.PLATE_NEAR, SC.PLATE_REACH,
                                                     [SC.PLATE_SEED_POINT], SC.PLATE_MIN_NODES)
        torch.cuda.synchronize()
        print(name, records[0].tolist())
        assert np.array_equal(records[0], p["picked"][name]), name
    assert p["picked"]["raw"][0] > 2 * p["picked"]["conditioned"][0]


def _robot(dev):
    """(robot blob, P, joints [3,9]) for Observation.robot_view."""
    from omg_planner_amd import ops, robot as rb
    model = rb.PandaModel(seed=0)
    return ops.robot_blob(model, dev), model.points_per_link, torch.from_numpy(np.tile(rb.HOME_CONFIG, (3, 1))).to(dev)


def test_conditioned_rendering_has_no_point_at_depth_zero(dev):
    """A rendered observation (instances and faces) conditioned with the simulated frames in place of its depth: the dropped
    pixels name no instance, so clouds(-1) has exactly one point per kept pixel that shows an instance, and none at the camera's
    origin, where a depth of 0 would put it."""
    from omg_planner_amd import camera, ops, sensor
    meshes, inst, begin, cams = FC.scene_records((0, 1))
    batch = ops.CameraBatch(meshes, inst, begin, cams, device=dev)
    t, inst_img, face_img = ops.render_depth(batch, FC.H, FC.W)
    e = SC.effect()
    obs = camera.Observation(batch, t, inst_img, face_img).conditioned(SC.EFFECT_TAU, SC.EFFECT_COS_MIN, SC.EFFECT_SCALE, table=e["table"],
                                                                       frames=torch.from_numpy(e["frame"]).to(dev),
                                                                       **{k: v for k, v in SC.EFFECT.items() if k != "tau"})
    clouds = obs.clouds(-1)
    torch.cuda.synchronize()
    assert _same(obs.t, e["depth2"]) and _same(obs.normals, e["normals"]) and _same(obs.flags, e["flags2"])
    kept = e["depth2"] > 0
    h_inst = inst_img.cpu().numpy()
    assert np.array_equal(obs.inst.cpu().numpy(), np.where(kept, h_inst, -1)) and np.array_equal(obs.face.cpu().numpy(), np.where(kept, face_img.cpu().numpy(), -1))
    dropped_hits = (~kept & (h_inst >= 0)).sum()
    assert dropped_hits > 50  # dropout, flying and the pixels beside them: the unconditioned instance image would emit them
    for s in range(3):
        pts = clouds[s].cpu().numpy()
        assert len(pts) == int((kept[s] & (h_inst[s] >= 0)).sum())
        assert np.linalg.norm(pts - np.asarray(FC.EYES[s]), axis=1).min() > SC.EFFECT["z_min"]
    assert (e["flags2"][~kept] != sensor.KEPT).all()
