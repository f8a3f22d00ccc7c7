"""The robot self-filter on the MI355X (csrc/omg_robot_filter.hip): omgx_render_spheres / omgx_clear_robot
against robot_filter.py bit for bit through the C ABI, one launch each, on the edge cases and the seeded batch, between guard
values, with either cull on and off; camera.Observation.robot_view at two joint vectors; the Panda composited in front of a
rendered scene through fuse_obstacles, integrate_obstacles and segment_obstacles with and without robot=; states beyond 2^32
elements; a short seeded fuzz run.  Every launch is followed by a checked synchronise."""
from __future__ import annotations

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import far_pool as FP
from tests import fusion_cases as FC
from tests import robot_filter_cases as RC
from tests import tsdf_cases as TC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD_T, GUARD_N = -77.25, -5  # what the images and the sphere array hold before a launch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _same(got, want) -> bool:
    got, want = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (got, want))
    want = np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.ascontiguousarray(got).tobytes() == want.tobytes()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(dev) if a.dtype.names else torch.from_numpy(a).to(dev)


def abi_render(dev, local, link, poses, cameras, cfg, H, W, pad, t_min, cull):
    """omgx_render_spheres on tensors that hold guard values with one more guarded image and one more guarded view's spheres behind
    them -> (cam_spheres [V,N,4], t_near, sphere) as numpy; asserts that the guards stand."""
    from omg_planner_amd import _lib
    vp = C.c_void_p
    local, link = np.ascontiguousarray(local, np.float64).reshape(-1, 4), np.ascontiguousarray(link, np.int32)
    poses, cameras, cfg = np.ascontiguousarray(poses, np.float64), np.ascontiguousarray(cameras), np.ascontiguousarray(cfg, np.int32)
    N, V = len(link), len(cameras)
    d = [_up(x, dev) for x in (local, link, poses, cameras, cfg)]
    cs = torch.full((V + 1, max(N, 1), 4), GUARD_T, dtype=torch.float64, device=dev)
    t = torch.full((V + 1, H, W), GUARD_T, dtype=torch.float64, device=dev)
    which = torch.full((V + 1, H, W), GUARD_N, dtype=torch.int32, device=dev)
    ptr = lambda x, n=1: vp(x.data_ptr()) if n else None
    rc = _lib.lib().omgx_render_spheres(ptr(d[0], N), vp(local.ctypes.data) if N else None, ptr(d[1], N), vp(link.ctypes.data) if N else None, N,
                                        ptr(d[2]), vp(poses.ctypes.data), len(poses), ptr(d[3]), vp(cameras.ctypes.data), ptr(d[4]),
                                        vp(cfg.ctypes.data), V, H, W, float(pad), float(t_min), int(cull), ptr(cs, N), ptr(t), ptr(which),
                                        vp(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OMGX_OK, (rc, _lib.lib().omgx_last_error())
    torch.cuda.synchronize()
    assert (t[V] == GUARD_T).all() and (which[V] == GUARD_N).all() and (cs.reshape(-1)[V * N * 4:] == GUARD_T).all()
    return cs.reshape(-1)[: V * N * 4].reshape(V, N, 4).cpu().numpy(), t[:V].cpu().numpy(), which[:V].cpu().numpy()


def abi_clear(dev, state, volumes, views, ranges, begin, depth, t_near, cam_spheres, near, tol, cull, check_spheres=True):
    """omgx_clear_robot in place on a copy of `state` -> numpy."""
    from omg_planner_amd import _lib, ops
    vp = C.c_void_p
    rec = ops.surface_records([tuple(v[:4]) + (0,) for v in volumes])
    views, ranges = np.ascontiguousarray(views, np.float64).reshape(-1, 16), np.ascontiguousarray(ranges, np.int32).reshape(-1, 2)
    begin, s = np.ascontiguousarray(begin, np.int64), np.ascontiguousarray(cam_spheres, np.float64)
    d_rec = torch.from_numpy(np.frombuffer(bytes(rec), np.uint8).copy()).to(dev)
    d = [_up(x, dev) for x in (views, ranges, begin, np.ascontiguousarray(depth, np.float64), np.ascontiguousarray(t_near, np.float64), s)]
    out = _up(np.array(state, np.uint8), dev)
    V, N = len(views), s.shape[1]
    ptr = lambda x, n=1: vp(x.data_ptr()) if n else None
    rc = _lib.lib().omgx_clear_robot(ptr(d_rec), C.cast(rec, vp), len(rec), ptr(d[0], V), vp(views.ctypes.data), V, ptr(d[1]), vp(ranges.ctypes.data),
                                     ptr(d[2]), vp(begin.ctypes.data), ptr(d[3], V), ptr(d[4], V), depth.shape[1], depth.shape[2], ptr(d[5], V * N),
                                     vp(s.ctypes.data) if check_spheres and V * N else None, N, float(near), float(tol), int(cull), ptr(out),
                                     out.numel(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OMGX_OK, (rc, _lib.lib().omgx_last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the device against the specification
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", (1, 0))
def test_edge_cases_in_one_launch_each_against_the_written_answers(dev, cull):
    e = RC.render_edge_launch()
    cs, t, which = abi_render(dev, e["local"], e["link"], e["link_poses"], e["cameras"], e["config_of_view"], e["H"], e["W"], 0.0, RC.RENDER_T_MIN, cull)
    from omg_planner_amd import robot_filter as rf
    want_cs = rf.camera_spheres(e["link_poses"], e["local"], e["link"], e["cameras"], e["config_of_view"], 0.0)
    want = rf.render_spheres(want_cs, e["cameras"], e["H"], e["W"], RC.RENDER_T_MIN)
    assert _same(cs, want_cs) and _same(t, want[0]) and _same(which, want[1])
    for k, (what, _, t_k, n) in enumerate(RC.RENDER_CASES):
        assert (t[k, 0, 0], which[k, 0, 0]) == (t_k, -1 if n < 0 else e["first"][k] + n), what
    # no sphere at all: every pixel a miss, nothing read or written for the spheres
    cs, t, which = abi_render(dev, np.zeros((0, 4)), [], e["link_poses"], e["cameras"], e["config_of_view"], 5, 17, 0.0, 0.0, cull)
    assert cs.shape == (len(e["cameras"]), 0, 4) and np.isposinf(t).all() and (which == -1).all()
    b = RC.clear_edge_batch()
    got = abi_clear(dev, b["state"], b["volumes"], RC.clear_views(), b["ranges"], b["begin"], RC.CLEAR_DEPTH, RC.CLEAR_T_NEAR, RC.CLEAR_SPHERES,
                    RC.CLEAR_NEAR, RC.CLEAR_TOL, cull)
    assert _same(got, b["want"])
    at = b["begin"]
    for m, (what, _, _, _, new) in enumerate(RC.CLEAR_CASES):
        assert got[at[m]: at[m] + len(new)].tolist() == new, what


@pytest.mark.parametrize("cull", (1, 0))
@pytest.mark.parametrize("N", RC.BATCH_N)
def test_seeded_batch_in_one_launch_each_against_the_specification(dev, N, cull):
    """40 x 48 images (edge tiles), three views of two configurations, a camera inside a sphere, depth values that are not
    finite, volumes of (2,2,2), (5,9,7) and (33,17,9) between guard bytes; N = 1, 7 and one more than the staging chunk."""
    c = RC.batch(N)
    cs, t, which = abi_render(dev, c["local"], c["link"], c["link_poses"], c["cameras"], c["config_of_view"], RC.BATCH_H, RC.BATCH_W, RC.BATCH_PAD,
                              RC.BATCH_T_MIN, cull)
    assert _same(cs, c["cam_spheres"]) and _same(t, c["t_near"]) and _same(which, c["sphere"])
    got = abi_clear(dev, c["state"], RC.BATCH_VOLUMES, c["views"], RC.BATCH_RANGES, c["begin"], c["depth"], t, cs, RC.BATCH_NEAR, RC.BATCH_TOL, cull,
                    check_spheres=bool(cull))
    assert _same(got, c["want"]) and (got == RC.GUARD).sum() == (c["state"] == RC.GUARD).sum()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the Panda in front of a rendered scene
# ---------------------------------------------------------------------------------------------------------------------
class _Panda:
    """One scene (the sphere and the slab at RC.PANDA_POSE) rendered on the device, and the arm at `joints` composited in as
    min(t_scene, the bare spheres): obs (the composite), clean (the arm-free observation), view (obs.robot_view at the padded
    radius), and the specification's own images from the DEVICE's link poses."""

    def __init__(self, dev, joints):
        from omg_planner_amd import camera, ops, robot as rb, robot_filter as rf
        self.model = rb.PandaModel(seed=0)
        self.blob, self.P = ops.robot_blob(self.model, dev), self.model.points_per_link
        meshes, inst, begin, cams = RC.panda_scene_records()
        self.batch = ops.CameraBatch(meshes, inst, begin, cams, device=dev)
        t_scene, inst_img, face = ops.render_depth(self.batch, FC.H, FC.W)
        self.clean = camera.Observation(self.batch, t_scene, inst_img, face)
        self.spheres = ops.RobotSpheres.from_points(self.model.collision_points, RC.PANDA_RADIUS, dev)
        self.joints = torch.from_numpy(np.ascontiguousarray(joints, np.float64).reshape(1, 9)).to(dev)
        bare = self.clean.robot_view(self.spheres, self.blob, self.P, self.joints, 0.0, RC.PANDA_TOL)
        self.obs = camera.Observation(self.batch, torch.minimum(t_scene, bare.t_near), inst_img, face)
        self.view = self.obs.robot_view(self.spheres, self.blob, self.P, self.joints, RC.PANDA_PAD, RC.PANDA_TOL)
        torch.cuda.synchronize()
        # the specification on the device's poses
        self.poses = ops.forward_kinematics(self.blob, self.P, self.joints, want_joint_info=False)[0].cpu().numpy()
        self.t_scene, self.t_arm = t_scene.cpu().numpy(), self.obs.t.cpu().numpy()
        local, link = RC.panda_spheres(self.model.collision_points)
        self.cs = rf.camera_spheres(self.poses, local, link, self.batch.h_cameras, [0], RC.PANDA_PAD)
        self.t_near, self.which = rf.render_spheres(self.cs, self.batch.h_cameras, FC.H, FC.W)
        self.mask = rf.explained(self.t_arm, self.t_near, RC.PANDA_TOL)
        # the sphere centres in the layout's frame, and the layout's nodes inside a padded sphere
        w = np.einsum("nij,nj->ni", self.poses[0, link][:, :3, :3], local[:, :3]) + self.poses[0, link][:, :3, 3]
        self.centres = w - RC.PANDA_POSE[:3, 3]
        idx = np.floor((self.centres - np.array(RC.PANDA_LAYOUT[0])) / RC.PANDA_LAYOUT[1]).astype(int)
        self.centre_nodes = idx[((idx >= 0) & (idx < 32)).all(1)]

    def spec_states(self, table_views, filtered=True):
        from omg_planner_amd import fusion, robot_filter as rf
        depth = rf.filter_depth(self.t_arm, self.t_near, RC.PANDA_TOL) if filtered else self.t_arm
        st = fusion.carve_views([RC.PANDA_VOLUME], table_views, [(0, 1)], depth, FC.BAND, FC.NEAR)
        return rf.clear_states(st, [RC.PANDA_VOLUME], table_views, [(0, 1)], self.t_arm, FC.NEAR, self.t_near, self.cs, RC.PANDA_TOL) if filtered else st

    def spec_fused(self, table_views, radius):
        """The specification's volume of fuse_obstacles(robot=) for the object at RC.PANDA_POSE: computed once for the tests that read it."""
        from omg_planner_amd import fusion
        if getattr(self, "_fused", None) is None:
            self._fused = (table_views.copy(), radius, fusion.signed_volume(self.spec_states(table_views).reshape(32, 32, 32), 0.01, radius, True))
        assert np.array_equal(self._fused[0], table_views) and self._fused[1] == radius
        return self._fused[2]


@pytest.fixture(scope="module")
def panda(dev):
    from omg_planner_amd import robot as rb
    return _Panda(dev, rb.HOME_CONFIG)


def _table(dev, reserve, objects=1):
    from omg_planner_amd import ops, scenes as sc
    placeholder = sc.sphere_sdf(0.05, (8, 8, 8), 0.05)
    scene = sc.Scene([sc.SceneObject(f"observed{k}", RC.PANDA_POSE, placeholder) for k in range(objects)], 0)
    return ops.DeviceScenes.from_scenes([scene], device=dev, share_grids=False, reserve_voxels=reserve)


def _pool(table, obj, n):
    off = int(table.sync_host()[table._index(0, obj)]["grid_offset"])
    return table.pool[off: off + n]


def test_robot_view_at_two_joint_vectors_equals_the_specification(dev):
    """Two scenes with the same camera and the arm at two configurations: link poses from ops.forward_kinematics; t_near, sphere,
    cam_spheres and mask are the specification's on those poses; filtered() sets t to 0.0 and inst to -1 on the mask only."""
    from omg_planner_amd import camera, ops, robot as rb, robot_filter as rf
    meshes, inst, _, cams = RC.panda_scene_records()
    batch = ops.CameraBatch(meshes, np.concatenate([inst, inst]), [0, 2, 4], np.concatenate([cams, cams]), device=dev)
    t, inst_img, face = ops.render_depth(batch, FC.H, FC.W)
    obs = camera.Observation(batch, t, inst_img, face)
    model = rb.PandaModel(seed=0)
    blob, P = ops.robot_blob(model, dev), model.points_per_link
    spheres = ops.RobotSpheres.from_points(model.collision_points, RC.PANDA_RADIUS, dev)
    joints = torch.from_numpy(np.stack([rb.HOME_CONFIG, RC.PANDA_MOVED])).to(dev)
    view = obs.robot_view(spheres, blob, P, joints, RC.PANDA_PAD, RC.PANDA_TOL)
    no_cull = obs.robot_view(spheres, blob, P, joints, RC.PANDA_PAD, RC.PANDA_TOL, cull=False)
    torch.cuda.synchronize()
    poses = ops.forward_kinematics(blob, P, joints, want_joint_info=False)[0].cpu().numpy()
    local, link = RC.panda_spheres(model.collision_points)
    cs = rf.camera_spheres(poses, local, link, batch.h_cameras, [0, 1], RC.PANDA_PAD)
    t_near, which = rf.render_spheres(cs, batch.h_cameras, FC.H, FC.W)
    mask = rf.explained(t.cpu().numpy(), t_near, RC.PANDA_TOL)
    assert _same(view.cam_spheres, cs) and _same(view.t_near, t_near) and _same(view.sphere, which) and _same(view.mask, mask)
    assert _same(no_cull.t_near, t_near) and _same(no_cull.sphere, which) and _same(view.h_cam_spheres, cs)
    assert 300 < mask[0].sum() < FC.H * FC.W // 2 and 300 < mask[1].sum() and not np.array_equal(mask[0], mask[1])
    out = view.filtered(obs)
    assert _same(out.t, rf.filter_depth(t.cpu().numpy(), t_near, RC.PANDA_TOL)) and _same(out.inst, np.where(mask, -1, inst_img.cpu().numpy()).astype(np.int32))
    assert out.batch is batch and _same(obs.t, t)  # the caller's images are not changed
    second = view.take([1, 1, 0])
    assert _same(second.t_near, t_near[[1, 1, 0]]) and _same(second.cam_spheres, cs[[1, 1, 0]]) and _same(second.mask, mask[[1, 1, 0]])
    # the mask as the skip of the support fit: the arm's pixels take no part
    intr = obs.intrinsics()
    assert not bool((ops.plane_mask(intr, t, np.array([[0.0, 0.0, -1.0, 0.4]] * 2), 0.01, skip=view.mask) & view.mask).any())


def test_fuse_obstacles_with_the_arm_in_the_image(dev, panda):
    """The hand and the fingers hang in front of the scene's sphere.  With robot=: the pool holds the specification's volume (the
    filtered depth carved, clear_states, the transform) bit for bit; the volume read at every sphere centre inside the layout is
    > 0; further than the radius from every exempt node it is the volume fused from the arm-free image.  With robot=None the same
    call leaves the parent's bits (the composite carved as it is), which are < 0 at those centres: the arm is an obstacle."""
    from omg_planner_amd import fusion
    n = 32 ** 3
    pairs, layouts = [(0, 0)], [RC.PANDA_LAYOUT]
    table = _table(dev, 4 * n)
    views = panda.obs.view_rows(table, pairs)
    radius = panda.obs.fuse_obstacles(table, pairs, layouts, FC.BAND, FC.NEAR, reach=0.1, robot=panda.view)
    torch.cuda.synchronize()
    assert radius == FC.RADIUS and not table._slots.pending
    want = panda.spec_fused(views, radius)
    got = _pool(table, 0, n).cpu().numpy().reshape(32, 32, 32)
    assert np.array_equal(got.view(np.uint32), FC.bits(want))
    i = panda.centre_nodes
    assert len(i) >= 20 and (got[i[:, 0], i[:, 1], i[:, 2]] > 0).all()
    clean = fusion.signed_volume(fusion.carve_views([RC.PANDA_VOLUME], views, [(0, 1)], panda.t_scene, FC.BAND, FC.NEAR).reshape(32, 32, 32), 0.01, radius, True)
    exempt = RC.panda_exempt(views, panda.mask, panda.cs)
    away = fusion.squared_distances(exempt.reshape(32, 32, 32), radius) >= radius * radius
    print("exempt nodes", int(exempt.sum()), "nodes further than the radius from all of them", int(away.sum()))
    assert away.sum() > 100 and np.array_equal(got[away].view(np.uint32), clean[away].view(np.uint32))
    assert _same(panda.obs.t, panda.t_arm)  # the caller's images are not changed
    # robot=None: what the parent commit computes
    assert panda.obs.fuse_obstacles(table, pairs, layouts, FC.BAND, FC.NEAR, reach=0.1, robot=None) == radius
    torch.cuda.synchronize()
    raw = fusion.signed_volume(panda.spec_states(views, filtered=False).reshape(32, 32, 32), 0.01, radius, True)
    got = _pool(table, 0, n).cpu().numpy().reshape(32, 32, 32)
    assert np.array_equal(got.view(np.uint32), FC.bits(raw)) and (got[i[:, 0], i[:, 1], i[:, 2]] < 0).any()


def test_fuse_obstacles_with_the_arm_sends_four_small_arrays_to_the_device(dev, panda, monkeypatch):
    """One fuse_obstacles(robot=) call uploads four host arrays, each once: the records at the slots' offsets, state_begin, the views
    and view_range, which the carve, the clear and the transform share.  The pool holds the bits of the test above."""
    from omg_planner_amd import ops
    n, uploads, real_upload = 32 ** 3, [], ops._upload
    table = _table(dev, 4 * n)
    views = panda.obs.view_rows(table, [(0, 0)])
    monkeypatch.setattr(ops, "_upload", lambda a, to: (uploads.append(bytes(a)), real_upload(a, to))[1])
    radius = panda.obs.fuse_obstacles(table, [(0, 0)], [RC.PANDA_LAYOUT], FC.BAND, FC.NEAR, reach=0.1, robot=panda.view)
    torch.cuda.synchronize()
    assert len(uploads) == 4 and len(set(uploads)) == 4 and not table._slots.pending
    assert np.array_equal(_pool(table, 0, n).cpu().numpy().reshape(32, 32, 32).view(np.uint32), FC.bits(panda.spec_fused(views, radius)))


def test_integrate_obstacles_over_two_frames_with_the_arm_moved(dev, panda):
    """Frame 1 with the hand over the sphere, frame 2 with the arm swung out of the layout, into the same TsdfVolumes.  With
    robot=: the pairs and the pool are the specification's (the filtered depths integrated; states, clear_states with the second
    frame's arm, the transform, the blend), and no node the arm occupied in frame 1 is occupied afterwards (unknown_occupied=False:
    a negative value is a SURFACE node).  With robot=None the same two calls leave the parent's bits."""
    from omg_planner_amd import fusion, robot_filter as rf, tsdf
    second = _Panda(dev, RC.PANDA_MOVED)
    n, vol = 32 ** 3, [RC.PANDA_VOLUME]
    pairs, layouts = [(0, 0)], [RC.PANDA_LAYOUT]
    for with_robot in (True, False):
        table = _table(dev, 4 * n)
        views = panda.obs.view_rows(table, pairs)
        held, D, W = None, None, None
        for frame in (panda, second):
            radius, held = frame.obs.integrate_obstacles(table, pairs, layouts, TC.TRUNC, FC.NEAR, reach=0.1, tsdf_volumes=held, unknown_occupied=False,
                                                         robot=frame.view if with_robot else None)
            depth = rf.filter_depth(frame.t_arm, frame.t_near, RC.PANDA_TOL) if with_robot else frame.t_arm
            D, W = tsdf.integrate(vol, views, [(0, 1)], depth, TC.TRUNC, FC.NEAR, tsdf=D, weight=W)
        torch.cuda.synchronize()
        assert held.frames == 2 and _same(held.tsdf, D) and _same(held.weight, W) and not table._slots.pending
        st = tsdf.states(D, W, 1.0)
        if with_robot:
            st = rf.clear_states(st, vol, views, [(0, 1)], second.t_arm, FC.NEAR, second.t_near, second.cs, RC.PANDA_TOL)
        want = tsdf.blend(fusion.distance_transform(st, vol, radius, False)[0], D, W, TC.TRUNC, 1.0)
        got = _pool(table, 0, n).cpu().numpy().reshape(32, 32, 32)
        assert np.array_equal(got.view(np.uint32), TC.bits(want)), with_robot
        p = fusion.node_points(np.array(RC.PANDA_LAYOUT[0]), 0.01, 0.5, (32, 32, 32))
        arm1 = (np.linalg.norm(p[:, None, :] - panda.centres[None], axis=2).min(1) <= RC.PANDA_RADIUS).reshape(32, 32, 32)
        assert arm1.sum() > 500
        if with_robot:
            assert (got[arm1] > 0).all() and (st.reshape(32, 32, 32)[arm1] != fusion.SURFACE).all()
        else:  # the failure the feature removes: the arm of frame 1 is still an obstacle after frame 2
            assert (got[arm1] < 0).any() and (st.reshape(32, 32, 32)[arm1] == fusion.SURFACE).any()


def test_segment_obstacles_with_the_arm_in_the_image(dev, panda):
    """With robot= no component's box meets a padded sphere, and labels, records and both volumes are the specification's on the
    cleared states; with robot=None the arm is labelled (some box meets a sphere) and the bits are the parent's."""
    from omg_planner_amd import fusion, segmentation as sg
    n = 32 ** 3
    seed, min_nodes = (0.0, 0.0, 0.08), 40
    o, delta = np.array(RC.PANDA_LAYOUT[0]), RC.PANDA_LAYOUT[1]
    for with_robot in (True, False):
        table = _table(dev, 12 * n, objects=2)
        views = panda.obs.view_rows(table, [(0, 1)])
        radius, records, comps = panda.obs.segment_obstacles(table, [(0, 0)], [(0, 1)], [RC.PANDA_LAYOUT], FC.BAND, FC.NEAR, 0.1, [seed], min_nodes,
                                                             robot=panda.view if with_robot else None)
        torch.cuda.synchronize()
        st = panda.spec_states(views, filtered=with_robot)
        labels = sg.label_components(st, [RC.PANDA_VOLUME], 1, 6)
        _, want_records = sg.component_records(labels, [RC.PANDA_VOLUME])
        assert np.array_equal(comps.labels.cpu().numpy(), labels) and np.array_equal(comps.records, want_records), with_robot
        rank = sg.pick_component(want_records, sg.point_to_index(RC.PANDA_VOLUME, seed), min_nodes)
        assert np.array_equal(records[0], want_records[rank])
        meets = 0
        for r in comps.records:  # the box of the component's node centres against every padded sphere
            lo, hi = o + (r[2:5] + 0.5) * delta, o + (r[5:8] + 0.5) * delta
            gap = np.linalg.norm(np.maximum(np.maximum(lo - panda.centres, panda.centres - hi), 0.0), axis=1)
            meets += int((gap <= RC.PANDA_RADIUS + RC.PANDA_PAD).any())
        print("robot" if with_robot else "no robot", len(comps.records), "components,", meets, "of them meet a padded sphere")
        assert (meets == 0) if with_robot else (meets > 0)
        # the obstacle's volume: the whole layout with the target taken out, from the same states
        crop = sg.crop_layout(RC.PANDA_VOLUME, want_records[rank], radius + 1)
        picks = [(0,) + tuple(crop[3]) + (rank, 0, 0, 0), (0, 0, 0, 0, rank, 1, 0, 0)]
        outs = [(crop[0], crop[1], "centre", crop[2]), RC.PANDA_VOLUME[:4]]
        cropped = sg.component_states(st, [RC.PANDA_VOLUME], None, labels, [0, len(want_records)], want_records, picks, outs)
        want = fusion.distance_transform(cropped, outs, radius, True)
        assert np.array_equal(_bits(_pool(table, 0, want[0].size)), FC.bits(want[0]).ravel()), with_robot
        assert np.array_equal(_bits(_pool(table, 1, n)), FC.bits(want[1]).ravel()), with_robot


# ---------------------------------------------------------------------------------------------------------------------
# 3. states beyond 2^32 elements
# ---------------------------------------------------------------------------------------------------------------------
def test_clear_robot_far_out_in_a_large_state_array(dev):
    """ops.clear_robot on states whose state_begin lies beyond 2^32 elements (tests/far_pool.py: B2 of a uint8 array of its own,
    4.3 GB) leaves the bytes of the compact run, and the guard pattern in the bands around them and in the alias window, where an
    offset cut to 32 bits would land."""
    from omg_planner_amd import ops
    c = RC.batch(7)
    sizes = [int(np.prod(v[3])) for v in RC.BATCH_VOLUMES]
    offs, used = FP.spread(sizes)
    need = FP.B2 + used + FP.BAND
    free, total = torch.cuda.mem_get_info(dev)
    if free < need + FP.HEADROOM:
        pytest.skip(f"the far state array needs {need + FP.HEADROOM} bytes of free device memory, {free} of {total} are free")
    depth, t_near, cs = (torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("depth", "t_near", "cam_spheres"))
    compact = FP.guard_compact(used, torch.empty(0, dtype=torch.uint8), dev)
    for o, b, s in zip(offs, c["begin"], sizes):
        compact[o: o + s] = torch.from_numpy(c["state"][int(b): int(b) + s]).to(dev)
    start = compact.clone()
    args = (RC.BATCH_VOLUMES, c["views"], RC.BATCH_RANGES, depth, RC.BATCH_NEAR, t_near, cs, RC.BATCH_TOL)
    ops.clear_robot(compact, np.array(offs, np.int64), *args)
    torch.cuda.synchronize()
    for o, b, s in zip(offs, c["begin"], sizes):
        assert _same(compact[o: o + s], c["want"][int(b): int(b) + s])
    view = torch.empty(need, dtype=torch.uint8, device=dev)
    FP.guard(view, FP.B2, used)
    view[FP.B2: FP.B2 + used] = start
    out = ops.clear_robot(view, FP.relocate(np.array(offs, np.int64), FP.B2), *args)
    torch.cuda.synchronize()
    assert out is view and FP.written(view, FP.B2, compact) == {"far": True, "bands": True, "alias": True}
    del view
    torch.cuda.empty_cache()


def test_a_short_seeded_fuzz_run(dev):
    spec = importlib.util.spec_from_file_location("fuzz_robot_filter", Path(__file__).resolve().parent / "fuzz" / "fuzz_robot_filter.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    assert fuzz.main(trials=fuzz.SMOKE_TRIALS, seed=fuzz.SMOKE_SEED) == 0


def partial_tiles_case():
    """Two spheres on link 0 (at the identity: local is the world) before two cameras of 17 x 33 pixels (2 x 3 tiles, partial both
    ways): in view 0 the large one lies over the corner where four tiles meet, in view 1 over the image's last row and last column
    -> dict(local, link, link_poses, rows [2,16], cameras, config_of_view, cam_spheres, t_near, sphere: the specification's)."""
    from omg_planner_amd import camera, robot_filter as rf
    local, link = np.array([(0.0, 0.0, 0.5, 0.08), (-0.07, -0.05, 0.4, 0.03)]), np.zeros(2, np.int64)
    poses, cfg = np.tile(np.eye(4), (1, 10, 1, 1)), np.zeros(2, np.int64)
    rows = np.stack([camera.camera_rows((30.0, 28.0, 16.0, 16.0), np.eye(4)), camera.camera_rows((26.0, 30.0, 31.0, 15.5), np.eye(4))])
    cameras = camera.camera_records(rows)
    cam_spheres = rf.camera_spheres(poses, local, link, cameras, cfg, 0.01)
    t_near, sphere = rf.render_spheres(cam_spheres, cameras, 17, 33, 1e-6)
    hit = sphere >= 0
    assert all(hit[0, r, c] for r in (15, 16) for c in (15, 16)) and hit[1, 16].any() and hit[1, :, 32].any()  # across the tiles' borders
    assert all(h.any() and not h.all() for h in hit) and not hit[1, 16].all() and not hit[1, :, 32].all() and (sphere == 1).any()
    return dict(local=local, link=link, link_poses=poses, rows=rows, cameras=cameras, config_of_view=cfg, cam_spheres=cam_spheres, t_near=t_near,
                sphere=sphere)


def test_partial_tiles_of_two_views_equal_the_specification(dev):
    """The smallest launch in which a wrong tile map or a wrong clamp of the lanes outside the image shows: 17 x 33 pixels and two
    views of two spheres.  cam_spheres, t_near and sphere equal robot_filter.py byte for byte with and without the cull, from
    camera records and from a CameraBatch's own; with an instance per sphere in that batch the cloud of pixel_clouds on the same
    images equals camera.pixel_clouds as bits."""
    from omg_planner_amd import camera, ops
    from tests import mesh_cases as MC
    c = partial_tiles_case()
    spheres = ops.RobotSpheres(c["local"], c["link"], device=dev)
    poses = torch.from_numpy(c["link_poses"]).to(dev)
    instances = np.zeros(4, camera.INSTANCE_DTYPE)
    instances["label"] = labels = [0, 1, 0, 1]  # (the instance image is the sphere image: sphere k of a view is its instance k)
    batch = ops.CameraBatch([MC.box_mesh(MC.BOX_HALF)], instances, [0, 2, 4], c["rows"], device=dev)
    for cameras in (c["cameras"], batch):
        for cull in (True, False):
            t_near, which, cs = ops.render_spheres(spheres, poses, cameras, c["config_of_view"], 17, 33, pad=0.01, t_min=1e-6, cull=cull)
            torch.cuda.synchronize()
            assert _same(cs, c["cam_spheres"]) and _same(t_near, c["t_near"]) and _same(which, c["sphere"]), cull
    for cls in (-1, 1):
        spec = camera.pixel_clouds(c["t_near"], c["sphere"], labels, [0, 2, 4], c["rows"], cls)
        points, begin = ops.pixel_clouds(batch, t_near, which, cls)
        torch.cuda.synchronize()
        assert len(spec[0]) > 0 and begin.tolist() == [0, len(spec[0]), len(spec[0]) + len(spec[1])], cls
        assert np.array_equal(points.cpu().numpy().view(np.int64), np.concatenate(spec).view(np.int64)), cls
