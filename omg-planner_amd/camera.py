"""A depth camera for the project's own scenes: the specification of omgx_render_depth / omgx_pixel_count / omgx_pixel_gather
(csrc/omg_camera.hip follows it operation by operation) and the device path `observe_scenes`.

The reference's perception entry (omg/core.py:826-867, `python -m omg.core -p`) renders the scene with an OpenGL/EGL renderer
(ycb_render/) to a mask and a point image, splits the pixels into target and non-target points, moves them to the robot base
frame with the view matrix (core.py:853: V[:3,:3].T (p - V[:3,3])) and draws a fixed number with np.random.choice; the
non-target cloud becomes the obstacle volume (PointEnv.compute_sdf_from_points, here ops.point_cloud_sdf).  An accelerator
without a graphics pipeline casts rays instead: one ray per pixel against the triangle meshes of the scene's instances.

Camera: intrinsics fx, fy, cx, cy and world_from_cam (12 doubles, the rows of a 3x4 matrix: the inverse of the reference's
renderer.V).  Optical axis +z, image row r downwards, column c to the right.  Pixel (r, c) is the ray from the camera origin
with dx = (c - cx) / fx, dy = (r - cy) / fy, dz = 1, so the hit parameter t is the depth along the axis.

Instance: one (mesh, pose, label), see INSTANCE_DTYPE and instance_records.

Everything specified is plain numpy float64 with every dot product written (x*x' + y*y') + z*z', so that the device can equal
the bits.  Not part of the contract: colour, textures, lighting, a far plane, noise (a sensor's frames become such images in sensor.py).  The robot's own links in a real image: robot_filter.py.
"""
from __future__ import annotations

import numpy as np

from . import _lib, grasps as _gr

# records of omgx_instance and omgx_camera (include/omg_hip.h section 14 explains the fields), 136 bytes each
INSTANCE_DTYPE, CAMERA_DTYPE = np.dtype(_lib.Instance), np.dtype(_lib.Camera)


def camera_rows(intrinsics, cam_from_world) -> np.ndarray:
    """One row of `cameras` [16]: fx, fy, cx, cy and the rows of world_from_cam = inv(cam_from_world) [3,4]."""
    k = np.asarray(intrinsics, np.float64).reshape(4)
    w = np.linalg.inv(np.asarray(cam_from_world, np.float64).reshape(4, 4))
    return np.concatenate([k, w[:3].ravel()])


def check_camera_rows(rows, S=None) -> np.ndarray:
    """`cameras` [S,16] (camera_rows) as float64, or ValueError: a wrong shape, a field that is not finite, a focal length of zero."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 2 or rows.shape[1] != 16 or (S is not None and len(rows) != S):
        raise ValueError(f"cameras must be [{'S' if S is None else S},16], got {rows.shape}")
    if not np.isfinite(rows).all() or (rows[:, :2] == 0).any():
        raise ValueError("a camera is not finite or has a focal length of zero")
    return rows


def camera_records(rows, inst_begin=None) -> np.ndarray:
    """CAMERA_DTYPE records of `cameras` [S,16] (camera_rows).  inst_begin [S+1]: scene s owns instances [inst_begin[s],
    inst_begin[s+1]); without it the instance range of every record stays (0, 0)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 16)
    rec = np.zeros(len(rows), CAMERA_DTYPE)
    for k, name in enumerate(("fx", "fy", "cx", "cy")):
        rec[name] = rows[:, k]
    rec["world_from_cam"] = rows[:, 4:]
    if inst_begin is not None:
        begin = np.asarray(inst_begin, np.int64).reshape(-1)
        rec["inst_begin"], rec["inst_count"] = begin[:-1], np.diff(begin)
    return rec


def instance_records(meshes, mesh_idx, poses, labels, cam_from_world) -> np.ndarray:
    """INSTANCE_DTYPE records of one scene's instances as one camera sees them.  meshes: the pool [(verts, faces)]; mesh_idx,
    poses [I,4,4] (object -> world), labels [I] (>= 0): one per instance; cam_from_world [4,4].

    m = rows of inv(cam_from_world @ pose) (np.linalg.inv; any invertible affine map keeps t).  The bounding ball: the
    instance's vertices in the camera frame, centre = the midpoint of their bounding box, r = the largest vertex distance
    from it, r2 = (r * (1 + 1e-6) + 1e-9) ** 2, q = ((c0*c0 + c1*c1) + c2*c2) - r2.  The kernel's contract starts at the
    records: how the host rounds m and the ball is not part of it."""
    cam_from_world = np.asarray(cam_from_world, np.float64).reshape(4, 4)
    rec = np.zeros(len(mesh_idx), INSTANCE_DTYPE)
    for i, (mi, pose, label) in enumerate(zip(mesh_idx, poses, labels)):
        if not 0 <= int(mi) < len(meshes):
            raise ValueError(f"instance {i}: mesh {mi} outside the pool of {len(meshes)}")
        if int(label) < 0:
            raise ValueError(f"instance {i}: label {label} is negative")
        cam_from_obj = cam_from_world @ np.asarray(pose, np.float64).reshape(4, 4)
        rec["m"][i] = np.linalg.inv(cam_from_obj)[:3].ravel()
        v = np.asarray(meshes[int(mi)][0], np.float64)
        vc = v @ cam_from_obj[:3, :3].T + cam_from_obj[:3, 3]
        c = 0.5 * (vc.min(0) + vc.max(0))
        r = float(np.sqrt(((vc - c) ** 2).sum(1)).max())
        r2 = (r * (1.0 + 1e-6) + 1e-9) ** 2
        rec["centre"][i] = c
        rec["q"][i] = ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) - r2
        rec["mesh"][i], rec["label"][i] = int(mi), int(label)
    return rec


def pixel_directions(cam, H: int, W: int):
    """(dx, dy) [H*W] of the pixels in row-major order: dx = (c - cx) / fx, dy = (r - cy) / fy."""
    r, c = np.divmod(np.arange(int(H) * int(W), dtype=np.int64), int(W))
    return (c.astype(np.float64) - cam[2]) / cam[0], (r.astype(np.float64) - cam[3]) / cam[1]


def instance_active(rec, dx, dy):
    """The cull of one instance record: can the pixel's ray meet the bounding ball?
    cd = (c0*dx + c1*dy) + c2, dd = (dx*dx + dy*dy) + 1.0, active = (q <= 0) | ((cd > 0) & (cd*cd >= q*dd))."""
    c, q = rec["centre"], float(rec["q"])
    cd = (c[0] * dx + c[1] * dy) + c[2]
    dd = (dx * dx + dy * dy) + 1.0
    return (q <= 0.0) | ((cd > 0.0) & (cd * cd >= q * dd))


def _check(instances, inst_begin, cameras):
    instances = np.asarray(instances)
    cameras = np.asarray(cameras, np.float64).reshape(-1, 16)
    inst_begin = np.asarray(inst_begin, np.int64)
    if instances.dtype != INSTANCE_DTYPE:
        raise ValueError("instances must be INSTANCE_DTYPE records (instance_records)")
    if len(inst_begin) != len(cameras) + 1 or inst_begin[0] < 0 or (np.diff(inst_begin) < 0).any() or inst_begin[-1] > len(instances):
        raise ValueError("inst_begin must be [S+1], ascending, within the instances")
    return instances, inst_begin, cameras


def render_depth(meshes, instances, inst_begin, cameras, H: int, W: int, cull: bool = True, t_min: float = 1e-6, tol: float = 1e-9):
    """Depth, instance and face images of S scenes -> (t [S,H,W] float64, inst [S,H,W] int32, face [S,H,W] int32); background:
    (+inf, -1, -1).  The specification of omgx_render_depth.

    meshes: the pool [(verts, faces)]; instances: INSTANCE_DTYPE records; scene s owns instances [inst_begin[s], inst_begin[s+1])
    (inst is local to the scene); cameras [S,16] (camera_rows).  Per pixel, from best = +inf, inst = -1, face = -1, for the
    scene's instances i = 0, 1, ... in order: active = instance_active (true everywhere with cull=False); the object-frame ray
    o' = (m[3], m[7], m[11]), d'_k = (m[4k]*dx + m[4k+1]*dy) + m[4k+2]; (t_i, f_i) = grasps.mesh_raycast(o', d', t_min, tol) on
    the instance's mesh; if active & (t_i < best): best = t_i, inst = i, face = f_i.  The strict < makes the lowest instance
    index win a tie.  The cull is part of the contract: an inactive pixel ignores the instance even if its ray would hit."""
    instances, inst_begin, cameras = _check(instances, inst_begin, cameras)
    S, H, W = len(cameras), int(H), int(W)
    t_img = np.full((S, H * W), np.inf)
    inst_img = np.full((S, H * W), -1, np.int32)
    face_img = np.full((S, H * W), -1, np.int32)
    for s in range(S):
        dx, dy = pixel_directions(cameras[s], H, W)
        for i, rec in enumerate(instances[inst_begin[s]: inst_begin[s + 1]]):
            active = instance_active(rec, dx, dy) if cull else np.ones(H * W, bool)
            if not active.any():
                continue  # (what the kernel skips too; the result is the same without this line)
            m = rec["m"]
            o = np.broadcast_to(np.array([m[3], m[7], m[11]]), (H * W, 3))
            d = np.stack([(m[4 * k] * dx + m[4 * k + 1] * dy) + m[4 * k + 2] for k in range(3)], -1)
            verts, faces = meshes[int(rec["mesh"])]
            t_i, f_i = _gr.mesh_raycast(verts, faces, o, d, t_min, tol)
            take = active & (t_i < t_img[s])
            t_img[s] = np.where(take, t_i, t_img[s])
            inst_img[s] = np.where(take, np.int32(i), inst_img[s])
            face_img[s] = np.where(take, f_i, face_img[s])
    return t_img.reshape(S, H, W), inst_img.reshape(S, H, W), face_img.reshape(S, H, W)


def pixel_mask(inst, labels, cls: int):
    """Which pixels of one scene's instance image [H,W] a cloud of class `cls` keeps: inst >= 0 and the instance's label equals
    cls; with cls < 0 every hit.  labels: the scene's own instance labels."""
    inst = np.asarray(inst)
    hit = (inst >= 0) & (inst < len(labels))  # anything else names no instance
    if int(cls) < 0 or len(labels) == 0:
        return hit
    return hit & (np.asarray(labels)[np.clip(inst, 0, len(labels) - 1)] == int(cls))


def pixel_clouds(t, inst, labels, inst_begin, cameras, cls: int):
    """The hit pixels of class `cls` as points in the world frame -> S arrays [N_s,3] float64.  The specification of
    omgx_pixel_count / omgx_pixel_gather.  t, inst [S,H,W]: render_depth's images; labels: the label of every instance (all
    scenes); the pixels are taken in row-major order (np.nonzero's); p = (t*dx, t*dy, t);
    w_k = ((W[4k]*p0 + W[4k+1]*p1) + W[4k+2]*p2) + W[4k+3] with W = world_from_cam."""
    cameras = np.asarray(cameras, np.float64).reshape(-1, 16)
    t, inst = np.asarray(t, np.float64), np.asarray(inst)
    S, H, W = t.shape
    out = []
    for s in range(S):
        keep = pixel_mask(inst[s], np.asarray(labels)[int(inst_begin[s]): int(inst_begin[s + 1])], cls).reshape(-1)
        dx, dy = pixel_directions(cameras[s], H, W)
        ts = t[s].reshape(-1)[keep]
        p = [ts * dx[keep], ts * dy[keep], ts]
        Wm = cameras[s, 4:]
        out.append(np.ascontiguousarray(np.stack([((Wm[4 * k] * p[0] + Wm[4 * k + 1] * p[1]) + Wm[4 * k + 2] * p[2]) + Wm[4 * k + 3]
                                                  for k in range(3)], -1)))
    return out


def draw(cloud, n: int, rng):
    """A fixed number of points of a cloud, as omg/core.py:855-856 draws them: cloud[rng.choice(len(cloud), n)].  On the host."""
    return cloud[rng.choice(len(cloud), int(n))]


def scene_records(scenes, meshes, cam_from_world, intrinsics):
    """The pooled meshes and records of S scenes.Scene -> (pool [(verts, faces)], instances, inst_begin [S+1], cameras [S,16]).
    meshes[s][o] is (verts, faces) in object o's frame or None (not drawn: the table); one instance per object that has a mesh,
    in object order, label 0 for scene.target_idx and 1 otherwise; a mesh given (the same arrays) to several objects is pooled
    once.  cam_from_world: [4,4] or [S,4,4]; intrinsics: (fx, fy, cx, cy) or [S,4]."""
    S = len(scenes)
    if len(meshes) != S:
        raise ValueError("meshes must have one list per scene")
    cfw = np.broadcast_to(np.asarray(cam_from_world, np.float64), (S, 4, 4))
    intr = np.broadcast_to(np.asarray(intrinsics, np.float64), (S, 4))
    pool, where, recs, begin = [], {}, [], [0]
    for s, scene in enumerate(scenes):
        if len(meshes[s]) != len(scene.objects):
            raise ValueError(f"scene {s}: meshes must have one entry (or None) per object")
        idx, poses, labels = [], [], []
        for o, obj in enumerate(scene.objects):
            if meshes[s][o] is None:
                continue
            key = (id(meshes[s][o][0]), id(meshes[s][o][1]))
            if key not in where:
                where[key] = len(pool)
                pool.append(meshes[s][o])
            idx.append(where[key]), poses.append(obj.pose_mat), labels.append(0 if o == scene.target_idx else 1)
        recs.append(instance_records(pool, idx, poses, labels, cfw[s]))
        begin.append(begin[-1] + len(idx))
    cameras = np.stack([camera_rows(intr[s], cfw[s]) for s in range(S)]) if S else np.zeros((0, 16))
    return pool, (np.concatenate(recs) if recs else np.zeros(0, INSTANCE_DTYPE)), np.array(begin, np.int64), cameras


class Observation:
    """observe_scenes' result: the images on the device (t [S,H,W] float64, inst and face [S,H,W] int32) and the batch;
    observe_volumes' has no face image and may have normals [S,H,W,3] float64; conditioned's has normals and the sensor flags
    [S,H,W] uint8; observe_frames' has no instances at all (inst and face are -1 everywhere)."""

    def __init__(self, batch, t, inst, face, normals=None, flags=None):
        self.batch, self.t, self.inst, self.face, self.normals, self.flags = batch, t, inst, face, normals, flags

    def _needs_instances(self, what: str) -> None:
        if getattr(self.batch, "frames_only", False):
            raise _lib.OmgHipError(f"{what} needs an instance image, and an observation built from sensor frames alone (observe_frames) has none")

    def conditioned(self, tau, cos_min: float = 0.0, scale: float = 1.0, z_min: float = 1e-3, z_max: float = 1e3, frames=None, **filter):
        """A new Observation on the same batch with the images conditioned as a sensor's frames (ops.condition_depth, then
        ops.depth_normals: two launches, no host sync; sensor.py is the specification): t is 0.0 where there is no return, a flying
        pixel or a grazing angle (cos < cos_min) and the bilateral filter's value elsewhere; inst and face are -1 on the dropped
        pixels, so that pixel_clouds emits no point at depth 0; normals [S,H,W,3] in the camera's frame, facing the camera (what
        observe_volumes' normals are); flags [S,H,W] uint8 (sensor.KEPT ...).  frames: None for self.t itself (float64, +inf is
        no return), or the sensor's [S,H,W] uint16 or float64 device tensor in its place (z = raw * scale for uint16).  tau =
        (t0, t1, t2); filter: min_support, radius, table, sigma_px, range_scale of ops.condition_depth."""
        import torch
        from . import ops
        source = self.t if frames is None else frames
        if tuple(source.shape) != tuple(self.t.shape):
            raise _lib.OmgHipError(f"frames must be {list(self.t.shape)}, as the observation's images, got {list(source.shape)}")
        depth, flags = ops.condition_depth(source, scale, z_min, z_max, tau, **filter)
        normals, t, flags, _ = ops.depth_normals(depth, self.intrinsics().reshape(-1, 4), tau, cos_min, flags=flags)
        dropped = ~(t > 0)
        inst = torch.where(dropped, torch.full_like(self.inst, -1), self.inst).contiguous()
        face = None if self.face is None else torch.where(dropped, torch.full_like(self.face, -1), self.face).contiguous()
        return Observation(self.batch, t, inst, face, normals, flags)

    def clouds(self, cls: int):
        """S contiguous float64 [N_s,3] device tensors in the world frame (what ops.point_cloud_sdf takes): class 0 is the
        target, 1 everything else, < 0 every hit."""
        from . import ops
        self._needs_instances("clouds")
        points, begin = ops.pixel_clouds(self.batch, self.t, self.inst, cls)
        return [points[int(begin[s]): int(begin[s + 1])] for s in range(len(begin) - 1)]

    def view_rows(self, table, pairs) -> np.ndarray:
        """fusion.view_rows [n,16] of the (scene, obj) `pairs` of an ops.DeviceScenes: the camera of the pair's scene, and
        cam_from_grid = inv(world_from_cam) @ world_from_obj with the object's pose from the table's host mirror."""
        from . import fusion
        cams, poses = self.batch.h_cameras, table_object_poses(table)
        views = np.zeros((len(pairs), 16))
        for m, (s, o) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2)):
            cam_from_world = np.linalg.inv(np.vstack([cams["world_from_cam"][s].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]]))
            views[m] = fusion.view_rows([cams[k][s] for k in ("fx", "fy", "cx", "cy")], cam_from_world @ poses[table._index(int(s), int(o))])
        return views

    def robot_view(self, spheres, robot_blob, P: int, joints, pad: float, tol: float, cull: bool = True):
        """The arm as this observation's cameras see it -> ops.RobotView (t_near, sphere, cam_spheres, tol, mask, all on the
        device).  spheres: ops.RobotSpheres; robot_blob, P: what ops.forward_kinematics takes; joints [S,9] float64 on the device:
        the arm's configuration in every scene's image.  One kinematics launch and one render launch (ops.render_spheres with the
        batch's own camera records; robot_filter.py is the specification); mask = explained(self.t, t_near, tol): the pixels
        that show the arm or what it hides, which serves as the `skip` of fit_supports too."""
        from . import ops
        S = self.batch.num_scenes
        if tuple(joints.shape) != (S, 9):
            raise _lib.OmgHipError(f"joints must be [{S},9], one configuration per scene, got {tuple(joints.shape)}")
        poses, _, _ = ops.forward_kinematics(robot_blob, P, joints, want_joint_info=False)
        H, W = int(self.t.shape[1]), int(self.t.shape[2])
        t_near, which, cam_spheres = ops.render_spheres(spheres, poses, self.batch, np.arange(S), H, W, pad=pad, cull=cull)
        view = ops.RobotView(t_near, which, cam_spheres, tol)
        view.mask = view.explained(self.t)
        return view

    def fuse_obstacles(self, table, pairs, layouts, band: float, near: float, reach: float, unknown_occupied: bool = True,
                       target_free: bool = True, robot=None) -> int:
        """The obstacle volumes of the (scene, obj) `pairs` of an ops.DeviceScenes from this observation's depth images
        (ops.DeviceScenes.fuse_obstacles, which documents layouts, band, near and reach): pair m is seen by the camera of its own
        scene, through the view row fusion.view_rows(intrinsics, cam_from_world @ world_from_obj) with the object's pose from the
        table's host mirror.  target_free: the pixels of label 0 (the target) count as background, so that the volume holds the
        non-target points only, as omg/core.py:849-851 splits them.  robot: robot_view's result (one image per scene): the arm's
        pixels carry no information and its nodes are cleared.  Returns the radius used."""
        pairs, depth, views, ranges, free_mask = self._obstacle_views(table, pairs, target_free)
        return table.fuse_obstacles(pairs, depth, views, ranges, layouts, band, near, reach, unknown_occupied, free_mask,
                                    robot=None if robot is None else robot.take(pairs[:, 0]))

    def _obstacle_views(self, table, pairs, target_free: bool):
        """What DeviceScenes.fuse_obstacles / integrate_obstacles take for the (scene, obj) `pairs`: (pairs [n,2], depth [n,H,W]:
        image m the one of pair m's scene, the view rows [n,16], view_range [n,2] = (m, 1), the target's pixels as a bool mask
        [n,H,W] or None)."""
        import torch
        if target_free:
            self._needs_instances("target_free")
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        views = self.view_rows(table, pairs)
        free_mask = None
        if target_free:
            labels, begin = self.batch.h_instances["label"], self.batch.h_inst_begin
            lut = [torch.from_numpy(np.concatenate([labels[int(begin[s]): int(begin[s + 1])] == 0, [False]])).to(self.inst.device)
                   for s in range(len(begin) - 1)]  # (the last entry: inst == -1, the background)
            free_mask = torch.stack([lut[int(s)][self.inst[int(s)].long()] for s in pairs[:, 0]])
        depth = self.t[torch.from_numpy(pairs[:, 0].copy()).to(self.t.device)].contiguous()
        return pairs, depth, views, np.stack([np.arange(len(pairs)), np.ones(len(pairs), np.int64)], -1), free_mask

    def integrate_obstacles(self, table, pairs, layouts, trunc: float, near: float, reach: float, tsdf_volumes=None,
                            unknown_occupied: bool = True, min_weight: float = 1.0, wmax: float = float("inf"), weights=None,
                            target_free: bool = True, robot=None):
        """fuse_obstacles with weighted TSDF fusion (ops.DeviceScenes.integrate_obstacles, which documents trunc, min_weight,
        wmax, weights and tsdf_volumes): the same view rows and the same target mask.  Passing the returned TsdfVolumes back in
        with a later observation adds its frame to the same volumes.  robot as fuse_obstacles takes it.
        Returns (radius, the TsdfVolumes)."""
        pairs, depth, views, ranges, free_mask = self._obstacle_views(table, pairs, target_free)
        return table.integrate_obstacles(pairs, tsdf_volumes, depth, views, ranges, layouts, trunc, near, reach, unknown_occupied, min_weight,
                                         wmax, weights, free_mask, robot=None if robot is None else robot.take(pairs[:, 0]))

    def segment_obstacles(self, table, target_pairs, obstacle_pairs, layouts, band: float, near: float, reach: float, seeds,
                          min_nodes: int, connectivity: int = 6, margin=None, free_mask=None, robot=None):
        """The target's and the obstacles' volumes of an ops.DeviceScenes from this observation's depth images ALONE
        (ops.DeviceScenes.segment_obstacles, which documents the arguments): no instance image is read.  Pair n is seen by the
        camera of its own scene through the view row of obstacle_pairs[n] (view_rows); the layout, the seed and the target's
        volume are in that object's frame, so target_pairs[n] should stand at the same pose.  free_mask: bool [n,H,W], the pixels
        that count as background (explained_mask of the known objects: the support); robot as fuse_obstacles takes it, so that
        the arm is no component.  -> (radius, records [n,8], Components)."""
        obstacle_pairs, depth, views, ranges, _ = self._obstacle_views(table, obstacle_pairs, target_free=False)
        return table.segment_obstacles(target_pairs, obstacle_pairs, depth, views, ranges, layouts, band, near, reach, seeds, min_nodes,
                                       connectivity, margin, free_mask, robot=None if robot is None else robot.take(obstacle_pairs[:, 0]))

    def intrinsics(self) -> np.ndarray:
        """[S,4] float64: fx, fy, cx, cy of every scene's camera, from the batch's host records."""
        cams = self.batch.h_cameras
        return np.stack([np.asarray(cams[k], np.float64) for k in ("fx", "fy", "cx", "cy")], -1)

    def fit_supports(self, triples, tol: float, up_world=None, cos_min: float = -1.0, refine: int = 2, min_nn: float = 1e-10, skip=None):
        """The support of every scene from its depth image ALONE: one plane per scene fitted to self.t (ops.fit_planes, which
        documents triples [S,K,3], tol, cos_min, refine and min_nn; planes.fit_planes is the specification), and the pixels on or
        behind it (ops.plane_mask), which segment_obstacles takes as free_mask in place of explained_mask's rendering of a known
        table.  up_world [3]: a direction of the world (the table's normal, roughly: gravity) that the plane's normal must agree
        with to within cos_min; it is turned into every camera's frame on the host (the rows of world_from_cam, transposed).
        skip: the pixels that take no part, as ops.fit_planes and ops.plane_mask take them (a RobotView's mask: the arm).
        -> (ops.PlaneFit, mask: bool [S,H,W] on the device).  The planes are in the cameras' frames: support_planes moves them."""
        from . import ops
        intr = self.intrinsics()
        up = None
        if up_world is not None:
            u = np.asarray(up_world, np.float64).reshape(3)
            up = np.stack([w.reshape(3, 4)[:, :3].T @ u for w in np.asarray(self.batch.h_cameras["world_from_cam"], np.float64)])
        fit = ops.fit_planes(intr, self.t, triples, tol, skip=skip, up=up, cos_min=cos_min, min_nn=min_nn, refine=refine)
        return fit, ops.plane_mask(intr, self.t, fit.planes, tol, skip=skip)

    def cam_from_world(self) -> np.ndarray:
        """[S,4,4] float64: the inverse (np.linalg.inv) of every scene's world_from_cam as the batch's host records hold it."""
        rows = np.asarray(self.batch.h_cameras["world_from_cam"], np.float64).reshape(-1, 3, 4)
        return np.stack([np.linalg.inv(np.vstack([w, [0.0, 0.0, 0.0, 1.0]])) for w in rows]) if len(rows) else np.zeros((0, 4, 4))

    def tracked(self, table, poses0=None, rounds: int = 1, skip=(), level: float = 0.0, min_inliers: int = 100, min_share: float = 0.5, **track):
        """The cameras of an observation made of sensor frames (observe_frames) corrected against the scene table: per round the
        table's volumes are ray-cast at the current cameras (observe_volumes with normals: the model), the frames are aligned to
        it (ops.track_cameras with self.t and self.normals; tracking.py is the specification), poses [S,12], stats [S,8] and the
        VALID pixel counts are downloaded once, and on the host tracking.accepted_mask (min_inliers, min_share) decides which
        views take tracking.compose's camera; a rejected view keeps the camera it had.  poses0 serves the first round, later
        rounds start from identity.  skip, level: observe_volumes'; track: stride, dist_max, cos_min, lambda0, step_tol,
        max_passes of ops.track_cameras.  -> (a new Observation with the same images on a new ops.FrameBatch with the corrected
        cameras, which integrate_obstacles, fuse_obstacles, segment_obstacles, fit_supports and robot_view take as any other;
        TrackResult: poses and stats of the last round, cam_from_world [S,4,4], accepted [S]: in any round).  It calls no planner."""
        import torch
        from . import ops, tracking
        if not getattr(self.batch, "frames_only", False):
            raise _lib.OmgHipError("tracked is for observations made of sensor frames (observe_frames): the instance records of a rendered "
                                   "observation are tied to the camera they were built for, and moving it would leave them stale")
        if int(rounds) < 1:
            raise _lib.OmgHipError(f"rounds must be >= 1, got {rounds}")
        S, H, W = (int(d) for d in self.t.shape)
        intr, cfw = self.intrinsics().reshape(S, 4), self.cam_from_world()
        stride = int(track.get("stride", 1))
        if stride < 1:
            raise _lib.OmgHipError("stride must be >= 1")
        there = (self.t > 0) & (self.t < float("inf"))
        if self.normals is not None:
            m = self.normals
            there &= (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2] > 0
        valid = there[:, ::stride, ::stride].reshape(S, -1).sum(1).to(torch.float64)  # tracking.valid_pixels, on the device
        accepted = np.zeros(S, bool)
        poses = stats = None
        for k in range(int(rounds)):
            model = observe_volumes(table, cfw, intr, H, W, level=level, skip=skip, want_normals=True)
            d_poses, d_stats = ops.track_cameras(self.t, self.normals, model.t, model.normals, intr, poses0 if k == 0 else None, **track)
            both = torch.cat([d_poses, d_stats, valid[:, None]], 1).cpu().numpy()  # one download
            poses, stats = np.ascontiguousarray(both[:, :12]), np.ascontiguousarray(both[:, 12:20])
            mask = tracking.accepted_mask(stats, min_inliers, min_share, both[:, 20])
            cfw = np.stack([tracking.compose(poses[s], cfw[s]) if mask[s] else cfw[s] for s in range(S)]) if S else cfw
            accepted |= mask
        cameras = np.stack([camera_rows(intr[s], cfw[s]) for s in range(S)]) if S else np.zeros((0, 16))
        obs = Observation(ops.FrameBatch(cameras, device=self.t.device), self.t, self.inst, self.face, self.normals, self.flags)
        return obs, TrackResult(poses=poses, cam_from_world=cfw, stats=stats, accepted=accepted)

    def support_planes(self, table, pairs, fit) -> np.ndarray:
        """The fitted planes [n,4] in the frames of the (scene, obj) `pairs` of an ops.DeviceScenes (what
        DeviceScenes.plane_obstacles takes): pair (s, o) gets the plane of scene s moved by planes.plane_to_frame with
        obj_from_cam = inv(world_from_obj) @ world_from_cam, the object's pose from the table's host mirror.  A scene without
        a plane is refused."""
        from . import planes as _pl
        cams, poses = self.batch.h_cameras, table_object_poses(table)
        h_planes = np.asarray(fit.h_planes if hasattr(fit, "h_planes") else fit.planes, np.float64).reshape(-1, 4)
        out = np.zeros((len(pairs), 4))
        for m, (s, o) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2)):
            if not _pl.has_plane(h_planes[s]):
                raise ValueError(f"scene {s} has no fitted plane")
            world_from_cam = np.vstack([np.asarray(cams["world_from_cam"][s], np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
            out[m] = _pl.plane_to_frame(h_planes[s], np.linalg.inv(poses[table._index(int(s), int(o))]) @ world_from_cam)
        return out


class TrackResult:
    """Observation.tracked's account, on the host: poses [S,12] (the rows [R t] of model_cam_from_live_cam) and stats [S,8] of the
    last round, cam_from_world [S,4,4]: the cameras of the returned observation, accepted [S] bool."""

    def __init__(self, poses, cam_from_world, stats, accepted):
        self.poses, self.cam_from_world, self.stats, self.accepted = poses, cam_from_world, stats, accepted


def explained_mask(t, t_known, tol: float):
    """The pixels of the depth images t that the known objects explain: t_known (their rendering, +inf where they are not seen)
    is finite and t >= t_known - tol.  Torch, elementwise, any shape -> bool.  As the free_mask of segment_obstacles it takes
    the support surface (observe_table on the table and plane rows) out before carving, so that objects standing on it are
    separate components; an object in front of the support stays (its depth is smaller by more than tol)."""
    import torch
    return torch.isfinite(t_known) & (t >= t_known - float(tol))


def observe_scenes(scenes, meshes, cam_from_world, intrinsics, H: int, W: int, cull: bool = True, device="cuda:0") -> Observation:
    """Depth and instance images of S scenes.Scene on the device, one launch (scene_records, ops.CameraBatch, ops.render_depth).
    It does not call the planner."""
    from . import ops
    pool, instances, inst_begin, cameras = scene_records(scenes, meshes, cam_from_world, intrinsics)
    if not pool:
        raise ValueError("no object of any scene has a mesh")
    batch = ops.CameraBatch(pool, instances, inst_begin, cameras, device=device)
    t, inst, face = ops.render_depth(batch, H, W, cull=cull)
    return Observation(batch, t, inst, face)


def observe_frames(frames, scale: float, cam_from_world, intrinsics, tau, cos_min: float = 0.0, z_min: float = 1e-3, z_max: float = 1e3,
                   device="cuda:0", **filter) -> Observation:
    """An Observation from sensor frames ALONE: frames [S,H,W], uint16 (z = raw * scale, 0 is no return) or float64 (z as given), a
    device tensor or a host array (uploaded), one per camera, conditioned on the device (Observation.conditioned, which documents
    tau, cos_min, z_min, z_max and filter).  cam_from_world: [4,4] or [S,4,4]; intrinsics: (fx, fy, cx, cy) or [S,4].  Its batch
    (ops.FrameBatch) has the cameras and no instances; inst and face are -1 everywhere; normals and flags are filled.
    What works on it: tracked (its cameras corrected against a scene table), segment_obstacles, fit_supports, support_planes, robot_view,
    view_rows, intrinsics, conditioned, and
    fuse_obstacles / integrate_obstacles with target_free=False.  What needs an instance image and raises: clouds, and
    fuse_obstacles / integrate_obstacles with target_free=True.  It does not call the planner."""
    import torch
    from . import ops
    if not isinstance(frames, torch.Tensor):
        frames = np.ascontiguousarray(frames)
        if frames.dtype not in (np.uint16, np.float64):
            raise _lib.OmgHipError(f"frames must be uint16 or float64, got {frames.dtype}")
        frames = torch.from_numpy(frames).to(device)
    if frames.dim() != 3:
        raise _lib.OmgHipError(f"frames must be [S,H,W], got {tuple(frames.shape)}")
    S = int(frames.shape[0])
    cfw = np.broadcast_to(np.asarray(cam_from_world, np.float64), (S, 4, 4))
    intr = np.broadcast_to(np.asarray(intrinsics, np.float64), (S, 4))
    cameras = np.stack([camera_rows(intr[s], cfw[s]) for s in range(S)]) if S else np.zeros((0, 16))
    batch = ops.FrameBatch(cameras, device=frames.device)
    none = torch.full(tuple(frames.shape), -1, dtype=torch.int32, device=frames.device)
    blank = Observation(batch, torch.zeros(tuple(frames.shape), dtype=torch.float64, device=frames.device), none, none)
    return blank.conditioned(tau, cos_min, scale, z_min, z_max, frames=frames.contiguous(), **filter)


def table_object_poses(table) -> np.ndarray:
    """world_from_obj [n,4,4] float64 of every record of an ops.DeviceScenes, from the host mirror: the inverse, in float64, of the
    float32 rows [R t] the record keeps (pose_inv)."""
    inv = np.asarray(table.host_objects["pose_inv"], np.float64).reshape(-1, 3, 4)
    out = np.tile(np.eye(4), (len(inv), 1, 1))
    for k, m in enumerate(inv):
        out[k, :3, :3] = m[:, :3].T
        out[k, :3, 3] = -(m[:, :3].T @ m[:, 3])
    return out


def observe_table(table, cam_from_world, intrinsics, H: int, W: int, level: float = 0.0, targets=None, skip=(), cull: bool = True) -> Observation:
    """observe_scenes for an ops.DeviceScenes that has no meshes: the level set of every object's volume is extracted on the device
    (DeviceScenes.object_surfaces, read in place, shared volumes once), downloaded once, and drawn at the object's pose
    (table_object_poses) through the host-side builders of observe_scenes (instance_records, ops.CameraBatch).  targets [S]: the
    object of each scene that gets label 0 (default 0), every other object 1; skip: (scene, object) pairs that are not drawn (a
    table slab); an object whose surface is empty at `level` is not drawn either.  It does not call the planner."""
    from . import ops
    S = table.num_scenes
    cfw = np.broadcast_to(np.asarray(cam_from_world, np.float64), (S, 4, 4))
    intr = np.broadcast_to(np.asarray(intrinsics, np.float64), (S, 4))
    verts, faces, vrows, frows, _ = table.object_surfaces(level=level)
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    poses, skip = table_object_poses(table), {(int(s), int(o)) for s, o in skip}
    pool, where, recs, begin = [], {}, [], [0]
    for s in range(S):
        lo, hi = int(table.host_scene_begin[s]), int(table.host_scene_begin[s + 1])
        target = 0 if targets is None else int(targets[s])
        idx, ps, labels = [], [], []
        for k in range(lo, hi):
            if (s, k - lo) in skip or frows[k, 1] == 0:
                continue
            key = (int(vrows[k, 0]), int(frows[k, 0]))
            if key not in where:
                where[key] = len(pool)
                pool.append((hv[vrows[k, 0]: vrows[k, 0] + vrows[k, 1]], hf[frows[k, 0]: frows[k, 0] + frows[k, 1]]))
            idx.append(where[key]), ps.append(poses[k]), labels.append(0 if k - lo == target else 1)
        recs.append(instance_records(pool, idx, ps, labels, cfw[s]))
        begin.append(begin[-1] + len(idx))
    if not pool:
        raise ValueError("no object of any scene has a surface at this level")
    cameras = np.stack([camera_rows(intr[s], cfw[s]) for s in range(S)])
    batch = ops.CameraBatch(pool, np.concatenate(recs), np.array(begin, np.int64), cameras, device=table.device)
    t, inst, face = ops.render_depth(batch, H, W, cull=cull)
    return Observation(batch, t, inst, face)


def observe_volumes(table, cam_from_world, intrinsics, H: int, W: int, level: float = 0.0, targets=None, skip=(), want_normals: bool = False,
                    **march) -> Observation:
    """observe_table without the meshes: the objects of an ops.DeviceScenes are ray-cast as volumes, in place, in one launch
    (ops.render_volumes; volume_camera.render_volumes is the specification).  Nothing is extracted or downloaded and no pose is
    read from the host mirror: a pose written on the device is seen without sync_host.  targets [S]: the object of each scene that
    gets label 0 (default 0), every other object 1; skip: (scene, object) pairs that are not drawn; march: min_step, relax,
    max_steps, t_min of ops.render_volumes.  The instance image names the object's index in its scene (observe_table's names the
    drawn instances); face is None; normals [S,H,W,3] (camera frame) with want_normals.  It does not call the planner."""
    from . import ops
    S = table.num_scenes
    cfw = np.broadcast_to(np.asarray(cam_from_world, np.float64), (S, 4, 4))
    intr = np.broadcast_to(np.asarray(intrinsics, np.float64), (S, 4))
    cameras = np.stack([camera_rows(intr[s], cfw[s]) for s in range(S)]) if S else np.zeros((0, 16))
    n = len(table.host_objects)
    labels, visible = np.ones(n, np.int64), np.ones(n, np.uint8)
    for s in range(S):
        labels[table._index(s, 0 if targets is None else int(targets[s]))] = 0
    for s, o in skip:
        visible[table._index(int(s), int(o))] = 0
    batch = ops.VolumeCameraBatch(table, cameras, labels)
    t, inst, normals, _ = ops.render_volumes(table, cameras, H, W, visible=visible, level=level, want_normals=want_normals, **march)
    return Observation(batch, t, inst, None, normals)
