"""The cases the robot self-filter's tests share (tests/test_robot_filter_cpu.py, tests/test_gpu_robot_filter.py,
tests/fuzz/fuzz_robot_filter.py): render and clear set-ups with the answers worked out by hand, the seeded random batch, and the
observed scene of fusion_cases with an arm of spheres in front of it.  Everything is computed once per process
(functools.lru_cache) and never changed."""
from __future__ import annotations

import functools

import numpy as np

from tests import fusion_cases as FC

INF, NAN = float("inf"), float("nan")
F, S, U = 0, 1, 2
CHUNK = 256  # OMGX_ROBOT_SPHERE_CHUNK (test_robot_filter_cpu.py asserts it is the header's)
GUARD = 9    # a state byte that is none of 0, 1, 2, around and between the volumes


def camera_records(cam_from_world, intrinsics):
    """camera.CAMERA_DTYPE records of V cameras: cam_from_world [V,4,4], intrinsics (fx, fy, cx, cy) or [V,4]."""
    from omg_planner_amd import camera
    cfw = np.asarray(cam_from_world, np.float64).reshape(-1, 4, 4)
    k = np.broadcast_to(np.asarray(intrinsics, np.float64), (len(cfw), 4))
    return camera.camera_records(np.array([camera.camera_rows(k[v], cfw[v]) for v in range(len(cfw))]).reshape(-1, 16))


# ---------------------------------------------------------------------------------------------------------------------
# render: one camera at the origin looking along +z with fx = fy = 1, cx = cy = 0, so that pixel (0, 0) is the ray (0, 0, 1) and
# dd = 1; t_min = 0.25.  Every number below is exact in binary.  (what it is about, spheres (x, y, z, R), t_near and sphere of
# pixel (0, 0))
# ---------------------------------------------------------------------------------------------------------------------
RENDER_T_MIN = 0.25
RENDER_CASES = (
    # b = 2, q = 4 - 0.25, disc = 0.25, s = 0.5: t0 = 1.5, t1 = 2.5
    ("a ray through the centre", [(0.0, 0.0, 2.0, 0.5)], 1.5, 0),
    # b = 2, q = (0.25 + 4) - 0.25 = 4, disc = 0: t0 = t1 = 2
    ("a tangent ray: disc == 0 is a hit", [(0.5, 0.0, 2.0, 0.5)], 2.0, 0),
    # b = 0, q = -1, disc = 1: t0 = -1, t1 = 1 > t_min: the entry is t_min
    ("the camera inside a sphere sees it at t_min", [(0.0, 0.0, 0.0, 1.0)], 0.25, 0),
    # b = -2, q = 3.75, disc = 0.25: t0 = -2.5, t1 = -1.5
    ("a sphere behind the camera", [(0.0, 0.0, -2.0, 0.5)], INF, -1),
    # b = -0.25, q = 0.0625 - 0.25, disc = 0.0625 + 0.1875 = 0.25: t1 = -0.25 + 0.5 = 0.25 == t_min
    ("t1 == t_min is a miss", [(0.0, 0.0, -0.25, 0.5)], INF, -1),
    ("two identical spheres: the lowest index", [(0.0, 0.0, 2.0, 0.5), (0.0, 0.0, 2.0, 0.5)], 1.5, 0),
    # the second is nearer (t0 = 1), the third ties with it
    ("the smallest entry wins, the lowest index on a tie", [(0.0, 0.0, 2.0, 0.5), (0.0, 0.0, 1.5, 0.5), (0.0, 0.0, 1.5, 0.5)], 1.0, 1),
    # q = 4, disc = 4 - 4 = 0: a point on the ray is hit at its depth
    ("radius 0 and pad 0: a point on the ray", [(0.0, 0.0, 2.0, 0.0)], 2.0, 0),
    ("radius 0 and pad 0: a point beside the ray", [(0.25, 0.0, 2.0, 0.0)], INF, -1),
)
RENDER_PAD_CASE = ("radius 0 with pad 0.5 is the first case", [(0.0, 0.0, 2.0, 0.0)], 0.5, 1.5, 0)
IDENTITY_CAMERA = (1.0, 1.0, 0.0, 0.0)


def render_edge_launch():
    """The render cases as ONE launch: case k's spheres sit on link k % 10 of configuration k, whose other links stand 1024 behind
    the camera (their spheres are misses for every pixel), and view k has configuration k.  -> dict(local, link, link_poses,
    cameras, config_of_view, first: the index of case k's first sphere, H, W)."""
    assert len(RENDER_CASES) <= 10
    local, link, first = [], [], []
    for k, (_, spheres, _, _) in enumerate(RENDER_CASES):
        first.append(len(local))
        local += list(spheres)
        link += [k] * len(spheres)
    K = len(RENDER_CASES)
    poses = np.tile(np.eye(4), (K, 10, 1, 1))
    for k in range(K):
        for l in range(10):
            if l != k:
                poses[k, l, 2, 3] = -1024.0
    return dict(local=np.array(local, np.float64), link=np.array(link, np.int64), link_poses=poses,
                cameras=camera_records(np.tile(np.eye(4), (K, 1, 1)), IDENTITY_CAMERA), config_of_view=np.arange(K), first=first, H=2, W=3)


# ---------------------------------------------------------------------------------------------------------------------
# clear: ONE ragged batch with the answers written out, as fusion_cases.EDGE_CASES.  Two identity cameras (node (x, y, z) falls
# on column floor(x / z + 0.5), row floor(y / z + 0.5)) with images of 2 x 4, near = 1, tol = 0.25.
# View 0 has the arm at depth 3 in most pixels and no sphere near the nodes; view 1 sees no arm (t_near = inf) but has spheres.
# ---------------------------------------------------------------------------------------------------------------------
CLEAR_NEAR, CLEAR_TOL = 1.0, 0.25
CLEAR_DEPTH = np.array([[[INF, 2.0, NAN, INF], [-1.0, 2.75, 0.0, INF]],
                        [[NAN, NAN, NAN, NAN], [NAN, NAN, NAN, NAN]]])
CLEAR_T_NEAR = np.array([[[3.0, 3.0, 3.0, 3.0], [3.0, 3.0, 3.0, INF]],
                         [[INF, INF, INF, INF], [INF, INF, INF, INF]]])
_FAR = (0.0, 0.0, -1024.0, 0.0)
CLEAR_SPHERES = np.array([[_FAR, _FAR], [(0.0, 0.0, 2.0, 0.5), (4.0, 0.0, 0.5, 0.5)]])
# (what it is about, volume, view range, old states, new states)
CLEAR_CASES = (
    # pixel (0, 0): depth inf behind the arm at 3: explained.  z = 0.5 .. 3.5
    ("front: z == near is not seen, z == t_near is not in front", ((0.0, 0.0, 0.5), 0.5, "node", (1, 1, 7)), (0, 1), [U] * 7, [U, U, F, F, F, U, U]),
    # x / z = -1, -0.5 .. 4.5 at z = 2, row 0: columns -1 | 0 0 1 1 2 2 3 3 | 4 4 5; depths inf, 2 (an object in front of the arm:
    # 2 < 3 - 0.25), NaN, inf
    ("columns: pixel -0.5 inside, W - 0.5 outside; an object in front of the arm and a NaN depth stay",
     ((-2.0, 0.0, 2.0), 1.0, "node", (12, 1, 1)), (0, 1), [U] * 12, [U, F, F, U, U, U, U, F, F, U, U, U]),
    # row 1 (y = 2 at z = 2), columns 0 .. 3: depths -1, 2.75 (== t_near - tol: explained), 0, and inf where no arm is seen
    ("depths negative and 0 are not explained, t_near - tol is; no arm, no clearing", ((0.0, 2.0, 2.0), 2.0, "node", (4, 1, 1)), (0, 1),
     [U] * 4, [U, F, U, U]),
    ("a SURFACE or FREE node in front of the arm stays", ((0.0, 0.0, 1.5), 0.5, "node", (1, 1, 3)), (0, 1), [S, F, U], [S, F, F]),
    # view 1, the sphere (0, 0, 2; 0.5): distances 1, 0.5 (== R: inside), 0, 0.5, 1
    ("SURFACE and UNKNOWN nodes inside a sphere become FREE", ((0.0, 0.0, 1.0), 0.5, "node", (1, 1, 5)), (1, 1), [S, S, S, U, U], [S, F, F, F, U]),
    # view 1, the sphere (4, 0, 0.5; 0.5): z = 0.5 < near, the node is not seen
    ("inside does not depend on seen", ((4.0, 0.0, 0.5), 1.0, "node", (1, 1, 1)), (1, 1), [S], [F]),
    ("an empty view range changes nothing", ((0.0, 0.0, 1.5), 0.5, "node", (1, 1, 3)), (0, 0), [S, U, F], [S, U, F]),
    # both views: front (view 0) does not free SURFACE, inside (view 1) does; z = 1.5 .. 3
    ("two views: inside in one of them is enough", ((0.0, 0.0, 1.5), 0.5, "node", (1, 1, 4)), (0, 2), [S, S, U, U], [F, F, F, U]),
    ("bytes that are no state stay unless a sphere holds them", ((0.0, 0.0, 2.0), 0.5, "node", (1, 1, 3)), (0, 2), [7, 7, 7], [F, F, 7]),
)


def clear_views():
    return np.stack([FC.view(), FC.view()])


def clear_edge_batch():
    """The clear cases as one batch with GUARD bytes before, between and behind the volumes -> dict(volumes, ranges, begin, state,
    want)."""
    volumes, ranges = [c[1] for c in CLEAR_CASES], [c[2] for c in CLEAR_CASES]
    begin, at = [], 3
    for c in CLEAR_CASES:
        begin.append(at)
        at += len(c[3]) + 2
    state, want = np.full(at + 1, GUARD, np.uint8), np.full(at + 1, GUARD, np.uint8)
    for b, c in zip(begin, CLEAR_CASES):
        state[b: b + len(c[3])], want[b: b + len(c[4])] = c[3], c[4]
    return dict(volumes=volumes, ranges=ranges, begin=np.array(begin, np.int64), state=state, want=want)


# ---------------------------------------------------------------------------------------------------------------------
# the seeded random batch: 40 x 48 images (edge tiles), V = 3 views of C = 2 configurations, three volumes of which the last
# spans several runs of 256 nodes, N spheres; the third camera stands inside a sphere of its configuration; depth images with
# values that are not finite, that are 0 or negative, and that lie within tol of the arm
# ---------------------------------------------------------------------------------------------------------------------
BATCH_H, BATCH_W = 40, 48
BATCH_N = (1, 7, CHUNK + 1)
BATCH_VOLUMES = [((-0.01, -0.01, 0.0), 0.01, "node", (2, 2, 2)), ((-0.03, -0.05, 0.0), 0.011, "centre", (5, 9, 7)),
                 ((-0.16, -0.08, -0.02), 0.01, "centre", (33, 17, 9))]
BATCH_RANGES = [(0, 3), (1, 2), (2, 1)]
BATCH_PAD, BATCH_T_MIN, BATCH_NEAR, BATCH_TOL = 0.01, 1e-6, 0.05, 0.01


def _random_pose(rng, reach):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    m = np.eye(4)
    m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    m[:3, 3] = rng.uniform(-reach, reach, 3)
    return m


@functools.lru_cache(maxsize=None)
def batch(N, seed=0):
    """One draw of the batch with N spheres, with the specification's own answers (cam_spheres, t_near, sphere, want)."""
    from omg_planner_amd import fusion, robot_filter as rf
    rng = np.random.default_rng(1000 * seed + N)
    local = np.concatenate([rng.uniform(-0.05, 0.05, (N, 3)), rng.uniform(0.0, 0.06, (N, 1))], 1)
    local[0, 3] = 0.05
    if N > 2:
        local[1, 3] = 0.0  # a point
        local[2] = local[0]  # two identical spheres
    link = rng.integers(0, 10, N)
    if N > 2:
        link[2] = link[0]
    poses = np.stack([np.stack([_random_pose(rng, 0.15) for _ in range(10)]) for _ in range(2)])
    config_of_view = np.array([0, 1, 1])
    # the third camera's eye lies 0.02 from the centre of sphere 0 (radius 0.05 + pad) in configuration 1
    inside = (poses[1, link[0]] @ np.append(local[0, :3], 1.0))[:3] + np.array([0.0, 0.02, 0.0])
    eyes = [(0.5, 0.1, 0.4), (-0.3, 0.45, 0.3), tuple(inside)]
    cfw = np.stack([FC.look_at(e, (0.0, 0.0, 0.03)) for e in eyes])
    cameras = camera_records(cfw, (60.0, 55.0, 23.5, 19.5))
    views = np.stack([fusion.view_rows((60.0, 55.0, 23.5, 19.5), cfw[v]) for v in range(3)])  # (the grid frame is the world frame)
    cam_spheres = rf.camera_spheres(poses, local, link, cameras, config_of_view, BATCH_PAD)
    t_near, which = rf.render_spheres(cam_spheres, cameras, BATCH_H, BATCH_W, BATCH_T_MIN)
    depth = rng.uniform(0.2, 0.9, t_near.shape)
    close = np.isfinite(t_near) & (rng.random(t_near.shape) < 0.6)
    depth[close] = (t_near + rng.uniform(-3 * BATCH_TOL, 3 * BATCH_TOL, t_near.shape))[close]
    on_edge = np.isfinite(t_near) & (rng.random(t_near.shape) < 0.05)
    depth[on_edge] = (t_near - BATCH_TOL)[on_edge]
    for value in (NAN, INF, -INF, 0.0, -0.3):
        depth[rng.random(depth.shape) < 0.03] = value
    sizes = [int(np.prod(v[3])) for v in BATCH_VOLUMES]
    begin, at = [], 5
    for n in sizes:
        begin.append(at)
        at += n + 7
    state = np.full(at, GUARD, np.uint8)
    for b, n in zip(begin, sizes):
        state[b: b + n] = rng.choice(np.array([F, S, U, 7], np.uint8), size=n, p=[0.2, 0.3, 0.45, 0.05])
    begin = np.array(begin, np.int64)
    want = rf.clear_states(state, BATCH_VOLUMES, views, BATCH_RANGES, depth, BATCH_NEAR, t_near, cam_spheres, BATCH_TOL, state_begin=begin)
    return dict(N=N, local=local, link=link, link_poses=poses, cameras=cameras, config_of_view=config_of_view, views=views,
                cam_spheres=cam_spheres, t_near=t_near, sphere=which, depth=depth, begin=begin, state=state, want=want)


# ---------------------------------------------------------------------------------------------------------------------
# the path: fusion_cases' scene (a sphere above a slab, three cameras, a 32 x 32 x 24 grid of 1 cm) with an arm of six spheres
# that reaches into the grid between the first camera and the scene.  Link 0 stands at the identity, so local is the world.
# ---------------------------------------------------------------------------------------------------------------------
ARM_RADIUS, ARM_PAD, ARM_TOL = 0.025, 0.01, 0.01
ARM_CENTRES = np.array([(0.10 + 0.03 * k, 0.09, 0.15 + 0.02 * k) for k in range(6)])


@functools.lru_cache(maxsize=None)
def scene_with_arm():
    """dict: t_scene (the arm-free images), t_arm (the arm of radius ARM_RADIUS composited in: min), cameras, views, and the
    filter's cam_spheres and t_near at radius + ARM_PAD."""
    from omg_planner_amd import robot_filter as rf
    t_scene, views = FC.scene_depth()
    cfw, intr = FC.scene_cameras()
    cameras = camera_records(cfw, intr)
    local = np.concatenate([ARM_CENTRES, np.full((len(ARM_CENTRES), 1), ARM_RADIUS)], 1)
    link, poses, cfg = np.zeros(len(local), np.int64), np.tile(np.eye(4), (1, 10, 1, 1)), np.zeros(3, np.int64)
    bare, _ = rf.render_spheres(rf.camera_spheres(poses, local, link, cameras, cfg, 0.0), cameras, FC.H, FC.W)
    cam_spheres = rf.camera_spheres(poses, local, link, cameras, cfg, ARM_PAD)
    t_near, _ = rf.render_spheres(cam_spheres, cameras, FC.H, FC.W)
    return dict(t_scene=t_scene, t_arm=np.minimum(t_scene, bare), cameras=cameras, views=views, local=local, link=link, link_poses=poses,
                config_of_view=cfg, cam_spheres=cam_spheres, t_near=t_near)


# ---------------------------------------------------------------------------------------------------------------------
# the Panda in front of fusion_cases' sphere and slab: the scene's frame stands at PANDA_POSE in the world (the robot's base
# frame), so that the hand and the fingers of the home configuration hang over the sphere, inside a 32^3 layout of 1 cm, and a
# 64 x 48 camera looks down on both.  One sphere of radius 0.04 per collision point.
# ---------------------------------------------------------------------------------------------------------------------
PANDA_POSE = np.eye(4)
PANDA_POSE[:3, 3] = (0.15625, 0.0, 0.34375)  # (exact in float32: the scene table keeps the pose's inverse in float32)
PANDA_LAYOUT = ((-0.16, -0.16, 0.0), 0.01, (32, 32, 32))
PANDA_VOLUME = PANDA_LAYOUT[:2] + ("centre", PANDA_LAYOUT[2], 0)
PANDA_EYE, PANDA_TARGET = (0.5, 0.05, 1.0), (0.16, 0.0, 0.45)
PANDA_RADIUS, PANDA_PAD, PANDA_TOL = 0.04, 0.01, 0.01
PANDA_MOVED = np.array([0.9, -1.0, 0.0, -2.0, 0.0, 1.571, 0.785, 0.04, 0.04])  # the second configuration: the hand swung aside


def panda_camera():
    """(cam_from_world [4,4], intrinsics)"""
    return FC.look_at(PANDA_EYE, PANDA_TARGET), (FC.F, FC.F, FC.CX, FC.CY)


def panda_scene_records():
    """What ops.CameraBatch takes for ONE scene: the sphere and the slab at PANDA_POSE, both label 1."""
    from omg_planner_amd import camera
    cfw, intr = panda_camera()
    meshes = FC.scene_meshes()
    return meshes, camera.instance_records(meshes, [0, 1], [PANDA_POSE, PANDA_POSE], [1, 1], cfw), np.array([0, 2], np.int64), camera.camera_rows(intr, cfw)[None]


def panda_spheres(collision_points):
    """(local [10 P, 4], link [10 P]) as ops.RobotSpheres.from_points lays them out."""
    pts = np.asarray(collision_points, np.float64)
    return np.concatenate([pts.reshape(-1, 3), np.full((pts.shape[0] * pts.shape[1], 1), PANDA_RADIUS)], 1), np.repeat(np.arange(10), pts.shape[1])


def panda_exempt(views, mask, cam_spheres, volume=None):
    """bool [nodes]: the nodes of the layout that lie inside a sphere of cam_spheres [V,N,4] or project onto a pixel of mask
    [V,H,W] in a view that sees them (near = FC.NEAR)."""
    from omg_planner_amd import fusion
    origin, delta, _, dims = (PANDA_VOLUME if volume is None else volume)[:4]
    p = fusion.node_points(np.array(origin), delta, 0.5, dims)
    out = np.zeros(len(p), bool)
    H, W = mask.shape[1:]
    for v in range(len(views)):
        q = np.stack([((views[v][4 + 4 * k] * p[:, 0] + views[v][5 + 4 * k] * p[:, 1]) + views[v][6 + 4 * k] * p[:, 2]) + views[v][7 + 4 * k] for k in range(3)], 1)
        c, r = np.floor((views[v][0] * (q[:, 0] / q[:, 2]) + views[v][2]) + 0.5), np.floor((views[v][1] * (q[:, 1] / q[:, 2]) + views[v][3]) + 0.5)
        seen = (q[:, 2] > FC.NEAR) & (c >= 0) & (c <= W - 1) & (r >= 0) & (r <= H - 1)
        out |= seen & mask[v][np.where(seen, r, 0).astype(int), np.where(seen, c, 0).astype(int)]
        for x, y, z, R in cam_spheres[v]:
            out |= ((q[:, 0] - x) ** 2 + (q[:, 1] - y) ** 2 + (q[:, 2] - z) ** 2) <= (R + 1e-9) ** 2
    return out
