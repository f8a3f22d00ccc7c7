"""The cases the camera-tracking tests share (tests/test_track_cpu.py, tests/test_gpu_track.py): the fronto-parallel planes whose
answers are worked by hand, seeded synthetic views for the bit comparisons, the views that stop at different turns, and the
recovery scene (slab, sphere, box) rendered by the project's own ray-cast.  Everything is computed once per process
(functools.lru_cache) and never changed."""
from __future__ import annotations

import functools

import numpy as np

from tests import volume_camera_cases as VC

SHAPES = ((1, 1), (16, 16), (17, 33), (23, 89), (32, 64), (3, 683), (48, 64))  # 2047, 2048 and 2049 pixels among them
STRIDES = (1, 2, 3)
PASSES = (0, 1, 2, 12)
TAU, NORMAL_COS = (0.012, 0.0, 0.02), 0.15  # sensor.depth_normals' arguments for every live normal map here
DEFAULT = dict(stride=1, dist_max=0.05, cos_min=0.7, lambda0=2.0 ** -10, step_tol=1e-6, max_passes=12)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same(got, want) -> bool:
    """(poses, stats) against (poses, stats) bit for bit; a NaN equals a NaN."""
    return bool(VC.same_bits(got[0], want[0]) and VC.same_bits(got[1], want[1]))


# ---------------------------------------------------------------------------------------------------------------------
# planes worked by hand: the identity camera fx = fy = 1, cx = cy = 0 unless said otherwise; the model plane z = 1 with the
# normal (0, 0, -1) (facing the camera), the live plane z = 1.25.  Every number is exact in binary.
# ---------------------------------------------------------------------------------------------------------------------
def planes(H, W, z_live=1.25, z_model=1.0, with_normals=True):
    """(zl [1,H,W], nl or None, zm, nm) of two fronto-parallel planes."""
    zl, zm = np.full((1, H, W), float(z_live)), np.full((1, H, W), float(z_model))
    n = np.zeros((1, H, W, 3))
    n[..., 2] = -1.0
    return zl, (n.copy() if with_normals else None), zm, n.copy()


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rigid(axis, angle, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = rotation(axis, angle), t
    return M


def rows(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).reshape(4, 4)[:3].reshape(12))


# ---------------------------------------------------------------------------------------------------------------------
# seeded synthetic views for the bit comparisons: a bumpy surface seen by V cameras with different intrinsics; the live frame is
# the model's own image, the start poses are a few millimetres and a degree away, so that trials are accepted and rejected;
# holes in both images, pixels without a normal, one model pixel with a zero normal
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic(H, W, V=3, seed=0, dirty=False):
    """(zl [V,H,W], nl [V,H,W,3], zm, nm, intrinsics [V,4], poses0 [V,12]).  dirty: NaN and infinities sprinkled in."""
    from omg_planner_amd import sensor
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    f = 0.9 * max(H, W, 8)
    intr = np.stack([[f * (1.0 + 0.1 * v), f * (1.0 - 0.05 * v), 0.5 * (W - 1) + 0.3 * v, 0.5 * (H - 1) - 0.2 * v] for v in range(V)]).reshape(V, 4)
    z = np.stack([0.8 + 0.1 * v + 0.06 * np.sin(0.37 * c + v) * np.cos(0.29 * r) + 0.002 * c + 0.03 * np.cos(0.11 * (r + c)) for v in range(V)]).reshape(V, H, W)
    zm = z.copy()
    zm[rng.random(z.shape) < 0.05] = np.inf
    nm = sensor.depth_normals(np.where(np.isfinite(zm), zm, 0.0), intr, TAU, NORMAL_COS)[0] if V else np.zeros((0, H, W, 3))
    zl = z.copy()
    zl[rng.random(z.shape) < 0.05] = 0.0
    nl, zl, _, _ = sensor.depth_normals(zl, intr, TAU, NORMAL_COS) if V else (np.zeros((0, H, W, 3)), zl, None, None)
    if V and H * W > 4:
        nm[0].reshape(-1, 3)[(H * W) // 2] = 0.0
    poses0 = np.stack([rows(rigid(rng.normal(size=3), np.deg2rad(rng.uniform(0.2, 1.5)), rng.uniform(-0.004, 0.004, 3))) for _ in range(V)]).reshape(V, 12)
    if dirty:
        for a in (zl, nl, zm, nm):
            bad = rng.random(a.shape) < 0.01
            a[bad] = rng.choice([np.nan, np.inf, -np.inf, 1e300, -1.0], size=int(bad.sum()))
        if V and rng.random() < 0.5:
            poses0[int(rng.integers(V)), int(rng.integers(12))] = rng.choice([np.nan, np.inf, 1e300])
    return tuple(np.ascontiguousarray(a) for a in (zl, nl, zm, nm, intr, poses0))


@functools.lru_cache(maxsize=None)
def synthetic_spec(H, W, stride, K, with_normals, V=3, seed=0):
    from omg_planner_amd import tracking
    zl, nl, zm, nm, intr, p0 = synthetic(H, W, V, seed)
    return tracking.track_cameras(zl, nl if with_normals else None, zm, nm, intr, p0, **dict(DEFAULT, stride=stride, max_passes=K))


# ---------------------------------------------------------------------------------------------------------------------
# four views that stop at different turns of one launch (step_tol = 1e-3, K = 6): every pixel invalid; a tenth of a millimetre
# from the optimum (one trial, converged); far away (K exhausted); a NaN in the pose
# ---------------------------------------------------------------------------------------------------------------------
TURNS = dict(DEFAULT, step_tol=1e-3, max_passes=6)


@functools.lru_cache(maxsize=None)
def turns():
    """(the arguments zl ... poses0 of 4 views of 32 x 48, the specification's (poses, stats))."""
    from omg_planner_amd import tracking
    zl, nl, zm, nm, intr, p0 = (a.copy() for a in synthetic(32, 48, 4, seed=5))
    zl[0], nl[0] = 0.0, 0.0
    p0[1] = rows(rigid((1.0, 0.0, 0.0), 0.0, (1e-4, 0.0, 0.0)))
    p0[2] = rows(rigid((0.3, 1.0, 0.2), np.deg2rad(4.0), (0.02, -0.015, 0.01)))
    p0[3] = rows(np.eye(4))
    p0[3, 5] = np.nan
    args = (zl, nl, zm, nm, intr, p0)
    return args, tracking.track_cameras(*args, **TURNS)


# ---------------------------------------------------------------------------------------------------------------------
# the recovery scene, built with the project's own code: a slab, a sphere and a box at 1 cm, a 120 x 160 camera with f = 150
# ---------------------------------------------------------------------------------------------------------------------
REC_H, REC_W, REC_F, REC_DELTA = 120, 160, 150.0, 0.01
REC_EYE, REC_TARGET = np.array([0.55, -0.45, 0.5]), np.array([0.0, 0.0, 0.03])
REC_ARGS = dict(stride=1, dist_max=0.05, cos_min=0.7, lambda0=2.0 ** -10, step_tol=1e-6, max_passes=30)
REC_INTRINSICS = (REC_F, REC_F, 0.5 * (REC_W - 1), 0.5 * (REC_H - 1))
REC_SEEDS = (1, 2, 3, 4, 5)  # the starts: a translation of 30 mm * u and a turn of 8 degrees * u' with u, u' uniform in [0, 1)
REC_VARIANTS = ((True, 1), (False, 2), (True, 2), (False, 1))  # (live normals?, stride)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """cam_from_world [4,4] of a camera at `eye` whose +z axis points at `target`, image rows downwards."""
    zc = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    zc /= np.linalg.norm(zc)
    xc = np.cross(zc, np.asarray(up, np.float64))
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    world_from_cam = np.eye(4)
    world_from_cam[:3, 0], world_from_cam[:3, 1], world_from_cam[:3, 2], world_from_cam[:3, 3] = xc, yc, zc, eye
    return np.linalg.inv(world_from_cam)


def scene_objects():
    """[(name, SdfGrid, world position)] of the recovery scene."""
    from omg_planner_amd import scenes
    return [("slab", scenes.box_sdf((0.30, 0.25, 0.02), (72, 60, 16), REC_DELTA), (0.0, 0.0, -0.02)),
            ("sphere", scenes.sphere_sdf(0.07, (24, 24, 24), REC_DELTA), (0.0, 0.0, 0.07)),
            ("box", scenes.box_sdf((0.04, 0.06, 0.05), (20, 24, 22), REC_DELTA), (0.17, -0.1, 0.05))]


@functools.lru_cache(maxsize=None)
def scene_table(S=1):
    """(objects, scene_begin, pool) of S copies of the scene (their volumes stored once), through volume_camera_cases.pack."""
    objs = []
    for _, g, at in scene_objects():
        pose = np.eye(4)
        pose[:3, 3] = at
        objs.append((np.asarray(g.data, np.float32), tuple(float(x) for x in g.origin), REC_DELTA, pose, 0))
    return VC.pack([objs] * S)


def render(cams_from_world, H=REC_H, W=REC_W, intrinsics=REC_INTRINSICS):
    """The specification's ray-cast of the scene at every camera -> (t [n,H,W], normals [n,H,W,3])."""
    from omg_planner_amd import camera, volume_camera as vc
    objects, begin, pool = scene_table()
    cfw = np.asarray(cams_from_world, np.float64).reshape(-1, 4, 4)
    n = len(cfw)
    cams = np.stack([camera.camera_rows(intrinsics, m) for m in cfw])
    t, _, normal, _ = vc.render_volumes(np.concatenate([objects] * n), np.arange(n + 1, dtype=np.int32) * len(objects), pool, cams, H, W,
                                        min_step=REC_DELTA / 16, max_steps=256)
    return t, normal


def moved_camera(cfw, seed):
    """(mm, degrees, cam_from_world) of the camera `cfw` moved by up to 30 mm and turned by up to 8 degrees about its own centre:
    both magnitudes uniform, both directions normal draws, from the seed."""
    rng = np.random.default_rng(seed)
    mm, degrees = 30.0 * rng.random(), 8.0 * rng.random()
    d = rng.normal(size=3)
    return mm, degrees, rigid(rng.normal(size=3), np.deg2rad(degrees), 1e-3 * mm * d / np.linalg.norm(d)) @ cfw


def camera_error(cfw, truth):
    """(distance of the camera centres in metres, angle between the orientations in degrees)."""
    a, b = np.linalg.inv(cfw), np.linalg.inv(truth)
    cosine = 0.5 * (np.trace(a[:3, :3].T @ b[:3, :3]) - 1.0)
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), float(np.rad2deg(np.arccos(np.clip(cosine, -1.0, 1.0))))


@functools.lru_cache(maxsize=None)
def recovery():
    """The model's images at the camera of the recovery scene, and per seed of REC_SEEDS the live frame (rendered at the moved
    camera; its normals by sensor.depth_normals) -> dict(cfw, zm, nm, k, starts=[dict(mm, degrees, truth, zl, nl)])."""
    from omg_planner_amd import sensor
    cfw = look_at(REC_EYE, REC_TARGET)
    moved = [moved_camera(cfw, seed) for seed in REC_SEEDS]
    t, normal = render([cfw] + [m[2] for m in moved])
    k = np.array([REC_INTRINSICS])
    starts = []
    for i, (mm, degrees, truth) in enumerate(moved):
        live = np.where(np.isfinite(t[i + 1: i + 2]), t[i + 1: i + 2], 0.0)
        nl, zl, _, _ = sensor.depth_normals(live, k, TAU, NORMAL_COS)
        starts.append(dict(mm=mm, degrees=degrees, truth=truth, zl=zl, nl=nl))
    return dict(cfw=cfw, zm=np.ascontiguousarray(t[:1]), nm=np.ascontiguousarray(normal[:1]), k=k, starts=starts)


@functools.lru_cache(maxsize=None)
def recovery_spec(i, with_normals=True, stride=1):
    """The specification's (poses, stats) of start i of the recovery scene, from identity."""
    from omg_planner_amd import tracking
    R = recovery()
    s = R["starts"][i]
    return tracking.track_cameras(s["zl"], s["nl"] if with_normals else None, R["zm"], R["nm"], R["k"], None, **dict(REC_ARGS, stride=stride))


# ---------------------------------------------------------------------------------------------------------------------
# Observation.tracked: three frames of the recovery scene rendered at their true cameras and announced with cameras 20 mm and
# 3 degrees off; the third true camera looks away from the scene, so that its frame is empty and its view is rejected
# ---------------------------------------------------------------------------------------------------------------------
ANNOUNCED_MM, ANNOUNCED_DEG = 20.0, 3.0


@functools.lru_cache(maxsize=None)
def announced():
    """dict(truth [3,4,4], announced [3,4,4], frames [3,H,W] float64 with 0.0 for no return)."""
    truth = np.stack([look_at(REC_EYE, REC_TARGET), look_at((-0.5, -0.5, 0.45), REC_TARGET), look_at(REC_EYE, 2.0 * REC_EYE)])
    off = []
    for v in range(3):
        rng = np.random.default_rng(40 + v)
        d = rng.normal(size=3)
        off.append(rigid(rng.normal(size=3), np.deg2rad(ANNOUNCED_DEG), 1e-3 * ANNOUNCED_MM * d / np.linalg.norm(d)) @ truth[v])
    t, _ = render(truth)
    return dict(truth=truth, announced=np.stack(off), frames=np.ascontiguousarray(np.where(np.isfinite(t), t, 0.0)))


# ---------------------------------------------------------------------------------------------------------------------
# the effect on a fused volume: the sphere scene of tests/fusion_cases.py (three 48 x 64 cameras), its noise-free frames announced
# with cameras 20 mm / 3 degrees off, and the scene as two volumes at 1 cm (the model the frames are tracked against)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def effect():
    """dict(truth [3,4,4], announced [3,4,4], intrinsics, frames [3,H,W] float64 with 0.0 for no return, table: (objects,
    scene_begin, pool) of three copies of the sphere and the slab)."""
    from omg_planner_amd import scenes
    from tests import fusion_cases as FC
    truth, intr = FC.scene_cameras()
    t, _ = FC.scene_depth()
    off = []
    for v in range(3):
        rng = np.random.default_rng(40 + v)
        d = rng.normal(size=3)
        off.append(rigid(rng.normal(size=3), np.deg2rad(ANNOUNCED_DEG), 1e-3 * ANNOUNCED_MM * d / np.linalg.norm(d)) @ truth[v])
    objs = []
    for g, at in ((scenes.sphere_sdf(FC.SPHERE_R, (20, 20, 20), REC_DELTA), FC.SPHERE_C), (scenes.box_sdf(tuple(FC.SLAB_HALF), (60, 60, 8), REC_DELTA), (0.0, 0.0, 0.0))):
        pose = np.eye(4)
        pose[:3, 3] = at
        objs.append((np.asarray(g.data, np.float32), tuple(float(x) for x in g.origin), REC_DELTA, pose, 0))
    return dict(truth=truth, announced=np.stack(off), intrinsics=intr, frames=np.ascontiguousarray(np.where(np.isfinite(t), t, 0.0)), table=VC.pack([objs] * 3))
