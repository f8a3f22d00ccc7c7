"""The cases the volume-camera tests share (tests/test_volume_camera_cpu.py, tests/test_gpu_volume_camera.py,
tests/fuzz/fuzz_volume_camera.py): the edges of the rule with their answers written out, a seeded random batch, the ragged batch
of the device test and the analytic sphere.  Everything is computed once per process (functools.lru_cache) and never changed."""
from __future__ import annotations

import functools

import numpy as np

_I, _N = float("inf"), float("nan")
IDENTITY_CAMERA = (1.0, 1.0, 0.0, 0.0) + (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0)


def same_bits(a, b) -> bool:
    """Equal float64 arrays bit for bit; a NaN equals a NaN (its sign and payload are the processor's, not the contract's)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan]))


def same_images(got, want) -> bool:
    """(t, inst, normal, steps) against (t, inst, normal, steps); a None in `got` is not compared."""
    return bool(same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and (got[2] is None or same_bits(got[2], want[2]))
                and (got[3] is None or np.array_equal(got[3], want[3])))


def record(dims, lo, delta, offset, pose=None, disabled=0):
    """One scenes.OBJECT_DTYPE record of a volume of `dims` samples with its min corner at `lo`, at element `offset` of the pool;
    pose [4,4]: object -> world (the record keeps the float32 rows of its inverse)."""
    from omg_planner_amd import scenes as sc
    r = np.zeros(1, sc.OBJECT_DTYPE)
    inv = np.eye(4) if pose is None else np.linalg.inv(np.asarray(pose, np.float64))
    r["pose_inv"][0] = inv[:3].ravel()
    r["lo"][0], r["dim"][0], r["delta"][0] = lo, dims, delta
    r["hi"][0] = np.asarray(lo, np.float64) + float(delta) * np.asarray(dims)
    r["epsilon"], r["padding_scale"], r["clearance"], r["disabled"], r["grid_offset"] = 0.2, 1.0, 0.01, disabled, offset
    return sc.finish_records(r)[0]


def pack(scenes, gap=3, fill=-7.5, shuffle=None):
    """scenes: [[(data [X,Y,Z] float32, lo, delta, pose or None, disabled)]] -> (objects, scene_begin int32 [S+1], pool).  A
    volume given twice (the same ndarray) is stored once; `gap` guard elements of `fill` lie before, between and behind the
    volumes; shuffle: the order of the distinct volumes in the pool."""
    distinct, seen = [], {}
    for objs in scenes:
        for data, *_ in objs:
            if id(data) not in seen:
                seen[id(data)] = len(distinct)
                distinct.append(data)
    order = list(range(len(distinct))) if shuffle is None else list(shuffle)
    offsets, at = {}, gap
    for v in order:
        offsets[v] = at
        at += distinct[v].size + gap
    pool = np.full(at, fill, np.float32)
    for v, data in enumerate(distinct):
        pool[offsets[v]: offsets[v] + data.size] = np.ascontiguousarray(data, np.float32).ravel()
    recs, begin = [], [0]
    for objs in scenes:
        for data, lo, delta, pose, disabled in objs:
            recs.append(record(data.shape, lo, delta, offsets[seen[id(data)]], pose, disabled))
        begin.append(len(recs))
    from omg_planner_amd import scenes as sc
    return (np.array(recs, sc.OBJECT_DTYPE) if recs else np.zeros(0, sc.OBJECT_DTYPE)), np.array(begin, np.int32), pool


# ---------------------------------------------------------------------------------------------------------------------
# The edges of the rule.  Every scene is seen by a 1 x 1 image through the identity camera (fx = fy = 1, cx = cy = 0, world frame =
# camera frame) unless said otherwise: the ray of the pixel is the +z axis.  Volumes have delta = 1 and values that depend on z
# only unless said otherwise, data[x, y, k] = zv[k], 3 x 3 samples across; with lo = (-1.5, -1.5, lz) the ray runs along the
# middle column (u_x = u_y = 1, ud_x = ud_y = 0: a ray along an axis, inside the slab), u_z = t - lz - 0.5: it enters the box at
# t0 = lz + 0.5 and leaves at t1 = t0 + len(zv) - 1, and nrm = 1.  min_step = 0.25 everywhere.  Every number below is exact in
# binary.  An answer is (t, inst, steps, normal).
# ---------------------------------------------------------------------------------------------------------------------
def zvol(zv, across=(3, 3), xv=None):
    zv = np.asarray(zv, np.float32)
    data = np.broadcast_to(zv, across + (len(zv),)).copy()
    if xv is not None:
        data += np.asarray(xv, np.float32)[:, None, None]
    return np.ascontiguousarray(data, np.float32)


_LINE = zvol([3, 2, 1, 0, -1])          # slope -1: from v = 3 at t0 one step of 3 lands on the sample that holds 0
_MID, _Z = (-1.5, -1.5), 1.5            # lo of the 3 x 3 volumes: the box is entered at t0 = 2
_BACK, _DOWN = (_I, -1, 0, (0.0, 0.0, 0.0)), (0.0, 0.0, -1.0)
_R125 = float(np.sqrt(1.25))
DEFAULT = dict(level=0.0, t_min=0.0, min_step=0.25, relax=1.0, max_steps=64)
_NAN_LINE = zvol([1, _N, 1, 1, -1])
_PINF_LINE = zvol([1, _I, 1, 1, -1])
_NINF_LINE = zvol([1, 1, -_I, 1, -1])
_RELAX_LINE = zvol([4, 3, 2, 1, 0, -1, -2])

# (what it is about, the scene's objects [(data, lo, delta, pose, disabled)], visible flags or None, camera or None, arguments
#  that differ from DEFAULT, the answer)
EDGE_CASES = (
    # t0 = 2: v = 1, s = 1, tn = 3 = t1, vn = -1: th = 2 + 1 * (1 / 2)
    ("a 2 x 2 x 2 volume (dim - 2 == 0)", [(zvol([1, -1], (2, 2)), (-1.0, -1.0, _Z), 1.0, None, 0)], None, None, {}, (2.5, 0, 2, _DOWN)),
    # v = 3 at t0 = 2, tn = 5, vn = 0 == level: th = 2 + 3 * (3 / 3)
    ("a crossing exactly at a sample (vn == level)", [(_LINE, _MID + (_Z,), 1.0, None, 0)], None, None, {}, (5.0, 0, 2, _DOWN)),
    # uo_x = (0 - 0.5) - 0.5 = -1 with ud_x == 0
    ("a ray along an axis, outside the slab", [(_LINE, (0.5, -1.5, _Z), 1.0, None, 0)], None, None, {}, _BACK),
    # uo_x = 2 = hi_x with ud_x == 0 is inside; i_x = min(2, 1) = 1, f_x = 1.0 reads the plane x = 2, which holds zv + 0.5:
    # v = 2.5 at t0, tn = 4.5, vn = (-0.5) + 0.5 = 0: th = 4.5; g = (0.5, 0, -1)
    ("a far-face sample with f == 1.0 across the ray", [(zvol([2, 1, 0, -1, -2], xv=[0, 0, 0.5]), (-2.5, -1.5, _Z), 1.0, None, 0)], None, None, {},
     (4.5, 0, 2, (0.5 / _R125, 0.0, -1.0 / _R125))),
    # t = 2: v = 1; tn = 3: v = 1; tn = 4 = t1: i_z = min(2, 1) = 1, f_z = 1.0 reads zv[2] = -1: th = 3 + 1 * (1 / 2)
    ("a far-face sample with f == 1.0 along the ray", [(zvol([1, 1, -1]), _MID + (_Z,), 1.0, None, 0)], None, None, {}, (3.5, 0, 3, _DOWN)),
    # cx = 1: dx = -1, the ray (-t, 0, t).  uo_x = 2: the x slab is [0, 2], the z slab [2, 6]: t0 == t1 == 2 at the corner
    # (u_x, u_z) = (0, 0), where v = 3 > level: the second sample is the same point, tn >= t1: a miss after two samples
    ("a ray that enters at a corner (t0 == t1)", [(_LINE, (-2.5, -1.5, _Z), 1.0, None, 0)], None, (1.0, 1.0, 1.0, 0.0) + IDENTITY_CAMERA[4:], {},
     (_I, -1, 2, (0.0, 0.0, 0.0))),
    # without t_min the ray would hit at t0 = 2 (v = -1).  t0 = 3.5: u_z = 1.5, v = 2 + 0.5 * (1 - 2) = 1.5; tn = 5: vn = -1.5:
    # th = 3.5 + 1.5 * (1.5 / 3)
    ("t_min inside the box", [(zvol([-1, 2, 1, -1.5, -2]), _MID + (_Z,), 1.0, None, 0)], None, None, dict(t_min=3.5), (4.25, 0, 2, _DOWN)),
    # lo_z = -1.5: uo_z = 1, the z slab is [-1, 2]; t0 = t_min = 0: v = zv[1] = -1 <= level
    ("a ray that starts inside the surface (hit at t0)", [(zvol([1, -1, -2, -3]), _MID + (-1.5,), 1.0, None, 0)], None, None, {}, (0.0, 0, 1, _DOWN)),
    # level = 0.5: v = 2.5, s = 2, tn = 4: vn = -1.5: th = 2 + 2 * (2 / 4)
    ("level != 0", [(zvol([2.5, 1, -1.5, -2]), _MID + (_Z,), 1.0, None, 0)], None, None, dict(level=0.5), (3.0, 0, 2, _DOWN)),
    # relax = 0.5 on slope -1: v = 4, 2, 1, 0.5, 0.25 at t = 2, 4, 5, 5.5, 5.75; then s = 0.125 < min_step: tn = 6, vn = 0: six samples
    ("relax < 1 (and min_step takes over)", [(_RELAX_LINE, _MID + (_Z,), 1.0, None, 0)], None, None, dict(relax=0.5), (6.0, 0, 6, _DOWN)),
    # the same with two steps: t = 2, 4, 5 and no crossing
    ("max_steps reached: a miss, steps == max_steps + 1", [(_RELAX_LINE, _MID + (_Z,), 1.0, None, 0)], None, None, dict(relax=0.5, max_steps=2),
     (_I, -1, 3, (0.0, 0.0, 0.0))),
    # A cell with a NaN corner gives NaN (0 * NaN): cells 0 and 1.  s = NaN: min_step.  t = 2, 2.25 ... 4 (nine samples), at
    # t = 4 (u_z = 2) v = 1; tn = 5: 1; tn = 6 = t1: -1: th = 5 + 1 * (1 / 2)
    ("a NaN voxel on the ray's way", [(_NAN_LINE, _MID + (_Z,), 1.0, None, 0)], None, None, {}, (5.5, 0, 11, _DOWN)),
    # +inf instead: 1 + 0 * inf and inf - inf are NaN as well: the same walk
    ("a +inf voxel on the ray's way", [(_PINF_LINE, _MID + (_Z,), 1.0, None, 0)], None, None, {}, (5.5, 0, 11, _DOWN)),
    # cell 0 is clean: v = 1 at t = 2, tn = 3; cells 1 and 2 give NaN (the lerps across the ray subtract -inf from -inf), never a
    # hit: t = 3, 3.25 ... 5 (nine samples), at t = 5 (u_z = 3) v = 1; tn = 6 = t1: -1
    ("a -inf voxel on the ray's way", [(_NINF_LINE, _MID + (_Z,), 1.0, None, 0)], None, None, {}, (5.5, 0, 11, _DOWN)),
    ("two visible objects with the same volume and pose: the lower index", [(_LINE, _MID + (_Z,), 1.0, None, 0), (_LINE, _MID + (_Z,), 1.0, None, 0)],
     None, None, {}, (5.0, 0, 4, _DOWN)),
    # the far one enters at t0 = 5: th = 8; it keeps its index in the scene
    ("an invisible object in front of a visible one", [(_LINE, _MID + (_Z,), 1.0, None, 0), (_LINE, _MID + (4.5,), 1.0, None, 0)], (0, 1), None, {},
     (8.0, 1, 2, _DOWN)),
    ("a disabled object is drawn", [(_LINE, _MID + (_Z,), 1.0, None, 1)], None, None, {}, (5.0, 0, 2, _DOWN)),
    ("a scene with no objects", [], None, None, {}, _BACK),
)


def edge_groups():
    """The edge cases grouped by their arguments -> [(arguments, [case index])]: one launch per group."""
    groups = {}
    for k, case in enumerate(EDGE_CASES):
        groups.setdefault(tuple(sorted({**DEFAULT, **case[4]}.items())), []).append(k)
    return [(dict(key), idx) for key, idx in groups.items()]


def edge_batch(idx):
    """The cases `idx` as the scenes of one table -> (objects, scene_begin, pool, cameras [S,16], visible uint8, answers)."""
    cases = [EDGE_CASES[k] for k in idx]
    objects, begin, pool = pack([c[1] for c in cases])
    visible = np.concatenate([np.ones(len(c[1]), np.uint8) if c[2] is None else np.array(c[2], np.uint8) for c in cases] + [np.zeros(0, np.uint8)])
    cameras = np.array([IDENTITY_CAMERA if c[3] is None else c[3] for c in cases], np.float64)
    return objects, begin, pool, cameras, visible, [c[5] for c in cases]


def edge_check(idx, t, inst, normal, steps):
    """Assert the images [S,1,1] of edge_batch(idx) against the written answers."""
    for s, k in enumerate(idx):
        what, want = EDGE_CASES[k][0], EDGE_CASES[k][5]
        got = (float(t[s, 0, 0]), int(inst[s, 0, 0]), int(steps[s, 0, 0]), tuple(float(x) for x in normal[s, 0, 0]))
        assert got == want, (what, got, want)


# ---------------------------------------------------------------------------------------------------------------------
# random batches
# ---------------------------------------------------------------------------------------------------------------------
def random_pose(rng, reach=0.05):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    P = np.eye(4)
    P[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    P[:3, 3] = rng.uniform(-reach, reach, 3)
    return P


def random_volume(rng, dims, delta, finite=False):
    """A float32 volume whose zero set is a wobbly sphere inside the grid, sometimes with a few voxels that are not finite."""
    ax = [(np.arange(d) + 0.5 - 0.5 * d) * delta for d in dims]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    r = 0.3 * delta * min(dims)
    data = np.sqrt(x * x + y * y + z * z) - r + 0.2 * delta * rng.normal(size=dims)
    if not finite and rng.random() < 0.3:
        bad = rng.random(dims) < 0.02
        data[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    return np.ascontiguousarray(data, np.float32), tuple(-0.5 * delta * d for d in dims)


def random_table(rng, S, max_objects=3, dims_choice=((5, 9, 7), (2, 2, 2), (8, 6, 11), (16, 16, 16), (3, 2, 4))):
    """S scenes of 0 .. max_objects objects with random rigid poses (some volumes shared), cameras inside and outside the boxes
    -> (objects, scene_begin, pool, cameras [S,16], visible uint8)."""
    from omg_planner_amd import camera
    made, scenes, cams = [], [], []
    for s in range(S):
        objs = []
        for _ in range(int(rng.integers(0, max_objects + 1))):
            if made and rng.random() < 0.3:
                data, lo, delta = made[int(rng.integers(len(made)))]
            else:
                dims = dims_choice[int(rng.integers(len(dims_choice)))]
                delta = float(rng.choice([0.01, 0.0125, 0.02])) * 16.0 / max(dims)  # every volume about 0.2 m on its longest side
                data, lo = random_volume(rng, dims, delta)
                made.append((data, lo, delta))
            objs.append((data, lo, delta, random_pose(rng), int(rng.random() < 0.2)))
        scenes.append(objs)
        inside = rng.random() < 0.25
        eye = rng.uniform(-0.03, 0.03, 3) if inside else np.array([0.0, 0.0, -0.3]) + rng.uniform(-0.03, 0.03, 3)
        cfw = np.linalg.inv(random_pose(rng, 0.0)) if inside else np.eye(4)
        world_from_cam = np.linalg.inv(cfw)
        world_from_cam[:3, 3] = eye
        f = float(rng.uniform(12.0, 30.0))
        cams.append(camera.camera_rows((f, f * 1.1, rng.uniform(5.0, 9.0), rng.uniform(4.0, 7.0)), np.linalg.inv(world_from_cam)))
    objects, begin, pool = pack(scenes, shuffle=list(rng.permutation(len(made))) if made else None)
    visible = (rng.random(len(objects)) < 0.8).astype(np.uint8)
    return objects, begin, pool, np.array(cams, np.float64).reshape(S, 16), visible


@functools.lru_cache(maxsize=None)
def random_batch():
    """The seeded batch of the CPU test: 6 scenes at 11 x 13 -> (table..., arguments, the specification's images)."""
    from omg_planner_amd import volume_camera as vc
    table = random_table(np.random.default_rng(2024), 6)
    args = dict(level=0.001, t_min=1e-6, min_step=0.002, relax=0.9, max_steps=48)
    return table, args, vc.render_volumes(*table[:4], 11, 13, visible=table[4], **args)


# ---------------------------------------------------------------------------------------------------------------------
# the ragged batch of the device test: S = 3 scenes with 0, 1 and 3 objects, volumes of (2,2,2), (5,9,7) and (16,16,16), two
# objects sharing one volume, pool offsets neither zero nor in order, a 17 x 33 image, one camera inside a volume
# ---------------------------------------------------------------------------------------------------------------------
RAGGED_H, RAGGED_W = 17, 33
RAGGED_ARGS = dict(level=0.0, t_min=1e-6, min_step=0.001, relax=1.0, max_steps=96)


@functools.lru_cache(maxsize=None)
def ragged_batch():
    from omg_planner_amd import camera, volume_camera as vc
    rng = np.random.default_rng(7)
    small, lo_s = random_volume(rng, (2, 2, 2), 0.05, True)
    small[:] = np.float32(0.01) - np.float32(0.05) * (np.arange(2, dtype=np.float32)[None, None, :])  # crosses zero along z
    mid, lo_m = random_volume(np.random.default_rng(8), (5, 9, 7), 0.02, True)
    big, lo_b = random_volume(np.random.default_rng(9), (16, 16, 16), 0.0125, True)
    at = lambda x, y, z: np.array([[1.0, 0, 0, x], [0, 1.0, 0, y], [0, 0, 1.0, z], [0, 0, 0, 1.0]])
    yaw = random_pose(np.random.default_rng(10), 0.0)
    yaw[:3, 3] = (0.09, 0.02, 0.0)
    scenes = [[], [(big, lo_b, 0.0125, at(0.0, 0.0, 0.0), 0)],
              # the mid volume twice (one copy turned and to the right, small on the image: the waves beside it see nothing), the 2^3 in front
              [(mid, lo_m, 0.02, at(-0.06, 0.0, 0.0), 0), (small, lo_s, 0.05, at(-0.06, 0.0, -0.15), 1), (mid, lo_m, 0.02, yaw, 0)]]
    objects, begin, pool = pack(scenes, shuffle=[1, 2, 0])
    assert begin.tolist() == [0, 0, 1, 4] and objects["grid_offset"].min() > 0 and len(set(np.sign(np.diff(objects["grid_offset"])))) > 1
    outside = np.eye(4)
    outside[:3, 3] = (0.0, 0.0, 0.45)  # cam_from_world: the camera stands at z = -0.45 and looks along +z
    inside = np.eye(4)
    inside[:3, 3] = (0.0, 0.0, 0.085)
    cams = np.stack([camera.camera_rows((40.0, 40.0, 16.0, 8.0), outside), camera.camera_rows((12.0, 12.0, 16.0, 8.0), inside),  # inside the box of `big`, before its surface
                     camera.camera_rows((30.0, 30.0, 20.0, 8.0), outside)])
    want = vc.render_volumes(objects, begin, pool, cams, RAGGED_H, RAGGED_W, **RAGGED_ARGS)
    return objects, begin, pool, cams, want


# ---------------------------------------------------------------------------------------------------------------------
# the analytic sphere: |x| - R on n^3 samples over a 0.32 m cube, a 48 x 64 camera with f = 60 at (0.02, -0.01, -0.6) looking along +z
# ---------------------------------------------------------------------------------------------------------------------
SPHERE_R, SPHERE_SIDE, SPHERE_EYE, SPHERE_F = 0.1, 0.32, np.array([0.02, -0.01, -0.6]), 60.0


@functools.lru_cache(maxsize=None)
def sphere_table(n):
    """(objects, scene_begin, pool, delta) of the n^3 sphere at the origin of the world."""
    delta = SPHERE_SIDE / n
    ax = (np.arange(n) + 0.5) * delta - 0.5 * SPHERE_SIDE
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    data = (np.sqrt(x * x + y * y + z * z) - SPHERE_R).astype(np.float32)
    return pack([[(data, (-0.5 * SPHERE_SIDE,) * 3, delta, None, 0)]], gap=0) + (delta,)


def sphere_camera(H, W):
    """camera rows [1,16] of the H x W camera (principal point at the image centre) and cam_from_world."""
    from omg_planner_amd import camera
    cfw = np.eye(4)
    cfw[:3, 3] = -SPHERE_EYE
    return camera.camera_rows((SPHERE_F * W / 64.0, SPHERE_F * W / 64.0, 0.5 * (W - 1), 0.5 * (H - 1)), cfw)[None], cfw


def sphere_analytic(cam, H, W):
    """The analytic ray-sphere answer per pixel -> (hit, t along the axis, normal [H,W,3] camera frame, cosine of incidence,
    closest approach of the ray to the centre)."""
    from omg_planner_amd import camera
    dx, dy = camera.pixel_directions(cam, H, W)
    d = np.stack([dx, dy, np.ones_like(dx)], -1)
    o = SPHERE_EYE  # (world frame = camera frame up to the translation)
    a, b, c = (d * d).sum(-1), (d * o).sum(-1), (o * o).sum() - SPHERE_R ** 2
    disc = b * b - a * c
    hit = disc > 0
    t = np.where(hit, (-b - np.sqrt(np.maximum(disc, 0.0))) / a, np.inf)
    p = o + t[:, None] * d
    nrm = np.where(hit[:, None], p / SPHERE_R, 0.0)
    cos = np.where(hit, -(nrm * d).sum(-1) / np.sqrt(a), 0.0)
    closest = np.sqrt(np.maximum((o * o).sum() - b * b / a, 0.0))
    sh = (H, W)
    return hit.reshape(sh), t.reshape(sh), nrm.reshape(sh + (3,)), cos.reshape(sh), closest.reshape(sh)


@functools.lru_cache(maxsize=None)
def sphere_render(n, H, W):
    """The specification's images of the n^3 sphere with min_step = delta / 16, max_steps = 256, relax = 1."""
    from omg_planner_amd import volume_camera as vc
    objects, begin, pool, delta = sphere_table(n)
    cam, _ = sphere_camera(H, W)
    return vc.render_volumes(objects, begin, pool, cam, H, W, min_step=delta / 16, max_steps=256, relax=1.0)
