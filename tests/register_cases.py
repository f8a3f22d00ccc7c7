"""Cases of the registration tests (test_register_cpu.py, test_gpu_register.py, fuzz/fuzz_register.py): volumes, clouds, poses
and the calls built from them.  A call is a dict of register_clouds' arguments; `spec(name)` is the specification's answer,
computed once and shared."""
from __future__ import annotations

import functools

import numpy as np

BOX_HALF = (0.06, 0.04, 0.09)
ELL_RADII = (0.07, 0.045, 0.09)
SPHERE_R = 0.06
DEFAULTS = dict(stride=1, trunc=0.03, lambda0=2.0 ** -10, step_tol=1e-6, max_passes=30)


# ---------------------------------------------------------------------------------------------------------------------
# volumes, records, surfaces, poses
# ---------------------------------------------------------------------------------------------------------------------
def centred_grid(dims, delta):
    """Voxel-centre coordinates of a grid centred on the origin -> (origin [3], x, y, z [dims])."""
    dims = tuple(int(d) for d in dims)
    origin = -0.5 * delta * np.array(dims, np.float64)
    ax = [origin[a] + (np.arange(dims[a]) + 0.5) * delta for a in range(3)]
    return (origin, *np.meshgrid(*ax, indexing="ij"))


def ellipsoid_distance(p, radii):
    """A first-order distance to the ellipsoid's surface (exact on it, good within a few voxels): k0 (k0 - 1) / k1 with
    k0 = |p / r|, k1 = |p / r^2|."""
    p, r = np.asarray(p, np.float64), np.asarray(radii, np.float64)
    k0 = np.sqrt(((p / r) ** 2).sum(-1))
    k1 = np.sqrt(((p / (r * r)) ** 2).sum(-1))
    return k0 * (k0 - 1.0) / np.maximum(k1, 1e-12)


def box_distance(p, half):
    q = np.abs(np.asarray(p, np.float64)) - np.asarray(half, np.float64)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def volume(kind, dims, delta):
    """-> scenes.SdfGrid of a box, an ellipsoid or a sphere centred in a grid of `dims` voxels."""
    from omg_planner_amd import scenes as S
    dims = tuple(int(d) for d in dims)
    if kind == "box":
        return S.box_sdf(BOX_HALF, dims, delta)
    origin, x, y, z = centred_grid(dims, delta)
    p = np.stack([x, y, z], -1)
    d = ellipsoid_distance(p, ELL_RADII) if kind == "ellipsoid" else np.sqrt((p * p).sum(-1)) - SPHERE_R
    return S.SdfGrid(d.astype(np.float32), origin, float(delta))


def table(grids, gaps=(0,)):
    """Object records and a ragged pool for a list of SdfGrid; gaps[i % len]: unused floats (NaN) in front of grid i."""
    from omg_planner_amd import scenes as S
    rec = np.zeros(len(grids), S.OBJECT_DTYPE)
    chunks, off = [], 0
    for i, g in enumerate(grids):
        gap = int(gaps[i % len(gaps)])
        chunks.append(np.full(gap, np.nan, np.float32))
        off += gap
        rec["pose_inv"][i] = np.eye(4, dtype=np.float32)[:3].ravel()
        rec["lo"][i] = g.min_coords.astype(np.float32)
        rec["hi"][i] = g.max_coords.astype(np.float32)
        rec["dim"][i] = g.data.shape
        rec["delta"][i] = g.delta
        rec["epsilon"][i], rec["padding_scale"][i], rec["clearance"][i] = 0.2, 1.0, 0.01
        rec["grid_offset"][i] = off
        chunks.append(np.ascontiguousarray(g.data, np.float32).reshape(-1))
        off += g.data.size
    S.finish_records(rec)
    return rec, np.concatenate(chunks)


def surface(kind, n, rng, faces=None):
    """n points on the surface in the object's frame.  Box: area-uniform over `faces` (0..5 = -x, +x, -y, +y, -z, +z; default
    all six)."""
    if kind == "box":
        h = np.array(BOX_HALF)
        faces = list(range(6)) if faces is None else list(faces)
        area = np.array([4 * h[(f // 2 + 1) % 3] * h[(f // 2 + 2) % 3] for f in faces])
        pick = rng.choice(len(faces), n, p=area / area.sum())
        p = rng.uniform(-1.0, 1.0, (n, 3)) * h
        for k, f in enumerate(faces):
            p[pick == k, f // 2] = h[f // 2] * (1.0 if f % 2 else -1.0)
        return p
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (np.array(ELL_RADII) if kind == "ellipsoid" else SPHERE_R)


def surface_distance(kind, p):
    """|distance| of object-frame points to the true surface."""
    if kind == "box":
        return np.abs(box_distance(p, BOX_HALF))
    if kind == "sphere":
        return np.abs(np.linalg.norm(p, axis=-1) - SPHERE_R)
    return np.abs(ellipsoid_distance(p, ELL_RADII))


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def random_pose(rng, spread=0.5):
    P = np.eye(4)
    P[:3, :3] = rotation(rng.normal(size=3), rng.uniform(0, np.pi))
    P[:3, 3] = rng.uniform(-spread, spread, 3)
    return P


def perturbed(P, rng, dist=0.02, angle=np.deg2rad(10.0)):
    """A start `dist` metres and `angle` radians away from P."""
    d = rng.normal(size=3)
    Q = P.copy()
    Q[:3, :3] = P[:3, :3] @ rotation(rng.normal(size=3), angle)
    Q[:3, 3] = P[:3, 3] + dist * d / np.linalg.norm(d)
    return Q


def rows(P):
    return np.asarray(P, np.float64).reshape(-1, 4, 4)[:, :3, :].reshape(-1, 12)


def to_object(row, pts):
    P = np.asarray(row, np.float64).reshape(3, 4)
    return (np.asarray(pts) - P[:, 3]) @ P[:, :3]


def to_world(P, pts):
    return np.asarray(pts) @ P[:3, :3].T + P[:3, 3]


# ---------------------------------------------------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------------------------------------------------
def _call(grids, obj_index, poses0, clouds, ranges=None, gaps=(0,), **kw):
    """clouds: a list of [n,3] world-frame arrays, packed in order; ranges default to one cloud per instance."""
    rec, pool = table(grids, gaps)
    begin = np.cumsum([0] + [len(c) for c in clouds])
    if ranges is None:
        ranges = np.stack([begin[:-1], begin[1:]], -1)
    c = dict(DEFAULTS, objects=rec, pool=pool, obj_index=np.asarray(obj_index, np.int32), poses0=rows(poses0),
             points=np.ascontiguousarray(np.concatenate(clouds) if clouds else np.zeros((0, 3))), ranges=np.asarray(ranges, np.int32).reshape(-1, 2))
    c.update(kw)
    return c


RECOVERY = [(kind, grid, delta, n) for kind in ("box", "ellipsoid") for grid, delta in ((16, 0.02), (24, 0.0125)) for n in (257, 600)]


def recovery(kind, grid, delta, n, seed=0, count=4):
    """`count` random true poses of one volume, full-surface clouds of n points, starts 20 mm / 10 degrees away."""
    rng = np.random.default_rng([seed, grid, n])
    g = volume(kind, (grid,) * 3, delta)
    truth = [random_pose(rng) for _ in range(count)]
    clouds = [to_world(P, surface(kind, n, rng)) for P in truth]
    c = _call([g], [0] * count, [perturbed(P, rng) for P in truth], clouds)
    c.update(kind=kind, truth=np.stack(truth), delta=delta)
    return c


def _one(kind, dims, delta, n, seed, faces=None, **kw):
    rng = np.random.default_rng(seed)
    g = volume(kind, dims, delta)
    P = random_pose(rng)
    cloud = to_world(P, surface(kind, n, rng, faces) if kind == "box" else surface(kind, n, rng))
    start = perturbed(P, rng, kw.pop("dist", 0.02), kw.pop("angle", np.deg2rad(10.0)))
    c = _call([g], [0], [start], [cloud], **kw)
    c.update(kind=kind, truth=P[None], delta=delta)
    return c


def _special(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "reject_accept":   # a far start with almost no damping: a trial overshoots and is rejected, later ones are accepted
        return _one("box", (16,) * 3, 0.02, 300, 11, lambda0=2.0 ** -20, dist=0.035, angle=np.deg2rad(25.0))
    if name == "small_trunc":     # trunc below the start's distance: the inlier set grows from pass to pass
        return _one("box", (24,) * 3, 0.0125, 400, 12, trunc=0.012)
    if name == "sphere":          # rotations are unobservable: the normal matrix is singular without the floor
        return _one("sphere", (16,) * 3, 0.02, 300, 13)
    if name == "one_face":        # the +x face, identity rotation: g = (1, 0, 0) exactly, three diagonal entries of H are exactly 0
        g = volume("box", (16,) * 3, 0.02)
        pts = surface("box", 200, rng, faces=[1]) * np.array([1.0, 0.7, 0.75])  # every cell touched lies wholly in the face's region
        start = np.eye(4)
        start[0, 3] = -0.004
        c = _call([g], [0], [start], [pts])
        c.update(kind="box", truth=np.eye(4)[None], delta=0.02)
        return c
    if name == "all_outside":
        g = volume("box", (16,) * 3, 0.02)
        return _call([g], [0], [random_pose(rng)], [rng.uniform(5.0, 6.0, (300, 3))])
    if name == "few_inliers":     # five points on the surface, the rest far away
        c = _one("box", (16,) * 3, 0.02, 5, 14, dist=0.002, angle=0.01)
        c["points"] = np.concatenate([c["points"], rng.uniform(5.0, 6.0, (40, 3))])
        c["ranges"] = np.array([[0, 45]], np.int32)
        return c
    if name == "not_finite":      # NaN, +-inf and 1e300 among good points
        c = _one("ellipsoid", (16,) * 3, 0.02, 300, 15)
        bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e300, 1e300, 1e300], [-1e300, 0, np.nan], [np.inf, -np.inf, np.nan]])
        c["points"][rng.choice(300, len(bad), replace=False)] = bad
        return c
    if name == "ragged":          # a non-cubic grid at a non-zero offset, between two other volumes, with unused floats between
        rng2 = np.random.default_rng(16)
        grids = [volume("box", (16,) * 3, 0.02), volume("ellipsoid", (8, 9, 10), 0.03), volume("sphere", (12, 10, 11), 0.02)]
        P = random_pose(rng2)
        cloud = to_world(P, surface("ellipsoid", 350, rng2))
        c = _call(grids, [1], [perturbed(P, rng2, 0.01, np.deg2rad(5.0))], [cloud], gaps=(3, 5, 1))
        c.update(kind="ellipsoid", truth=P[None], delta=0.03)
        return c
    if name == "shared_range":    # one cloud from two starts: a near one and a far one; and a third instance with its own range
        rng2 = np.random.default_rng(17)
        g = volume("box", (16,) * 3, 0.02)
        P = random_pose(rng2)
        cloud = to_world(P, surface("box", 300, rng2))
        starts = [perturbed(P, rng2, 0.05, np.deg2rad(40.0)), perturbed(P, rng2, 0.01, np.deg2rad(5.0)), perturbed(P, rng2)]
        c = _call([g], [0, 0, 0], starts, [cloud], ranges=[[0, 300], [0, 300], [100, 300]])
        c.update(kind="box", truth=np.stack([P] * 3), delta=0.02)
        return c
    if name == "empty_range":
        c = _one("box", (16,) * 3, 0.02, 100, 18)
        c["ranges"] = np.array([[37, 37]], np.int32)
        return c
    if name == "stride3":
        return _one("ellipsoid", (24,) * 3, 0.0125, 900, 19, stride=3)
    if name == "k0":
        return _one("box", (16,) * 3, 0.02, 300, 20, max_passes=0)
    raise KeyError(name)


SPECIAL = ["reject_accept", "small_trunc", "sphere", "one_face", "all_outside", "few_inliers", "not_finite", "ragged", "shared_range", "empty_range",
           "stride3", "k0"]
ALL = [f"{k}{g}_{n}" for k, g, _, n in RECOVERY] + SPECIAL


@functools.lru_cache(maxsize=None)
def call(name):
    for k, g, d, n in RECOVERY:
        if name == f"{k}{g}_{n}":
            return recovery(k, g, d, n)
    return _special(name)


ARGS = ("objects", "pool", "obj_index", "poses0", "points", "ranges", "stride", "trunc", "lambda0", "step_tol", "max_passes")


def args(c):
    return [c[k] for k in ARGS]


@functools.lru_cache(maxsize=None)
def spec(name):
    from omg_planner_amd import registration as reg
    poses, stats = reg.register_clouds(*args(call(name)))
    poses.setflags(write=False), stats.setflags(write=False)
    return poses, stats


def history(c, m=0):
    """The specification's loop for instance m with every trial recorded -> [(accepted, cost, count)] (pass 0 first)."""
    from omg_planner_amd import registration as reg
    out = []
    pts = c["points"][c["ranges"][m, 0]: c["ranges"][m, 1]: c["stride"]]
    orig = reg.one_pass

    def spy(*a):
        r = orig(*a)
        out.append(r[:2])
        return r
    reg.one_pass = spy
    try:
        reg.register_clouds(c["objects"], c["pool"], c["obj_index"][m: m + 1], c["poses0"][m: m + 1], pts, [[0, len(pts)]], 1, c["trunc"],
                            c["lambda0"], c["step_tol"], c["max_passes"])
    finally:
        reg.one_pass = orig
    return out


def lengths_call(K, stride, lengths=(0, 1, 5, 6, 63, 64, 65, 255, 256, 257, 513, 1025)):
    """One instance per range length, all ranges inside one cloud around one pose (the lengths are numbers of USED points:
    the range is stride times as long, less a remainder)."""
    rng = np.random.default_rng([K, stride])
    g = volume("ellipsoid", (16,) * 3, 0.02)
    P = random_pose(rng)
    total = max(lengths) * stride + 40
    cloud = to_world(P, surface("ellipsoid", total, rng))
    ranges = []
    for k, n in enumerate(lengths):
        b = int(rng.integers(0, total - n * stride + 1))
        e = b + (0 if n == 0 else (n - 1) * stride + 1 + int(rng.integers(0, stride)))
        ranges.append((b, min(e, total)))
    starts = [perturbed(P, rng, 0.01, np.deg2rad(6.0)) for _ in lengths]
    return _call([g], [0] * len(lengths), starts, [cloud], ranges=ranges, stride=stride, max_passes=K)


# ---------------------------------------------------------------------------------------------------------------------
# end to end at toy size: meshes -> volumes -> depth images -> clouds -> poses, all by the specifications
# ---------------------------------------------------------------------------------------------------------------------
TOY_H, TOY_W, TOY_INTR, TOY_DELTA = 40, 48, (80.0, 80.0, 23.5, 19.5), 0.01
TOY_MIN_INLIERS = 30


def toy_meshes():
    """A 12-face box and an 80-face ellipsoid."""
    from tests import mesh_cases as MC
    v, f = MC.icosphere(1, 1.0)
    return [MC.box_mesh(BOX_HALF), (v * np.array(ELL_RADII), f)]


def toy_layout():
    """Two scenes of (box, ellipsoid) seen by one tilted camera above them -> (cam_from_world [4,4], truth [2,2,4,4], starts
    [2,2,4,4]): object -> world poses."""
    from tests import mesh_cases as MC
    world_from_cam = np.eye(4)
    world_from_cam[:3, :3] = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]]) @ MC.pose((0.12, -0.08, 0.05))[:3, :3]
    world_from_cam[:3, 3] = (0.47, 0.0, 0.95)
    rng = np.random.default_rng(5)
    truth = np.zeros((2, 2, 4, 4))
    for s in range(2):
        truth[s, 0] = MC.pose(rng.normal(size=3) * 0.5, (0.36 + 0.01 * s, 0.02, 0.35))
        truth[s, 1] = MC.pose(rng.normal(size=3) * 0.5, (0.58, -0.03 + 0.02 * s, 0.33))
    starts = np.stack([np.stack([perturbed(truth[s, o], rng) for o in range(2)]) for s in range(2)])
    return np.linalg.inv(world_from_cam), truth, starts


@functools.lru_cache(maxsize=None)
def toy():
    """-> dict: meshes, grids (SdfGrid), cam_from_world, truth, instances / inst_begin / cameras (camera.py records), clouds
    {(scene, obj): [n,3]}, and `call`: register_clouds' arguments for the instances
      0..3: (scene 0, box), (scene 1, box), (scene 0, ellipsoid), (scene 1, ellipsoid), each on its own cloud from a start 20 mm /
            10 degrees away (class-major, as two ops.pixel_clouds calls pack the points);
      4:    (scene 0, box) again from a far start on the same range;   5: (scene 1, ellipsoid) again on an empty range
    with `pairs` [6,2]."""
    from omg_planner_amd import camera as cam, scenes as S
    meshes = toy_meshes()
    grids = [S.mesh_sdf(v, f, TOY_DELTA, padding=4) for v, f in meshes]
    cfw, truth, starts = toy_layout()
    inst = np.concatenate([cam.instance_records(meshes, [0, 1], truth[s], [0, 1], cfw) for s in range(2)])
    inst_begin = np.array([0, 2, 4])
    cameras = np.stack([cam.camera_rows(TOY_INTR, cfw)] * 2)
    t, img, _ = cam.render_depth(meshes, inst, inst_begin, cameras, TOY_H, TOY_W)
    clouds, packed, ranges, pairs, poses0, n = {}, [], [], [], [], 0
    for cls in (0, 1):
        per_scene = cam.pixel_clouds(t, img, inst["label"], inst_begin, cameras, cls)
        for s in range(2):
            clouds[(s, cls)] = per_scene[s]
            packed.append(per_scene[s])
            ranges.append((n, n + len(per_scene[s])))
            n += len(per_scene[s])
            pairs.append((s, cls)), poses0.append(starts[s, cls])
    rng = np.random.default_rng(6)
    pairs += [(0, 0), (1, 1)]
    poses0 += [perturbed(truth[0, 0], rng, 0.05, np.deg2rad(40.0)), starts[1, 1]]
    ranges += [ranges[0], (7, 7)]
    rec, pool = table(grids)
    c = dict(DEFAULTS, objects=rec, pool=pool, obj_index=np.array([o for _, o in pairs], np.int32), poses0=rows(np.stack(poses0)),
             points=np.ascontiguousarray(np.concatenate(packed)), ranges=np.array(ranges, np.int32))
    return dict(meshes=meshes, grids=grids, cam_from_world=cfw, truth=truth, instances=inst, inst_begin=inst_begin, cameras=cameras, clouds=clouds,
                call=c, pairs=np.array(pairs))


@functools.lru_cache(maxsize=None)
def toy_spec():
    from omg_planner_amd import registration as reg
    poses, stats = reg.register_clouds(*args(toy()["call"]))
    poses.setflags(write=False), stats.setflags(write=False)
    return poses, stats


# ---------------------------------------------------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------------------------------------------------
def device_scenes(c, dev):
    """A call's records and pool as one scene of an ops.DeviceScenes -> (dscenes, pairs [M,2])."""
    from omg_planner_amd import ops, scenes as S
    ds = ops.DeviceScenes(S.SceneBatch(c["objects"].copy(), np.array([0, len(c["objects"])], np.int32), c["pool"]), device=dev)
    return ds, np.stack([np.zeros(len(c["obj_index"]), np.int64), np.asarray(c["obj_index"], np.int64)], -1)


def device_register(c, dev, out=None, ds=None):
    """ops.register_clouds on a call -> (poses, stats) device tensors."""
    import torch
    from omg_planner_amd import ops
    built, pairs = device_scenes(c, dev)
    points = torch.from_numpy(np.ascontiguousarray(c["points"], np.float64).reshape(-1, 3)).to(dev)
    poses0 = torch.from_numpy(np.ascontiguousarray(c["poses0"], np.float64)).to(dev)
    return ops.register_clouds(ds or built, pairs, poses0, points, c["ranges"], stride=c["stride"], trunc=c["trunc"], lambda0=c["lambda0"],
                               step_tol=c["step_tol"], max_passes=c["max_passes"], out=out)
