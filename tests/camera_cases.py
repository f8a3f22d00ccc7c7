"""Scenes shared by the depth-camera tests (test_camera_cpu.py, test_gpu_camera.py): every scene either file renders is built
here by name, so that the cull-neutrality test can walk all of them, and the specification's answer is computed once per scene."""
from __future__ import annotations

import numpy as np

from tests import mesh_cases as MC

TILE = 256  # omgx_mesh_sdf_tile(); test_camera_cpu.py asserts it


def _affine(rotvec=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0), scale=1.0):
    P = MC.pose(rotvec, t)
    P[:3, :3] *= scale
    return P


def _truncated(nf):
    v, f = MC.icosphere(3)
    return v, np.ascontiguousarray(f[:nf])


def at_pixel(intr, H, W, ur, uc, z):
    """The camera-frame point at depth z that projects to the image fraction (ur, uc) of an H x W image."""
    fx, fy, cx, cy = intr
    return ((uc * W - cx) / fx * z, (ur * H - cy) / fy * z, z)


def build(meshes, scenes, H, W):
    """scenes: per scene (intrinsics, cam_from_world, [(mesh, pose in the world, label)]) -> the dict every test takes."""
    from omg_planner_amd import camera as cam
    recs, begin, rows = [], [0], []
    for intr, cfw, items in scenes:
        recs.append(cam.instance_records(meshes, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items], cfw))
        begin.append(begin[-1] + len(items))
        rows.append(cam.camera_rows(intr, cfw))
    return dict(meshes=meshes, instances=np.concatenate(recs), inst_begin=np.array(begin, np.int64), cameras=np.stack(rows), H=H, W=W,
                poses=[[i[1] for i in items] for _, _, items in scenes], cam_from_world=[np.asarray(c, np.float64) for _, c, _ in scenes])


def single(scene, s):
    """Scene s of a multi-scene dict as a dict of its own."""
    b0, b1 = int(scene["inst_begin"][s]), int(scene["inst_begin"][s + 1])
    return dict(scene, instances=scene["instances"][b0:b1], inst_begin=np.array([0, b1 - b0], np.int64), cameras=scene["cameras"][s: s + 1],
                poses=[scene["poses"][s]], cam_from_world=[scene["cam_from_world"][s]])


EYE = np.eye(4)
BOX = MC.box_mesh(MC.BOX_HALF)
INTR = (100.0, 100.0, 15.5, 19.5)        # the 40 x 32 image of the known-answer scenes
BOX_POSED = MC.pose((0.2, 0.1, -0.3), (0.02, -0.01, 0.5))
CAM_POSED = MC.pose((0.3, -0.2, 0.1), (0.4, -0.3, 0.2))  # cam_from_world of the posed camera


def _known(items, cfw=EYE, meshes=None):
    return lambda: build(meshes or [BOX], [(INTR, cfw, items)], 40, 32)


def _sized(H, W, outside=False, S3=False):
    """The scene of the device tests at H x W: the four truncated spheres around the LDS tile, the box, a duplicate of the box at
    the same pose and a box behind the camera; some scaled (an affine pose).  S3: three scenes with 0, 1 and 6 instances and three
    different cameras."""
    def make():
        f = 0.9 * max(H, W, 8)
        intr = (f, 1.1 * f, -5.0, H + 23.0) if outside else (f, 1.1 * f, 0.5 * (W - 1), 0.5 * (H - 1))
        meshes = [_truncated(TILE - 1), _truncated(TILE), _truncated(TILE + 1), _truncated(2 * TILE + 1), BOX]
        items = [(0, _affine((0.3, 0.1, 0.0), at_pixel(intr, H, W, 0.25, 0.2, 0.5), 2.0), 1),
                 (1, _affine((0.0, 2.0, 0.3), at_pixel(intr, H, W, 0.7, 0.3, 0.45), 2.5), 0),
                 (4, _affine((0.2, 0.1, -0.3), at_pixel(intr, H, W, 0.5, 0.5, 0.4), 1.5), 2),
                 (4, _affine((0.2, 0.1, -0.3), at_pixel(intr, H, W, 0.5, 0.5, 0.4), 1.5), 1),     # the duplicate: never seen
                 (2, _affine((1.0, -0.4, 0.2), at_pixel(intr, H, W, 0.3, 0.8, 0.6), 3.0), 0),
                 (3, _affine((-0.5, 0.2, 2.5), at_pixel(intr, H, W, 0.8, 0.75, 0.5), 2.0), 1),
                 (4, _affine((0.0, 0.0, 0.0), (0.0, 0.0, -0.5)), 0)]                                # behind the camera
        if not S3:
            return build(meshes, [(intr, EYE, items)], H, W)
        intr2 = (1.3 * f, f, 0.4 * W, 0.6 * H)
        cfw2 = MC.pose((0.05, -0.1, 0.2), (0.01, 0.02, -0.03))
        world = lambda cfw, its: [(m, np.linalg.inv(cfw) @ p, l) for m, p, l in its]
        return build(meshes, [(intr, EYE, []), (intr2, cfw2, world(cfw2, items[2:3])), (intr, CAM_POSED, world(CAM_POSED, items[1:]))], H, W)
    return make


def _random(k):
    """33 x 35 pixels; six instances each of icosphere(2), the box and the first 257 faces of icosphere(3) at random poses with
    z in [-0.1, 0.9]; one stream RandomState(0) for all twelve, so scene k draws after the scenes before it."""
    def make():
        rng = np.random.RandomState(0)
        meshes = [MC.icosphere(2), BOX, _truncated(257)]
        for _ in range(k + 1):
            items = [(m, MC.pose(rng.uniform(-1.5, 1.5, 3), (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.9))), int(rng.randint(0, 2)))
                     for m in (0, 1, 2) for _ in range(6)]
        return build(meshes, [((30.0, 30.0, 17.0, 16.0), EYE, items)], 33, 35)
    return make


SCENES = {
    "box_axis": _known([(0, MC.pose(t=(0.0, 0.0, 0.5)), 0)]),
    "box_posed": _known([(0, BOX_POSED, 3)]),
    "box_behind": _known([(0, MC.pose((0.2, 0.1, -0.3), (0.0, 0.0, -0.5)), 0)]),
    "box_offscreen": _known([(0, MC.pose(t=(2.0, 0.0, 0.5)), 0)]),
    "inside_sphere": _known([(0, MC.pose(t=(0.0, 0.0, 0.01)), 0)], meshes=[MC.icosphere(2)]),
    # the far box first, the near one second and shifted: the nearer wins where they overlap, whatever the order
    "overlap": _known([(0, MC.pose(t=(0.0, 0.0, 0.6)), 0), (0, MC.pose(t=(0.04, 0.05, 0.45)), 1)]),
    "duplicate": _known([(0, BOX_POSED, 0), (0, BOX_POSED, 1)]),
    "shared_mesh": _known([(0, MC.pose((0.0, 0.5, 0.0), (-0.08, 0.0, 0.5)), 0), (0, MC.pose((0.4, 0.0, 0.2), (0.08, 0.05, 0.55)), 1)]),
    "posed_camera": _known([(0, np.linalg.inv(CAM_POSED) @ BOX_POSED, 0), (0, np.linalg.inv(CAM_POSED) @ MC.pose(t=(-0.08, 0.1, 0.6)), 1)],
                           cfw=CAM_POSED),
    "1x1": _sized(1, 1), "15x17": _sized(15, 17), "16x16": _sized(16, 16), "17x33": _sized(17, 33, outside=True),
    "multi": _sized(17, 33, S3=True),
    "1x257": _sized(1, 257), "25x41": _sized(25, 41),
}


def _observed():
    """Two scenes.Scene as camera.observe_scenes takes them (a table without a mesh, a target, obstacles; two cameras looking
    down, 40 x 48 pixels), with the records camera.scene_records makes of them."""
    from omg_planner_amd import camera as cam, scenes as S
    grid = S.SdfGrid(np.ones((2, 2, 2), np.float32), np.zeros(3), 0.1)
    ball = MC.icosphere(2)
    cfw = np.stack([np.linalg.inv(MC.pose((np.pi, 0.0, 0.0), (0.5, 0.0, 0.9))), np.linalg.inv(MC.pose((np.pi, 0.1, 0.0), (0.45, 0.05, 0.8)))])
    scenes = [S.Scene([S.SceneObject("table", np.eye(4), grid), S.SceneObject("a", MC.pose((0.0, 0.0, 0.3), (0.5, 0.0, 0.2)), grid),
                       S.SceneObject("b", MC.pose(t=(0.6, 0.15, 0.25)), grid), S.SceneObject("c", MC.pose((0.2, 0.0, 0.0), (0.4, -0.12, 0.15)), grid)], 1),
              S.Scene([S.SceneObject("b", MC.pose(t=(0.5, 0.1, 0.2)), grid), S.SceneObject("a", MC.pose((0.0, 0.0, 1.0), (0.42, -0.05, 0.25)), grid)], 0)]
    meshes = [[None, BOX, ball, BOX], [ball, BOX]]
    intr = (60.0, 60.0, 23.5, 19.5)
    pool, instances, begin, cameras = cam.scene_records(scenes, meshes, cfw, intr)
    return dict(meshes=pool, instances=instances, inst_begin=begin, cameras=cameras, H=40, W=48, cam_from_world=list(cfw),
                poses=[[o.pose_mat for o, m in zip(sc.objects, ms) if m is not None] for sc, ms in zip(scenes, meshes)],
                scenes=scenes, scene_meshes=meshes, intrinsics=intr)


def _many():
    """70 scenes of 17 x 18 pixels (2 x 2 tiles each), every one with its own camera; 0..4 instances per scene in a cycle, of the box
    and icosphere(1) at random affine poses (a scale per axis, the first instance of all mirrored) with z in [-0.1, 0.9] in front
    of the scene's camera."""
    rng = np.random.RandomState(70)
    meshes = [BOX, MC.icosphere(1)]
    scenes = []
    for s in range(70):
        intr = (rng.uniform(14.0, 30.0), rng.uniform(14.0, 30.0), rng.uniform(2.0, 16.0), rng.uniform(2.0, 15.0))
        cfw = MC.pose(rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.3, 0.3, 3))
        items = []
        for _ in range(s % 5):
            P = MC.pose(rng.uniform(-1.5, 1.5, 3), (rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), rng.uniform(-0.1, 0.9)))
            scale = rng.uniform(0.6, 2.5, 3)
            if not any(len(it) for _, _, it in scenes) and not items:
                scale[0] = -scale[0]                                    # the mirrored one
            P[:3, :3] = P[:3, :3] * scale
            items.append((int(rng.randint(0, 2)), np.linalg.inv(cfw) @ P, int(rng.randint(0, 2))))
        scenes.append((intr, cfw, items))
    return build(meshes, scenes, 17, 18)


SCENES["observed"] = _observed
SCENES["many"] = _many
SCENES.update({f"random{k}": _random(k) for k in range(12)})
RANDOM = [f"random{k}" for k in range(12)]

_BUILT, _SPEC = {}, {}


def scene(name):
    if name not in _BUILT:
        _BUILT[name] = SCENES[name]()
    return _BUILT[name]


def spec(name, cull=True):
    """camera.render_depth's (t, inst, face) of a named scene, computed once and never written to."""
    from omg_planner_amd import camera as cam
    if (name, cull) not in _SPEC:
        sc = scene(name)
        out = cam.render_depth(sc["meshes"], sc["instances"], sc["inst_begin"], sc["cameras"], sc["H"], sc["W"], cull=cull)
        for a in out:
            a.setflags(write=False)
        _SPEC[(name, cull)] = out
    return _SPEC[(name, cull)]


def labels(sc):
    return sc["instances"]["label"]


def box_slab(pose, cfw, intr, H, W, half=MC.BOX_HALF):
    """The known answer for a box: (t [H,W], quad [H,W]) of the slab method in the box's frame, +inf / -1 for a miss; quad q is the
    face pair (2q, 2q + 1) of MC.box_mesh.  Independent of the specification: matrices applied with @."""
    fx, fy, cx, cy = intr
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d_cam = np.stack([(c - cx) / fx, (r - cy) / fy, np.ones((H, W))], -1)
    M = np.linalg.inv(np.asarray(cfw) @ np.asarray(pose))
    o, d = M[:3, 3], d_cam @ M[:3, :3].T
    h = np.asarray(half)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (-h - o) / d, (h - o) / d
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    axis = lo.argmax(-1)
    near, far = lo.max(-1), hi.min(-1)
    hit = (near <= far) & (near > 0)
    sign = -np.sign(np.take_along_axis(d, axis[..., None], -1)[..., 0])   # entering through the face the ray runs against
    quad = 2 * axis + (sign > 0)
    return np.where(hit, near, np.inf), np.where(hit, quad, -1)


# ---------------------------------------------------------------------------------------------------------------------
# synthetic images for the cloud kernels: no render, the instance image is drawn directly
# ---------------------------------------------------------------------------------------------------------------------
EDGE_LANES = (0, 63, 64, 127, 128, 191, 192, 255)   # first and last lane of every wave of a group of 256 pixels
PATTERNS = ("random", "full", "edges", "blocks")
# (S, H, W) -> the scan entries n = S * groups k_pixel_scan walks (256 per pass, 64 per wave), and the patterns the device runs
CLOUD_SHAPES = {
    (63, 5, 7): (63, ("random", "full")), (64, 5, 7): (64, ("random", "edges")), (65, 5, 7): (65, ("random", "blocks")),
    (255, 3, 3): (255, ("random", "blocks")), (256, 3, 3): (256, ("random", "full")), (257, 3, 3): (257, ("random", "edges")),
    (600, 5, 7): (600, PATTERNS),
    (86, 20, 30): (258, PATTERNS),            # 3 groups per scene: 256 = 85 * 3 + 1, a scene boundary off the pass boundary
    (1, 257, 256): (257, PATTERNS),           # one scene across two passes
    (2, 1, 33285): (262, ("random", "blocks")),
    (3, 300, 300): (1056, ("random", "blocks")),
}
CLOUD_CASES = [(*shape, pattern) for shape, (_, patterns) in CLOUD_SHAPES.items() for pattern in patterns]
CLOUD_CLASSES = (9, 0, 1, -1)


def synthetic_count(s):
    """Instances of scene s of a synthetic case: 3, 0, 1, 2, 3, 0, ...  Every fourth scene has none; the cycle starts at 3 so that
    a case of one scene has the labels 0, 1 and 2 and a case of two has a scene without instances."""
    return (s + 3) % 4


def _random_inst(rng, n, count):
    """n values uniform in [-2, count + 1]: out of range on both sides."""
    return rng.randint(-2, count + 2, n).astype(np.int32)


def synthetic(S, H, W, pattern, seed):
    """A scene dict (one box in the pool; scene s owns synthetic_count(s) instances with the labels 0, 1, 2 in order; random
    intrinsics with the principal point inside the image or outside it and a random posed camera per scene) plus the images
    `t` [S,H,W] float64 and `inst` [S,H,W] int32 that ops.pixel_clouds / camera.pixel_clouds take.  inst by pattern:
      random: uniform in [-2, count + 1], a handful of pixels INT32_MAX and INT32_MIN;
      full:   0 everywhere, also in the scenes without instances (which keep nothing);
      edges:  -1 except at the row-major pixels p with p % 256 in EDGE_LANES and at the last pixel, which name a valid instance
              (0 in a scene without instances);
      blocks: group g (256 row-major pixels) of scene s names valid instances everywhere when (g + s) % 3 == 0, is -1 when it is
              1 and `random` otherwise.
    t is uniform(0.1, 2) where a cloud of class -1 keeps the pixel, elsewhere +inf or (one in eight) NaN."""
    rng = np.random.RandomState(seed)
    HW = H * W
    scenes = []
    for s in range(S):
        f = rng.uniform(0.5, 2.0) * max(H, W, 8)
        cx, cy = (rng.uniform(0, W), rng.uniform(0, H)) if rng.rand() < 0.5 else (rng.uniform(-2.0 * W, -1.0), rng.uniform(H + 1.0, 3.0 * H))
        cfw = MC.pose(rng.uniform(-1.0, 1.0, 3), rng.uniform(-0.5, 0.5, 3))
        items = [(0, MC.pose(rng.uniform(-1.0, 1.0, 3), rng.uniform(-0.5, 0.5, 3)), i % 3) for i in range(synthetic_count(s))]
        scenes.append(((f, rng.uniform(0.8, 1.2) * f, cx, cy), cfw, items))
    sc = build([BOX], scenes, H, W)
    inst = np.empty((S, HW), np.int32)
    p = np.arange(HW)
    for s in range(S):
        count = synthetic_count(s)
        valid = rng.randint(0, max(count, 1), HW).astype(np.int32)
        if pattern == "random":
            inst[s] = _random_inst(rng, HW, count)
            at = rng.randint(0, HW, 4)
            inst[s, at[:2]], inst[s, at[2:]] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
        elif pattern == "full":
            inst[s] = 0
        elif pattern == "edges":
            inst[s] = np.where(np.isin(p % TILE, EDGE_LANES) | (p == HW - 1), valid, -1)
        elif pattern == "blocks":
            kind = (p // TILE + s) % 3
            inst[s] = np.where(kind == 0, valid, np.where(kind == 1, -1, _random_inst(rng, HW, count)))
        else:
            raise ValueError(pattern)
    counts = np.array([synthetic_count(s) for s in range(S)])[:, None]
    kept = (inst >= 0) & (inst < counts)
    t = np.where(kept, rng.uniform(0.1, 2.0, (S, HW)), np.where(rng.rand(S, HW) < 0.125, np.nan, np.inf))
    return dict(sc, t=t.reshape(S, H, W), inst=inst.reshape(S, H, W), pattern=pattern)


_CLOUD, _CLOUD_SPEC = {}, {}


def cloud_case(S, H, W, pattern):
    """synthetic() of a case of CLOUD_CASES, built once; the seed is the case's place in the list."""
    key = (S, H, W, pattern)
    if key not in _CLOUD:
        _CLOUD[key] = synthetic(S, H, W, pattern, 1000 + CLOUD_CASES.index(key))
        _CLOUD[key]["t"].setflags(write=False), _CLOUD[key]["inst"].setflags(write=False)
    return _CLOUD[key]


def cloud_spec(S, H, W, pattern, cls):
    """camera.pixel_clouds of a synthetic case -> (scene_begin [S+1], the points of all scenes [N,3]), computed once."""
    from omg_planner_amd import camera as cam
    key = (S, H, W, pattern, cls)
    if key not in _CLOUD_SPEC:
        sc = cloud_case(S, H, W, pattern)
        per = cam.pixel_clouds(sc["t"], sc["inst"], labels(sc), sc["inst_begin"], sc["cameras"], cls)
        flat = np.concatenate(per)
        flat.setflags(write=False)
        _CLOUD_SPEC[key] = (np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int64), flat)
    return _CLOUD_SPEC[key]
