"""The cases the depth-fusion tests share (tests/test_fusion_cpu.py, tests/test_gpu_fusion.py, tests/fuzz/fuzz_fusion.py): state
grids for the distance transform, carve set-ups with known answers, the observed scene of a sphere on a slab, and the shapes
that straddle the chunk of the y and x passes.  Everything is computed once per process (functools.lru_cache) and never changed."""
from __future__ import annotations

import functools

import numpy as np

from tests import mesh_cases as MC

CHUNK = 64  # OMGX_FUSION_CHUNK (test_fusion_cpu.py asserts it is the header's)
GRIDS = ((5, 7, 9), (1, 6, 4), (17, 3, 33), (8, 8, 8))
RADII = (1, 3, 40)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# distance transform: states -> volumes
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def states(name):
    """uint8 [X,Y,Z] with 0, 1, 2 and a few bytes that are none of them (they count as unknown)."""
    if name == "all_free":
        return np.zeros((8, 8, 8), np.uint8)
    if name == "all_occupied":
        return np.ones((8, 8, 8), np.uint8)
    if name.startswith(("straddle", "long")):  # <axis>: one axis of 2 * chunk + 3 (long: 4 * chunk + 5), the others of 3 and 2
        axis = int(name[-1])
        dims = [3, 2, 3]
        dims[axis] = 2 * CHUNK + 3 if name.startswith("straddle") else 4 * CHUNK + 5
        rng = np.random.default_rng(100 + axis)
        s = (rng.random(dims) < 0.02).astype(np.uint8)  # few occupied nodes: distances reach across the chunks
        s[rng.random(dims) < 0.01] = 2
        return s
    dims = tuple(int(d) for d in name.split("x"))
    rng = np.random.default_rng(sum(dims))
    s = rng.choice(np.array([0, 1, 2, 7], np.uint8), size=dims, p=[0.6, 0.15, 0.2, 0.05])
    return np.ascontiguousarray(s)


TRANSFORM = tuple("x".join(map(str, g)) for g in GRIDS) + ("all_free", "all_occupied")
# (long: with radius 255 a chunk of the x or y pass stages all 261 lines, more than 64 KB of LDS)
STRADDLE = ("straddle0", "straddle1", "straddle2", "long0", "long1")
STRADDLE_RADII = (1, 5, 70, 255)  # inside a chunk, across one chunk (70 > 64), the largest (255 > the axis of 131)


def brute_d2(mask, radius):
    """min(radius^2, squared index distance to the nearest node of mask) by all pairs (small grids)."""
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in mask.shape], indexing="ij"), -1).reshape(-1, 3)
    sel = idx[mask.ravel()]
    if not len(sel):
        return np.full(mask.shape, radius * radius, np.int64)
    d2 = ((idx[:, None, :] - sel[None, :, :]) ** 2).sum(-1).min(1)
    return np.minimum(d2, radius * radius).reshape(mask.shape).astype(np.int64)


def scipy_d2(mask, radius):
    """The same from scipy.ndimage.distance_transform_edt's nearest-node indices (exact integers)."""
    from scipy import ndimage
    if not mask.any():
        return np.full(mask.shape, radius * radius, np.int64)
    near = ndimage.distance_transform_edt(~mask, return_distances=False, return_indices=True)
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in mask.shape], indexing="ij"))
    return np.minimum(((near.astype(np.int64) - idx) ** 2).sum(0), radius * radius)


# ---------------------------------------------------------------------------------------------------------------------
# carve: set-ups with known answers.  One camera at the origin of the grid frame looking along +z of the grid (cam_from_grid =
# identity), fx = fy = 1, cx = cy = 0 unless said otherwise: node (x, y, z) projects to column floor(x / z + 0.5), row floor(y / z + 0.5).
# ---------------------------------------------------------------------------------------------------------------------
IDENTITY = np.eye(4)[:3]


def view(fx=1.0, fy=1.0, cx=0.0, cy=0.0, m=IDENTITY):
    from omg_planner_amd import fusion
    return fusion.view_rows((fx, fy, cx, cy), m)


def line_volume(points_z, x=0.0, y=0.0):
    """A 1 x 1 x n volume of node samples whose k-th node is (x, y, points_z[0] + k * delta): equally spaced z."""
    z = np.asarray(points_z, np.float64)
    delta = float(z[1] - z[0]) if len(z) > 1 else 1.0
    return ((x, y, float(z[0])), delta, "node", (1, 1, len(z)))


# The edges of the carve rule as ONE ragged batch with the answers written out: three images of 2 x 4, band 0.5, near 1.0.  Views
# 0 and 1 are the identity camera above; view 2 has fx = fy = 2, cx = 1 and stands 1 behind the origin (z_cam = z + 1, column
# floor(2 x / z_cam + 1.5)).  Every coordinate and depth below, and every quotient that lies on an edge, is exact in binary.
_I, _N = float("inf"), float("nan")
_F, _S, _U = 0, 1, 2
EDGE_BAND, EDGE_NEAR = 0.5, 1.0
EDGE_DEPTH = np.array([[[_I, _I, _I, _I], [_I, _I, _I, _I]],
                       [[_N, 0.0, -1.0, _I], [3.0, _I, _I, _I]],
                       [[_I, 3.0, 2.0, _I], [_I, _I, _I, _I]]])
_MOVED = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 1.0]])
# (what it is about, volume, view range, states)
EDGE_CASES = (
    ("z at near says nothing (the test is z > near)", ((0.0, 0.0, 0.5), 0.5, "node", (1, 1, 3)), (0, 1), [_U, _U, _F]),
    # x / z = -1, -0.5 .. 3, 3.5, 4 at z = 2 on W = 4: -0.5 is the left edge of pixel 0 (inside), 3.5 = W - 0.5 outside
    ("columns: pixel -0.5 inside, W - 0.5 outside", ((-2.0, 0.0, 2.0), 1.0, "node", (11, 1, 1)), (0, 1), [_U] + [_F] * 8 + [_U, _U]),
    # y / z = -1, -0.5, 0, 0.5, 1, 1.5 at z = 2 on H = 2
    ("rows: pixel -0.5 inside, H - 0.5 outside", ((0.0, -2.0, 2.0), 1.0, "node", (1, 6, 1)), (0, 1), [_U, _F, _F, _F, _F, _U]),
    ("the columns again as voxel centres", ((-2.5, -0.5, 1.5), 1.0, "centre", (11, 1, 1)), (0, 1), [_U] + [_F] * 8 + [_U, _U]),
    # columns 0 .. 3 of image 1's first row at z = 2
    ("depths NaN, 0 and negative say nothing, +inf frees", ((0.0, 0.0, 2.0), 2.0, "node", (4, 1, 1)), (1, 1), [_U, _U, _U, _F]),
    # y = 2.5: row 1, column 0 of image 1 (d = 3) for z = 2.25 .. 3.75
    ("z at d - band and at d + band is surface", ((0.0, 2.5, 2.25), 0.25, "node", (1, 1, 7)), (1, 1), [_F, _S, _S, _S, _S, _S, _U]),
    # views 0 (free everywhere) and 1 (d = 3): z = 3 surface in one and free in the other; z = 4 behind one and free in the other
    ("surface wins over free; free wins over nothing", ((0.0, 2.5, 3.0), 1.0, "node", (1, 1, 2)), (0, 2), [_S, _F]),
    # x = -1 .. 1 at z = 1: z_cam = 2, columns 0, 1, 1, 2, 2 of image 2's first row (inf, 3, 2)
    ("a moved camera with its own intrinsics", ((-1.0, 0.0, 1.0), 0.5, "node", (5, 1, 1)), (2, 1), [_F, _F, _F, _S, _S]),
    ("no views: nothing is known", ((0.0, 0.0, 2.0), 1.0, "node", (1, 1, 3)), (0, 0), [_U, _U, _U]),
)


def edge_views():
    return np.stack([view(), view(), view(2.0, 2.0, 1.0, 0.0, _MOVED)])


# ---------------------------------------------------------------------------------------------------------------------
# the observed scene: a sphere above a slab, three cameras
# ---------------------------------------------------------------------------------------------------------------------
SPHERE_C, SPHERE_R, SLAB_HALF = np.array([0.0, 0.0, 0.08]), 0.06, np.array([0.25, 0.25, 0.01])
EYES = ((0.6, 0.0, 0.5), (-0.3, 0.52, 0.5), (-0.3, -0.52, 0.5))
TARGET = (0.0, 0.0, 0.05)
H, W, F, CX, CY = 48, 64, 80.0, 31.5, 23.5
ORIGIN, DELTA, DIMS, BAND, NEAR, RADIUS = (-0.16, -0.16, -0.04), 0.01, (32, 32, 24), 0.015, 0.05, 12
SCENE_VOLUME = (ORIGIN, DELTA, "centre", DIMS, 0)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """cam_from_world [4,4] of a camera at `eye` whose optical axis (+z) points at `target`, rows downwards."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(-up, z)
    x = x / np.linalg.norm(x)  # to the right; y = z cross x points down
    y = np.cross(z, x)
    world_from_cam = np.eye(4)
    world_from_cam[:3, 0], world_from_cam[:3, 1], world_from_cam[:3, 2], world_from_cam[:3, 3] = x, y, z, eye
    return np.linalg.inv(world_from_cam)


@functools.lru_cache(maxsize=None)
def scene_meshes():
    return [MC.icosphere(2, SPHERE_R, tuple(SPHERE_C)), MC.box_mesh(tuple(SLAB_HALF))]


@functools.lru_cache(maxsize=None)
def scene_cameras():
    """(cam_from_world [3,4,4], intrinsics)"""
    return np.stack([look_at(e, TARGET) for e in EYES]), (F, F, CX, CY)


@functools.lru_cache(maxsize=None)
def scene_records(labels=(1, 1)):
    """What camera.render_depth / ops.CameraBatch take for the three cameras as three `scenes` of the same two instances (the
    sphere, the slab) with these labels: label 0 is the target."""
    from omg_planner_amd import camera
    cfw, intr = scene_cameras()
    meshes = scene_meshes()
    recs = [camera.instance_records(meshes, [0, 1], [np.eye(4), np.eye(4)], list(labels), cfw[s]) for s in range(3)]
    cams = np.stack([camera.camera_rows(intr, cfw[s]) for s in range(3)])
    return meshes, np.concatenate(recs), np.array([0, 2, 4, 6], np.int64), cams


@functools.lru_cache(maxsize=None)
def _scene_render():
    from omg_planner_amd import camera
    meshes, inst, begin, cams = scene_records()
    t, inst_img, _ = camera.render_depth(meshes, inst, begin, cams, H, W)
    return t, inst_img


def scene_sphere_pixels():
    """bool [3,H,W]: the pixels at which a camera sees the sphere (instance 0 of its scene)."""
    return _scene_render()[1] == 0


@functools.lru_cache(maxsize=None)
def scene_depth():
    """depth [3,H,W] float64 of the three cameras (camera.render_depth, the specification), and the view rows [3,16]."""
    from omg_planner_amd import fusion
    t, _ = _scene_render()
    cfw, intr = scene_cameras()
    return t, np.stack([fusion.view_rows(intr, cfw[s]) for s in range(3)])  # (the grid frame is the world frame)


@functools.lru_cache(maxsize=None)
def scene_states(num_views):
    from omg_planner_amd import fusion
    t, views = scene_depth()
    return fusion.carve_views([SCENE_VOLUME], views, [(0, num_views)], t, BAND, NEAR).reshape(DIMS)


@functools.lru_cache(maxsize=None)
def scene_volume(num_views, unknown_occupied=True):
    from omg_planner_amd import fusion
    return fusion.signed_volume(scene_states(num_views), DELTA, RADIUS, unknown_occupied)


@functools.lru_cache(maxsize=None)
def scene_analytic():
    """The signed distance of every node to the analytic solid (sphere or slab), [X,Y,Z] float64, and the nodes [N,3]."""
    from omg_planner_amd import fusion
    p = fusion.node_points(np.array(ORIGIN), DELTA, 0.5, DIMS)
    sphere = np.linalg.norm(p - SPHERE_C, axis=1) - SPHERE_R
    q = np.abs(p) - SLAB_HALF
    box = np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0)
    return np.minimum(sphere, box).reshape(DIMS), p


# ---------------------------------------------------------------------------------------------------------------------
# a ragged batch for the device and the host harness: three volumes of different dims and sample offsets, overlapping view
# ranges over the scene's three images
# ---------------------------------------------------------------------------------------------------------------------
RAGGED = [((-0.16, -0.16, -0.04), 0.02, "centre", (16, 16, 12)), ((-0.1, -0.12, 0.0), 0.013, "node", (17, 9, 5)),
          ((-0.05, -0.05, 0.01), 0.01, "centre", (7, 10, 13))]
RAGGED_RANGES = [(0, 3), (1, 2), (2, 1)]
RAGGED_RADIUS = 6

# ---------------------------------------------------------------------------------------------------------------------
# six volumes for the workgroup-to-volume search: at 256 nodes per workgroup they take 1, 1, 1, 2, 3 and 2 workgroups (the
# prefix table 0, 1, 2, 3, 5, 8): a single node, a partly and an exactly full workgroup, one node past a full one, a long thin
# row, and no power of two of them; both sample offsets; two views of 8 x 8 pixels
# ---------------------------------------------------------------------------------------------------------------------
LOCATE_DIMS = ((1, 1, 1), (5, 7, 3), (4, 8, 8), (257, 1, 1), (1, 1, 513), (3, 3, 29))
LOCATE_FIRST_WORKGROUP = (0, 1, 2, 3, 5, 8, 10)
LOCATE = [((-0.03 + 0.004 * m, -0.02, 0.01 * m), 0.004 + 0.0005 * m, ("centre", "node")[m % 2], d) for m, d in enumerate(LOCATE_DIMS)]
LOCATE_RANGES = [(0, 2), (1, 1), (0, 1), (0, 2), (0, 2), (1, 1)]
LOCATE_BAND, LOCATE_NEAR, LOCATE_RADIUS = 0.02, 0.05, 5


def locate_views():
    """(depth [2,8,8] float64 with background and void pixels, view rows [2,16]): a camera 0.3 below the origin that looks along
    +z and one 0.3 behind it that looks along +x."""
    r, c = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    depth = np.stack([0.3 + 0.02 * ((3 * r + c) % 7), 0.28 + 0.03 * ((r + 2 * c) % 9)]).astype(np.float64)
    depth[0, 0, 0], depth[1, 7, 7], depth[1, 2, 3] = np.inf, np.inf, 0.0
    along_z = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0.3]])
    along_x = np.array([[0, 1.0, 0, 0], [0, 0, 1.0, 0], [1.0, 0, 0, 0.3]])
    return depth, np.stack([view(12.0, 12.0, 3.5, 3.5, along_z), view(10.0, 10.0, 3.5, 3.5, along_x)])
