"""The cases the clearance tests share (tests/test_clearance_cpu.py, tests/test_gpu_clearance.py): the edges of the rule with
their answers written out, the seeded batches of both ops, the draws of the fuzz run and the tunnelling scene.  Everything is
computed once per process (functools.lru_cache) and never changed."""
from __future__ import annotations

import functools

import numpy as np

from tests import volume_camera_cases as VC

INF, NAN = float("inf"), float("nan")
BATCH_N = (0, 1, 63, 64, 65, 257)   # no sphere, one, one less / exactly / one more than a wave, one more than the staging chunk
BATCH_B = (1, 4, 5, 17)             # one configuration, one workgroup's four, one more, several workgroups and a partial one
BATCH_S = (1, 3)
BATCH_DIMS = ((2, 2, 2), (5, 9, 7), (33, 17, 9))
BATCH_BEYOND = 0.15
SELF_N = (0, 1, 2, 65, 300, 1024)


def same(a, b) -> bool:
    """Equal arrays: float64 bit for bit (VC.same_bits: a NaN equals a NaN), integers exactly, dtype and shape included."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return VC.same_bits(a, b) if a.dtype == np.float64 else bool(np.array_equal(a, b))


def same_results(got, want) -> bool:
    """Tuples of arrays, None against None."""
    return len(got) == len(want) and all((g is None and w is None) or (g is not None and w is not None and same(g, w)) for g, w in zip(got, want))


def rigid(rng, reach=0.3):
    """A random rigid transform [4,4] with its translation inside +-reach."""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = q, rng.uniform(-reach, reach, 3)
    return out


def blob_volume(rng, dims, delta):
    """A volume that looks like a distance: the distance to a ball around the grid's middle plus a little noise, float32."""
    ax = [(np.arange(d) + 0.5) * delta for d in dims]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    mid = 0.5 * delta * np.asarray(dims)
    r = np.sqrt((x - mid[0]) ** 2 + (y - mid[1]) ** 2 + (z - mid[2]) ** 2) - 0.3 * delta * min(dims)
    return np.ascontiguousarray(r + rng.normal(scale=0.1 * delta, size=dims), np.float32)


def spheres(rng, N, zero_radius=True):
    """N spheres: centres within 8 cm of their link's frame, radii up to 6 cm, some of radius 0 -> (local [N,4], link [N] int32)."""
    local = np.concatenate([rng.uniform(-0.08, 0.08, (N, 3)), rng.uniform(0.0, 0.06, (N, 1))], 1)
    if zero_radius and N:
        local[rng.integers(0, N, max(1, N // 8)), 3] = 0.0
    return np.ascontiguousarray(local), rng.integers(0, 10, N).astype(np.int32)


def link_poses(rng, B, reach=0.3):
    return np.ascontiguousarray(np.stack([np.stack([rigid(rng, reach) for _ in range(10)]) for _ in range(B)])) if B else np.zeros((0, 10, 4, 4))


@functools.lru_cache(maxsize=None)
def table(S):
    """Five records over the three volumes of BATCH_DIMS, which lie at non-zero offsets of a ragged pool with NaN before, between
    and behind them (shuffled: the pool's order is not the records'): the three volumes, a DISABLED record on the second volume
    and a record on the third that the flags of `visible` make INVISIBLE.  S = 1: one scene owns all; S = 3: scene 0 the first
    three, scene 1 NOTHING, scene 2 the last two -> (objects, scene_begin, pool, visible flags)."""
    rng = np.random.default_rng(11)
    deltas = (0.12, 0.03, 0.012)
    vols = [blob_volume(rng, d, h) for d, h in zip(BATCH_DIMS, deltas)]
    objs = [(vols[k], tuple(rng.uniform(-0.1, 0.0, 3)), deltas[k], rigid(rng, 0.15), 0) for k in range(3)]
    objs.append((vols[1], tuple(rng.uniform(-0.1, 0.0, 3)), deltas[1], rigid(rng, 0.15), 1))
    objs.append((vols[2], tuple(rng.uniform(-0.1, 0.0, 3)), deltas[2], rigid(rng, 0.15), 0))
    scenes = [objs] if S == 1 else [objs[:3], [], objs[3:]]
    objects, begin, pool = VC.pack(scenes, gap=5, fill=NAN, shuffle=(2, 0, 1))
    assert (objects["grid_offset"] > 0).all() and np.isnan(pool).sum() == 5 * 4
    return objects, begin, pool, np.array([1, 1, 1, 1, 0], np.uint8)


@functools.lru_cache(maxsize=None)
def batch(N, B, S, flags):
    """One launch of omgx_sphere_clearance and its answer: N spheres at B configurations spread over S scenes; flags: whether
    `visible` is given (the invisible record is left out, the disabled one is used) or None (the other way round) -> dict with
    the arguments, world [B,N,4] and want: the specification's six outputs."""
    from omg_planner_amd import clearance as cl
    rng = np.random.default_rng(1000 * N + 10 * B + S + 7 * flags)
    objects, begin, pool, vis = table(S)
    local, link = spheres(rng, N)
    poses = link_poses(rng, B)
    cfg = rng.integers(0, S, B).astype(np.int32)
    if S == 3 and B >= 4:
        cfg[:3] = (0, 1, 2)  # every scene, the empty one included
    pad = np.ascontiguousarray(rng.uniform(0.0, 0.05, (B, 10)))
    visible = vis if flags else None
    world = cl.world_spheres(poses, local, link)
    want = cl.sphere_clearance(objects, begin, pool, visible, cfg, world, link, pad, BATCH_BEYOND)
    return dict(objects=objects, begin=begin, pool=pool, visible=visible, cfg=cfg, poses=poses, local=local, link=link, pad=pad,
                beyond=BATCH_BEYOND, world=world, want=want)


BATCHES = tuple((N, B, S, (i + j + k) % 2) for i, N in enumerate(BATCH_N) for j, B in enumerate(BATCH_B) for k, S in enumerate(BATCH_S))


@functools.lru_cache(maxsize=None)
def self_batch(N):
    """One launch of omgx_self_clearance: N spheres at 3 configurations, pads, a pair table with some links off."""
    from omg_planner_amd import clearance as cl
    rng = np.random.default_rng(50 + N)
    local, link = spheres(rng, N)
    world = cl.world_spheres(link_poses(rng, 3, 0.1), local, link)
    pairs = (rng.uniform(size=(10, 10)) < 0.7).astype(np.uint8)
    pad = np.ascontiguousarray(rng.uniform(0.0, 0.02, (3, 10)))
    return dict(world=world, link=link, pairs=pairs, pad=pad, want=cl.self_clearance(world, link, pairs, pad),
                want_bare=cl.self_clearance(world, link, pairs, None))


# ---------------------------------------------------------------------------------------------------------------------
# The edges of the rule.  Every link pose is the identity (a sphere's local centre is its world centre) and so is every object's
# pose.  The volume LINE has 3 x 3 x 3 samples with delta = 0.5 and lo = 0: the samples stand at 0.25, 0.75, 1.25 on every axis,
# u = 2 q - 0.5, the box of the samples is [0.25, 1.25]^3, and data[i, j, k] = 0.5 i, so that v = 0.5 u_x inside.  Every number
# below is exact in binary.  An answer is (clear, clear_sphere, clear_object, margin, margin_sphere, margin_object).
# ---------------------------------------------------------------------------------------------------------------------
def xvol(xv, across=(3, 3)):
    xv = np.asarray(xv, np.float32)
    return np.ascontiguousarray(np.broadcast_to(xv[:, None, None], (len(xv),) + across), np.float32)


_LINE = xvol([0.0, 0.5, 1.0])
_NAN_CELL = xvol([0.0, NAN, 1.0])
_OBJ = lambda data: (data, (0.0, 0.0, 0.0), 0.5, None, 0)
_MID = (0.75, 0.75)
_NOBODY = (INF, -1, -1)
_BELOW = float(np.nextafter(0.5, 0.0))

# (what it is about, the scene's objects, spheres [(x, y, z, r)], links, pad row [10] or None, beyond, the answer)
EDGE_CASES = (
    # u = (2, 1, 1): u_x == hi_x, i_x = min(2, 1) = 1, f_x = 1.0 reads the plane x = 2: v = 1.0; e = 0
    ("a centre on the far face (f == 1.0)", [_OBJ(_LINE)], [(1.25,) + _MID + (0.25,)], [0], None, 0.5, (0.75, 0, 0) + _NOBODY),
    # u = (0, 0, 0): on the box's corner, e == 0 exactly, v = 0
    ("a centre exactly on the box (e == 0), radius 0", [_OBJ(_LINE)], [(0.25, 0.25, 0.25, 0.0)], [0], None, 0.0, (0.0, 0, 0) + _NOBODY),
    # u = (-1, 1, 1): c = (0, 1, 1), x = (-1, 0, 0), e = 1 / 2 = delta; v(c) = 0: d = -0.5
    ("one voxel outside (e == delta, d = v - delta)", [_OBJ(_LINE)], [(-0.25,) + _MID + (0.125,)], [0], None, 1.0, (-0.625, 0, 0) + _NOBODY),
    ("exactly at e == beyond", [_OBJ(_LINE)], [(-0.25,) + _MID + (0.125,)], [0], None, 0.5, (-0.625, 0, 0) + _NOBODY),
    ("one ulp beyond", [_OBJ(_LINE)], [(-0.25,) + _MID + (0.125,)], [0], None, _BELOW, _NOBODY + _NOBODY),
    # both at u_x = 1: v = 0.5, minus 0.25
    ("two identical spheres: the lowest index wins", [_OBJ(_LINE)], [(0.75,) + _MID + (0.25,)] * 2, [3, 4], None, 0.5, (0.25, 0, 0) + _NOBODY),
    ("two identical objects: the lowest index wins", [_OBJ(_LINE), _OBJ(_LINE)], [(0.75,) + _MID + (0.25,)], [0], None, 0.5, (0.25, 0, 0) + _NOBODY),
    # u_x = 0.5 lies in the cell between the planes x = 0 and x = 1, and the plane x = 1 is NaN
    ("a NaN voxel in the cell: the only pair, nobody wins", [_OBJ(_NAN_CELL)], [(0.5,) + _MID + (0.25,)], [0], None, 0.5, _NOBODY + _NOBODY),
    # the second object gives v = 0.25 at u_x = 0.5
    ("a NaN voxel in the cell: the pair never wins", [_OBJ(_NAN_CELL), _OBJ(_LINE)], [(0.5,) + _MID + (0.125,)], [0], None, 0.5,
     (0.125, 0, 1) + _NOBODY),
    # sphere 0 (link 0): v = 0.5 - 0.25 = 0.25; sphere 1 (link 1): v = 0.75 - 0.25 = 0.5; the pad of link 1 is 0.375: 0.125 < 0.25
    ("pad moves the argmin to another link", [_OBJ(_LINE)], [(0.75,) + _MID + (0.25,), (1.0,) + _MID + (0.25,)], [0, 1],
     (0.0, 0.375) + (0.0,) * 8, 0.5, (0.25, 0, 0, 0.125, 1, 0)),
    ("a scene without objects", [], [(0.75,) + _MID + (0.25,)], [0], None, 0.5, _NOBODY + _NOBODY),
)


@functools.lru_cache(maxsize=None)
def edge_launch():
    """The edge cases as the device gets them: one launch per distinct (pad given or not, beyond) would hide nothing, but the
    scenes can share a table: scene k holds case k's objects, configuration k (identity poses) stands in scene k.  The spheres
    differ from case to case, so this returns one launch PER CASE over the shared table -> (objects, scene_begin, pool, [dict(cfg,
    poses, local, link, pad, beyond, want)])."""
    objects, begin, pool = VC.pack([objs for _, objs, *_ in EDGE_CASES], gap=4, fill=NAN)
    poses = np.ascontiguousarray(np.tile(np.eye(4), (1, 10, 1, 1)))
    out = []
    for k, (what, _, sph, links, pad, beyond, want) in enumerate(EDGE_CASES):
        out.append(dict(what=what, cfg=np.array([k], np.int32), poses=poses, local=np.ascontiguousarray(sph, np.float64), link=np.array(links, np.int32),
                        pad=np.ascontiguousarray([pad], np.float64) if pad is not None else None, beyond=beyond,
                        want=want if pad is not None else want[:3] + (None, None, None)))
    return objects, begin, pool, out


_TOUCH = [(0.0, 0.0, 0.0, 0.25), (0.5, 0.0, 0.0, 0.25)]
_ALL = np.ones((10, 10), np.uint8) - np.eye(10, dtype=np.uint8)
# (what it is about, spheres, links, pairs, pad row or None, the answer (self_clear, i, j))
SELF_CASES = (
    ("two touching spheres", _TOUCH, [0, 1], _ALL, None, (0.0, 0, 1)),
    ("pairs all zero", _TOUCH, [0, 1], np.zeros((10, 10), np.uint8), None, _NOBODY),
    ("the same link: not a pair of the table's diagonal", _TOUCH, [2, 2], _ALL, None, _NOBODY),
    ("radius 0", [(0.0, 0.0, 0.0, 0.0), (0.0, 0.75, 0.0, 0.0)], [0, 9], _ALL, None, (0.75, 0, 1)),
    ("identical pairs: the lowest (i, j) wins", _TOUCH + _TOUCH, [0, 1, 0, 1], _ALL, None, (0.0, 0, 1)),
    # 0.5 - ((0.25 + 0.125) + (0.25 + 0.0625))
    ("pads by link", _TOUCH, [0, 1], _ALL, (0.125, 0.0625) + (0.0,) * 8, (-0.1875, 0, 1)),
    ("one sphere", _TOUCH[:1], [0], _ALL, None, _NOBODY),
)


# ---------------------------------------------------------------------------------------------------------------------
# The draws of the fuzz run
# ---------------------------------------------------------------------------------------------------------------------
FUZZ_SEED, FUZZ_TRIALS = 20260, 20


def draw(rng):
    """One trial: N <= 300 spheres, B <= 40 configurations, S <= 4 scenes of 0..3 random grids at random poses, random beyond and
    pads, voxels that are not finite -> the arguments of one launch of each op."""
    N = int(rng.integers(2, 301)) if rng.uniform() < 0.5 else int(rng.choice([0, 1, 64, 65, 257]))
    B, S = int(rng.integers(1, 41)), int(rng.integers(1, 5))
    scenes = []
    for _ in range(S):
        objs = []
        for _ in range(int(rng.integers(0, 4))):
            dims = tuple(int(d) for d in rng.integers(2, 12, 3))
            delta = float(rng.uniform(0.01, 0.06))
            data = blob_volume(rng, dims, delta)
            bad = rng.uniform(size=dims) < 0.02
            data[bad] = rng.choice(np.array([NAN, INF, -INF], np.float32), int(bad.sum()))
            objs.append((data, tuple(rng.uniform(-0.2, 0.0, 3)), delta, rigid(rng, 0.2), int(rng.uniform() < 0.2)))
        scenes.append(objs)
    objects, begin, pool = VC.pack(scenes, gap=3, fill=NAN)
    local, link = spheres(rng, N)
    visible = (rng.uniform(size=len(objects)) < 0.8).astype(np.uint8) if rng.uniform() < 0.5 else None
    return dict(N=N, B=B, S=S, objects=objects, begin=begin, pool=pool, visible=visible, cfg=rng.integers(0, S, B).astype(np.int32),
                poses=link_poses(rng, B), local=local, link=link, pad=np.ascontiguousarray(rng.uniform(0.0, 0.05, (B, 10))) if rng.uniform() < 0.7 else None,
                beyond=float(rng.choice([0.0, 0.02, 0.1, 0.5])), cull=int(rng.integers(0, 2)), pairs=(rng.uniform(size=(10, 10)) < 0.6).astype(np.uint8))


def specification(c):
    """-> (world, the six outputs, the self op's three)."""
    from omg_planner_amd import clearance as cl
    world = cl.world_spheres(c["poses"], c["local"], c["link"])
    return world, cl.sphere_clearance(c["objects"], c["begin"], c["pool"], c["visible"], c["cfg"], world, c["link"], c["pad"], c["beyond"]), \
        cl.self_clearance(world, c["link"], c["pairs"], c["pad"])


# ---------------------------------------------------------------------------------------------------------------------
# Tunnelling: a plate between two waypoints
# ---------------------------------------------------------------------------------------------------------------------
PLATE_HALF = (0.06, 0.01, 0.06)     # a 2 cm plate (scenes.box_sdf), 12 cm square
PLATE_GRID, PLATE_DELTA = (48, 32, 48), 0.01
PLATE_SWING = 0.5                 # joint 0 turns from -PLATE_SWING to +PLATE_SWING
PLATE_LIFT = 0.15                   # the lifted plate: the same motion passes 9 cm below its edge, inside its grid
PLATE_RADIUS = 0.02
PLATE_BEYOND = 0.3
PLATE_K = (1, 16)                   # K = 1: nothing seen, nothing certified; K = 16: the hit seen, the lifted motion certified


@functools.lru_cache(maxsize=None)
def plate():
    """The scene table of the tunnelling case on the host: scene 0 holds the plate in the plane the hand sweeps through (through
    the hand's position at joint 0 = 0, its normal along the hand's motion there), scene 1 the same plate lifted by PLATE_LIFT
    along z -> dict(objects, begin, pool, traj [2,2,9], local, link, rho, r_max, model)."""
    from omg_planner_amd import clearance as cl, robot as rb, scenes as sc
    from oracle import oracle as orc
    model = rb.PandaModel(seed=0)
    q0 = rb.HOME_CONFIG.copy()
    q0[0] = 0.0
    hand = orc.fk(model.blob(), q0[None])[0][0, 7]
    # joint 0 turns about the world's z through the base: at q_0 = 0 the hand moves along z x p
    p = hand[:3, 3]
    along = np.cross([0.0, 0.0, 1.0], p)
    along /= np.linalg.norm(along)
    up = np.array([0.0, 0.0, 1.0])
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = np.cross(along, up), along, up, p  # the plate's thin axis (y) along the motion
    lifted = pose.copy()
    lifted[2, 3] += PLATE_LIFT
    grid = sc.box_sdf(PLATE_HALF, PLATE_GRID, PLATE_DELTA)
    objects, begin, pool = VC.pack([[(grid.data, tuple(grid.origin), PLATE_DELTA, pose, 0)], [(grid.data, tuple(grid.origin), PLATE_DELTA, lifted, 0)]],
                                   gap=2, fill=NAN)
    a, b = q0.copy(), q0.copy()
    a[0], b[0] = -PLATE_SWING, PLATE_SWING
    traj = np.ascontiguousarray(np.stack([np.stack([a, b])] * 2))
    local = np.array([(0.0, 0.0, 0.0, PLATE_RADIUS)])  # one sphere at the hand's frame
    link = np.array([7], np.int32)
    rho = cl.reach_table(model, local, link, 0.04)
    return dict(objects=objects, begin=begin, pool=pool, traj=traj, local=local, link=link, rho=rho, r_max=PLATE_RADIUS, model=model)


def plate_report(K, poses_of=None):
    """The specification's report of the two plans at K samples per segment; poses_of(q [B,9]) -> link poses [B,10,4,4] (default
    oracle.fk) -> (report dict, clear [2,T], margin [2,T])."""
    from omg_planner_amd import clearance as cl
    from oracle import oracle as orc
    c = plate()
    q = cl.dense_configs(c["traj"], K)
    T = q.shape[1]
    poses = (poses_of or (lambda x: orc.fk(c["model"].blob(), x)[0]))(q.reshape(-1, 9))
    world = cl.world_spheres(poses, c["local"], c["link"])
    pad = cl.sample_pads(cl.segment_halves(c["traj"], K, c["rho"]), K, 0.0).reshape(-1, 10)
    out = cl.sphere_clearance(c["objects"], c["begin"], c["pool"], None, np.repeat([0, 1], T), world, c["link"], pad, PLATE_BEYOND)
    clear, margin = out[0].reshape(2, T), out[3].reshape(2, T)
    return cl.plan_report(c["traj"], K, c["rho"], c["r_max"], 0.0, PLATE_BEYOND, clear, margin), out
