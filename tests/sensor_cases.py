"""The cases the depth-conditioning tests share (tests/test_sensor_cpu.py, tests/test_gpu_sensor.py): the shapes and seeded frames
on which the host harness and the device must equal omg-planner_amd/sensor.py bit for bit, the fuzz generator, the sphere scene
of tests/fusion_cases.py seen by a simulated sensor, and a plate in front of a wall whose flying pixels bridge the two.  Everything is computed once per process
(functools.lru_cache) and never changed."""
from __future__ import annotations

import functools

import numpy as np

from tests import fusion_cases as FC

INF, NAN = float("inf"), float("nan")

# ---------------------------------------------------------------------------------------------------------------------
# bit-for-bit cases: V = 3 views with three different intrinsics
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (16, 16), (17, 33), (40, 50))  # one pixel; one tile; partial tiles both ways; several tiles
RADII = (0, 1, 3, 7)
KINDS = ("uint16", "float64")
V = 3
INTRINSICS = np.array([(60.0, 60.0, 20.5, 15.5), (45.0, 52.0, 3.25, 30.0), (-80.0, 70.0, 24.0, -2.0)])
SCALE, Z_MIN, Z_MAX = 0.001, 0.3, 4.0
TAU = (0.002, 0.001, 0.004)
MIN_SUPPORT, RANGE_SCALE, COS_MIN = 3, 2.5, 0.97  # (the planes are nearly fronto-parallel: a cosine that splits them)


def table(R, seed=5):
    """(2R+1)^2 spatial weights that are NOT symmetric (a transposed or mirrored window changes the sums), some of them 0."""
    w = np.random.default_rng(seed + R).uniform(0.05, 1.0, (2 * R + 1) ** 2)
    w[::7] = 0.0
    w[len(w) // 2] = 1.0
    return w


def frames(Vn, H, W, kind, seed):
    """Vn frames of H x W: a tilted plane with a nearer box in front of it (steps on every side), millimetre noise, holes, lone
    pixels far from everything, values at and beyond z_min and z_max; float64 frames also carry NaN, +-inf, 0 and negatives."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((Vn, H, W))
    for v in range(Vn):
        z = rng.uniform(0.6, 2.5) + rng.uniform(-0.004, 0.004) * r + rng.uniform(-0.004, 0.004) * c
        r0, c0 = rng.integers(0, H), rng.integers(0, W)
        box = (r >= r0) & (r < r0 + max(2, H // 3)) & (c >= c0) & (c < c0 + max(2, W // 3))
        z = np.where(box, z - rng.uniform(0.1, 0.4), z) + 0.001 * rng.standard_normal((H, W))
        u = rng.random((H, W))
        z = np.where(u < 0.05, 0.0, z)                                    # holes
        z = np.where((u >= 0.05) & (u < 0.07), z + rng.uniform(0.1, 1.0, (H, W)), z)  # lone pixels
        z = np.where((u >= 0.07) & (u < 0.08), Z_MIN, z)
        z = np.where((u >= 0.08) & (u < 0.09), Z_MAX, z)
        z = np.where((u >= 0.09) & (u < 0.10), Z_MAX + 0.001, z)
        z = np.where((u >= 0.10) & (u < 0.11), Z_MIN - 0.001, z)
        out[v] = z
    if kind == "uint16":
        return np.clip(np.rint(out / SCALE), 0, 65535).astype(np.uint16)
    u = rng.random(out.shape)
    for lo, bad in ((0.00, NAN), (0.01, INF), (0.02, -INF), (0.03, -1.0)):
        out = np.where((u >= lo) & (u < lo + 0.01), bad, out)
    return out


@functools.lru_cache(maxsize=None)
def bit_case(H, W, R, kind):
    """The inputs and the specification's answers for one shape, radius and input kind."""
    from omg_planner_amd import sensor
    f = frames(V, H, W, kind, 1000 * H + 10 * W + R)
    depth, flags = sensor.condition_depth(f, SCALE, Z_MIN, Z_MAX, TAU, MIN_SUPPORT, R, table(R), RANGE_SCALE)
    normals, depth2, flags2, cosine = sensor.depth_normals(depth, INTRINSICS, TAU, COS_MIN, flags)
    return dict(frames=f, table=table(R), depth=depth, flags=flags, normals=normals, depth2=depth2, flags2=flags2, cosine=cosine)


def draw(rng):
    """One fuzz case: random sizes, radius, table, thresholds and input kind."""
    H, W, Vn, R = int(rng.integers(1, 71)), int(rng.integers(1, 71)), int(rng.integers(1, 6)), int(rng.integers(0, 8))
    kind = KINDS[int(rng.integers(0, 2))]
    w = rng.uniform(0.0, 1.0, (2 * R + 1) ** 2)
    w[len(w) // 2] = rng.uniform(0.1, 1.0)
    k = np.stack([rng.uniform(30.0, 90.0, Vn) * rng.choice([-1.0, 1.0], Vn), rng.uniform(30.0, 90.0, Vn), rng.uniform(-5.0, W + 5.0, Vn),
                  rng.uniform(-5.0, H + 5.0, Vn)], -1)
    return dict(frames=frames(Vn, H, W, kind, int(rng.integers(1 << 30))), scale=SCALE, z_min=float(rng.uniform(0.2, 0.7)),
                z_max=float(rng.uniform(2.0, 4.5)), tau=tuple(rng.uniform(0.0, 0.006, 3)), min_support=int(rng.integers(0, 9)), radius=R, table=w,
                range_scale=float(rng.uniform(0.5, 4.0)), intrinsics=k, cos_min=float(rng.uniform(0.6, 1.0)))


def specification(c):
    from omg_planner_amd import sensor
    depth, flags = sensor.condition_depth(c["frames"], c["scale"], c["z_min"], c["z_max"], c["tau"], c["min_support"], c["radius"], c["table"],
                                          c["range_scale"])
    return (depth, flags) + sensor.depth_normals(depth, c["intrinsics"], c["tau"], c["cos_min"], flags)


FUZZ_SEED, FUZZ_TRIALS = 20260, 12

# ---------------------------------------------------------------------------------------------------------------------
# the effect: fusion_cases' sphere on a slab (three 64 x 48 cameras about 0.78 m away) through a simulated sensor
# ---------------------------------------------------------------------------------------------------------------------
EFFECT_SEED = 7
EFFECT_SCALE, EFFECT_SIGMA, EFFECT_DROPOUT = 0.001, (0.001, 0.003), 0.01   # about 3 mm of noise at 0.8 m
EFFECT_TAU = (0.012, 0.0, 0.02)                                           # about 25 mm there: above a slab row's depth step
EFFECT = dict(z_min=0.1, z_max=5.0, tau=EFFECT_TAU, min_support=3, radius=2, range_scale=2.0)
EFFECT_SIGMA_PX, EFFECT_COS_MIN = 1.5, 0.15
MAX_DROPPED_SHARE = 0.02


@functools.lru_cache(maxsize=None)
def effect():
    """The simulated frames of the scene's three cameras and what the specification makes of them."""
    from omg_planner_amd import sensor
    t, _ = FC.scene_depth()
    frame, masks = sensor.simulate(t, np.random.default_rng(EFFECT_SEED), EFFECT_SCALE, EFFECT_SIGMA, EFFECT_DROPOUT, flying=EFFECT_TAU)
    tab = sensor.gaussian_table(EFFECT["radius"], EFFECT_SIGMA_PX)
    depth, flags = sensor.condition_depth(frame, EFFECT_SCALE, table=tab, **EFFECT)
    _, intr = FC.scene_cameras()
    k = np.tile(np.asarray(intr, np.float64), (3, 1))
    normals, depth2, flags2, cosine = sensor.depth_normals(depth, k, EFFECT_TAU, EFFECT_COS_MIN, flags)
    return dict(t=t, frame=frame, masks=masks, table=tab, depth=depth, flags=flags, intrinsics=k, normals=normals, depth2=depth2, flags2=flags2,
                cosine=cosine)


def effect_figures(e):
    """(flying pixels simulated, of them flagged FLYING, share of true-surface pixels dropped, rms of the raw frame, rms of the
    conditioned one) — the rms over the kept pixels whose noise-free 3 x 3 neighbourhood is continuous (every neighbour inside the
    image, finite and within tau of the centre)."""
    from omg_planner_amd import sensor
    t, m = e["t"], e["masks"]
    true = ~m["background"] & ~m["dropout"] & ~m["flying"]
    dropped = true & (e["flags2"] & 7 != sensor.KEPT)
    clean = np.where(np.isfinite(t), t, 0.0)
    smooth = np.isfinite(t)
    tau = sensor._tau(clean, EFFECT_TAU)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            smooth &= sensor._near(sensor._shift(clean, dr, dc), clean, tau)
    sel = true & smooth & (e["flags2"] & 7 == sensor.KEPT)
    raw = e["frame"].astype(np.float64) * EFFECT_SCALE
    rms = lambda x: float(np.sqrt(np.mean((x[sel] - t[sel]) ** 2)))
    return (int(m["flying"].sum()), int((e["flags"][m["flying"]] == sensor.FLYING).sum()), float(dropped.sum() / true.sum()), rms(raw),
            rms(e["depth2"]), int(sel.sum()))


# ---------------------------------------------------------------------------------------------------------------------
# flying pixels that bridge: a plate 5 cm in front of a wall, seen frontally by one 64 x 48 camera at the origin.  With a carve
# band of 1.5 cm the plate's and the wall's SURFACE nodes are 2 cm apart; a flying pixel at the mid depth fills exactly that.
# ---------------------------------------------------------------------------------------------------------------------
PLATE_SEED, PLATE_K = 11, (80.0, 80.0, 31.5, 23.5)
PLATE_Z, WALL_Z, PLATE_ROWS, PLATE_COLS = 0.75, 0.80, (14, 34), (20, 44)
PLATE_TAU = (0.008, 0.0, 0.0)  # 4 tau = 3.2 cm, below the gap
PLATE = dict(z_min=0.1, z_max=5.0, tau=PLATE_TAU, min_support=3, radius=1, range_scale=2.0)
PLATE_SIGMA_PX, PLATE_COS_MIN = 0.8, 0.15
PLATE_LAYOUT = ((-0.16, -0.12, 0.68), 0.01, (32, 24, 16))
PLATE_BAND, PLATE_NEAR, PLATE_REACH, PLATE_SEED_POINT, PLATE_MIN_NODES = 0.015, 0.05, 0.05, (0.0, 0.0, PLATE_Z), 20


@functools.lru_cache(maxsize=None)
def plate():
    """The simulated frame of the plate scene, the specification's conditioned image, and per image (raw, conditioned) the
    record of the component segmentation picks at the plate (segmentation.py on fusion.carve_views: the CPU construction)."""
    from omg_planner_amd import fusion, segmentation as sg, sensor
    t = np.full((1, FC.H, FC.W), WALL_Z)
    t[0, PLATE_ROWS[0]: PLATE_ROWS[1], PLATE_COLS[0]: PLATE_COLS[1]] = PLATE_Z
    frame, masks = sensor.simulate(t, np.random.default_rng(PLATE_SEED), 0.001, (0.0005, 0.0), 0.0, flying=PLATE_TAU)
    tab = sensor.gaussian_table(PLATE["radius"], PLATE_SIGMA_PX)
    depth, flags = sensor.condition_depth(frame, 0.001, table=tab, **PLATE)
    _, depth2, flags2, _ = sensor.depth_normals(depth, [PLATE_K], PLATE_TAU, PLATE_COS_MIN, flags)
    volume = (PLATE_LAYOUT[0], PLATE_LAYOUT[1], "centre", PLATE_LAYOUT[2])
    views = np.stack([fusion.view_rows(PLATE_K, np.eye(4))])
    picked = {}
    for name, img in (("raw", frame.astype(np.float64) * 0.001), ("conditioned", depth2)):
        state = fusion.carve_views([volume + (0,)], views, [(0, 1)], img, PLATE_BAND, PLATE_NEAR)
        _, records = sg.component_records(sg.label_components(state, [volume + (0,)], 1, 6), [volume + (0,)])
        picked[name] = records[sg.pick_component(records, sg.point_to_index(volume, PLATE_SEED_POINT), PLATE_MIN_NODES)]
    return dict(t=t, frame=frame, masks=masks, table=tab, depth2=depth2, flags2=flags2, picked=picked)
