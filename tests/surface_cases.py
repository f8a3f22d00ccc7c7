"""Volumes shared by the surface-extraction tests (test_surface_cpu.py, test_gpu_surface.py): every volume either file extracts is
built here by name, the specification's answer (scenes.surface_nets) is computed once per case, and the mesh properties both files
assert are measured here."""
from __future__ import annotations

import functools

import numpy as np

BLOCK = 256  # OMGX_SURFACE_NODES_PER_WORKGROUP; test_surface_cpu.py asserts it
OFFSET = {"centre": 0.5, "node": 0.0}
SPHERE_R, BOX_HALF, TWO_R, TWO_X = 0.07, (0.05, 0.07, 0.03), 0.04, 0.047


def positions(dims, origin, delta, sample):
    ax = [origin[a] + (np.arange(dims[a], dtype=np.float64) + OFFSET[sample]) * delta for a in range(3)]
    return np.meshgrid(*ax, indexing="ij")


def sphere(dims, delta, sample, r, centre=(0.0, 0.0, 0.0), origin=None):
    origin = -0.5 * delta * np.array(dims, np.float64) if origin is None else np.asarray(origin, np.float64)
    x, y, z = positions(dims, origin, delta, sample)
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - r
    return d.astype(np.float32), origin


def box(dims, delta, sample, half):
    origin = -0.5 * delta * np.array(dims, np.float64)
    x, y, z = positions(dims, origin, delta, sample)
    q = np.stack([np.abs(x) - half[0], np.abs(y) - half[1], np.abs(z) - half[2]], -1)
    return (np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)).astype(np.float32), origin


def _case(data, origin, delta=0.01, sample="centre", level=0.0):
    return dict(data=np.ascontiguousarray(data, np.float32), origin=np.asarray(origin, np.float64), delta=float(delta), sample=sample,
                level=float(level))


SHAPES = ("sphere", "box", "two_spheres")
ANALYTIC_VOLUME = {"sphere": 4.0 / 3.0 * np.pi * SPHERE_R ** 3, "box": 8.0 * BOX_HALF[0] * BOX_HALF[1] * BOX_HALF[2],
                   "two_spheres": 2 * 4.0 / 3.0 * np.pi * TWO_R ** 3}
COMPONENTS = {("sphere", 0.0): 1, ("box", 0.0): 1, ("two_spheres", 0.0): 2, ("sphere", 0.01): 1, ("box", 0.01): 1, ("two_spheres", 0.01): 1}


def shape(name, sample="centre", level=0.0, n=24, delta=0.01):
    dims = (n, n, n)
    if name == "sphere":
        d, o = sphere(dims, delta, sample, SPHERE_R)
    elif name == "box":
        d, o = box(dims, delta, sample, BOX_HALF)
    else:
        a, o = sphere(dims, delta, sample, TWO_R, (-TWO_X, 0.0, 0.0))
        b, _ = sphere(dims, delta, sample, TWO_R, (TWO_X, 0.0, 0.0))
        d = np.minimum(a, b)
    return _case(d, o, delta, sample, level)


def _small_sphere(dims, r, sample="centre", level=0.0, centre=(0.0, 0.0, 0.0)):
    d, o = sphere(dims, 0.01, sample, r, centre)
    return _case(d, o, 0.01, sample, level)


def _with(case, edits):
    d = case["data"].copy()
    for idx, val in edits:
        d[idx] = val
    return dict(case, data=d)


def _near_surface(case, inside: bool):
    """An index of a sample next to the surface: inside with an outside neighbour along x (or the reverse), away from the border."""
    ins = case["data"] < np.float32(case["level"])
    a, b = (ins[1:-2, 1:-1, 1:-1], ~ins[2:-1, 1:-1, 1:-1]) if inside else (~ins[1:-2, 1:-1, 1:-1], ins[2:-1, 1:-1, 1:-1])
    i, j, k = np.argwhere(a & b)[0]
    return int(i) + 1, int(j) + 1, int(k) + 1


def _next_x(idx):
    return idx[0] + 1, idx[1], idx[2]


def _padded():
    """A 10^3 sphere volume inside the reference's pad-to-max layout: the rest of a 14 x 12 x 16 block is the 1.0 filler."""
    d, _ = sphere((10, 10, 10), 0.01, "centre", 0.03)
    out = np.full((14, 12, 16), 1.0, np.float32)
    out[:10, :10, :10] = d
    return _case(out, (-0.05, -0.05, -0.05))


def _cloud():
    """The unsigned nearest-point distance of a cloud on a small box's surface (scenes.point_cloud_sdf: node samples)."""
    from omg_planner_amd import scenes
    rng = np.random.default_rng(5)
    p = rng.uniform(-1.0, 1.0, (600, 3)) * np.array([0.03, 0.04, 0.02])
    ax = rng.integers(0, 3, 600)
    p[np.arange(600), ax] = np.sign(p[np.arange(600), ax]) * np.array([0.03, 0.04, 0.02])[ax]
    g = scenes.point_cloud_sdf(p, grid_resolution=0.01, margin=0.04)
    return dict(_case(g.data, g.origin, g.delta, "node", 0.015), points=p)


def _smooth(seed):
    """A random smooth volume, dims 2..20 per axis, with a random level inside its range."""
    rng = np.random.default_rng(seed)
    dims = tuple(int(d) for d in rng.integers(2, 21, 3))
    delta = float(rng.uniform(0.005, 0.02))
    origin = rng.uniform(-0.1, 0.1, 3)
    sample = ("centre", "node")[int(rng.integers(0, 2))]
    x, y, z = positions(dims, origin, delta, sample)
    f = np.zeros(dims)
    for _ in range(4):
        k, ph, amp = rng.uniform(10.0, 60.0, 3), rng.uniform(0.0, 6.28, 3), rng.uniform(0.2, 1.0)
        f += amp * np.sin(k[0] * x + ph[0]) * np.sin(k[1] * y + ph[1]) * np.sin(k[2] * z + ph[2])
    f = (0.02 * f).astype(np.float32)
    return _case(f, origin, delta, sample, float(rng.uniform(np.percentile(f, 20), np.percentile(f, 80))))


def _equal_to_level():
    c = _small_sphere((9, 8, 7), 0.025)
    i, j, k = _near_surface(c, inside=False)
    return _with(c, [((i, j, k), 0.0), ((i + 1, j, k), -0.0)])  # -0.0 < 0.0 is false: both are outside


@functools.lru_cache(maxsize=None)
def case(name):
    n24 = {f"{s}_{sm}_{lv}": (lambda s=s, sm=sm, lv=lv: shape(s, sm, lv)) for s in SHAPES for sm in ("centre", "node") for lv in (0.0, 0.01)}
    nanc = _small_sphere((9, 8, 7), 0.025)
    table = {
        **n24,
        "sphere_centre_-0.005": lambda: shape("sphere", "centre", -0.005),
        "2x2x2": lambda: _case(np.array([[[-1.0, 1.0], [1.0, 1.0]], [[1.0, 1.0], [1.0, 2.0]]]), (0.0, 0.0, 0.0)),
        "2x2x2_half": lambda: _case(np.array([[[-1.0, -1.0], [-1.0, -3.0]], [[1.0, 1.0], [1.0, 2.0]]]), (0.1, 0.2, 0.3), sample="node"),
        "dim1_x": lambda: _case(sphere((1, 8, 8), 0.01, "centre", 0.02)[0], (0.0, 0.0, 0.0)),
        "dim1_z": lambda: _case(sphere((6, 5, 1), 0.01, "centre", 0.02)[0], (0.0, 0.0, 0.0)),
        "z2": lambda: _small_sphere((9, 9, 2), 0.03),
        "z65": lambda: _small_sphere((5, 4, 65), 0.015, level=0.002),
        "all_inside": lambda: _case(np.full((5, 6, 7), -1.0), (0.0, 0.0, 0.0)),
        "all_outside": lambda: _case(np.full((5, 6, 7), 1.0), (0.0, 0.0, 0.0)),
        "leaves_grid": lambda: _small_sphere((8, 8, 8), 0.045),
        "nan_inside": lambda: _with(nanc, [(_near_surface(nanc, True), np.nan)]),
        # (the outside sample at the far end b of a crossing x edge: +inf there gives t = 0, NaN gives t = 0.5)
        "nan_outside": lambda: _with(nanc, [(_next_x(_near_surface(nanc, True)), np.nan)]),
        "plus_inf": lambda: _with(nanc, [(_next_x(_near_surface(nanc, True)), np.inf)]),
        "minus_inf": lambda: _with(nanc, [(_near_surface(nanc, True), -np.inf)]),
        "inf_both": lambda: _with(nanc, [(_next_x(_near_surface(nanc, False)), -np.inf), (_near_surface(nanc, False), np.inf)]),
        "equal_to_level": _equal_to_level,
        "padded": _padded,
        "cloud": _cloud,
        # around the 256-sample workgroup: the surface crosses the group border
        "252": lambda: _small_sphere((6, 6, 7), 0.022),
        "256": lambda: _small_sphere((4, 8, 8), 0.015, sample="node"),
        "294": lambda: _small_sphere((6, 7, 7), 0.024, level=0.01),
        "17x9x5": lambda: _small_sphere((17, 9, 5), 0.018, level=-0.005, centre=(0.03, 0.0, 0.0)),
        "17x9x5_node": lambda: _small_sphere((17, 9, 5), 0.03, sample="node", centre=(-0.02, 0.01, 0.0)),
    }
    if name.startswith("smooth"):
        return _smooth(int(name[6:]))
    return table[name]()


N24 = tuple(f"{s}_{sm}_{lv}" for s in SHAPES for sm in ("centre", "node") for lv in (0.0, 0.01))
EDGE = ("2x2x2", "2x2x2_half", "dim1_x", "dim1_z", "z2", "z65", "all_inside", "all_outside", "leaves_grid", "nan_inside", "nan_outside", "plus_inf",
        "minus_inf", "inf_both", "equal_to_level", "padded", "cloud")
GROUPS = ("252", "256", "294", "17x9x5", "17x9x5_node", "sphere_centre_-0.005")
SMOOTH = tuple(f"smooth{s}" for s in range(12))
ALL = N24 + EDGE + GROUPS + SMOOTH
EMPTY = ("dim1_x", "dim1_z", "all_inside", "all_outside")


@functools.lru_cache(maxsize=None)
def spec(name):
    """(verts, faces, open_edges) of scenes.surface_nets for the case; computed once and never written to."""
    from omg_planner_amd import scenes
    c = case(name)
    v, f, o = scenes.surface_nets(c["data"], c["origin"], c["delta"], c["sample"], c["level"])
    v.setflags(write=False), f.setflags(write=False)
    return v, f, o


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# what a mesh is
# ---------------------------------------------------------------------------------------------------------------------
def unpaired_directed_edges(faces):
    """Directed edges (a, b) of the faces that do not have exactly one opposite (b, a), plus those that occur more than once."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    key, back = e[:, 0] << 32 | e[:, 1], e[:, 1] << 32 | e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    return int((cnt != 1).sum() + (~np.isin(back, uniq)).sum())


def components(n_verts, faces):
    parent = np.arange(n_verts)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in faces:
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra
        parent[find(rc)] = ra
    return len({find(x) for x in range(n_verts)})


def euler(n_verts, faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return n_verts - len(np.unique(e, axis=0)) + len(faces)


def signed_volume(verts, faces):
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def zero_area_faces(verts, faces):
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    return int((np.linalg.norm(np.cross(b - a, c - a), axis=1) == 0).sum())
