"""Goal-set selection without a GPU: the exactness argument behind omgx_select_goals (numpy's summation order of a 9-vector's
norm, and `norm < 0.5` <=> `sum < 0.25`), a numpy restatement of the kernel's blocked walk against goalset.select_goals and the
reference's own setup_goal_set (tests/golden/setup_*.npz, tests/golden/make_setup_golden.py), the batched draw against a loop
of the reference's planners, ops.select_goals' argument checks and the selection kernel's register budget."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from omg_planner_amd import goalset
from tests import kernel_build as KB

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
FIXTURES = sorted(GOLDEN.glob("setup_*.npz"))


def dist2(a, b):
    """The kernel's squared distance: nine squares summed (((0+1)+(2+3))+((4+5)+(6+7)))+8."""
    q = (a - b) ** 2
    return (((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) + ((q[..., 4] + q[..., 5]) + (q[..., 6] + q[..., 7]))) + q[..., 8]


class TakeAll:
    """An rng whose choice returns the population in order: select_goals' `chosen` is then the reference's `indexes`."""

    def choice(self, a, k, replace=False):
        return (np.arange(a) if np.isscalar(a) else np.asarray(a))[:k]


def reference_rows(goals, collide, allow=5, fc=True, fd=True):
    """The rows (of `goals`) the reference's `indexes` name, through goalset.select_goals."""
    n = len(goals)
    col = np.zeros(n, np.float32) if collide is None else np.asarray(collide)
    _, _, _, chosen = goalset.select_goals(list(goals), list(goals), col, np.zeros(n, np.float32), allow, 10 ** 9, fc, fd, TakeAll())
    free = np.flatnonzero(col <= allow) if fc else np.arange(n)
    return free[np.asarray(chosen, np.int64)]


def blocked_rows(goals, collide, allow=5, fc=True, fd=True, block=64):
    """The kernel's walk (omg_goal_select.hip): compaction, then blocks of 64 — (a) against the kept set of earlier blocks,
    (b) the in-block masks and the ordered scan, (c) append; kept free[p] emits free[p - 1]."""
    g = np.asarray(goals, np.float64).reshape(-1, 9)
    n = g.shape[0]
    free = np.flatnonzero(np.asarray(collide)[:n] <= allow) if (fc and collide is not None) else np.arange(n)
    if not fd or free.size == 0:
        return free if not fd else free[:0]
    kept, out = [free[0]], []
    for p0 in range(1, free.size, block):
        ps = np.arange(p0, min(p0 + block, free.size))
        c = g[free[ps]]
        near = (dist2(g[np.array(kept)][None, :, :], c[:, None, :]) < 0.25).any(axis=1)
        close = dist2(c[None, :, :], c[:, None, :]) < 0.25  # [l, j]
        keep = np.zeros(ps.size, bool)
        for j in range(ps.size):
            keep[j] = not near[j] and not (close[j, :j] & keep[:j]).any()
        for j in np.flatnonzero(keep):
            kept.append(free[ps[j]])
            out.append(free[ps[j] - 1])
    return np.array(out, np.int64)


def goal_sets(kind, n, rng):
    if kind == "random":
        return rng.uniform(-1.0, 1.0, (n, 9))
    if kind == "clustered":
        centres = rng.uniform(-2.0, 2.0, (max(1, n // 12), 9))
        return centres[rng.randint(len(centres), size=n)] + rng.normal(0, 0.2, (n, 9))
    # adversarial: pairs at 0.5 +- a few ulp from a chain of base points, in random directions
    base = rng.uniform(-3, 3, (max(1, (n + 1) // 2), 9))
    u = rng.normal(size=base.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 0.5 + rng.randint(-4, 5, size=(len(base), 1)) * np.finfo(float).eps
    g = np.concatenate([base, base + u * r])[:n]
    return g[rng.permutation(len(g))]


def test_numpy_norm_sums_in_the_kernel_order():
    rng = np.random.RandomState(0)
    for rows in (1, 7, 64, 69):
        d = rng.normal(0, 0.3, (rows, 9))
        assert np.array_equal(np.linalg.norm(d, axis=-1), np.sqrt(dist2(d, 0.0)))
    d = rng.normal(0, 0.3, (200_000, 9)) * rng.uniform(0.01, 3, (200_000, 1))
    assert np.array_equal(np.linalg.norm(d, axis=-1), np.sqrt(dist2(d, 0.0)))
    assert np.array_equal(np.linalg.norm(d, axis=-1) < 0.5, dist2(d, 0.0) < 0.25)


def test_squared_threshold_is_exact_at_the_boundary():
    below = np.nextafter(0.25, 0.0)  # 0.25 - 2**-55
    assert np.sqrt(below) < 0.5 and np.sqrt(0.25) == 0.5 and np.sqrt(np.nextafter(0.25, 1.0)) >= 0.5
    rng = np.random.RandomState(1)
    d = rng.normal(0, 0.1, (20_000, 9))
    d[:, :8] *= 0.4 / np.sqrt((d[:, :8] ** 2).sum(1, keepdims=True))  # |d[:8]| = 0.4: d8 ~ 0.3 closes the norm at 0.5
    p8 = (((d[:, 0] ** 2 + d[:, 1] ** 2) + (d[:, 2] ** 2 + d[:, 3] ** 2)) + ((d[:, 4] ** 2 + d[:, 5] ** 2) + (d[:, 6] ** 2 + d[:, 7] ** 2)))
    d[:, 8] = np.sqrt(0.25 - p8)
    for k in range(-6, 7):
        e = d.copy()
        e[:, 8] = e[:, 8] + k * np.spacing(e[:, 8])
        s = dist2(e, 0.0)
        assert np.array_equal(np.linalg.norm(e, axis=-1) < 0.5, s < 0.25)


@pytest.mark.parametrize("kind", ["random", "clustered", "adversarial"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 40, 200, 700])
def test_restatement_equals_select_goals(kind, n):
    rng = np.random.RandomState(1000 * ["random", "clustered", "adversarial"].index(kind) + n)
    g = goal_sets(kind, n, rng)
    col = rng.randint(0, 9, n).astype(np.float32)
    for fc in (True, False):
        for fd in (True, False):
            want = reference_rows(g, col, 5, fc, fd)
            got = blocked_rows(g, col, 5, fc, fd)
            assert np.array_equal(got, want), (kind, n, fc, fd)


def test_restatement_edge_cases():
    rng = np.random.RandomState(3)
    g = rng.uniform(-1, 1, (50, 9))
    col = np.full(50, 9.0, np.float32)  # every row colliding
    assert reference_rows(g, col).size == 0 and blocked_rows(g, col).size == 0
    one = np.tile(g[:1], (30, 1)) + 1e-3 * rng.normal(size=(30, 9))  # exactly one diverse goal: "IK FAIL"
    assert reference_rows(one, None).size == 0 and blocked_rows(one, None).size == 0
    grid = np.eye(9)[None].repeat(20, 0).reshape(-1, 9) * np.arange(1, 181)[:, None]  # 180 goals, all far apart
    for m in (63, 64, 65, 128, 129):  # blocks ending at 63, 64 and 65 candidates
        gg = grid[:m + 1]
        want = reference_rows(gg, None)
        assert want.size == m and np.array_equal(blocked_rows(gg, None), want)
        assert np.array_equal(want, np.arange(m))  # the off-by-one: kept goal p emits p - 1


def test_batched_draw_equals_a_loop_of_the_reference():
    """draw_positions over S scenes on one RandomState = select_goals scene after scene on another with the same seed, including
    scenes that skip the draw (no candidates) and scenes with more candidates than goal_set_max_num."""
    rng = np.random.RandomState(11)
    sets = [goal_sets("clustered", n, rng) for n in (0, 300, 1, 60, 500, 2, 250)]
    cols = [rng.randint(0, 8, len(g)).astype(np.float32) for g in sets]
    loop_rng, batch_rng = np.random.RandomState(5), np.random.RandomState(5)
    want = []
    for g, c in zip(sets, cols):
        grasps, _, _, _ = goalset.select_goals(list(g), list(g), c, np.zeros(len(g), np.float32), 5, 40, rng=loop_rng)
        want.append(np.array(grasps).reshape(-1, 9))
    rows = [blocked_rows(g, c) for g, c in zip(sets, cols)]
    pos, k = goalset.draw_positions([r.size for r in rows], 40, batch_rng)
    assert k.tolist() == [len(w) for w in want] and 0 in k.tolist() and 40 in k.tolist()
    for s in range(len(sets)):
        assert np.array_equal(sets[s][rows[s][pos[s, :k[s]]]], want[s])
    assert loop_rng.randint(1 << 30) == batch_rng.randint(1 << 30)  # the streams were consumed alike


def _fixture_objects(d):
    return [o for o in range(int(d["num_objects"]))]


@pytest.mark.parametrize("path", FIXTURES, ids=[p.stem for p in FIXTURES])
def test_restatement_reproduces_reference_fixture(path):
    """The reference's own setup_goal_set (make_setup_golden.py) picked goals = blocked_rows + draw_positions on its seed."""
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    rng = np.random.RandomState(int(d["seed"]))
    for o in _fixture_objects(d):
        g = d[f"goals_{o}"]
        if not (len(g) > 0 and bool(d[f"compute_grasp_{o}"])):
            continue
        rows = blocked_rows(g, d[f"collide_{o}"], float(d["allow_collision_point"]), bool(d["filter_collision"]),
                            bool(d["filter_diversity"]))
        pos, k = goalset.draw_positions([rows.size], int(d["goal_set_max_num"]), rng)
        pick = rows[pos[0, :k[0]]]
        assert np.array_equal(g[pick].reshape(-1, 9), d[f"out_grasps_{o}"].reshape(-1, 9)), o
        assert np.array_equal(d[f"pot_{o}"][pick], d[f"out_potentials_{o}"].reshape(-1)), o
        assert np.array_equal(d[f"reach_{o}"][pick].reshape(-1), d[f"out_reach_{o}"].reshape(-1)), o


def test_fixtures_cover_the_issue_cases():
    names = {p.stem for p in FIXTURES}
    assert {"setup_standoff", "setup_nostandoff", "setup_nocollision", "setup_nodiversity", "setup_ikfail"} <= names
    with np.load(GOLDEN / "setup_ikfail.npz", allow_pickle=False) as z:
        assert any(int(z[f"out_count_{o}"]) == 0 and len(z[f"goals_{o}"]) > 0 for o in range(int(z["num_objects"])))


def test_select_goals_argument_checks_without_gpu():
    import torch
    from omg_planner_amd import _lib, ops
    g = torch.zeros((2, 5, 9), dtype=torch.float64)
    E = _lib.OmgHipError
    with pytest.raises(E, match="S, G, 9"):
        ops.select_goals(torch.zeros((2, 5, 8), dtype=torch.float64), [1, 1])
    with pytest.raises(E, match="float64"):
        ops.select_goals(g.float(), [1, 1])
    with pytest.raises(E, match="S integers"):
        ops.select_goals(g, [1, 1, 1])
    with pytest.raises(E, match="S integers"):
        ops.select_goals(g, [1.0, 2.0])
    with pytest.raises(E, match="lie in"):
        ops.select_goals(g, [1, 6])
    with pytest.raises(E, match="lie in"):
        ops.select_goals(g, [-1, 2])
    with pytest.raises(E, match="S, G"):
        ops.select_goals(g, [1, 1], torch.zeros((2, 4), dtype=torch.float32))
    with pytest.raises(E, match="float32"):
        ops.select_goals(g, [1, 1], torch.zeros((2, 5), dtype=torch.float64))
    with pytest.raises(E, match="NaN"):
        ops.select_goals(g, [1, 1], None, float("nan"))
    with pytest.raises(E, match="device tensor"):
        ops.select_goals(g, [1, 1])


def test_select_goals_abi_checks_without_gpu():
    from omg_planner_amd import _lib
    lib = _lib.lib()
    d = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first or launches nothing

    def call(S=2, G=4, counts=(1, 2), div=1, allow=5.0, ws=d, out=d):
        hc = (C.c_int32 * len(counts))(*counts) if counts is not None else None
        return lib.omgx_select_goals(d, d, hc, S, G, None, allow, div, out, d, d, ws, None)

    INV = _lib.OMGX_ERR_INVALID
    assert call(S=-1) == INV and call(G=-1) == INV and call(G=(1 << 24) + 1) == INV
    assert call(counts=(1, 5)) == INV and call(counts=(-1, 0)) == INV
    assert call(div=2) == INV and call(allow=float("nan")) == INV
    assert call(ws=None) == INV and call(out=None) == INV
    assert call(S=0, counts=()) == _lib.OMGX_OK  # nothing to select: nothing launched
    assert lib.omgx_select_goals_workspace_bytes(100, 855) == 100 * 855 * 8
    assert lib.omgx_select_goals_workspace_bytes(0, 855) == 0 and lib.omgx_select_goals_workspace_bytes(3, 0) == 0


@KB.requires_hipcc
def test_select_kernel_does_not_spill(tmp_path):
    """k_select_goals keeps a candidate's nine doubles and the block masks in registers: no scratch."""
    v = KB.one(KB.kernel_resources("omg_goal_select.hip", tmp_path), "k_select_goals")
    assert v["ScratchSize [bytes/lane]"] == 0
    assert v["Occupancy [waves/SIMD]"] >= 1
