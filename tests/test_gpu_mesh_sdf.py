"""omgx_mesh_sdf on the device (include/omg_hip.h section 12, ABI 14) against its host specification scenes.mesh_sdf: the float32
magnitudes bit for bit (both sides do the same IEEE float64 operations in the same order, with correctly rounded division and
square root), the signs wherever the winding number decides them; a ragged batch in one launch; a volume written straight into
the SDF pool and fitted there; and a plan through a scene whose object came from a mesh.  The host side alone is
tests/test_mesh_sdf_cpu.py."""
from __future__ import annotations

import copy
import functools

import numpy as np
import pytest

from tests import mesh_cases as MC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _tile():
    from omg_planner_amd import _lib
    return int(_lib.lib().omgx_mesh_sdf_tile())


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(verts, faces, closed)"""
    if name == "box":
        return (*MC.box_mesh(MC.BOX_HALF), True)
    if name == "rot_box":
        return (*MC.box_mesh(MC.BOX_HALF, MC.pose((0.2, 0.1, -0.3), (0.01, 0.0, 0.02))), True)
    if name == "far_box":  # translated by 1.5 m
        return (*MC.box_mesh(MC.BOX_HALF, MC.pose((1.1, 0.4, -0.7), (-0.4, 1.5, 0.25))), True)
    if name == "ico80":
        return (*MC.icosphere(1, 0.06, (0.003, -0.002, 0.001)), True)
    if name == "ico320":
        return (*MC.icosphere(2, 0.06, (0.003, -0.002, 0.001)), True)
    if name.startswith("cut"):  # the first T-1 / T / T+1 / 2T+1 faces of a 1280-face icosphere: open meshes
        T = _tile()
        n = {"cutT-1": T - 1, "cutT": T, "cutT+1": T + 1, "cut2T+1": 2 * T + 1}[name]
        v, f = MC.icosphere(3, 0.06, (0.003, -0.002, 0.001))
        assert n < len(f)
        return v, f[:n].copy(), False
    raise KeyError(name)


# mesh, delta, padding, sample, explicit (origin, dims) or None
CASES = {
    "box-centre": ("box", 0.01, 3, "centre", None),                                           # 16 x 22 x 12 = 16.5 workgroups
    "box-node-shifted": ("box", 0.01, 3, "node", ((-0.0773, -0.1081, -0.0569), (16, 23, 12))),  # no node on the surface
    "rot_box-node": ("rot_box", 0.012, 2, "node", None),
    "far_box-centre": ("far_box", 0.009, 2, "centre", None),
    "far_box-node": ("far_box", 0.011, 1, "node", None),
    "ico80-centre": ("ico80", 0.012, 2, "centre", None),                                       # 14^3 = 2744 nodes
    "ico320-node": ("ico320", 0.0123, 2, "node", None),
    "cutT-1-centre": ("cutT-1", 0.016, 1, "centre", None),
    "cutT-node": ("cutT", 0.016, 1, "node", None),
    "cutT+1-centre": ("cutT+1", 0.016, 1, "centre", None),
    "cut2T+1-node": ("cut2T+1", 0.016, 1, "node", None),
    "one-node-inside": ("rot_box", 0.01, 0, "centre", ((0.0, 0.0, 0.01), (1, 1, 1))),
    "one-node-outside": ("ico80", 0.05, 0, "node", ((0.2, -0.1, 0.05), (1, 1, 1))),
    "column-1x1x300": ("rot_box", 0.001, 0, "centre", ((0.004, 0.003, -0.15), (1, 1, 300))),
    "column-300x1x1": ("ico320", 0.001, 0, "node", ((-0.1503, 0.003, 0.002), (300, 1, 1))),
}


@functools.lru_cache(maxsize=None)
def _host(case):
    """The host specification of a case, computed once: (origin, dims, d float64 [N], w float64 [N], grid float32 [X,Y,Z])."""
    from omg_planner_amd import scenes as sc
    name, delta, padding, sample, layout = CASES[case]
    v, f, _ = _mesh(name)
    origin, dims = sc.mesh_grid_layout(v, delta, padding) if layout is None else (np.array(layout[0]), layout[1])
    d, w = sc.mesh_distance_winding(v, f, sc.mesh_nodes(origin, dims, delta, sample))
    grid = sc.mesh_sdf(v, f, delta, padding, sample, None if layout is None else layout[0], None if layout is None else layout[1])
    for a in (d, w, grid.data):
        a.setflags(write=False)
    return origin, tuple(int(x) for x in dims), d, w, grid


@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_host_specification(dev, case):
    from omg_planner_amd import ops
    name, delta, padding, sample, layout = CASES[case]
    v, f, closed = _mesh(name)
    origin, dims, d, w, want = _host(case)
    got, g_origin, g_delta = ops.mesh_sdf(v, f, delta, padding, sample, None if layout is None else layout[0],
                                          None if layout is None else layout[1], device=dev)
    assert tuple(got.shape) == dims == want.data.shape and got.dtype == torch.float32 and g_delta == delta
    np.testing.assert_array_equal(g_origin, origin)
    got = got.cpu().numpy()
    n = int(np.prod(dims))
    print(f"{case}: grid {dims} = {n} nodes ({n / 256:.2f} workgroups), {len(f)} faces, min | |w| - 0.5 | = {np.abs(np.abs(w) - 0.5).min():.3e}")
    # the magnitudes: bit for bit
    np.testing.assert_array_equal(np.abs(got).view(np.uint32), np.abs(want.data).view(np.uint32))
    # the signs: on every node of a closed mesh, and of an open one wherever the host's winding number is clear of the threshold
    assert d.min() > 0.0  # no node on the surface, where there is no sign
    gap = np.abs(np.abs(w) - 0.5)
    if closed:
        assert gap.min() > 0.4
        decided = np.ones(n, bool)
    else:
        decided = gap > 1e-3
        assert (~decided).sum() < 0.005 * n
    np.testing.assert_array_equal(np.signbit(got).ravel()[decided], np.signbit(want.data).ravel()[decided])


def test_cases_cover_what_they_should():
    """The case list keeps its promises: face counts around the tile, a node count that is no multiple of 256, the single node,
    the column, both conventions on closed and open meshes, a mesh 1.5 m from the origin."""
    from omg_planner_amd import scenes as sc
    T = _tile()
    counts = {len(_mesh(CASES[c][0])[1]) for c in CASES}
    assert {12, 80, 320, T - 1, T, T + 1, 2 * T + 1} <= counts
    dims = []
    for c, (name, delta, padding, sample, layout) in CASES.items():
        dims.append(tuple(int(x) for x in (sc.mesh_grid_layout(_mesh(name)[0], delta, padding)[1] if layout is None else layout[1])))
    assert (1, 1, 1) in dims and (1, 1, 300) in dims and any(int(np.prod(d)) % 256 and np.prod(d) > 256 for d in dims)
    for closed in (True, False):
        assert {CASES[c][3] for c in CASES if _mesh(CASES[c][0])[2] == closed} == {"centre", "node"}
    assert np.abs(_mesh("far_box")[0]).max() > 1.5


def test_ragged_batch_equals_single_launches(dev):
    """Five meshes with different face counts, dims, spacings and conventions in ONE launch, at scattered offsets of one
    buffer: every volume equals its own single launch bit for bit, and the gaps keep the pattern they held."""
    from omg_planner_amd import ops, scenes as sc
    names = ["box-centre", "cutT+1-centre", "one-node-inside", "ico80-centre", "far_box-node"]
    meshes = [_mesh(CASES[c][0])[:2] for c in names]
    deltas, pads, samples = [CASES[c][1] for c in names], [CASES[c][2] for c in names], [CASES[c][3] for c in names]
    lay = [sc.mesh_grid_layout(m[0], CASES[c][1], CASES[c][2]) if CASES[c][4] is None else CASES[c][4] for c, m in zip(names, meshes)]
    origins, dims = [np.asarray(l[0], np.float64) for l in lay], [tuple(int(x) for x in l[1]) for l in lay]
    sizes = [int(np.prod(d)) for d in dims]
    order = [3, 0, 4, 1, 2]  # where the volumes go: not in batch order, with gaps of different sizes between them
    offsets, at = [0] * 5, 7
    for m in order:
        offsets[m] = at
        at += sizes[m] + 1 + 100 * m
    total = at + 13
    sentinel = torch.arange(total, dtype=torch.float32, device=dev) * 0.5 + 1000.0
    buf = sentinel.clone()
    grids, g_origins, g_deltas, dropped = ops.mesh_sdf_batch(meshes, deltas, pads, samples, origins, dims, out=buf, out_offsets=offsets)
    assert dropped == [0] * 5 and g_deltas == deltas
    written = torch.zeros(total, dtype=torch.bool, device=dev)
    for m, c in enumerate(names):
        single, _, _ = ops.mesh_sdf(*meshes[m], deltas[m], pads[m], samples[m], origins[m], dims[m], device=dev)
        assert grids[m].data_ptr() == buf.data_ptr() + 4 * offsets[m] and tuple(grids[m].shape) == dims[m]
        assert torch.equal(grids[m].view(torch.int32), single.view(torch.int32)), c
        np.testing.assert_array_equal(np.abs(single.cpu().numpy()), np.abs(_host(c)[4].data))
        written[offsets[m]: offsets[m] + sizes[m]] = True
    assert int((~written).sum()) == total - sum(sizes) and torch.equal(buf[~written], sentinel[~written])
    # without `out` the volumes lie back to back in one buffer
    flat, _, _, _ = ops.mesh_sdf_batch(meshes, deltas, pads, samples, origins, dims, device=dev)
    for m in range(5):
        assert torch.equal(flat[m].view(torch.int32), grids[m].view(torch.int32))
        assert flat[m].data_ptr() == flat[0].data_ptr() + 4 * sum(sizes[:m])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _box_scene(sdf, table):
    from omg_planner_amd import scenes as sc
    return sc.Scene([sc.SceneObject("obj_0", sc._yaw_pose(0.5, 0.1, 0.15, 0.4), sdf), sc.SceneObject("table", sc._yaw_pose(0.5, 0.0, 0.02, 0.0), table)], 0)


def test_in_place_into_the_pool_and_fitted_there(dev):
    """ops.mesh_sdf(out=DeviceScenes.grid_slot(...)) writes the pool, replace_grid fits the influence region on the device: the
    record equals the one DeviceScenes.from_scenes builds from the host specification's SdfGrid."""
    from omg_planner_amd import ops, scenes as sc
    v, f, _ = _mesh("rot_box")
    delta, padding = 0.012, 4
    host = sc.mesh_sdf(v, f, delta, padding)
    table = sc.box_sdf((0.6, 0.4, 0.02), (48, 32, 16), 1.5 / 48)
    want = ops.DeviceScenes.from_scenes([_box_scene(host, table)], device=dev)
    torch.cuda.synchronize()
    want_rec = want.sync_host()[0]
    ds = ops.DeviceScenes.from_scenes([_box_scene(sc.sphere_sdf(0.05, (8, 8, 8), 0.05), table)], device=dev, reserve_voxels=host.data.size)
    origin, dims = sc.mesh_grid_layout(v, delta, padding)
    slot = ds.grid_slot(0, 0, dims)
    version = slot._version
    grid, g_origin, g_delta = ops.mesh_sdf(v, f, delta, padding, out=slot)
    assert grid.data_ptr() == slot.data_ptr() and slot._version > version
    ds.replace_grid(0, 0, grid, g_origin, g_delta, fit="device")
    torch.cuda.synchronize()
    got_rec = ds.sync_host()[0]
    off = int(got_rec["grid_offset"])
    assert torch.equal(ds.pool[off: off + host.data.size].view(torch.int32), torch.from_numpy(host.data.ravel()).to(dev).view(torch.int32))
    for name in ("lo", "hi", "dim", "delta", "inv_extent", "inv_delta", "pose_inv", "epsilon", "clearance", "rb_c", "rb_h", "rb_r", "rb_r2"):
        assert np.array_equal(got_rec[name], want_rec[name]), (name, got_rec[name], want_rec[name])
    with pytest.raises(Exception):
        ops.mesh_sdf(v, f, delta, padding, out=slot.reshape(-1)[:-1])  # a view of the wrong size is refused


def test_through_the_planner(dev):
    """Table slab + a box built from its mesh, S = 2 scenes, 8 goals, 30 waypoints: the table built by replace_grid from the device
    volume, by from_scenes from the host specification's SdfGrid and by from_scenes from the analytic box_sdf grid give the same
    collision statistics and the same plan, bit for bit."""
    from omg_planner_amd import goalset, ops, robot as rb, scenes as sc
    from omg_planner_amd.config import Config
    from omg_planner_amd.engine import ChompEngine
    S, G, n = 2, 8, 30
    half, shape, delta = MC.BOX_HALF, (32, 32, 32), 0.6 / 32
    analytic = sc.box_sdf(half, shape, delta)
    v, f = MC.box_mesh(half)
    host = sc.mesh_sdf(v, f, delta, sample="centre", origin=analytic.origin, dims=shape)
    np.testing.assert_array_equal(host.data.view(np.uint32), analytic.data.view(np.uint32))  # (test_mesh_sdf_cpu.py asserts it on the CPU too)
    table = sc.box_sdf((0.6, 0.4, 0.02), (48, 32, 16), 1.5 / 48)
    model = rb.PandaModel(seed=0)
    cfg = Config(timesteps=n, use_standoff=False)
    cfg.optim_steps, cfg.timeout = 10, -1
    kw = cfg.layer_kwargs()
    start = np.tile(rb.HOME_CONFIG, (S, 1))
    goals = np.stack([sc.make_goal_set(s, G) for s in range(S)])
    robot = ops.robot_blob(model, dev)

    def scenes_with(sdf):
        out = [_box_scene(sdf, table) for _ in range(S)]
        out[1].objects[0].pose_mat = sc._yaw_pose(0.42, -0.12, 0.16, -0.9)
        return out
    tables = {"host": ops.DeviceScenes.from_scenes(scenes_with(host), kw, dev), "analytic": ops.DeviceScenes.from_scenes(scenes_with(analytic), kw, dev)}
    ds = ops.DeviceScenes.from_scenes(scenes_with(sc.sphere_sdf(0.05, (8, 8, 8), 0.05)), kw, dev, reserve_voxels=2 * host.data.size)
    slots = [ds.grid_slot(s, 0, shape) for s in range(S)]
    offs = [(slots[s].data_ptr() - ds.pool.data_ptr()) // 4 for s in range(S)]
    grids, origins, deltas, _ = ops.mesh_sdf_batch([(v, f)] * S, delta, 0, "centre", [analytic.origin] * S, [shape] * S, out=ds.pool, out_offsets=offs)
    for s in range(S):
        assert grids[s].data_ptr() == slots[s].data_ptr()
        assert torch.equal(grids[s].view(torch.int32), torch.from_numpy(host.data).to(dev).view(torch.int32))
        ds.replace_grid(s, 0, grids[s], origins[s], deltas[s], fit="device")
    tables["device"] = ds
    results = {}
    for name, tab in tables.items():
        col, pot = goalset.goal_collision_stats(robot, model.points_per_link, tab, torch.as_tensor(goals, device=dev))
        eng = ChompEngine(model, tab, copy.deepcopy(cfg), start, goals, device=dev, ol_alg="MD")
        eng.plan(early_stop=False)
        torch.cuda.synchronize()
        results[name] = (col.clone(), pot.clone(), eng.traj.clone(), eng.info.clone(), eng.goal_idx.clone())
    assert float(results["host"][1].abs().sum()) > 0  # the box and the table are within reach of the goals
    for name in ("device", "analytic"):
        for a, b, what in zip(results[name], results["host"], ("collide", "potentials", "traj", "info", "goal_idx")):
            assert _same_bits(a, b), (name, what)
