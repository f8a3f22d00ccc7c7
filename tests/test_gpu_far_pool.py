"""The pool kernels with their volumes beyond 2^32 elements (tests/far_pool.py explains the buffer and why exactly these
placements; read its docstring before adding one).  Every volume lies at a 64-bit element offset (omgx_object.grid_offset,
omgx_mesh.out_offset, state_begin / comp_begin / out_begin) to which a 32-bit node index is added, in about forty places that
carry the base in very different ways.  For every entry point below the call on a table whose volumes lie at B1 = 2^30 + 4099
(byte offsets pass 2^32) or B2 = 2^32 + 4099 (element offsets pass 2^32) of one 16.1 GiB buffer must leave the SAME BITS as the
call on the compact table — outputs, statuses, counts, records, and for writers the volumes at the far place — and touch nothing
else: the alias window, where an offset cut to 32 bits lands, and a band around every far volume hold a guard pattern afterwards.
The expected value is the compact run (the other GPU modules pin that one to the specifications), so the tolerance is zero.
Every group has a control: records pointed at the alias window on purpose must give other bits, else the group proves nothing.

The one skip of the module: less free device memory than the buffer and 2 GiB.  omgx_label_components sets every label of the
state array to -1 before it labels (its contract for elements outside the volumes), so labels cannot share the buffer: the
wrapper's own label array of state.numel() int32 elements is alive beside the buffer during the three segmentation tests."""
from __future__ import annotations

import copy
import time

import numpy as np
import pytest

from tests import far_pool as FP
from tests import fusion_cases as FC
from tests import mesh_cases as MC
from tests import plane_cases as PC
from tests import register_cases as RC
from tests import segment_cases as SC
from tests import surface_cases as SFC
from tests import tsdf_cases as TC
from tests import volume_camera_cases as VC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BASES = pytest.mark.parametrize("base", FP.BASES, ids=["B1", "B2"])
STATE = ("traj", "info", "goal_idx", "learner_state", "goal_cost", "end", "goal_rows", "cost_traj", "grad", "pot", "col")  # test_gpu_pipeline._assert_same's
PLANNER_STATE = STATE + ("pgrad", "goal_col", "active")
MODES = {"fused": {}, "serial": {}, "latency": dict(latency_mode=True), "split2": dict(goal_parts=2), "split4": dict(goal_parts=4),
         "prepass": dict(prepass=True), "persistent": {}}
ALL_FINE = {"far": True, "bands": True, "alias": True}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


class _Far:
    """The buffer, handed out lane by lane; dropped in the fixture's teardown."""

    def __init__(self, buf):
        self.buf = buf

    def lane(self, j, dtype=torch.float32):
        return FP.lane(self.buf, j, dtype)


@pytest.fixture(scope="module")
def far(dev):
    import test_gpu_pipeline
    assert STATE == test_gpu_pipeline.STATE
    free, total = torch.cuda.mem_get_info(dev)
    need = 4 * FP.ELEMS + FP.HEADROOM
    if free < need:
        pytest.skip(f"the far-pool buffer needs {need} bytes of free device memory (4 * (2^32 + {FP.RESERVE}) and 2 GiB), {free} of {total} are free")
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    holder = _Far(torch.empty(FP.ELEMS, dtype=torch.float32, device=dev))
    yield holder
    torch.cuda.synchronize(dev)
    print(f"\nfar pool: peak torch.cuda.max_memory_allocated {torch.cuda.max_memory_allocated(dev)} bytes "
          f"({torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB), module wall time {time.perf_counter() - t0:.1f} s")
    holder.buf = None
    torch.cuda.empty_cache()


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b) -> bool:
    """Equal bits, tensor or array, NaNs included; None equals None."""
    if a is None or b is None:
        return a is None and b is None
    a, b = (_np(x) if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(got, want) -> bool:
    return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))


def _written(view, base, compact):
    torch.cuda.synchronize()
    return FP.written(view, base, compact)


# =====================================================================================================================
# 1. planner kernels through DeviceScenes.over_pool
# =====================================================================================================================
@pytest.fixture(scope="module")
def workload():
    import bench
    cfg, model, batch, start, goals = bench.build_workload(3, 8, 12, 32, 0, False)
    assert batch.pool.size <= FP.MAX_USED and batch.objects["grid_offset"].max() > 0
    return cfg, model, batch, start, goals


def _table(far, workload, base, delta=None):
    """The workload's table around lane 0: the pool at `base`, its negation in the alias window; records moved by `delta`
    (default: to the base; FP.K: the control, pointed at the alias window)."""
    from omg_planner_amd import ops
    batch = workload[2]
    view = far.lane(0)
    FP.place(view, np.asarray(batch.pool, np.float32), base)
    return ops.DeviceScenes.over_pool(FP.relocate(batch.objects, base if delta is None else delta), batch.scene_begin, view)


def _plan(dev, workload, table, mode):
    """Three iterations of an engine on `table` in a launch variant -> the state as host arrays (and the persistent status)."""
    from omg_planner_amd.engine import ChompEngine
    cfg, model, batch, start, goals = workload
    eng = ChompEngine(model, table, copy.deepcopy(cfg), start, goals, device=dev, ol_alg="MD", **MODES[mode])
    assert eng.scenes is table
    status = None
    if mode == "serial":
        eng.separate_launches = True
    if mode == "persistent":
        assert eng.persistent_ok()
        eng.select_initial_goal()
        eng.pose_hand_over(True)
        eng.run_persistent(range(3))
        status = eng.persistent_status()
    else:
        for t in range(3):
            eng.iterate(t)
    eng.join()
    torch.cuda.synchronize()
    out = {k: _np(getattr(eng, k)).copy() for k in PLANNER_STATE}
    out["status"] = status
    return out


_COMPACT_PLANS: dict = {}


def _compact_plan(dev, workload, mode):
    from omg_planner_amd import ops
    if mode not in _COMPACT_PLANS:
        _COMPACT_PLANS[mode] = _plan(dev, workload, ops.DeviceScenes(workload[2], dev), mode)
    return _COMPACT_PLANS[mode]


def _plans_differ(a, b):
    return [k for k in PLANNER_STATE if not _same(a[k], b[k])]


@BASES
@pytest.mark.parametrize("mode", list(MODES))
def test_engine_iterations_on_a_far_table(dev, far, workload, base, mode):
    """fused, serial, latency, split2, split4 (test_engine_plan_matches_reference_planner_loop's variants), the kinematics pre-pass
    and one persistent launch: goal costs (the goal-set queue's staged byte offset) and pot, pgrad, col (the layer's
    pool + grid_offset) among the state."""
    want = _compact_plan(dev, workload, mode)
    # the compact run reaches the pool at all: potentials that are not zero and points in collision
    assert np.count_nonzero(want["pot"]) > 0 and (want["col"] > 0).any() and np.isfinite(want["goal_cost"]).all()
    got = _plan(dev, workload, _table(far, workload, base), mode)
    assert _plans_differ(got, want) == []
    if mode == "persistent":
        assert got["status"] == want["status"] and got["status"]["failure"] == 0 and got["status"]["scenes_planned"] == 3, got["status"]


@BASES
def test_planner_entry_points_called_directly_and_the_control(dev, far, workload, base):
    """ops.fk_sdf and ops.goalset_cost on the far table, and the group's control: the records pointed at the alias window (the
    negated pool) give other costs, other layer outputs and another plan."""
    from omg_planner_amd import ops
    cfg, model, batch, start, goals = workload
    robot, P, n = ops.robot_blob(model, dev), model.points_per_link, cfg.timesteps
    joints = torch.from_numpy(np.ascontiguousarray(np.linspace(start, goals[:, 0], n).transpose(1, 0, 2))).to(dev)
    d_goals = torch.from_numpy(np.ascontiguousarray(goals, np.float64)).to(dev)

    def direct(table):
        layer = ops.fk_sdf(robot, P, table, joints)
        cost, col, _ = ops.goalset_cost(robot, P, table, joints[:, 0], d_goals, n, cfg.time_interval)
        pre, pre_col, _ = ops.goalset_cost(robot, P, table, joints[:, 0], d_goals, n, cfg.time_interval, prepass=True)
        torch.cuda.synchronize()
        return tuple(_np(x) for x in (*layer, cost, col, pre, pre_col))

    want = direct(ops.DeviceScenes(batch, dev))
    # (pot, grad, col, goal cost, goal collides, and the last two through the pre-pass)
    assert np.count_nonzero(want[0]) > 0 and (want[2] > 0).any() and (want[3] > 0).any() and _same(want[3], want[5]) and _same(want[4], want[6])
    got = direct(_table(far, workload, base))
    assert _all_same(got, want)
    alias = _table(far, workload, base, delta=FP.K)
    ctrl = direct(alias)
    assert not _same(ctrl[0], want[0]) and not _same(ctrl[1], want[1]) and not _same(ctrl[3], want[3]) and not _same(ctrl[5], want[5])
    plan = _plan(dev, workload, alias, "fused")
    differ = _plans_differ(plan, _compact_plan(dev, workload, "fused"))
    assert {"goal_cost", "pot", "traj"} <= set(differ), differ


# =====================================================================================================================
# 2. scene kernels
# =====================================================================================================================
def _hashes(table):
    from omg_planner_amd import _lib, ops
    n = len(table.host_objects)
    out = torch.empty((n, 2), dtype=torch.int64, device=table.device)
    _lib.check(_lib.lib().omgx_volume_hashes(ops._ptr(table.objects), n, ops._ptr(table.pool), ops._ptr(out), ops._stream()), "omgx_volume_hashes")
    return _np(out)


def _records_without_offset(rec):
    return [np.ascontiguousarray(rec[name]).tobytes() for name in rec.dtype.names if name != "grid_offset"]


@BASES
def test_scene_kernels_on_a_far_table(dev, far, workload, base):
    """omgx_volume_hashes and omgx_fit_influence_regions (fit_all), then a moved object and one layer launch."""
    from omg_planner_amd import ops, scenes as S
    cfg, model, batch, start, goals = workload
    robot, P = ops.robot_blob(model, dev), model.points_per_link
    joints = torch.from_numpy(np.ascontiguousarray(np.linspace(start, goals[:, 0], cfg.timesteps).transpose(1, 0, 2))).to(dev)
    pose = S._yaw_pose(0.45, 0.05, 0.3, 0.7)

    def run(table):
        h = _hashes(table)
        fits = table.fit_all()
        rec = table.sync_host().copy()
        table.set_object_pose(1, 2, pose)
        layer = ops.fk_sdf(robot, P, table, joints)
        torch.cuda.synchronize()
        return h, fits, rec, table.sync_host().copy(), tuple(_np(x) for x in layer)

    compact_pool = torch.from_numpy(np.ascontiguousarray(batch.pool, np.float32).reshape(-1)).to(dev)
    want = run(ops.DeviceScenes.over_pool(batch.objects, batch.scene_begin, compact_pool))
    got = run(_table(far, workload, base))
    assert want[1] > 0 and np.count_nonzero(want[4][0]) > 0
    assert _same(got[0], want[0]) and got[1] == want[1] and _all_same(got[4], want[4])
    for g, w in ((got[2], want[2]), (got[3], want[3])):
        assert _records_without_offset(g) == _records_without_offset(w)
        assert np.array_equal(g["grid_offset"], w["grid_offset"] + base)
    assert not _same(want[2]["pose_inv"], want[3]["pose_inv"])
    # the control: hashes, fitted regions and the layer of the records that point at the negated pool
    ctrl = run(_table(far, workload, base, delta=FP.K))
    assert not _same(ctrl[0], want[0]) and _records_without_offset(ctrl[2]) != _records_without_offset(want[2]) and not _same(ctrl[4][0], want[4][0])


# =====================================================================================================================
# 3. readers of volumes
# =====================================================================================================================
def _over(far, objects, begin, pool, base, delta=None, lane=0):
    from omg_planner_amd import ops
    view = far.lane(lane)
    FP.place(view, np.asarray(pool, np.float32), base)
    return ops.DeviceScenes.over_pool(FP.relocate(objects, base if delta is None else delta), begin, view)


@BASES
def test_register_clouds_on_a_far_table(dev, far, base):
    from omg_planner_amd import ops, registration as reg
    c = RC.call("box16_257")
    c = dict(c, obj_index=c["obj_index"][:1], poses0=c["poses0"][:1], ranges=c["ranges"][:1])  # one pair, 257 points
    assert int(c["ranges"][0, 1] - c["ranges"][0, 0]) == 257
    begin = np.array([0, len(c["objects"])], np.int32)
    want = RC.device_register(c, dev)
    torch.cuda.synchronize()
    assert float(want[1][0, reg.COUNT0]) >= 6
    got = RC.device_register(c, dev, ds=_over(far, c["objects"], begin, c["pool"], base))
    assert _all_same(got, want)
    ctrl = RC.device_register(c, dev, ds=_over(far, c["objects"], begin, c["pool"], base, delta=FP.K))
    assert not _same(ctrl[0], want[0]) and not _same(ctrl[1], want[1])


@pytest.fixture(scope="module")
def two_spheres():
    """(objects, scene_begin, pool, camera rows [1,16]): one scene of a 16^3 and a 9 x 12 x 10 sphere volume side by side, seen by a
    32 x 24 camera that stands 0.45 in front of them."""
    from omg_planner_amd import camera
    a, lo_a = SFC.sphere((16, 16, 16), 0.01, "centre", 0.05)
    b, lo_b = SFC.sphere((9, 12, 10), 0.01, "centre", 0.03)
    at = lambda x, y, z: np.array([[1.0, 0, 0, x], [0, 1.0, 0, y], [0, 0, 1.0, z], [0, 0, 0, 1.0]])
    objects, begin, pool = VC.pack([[(a, lo_a, 0.01, at(-0.07, 0.0, 0.0), 0), (b, lo_b, 0.01, at(0.07, 0.01, 0.0), 0)]], gap=3)
    cfw = np.eye(4)
    cfw[:3, 3] = (0.0, 0.0, 0.45)
    return objects, begin, pool, camera.camera_rows((40.0, 40.0, 15.5, 11.5), cfw)[None]


@BASES
def test_render_volumes_on_a_far_table(dev, far, two_spheres, base):
    from omg_planner_amd import ops
    objects, begin, pool, cams = two_spheres

    def render(table):
        out = ops.render_volumes(table, cams, 24, 32, want_normals=True, want_steps=True, **VC.RAGGED_ARGS)
        torch.cuda.synchronize()
        return tuple(_np(x) for x in out)

    want = render(ops.DeviceScenes.over_pool(objects, begin, torch.from_numpy(pool).to(dev)))
    assert (want[1] == 0).any() and (want[1] == 1).any() and (want[1] == -1).any() and np.isfinite(want[0][want[1] >= 0]).all()
    assert _all_same(render(_over(far, objects, begin, pool, base)), want)
    ctrl = render(_over(far, objects, begin, pool, base, delta=FP.K))
    assert not _same(ctrl[0], want[0]) and not _same(ctrl[1], want[1])


@BASES
def test_surface_extraction_on_far_volumes(dev, far, two_spheres, base):
    """ops.surface_meshes on far layouts and DeviceScenes.object_surfaces on the far table: vertices, faces, rows, open edges."""
    from omg_planner_amd import ops
    objects, begin, pool, _ = two_spheres
    layouts = [(objects["lo"][i].astype(np.float64), float(objects["delta"][i]), "centre", tuple(int(d) for d in objects["dim"][i]),
                int(objects["grid_offset"][i])) for i in range(2)]
    compact = torch.from_numpy(pool).to(dev)
    want = ops.surface_meshes(compact, layouts)
    want_t = ops.DeviceScenes.over_pool(objects, begin, compact).object_surfaces()
    torch.cuda.synchronize()
    assert want[2][:, 1].min() > 0 and want[3][:, 1].min() > 0 and (want[4] == 0).all() and _all_same(want, want_t)
    table = _over(far, objects, begin, pool, base)
    assert _all_same(ops.surface_meshes(table.pool, FP.relocate(layouts, base)), want)
    assert _all_same(table.object_surfaces(), want)
    ctrl = ops.surface_meshes(table.pool, FP.relocate(layouts, FP.K))  # the negated spheres: the same vertices, the faces turned
    assert not _same(ctrl[1], want[1])


@BASES
def test_grasp_poses_probe_a_far_pool(dev, far, base):
    """omgx_grasp_poses with 100 probe points in volumes that omgx_mesh_sdf wrote: a small sphere and a box, 128 contact pairs each."""
    from omg_planner_amd import grasps as G, ops
    cone = np.deg2rad(15.0)
    meshes, rows = [], []
    for m, (v, f) in enumerate((MC.icosphere(2, 0.025), MC.box_mesh(MC.BOX_HALF))):
        v, f = G.outward_mesh(v, f)
        rng = np.random.RandomState(m)
        p1, _, n1 = G.surface_samples(v, f, 128, rng)
        d = G.ray_directions(n1, cone, rng)
        t, f2 = G.mesh_raycast(v, f, p1, d)
        meshes.append((v, f)), rows.append(dict(p1=p1, n1=n1, d=d, t=t, f2=f2, nrm=G.face_normals(v, f)[0]))
    up = lambda key, dtype=np.float64: torch.from_numpy(np.ascontiguousarray(np.concatenate([r[key] for r in rows]), dtype)).to(dev)
    from omg_planner_amd import scenes as sc
    samples = ["centre", "node"]
    sizes = [int(np.prod(sc.mesh_grid_layout(v, 0.005, 4)[1])) for v, _ in meshes]
    offsets = [17, 17 + sizes[0] + 5]
    compact = torch.full((offsets[1] + sizes[1] + 9,), 1.0, dtype=torch.float32, device=dev)
    grids, origins, deltas, _ = ops.mesh_sdf_batch(meshes, 0.005, 4, samples, out=compact, out_offsets=offsets)
    layout = [(origins[m], deltas[m], samples[m], tuple(grids[m].shape), offsets[m]) for m in range(2)]
    angles, probe = G.approach_angles(8), G.default_probe()[:100]

    def poses(pool, lay):
        batch = ops.RayBatch(meshes, [128, 128], chunks=1, device=dev, layout=lay)
        out = ops.grasp_poses(batch, up("p1"), up("n1"), up("d"), up("t"), up("f2", np.int32), up("nrm"), angles, probe, pool,
                              cos_cone=float(np.cos(cone)), clearance=0.004)
        torch.cuda.synchronize()
        return tuple(_np(x) for x in out)

    want = poses(compact, layout)
    assert all(0 < want[1][128 * m: 128 * (m + 1)].sum() for m in range(2))  # both volumes let some hands through
    view = far.lane(0)
    FP.place(view, _np(compact), base)
    assert _all_same(poses(view, FP.relocate(layout, base)), want)
    ctrl = poses(view, FP.relocate(layout, FP.K))  # inside and outside have changed places: the probe meets the object
    assert not _same(ctrl[1], want[1])


# =====================================================================================================================
# 4. writers of volumes and states
# =====================================================================================================================
def _mesh_volumes():
    from omg_planner_amd import scenes as sc
    meshes = [MC.icosphere(1, 0.03), MC.box_mesh((0.02, 0.03, 0.01))]
    sizes = [int(np.prod(sc.mesh_grid_layout(v, 0.01, 2)[1])) for v, _ in meshes]
    return meshes, sizes


@BASES
def test_mesh_sdf_batch_writes_far_volumes_and_the_control(dev, far, base):
    """mesh_sdf_batch(out=, out_offsets=); and the writers' control: volumes sent to the alias window on purpose are found there by
    the guard check."""
    from omg_planner_amd import ops
    meshes, sizes = _mesh_volumes()
    offs, used = FP.spread(sizes)
    compact = FP.guard_compact(used, far.buf, dev)
    ops.mesh_sdf_batch(meshes, 0.01, 2, ["centre", "node"], out=compact, out_offsets=offs)
    view = far.lane(0)
    FP.guard(view, base, used)
    grids, _, _, _ = ops.mesh_sdf_batch(meshes, 0.01, 2, ["centre", "node"], out=view, out_offsets=FP.relocate(offs, base).tolist())
    assert _written(view, base, compact) == ALL_FINE
    assert grids[1].data_ptr() == view.data_ptr() + 4 * (base + offs[1]) and float(compact[offs[1]]) > 0 > float(compact[: sizes[0]].min())
    ops.mesh_sdf_batch(meshes, 0.01, 2, ["centre", "node"], out=view, out_offsets=FP.relocate(offs, FP.K).tolist())
    w = _written(view, base, compact)
    assert w == {"far": True, "bands": True, "alias": False}, w
    assert torch.equal(view[FP.K: FP.K + used].view(torch.int32)[: sizes[0]], compact.view(torch.int32)[: sizes[0]])


@pytest.fixture(scope="module")
def fused(dev):
    """The compact runs of the fusion and TSDF calls over FC.RAGGED (3 072, 765 and 910 nodes; three views), every array with the
    guard pattern between its volumes: what the far runs must reproduce, and what the far readers are given."""
    from omg_planner_amd import ops
    t, views = FC.scene_depth()
    depth = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    vols = [tuple(v) for v in FC.RAGGED]
    nodes = [int(np.prod(v[3])) for v in vols]
    offs, used = FP.spread(nodes)
    f32, u8 = torch.empty(0, dtype=torch.float32), torch.empty(0, dtype=torch.uint8)
    at = lambda delta: [v + (o + delta,) for v, o in zip(vols, offs)]
    r = dict(depth=depth, views=views, vols=vols, nodes=nodes, offs=np.array(offs, np.int64), used=used, at=at, mw=1.5,
             weights=np.array(TC.RAGGED_WEIGHTS), first=[(a, min(n, 1)) for a, n in FC.RAGGED_RANGES],
             rest=[(a + min(n, 1), n - min(n, 1)) for a, n in FC.RAGGED_RANGES])
    r["state"] = FP.guard_compact(used, u8, dev)
    ops.carve_views(vols, views, FC.RAGGED_RANGES, depth, FC.BAND, FC.NEAR, state=r["state"], state_begin=r["offs"])
    r["volume"] = FP.guard_compact(used, f32, dev)
    ops.distance_transform(r["state"], r["offs"], at(0), FC.RAGGED_RADIUS, True, out=r["volume"])
    r["tsdf"], r["weight"] = FP.guard_compact(used, f32, dev), FP.guard_compact(used, f32, dev)
    for ranges, merge in ((r["first"], False), (r["rest"], True)):
        ops.tsdf_integrate(vols, views, ranges, depth, TC.TRUNC, FC.NEAR, r["weights"], TC.RAGGED_WMAX, tsdf=r["tsdf"], weight=r["weight"],
                           state_begin=r["offs"], merge=merge)
    r["tsdf_state"] = FP.guard_compact(used, u8, dev)
    ops.tsdf_states(r["tsdf"], r["weight"], r["offs"], vols, r["mw"], state=r["tsdf_state"])
    r["tsdf_volume"] = FP.guard_compact(used, f32, dev)
    ops.distance_transform(r["tsdf_state"], r["offs"], at(0), TC.RAGGED_RADIUS, True, out=r["tsdf_volume"])
    r["blended"] = r["tsdf_volume"].clone()
    ops.tsdf_blend(r["tsdf"], r["weight"], r["offs"], at(0), TC.TRUNC, r["mw"], r["blended"])
    r["fuse_tsdf"] = FP.guard_compact(used, f32, dev)
    ops.fuse_tsdf(at(0), views, FC.RAGGED_RANGES, depth, TC.TRUNC, FC.NEAR, TC.RAGGED_RADIUS, True, r["mw"], r["weights"], TC.RAGGED_WMAX, out=r["fuse_tsdf"])
    torch.cuda.synchronize()
    s = _np(r["state"])
    assert all((s[o: o + n] == k).any() for o, n in zip(offs, nodes) for k in (0, 1, 2))  # every volume has free, surface and unknown nodes
    assert not _same(r["blended"], r["tsdf_volume"])
    return r


@BASES
def test_carve_views_writes_far_states(dev, far, fused, base):
    from omg_planner_amd import ops
    f = fused
    view = far.lane(1, torch.uint8)
    FP.guard(view, base, f["used"])
    state, begin = ops.carve_views(f["vols"], f["views"], FC.RAGGED_RANGES, f["depth"], FC.BAND, FC.NEAR, state=view, state_begin=FP.relocate(f["offs"], base))
    assert state is view and begin.tolist() == (f["offs"] + base).tolist()
    assert _written(view, base, f["state"]) == ALL_FINE
    # ... and carved in two calls, the second merging into what the first left far out
    FP.guard(view, base, f["used"])
    for ranges, merge in ((f["first"], False), (f["rest"], True)):
        ops.carve_views(f["vols"], f["views"], ranges, f["depth"], FC.BAND, FC.NEAR, state=view, state_begin=FP.relocate(f["offs"], base), merge=merge)
    assert _written(view, base, f["state"]) == ALL_FINE


@BASES
def test_distance_transform_reads_far_states_and_writes_far_volumes(dev, far, fused, base):
    from omg_planner_amd import ops
    f = fused
    state, pool = far.lane(1, torch.uint8), far.lane(0)
    FP.place(state, _np(f["state"]), base)
    FP.guard(pool, base, f["used"])
    out = ops.distance_transform(state, FP.relocate(f["offs"], base), f["at"](base), FC.RAGGED_RADIUS, True, out=pool)
    assert out is pool and _written(pool, base, f["volume"]) == ALL_FINE
    # the control of the state readers: states read from the alias window (free and surface swapped) give other volumes
    FP.guard(pool, base, f["used"])
    ops.distance_transform(state, FP.relocate(f["offs"], FP.K), f["at"](base), FC.RAGGED_RADIUS, True, out=pool)
    w = _written(pool, base, f["volume"])
    assert w == {"far": False, "bands": True, "alias": True}, w


@BASES
def test_tsdf_integrate_writes_and_merges_far_pairs(dev, far, fused, base):
    """tsdf and weight are two lanes of the one buffer, indexed by the same far state_begin; the second call merges."""
    from omg_planner_amd import ops
    f = fused
    d, w = far.lane(0), far.lane(1)
    FP.guard(d, base, f["used"]), FP.guard(w, base, f["used"])
    for ranges, merge in ((f["first"], False), (f["rest"], True)):
        ops.tsdf_integrate(f["vols"], f["views"], ranges, f["depth"], TC.TRUNC, FC.NEAR, f["weights"], TC.RAGGED_WMAX, tsdf=d, weight=w,
                           state_begin=FP.relocate(f["offs"], base), merge=merge)
    assert _written(d, base, f["tsdf"]) == ALL_FINE and _written(w, base, f["weight"]) == ALL_FINE
    assert float(_np(f["weight"])[: f["nodes"][0]].max()) == TC.RAGGED_WMAX  # the merging call reached the cap: it read the first call's pairs


@BASES
def test_tsdf_states_and_blend_on_far_pairs(dev, far, fused, base):
    from omg_planner_amd import ops
    f = fused
    begin = FP.relocate(f["offs"], base)
    pool, d, w, state = far.lane(0), far.lane(1), far.lane(2), far.lane(3, torch.uint8)
    FP.place(d, _np(f["tsdf"]), base), FP.place(w, _np(f["weight"]), base)
    FP.guard(state, base, f["used"])
    assert ops.tsdf_states(d, w, begin, f["vols"], f["mw"], state=state) is state
    assert _written(state, base, f["tsdf_state"]) == ALL_FINE
    # blend: the volumes the distance transform wrote lie far out and are changed in place
    FP.guard(pool, base, f["used"])
    pool[base: base + f["used"]].copy_(f["tsdf_volume"])
    assert ops.tsdf_blend(d, w, begin, f["at"](base), TC.TRUNC, f["mw"], pool) is pool
    assert _written(pool, base, f["blended"]) == ALL_FINE
    # the control of the pair readers: pairs read from the alias window (negated) give other states.  (The one state_begin
    # serves the pairs and the states, so these states land in the alias window too: the far region keeps the guard.)
    FP.guard(state, base, f["used"])
    ops.tsdf_states(d, w, FP.relocate(f["offs"], FP.K), f["vols"], f["mw"], state=state)
    wr = _written(state, base, f["tsdf_state"])
    assert wr["far"] is False and wr["alias"] is False and wr["bands"] is True, wr
    n0 = f["nodes"][0]
    assert not torch.equal(state[FP.K: FP.K + n0], f["tsdf_state"][:n0]) and bool((state[FP.K: FP.K + n0] != FP.GUARD8).all())


@BASES
def test_fuse_tsdf_writes_far_volumes(dev, far, fused, base):
    from omg_planner_amd import ops
    f = fused
    pool = far.lane(0)
    FP.guard(pool, base, f["used"])
    out = ops.fuse_tsdf(f["at"](base), f["views"], FC.RAGGED_RANGES, f["depth"], TC.TRUNC, FC.NEAR, TC.RAGGED_RADIUS, True, f["mw"], f["weights"],
                        TC.RAGGED_WMAX, out=pool)
    assert out is pool and _written(pool, base, f["fuse_tsdf"]) == ALL_FINE


@BASES
def test_plane_volumes_writes_far_volumes(dev, far, base):
    from omg_planner_amd import ops
    vols = [tuple(v) for v in PC.VOLUMES]
    offs, used = FP.spread([int(np.prod(v[3])) for v in vols])
    compact = FP.guard_compact(used, far.buf, dev)
    ops.plane_volumes([v + (o,) for v, o in zip(vols, offs)], PC.VOLUME_PLANES, out=compact)
    pool = far.lane(0)
    FP.guard(pool, base, used)
    assert ops.plane_volumes([v + (o + base,) for v, o in zip(vols, offs)], PC.VOLUME_PLANES, out=pool) is pool
    assert _written(pool, base, compact) == ALL_FINE
    assert (_np(compact)[offs[0]: offs[0] + 3072] > 0).any() and (_np(compact)[offs[0]: offs[0] + 3072] < 0).any()


SEGMENT = ("serpentine", "all", "bar", "random31", "values", "one_bg")


@pytest.fixture(scope="module")
def segments():
    """Six of segment_cases' state grids as a batch (volumes, state with SURFACE bytes between the volumes as SC.batch() has them,
    state_begin, used)."""
    grids = [SC.cases()[n][0] for n in SEGMENT]
    volumes = [SC.volume_of(g, m) for m, g in enumerate(grids)]
    offs, used = FP.spread([g.size for g in grids])
    state = np.full(used, SC.GUARD, np.uint8)
    for o, g in zip(offs, grids):
        state[o: o + g.size] = g.ravel()
    return volumes, state, np.array(offs, np.int64), used


def _labels_fine(comps, want, base, used):
    """The labels of the far run: the compact run's in the far region, -1 (omgx_label_components' fill) in the bands around it and
    all over the alias window, where a label written through a wrapped offset would show."""
    lab = comps.labels
    return (torch.equal(lab[base: base + used], want.labels) and bool((lab[base - FP.BAND: base] == -1).all())
            and bool((lab[base + used:] == -1).all()) and bool((lab[: FP.K + used + FP.BAND] == -1).all()))


@BASES
@pytest.mark.parametrize("connectivity", [6, 26])
def test_label_components_and_records_on_far_states(dev, far, segments, base, connectivity):
    """omgx_label_components and omgx_component_records: the labels lie in the wrapper's own array at the far state_begin."""
    from omg_planner_amd import ops
    volumes, h_state, offs, used = segments
    want = ops.label_components(torch.from_numpy(h_state).to(dev), offs, volumes, 1, connectivity)
    assert want.counts.tolist()[:3] == [1, 1, 1] and want.counts[3] > 1 and want.counts[5] == 0 and bool((want.labels[: offs[1]] >= 0).any())
    view = far.lane(1, torch.uint8)
    FP.place(view, h_state, base)
    state = view[: base + used + FP.BAND]
    got = ops.label_components(state, FP.relocate(offs, base), volumes, 1, connectivity)
    torch.cuda.synchronize()
    assert _same(got.counts, want.counts) and _same(got.comp_begin, want.comp_begin) and _same(got.records, want.records) and _same(got.d_records, want.d_records)
    assert _labels_fine(got, want, base, used)
    del got
    # the control: the states of the alias window (free and surface swapped) have other components
    ctrl = ops.label_components(state, FP.relocate(offs, FP.K), volumes, 1, connectivity)
    assert not _same(ctrl.counts, want.counts)


@BASES
def test_component_states_with_far_states_labels_and_outputs(dev, far, segments, base):
    from omg_planner_amd import ops
    volumes, h_state, offs, used = segments
    c_state = torch.from_numpy(h_state).to(dev)
    comps = ops.label_components(c_state, offs, volumes, 1, 6)
    picks, outs, _ = SC.picks_for(volumes, comps.comp_begin, comps.records, seed=3, per_volume=1)
    out_offs, out_used = FP.spread([int(np.prod(o[3])) for o in outs])
    want = FP.guard_compact(out_used, c_state, dev)
    ops.component_states(c_state, comps, picks, outs, out_begin=np.array(out_offs, np.int64), out=want)
    assert len(picks) >= 10 and {int(p[5]) for p in picks} == {0, 1}
    view, out = far.lane(1, torch.uint8), far.lane(2, torch.uint8)
    FP.place(view, h_state, base)
    state = view[: base + used + FP.BAND]
    far_comps = ops.label_components(state, FP.relocate(offs, base), volumes, 1, 6)
    FP.guard(out, base, out_used)
    got, got_begin = ops.component_states(state, far_comps, picks, outs, out_begin=FP.relocate(out_offs, base), out=out)
    assert got is out and got_begin.tolist() == [o + base for o in out_offs]
    assert _written(out, base, want) == ALL_FINE
    h = _np(want)
    assert all((h[o: o + int(np.prod(v[3]))] != FP.GUARD8).all() for o, v in zip(out_offs, outs)) and {0, 1} <= set(np.unique(h).tolist())
