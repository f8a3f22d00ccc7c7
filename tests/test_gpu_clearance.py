"""Plan clearance on the MI355X (csrc/omg_clearance.hip): omgx_sphere_clearance / omgx_self_clearance
against clearance.py bit for bit through the C ABI, one launch each, on the edge cases and the seeded batches, between guard
values, with the cull on and off; ops.dense_configs as bits; DeviceScenes.plan_clearance on the tunnelling scene against the
specification's report on the device's own link poses, also on a side stream; pipeline.check_plans on two planned scenes; a short
seeded fuzz run; a pool beyond 2^32 elements.  Every launch is followed by a checked synchronise."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import clearance_cases as CC
from tests import far_pool as FP

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD_V, GUARD_N = -77.25, -5  # what the outputs hold before a launch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(dev) if a.dtype.names else torch.from_numpy(a).to(dev)


def _h(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def abi_sphere(dev, c, cull, pad="own", d_pool=None, objects=None):
    """omgx_sphere_clearance on outputs that hold guard values, with one more guarded row behind them -> (the six outputs, world) as
    numpy; asserts that the guards stand.  d_pool, objects: another pool on the device and the records that address it."""
    from omg_planner_amd import _lib
    vp = C.c_void_p
    pad = c["pad"] if isinstance(pad, str) else pad
    objects = np.ascontiguousarray(c["objects"] if objects is None else objects)
    begin, cfg = np.ascontiguousarray(c["begin"], np.int32), np.ascontiguousarray(c["cfg"], np.int32)
    poses, local, link = np.ascontiguousarray(c["poses"], np.float64), np.ascontiguousarray(c["local"], np.float64).reshape(-1, 4), np.ascontiguousarray(c["link"], np.int32)
    vis = None if c.get("visible") is None else np.ascontiguousarray(c["visible"], np.uint8)
    d_pool = _up(np.ascontiguousarray(c["pool"], np.float32), dev) if d_pool is None else d_pool
    B, N, n = len(cfg), len(link), len(objects)
    d = dict(objects=_up(objects, dev) if n else None, begin=_up(begin, dev), cfg=_up(cfg, dev) if B else None, poses=_up(poses, dev) if B else None,
             local=_up(local, dev) if N else None, link=_up(link, dev) if N else None, vis=None if vis is None or not n else _up(vis, dev),
             pad=None if pad is None else _up(np.ascontiguousarray(pad, np.float64), dev))
    f64 = lambda: torch.full((B + 1,), GUARD_V, dtype=torch.float64, device=dev)
    i32 = lambda: torch.full((B + 1,), GUARD_N, dtype=torch.int32, device=dev)
    out = [f64(), i32(), i32()] + ([f64(), i32(), i32()] if pad is not None else [None, None, None])
    world = torch.full((B + 1, max(N, 1), 4), GUARD_V, dtype=torch.float64, device=dev)
    ptr = lambda x: None if x is None else vp(x.data_ptr())
    rc = _lib.lib().omgx_sphere_clearance(ptr(d["objects"]), _h(objects) if n else None, n, ptr(d["begin"]), _h(begin), len(begin) - 1, ptr(d_pool),
                                          d_pool.numel(), ptr(d["vis"]), _h(vis) if d["vis"] is not None else None, ptr(d["cfg"]), _h(cfg) if B else None, B,
                                          ptr(d["poses"]), ptr(d["local"]), _h(local) if N else None, ptr(d["link"]), _h(link) if N else None, N,
                                          ptr(d["pad"]), float(c["beyond"]), int(cull), *[ptr(x) for x in out], ptr(world),
                                          vp(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OMGX_OK, (rc, _lib.lib().omgx_last_error())
    torch.cuda.synchronize()
    assert all(x is None or x[B].item() == (GUARD_V if x.dtype == torch.float64 else GUARD_N) for x in out)
    assert (world.reshape(-1)[B * N * 4:] == GUARD_V).all()
    return tuple(None if x is None else x[:B].cpu().numpy() for x in out), world.reshape(-1)[: B * N * 4].reshape(B, N, 4).cpu().numpy()


def abi_self(dev, world, link, pairs, pad):
    from omg_planner_amd import _lib
    vp = C.c_void_p
    world, link, pairs = np.ascontiguousarray(world, np.float64), np.ascontiguousarray(link, np.int32), np.ascontiguousarray(pairs, np.uint8)
    B, N = world.shape[:2]
    d_world, d_link, d_pairs = (_up(world, dev) if B * N else None), (_up(link, dev) if N else None), _up(pairs, dev)
    d_pad = None if pad is None else _up(np.ascontiguousarray(pad, np.float64), dev)
    out = [torch.full((B + 1,), GUARD_V, dtype=torch.float64, device=dev)] + [torch.full((B + 1,), GUARD_N, dtype=torch.int32, device=dev) for _ in range(2)]
    ptr = lambda x: None if x is None else vp(x.data_ptr())
    rc = _lib.lib().omgx_self_clearance(ptr(d_world), B, ptr(d_link), _h(link) if N else None, N, ptr(d_pairs), ptr(d_pad), *[ptr(x) for x in out],
                                        vp(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OMGX_OK, (rc, _lib.lib().omgx_last_error())
    torch.cuda.synchronize()
    assert out[0][B].item() == GUARD_V and out[1][B].item() == GUARD_N and out[2][B].item() == GUARD_N
    return tuple(x[:B].cpu().numpy() for x in out)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the device against the specification
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", (1, 0))
def test_edge_cases_against_the_written_answers(dev, cull):
    objects, begin, pool, launches = CC.edge_launch()
    d_pool = _up(pool, dev)
    for L in launches:
        got, world = abi_sphere(dev, dict(L, objects=objects, begin=begin, pool=pool), cull, d_pool=d_pool)
        assert tuple(None if x is None else x[0].item() for x in got) == L["want"] and CC.same(world[0], L["local"]), L["what"]
    for what, sph, links, pairs, pad, want in CC.SELF_CASES:
        got = abi_self(dev, np.array([sph], np.float64), links, pairs, None if pad is None else np.array([pad]))
        assert tuple(x[0].item() for x in got) == want, what


@pytest.mark.parametrize("cull", (1, 0))
def test_seeded_batches_in_one_launch_each_against_the_specification(dev, cull):
    """N in {0, 1, 63, 64, 65, 257} x B in {1, 4, 5, 17} x S in {1, 3}: volumes of (2,2,2), (5,9,7), (33,17,9) at non-zero offsets of
    a ragged pool with NaN between them, a scene without objects, a disabled and an invisible record; the six outputs and
    world_out equal clearance.py's bits, with pads and without."""
    pools = {S: _up(CC.table(S)[2], dev) for S in CC.BATCH_S}
    for key in CC.BATCHES:
        c = CC.batch(*key)
        got, world = abi_sphere(dev, c, cull, d_pool=pools[key[2]])
        assert CC.same_results(got, c["want"]) and CC.same(world, c["world"]), key
        if key[1] == 5:
            got, _ = abi_sphere(dev, c, cull, pad=None, d_pool=pools[key[2]])
            assert CC.same_results(got, c["want"][:3] + (None, None, None)), key


@pytest.mark.parametrize("N", CC.SELF_N)
def test_self_clearance_against_the_specification(dev, N):
    c = CC.self_batch(N)
    assert CC.same_results(abi_self(dev, c["world"], c["link"], c["pairs"], c["pad"]), c["want"])
    assert CC.same_results(abi_self(dev, c["world"], c["link"], c["pairs"], None), c["want_bare"])


def test_wrappers_on_a_seeded_batch(dev):
    """ops.sphere_clearance and ops.self_clearance on a DeviceScenes.over_pool table: the same bits, cull on and off, the world
    spheres on request; a specification error is an OmgHipError before any launch."""
    from omg_planner_amd import _lib, clearance as cl, ops
    c = CC.batch(257, 17, 3, 1)
    table = ops.DeviceScenes.over_pool(c["objects"], c["begin"], _up(c["pool"], dev))
    spheres = ops.RobotSpheres(c["local"], c["link"], device=dev)
    poses, pad = _up(c["poses"], dev), _up(c["pad"], dev)
    for cull in (True, False):
        out = ops.sphere_clearance(table, spheres, poses, c["cfg"], visible=c["visible"], pad=pad, beyond=c["beyond"], cull=cull, want_world=True)
        torch.cuda.synchronize()
        assert CC.same_results(tuple(x.cpu().numpy() for x in out[:6]), c["want"]) and CC.same(out[6].cpu().numpy(), c["world"])
    bare = ops.sphere_clearance(table, spheres, poses, c["cfg"], visible=c["visible"], beyond=c["beyond"])
    assert bare[3] is None and bare[6] is None and CC.same(bare[0].cpu().numpy(), c["want"][0])
    pairs = ops.default_self_pairs()
    small = ops.RobotSpheres(c["local"][:200], c["link"][:200], device=dev)
    got = ops.self_clearance(out[6][:, :200].contiguous(), small, pairs, pad=pad)
    torch.cuda.synchronize()
    assert CC.same_results(tuple(x.cpu().numpy() for x in got), cl.self_clearance(c["world"][:, :200], c["link"][:200], pairs, c["pad"]))
    E = _lib.OmgHipError
    for bad in (dict(beyond=-1.0), dict(beyond=float("nan")), dict(scene_of_config=np.full(17, 3)), dict(visible=[1, 1]), dict(pad=pad[:, :9].contiguous()),
                dict(link_poses=poses[:, :9].contiguous()), dict(link_poses=poses.cpu())):
        with pytest.raises(E):
            ops.sphere_clearance(**{**dict(table=table, spheres=spheres, link_poses=poses, scene_of_config=c["cfg"], visible=None, pad=pad, beyond=0.1), **bad})
    broken = c["objects"].copy()
    broken["dim"][0] = (1, 2, 2)
    with pytest.raises(E, match="two samples"):
        ops.sphere_clearance(ops.DeviceScenes.over_pool(broken, c["begin"], table.pool), spheres, poses, c["cfg"])
    with pytest.raises(E, match="at most"):
        ops.self_clearance(torch.zeros((1, 1025, 4), dtype=torch.float64, device=dev), ops.RobotSpheres(np.zeros((1025, 4)), np.zeros(1025), device=dev), pairs)


def test_dense_configs_equals_numpy_as_bits(dev):
    from omg_planner_amd import clearance as cl, ops
    rng = np.random.default_rng(3)
    traj = rng.uniform(-2.0, 2.0, (3, 7, 9))
    traj[0, 1, 2], traj[1, 0, 0] = -0.0, -0.0
    for K in (1, 2, 7, 8):
        got = ops.dense_configs(_up(traj, dev), K)
        assert CC.same(got.cpu().numpy(), cl.dense_configs(traj, K)), K
    assert CC.same(ops.dense_configs(_up(traj[:, :1], dev), 4).cpu().numpy(), traj[:, :1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the path
# ---------------------------------------------------------------------------------------------------------------------
def _plate_on_device(dev):
    from omg_planner_amd import ops
    c = CC.plate()
    table = ops.DeviceScenes.over_pool(c["objects"], c["begin"], _up(c["pool"], dev))
    spheres = ops.RobotSpheres(c["local"], c["link"], device=dev)
    blob = ops.robot_blob(c["model"], dev)
    return c, table, spheres, blob


def _report_equals(got, want, out_want, S, T):
    """An ops.PlanClearance against the specification's report and six outputs."""
    names = ("clear", "clear_sphere", "clear_object", "margin", "margin_sphere", "margin_object")
    for name, w in zip(names, out_want):
        assert CC.same(getattr(got, name).cpu().numpy(), w.reshape(S, T)), name
    for name, w in want.items():
        assert CC.same(getattr(got, name).cpu().numpy(), w), name


@pytest.mark.parametrize("side_stream", (False, True))
def test_plan_clearance_on_the_tunnelling_scene_equals_the_specifications_report(dev, side_stream):
    """The plate between two waypoints (tests/clearance_cases.py): at K = 1 and K = 16 every per-sample, per-segment and per-plan
    tensor of DeviceScenes.plan_clearance equals clearance.py on the device's own link poses, and shows the four outcomes.  On a
    side stream the two calls are enqueued back to back and synchronised once at the end."""
    from omg_planner_amd import ops
    c, table, spheres, blob = _plate_on_device(dev)
    traj = _up(c["traj"], dev)
    P = c["model"].points_per_link
    fk = lambda q: ops.forward_kinematics(blob, P, _up(q, dev), want_joint_info=False)[0].cpu().numpy()
    stream = torch.cuda.Stream(dev) if side_stream else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        got = [table.plan_clearance(spheres, blob, P, traj, K, beyond=CC.PLATE_BEYOND, rho=c["rho"], pairs=ops.default_self_pairs()) for K in CC.PLATE_K]
    stream.synchronize()
    for K, g in zip(CC.PLATE_K, got):
        want, out_want = CC.plate_report(K, fk)
        _report_equals(g, want, out_want, 2, K + 1)
        assert g.K == K and tuple(g.q.shape) == (2, K + 1, 9) and g.self_clear.shape == (2, K + 1) and (g.self_i == -1).all()  # one sphere: no pair
    few, many = got
    assert few.collides.tolist() == [False, False] and few.plan_certified.tolist() == [False, False]
    assert many.collides.tolist() == [True, False] and 0 < int(many.first_hit[0]) < CC.PLATE_K[1] and many.plan_certified.tolist() == [False, True]
    E = __import__("omg_planner_amd")._lib.OmgHipError
    for bad in (dict(substeps=0), dict(slack=-0.1), dict(beyond=float("inf")), dict(rho=np.zeros((9, 10))), dict(scene_of_plan=[0, 2]), dict(traj=traj.cpu())):
        with pytest.raises(E):
            table.plan_clearance(**{**dict(spheres=spheres, robot_blob=blob, P=P, traj=traj, substeps=2, rho=c["rho"]), **bad})
    with pytest.raises(E, match="reach_table"):
        table.plan_clearance(ops.RobotSpheres(c["local"], c["link"], device=dev), blob, P, traj, 2)


@pytest.fixture(scope="module")
def planned(dev):
    """Two tabletop scenes with a standing box as the target, planned by plan_meshes (tests/test_gpu_grasp_sampling.py's fixture)."""
    from omg_planner_amd import ops, pipeline, robot as rb
    from omg_planner_amd.config import Config
    from tests import mesh_cases as MC
    from tests import test_gpu_grasp_sampling as GS
    cfg = Config(use_standoff=True, timeout=-1, silent=True)
    model = rb.PandaModel()
    scenes = GS._box_scenes()
    start = np.tile(rb.HOME_CONFIG, (2, 1))
    plans, _ = pipeline.plan_meshes(model, scenes, [MC.box_mesh(MC.BOX_HALF)] * 2, start, cfg, n_rays=256, n_angles=8, ol_alg="MD",
                                    rng=np.random.RandomState(0), grasp_rng=[np.random.RandomState(7), np.random.RandomState(8)], max_grasps=64,
                                    device=dev, cone=GS.CONE)
    table = ops.DeviceScenes.from_scenes(scenes, cfg.layer_kwargs(), device=dev)
    spheres = ops.RobotSpheres.from_points(model.collision_points, 0.02, dev)
    torch.cuda.synchronize()
    assert plans.planned.all()
    return model, scenes, plans, table, spheres


def test_check_plans_on_two_planned_scenes(dev, planned):
    """Shapes and masks; the report equals the specification on the device's link poses; with planned = (True, False) the second
    row says nothing and the first is unchanged; with skip_targets=False the last sample's nearest object is the target."""
    from omg_planner_amd import clearance as cl, ops, pipeline
    model, scenes, plans, table, spheres = planned
    K, n = 4, plans.traj.shape[1]
    T = (n - 1) * K + 1
    rep = pipeline.check_plans(model, table, plans, spheres, K, targets=scenes, beyond=0.2)
    torch.cuda.synchronize()
    assert tuple(rep.clear.shape) == (2, T) and tuple(rep.half.shape) == (2, n - 1, 10) and tuple(rep.certified.shape) == (2, n - 1)
    assert rep.certified.dtype == torch.bool and rep.collides.dtype == torch.bool and rep.first_hit.dtype == torch.int64 and rep.self_clear.shape == (2, T)
    assert tuple(rep.min_clearance.shape) == (2,) and torch.isfinite(rep.min_clearance).all()
    # the specification on the device's poses
    traj = plans.traj.cpu().numpy()
    q = cl.dense_configs(traj, K)
    poses = ops.forward_kinematics(plans.engine.robot, model.points_per_link, _up(q.reshape(-1, 9), dev), want_joint_info=False)[0].cpu().numpy()
    world = cl.world_spheres(poses, spheres.h_local, spheres.h_link)
    pad = cl.sample_pads(cl.segment_halves(traj, K, spheres.rho), K, 0.0).reshape(-1, 10)
    visible = table.host_objects["disabled"] == 0
    for s, sc_ in enumerate(scenes):
        visible[table._index(s, sc_.target_idx)] = False
    out = cl.sphere_clearance(table.host_objects, table.host_scene_begin, table.pool.cpu().numpy(), visible, np.repeat([0, 1], T), world, spheres.h_link, pad, 0.2)
    want = cl.plan_report(traj, K, spheres.rho, float(spheres.h_local[:, 3].max()), 0.0, 0.2, out[0].reshape(2, T), out[3].reshape(2, T))
    _report_equals(rep, want, out, 2, T)
    own = cl.self_clearance(world, spheres.h_link, ops.default_self_pairs(True), pad)
    assert CC.same_results(tuple(x.cpu().numpy().reshape(-1) for x in (rep.self_clear, rep.self_i, rep.self_j)), own)
    print("min clearance", rep.min_clearance.tolist(), "collides", rep.collides.tolist(), "certified segments", rep.certified.sum(dim=1).tolist(), "of", n - 1)
    # an unplanned row
    half = pipeline.check_plans(model, table, dataclasses.replace(plans, planned=np.array([True, False])), spheres, K, targets=scenes, beyond=0.2)
    torch.cuda.synchronize()
    for name in ("clear", "margin", "clear_object", "segment_margin", "certified", "first_hit", "q", "self_clear", "half"):
        assert torch.equal(getattr(half, name)[0], getattr(rep, name)[0]), name
    assert torch.isposinf(half.clear[1]).all() and (half.clear_sphere[1] == -1).all() and not half.certified[1].any() and not half.plan_certified[1]
    assert not half.collides[1] and half.first_hit[1] == -1 and torch.isposinf(half.min_clearance[1]) and (half.self_i[1] == -1).all()
    # the target in: the plan ends at it
    full = pipeline.check_plans(model, table, plans, spheres, K, skip_targets=False, pairs=False, beyond=0.2)
    torch.cuda.synchronize()
    assert full.self_clear is None and full.clear_object[:, -1].tolist() == [sc_.target_idx for sc_ in scenes]
    assert (full.clear <= rep.clear).all()
    with pytest.raises(ValueError, match="targets"):
        pipeline.check_plans(model, table, plans, spheres, K)


# ---------------------------------------------------------------------------------------------------------------------
# 3. fuzz, and a far pool
# ---------------------------------------------------------------------------------------------------------------------
def test_a_short_seeded_fuzz_run(dev):
    rng = np.random.default_rng(CC.FUZZ_SEED)
    for trial in range(CC.FUZZ_TRIALS):
        c = CC.draw(rng)
        world, want, want_self = CC.specification(c)
        got, got_world = abi_sphere(dev, c, c["cull"])
        assert CC.same_results(got, want) and CC.same(got_world, world), (trial, c["N"], c["B"], c["S"])
        assert CC.same_results(abi_self(dev, world, c["link"], c["pairs"], c["pad"]), want_self), (trial, c["N"])


def test_sphere_clearance_on_a_far_pool(dev):
    """The records moved to an element offset beyond 2^32 of one large buffer (tests/far_pool.py: B2, the module's own skip rule):
    the same bits as on the compact pool; with the records moved by K alone (the alias window, which holds the volumes negated)
    other bits: the test can tell."""
    free, total = torch.cuda.mem_get_info(dev)
    need = 4 * FP.ELEMS + FP.HEADROOM
    if free < need:
        pytest.skip(f"the far-pool buffer needs {need} bytes of free device memory (4 * (2^32 + {FP.RESERVE}) and 2 GiB), {free} of {total} are free")
    c = CC.batch(65, 5, 1, 0)
    buf = torch.empty(FP.ELEMS, dtype=torch.float32, device=dev)
    view = FP.lane(buf, 0)
    FP.place(view, c["pool"], FP.B2)
    got, _ = abi_sphere(dev, c, 1, d_pool=view, objects=FP.relocate(c["objects"], FP.B2))
    assert CC.same_results(got, c["want"])
    ctrl, _ = abi_sphere(dev, c, 1, d_pool=view, objects=FP.relocate(c["objects"], FP.K))
    assert not CC.same(ctrl[0], c["want"][0])
    del view, buf
    torch.cuda.empty_cache()
