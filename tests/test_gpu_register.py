"""Registration on the MI355X (csrc/omg_register.hip): omgx_register_clouds against
registration.register_clouds bit for bit around a lane's first and second point, the wave boundaries and the zero-padded tail,
on every special case of the CPU file; 70 instances in one launch against single launches between sentinels; out= in place;
set_object_poses against set_object_pose; refine_scene_poses on two scenes built on the device; a short seeded fuzz run."""
from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import register_cases as RC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _same(got, want):
    """poses and stats as int64 bits, device against specification."""
    torch.cuda.synchronize()
    return all(torch.equal(g.cpu().view(torch.int64), torch.from_numpy(np.array(w)).view(torch.int64)) for g, w in zip(got, want))


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("K", [0, 1, 2, 12])
def test_range_lengths_equal_the_specification_bit_for_bit(dev, K, stride):
    """0, 1, 5, 6, 63, 64, 65, 255, 256, 257, 513 and 1025 used points: no point, fewer than six, a lane's first and second
    point, the wave boundaries and the zero-padded tail, one instance each in one launch."""
    from omg_planner_amd import registration as reg
    c = RC.lengths_call(K, stride)
    assert [len(range(b, e, stride)) for b, e in c["ranges"]] == [0, 1, 5, 6, 63, 64, 65, 255, 256, 257, 513, 1025]
    want = reg.register_clouds(*RC.args(c))
    assert (want[1][3:, reg.COUNT0] >= 6).all() and (K == 0 or (want[1][3:, reg.TRIALS] >= 1).all())
    assert _same(RC.device_register(c, dev), want), (K, stride)


@pytest.mark.parametrize("name", RC.ALL + ["toy"])
def test_cases_of_the_cpu_file_equal_the_specification_bit_for_bit(dev, name):
    c, want = (RC.toy()["call"], RC.toy_spec()) if name == "toy" else (RC.call(name), RC.spec(name))
    assert max(int(np.prod(d)) for d in c["objects"]["dim"]) <= 24 ** 3   # voxels; the toy grids (23 x 17 x 26 at most) have an axis of 26
    assert _same(RC.device_register(c, dev), want), name


def _seventy():
    """70 instances on three volumes of a ragged pool: unequal ranges, several shared, three empty."""
    rng = np.random.default_rng(70)
    kinds = ["box", "ellipsoid", "sphere"]
    grids = [RC.volume("box", (16,) * 3, 0.02), RC.volume("ellipsoid", (8, 9, 10), 0.03), RC.volume("sphere", (12, 10, 11), 0.02)]
    truth = [RC.random_pose(rng) for _ in range(12)]
    kind_of = [int(rng.integers(3)) for _ in truth]
    clouds = [RC.to_world(P, RC.surface(kinds[k], int(rng.integers(20, 420)), rng)) for P, k in zip(truth, kind_of)]
    begin = np.cumsum([0] + [len(x) for x in clouds])
    index, starts, ranges = [], [], []
    for m in range(70):
        t = m % 12 if m < 24 else int(rng.integers(12))      # every cloud at least twice: shared ranges
        index.append(kind_of[t]), starts.append(RC.perturbed(truth[t], rng, 0.015, np.deg2rad(8.0)))
        ranges.append((begin[t], begin[t + 1]) if m < 40 else (begin[t] + int(rng.integers(0, 10)), begin[t + 1] - int(rng.integers(0, 10))))
    for m in (5, 33, 69):
        ranges[m] = (ranges[m][0], ranges[m][0])
    return RC._call(grids, index, starts, clouds, ranges=ranges, gaps=(4, 1, 6), max_passes=6)


def test_seventy_instances_in_one_launch_equal_single_launches(dev):
    """One launch of 70 workgroups against the same instances launched alone, and against the specification; poses and stats are
    written between sentinels that must survive."""
    from omg_planner_amd import registration as reg
    c = _seventy()
    M = 70
    assert len({tuple(r) for r in c["ranges"].tolist()}) < M - 10 and (c["ranges"][:, 0] == c["ranges"][:, 1]).sum() == 3
    ds, _ = RC.device_scenes(c, dev)
    guard = 5
    P = torch.full((M + 2 * guard, 12), -7.25, dtype=torch.float64, device=dev)
    S = torch.full((M + 2 * guard, 8), -7.25, dtype=torch.float64, device=dev)
    got = RC.device_register(c, dev, out=(P[guard: guard + M], S[guard: guard + M]), ds=ds)
    assert got[0].data_ptr() == P[guard].data_ptr()
    assert _same(got, reg.register_clouds(*RC.args(c)))
    for t in (P, S):
        assert (t[:guard] == -7.25).all() and (t[guard + M:] == -7.25).all()
    for m in range(M):
        one = dict(c, obj_index=c["obj_index"][m: m + 1], poses0=c["poses0"][m: m + 1], ranges=c["ranges"][m: m + 1])
        alone = RC.device_register(one, dev, ds=ds)
        assert torch.equal(alone[0][0].view(torch.int64), got[0][m].view(torch.int64)) and torch.equal(alone[1][0].view(torch.int64), got[1][m].view(torch.int64)), m


def test_out_is_written_in_place_and_checked(dev):
    from omg_planner_amd import _lib
    c = RC.call("shared_range")
    out = (torch.zeros((3, 12), dtype=torch.float64, device=dev), torch.zeros((3, 8), dtype=torch.float64, device=dev))
    got = RC.device_register(c, dev, out=out)
    assert got[0] is out[0] and got[1] is out[1] and _same(out, RC.spec("shared_range"))
    for bad in ((out[0][:2], out[1]), (out[0], out[1].float()), (out[0].cpu(), out[1]), (out[0], torch.zeros((3, 9), dtype=torch.float64, device=dev))):
        with pytest.raises(_lib.OmgHipError):
            RC.device_register(c, dev, out=bad)
    none = dict(c, obj_index=c["obj_index"][:0], poses0=c["poses0"][:0], ranges=c["ranges"][:0])
    empty = RC.device_register(none, dev)
    assert tuple(empty[0].shape) == (0, 12) and tuple(empty[1].shape) == (0, 8)


def test_wrapper_refuses_what_only_a_device_shows(dev):
    """The wrapper's checks that need device tensors to be reached at all, through ops.register_clouds itself: tensors of the wrong
    type or on the host, every scalar and range error with everything else valid and on the device, and a record whose grid the C
    ABI refuses (a dim below 2, a grid that leaves the pool) on the host mirror, before anything is launched."""
    from omg_planner_amd import _lib, ops
    E = _lib.OmgHipError
    c = RC.call("shared_range")
    ds, pairs = RC.device_scenes(c, dev)
    points, poses0 = torch.from_numpy(c["points"]).to(dev), torch.from_numpy(c["poses0"]).to(dev)
    run = lambda pairs=pairs, poses0=poses0, points=points, ranges=c["ranges"], **kw: ops.register_clouds(ds, pairs, poses0, points, ranges, **kw)
    assert _same(run(), RC.spec("shared_range"))
    for kw in (dict(stride=0), dict(max_passes=-1), dict(max_passes=65), dict(trunc=0.0), dict(trunc=float("nan")), dict(lambda0=-1.0),
               dict(lambda0=float("inf")), dict(ranges=[(0, 300), (0, 301), (100, 300)]), dict(ranges=[(0, 300), (7, 6), (100, 300)]),
               dict(ranges=[(0, 300), (-1, 6), (100, 300)]), dict(ranges=c["ranges"][:2]), dict(points=points.float()), dict(points=points.cpu()),
               dict(points=points.T.contiguous().T), dict(poses0=poses0.cpu()), dict(poses0=poses0.float()), dict(poses0=poses0[:2]),
               dict(poses0=torch.zeros((3, 16), dtype=torch.float64, device=dev)[:, :12])):
        with pytest.raises(E):
            run(**kw)
    with pytest.raises(IndexError):
        run(pairs=[(0, 0), (0, 1), (0, 0)])
    good = ds.host_objects.copy()
    for field, value in (("dim", (16, 1, 16)), ("grid_offset", len(c["pool"]) - 16 ** 3 + 1), ("grid_offset", -1)):
        ds.host_objects[field][0] = value
        with pytest.raises(E, match="invalid argument"):
            run()
        ds.host_objects[:] = good
    assert _same(run(), RC.spec("shared_range"))


def test_set_object_poses_equals_set_object_pose(dev):
    """The record bytes on the device and the host mirror after one scatter, against one call per object."""
    from omg_planner_amd import ops, scenes as S
    scenes = [S.make_tabletop_scene(s, num_objects=3, grid=8, table_grid=(8, 8, 4)) for s in range(4)]
    batch = S.pack_table(scenes, tight=False)
    one, many = ops.DeviceScenes(batch, device=dev), ops.DeviceScenes(batch, device=dev)
    rng = np.random.default_rng(4)
    pairs = [(3, 1), (0, 0), (1, 3), (2, 2), (3, 0)]
    poses = np.stack([RC.random_pose(rng) for _ in pairs])
    for (s, o), Pm in zip(pairs, poses):
        one.set_object_pose(s, o, Pm)
    before = many.objects.clone()
    many.set_object_poses(pairs, torch.from_numpy(poses).to(dev))
    torch.cuda.synchronize()
    assert torch.equal(many.objects, one.objects) and not torch.equal(many.objects, before)
    assert many.host_objects.tobytes() == one.host_objects.tobytes() and many.sync_host().tobytes() == one.sync_host().tobytes()


def test_refine_scene_poses_on_two_scenes_built_on_the_device(dev):
    """Volumes by ops.mesh_sdf, images by ops.render_depth, clouds by ops.pixel_clouds, poses by refine_scene_poses: the device
    chain has the bits of the specification chain (scenes.mesh_sdf, camera.render_depth, camera.pixel_clouds,
    registration.register_clouds), the accepted mask is the specified one, and after the write-back the scenes are those of a
    DeviceScenes built with the refined poses: ops.fk_sdf of a fixed configuration is equal."""
    from omg_planner_amd import ops, registration as reg, robot as rb, scenes as S
    T = RC.toy()
    c = T["call"]
    want_poses, want_stats = RC.toy_spec()
    cfw, truth = T["cam_from_world"], T["truth"]
    _, starts = RC.toy_layout()[1:]
    grids = []
    for (v, f), spec in zip(T["meshes"], T["grids"]):
        g, origin, delta = ops.mesh_sdf(v, f, RC.TOY_DELTA, padding=4, device=dev)
        assert np.array_equal(g.cpu().numpy(), spec.data) and np.array_equal(origin, spec.origin)
        grids.append(S.SdfGrid(g.cpu().numpy(), origin, delta))

    def build(poses):
        return ops.DeviceScenes.from_scenes([S.Scene([S.SceneObject("box", poses[s][0], grids[0]), S.SceneObject("ellipsoid", poses[s][1], grids[1])], 0)
                                             for s in range(2)], device=dev)
    dscenes = build(starts)
    cam = ops.CameraBatch(T["meshes"], T["instances"], T["inst_begin"], T["cameras"], device=dev)
    t, img, _ = ops.render_depth(cam, RC.TOY_H, RC.TOY_W, want_face=False)
    clouds = [ops.pixel_clouds(cam, t, img, cls) for cls in (0, 1)]
    points = torch.cat([p for p, _ in clouds])
    assert torch.equal(points.cpu().view(torch.int64), torch.from_numpy(c["points"]).view(torch.int64))
    ranges, n = [], 0
    for _, begin in clouds:
        ranges += [(n + int(begin[s]), n + int(begin[s + 1])) for s in range(2)]
        n += int(begin[-1])
    ranges += [ranges[0], (7, 7)]
    assert np.array_equal(np.array(ranges), c["ranges"])
    poses0 = torch.from_numpy(c["poses0"]).to(dev)
    before = dscenes.objects.clone()
    poses, stats, mask = reg.refine_scene_poses(dscenes, T["pairs"], poses0, points, ranges, min_inliers=RC.TOY_MIN_INLIERS, write_back=False)
    assert torch.equal(dscenes.objects, before)
    assert np.array_equal(poses.view(np.int64), want_poses.view(np.int64)) and np.array_equal(stats.view(np.int64), want_stats.view(np.int64))
    want_mask = reg.accepted_mask(want_stats, T["pairs"], RC.TOY_MIN_INLIERS)
    assert np.array_equal(mask, want_mask) and mask.sum() == 3 and not mask[3] and not mask[5]
    again = reg.refine_scene_poses(dscenes, T["pairs"], poses0, points, ranges, min_inliers=RC.TOY_MIN_INLIERS)
    assert np.array_equal(again[0].view(np.int64), poses.view(np.int64)) and np.array_equal(again[2], mask)
    refined = [[starts[s][o].copy() for o in range(2)] for s in range(2)]
    for m in np.nonzero(mask)[0]:
        s, o = T["pairs"][m]
        refined[s][o] = reg.pose_mats(poses[m: m + 1])[0]
        assert np.linalg.norm(refined[s][o][:3, 3] - truth[s, o][:3, 3]) < 0.5 * RC.TOY_DELTA
    direct = build(refined)
    torch.cuda.synchronize()
    assert torch.equal(dscenes.objects, direct.objects) and dscenes.host_objects["pose_inv"].tobytes() == direct.host_objects["pose_inv"].tobytes()
    model = rb.PandaModel(seed=0)
    robot = ops.robot_blob(model, dev)
    joints = torch.from_numpy(np.tile(np.array([0.0, 0.3, 0.0, -1.8, 0.0, 2.1, 0.8, 0.04, 0.04]), (2, 1, 1))).to(dev)  # the hand above the objects
    a, b = ops.fk_sdf(robot, model.points_per_link, dscenes, joints), ops.fk_sdf(robot, model.points_per_link, direct, joints)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    moved = ops.fk_sdf(robot, model.points_per_link, build(starts), joints)
    assert (a[0] != 0).sum() > 20 and not torch.equal(moved[0], a[0])   # the robot feels the objects, and feels them move


def test_a_short_seeded_fuzz_run(dev):
    spec = importlib.util.spec_from_file_location("fuzz_register", Path(__file__).resolve().parent / "fuzz" / "fuzz_register.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    assert fuzz.main(trials=30, seed=20261) == 0
