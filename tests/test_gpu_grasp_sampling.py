"""Grasp sampling on the MI355X (csrc/omg_grasp.hip): omgx_mesh_raycast against grasps.mesh_raycast bit for
bit around the LDS tile, the workgroup size and the chunk split; a ragged batch against single launches; omgx_grasp_poses against
grasps.grasp_poses on volumes omgx_mesh_sdf wrote into a pool; and the chain from meshes to plans."""
from __future__ import annotations

import numpy as np
import pytest

from test_grasp_sampling_cpu import CONE, chain
from tests import grasp_cases as GC
from tests import mesh_cases as MC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RAY_COUNTS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _same(t, face, want_t, want_face):
    """t as int64 bits and face, device against specification."""
    torch.cuda.synchronize()
    return (torch.equal(t.cpu().view(torch.int64), torch.from_numpy(np.ascontiguousarray(want_t)).view(torch.int64)) and
            torch.equal(face.cpu(), torch.from_numpy(np.ascontiguousarray(want_face))))


_TRUNCATED = {}


def truncated_sphere(nf):
    """icosphere(3)'s first nf faces (an open mesh), 257 rays — cracks through its vertices and edges, rays that leave it, rays in
    the planes of faces, random ones — and the specification's answer, computed once."""
    from omg_planner_amd import grasps as G
    if nf not in _TRUNCATED:
        v, f = MC.icosphere(3)
        f = np.ascontiguousarray(f[:nf])
        parts = [GC.sphere_crack_rays(v, f, 60)[:2], GC.outward_rays(v, f, 16), GC.mixed_rays(v, f, 181, seed=nf)]
        o = np.ascontiguousarray(np.concatenate([p[0] for p in parts]))
        d = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
        order = np.random.RandomState(nf).permutation(len(o))  # every ray count gets some of each kind
        o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
        t, face = G.mesh_raycast(v, f, o, d)
        assert (face >= 0).sum() > 40 and (face < 0).sum() > 40 and not np.isnan(t).any()
        _TRUNCATED[nf] = (v, f, o, d, t, face)
    return _TRUNCATED[nf]


@pytest.mark.parametrize("chunks", [1, 2, 7, 0])
@pytest.mark.parametrize("faces_vs_tile", [-1, 0, 1, "2T+1"])
def test_ray_cast_equals_the_specification_bit_for_bit(dev, faces_vs_tile, chunks):
    from omg_planner_amd import _lib, ops
    T = int(_lib.lib().omgx_mesh_sdf_tile())
    nf = 2 * T + 1 if faces_vs_tile == "2T+1" else T + faces_vs_tile
    v, f, o, d, want_t, want_face = truncated_sphere(nf)
    for n in RAY_COUNTS:
        t, face = ops.mesh_raycast(v, f, o[:n], d[:n], chunks=chunks, device=dev)
        assert t.dtype == torch.float64 and face.dtype == torch.int32 and t.shape == (n,)
        assert _same(t, face, want_t[:n], want_face[:n]), (nf, chunks, n)


def test_ragged_batch_equals_single_launches(dev):
    """Four meshes with (65, 0, 1, 257) rays at scattered rows between sentinels: the batch (automatic chunks, and a forced 3)
    equals the single launches and the specification bit for bit, and no other row is written."""
    from omg_planner_amd import grasps as G, ops
    meshes = [MC.box_mesh(MC.BOX_HALF), MC.box_mesh(MC.BOX_HALF, GC.BOX_POSE), MC.icosphere(2), MC.icosphere(3)]
    counts, begins, N = (65, 0, 1, 257), (5, 100, 90, 120), 400
    o, d = np.full((N, 3), 1e30), np.full((N, 3), 1e30)
    for m, (v, f) in enumerate(meshes):
        if counts[m]:
            extra = GC.box_diagonal_rays(GC.BOX_POSE if m == 1 else None, 3) if m < 2 else GC.sphere_crack_rays(v, f, 30)
            k = min(len(extra[0]), counts[m] - 1)
            rows = slice(begins[m], begins[m] + counts[m])
            o[rows], d[rows] = GC.mixed_rays(np.asarray(v), np.asarray(f), counts[m], seed=m)
            o[begins[m]: begins[m] + k], d[begins[m]: begins[m] + k] = extra[0][:k], extra[1][:k]
    d_o, d_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    owned = np.zeros(N, bool)
    for m in range(4):
        owned[begins[m]: begins[m] + counts[m]] = True
    for chunks in (0, 3):
        t = torch.full((N,), -7.0, dtype=torch.float64, device=dev)
        face = torch.full((N,), -9, dtype=torch.int32, device=dev)
        batch = ops.RayBatch(meshes, counts, ray_begins=begins, num_rays=N, chunks=chunks, device=dev)
        got = ops.mesh_raycast_batch(batch, d_o, d_d, out=(t, face))
        assert got[0] is t and got[1] is face
        torch.cuda.synchronize()
        ht, hf = t.cpu().numpy(), face.cpu().numpy()
        assert (ht[~owned] == -7.0).all() and (hf[~owned] == -9).all()
        for m, (v, f) in enumerate(meshes):
            if not counts[m]:
                continue
            rows = slice(begins[m], begins[m] + counts[m])
            st, sf = ops.mesh_raycast(v, f, o[rows], d[rows], chunks=1, device=dev)
            assert _same(st, sf, ht[rows], hf[rows]), (chunks, m)
            want_t, want_f = G.mesh_raycast(v, f, o[rows], d[rows])
            assert np.array_equal(ht[rows].view(np.int64), want_t.view(np.int64)) and np.array_equal(hf[rows], want_f), (chunks, m)
    # a batch without a single ray is legal and launches nothing
    batch = ops.RayBatch(meshes[:2], (0, 0), num_rays=4, chunks=0, device=dev)
    t, face = ops.mesh_raycast_batch(batch, d_o[:4].contiguous(), d_d[:4].contiguous())
    assert (t == 0).all() and (face == 0).all()


@pytest.fixture(scope="module")
def pooled(dev):
    """Three volumes written by ops.mesh_sdf_batch into one pool at non-zero offsets (both sample conventions), and 512 contact
    pairs per mesh from the specification's chain."""
    from omg_planner_amd import ops, scenes as sc
    names, samples = ("box", "posed_box", "small_sphere"), ("centre", "node", "centre")
    cs_ = [chain(n) for n in names]
    meshes = [(c["v"], c["f"]) for c in cs_]
    sizes = [int(np.prod(sc.mesh_grid_layout(c["v"], 0.005, 4)[1])) for c in cs_]
    offsets = [17, 17 + sizes[0] + 1000, 17 + sizes[0] + 1000 + sizes[1] + 3]
    pool = torch.full((offsets[2] + sizes[2] + 50,), float("nan"), dtype=torch.float32, device=dev)
    grids, origins, deltas, _ = ops.mesh_sdf_batch(meshes, 0.005, 4, list(samples), out=pool, out_offsets=offsets)
    torch.cuda.synchronize()
    spec_grids = [sc.SdfGrid(g.cpu().numpy(), origins[m], deltas[m]) for m, g in enumerate(grids)]
    layout = [(origins[m], deltas[m], samples[m], tuple(grids[m].shape), offsets[m]) for m in range(3)]
    return dict(chains=cs_, meshes=meshes, samples=samples, pool=pool, grids=spec_grids, layout=layout)


@pytest.mark.parametrize("clearance,probe_points", [(0.0, 100), (0.004, 1), (0.004, 100)])
def test_poses_kernel_equals_the_specification(dev, pooled, clearance, probe_points):
    from omg_planner_amd import grasps as G, ops
    cs_ = pooled["chains"]
    probe = G.default_probe()[:probe_points] if probe_points > 1 else G.default_probe()[82:83]  # the middle of the palm
    angles = G.approach_angles(8)
    batch = ops.RayBatch(pooled["meshes"], [512] * 3, chunks=2, device=dev, layout=pooled["layout"])
    up = lambda key, dtype=np.float64: torch.from_numpy(np.ascontiguousarray(np.concatenate([c[key] for c in cs_]), dtype)).to(dev)
    poses, valid = ops.grasp_poses(batch, up("p1"), up("n1"), up("d"), up("t"), up("f2", np.int32), up("nrm"), angles, probe, pooled["pool"],
                                   cos_cone=float(np.cos(CONE)), clearance=clearance)
    torch.cuda.synchronize()
    poses, valid = poses.cpu().numpy(), valid.cpu().numpy()
    assert poses.shape == (1536, 8, 4, 4) and valid.dtype == np.uint8
    total = 0
    for m, c in enumerate(cs_):
        want_p, want_v, _ = G.grasp_poses(c["p1"], c["n1"], c["d"], c["t"], c["f2"], c["nrm"], angles, pooled["grids"][m], probe, cone=CONE,
                                          clearance=clearance, sample=pooled["samples"][m])
        rows = slice(512 * m, 512 * (m + 1))
        assert np.array_equal(poses[rows].view(np.int64), want_p.view(np.int64)), m
        assert np.array_equal(valid[rows].astype(bool), want_v), m
        total += int(want_v.sum())
        assert 0 < want_v.sum() < (want_p[:, :, 3, 3] == 1).sum()  # some pairs pass the gripper check and some fail it
    assert total > 0


def test_sample_grasp_sets_equals_the_specification(dev):
    from omg_planner_amd import grasps as G
    names = ("box", "posed_box", "small_sphere")
    meshes = [(chain(n)["v"], chain(n)["f"]) for n in names]
    grids = [chain(n)["grid"] for n in names]
    # one stream per mesh, with the draw of max_grasps
    got = G.sample_grasp_sets(meshes, grids, 300, 8, [np.random.RandomState(10 + s) for s in range(3)], cone=CONE, max_grasps=40, device=dev)
    for s in range(3):
        want = G.sample_grasps(*meshes[s], grids[s], 300, 8, np.random.RandomState(10 + s), cone=CONE, max_grasps=40)
        assert got[s].shape == want.shape == (40, 4, 4) and np.array_equal(got[s], want), s
    # one stream for all, every valid grasp; a flipped mesh gives the same set
    flipped = [(meshes[0][0], meshes[0][1][:, ::-1].copy())] + meshes[1:]
    got = G.sample_grasp_sets(flipped, grids, 300, 8, np.random.RandomState(2), cone=CONE, chunks=3, device=dev)
    rng = np.random.RandomState(2)
    for s in range(3):
        want = G.sample_grasps(*meshes[s], grids[s], 300, 8, rng, cone=CONE)
        assert len(want) > 0 and np.array_equal(got[s], want), s
    # the volumes read in place from a scene table's pool (origin and voxel size as its records hold them: float32)
    from omg_planner_amd import ops, scenes as sc
    from omg_planner_amd.config import Config
    table = ops.DeviceScenes.from_scenes(_box_scenes(), Config().layer_kwargs(), device=dev)
    got = G.sample_grasp_sets([meshes[0]] * 2, table, 300, 8, [np.random.RandomState(5), np.random.RandomState(6)], cone=CONE, device=dev)
    for s in range(2):
        rec = table.host_objects[int(table.host_scene_begin[s])]
        grid = sc.SdfGrid(grids[0].data, rec["lo"].astype(np.float64), float(rec["delta"]))
        want = G.sample_grasps(*meshes[0], grid, 300, 8, np.random.RandomState(5 + s), cone=CONE)
        assert len(want) > 0 and np.array_equal(got[s], want), s


BOX_ON_TABLE = (0.5, 0.0, 0.125, 0.4)  # x, y, z, yaw of the standing box (its thin axis horizontal)


def _box_scenes():
    """Two tabletop scenes whose target is the test box standing on its 0.10 x 0.06 side, its volume from scenes.mesh_sdf."""
    from omg_planner_amd import scenes as sc
    grid = chain("box")["grid"]
    x, y, z, yaw = BOX_ON_TABLE
    stand = MC.pose((np.pi / 2, 0.0, 0.0))  # the box's y axis up, its z (the 0.06 side) horizontal
    out = []
    for seed in (3, 4):
        scene = sc.make_tabletop_scene(seed, num_objects=1, grid=32, table_grid=(48, 32, 16))
        scene.objects[0] = sc.SceneObject("box", sc._yaw_pose(x, y, z, yaw + 0.5 * (seed - 3)) @ stand, grid)
        out.append(scene)
    return out


def test_plan_meshes_from_device_and_specification_grasps(dev):
    """plan_meshes on two tabletop scenes with the box as target: the grasps the device sampled equal the specification's, and
    the trajectories equal those of plan_grasps on the specification's grasps (sample_grasps on the host). The box stands on its
    0.10 x 0.06 side at BOX_ON_TABLE = (x 0.5, y 0.0, z 0.125, yaw 0.4 and 0.9), so that its thin axis is horizontal and the
    hand can come from above; on the MI355X that gave 64 and 64 grasps (256 rays x 8 angles, max_grasps 64), 79 and 145
    collision-free goals, goal sets of 45 and 56, and both scenes planned."""
    from omg_planner_amd import grasps as G, pipeline, robot as rb
    from omg_planner_amd.config import Config
    cfg = Config(use_standoff=True, timeout=-1, silent=True)
    model = rb.PandaModel()
    scenes = _box_scenes()
    meshes = [MC.box_mesh(MC.BOX_HALF)] * 2
    start = np.tile(np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785, 0.04, 0.04]), (2, 1))

    rngs = lambda: [np.random.RandomState(7), np.random.RandomState(8)]
    res, sets = pipeline.plan_meshes(model, scenes, meshes, start, cfg, n_rays=256, n_angles=8, ol_alg="MD", rng=np.random.RandomState(0),
                                     grasp_rng=rngs(), max_grasps=64, device=dev, cone=CONE)
    grids = [s_.objects[s_.target_idx].sdf for s_ in scenes]
    ref_sets = [G.sample_grasps(*meshes[s], grids[s], 256, 8, rngs()[s], cone=CONE, max_grasps=64) for s in range(2)]
    ref = pipeline.plan_grasps(model, scenes, ref_sets, start, cfg, ol_alg="MD", rng=np.random.RandomState(0), device=dev)
    print("grasps", [len(s) for s in sets], "goals", res.goal_counts.tolist(), "free", np.asarray(res.num_free).tolist(),
          "planned", res.planned.tolist())
    assert all(np.array_equal(a, b) for a, b in zip(sets, ref_sets)) and all(len(s) > 0 for s in sets)
    assert res.planned.any() and np.array_equal(res.planned, ref.planned)
    assert torch.equal(res.traj, ref.traj) and torch.equal(res.goal_idx, ref.goal_idx) and torch.equal(res.goal_set, ref.goal_set)
    gi = res.goal_idx.cpu().numpy()
    assert all(0 <= gi[s] < res.goal_counts[s] for s in np.flatnonzero(res.planned))
    info = res.info.cpu().numpy()
    assert np.isfinite(info[res.planned, 0]).all()
