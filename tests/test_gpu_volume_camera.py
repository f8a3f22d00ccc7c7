"""The depth camera on the SDF pool on the MI355X (csrc/omg_volume_camera.hip): omgx_render_volumes against
volume_camera.py bit for bit: a ragged batch between guard values through the C ABI, the rule's edges against their written
answers, a pose written on the device and seen at once, camera.observe_volumes on the observed scene (clouds, a plane
half-space against observe_table's route), a TSDF-fused volume rendered back onto the frame it came from, and a short seeded
fuzz run.  Every launch is followed by a checked synchronise."""
from __future__ import annotations

import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import volume_camera_cases as VC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _table(dev, objects, begin, pool):
    from omg_planner_amd import ops, scenes as sc
    return ops.DeviceScenes(sc.SceneBatch(objects, begin, pool), device=dev)


def _host(images):
    return tuple(None if x is None else x.cpu().numpy() for x in images)


def test_ragged_batch_between_guards_against_the_specification(dev):
    """S = 3 scenes with 0, 1 and 3 objects (dims (16,16,16); (5,9,7), (2,2,2), (5,9,7) again: one volume twice), pool offsets
    neither zero nor in order, a 17 x 33 image (partial tiles both ways; in scene 2 the wave of the first 8 x 8 block meets no box
    while the one beside it marches), the camera of scene 1 inside its volume's box: ONE launch through the C ABI gives the
    specification's images bit for bit, every element between the guard values is overwritten and nothing outside them is; with
    normal_out and steps_out NULL t and inst are the same."""
    from omg_planner_amd import _lib
    objects, begin, pool, cams, want = VC.ragged_batch()
    S, H, W = 3, VC.RAGGED_H, VC.RAGGED_W
    assert [tuple(r["dim"]) for r in objects] == [(16, 16, 16), (5, 9, 7), (2, 2, 2), (5, 9, 7)] and objects["grid_offset"][1] == objects["grid_offset"][3]
    assert (want[3][2][:8, :8] == 0).all() and (want[3][2][:8, 8:16] > 0).any() and set(np.unique(want[1][2])) == {-1, 0, 1, 2}
    assert (want[1][0] == -1).all() and (want[1][1] == 0).sum() > 300 and want[3][1].min() >= 1 and want[3][1].max() > 20
    l, vp = _lib.lib(), C.c_void_p
    ptr = lambda x: vp(x.data_ptr())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_objects, d_begin, d_pool, d_cams = up(objects.view(np.uint8)), up(begin), up(pool), up(cams)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    n, pad = S * H * W, 7
    a = VC.RAGGED_ARGS

    def launch(with_normals):
        bufs = [torch.full((k * n + 2 * pad,), g, dtype=dt, device=dev)
                for k, g, dt in ((1, 7.5, torch.float64), (1, 77, torch.int32), (3, 7.5, torch.float64), (1, 77, torch.int32))]
        inner = [b[pad: b.numel() - pad] for b in bufs]
        rc = l.omgx_render_volumes(ptr(d_objects), vp(objects.ctypes.data), len(objects), ptr(d_begin), vp(begin.ctypes.data), S, ptr(d_pool), len(pool),
                                   ptr(d_cams), vp(cams.ctypes.data), None, None, H, W, a["level"], a["t_min"], a["min_step"], a["relax"], a["max_steps"],
                                   ptr(inner[0]), ptr(inner[1]), ptr(inner[2]) if with_normals else None, ptr(inner[3]) if with_normals else None, stream)
        assert rc == 0, l.omgx_last_error()
        torch.cuda.synchronize()
        return [b.cpu().numpy() for b in bufs]

    for with_normals in (True, False):
        t, inst, normal, steps = launch(with_normals)
        for h, g in ((t, 7.5), (inst, 77), (normal, 7.5), (steps, 77)):
            assert (h[:pad] == g).all() and (h[-pad:] == g).all()
        assert VC.same_bits(t[pad:-pad].reshape(S, H, W), want[0]) and np.array_equal(inst[pad:-pad].reshape(S, H, W), want[1]), with_normals
        if with_normals:
            assert VC.same_bits(normal[pad:-pad].reshape(S, H, W, 3), want[2]) and np.array_equal(steps[pad:-pad].reshape(S, H, W), want[3])
            assert not (inst[pad:-pad] == 77).any() and not (steps[pad:-pad] == 77).any()  # (7.5 is no answer either: every element was written)
            assert not (t[pad:-pad] == 7.5).any() and not (normal[pad:-pad] == 7.5).any()
        else:
            assert (normal == 7.5).all() and (steps == 77).all()
    # no scenes: nothing is launched
    assert l.omgx_render_volumes(ptr(d_objects), vp(objects.ctypes.data), len(objects), None, None, 0, ptr(d_pool), len(pool), None, None, None, None, H, W,
                                 0.0, 0.0, 0.001, 1.0, 8, None, None, None, None, stream) == 0
    torch.cuda.synchronize()


def test_edges_as_batches_against_the_written_answers(dev):
    """The edges of the rule (VC.EDGE_CASES), the cases that share their arguments as the scenes of one launch: the device gives the
    answers written out in tests/volume_camera_cases.py."""
    from omg_planner_amd import ops
    for args, idx in VC.edge_groups():
        objects, begin, pool, cameras, visible, _ = VC.edge_batch(idx)
        got = ops.render_volumes(_table(dev, objects, begin, pool), cameras, 1, 1, visible=visible, want_normals=True, want_steps=True, **args)
        torch.cuda.synchronize()
        VC.edge_check(idx, *_host(got))


def test_a_pose_written_on_the_device_is_seen_at_once(dev):
    """set_object_poses, then render_volumes without sync_host: the specification at the new pose.  Then the record's pose rows are
    written on the device alone, so that the host mirror is stale, which is what observe_table reads: the images follow the
    device, not the mirror."""
    from omg_planner_amd import ops, volume_camera as vc
    objects, begin, pool, cams, want = VC.ragged_batch()
    table = _table(dev, objects, begin, pool)
    H, W, a = VC.RAGGED_H, VC.RAGGED_W, VC.RAGGED_ARGS
    spec = lambda recs: vc.render_volumes(recs, begin, pool, cams, H, W, **a)
    render = lambda: _host(ops.render_volumes(table, cams, H, W, want_normals=True, want_steps=True, **a))
    assert VC.same_images(render(), want)
    moved = VC.random_pose(np.random.default_rng(11), 0.0)
    moved[:3, 3] = (-0.05, 0.01, 0.02)
    table.set_object_poses([(2, 0)], moved[None])
    got = render()
    torch.cuda.synchronize()
    first = spec(table.host_objects)  # (set_object_poses keeps the mirror)
    assert VC.same_images(got, first) and not np.array_equal(first[1], want[1])
    # the device alone
    again = np.eye(4)
    again[:3, 3] = (-0.04, -0.01, 0.0)
    rows = np.linalg.inv(again)[:3].astype(np.float32).reshape(1, 12)
    k = table._index(2, 0)
    table.objects.view(-1, objects.dtype.itemsize)[k, :48].copy_(torch.from_numpy(rows.view(np.uint8).reshape(48)).to(dev))
    got = render()
    torch.cuda.synchronize()
    on_device = table.host_objects.copy()
    on_device["pose_inv"][k] = rows[0]
    second = spec(on_device)
    assert np.array_equal(table.host_objects["pose_inv"][k], first_pose_rows(moved)) and VC.same_images(got, second)
    assert not VC.same_bits(second[0], first[0])
    assert np.array_equal(table.sync_host()["pose_inv"][k], rows[0])


def first_pose_rows(pose):
    from omg_planner_amd import scenes as sc
    return sc.se3_inverse(pose)[:3, :4].astype(np.float32).ravel()


# ---------------------------------------------------------------------------------------------------------------------
# the observed scene of fusion_cases: a sphere above a slab, three cameras, as three scenes of one table
# ---------------------------------------------------------------------------------------------------------------------
def _scene_table(dev, reserve=0):
    from omg_planner_amd import ops, scenes as sc
    sphere = sc.sphere_sdf(FC.SPHERE_R, (20, 20, 20), 0.01)
    slab = sc.box_sdf(tuple(FC.SLAB_HALF), (56, 56, 8), 0.01)
    lifted = np.eye(4)
    lifted[:3, 3] = FC.SPHERE_C
    made = [sc.Scene([sc.SceneObject("sphere", lifted, sphere), sc.SceneObject("slab", np.eye(4), slab)], 0) for _ in range(3)]
    return ops.DeviceScenes.from_scenes(made, device=dev, reserve_voxels=reserve)


def test_observe_volumes_clouds_and_a_plane_halfspace_against_observe_table(dev):
    """camera.observe_volumes on the sphere and the slab as volumes: clouds(1) equals camera.pixel_clouds of the specification's
    images bit for bit (and clouds(0) is the sphere).  Then the slab's volume is replaced by the half-space under its top
    (plane_obstacles) and rendered alone by both routes: camera.explained_mask of the observed depth is the same mask, except on
    pixels within one pixel of the sheet's silhouette (the volume also shows the thin side of its box there, and surface nets
    end half a cell inside it); their number is printed: 140 of 4830 on the MI355X, as in numpy."""
    from omg_planner_amd import camera, volume_camera as vc
    cfw, intr = FC.scene_cameras()
    table = _scene_table(dev, reserve=3 * 52 * 52 * 4)
    obs = camera.observe_volumes(table, cfw, intr, FC.H, FC.W, want_normals=True, min_step=0.0005, max_steps=256)
    clouds = [[c.cpu().numpy() for c in obs.clouds(cls)] for cls in (0, 1)]
    torch.cuda.synchronize()
    cams = np.stack([camera.camera_rows(intr, cfw[s]) for s in range(3)])
    want = vc.render_volumes(table.host_objects, table.host_scene_begin, table.pool.cpu().numpy(), cams, FC.H, FC.W, min_step=0.0005, max_steps=256)
    assert VC.same_images(_host((obs.t, obs.inst, obs.normals, None)), want) and obs.face is None
    labels = np.array([0, 1] * 3)
    for cls in (0, 1):
        spec = camera.pixel_clouds(want[0], want[1], labels, table.host_scene_begin, cams, cls)
        for s in range(3):
            assert len(spec[s]) > 100 and np.array_equal(clouds[cls][s].view(np.int64), spec[s].view(np.int64)), (cls, s)
    # the images are the scene's: near the triangle camera's
    t_mesh = FC.scene_depth()[0]
    both = np.isfinite(want[0]) & np.isfinite(t_mesh)
    assert both.mean() > 0.5 and np.median(np.abs(want[0][both] - t_mesh[both])) < 0.005
    # the half-space under the slab's top on a 1 cm layout, its lowest layer of samples a quarter of a voxel under the plane: the
    # side of the box and the half cell by which surface nets end inside it are both less than a pixel here
    layout = ((-0.26, -0.26, FC.SLAB_HALF[2] - 0.0075), 0.01, (52, 52, 4))
    pairs = [(s, 1) for s in range(3)]
    table.plane_obstacles(pairs, np.tile([0.0, 0.0, 1.0, -FC.SLAB_HALF[2]], (3, 1)), [layout] * 3)
    torch.cuda.synchronize()
    skip = [(s, 0) for s in range(3)]
    by_volume = camera.observe_volumes(table, cfw, intr, FC.H, FC.W, skip=skip, min_step=0.0005, max_steps=256)
    by_mesh = camera.observe_table(table, cfw, intr, FC.H, FC.W, skip=skip)
    t = torch.from_numpy(t_mesh).to(dev)
    tol = 0.005
    mask_v, mask_m = camera.explained_mask(t, by_volume.t, tol).cpu().numpy(), camera.explained_mask(t, by_mesh.t, tol).cpu().numpy()
    torch.cuda.synchronize()
    seen = np.isfinite(by_mesh.t.cpu().numpy())
    grown, shrunk, edged = seen.copy(), seen.copy(), np.pad(seen, ((0, 0), (1, 1), (1, 1)), mode="edge")
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            grown |= edged[:, dr: dr + FC.H, dc: dc + FC.W]
            shrunk &= edged[:, dr: dr + FC.H, dc: dc + FC.W]
    differ = mask_v != mask_m
    print(f"explained_mask: {int(differ.sum())} of {int(mask_m.sum())} pixels differ, all within one pixel of the silhouette")
    assert mask_m.sum() > 1000 and not (differ & ~(grown & ~shrunk)).any()
    assert (by_volume.inst.cpu().numpy()[mask_v] == 1).all()


def test_a_fused_volume_renders_back_onto_its_frame(dev):
    """The scene's three depth images integrated into a table's obstacle (integrate_obstacles: a TSDF-blended volume) and rendered
    from the first camera with relax = 0.5: the device equals the specification on the downloaded pool, and the share of the
    pixels finite in both images whose predicted depth lies within the truncation of the observed one (printed: 0.9076 of 844;
    the rest lie on silhouettes, where the two images show different surfaces) is at least the specification's."""
    from omg_planner_amd import camera, ops, scenes as sc, volume_camera as vc
    from tests import tsdf_cases as TC
    t_host, views = FC.scene_depth()
    t = torch.from_numpy(t_host).to(dev)
    made = [sc.Scene([sc.SceneObject("obstacles", np.eye(4), sc.sphere_sdf(0.05, (8, 8, 8), 0.05))], 0)]
    table = ops.DeviceScenes.from_scenes(made, device=dev, reserve_voxels=2 * int(np.prod(FC.DIMS)))
    table.integrate_obstacles([(0, 0)], None, t, views, [(0, 3)], [(FC.ORIGIN, FC.DELTA, FC.DIMS)], TC.TRUNC, FC.NEAR, reach=0.1)
    torch.cuda.synchronize()
    cfw, intr = FC.scene_cameras()
    cams = camera.camera_rows(intr, cfw[0])[None]
    args = dict(relax=0.5, min_step=FC.DELTA / 16, max_steps=512)
    got = _host(ops.render_volumes(table, cams, FC.H, FC.W, want_normals=True, want_steps=True, **args))
    torch.cuda.synchronize()
    recs = table.sync_host()
    assert tuple(recs[0]["dim"]) == FC.DIMS
    want = vc.render_volumes(recs, table.host_scene_begin, table.pool.cpu().numpy(), cams, FC.H, FC.W, **args)
    assert VC.same_images(got, want)

    def share(pred):
        both = np.isfinite(pred) & np.isfinite(t_host[0])
        return float((np.abs(pred[both] - t_host[0][both]) <= TC.TRUNC).sum()) / max(int(both.sum()), 1), int(both.sum())
    (mine, n), (spec, _) = share(got[0][0]), share(want[0][0])
    print(f"{mine:.4f} of the {n} pixels finite in both images lie within the truncation ({TC.TRUNC} m) of the observed depth")
    assert n > 500 and mine >= spec > 0


def test_scene_range_views_render_their_scenes(dev):
    from omg_planner_amd import ops
    objects, begin, pool, cams, want = VC.ragged_batch()
    table = _table(dev, objects, begin, pool)
    got = _host(ops.render_volumes(table.scene_range(1, 3), cams[1:], VC.RAGGED_H, VC.RAGGED_W, want_normals=True, want_steps=True, **VC.RAGGED_ARGS))
    torch.cuda.synchronize()
    assert VC.same_images(got, tuple(w[1:] for w in want))
    batch = ops.VolumeCameraBatch(table, cams, [0, 1, 0, 1])
    assert batch.num_scenes == 3 and batch.h_inst_begin.tolist() == [0, 0, 1, 4] and batch.h_cameras["inst_count"].tolist() == [0, 1, 3]


def test_a_short_seeded_fuzz_run(dev):
    spec = importlib.util.spec_from_file_location("fuzz_volume_camera", Path(__file__).resolve().parent / "fuzz" / "fuzz_volume_camera.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    assert fuzz.main(trials=fuzz.SMOKE_TRIALS, seed=fuzz.SMOKE_SEED) == 0


def partial_tiles_case():
    """The 8^3 sphere as the one object of two scenes, before two cameras of 17 x 33 pixels (2 x 3 tiles, partial both ways): in view
    0 it lies over the corner where four tiles meet, in view 1 over the image's last row and last column -> (objects, scene_begin,
    pool, cameras, arguments, the specification's images)."""
    from omg_planner_amd import camera, volume_camera as vc
    objects, _, pool, delta = VC.sphere_table(8)
    assert tuple(objects["dim"][0]) == (8, 8, 8)
    objects, begin = np.concatenate([objects, objects]), np.array([0, 1, 2], np.int32)
    cfw = np.eye(4)
    cfw[:3, 3] = -VC.SPHERE_EYE
    cams = np.stack([camera.camera_rows((50.0, 46.0, 16.0, 16.0), cfw), camera.camera_rows((44.0, 50.0, 31.0, 15.5), cfw)])
    args = dict(min_step=delta / 16, max_steps=256, relax=1.0)
    want = vc.render_volumes(objects, begin, pool, cams, 17, 33, **args)
    hit = want[1] >= 0
    assert all(hit[0, r, c] for r in (15, 16) for c in (15, 16)) and hit[1, 16].any() and hit[1, :, 32].any()  # across the tiles' borders
    assert all(h.any() and not h.all() for h in hit) and not hit[1, 16].all() and not hit[1, :, 32].all()
    return objects, begin, pool, cams, args, want


def test_partial_tiles_of_two_views_equal_the_specification(dev):
    """The smallest launch in which a wrong tile map or a wrong clamp of the lanes outside the image shows: 17 x 33 pixels and two
    views of one 8^3 volume.  Depth and normal as bits, object and steps equal volume_camera.render_volumes, and the cloud of
    pixel_clouds on the same images equals camera.pixel_clouds as bits."""
    from omg_planner_amd import camera, ops
    objects, begin, pool, cams, args, want = partial_tiles_case()
    table = _table(dev, objects, begin, pool)
    got = ops.render_volumes(table, cams, 17, 33, want_normals=True, want_steps=True, **args)
    torch.cuda.synchronize()
    assert got[0].shape == (2, 17, 33) and VC.same_images(_host(got), want)
    labels = [1, 0]
    batch = ops.VolumeCameraBatch(table, cams, labels)
    for cls in (-1, 1):
        spec = camera.pixel_clouds(want[0], want[1], labels, table.host_scene_begin, cams, cls)
        points, at = ops.pixel_clouds(batch, got[0], got[1], cls)
        torch.cuda.synchronize()
        assert len(spec[0]) > 0 and at.tolist() == [0, len(spec[0]), len(spec[0]) + len(spec[1])], cls
        assert np.array_equal(points.cpu().numpy().view(np.int64), np.concatenate(spec).view(np.int64)), cls
