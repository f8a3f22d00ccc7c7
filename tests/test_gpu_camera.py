"""The depth camera on the MI355X (csrc/omg_camera.hip): omgx_render_depth against camera.render_depth bit
for bit around the pixel tile and the LDS face tile, with and without the cull and the face image; a launch of three scenes
against single launches between sentinels; the clouds against camera.pixel_clouds around the group of 256 pixels; the render
against the per-instance ray casts it replaces; and the chain from scenes to an obstacle volume."""
from __future__ import annotations

import numpy as np
import pytest

from tests import camera_cases as CC
from tests import mesh_cases as MC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


_BATCH = {}


def batch_of(name, dev):
    from omg_planner_amd import ops
    if name not in _BATCH:
        sc = CC.scene(name)
        _BATCH[name] = ops.CameraBatch(sc["meshes"], sc["instances"], sc["inst_begin"], sc["cameras"], device=dev)
    return _BATCH[name]


def _same(got, want):
    """t as int64 bits, inst and face (where asked for), device against specification."""
    torch.cuda.synchronize()
    ok = torch.equal(got[0].cpu().view(torch.int64), torch.from_numpy(np.array(want[0])).view(torch.int64))
    ok = ok and torch.equal(got[1].cpu(), torch.from_numpy(np.array(want[1])))
    return ok and (got[2] is None or torch.equal(got[2].cpu(), torch.from_numpy(np.array(want[2]))))


def _mixed(name):
    """A scene is only used once it shows hits and background (a single pixel: either)."""
    inst = CC.spec(name)[1]
    assert inst.size == 1 or ((inst >= 0).any() and (inst < 0).any()), name


@pytest.mark.parametrize("name", ["1x1", "15x17", "16x16", "17x33", "25x41", "inside_sphere", "overlap", "duplicate", "box_behind"])
def test_render_equals_the_specification_bit_for_bit(dev, name):
    """Image sizes around the 16 x 16 pixel tile (17x33 with the principal point outside the image), meshes of T - 1, T, T + 1 and
    2T + 1 faces for the LDS tile T and the box, a duplicate and an instance behind the camera; with the cull, without it, and
    without the face image."""
    from omg_planner_amd import _lib, ops
    sc = CC.scene(name)
    if name[0].isdigit():
        T = int(_lib.lib().omgx_mesh_sdf_tile())
        assert sorted(len(f) for _, f in sc["meshes"]) == [12, T - 1, T, T + 1, 2 * T + 1]
        _mixed(name)
    b = batch_of(name, dev)
    for cull in (True, False):
        got = ops.render_depth(b, sc["H"], sc["W"], cull=cull)
        assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
        assert got[0].shape == (1, sc["H"], sc["W"])
        assert _same(got, CC.spec(name, cull)), (name, cull)
        bare = ops.render_depth(b, sc["H"], sc["W"], cull=cull, want_face=False)
        assert bare[2] is None and _same(bare, CC.spec(name, cull)), (name, cull)


@pytest.mark.parametrize("name", CC.RANDOM[:4])
def test_random_scenes_equal_the_specification(dev, name):
    from omg_planner_amd import ops
    sc = CC.scene(name)
    inst = CC.spec(name)[1][0]
    seen = CC.labels(sc)[inst[inst >= 0]]
    assert (inst >= 0).any() and (inst < 0).any() and (seen == 0).any() and (seen == 1).any()
    for cull in (True, False):
        assert _same(ops.render_depth(batch_of(name, dev), sc["H"], sc["W"], cull=cull), CC.spec(name, cull)), (name, cull)


def _guarded(shape, dtype, fill, dev, pad=300):
    """A tensor of `shape` inside a larger buffer of sentinels -> (view, buffer, pad)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    return buf[pad: pad + n].view(shape), buf, pad


def test_three_scenes_in_one_launch_equal_single_launches(dev):
    """S = 3 scenes with 0, 1 and 6 instances (a duplicate and one behind the camera among them) and three cameras in one
    launch: the specification's bits, the bits of three single-scene launches, and nothing written outside the images."""
    from omg_planner_amd import ops
    sc = CC.scene("multi")
    H, W = sc["H"], sc["W"]
    assert np.diff(sc["inst_begin"]).tolist() == [0, 1, 6]
    want = CC.spec("multi")
    assert (want[1][0] == -1).all() and (want[1][1] >= 0).any() and len(np.unique(want[1][2])) >= 4
    for cull in (True, False):
        (t, tb, pad), (ii, ib, _), (ff, fb, _) = (_guarded((3, H, W), dt, fill, dev) for dt, fill in
                                                   ((torch.float64, -7.0), (torch.int32, -9), (torch.int32, -9)))
        got = ops.render_depth(batch_of("multi", dev), H, W, cull=cull, out=(t, ii, ff))
        assert got[0] is t and _same(got, CC.spec("multi", cull))
        for buf, fill in ((tb, -7.0), (ib, -9), (fb, -9)):
            assert (buf[:pad] == fill).all() and (buf[-pad:] == fill).all()
        for s in range(3):
            one = CC.single(sc, s)
            b1 = ops.CameraBatch(one["meshes"], one["instances"], one["inst_begin"], one["cameras"], device=dev)
            assert _same(ops.render_depth(b1, H, W, cull=cull), [a[s: s + 1] for a in CC.spec("multi", cull)]), (cull, s)


def _spec_clouds(name, cls):
    from omg_planner_amd import camera as cam
    sc = CC.scene(name)
    t, inst, _ = CC.spec(name)
    return cam.pixel_clouds(t, inst, CC.labels(sc), sc["inst_begin"], sc["cameras"], cls)


@pytest.mark.parametrize("name", ["15x17", "16x16", "1x257", "25x41", "multi"])
def test_clouds_equal_the_specification_bit_for_bit(dev, name):
    """H * W = 255, 256, 257 and 4 * 256 + 1 pixels, and the three scenes of `multi` packed into one list: for classes that select
    nothing (9), a strict subset (0, 1, 2; 2 is everything in multi's second scene), and every hit (-1), the points in pixel order
    as int64 bits, scene_begin, sentinels around the packed rows, and a cap below the total."""
    from omg_planner_amd import ops
    sc = CC.scene(name)
    H, W = sc["H"], sc["W"]
    assert H * W == {"15x17": 255, "16x16": 256, "1x257": 257, "25x41": 1025, "multi": 561}[name]
    _mixed(name)
    b = batch_of(name, dev)
    t, inst, _ = (torch.from_numpy(np.array(a)).to(dev) for a in CC.spec(name))
    totals = {}
    for cls in (9, 0, 1, 2, -1):
        want = _spec_clouds(name, cls)
        begin = np.concatenate([[0], np.cumsum([len(w) for w in want])])
        flat = np.concatenate(want)
        totals[cls] = len(flat)
        points, got_begin = ops.pixel_clouds(b, t, inst, cls)
        torch.cuda.synchronize()
        assert points.dtype == torch.float64 and points.shape == (len(flat), 3) and points.is_contiguous()
        assert got_begin.tolist() == begin.tolist(), (name, cls)
        assert np.array_equal(points.cpu().numpy().view(np.int64), flat.view(np.int64)), (name, cls)
        # room for more rows than there are: the rest stays as it was; room for fewer: exactly `cap` rows are written
        for cap in (len(flat) + 7, max(len(flat) - 5, 0)):
            view, buf, pad = _guarded((cap, 3), torch.float64, -7.0, dev, pad=30)
            out, _ = ops.pixel_clouds(b, t, inst, cls, out=view)
            torch.cuda.synchronize()
            n = min(cap, len(flat))
            assert out is view and np.array_equal(view[:n].cpu().numpy().view(np.int64), flat[:n].view(np.int64)), (name, cls, cap)
            assert (view[n:] == -7.0).all() and (buf[:pad] == -7.0).all() and (buf[-pad:] == -7.0).all(), (name, cls, cap)
    assert totals[9] == 0 and 0 < totals[0] < totals[-1] and 0 < totals[1] < totals[-1] and totals[0] + totals[1] + totals[2] == totals[-1]
    if name == "multi":
        every = _spec_clouds(name, -1)
        assert len(every[0]) == 0 and len(_spec_clouds(name, 2)[1]) == len(every[1]) > 0   # class 2 is all of the second scene


def test_render_equals_the_per_instance_ray_casts_it_replaces(dev):
    """One small scene: every instance's rays moved to its frame by the specification's formula and cast by ops.mesh_raycast, the
    nearest over the instances taken in order with the strict <: the same t, instance and face as one render."""
    from omg_planner_amd import camera as cam, ops
    sc = CC.scene("15x17")
    H, W = sc["H"], sc["W"]
    dx, dy = cam.pixel_directions(sc["cameras"][0], H, W)
    best = torch.full((H * W,), float("inf"), dtype=torch.float64, device=dev)
    inst = torch.full((H * W,), -1, dtype=torch.int32, device=dev)
    face = torch.full((H * W,), -1, dtype=torch.int32, device=dev)
    for i, rec in enumerate(sc["instances"]):
        m = rec["m"]
        o = np.ascontiguousarray(np.broadcast_to(np.array([m[3], m[7], m[11]]), (H * W, 3)))
        d = np.ascontiguousarray(np.stack([(m[4 * k] * dx + m[4 * k + 1] * dy) + m[4 * k + 2] for k in range(3)], -1))
        t_i, f_i = ops.mesh_raycast(*sc["meshes"][int(rec["mesh"])], o, d, chunks=1, device=dev)
        take = torch.from_numpy(cam.instance_active(rec, dx, dy)).to(dev) & (t_i < best)
        best, inst, face = torch.where(take, t_i, best), torch.where(take, torch.full_like(inst, i), inst), torch.where(take, f_i, face)
    got = ops.render_depth(batch_of("15x17", dev), H, W)
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(-1).view(torch.int64), best.view(torch.int64)) and torch.equal(got[1].view(-1), inst)
    assert torch.equal(got[2].view(-1), face) and (inst >= 0).any()


def test_scenes_to_obstacle_volume(dev):
    """observe_scenes on the two scenes of `observed` (a table without a mesh, a target, obstacles; two cameras): the images equal
    the specification's, the label-1 cloud of each scene is a contiguous float64 tensor with the specification's bits, and
    ops.point_cloud_sdf of it equals scenes.point_cloud_sdf of the specification's cloud."""
    from omg_planner_amd import camera as cam, ops, scenes as S
    sc = CC.scene("observed")
    H, W = sc["H"], sc["W"]
    assert len(sc["meshes"]) == 2 and sc["inst_begin"].tolist() == [0, 3, 5]
    obs = cam.observe_scenes(sc["scenes"], sc["scene_meshes"], np.stack(sc["cam_from_world"]), sc["intrinsics"], H, W, device=dev)
    assert obs.batch.h_instances.tobytes() == sc["instances"].tobytes()      # the records the neutrality test walks
    want = CC.spec("observed")
    assert _same((obs.t, obs.inst, obs.face), want)
    spec_clouds = cam.pixel_clouds(want[0], want[1], CC.labels(sc), sc["inst_begin"], sc["cameras"], 1)
    clouds = obs.clouds(1)
    assert len(obs.clouds(0)) == 2 and all(len(c) > 0 for c in obs.clouds(0))
    for s in range(2):
        assert len(spec_clouds[s]) > 50 and clouds[s].is_contiguous() and clouds[s].dtype == torch.float64
        assert np.array_equal(clouds[s].cpu().numpy().view(np.int64), spec_clouds[s].view(np.int64)), s
        vol, origin, res = ops.point_cloud_sdf(clouds[s])
        ref = S.point_cloud_sdf(spec_clouds[s])
        torch.cuda.synchronize()
        assert np.array_equal(origin, ref.origin) and res == ref.delta
        assert torch.equal(vol.cpu(), torch.from_numpy(ref.data)), s


def test_no_scene_at_all(dev):
    """num_scenes == 0 is legal: the render launches nothing and returns empty images; the count writes scene_begin = [0] and the
    gather nothing.  An inst_begin that does not fit is still rejected."""
    from omg_planner_amd import _lib, ops
    sc = CC.scene("box_axis")
    b = ops.CameraBatch(sc["meshes"], sc["instances"], [0], np.zeros((0, 16)), device=dev)
    t, inst, face = ops.render_depth(b, 5, 7)
    assert t.shape == inst.shape == face.shape == (0, 5, 7)
    points, begin = ops.pixel_clouds(b, t, inst, -1)
    torch.cuda.synchronize()
    assert points.shape == (0, 3) and begin.tolist() == [0]
    for bad in ([5], [-1], [0, 0]):
        with pytest.raises(_lib.OmgHipError, match="inst_begin"):
            ops.CameraBatch(sc["meshes"], sc["instances"], bad, np.zeros((0, 16)), device=dev)


# ---------------------------------------------------------------------------------------------------------------------
# the cloud kernels on synthetic images: every path of k_pixel_scan, many scenes, instance values that name nothing
# ---------------------------------------------------------------------------------------------------------------------
_CLOUD_BATCH = {}


def _cloud_batch(S, H, W, pattern, dev):
    """(CameraBatch, t, inst on the device) of a synthetic case; the batch is shared by the patterns of a shape (the records of
    CC.synthetic depend on the seed, so it is keyed by the whole case)."""
    from omg_planner_amd import ops
    key = (S, H, W, pattern)
    if key not in _CLOUD_BATCH:
        sc = CC.cloud_case(*key)
        b = ops.CameraBatch(sc["meshes"], sc["instances"], sc["inst_begin"], sc["cameras"], device=dev)
        _CLOUD_BATCH[key] = (b, torch.from_numpy(np.array(sc["t"])).to(dev), torch.from_numpy(np.array(sc["inst"])).to(dev))
    return _CLOUD_BATCH[key]


@pytest.mark.parametrize("S,H,W,pattern", CC.CLOUD_CASES)
def test_clouds_of_synthetic_images_equal_the_specification(dev, S, H, W, pattern):
    """Instance images drawn on the host (CC.synthetic: values outside [0, inst_count) on both sides, INT32_MAX and INT32_MIN,
    scenes without instances, NaN depths in dropped pixels) at the smallest shapes whose scan of S * groups entries reaches the
    second wave (63, 64, 65 entries), a second pass and its carry (255, 256, 257), three and five passes (600, 1 056), a scene
    boundary inside a pass (86 scenes of 3 groups, 2 scenes of 131) and one scene across passes (257 groups): scene_begin, the
    points as int64 bits in pixel order, and a cap above and below the total between sentinels, for a class that keeps nothing
    (9), labels 0 and 1, and every hit (-1)."""
    from omg_planner_amd import ops
    b, t, inst = _cloud_batch(S, H, W, pattern, dev)
    assert b.num_scenes == S and S * -(-H * W // CC.TILE) == CC.CLOUD_SHAPES[(S, H, W)][0]
    for cls in CC.CLOUD_CLASSES:
        begin, flat = CC.cloud_spec(S, H, W, pattern, cls)
        points, got_begin = ops.pixel_clouds(b, t, inst, cls)
        torch.cuda.synchronize()
        assert got_begin.tolist() == begin.tolist(), (cls, np.flatnonzero(got_begin != begin)[:5].tolist())
        assert points.dtype == torch.float64 and points.shape == (len(flat), 3) and points.is_contiguous()
        assert np.array_equal(points.cpu().numpy().view(np.int64), flat.view(np.int64)), cls
        for cap in (len(flat) + 7, max(len(flat) - 5, 0)):
            view, buf, pad = _guarded((cap, 3), torch.float64, -7.0, dev, pad=30)
            out, got_begin = ops.pixel_clouds(b, t, inst, cls, out=view)
            torch.cuda.synchronize()
            n = min(cap, len(flat))
            assert out is view and got_begin.tolist() == begin.tolist(), (cls, cap)
            assert np.array_equal(view[:n].cpu().numpy().view(np.int64), flat[:n].view(np.int64)), (cls, cap)
            assert (view[n:] == -7.0).all() and (buf[:pad] == -7.0).all() and (buf[-pad:] == -7.0).all(), (cls, cap)


def test_cloud_entry_points_stay_inside_exact_buffers(dev):
    """omgx_pixel_count and omgx_pixel_gather called as ops.pixel_clouds calls them, on 86 scenes of 3 groups (`blocks`), with a
    workspace of exactly omgx_pixel_clouds_workspace_bytes / 4 int32 and a scene_begin of exactly S + 1, both views inside
    sentinels: the sentinels on both sides survive each call, and scene_begin and the points are the specification's."""
    import ctypes as C
    from omg_planner_amd import _lib
    from omg_planner_amd.ops import _ptr
    S, H, W, pattern = 86, 20, 30, "blocks"
    b, t, inst = _cloud_batch(S, H, W, pattern, dev)
    l = _lib.lib()
    n = int(l.omgx_pixel_clouds_workspace_bytes(S, H, W)) // 4
    assert n == 258
    for cls in (-1, 1):
        want_begin, flat = CC.cloud_spec(S, H, W, pattern, cls)
        ws, ws_buf, pad = _guarded((n,), torch.int32, -9, dev)
        begin, begin_buf, _ = _guarded((S + 1,), torch.int32, -9, dev)
        points, points_buf, _ = _guarded((len(flat), 3), torch.float64, -7.0, dev)

        def intact():
            torch.cuda.synchronize()
            return all(bool((x[:pad] == fill).all()) and bool((x[-pad:] == fill).all())
                       for x, fill in ((ws_buf, -9), (begin_buf, -9), (points_buf, -7.0)))
        assert l.omgx_pixel_count(*b._records(), H, W, _ptr(inst), cls, _ptr(ws), _ptr(begin), None) == _lib.OMGX_OK
        assert intact(), cls
        assert begin.cpu().tolist() == want_begin.tolist(), cls
        assert (ws >= 0).all() and (ws <= len(flat)).all() and (ws[1:] >= ws[:-1]).all()      # the exclusive offsets
        assert l.omgx_pixel_gather(*b._records(host=False), H, W, _ptr(t), _ptr(inst), cls, _ptr(ws), _ptr(points), len(flat), None) == _lib.OMGX_OK
        assert intact(), cls
        assert np.array_equal(points.cpu().numpy().view(np.int64), flat.view(np.int64)), cls


# ---------------------------------------------------------------------------------------------------------------------
# many scenes in one render
# ---------------------------------------------------------------------------------------------------------------------
def test_seventy_scenes_in_one_render(dev):
    """`many`: 70 scenes of 2 x 2 tiles with 0..4 instances in a cycle, a camera each, affine poses and a mirrored one: the
    images equal the specification's with and without the cull, the clouds of the device images (140 scan entries) equal the
    specification's, and scenes 3, 35 and 69 rendered alone give the bits they have in the batch."""
    from omg_planner_amd import camera as cam, ops
    sc = CC.scene("many")
    H, W, S = sc["H"], sc["W"], 70
    assert len(sc["cameras"]) == S and (H, W) == (17, 18) and np.diff(sc["inst_begin"]).tolist() == [s % 5 for s in range(S)]
    assert min(np.linalg.det(np.asarray(p)[:3, :3]) for ps in sc["poses"] for p in ps) < 0       # the mirrored instance
    b = batch_of("many", dev)
    for cull in (True, False):
        got = ops.render_depth(b, H, W, cull=cull)
        assert got[0].shape == (S, H, W) and _same(got, CC.spec("many", cull)), cull
        for s in (3, 35, 69):
            one = CC.single(sc, s)
            b1 = ops.CameraBatch(one["meshes"], one["instances"], one["inst_begin"], one["cameras"], device=dev)
            assert _same(ops.render_depth(b1, H, W, cull=cull), [a[s: s + 1] for a in CC.spec("many", cull)]), (cull, s)
    t, inst, _ = ops.render_depth(b, H, W)
    want_t, want_inst, _ = CC.spec("many")
    for cls in (0, 1, -1):
        want = cam.pixel_clouds(want_t, want_inst, CC.labels(sc), sc["inst_begin"], sc["cameras"], cls)
        flat = np.concatenate(want)
        points, begin = ops.pixel_clouds(b, t, inst, cls)
        torch.cuda.synchronize()
        assert len(flat) > 0 and begin.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist(), cls
        assert np.array_equal(points.cpu().numpy().view(np.int64), flat.view(np.int64)), cls


def partial_tiles_case():
    """One box before two cameras of 17 x 33 pixels (2 x 3 tiles, partial both ways): in view 0 it lies over the corner where four
    tiles meet, in view 1 over the image's last row and last column -> (scene dict, the specification's images)."""
    from omg_planner_amd import camera as cam
    H, W = 17, 33
    intr = [(30.0, 28.0, 16.0, 8.0), (26.0, 30.0, 14.5, 9.25)]
    views = [(intr[0], CC.EYE, [(0, MC.pose((0.2, 0.1, -0.3), CC.at_pixel(intr[0], H, W, 16.0 / H, 16.0 / W, 0.3)), 0)]),
             (intr[1], CC.EYE, [(0, MC.pose((-0.1, 0.3, 0.2), CC.at_pixel(intr[1], H, W, 15.0 / H, 30.0 / W, 0.25)), 1)])]
    sc = CC.build([CC.BOX], views, H, W)
    want = cam.render_depth(sc["meshes"], sc["instances"], sc["inst_begin"], sc["cameras"], H, W)
    hit = want[1] >= 0
    assert all(hit[0, r, c] for r in (15, 16) for c in (15, 16)) and hit[1, 16].any() and hit[1, :, 32].any()  # across the tiles' borders
    assert all(h.any() and not h.all() for h in hit) and not hit[1, 16].all() and not hit[1, :, 32].all()
    return sc, want


def test_partial_tiles_of_two_views_equal_the_specification(dev):
    """The smallest launch in which a wrong tile map or a wrong clamp of the lanes outside the image shows: 17 x 33 pixels and two
    views of one box.  Depth as bits, instance and face equal camera.render_depth with and without the cull, and the cloud of
    pixel_clouds on the same images equals camera.pixel_clouds as bits."""
    from omg_planner_amd import camera as cam, ops
    sc, want = partial_tiles_case()
    b = ops.CameraBatch(sc["meshes"], sc["instances"], sc["inst_begin"], sc["cameras"], device=dev)
    for cull in (True, False):
        got = ops.render_depth(b, sc["H"], sc["W"], cull=cull)
        assert got[0].shape == (2, 17, 33) and _same(got, want), cull
    for cls in (-1, 1):
        spec = cam.pixel_clouds(want[0], want[1], CC.labels(sc), sc["inst_begin"], sc["cameras"], cls)
        points, begin = ops.pixel_clouds(b, got[0], got[1], cls)
        torch.cuda.synchronize()
        assert len(spec[1]) > 0 and begin.tolist() == [0, len(spec[0]), len(spec[0]) + len(spec[1])], cls
        assert np.array_equal(points.cpu().numpy().view(np.int64), np.concatenate(spec).view(np.int64)), cls
