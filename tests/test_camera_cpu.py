"""CPU tests of the depth camera (omg-planner_amd/camera.py, csrc/omg_camera.hip): the specification against
known answers, the tie rule, the world-frame clouds and their order, the neutrality of the cull on every scene the camera tests
use, csrc/omg_camera_body.h compiled for the host against the specification bit for bit, every argument error of the C ABI and
of the wrappers, and the kernels' register budget."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import camera_cases as CC
from tests import kernel_build as KB
from tests import mesh_cases as MC


@pytest.fixture(scope="module")
def cam():
    from omg_planner_amd import camera
    return camera


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pose", [("box_axis", MC.pose(t=(0.0, 0.0, 0.5))), ("box_posed", CC.BOX_POSED)])
def test_box_in_front_of_the_camera(name, pose):
    t, inst, face = (a[0] for a in CC.spec(name))
    assert t.dtype == np.float64 and inst.dtype == np.int32 and face.dtype == np.int32 and t.shape == (40, 32)
    want_t, quad = CC.box_slab(pose, CC.EYE, CC.INTR, 40, 32)
    hit = np.isfinite(want_t)
    assert 100 < hit.sum() < 40 * 32 - 100
    assert np.array_equal(np.isfinite(t), hit) and np.array_equal(inst, np.where(hit, 0, -1))
    assert np.abs(t[hit] - want_t[hit]).max() <= 1e-12
    assert ((face[hit] == 2 * quad[hit]) | (face[hit] == 2 * quad[hit] + 1)).all() and (face[~hit] == -1).all()
    if name == "box_axis":
        assert np.abs(t[hit] - 0.47).max() <= 1e-12 and set(np.unique(face[hit])) == {8, 9}   # the slab distance to the face z = -0.03
    else:
        assert len(np.unique(quad[hit])) >= 2                                                  # more than one side is seen


@pytest.mark.parametrize("name", ["box_behind", "box_offscreen"])
def test_nothing_to_see(name):
    for cull in (True, False):
        t, inst, face = CC.spec(name, cull)
        assert np.isposinf(t).all() and (inst == -1).all() and (face == -1).all()


def test_camera_inside_a_sphere(cam):
    sc = CC.scene("inside_sphere")
    assert sc["instances"]["q"][0] <= 0.0                        # the branch q <= 0: the ball contains the camera
    t, inst, face = CC.spec("inside_sphere")
    assert np.isfinite(t).all() and (t > 0).all() and (inst == 0).all() and (face >= 0).all()
    dx, dy = cam.pixel_directions(sc["cameras"][0], sc["H"], sc["W"])
    p = np.stack([t[0].ravel() * dx, t[0].ravel() * dy, t[0].ravel()], -1) - np.array([0.0, 0.0, 0.01])
    rad = np.sqrt((p * p).sum(1))
    assert rad.max() <= 0.06 + 1e-12 and rad.min() >= 0.06 * 0.97   # on the faces of the inscribed polyhedron


def test_the_nearer_instance_wins_and_index_zero_wins_a_tie():
    t, inst, _ = (a[0] for a in CC.spec("overlap"))
    far = CC.box_slab(MC.pose(t=(0.0, 0.0, 0.6)), CC.EYE, CC.INTR, 40, 32)[0]
    near = CC.box_slab(MC.pose(t=(0.04, 0.05, 0.45)), CC.EYE, CC.INTR, 40, 32)[0]
    both = np.isfinite(far) & np.isfinite(near)
    assert both.sum() > 50 and (np.isfinite(far) & ~np.isfinite(near)).sum() > 50
    assert (inst[both] == 1).all() and np.abs(t[both] - near[both]).max() <= 1e-12     # instance 1 is the nearer one
    assert (inst[np.isfinite(far) & ~np.isfinite(near)] == 0).all()
    t2, inst2, face2 = (a[0] for a in CC.spec("duplicate"))
    t1, inst1, face1 = (a[0] for a in CC.spec("box_posed"))
    assert np.array_equal(_bits(t2), _bits(t1)) and np.array_equal(inst2, inst1) and np.array_equal(face2, face1) and inst2.max() == 0


def test_one_mesh_at_two_poses():
    sc = CC.scene("shared_mesh")
    assert len(sc["meshes"]) == 1 and (sc["instances"]["mesh"] == 0).all()
    t, inst, _ = (a[0] for a in CC.spec("shared_mesh"))
    for i in (0, 1):
        want = CC.box_slab(sc["poses"][0][i], CC.EYE, CC.INTR, 40, 32)[0]
        mine = inst == i
        assert mine.sum() > 50 and np.abs(t[mine] - want[mine]).max() <= 1e-12
    assert np.array_equal(inst >= 0, np.isfinite(t))


def test_world_points_of_a_posed_camera_and_cloud_order(cam):
    sc = CC.scene("posed_camera")
    t, inst, _ = CC.spec("posed_camera")
    lab = CC.labels(sc)
    world_from_cam = np.linalg.inv(CC.CAM_POSED)
    for cls in (-1, 0, 1, 5):
        cloud = cam.pixel_clouds(t, inst, lab, sc["inst_begin"], sc["cameras"], cls)[0]
        keep = (inst[0] >= 0) if cls < 0 else (inst[0] >= 0) & (lab[np.maximum(inst[0], 0)] == cls)
        rr, cc = np.nonzero(keep)                                                          # row-major: the cloud's order
        assert cloud.shape == (len(rr), 3) and cloud.dtype == np.float64
        tt = t[0][rr, cc]
        p_cam = np.stack([tt * (cc - CC.INTR[2]) / CC.INTR[0], tt * (rr - CC.INTR[3]) / CC.INTR[1], tt, np.ones_like(tt)], -1)
        want = (p_cam @ world_from_cam.T)[:, :3]
        assert len(rr) == 0 or np.abs(cloud - want).max() <= 1e-12
        assert (len(rr) == 0) == (cls == 5)
    # the box seen by the posed camera is the box seen from the origin: the same depths to rounding
    t0 = CC.spec("box_posed")[0][0]
    mine = inst[0] == 0
    assert mine.sum() > 100 and np.abs(t[0][mine] - t0[mine]).max() <= 1e-12
    # draw: the reference's np.random.choice with replacement
    cloud = cam.pixel_clouds(t, inst, lab, sc["inst_begin"], sc["cameras"], -1)[0]
    got = cam.draw(cloud, 50, np.random.RandomState(3))
    assert np.array_equal(got, cloud[np.random.RandomState(3).choice(len(cloud), 50)])


def test_scene_records_from_scenes(cam):
    from omg_planner_amd import scenes as S
    grid = S.SdfGrid(np.ones((2, 2, 2), np.float32), np.zeros(3), 0.1)
    box = CC.BOX
    sc = [S.Scene([S.SceneObject("table", np.eye(4), grid), S.SceneObject("a", MC.pose(t=(0.0, 0.0, 0.5)), grid),
                   S.SceneObject("b", MC.pose(t=(0.1, 0.0, 0.6)), grid)], target_idx=2),
          S.Scene([S.SceneObject("a", MC.pose(t=(0.0, 0.0, 0.5)), grid)], target_idx=0)]
    pool, inst, begin, cams = cam.scene_records(sc, [[None, box, box], [box]], np.eye(4), CC.INTR)
    assert len(pool) == 1 and begin.tolist() == [0, 2, 3] and inst["label"].tolist() == [1, 0, 0] and cams.shape == (2, 16)
    one = CC.scene("box_axis")
    assert np.array_equal(inst[2:].tobytes(), one["instances"].tobytes()) and np.array_equal(cams[1], one["cameras"][0])
    with pytest.raises(ValueError):
        cam.scene_records(sc, [[None, box], [box]], np.eye(4), CC.INTR)


# ---------------------------------------------------------------------------------------------------------------------
# the cull changes nothing
# ---------------------------------------------------------------------------------------------------------------------
def test_cull_is_neutral_on_every_scene_of_the_camera_tests(cam):
    """render_depth(cull=True) equals cull=False as bits on every scene of tests/camera_cases.py (all of them, the twelve random
    ones included), and the scenes exercise both sides of the cull: an instance that no pixel of some 16 x 16 tile can hit, and one
    that only part of a tile can."""
    skipped_tile = partial_tile = 0
    removed = []
    for name in CC.SCENES:
        a, b = CC.spec(name, True), CC.spec(name, False)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), name
        sc = CC.scene(name)
        H, W = sc["H"], sc["W"]
        for s in range(len(sc["cameras"])):
            dx, dy = cam.pixel_directions(sc["cameras"][s], H, W)
            for rec in sc["instances"][sc["inst_begin"][s]: sc["inst_begin"][s + 1]]:
                act = cam.instance_active(rec, dx, dy).reshape(H, W)
                if name in CC.RANDOM:
                    removed.append(1.0 - act.mean())
                for r0 in range(0, H, 16):
                    for c0 in range(0, W, 16):
                        tile = act[r0: r0 + 16, c0: c0 + 16]
                        skipped_tile += not tile.any()
                        partial_tile += tile.any() and not tile.all()
    assert skipped_tile > 0 and partial_tile > 0
    assert np.mean(removed) > 0.8                                   # most (pixel, instance) tests of the random scenes are culled


def test_random_scenes_have_hits_background_and_both_labels():
    for name in CC.RANDOM:
        sc = CC.scene(name)
        inst = CC.spec(name)[1][0]
        seen = CC.labels(sc)[inst[inst >= 0]]
        assert (inst >= 0).any() and (inst < 0).any() and (seen == 0).any() and (seen == 1).any(), name


def test_many_scenes_keep_their_promises():
    """`many` (70 scenes, 0..4 instances in a cycle): a scene without instances is all background, some scene shows both labels,
    most scenes show something, and the cull changes no bit."""
    sc = CC.scene("many")
    t, inst, face = CC.spec("many")
    counts = np.diff(sc["inst_begin"])
    assert len(counts) == 70 and counts.tolist() == [s % 5 for s in range(70)] and t.shape == (70, 17, 18)
    assert {int(m) for m in sc["instances"]["mesh"]} == {0, 1} and len(sc["meshes"]) == 2
    both = shown = 0
    for s in range(70):
        if counts[s] == 0:
            assert np.isposinf(t[s]).all() and (inst[s] == -1).all() and (face[s] == -1).all(), s
            continue
        assert inst[s].max() < counts[s]
        seen = CC.labels(sc)[sc["inst_begin"][s] + inst[s][inst[s] >= 0]]
        shown += len(seen) > 0 and (inst[s] < 0).any()
        both += (seen == 0).any() and (seen == 1).any()
    assert both >= 1 and shown >= 28                               # at least half of the 56 scenes with instances: hits and background
    a, b = CC.spec("many", True), CC.spec("many", False)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic images of the cloud tests
# ---------------------------------------------------------------------------------------------------------------------
def test_synthetic_cloud_cases_keep_their_promises(cam):
    """Every (shape, pattern) test_gpu_camera.py runs, by the specification alone: the scan has the tabled number of entries; the
    classes 0, 1 and -1 keep something (`full` names label 0 only) and class 9 nothing; with more than one scene one keeps nothing and one something; `blocks`
    and `full` have a group with every pixel kept (256 of them wherever the image has as many) and, with more than one scene, a
    group with none; `edges` keeps exactly the listed lanes and the last pixel; `random` names instances past the scene's count
    and below -1; a NaN depth lies in no kept pixel."""
    assert sorted({n for n, _ in CC.CLOUD_SHAPES.values()}) == [63, 64, 65, 255, 256, 257, 258, 262, 600, 1056]
    assert all(p[0] == "random" and len(p) >= 2 for _, p in CC.CLOUD_SHAPES.values()) and len(CC.CLOUD_CASES) == 28
    for S, H, W, pattern in CC.CLOUD_CASES:
        case = (S, H, W, pattern)
        sc = CC.cloud_case(*case)
        HW, groups = H * W, -(-H * W // CC.TILE)
        assert S * groups == CC.CLOUD_SHAPES[(S, H, W)][0], case
        counts = np.diff(sc["inst_begin"])
        assert counts.tolist() == [CC.synthetic_count(s) for s in range(S)] and sc["t"].shape == sc["inst"].shape == (S, H, W)
        assert all(CC.labels(sc)[sc["inst_begin"][s]: sc["inst_begin"][s + 1]].tolist() == [0, 1, 2][: counts[s]] for s in range(S))
        totals = {cls: int(CC.cloud_spec(*case, cls)[0][-1]) for cls in CC.CLOUD_CLASSES}
        if pattern == "full":                                    # instance 0 everywhere, whose label is 0: class 1 keeps nothing
            assert totals[9] == 0 == totals[1] and 0 < totals[0] == totals[-1], (case, totals)
        else:
            assert totals[9] == 0 and 0 < totals[0] < totals[-1] and 0 < totals[1] < totals[-1], (case, totals)
        begin, flat = CC.cloud_spec(*case, -1)
        per_scene = np.diff(begin)
        assert np.isfinite(flat).all() and (np.isnan(sc["t"]).any() or totals[-1] == S * H * W), case   # NaN among the dropped pixels
        if S > 1:
            assert (per_scene == 0).any() and (per_scene > 0).any() and (per_scene[counts == 0] == 0).all(), case
        inst = sc["inst"].reshape(S, HW)
        kept = np.stack([cam.pixel_mask(inst[s], np.zeros(counts[s]), -1) for s in range(S)])
        assert kept.sum() == totals[-1] and np.isfinite(sc["t"].reshape(S, HW)[kept]).all() and not np.isfinite(sc["t"].reshape(S, HW)[~kept]).any()
        padded = np.zeros((S, groups * CC.TILE), bool)
        padded[:, :HW] = kept
        in_group = padded.reshape(S, groups, CC.TILE).sum(-1)
        size = np.minimum(CC.TILE, HW - CC.TILE * np.arange(groups))          # pixels of each group: the last may be partial
        if pattern in ("blocks", "full"):
            assert (in_group == size).any() and (HW < CC.TILE or (in_group == CC.TILE).any()), case
            assert S == 1 or (in_group == 0).any(), case
        if pattern == "blocks" and groups >= 3:
            assert (in_group == 0).any() and ((in_group > 0) & (in_group < size)).any(), case
        if pattern == "edges":
            p = np.arange(HW)
            listed = np.isin(p % CC.TILE, CC.EDGE_LANES) | (p == HW - 1)
            assert all(np.array_equal(kept[s], listed if counts[s] else np.zeros(HW, bool)) for s in range(S)), case
        if pattern == "random":
            assert (inst >= counts[:, None]).any() and (inst <= -2).any() and (inst == -1).any(), case
            assert (inst == np.iinfo(np.int32).max).any() and (inst == np.iinfo(np.int32).min).any(), case


# ---------------------------------------------------------------------------------------------------------------------
# the kernel bodies compiled for the host
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include "omg_camera_body.h"
struct rec { double m[12]; double centre[3]; double q; int32_t mesh, label; };
extern "C" void host_render(const double* verts, const int32_t* faces, const int32_t* vert_begin, const int32_t* face_begin,
                            const int32_t* face_count, const rec* inst, int n_inst, const double* camera, int H, int W, int cull,
                            double t_min, double tol, double* t_out, int32_t* i_out, int32_t* f_out) {
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            double dx, dy;
            image_pixel_dir(r, c, camera[0], camera[1], camera[2], camera[3], dx, dy);
            double best = __builtin_inf();
            int32_t bi = -1, bf = -1;
            for (int i = 0; i < n_inst; ++i) {
                if (cull && !camera_instance_active(inst[i].centre, inst[i].q, dx, dy)) continue;
                double o[3], d[3];
                camera_object_ray(inst[i].m, dx, dy, o, d);
                const double* mv = verts + (long)vert_begin[inst[i].mesh] * 3;
                const int32_t* mf = faces + (long)face_begin[inst[i].mesh] * 3;
                double b = best;   // seeded with the running best, as the kernel does
                int32_t f = -1;
                for (int q = 0; q < face_count[inst[i].mesh]; ++q) {
                    double T[9];
                    for (int k = 0; k < 3; ++k)
                        for (int a = 0; a < 3; ++a) T[k * 3 + a] = mv[mf[q * 3 + k] * 3 + a];
                    mesh_raycast_pair(o[0], o[1], o[2], d[0], d[1], d[2], T, q, t_min, -tol, 1.0 + tol, b, f);
                }
                if (b < best) best = b, bi = i, bf = f;
            }
            t_out[r * W + c] = best, i_out[r * W + c] = bi, f_out[r * W + c] = bf;
        }
}
extern "C" int host_cloud(const rec* inst, int n_inst, const double* camera, int H, int W, const double* t, const int32_t* img,
                          int cls, double* points) {
    int n = 0;
    for (int p = 0; p < H * W; ++p) {
        const int32_t i = img[p];
        const int32_t label = (i >= 0 && i < n_inst) ? inst[i].label : -1;
        if (!camera_pixel_kept(i, n_inst, label, cls)) continue;
        double dx, dy;
        image_pixel_dir(p / W, p % W, camera[0], camera[1], camera[2], camera[3], dx, dy);
        camera_world_point(camera + 4, t[p], dx, dy, points + 3 * n++);
    }
    return n;
}
"""


@KB.requires_host_cxx
def test_kernel_bodies_compiled_for_the_host_equal_the_specification(cam, tmp_path):
    """csrc/omg_camera_body.h is what the kernels do per pixel and per (pixel, instance) pair; compiled for the host without
    contraction, and with the per-mesh loop seeded by the running best as in k_render_depth, it gives the specification's t as
    int64 bits, its instance and its face on every pixel of the known-answer scenes, two device scenes and three random ones,
    with and without the cull, and the world-frame clouds as bits."""
    lib = KB.host_harness(_HOST_HARNESS, tmp_path)
    vp, dbl, i = C.c_void_p, C.c_double, C.c_int
    lib.host_render.argtypes = [vp] * 6 + [i, vp, i, i, i, dbl, dbl, vp, vp, vp]
    lib.host_cloud.argtypes = [vp, i, vp, i, i, vp, vp, i, vp]
    pixels = 0
    for name in ("box_axis", "box_posed", "box_behind", "inside_sphere", "overlap", "duplicate", "shared_mesh", "posed_camera", "17x33", "multi",
                 "random0", "random5", "random11"):
        sc = CC.scene(name)
        H, W = sc["H"], sc["W"]
        verts = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64) for v, _ in sc["meshes"]]))
        faces = np.ascontiguousarray(np.concatenate([np.asarray(f, np.int32) for _, f in sc["meshes"]]))
        vb = np.cumsum([0] + [len(v) for v, _ in sc["meshes"]]).astype(np.int32)
        fb = np.cumsum([0] + [len(f) for _, f in sc["meshes"]]).astype(np.int32)
        fc = np.array([len(f) for _, f in sc["meshes"]], np.int32)
        for s in range(len(sc["cameras"])):
            inst = np.ascontiguousarray(sc["instances"][sc["inst_begin"][s]: sc["inst_begin"][s + 1]])
            camera = np.ascontiguousarray(sc["cameras"][s])
            for cull in (1, 0):
                want = [a[s] for a in CC.spec(name, bool(cull))]
                t, ii, ff = np.zeros((H, W)), np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
                lib.host_render(verts.ctypes.data, faces.ctypes.data, vb.ctypes.data, fb.ctypes.data, fc.ctypes.data, inst.ctypes.data, len(inst),
                                camera.ctypes.data, H, W, cull, 1e-6, 1e-9, t.ctypes.data, ii.ctypes.data, ff.ctypes.data)
                assert np.array_equal(_bits(t), _bits(want[0])) and np.array_equal(ii, want[1]) and np.array_equal(ff, want[2]), (name, s, cull)
            pixels += H * W
            for cls in (-1, 0, 1, 9):
                one = CC.single(sc, s)
                cloud = cam.pixel_clouds(want[0][None], want[1][None], inst["label"], one["inst_begin"], one["cameras"], cls)[0]
                pts = np.full((H * W, 3), 7.0)
                timg, iimg = np.ascontiguousarray(want[0]), np.ascontiguousarray(want[1])
                n = lib.host_cloud(inst.ctypes.data, len(inst), camera.ctypes.data, H, W, timg.ctypes.data, iimg.ctypes.data, cls, pts.ctypes.data)
                assert n == len(cloud) and np.array_equal(_bits(pts[:n]), _bits(cloud)), (name, s, cls)
    assert pixels >= 10000


# ---------------------------------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _records(I=3, S=2):
    from omg_planner_amd import _lib
    inst, cams = (_lib.Instance * I)(), (_lib.Camera * S)()
    for k in range(I):
        inst[k].m[:] = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, -0.5]
        inst[k].centre[:], inst[k].q, inst[k].mesh, inst[k].label = [0.0, 0.0, 0.5], 0.24, k % 2, k
    for s in range(S):
        cams[s].fx, cams[s].fy, cams[s].cx, cams[s].cy = 100.0, 100.0, 8.0, 8.0
        cams[s].world_from_cam[:] = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
        cams[s].inst_begin, cams[s].inst_count = (0, 1) if s == 0 else (1, I - 1)
    return inst, cams


def _meshes(M=2, **over):
    from omg_planner_amd import _lib
    rec = (_lib.Mesh * M)()
    for m in range(M):
        r = rec[m]
        r.delta, r.sample_offset, r.dims[:] = 1.0, 0.5, [1, 1, 1]
        r.vert_begin, r.vert_count, r.face_begin, r.face_count = 8 * m, 8, 12 * m, 12
    for k, val in over.items():
        setattr(rec[M - 1], k, val)
    return rec


def test_c_abi_argument_checks_without_gpu():
    """Every OMGX_ERR_INVALID / OMGX_ERR_UNSUPPORTED case of the four entry points is decided on the host copies before any HIP
    call."""
    from omg_planner_amd import _lib
    from omg_planner_amd import camera as cam
    lib = _lib.lib()
    assert C.sizeof(_lib.Camera) == 136 == cam.CAMERA_DTYPE.itemsize and C.sizeof(_lib.Instance) == 136 == cam.INSTANCE_DTYPE.itemsize
    for struct, dtype in ((_lib.Camera, cam.CAMERA_DTYPE), (_lib.Instance, cam.INSTANCE_DTYPE)):
        assert [(n, getattr(struct, n).offset) for n, _ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]
    assert _lib.CAMERA_PIXELS_PER_WORKGROUP == 256 == lib.omgx_mesh_sdf_tile() == CC.TILE and lib.omgx_abi_version() == 14
    INV, UNS, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED, _lib.OMGX_OK
    assert lib.omgx_pixel_clouds_workspace_bytes(3, 17, 33) == 3 * 3 * 4 and lib.omgx_pixel_clouds_workspace_bytes(0, 4, 4) == 0
    assert lib.omgx_pixel_clouds_workspace_bytes(2, 16, 16) == 2 * 4 and lib.omgx_pixel_clouds_workspace_bytes(1, 1, 257) == 2 * 4
    assert lib.omgx_pixel_clouds_workspace_bytes(-1, 4, 4) == INV and lib.omgx_pixel_clouds_workspace_bytes(1, 0, 4) == INV
    assert lib.omgx_pixel_clouds_workspace_bytes(1, 4, 0) == INV
    d = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    vpc = lambda x: C.cast(x, C.c_void_p)

    def render(inst=None, cams=None, mesh=None, M=2, I=3, S=2, H=16, W=16, t_min=1e-6, tol=1e-9, host=(True, True, True), **ptr):
        i0, c0 = _records()
        inst, cams, mesh = inst or i0, cams or c0, mesh or _meshes(max(M, 1))
        p = dict(verts=d, faces=d, meshes=d, instances=d, cameras=d, t=d, img=d, face=d)
        p.update(ptr)
        return lib.omgx_render_depth(p["verts"], p["faces"], p["meshes"], vpc(mesh) if host[0] else None, M, p["instances"],
                                     vpc(inst) if host[1] else None, I, p["cameras"], vpc(cams) if host[2] else None, S, H, W, 1, t_min, tol,
                                     p["t"], p["img"], p["face"], None)

    def count(inst=None, cams=None, I=3, S=2, H=16, W=16, host=(True, True), **ptr):
        i0, c0 = _records()
        inst, cams = inst or i0, cams or c0
        p = dict(instances=d, cameras=d, img=d, ws=d, begin=d)
        p.update(ptr)
        return lib.omgx_pixel_count(p["instances"], vpc(inst) if host[0] else None, I, p["cameras"], vpc(cams) if host[1] else None, S, H, W,
                                    p["img"], 0, p["ws"], p["begin"], None)

    def gather(I=3, S=2, H=16, W=16, cap=10, **ptr):
        p = dict(instances=d, cameras=d, t=d, img=d, ws=d, points=d)
        p.update(ptr)
        return lib.omgx_pixel_gather(p["instances"], I, p["cameras"], S, H, W, p["t"], p["img"], 0, p["ws"], p["points"], cap, None)

    for k in ("verts", "faces", "meshes", "instances", "cameras", "t", "img"):
        assert render(**{k: None}) == INV, k
    for k in range(3):
        assert render(host=tuple(j != k for j in range(3))) == INV, k
    for k in ("instances", "cameras", "img", "ws", "begin"):
        assert count(**{k: None}) == INV, k
    assert count(host=(False, True)) == INV and count(host=(True, False)) == INV
    for k in ("instances", "cameras", "t", "img", "ws", "points"):
        assert gather(**{k: None}) == INV, k
    assert gather(cap=-1) == INV and gather(I=-1) == INV and gather(S=-1) == INV
    assert render(M=0) == INV and render(M=-1) == INV and render(I=-1) == INV and render(S=-1) == INV and count(I=-1) == INV and count(S=-1) == INV
    for fn in (render, count, gather):
        assert fn(H=0) == INV and fn(W=0) == INV and fn(H=-3) == INV, fn
    for bad in (-1e-6, float("nan"), float("inf")):
        assert render(t_min=bad) == INV and render(tol=bad) == INV
    for k in ("face_count", "vert_count"):
        assert render(mesh=_meshes(**{k: 0})) == INV, k
    assert render(mesh=_meshes(vert_begin=-1)) == INV and render(mesh=_meshes(face_begin=-1)) == INV
    nan, inf = float("nan"), float("inf")
    for fn in (render, count):
        for field in ("fx", "fy"):
            for bad in (0.0, nan, inf, -inf):
                inst, cams = _records()
                setattr(cams[1], field, bad)
                assert fn(cams=cams) == INV, (field, bad)
        for field in ("cx", "cy"):
            for bad in (nan, inf):
                inst, cams = _records()
                setattr(cams[0], field, bad)
                assert fn(cams=cams) == INV, (field, bad)
        for k in (0, 11):
            inst, cams = _records()
            cams[1].world_from_cam[k] = nan
            assert fn(cams=cams) == INV
            inst, cams = _records()
            inst[2].m[k] = inf
            assert fn(inst=inst) == INV
        for k in range(3):
            inst, cams = _records()
            inst[1].centre[k] = nan
            assert fn(inst=inst) == INV
        inst, cams = _records()
        inst[0].q = -inf
        assert fn(inst=inst) == INV
        inst, cams = _records()
        inst[2].label = -1
        assert fn(inst=inst) == INV
        for begin, cnt in ((-1, 1), (0, -1), (2, 2), (3, 1), (0, 4)):
            inst, cams = _records()
            cams[1].inst_begin, cams[1].inst_count = begin, cnt
            assert fn(cams=cams) == INV, (begin, cnt)
    for bad in (-1, 2, 7):
        inst, cams = _records()
        inst[1].mesh = bad
        assert render(inst=inst) == INV, bad
    inst, cams = _records()
    inst[1].mesh = 1                                                     # legal with two meshes, outside a pool of one
    assert render(inst=inst, M=1) == INV
    # limits: the tile index is gridDim.x, the cloud's offsets are int32
    one = _records(S=1)
    one[1][0].inst_begin, one[1][0].inst_count = 0, 3
    for fn in (render, count):
        assert fn(inst=one[0], cams=one[1], S=1, H=16 * 4096, W=16 * 2048 + 1) == UNS
        assert fn(inst=one[0], cams=one[1], S=1, H=46341, W=46341) == UNS
    assert gather(S=1, H=46341, W=46341) == UNS and gather(S=65536, H=1, W=1) == UNS
    assert render(inst=one[0], cams=one[1], S=1, H=1, W=16 * (1 << 23) + 1) == UNS       # too many tiles, though few pixels
    # nothing to do: no scene (instances, cameras and images may then be NULL); no row to write
    assert render(S=0, cameras=None, t=None, img=None, face=None, host=(True, True, False)) == OK
    assert render(S=0, I=0, instances=None, cameras=None, t=None, img=None, host=(True, False, False)) == OK
    assert gather(S=0, cameras=None, t=None, img=None, ws=None, points=None, cap=0) == OK and gather(cap=0, points=None) == OK


def test_wrapper_checks_without_gpu(cam):
    import torch
    from omg_planner_amd import _lib, ops
    E = _lib.OmgHipError
    sc = CC.scene("shared_mesh")
    args = lambda **kw: [kw.get(k, sc[k]) for k in ("meshes", "instances", "inst_begin", "cameras")]
    b = ops.CameraBatch(*args(), device="cpu")
    assert (b.num_meshes, b.num_instances, b.num_scenes) == (1, 2, 1) and b.h_cameras["inst_count"].tolist() == [2]
    assert b.d_instances.numel() == 2 * 136 and b.d_cameras.numel() == 136 and b.faces.dtype == torch.int32
    v, f = CC.BOX
    bad = f.copy()
    bad[3, 1] = 8
    with pytest.raises(E, match="indices"):
        ops.CameraBatch(*args(meshes=[(v, bad)]), device="cpu")
    with pytest.raises(E, match="zero area"):   # dropping them would renumber the faces the face image names
        ops.CameraBatch(*args(meshes=[(v, np.concatenate([f[:3], [[0, 0, 1]], f[3:]]))]), device="cpu")
    with pytest.raises(E):
        ops.CameraBatch(*args(meshes=[]), device="cpu")
    with pytest.raises(E, match="INSTANCE_DTYPE"):
        ops.CameraBatch(*args(instances=np.zeros((2, 17))), device="cpu")
    with pytest.raises(E, match="cameras"):
        ops.CameraBatch(*args(cameras=np.zeros((1, 12))), device="cpu")
    for begin in ([0], [0, 3], [1, 0], [-1, 2], [0, 1, 2]):
        with pytest.raises(E, match="inst_begin"):
            ops.CameraBatch(*args(inst_begin=begin), device="cpu")
    for begin in ([5], [-1], [0, 0]):                                       # no scene at all: inst_begin is still checked
        with pytest.raises(E, match="inst_begin"):
            ops.CameraBatch(*args(inst_begin=begin, cameras=np.zeros((0, 16))), device="cpu")
    assert ops.CameraBatch(*args(inst_begin=[0], cameras=np.zeros((0, 16))), device="cpu").num_scenes == 0
    for col, val in ((0, 0.0), (1, np.nan), (3, np.inf), (9, np.nan)):
        c = sc["cameras"].copy()
        c[0, col] = val
        with pytest.raises(E, match="camera"):
            ops.CameraBatch(*args(cameras=c), device="cpu")
    for field, val in (("m", np.nan), ("centre", np.inf), ("q", np.nan), ("label", -1), ("mesh", 1), ("mesh", -1)):
        i = sc["instances"].copy()
        i[field][1] = val
        with pytest.raises(E):
            ops.CameraBatch(*args(instances=i), device="cpu")
    with pytest.raises(E, match="H and W"):
        ops.render_depth(b, 0, 4)
    with pytest.raises(E, match="finite"):
        ops.render_depth(b, 4, 4, tol=-1.0)
    with pytest.raises(E, match="device tensor"):
        ops.render_depth(b, 4, 4, out=(torch.zeros((1, 4, 4), dtype=torch.float64), torch.zeros((1, 4, 4), dtype=torch.int32), None))
    with pytest.raises(E, match="device tensor"):
        ops.pixel_clouds(b, torch.zeros((1, 4, 4), dtype=torch.float64), torch.zeros((1, 4, 4), dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="label"):
        cam.instance_records([CC.BOX], [0], [np.eye(4)], [-1], np.eye(4))
    with pytest.raises(ValueError, match="mesh"):
        cam.instance_records([CC.BOX], [1], [np.eye(4)], [0], np.eye(4))
    with pytest.raises(ValueError):
        cam.render_depth(sc["meshes"], sc["instances"], [0, 3], sc["cameras"], 4, 4)


# ---------------------------------------------------------------------------------------------------------------------
# registers
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_camera_kernels_do_not_spill(tmp_path):
    """The compiler's resource remarks for csrc/omg_camera.hip: no kernel uses scratch, and k_render_depth keeps a pixel's state
    and a face's nine coordinates in few enough registers for at least four waves per SIMD."""
    seen = KB.kernel_resources("omg_camera.hip", tmp_path)
    kernels = {k: KB.one(seen, k) for k in ("k_render_depth", "k_pixel_count", "k_pixel_scan", "k_pixel_gather")}
    for k, v in kernels.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    assert kernels["k_render_depth"]["Occupancy [waves/SIMD]"] >= 4 and kernels["k_render_depth"]["VGPRs"] <= 128, kernels
