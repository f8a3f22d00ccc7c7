"""CPU tests of the robot self-filter (omg-planner_amd/robot_filter.py, csrc/omg_robot_filter.hip): the
specification at its edges as answers worked out by hand; csrc/omg_robot_filter_body.h compiled for the host equals the
specification bit for bit, with and without both culls; the path in numpy on fusion_cases' scene with an arm in front of it; every
argument error of the specification, of the C ABI and of the wrappers; the kernels use no scratch."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import kernel_build as KB
from tests import robot_filter_cases as RC

INF, NAN = RC.INF, RC.NAN


def _identity_cameras(V=1):
    return RC.camera_records(np.tile(np.eye(4), (V, 1, 1)), RC.IDENTITY_CAMERA)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the specification at its edges
# ---------------------------------------------------------------------------------------------------------------------
def test_render_edge_cases_as_known_answers():
    """One camera at the origin looking along +z, fx = fy = 1, cx = cy = 0: pixel (0, 0) is the ray (0, 0, 1); t_min = 0.25."""
    from omg_planner_amd import robot_filter as rf
    cam = _identity_cameras()
    for what, spheres, t, n in RC.RENDER_CASES:
        t_near, which = rf.render_spheres(np.array([spheres]), cam, 1, 1, RC.RENDER_T_MIN)
        assert t_near.shape == (1, 1, 1) and t_near.dtype == np.float64 and which.dtype == np.int32
        assert (t_near[0, 0, 0], which[0, 0, 0]) == (t, n), what
    # radius 0 with pad > 0: camera_spheres adds the pad, and an identity pose and camera leave the centre as it is
    what, spheres, pad, t, n = RC.RENDER_PAD_CASE
    local = np.array(spheres)
    cs = rf.camera_spheres(np.tile(np.eye(4), (1, 10, 1, 1)), local, [3], cam, [0], pad)
    assert cs.tolist() == [[[0.0, 0.0, 2.0, 0.5]]]
    t_near, which = rf.render_spheres(cs, cam, 1, 1, RC.RENDER_T_MIN)
    assert (t_near[0, 0, 0], which[0, 0, 0]) == (t, n), what
    # N = 0: all misses, and an array of no spheres
    cs = rf.camera_spheres(np.tile(np.eye(4), (1, 10, 1, 1)), np.zeros((0, 4)), [], cam, [0], 0.0)
    t_near, which = rf.render_spheres(cs, cam, 2, 3)
    assert cs.shape == (1, 0, 4) and np.isposinf(t_near).all() and (which == -1).all() and t_near.shape == (1, 2, 3)
    # the cases as one launch (what the device gets): the same answers at pixel (0, 0) of every view
    e = RC.render_edge_launch()
    cs = rf.camera_spheres(e["link_poses"], e["local"], e["link"], e["cameras"], e["config_of_view"], 0.0)
    t_near, which = rf.render_spheres(cs, e["cameras"], e["H"], e["W"], RC.RENDER_T_MIN)
    for k, (what, _, t, n) in enumerate(RC.RENDER_CASES):
        assert (t_near[k, 0, 0], which[k, 0, 0]) == (t, -1 if n < 0 else e["first"][k] + n), what


def test_camera_spheres_of_two_views_with_different_configurations():
    """A sphere at (1, 2, 3) of link 4; configuration 0 moves the link by (0, 0, 4), configuration 1 turns it a quarter about z;
    view 0: a camera at (0, 0, -1) looking along +z; view 1: a camera at the origin whose axes x, y, z are the world's +y, -z and
    -x (world_from_cam's columns are the camera's axes)."""
    from omg_planner_amd import robot_filter as rf
    poses = np.tile(np.eye(4), (2, 10, 1, 1))
    poses[0, 4, 2, 3] = 4.0
    poses[1, 4, :3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    back = np.eye(4)
    back[2, 3] = -1.0  # world_from_cam
    along_x = np.eye(4)
    along_x[:3, :3] = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0]]).T
    cams = RC.camera_records(np.stack([np.linalg.inv(back), np.linalg.inv(along_x)]), RC.IDENTITY_CAMERA)
    cs = rf.camera_spheres(poses, [(1.0, 2.0, 3.0, 0.25)], [4], cams, [0, 1], 0.5)
    # view 0: w = (1, 2, 7), minus t = (0, 0, -1): (1, 2, 8).  view 1: w = (-2, 1, 3); c = R^T w with R's columns (0, 1, 0), (0, 0, -1), (-1, 0, 0)
    assert cs.tolist() == [[[1.0, 2.0, 8.0, 0.75]], [[1.0, -3.0, 2.0, 0.75]]]
    assert rf.camera_spheres(poses, [(1.0, 2.0, 3.0, 0.25)], [4], cams, [1, 0], 0.5)[:, 0, :3].tolist() == [[-2.0, 1.0, 4.0], [2.0, -7.0, -1.0]]


def test_explained_and_filter_depth():
    from omg_planner_amd import robot_filter as rf
    depth = np.array([NAN, 0.0, -1.0, INF, 2.0, 2.75, 2.5, 3.5, INF, 1.0])
    t_near = np.array([3.0] * 8 + [INF, INF])
    want = [False, False, False, True, False, True, False, True, False, False]
    assert rf.explained(depth, t_near, 0.25).tolist() == want
    out = rf.filter_depth(depth, t_near, 0.25)
    assert out[want].tolist() == [0.0, 0.0, 0.0] and np.array_equal(out[~np.array(want)], depth[~np.array(want)], equal_nan=True)
    assert np.isnan(depth[0]) and depth[3] == INF  # the caller's images are not changed


def test_clear_edge_cases_as_known_answers():
    from omg_planner_amd import fusion, robot_filter as rf
    assert (fusion.FREE, fusion.SURFACE, fusion.UNKNOWN) == (RC.F, RC.S, RC.U)
    for what, volume, rng_, old, new in RC.CLEAR_CASES:  # one by one, back to back
        got = rf.clear_states(np.array(old, np.uint8), [volume], RC.clear_views(), [rng_], RC.CLEAR_DEPTH, RC.CLEAR_NEAR, RC.CLEAR_T_NEAR,
                              RC.CLEAR_SPHERES, RC.CLEAR_TOL)
        assert got.tolist() == new, what
    b = RC.clear_edge_batch()  # as one batch, with guard bytes around and between the volumes
    state = b["state"].copy()
    got = rf.clear_states(state, b["volumes"], RC.clear_views(), b["ranges"], RC.CLEAR_DEPTH, RC.CLEAR_NEAR, RC.CLEAR_T_NEAR, RC.CLEAR_SPHERES,
                          RC.CLEAR_TOL, state_begin=b["begin"])
    assert np.array_equal(got, b["want"]) and np.array_equal(state, b["state"]) and (got == RC.GUARD).sum() == (b["state"] == RC.GUARD).sum()


# ---------------------------------------------------------------------------------------------------------------------
# 2. csrc/omg_robot_filter_body.h on the host
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include "omg_robot_filter_body.h"
// cam: fx, fy, cx, cy, world_from_cam [12] per view.
extern "C" void host_camera_spheres(const double* poses, const double* local, const int32_t* link, int N, const double* cam,
                                    const int32_t* config_of_view, int V, double pad, double* out) {
    for (int v = 0; v < V; ++v)
        for (int n = 0; n < N; ++n)
            robot_camera_sphere(poses + ((int64_t)config_of_view[v] * 10 + link[n]) * 16, local + n * 4, cam + v * 16 + 4, pad, out + ((int64_t)v * N + n) * 4);
}
// Pixel by pixel as a lane of k_render_spheres walks the spheres; cull: a pixel skips the sphere its own cone test refuses (the
// kernel skips only where the whole wave refuses: what is proven here for every lane holds for every wave).
extern "C" void host_render(const double* spheres, int N, const double* cam, int V, int H, int W, double t_min, int cull, double* t_out,
                            int32_t* sphere_out) {
    for (int v = 0; v < V; ++v)
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const double* k = cam + v * 16;
                const double dx = ((double)c - k[2]) / k[0], dy = ((double)r - k[3]) / k[1], dd = (dx * dx + dy * dy) + 1.0;
                double best = __builtin_inf();
                int32_t which = -1;
                for (int n = 0; n < N; ++n) {
                    const double* s = spheres + ((int64_t)v * N + n) * 4;
                    const double q = robot_sphere_q(s);
                    if (cull && !robot_sphere_active(s, q, dx, dy, dd)) continue;
                    double entry;
                    if (robot_sphere_entry(s, q, dx, dy, dd, t_min, &entry) && entry < best) best = entry, which = n;
                }
                t_out[((int64_t)v * H + r) * W + c] = best, sphere_out[((int64_t)v * H + r) * W + c] = which;
            }
}
// One volume in runs of 256 nodes as k_clear_robot visits them; cull: the run drops the spheres robot_run_drops names.
// -> the number of (run, view, sphere) triples dropped.
extern "C" int64_t host_clear(const omgx_mesh* ms, const double* views, int v0, int count, const double* depth, const double* t_near, int H,
                              int W, const double* spheres, int N, double near, double tol, int cull, uint8_t* state) {
    const int64_t total = (int64_t)ms->dims[0] * ms->dims[1] * ms->dims[2];
    int64_t dropped = 0;
    for (int64_t id0 = 0; id0 < total; id0 += 256) {
        const int64_t last = id0 + 255 < total - 1 ? id0 + 255 : total - 1;
        int lo[3], hi[3];
        robot_run_box(ms->dims, (uint32_t)id0, (uint32_t)last, lo, hi);
        for (int64_t id = id0; id <= last; ++id) {
            double p[3];
            volume_node_point(*ms, (uint32_t)id, p);
            bool inside = false, front = false;
            for (int v = v0; v < v0 + count; ++v) {
                double q[3], ball[5];
                bool f;
                robot_view_front(views + 16 * v, depth + (int64_t)v * H * W, t_near + (int64_t)v * H * W, H, W, p, near, tol, q, &f);
                front = front || f;
                robot_run_ball(*ms, lo, hi, views + 16 * v, ball);
                for (int n = 0; n < N; ++n) {
                    const double* s = spheres + ((int64_t)v * N + n) * 4;
                    if (cull && robot_run_drops(ball, s)) {
                        dropped += id == id0;
                        continue;
                    }
                    inside = inside || robot_inside(q, s[0], s[1], s[2], s[3] * s[3]);
                }
            }
            state[id] = robot_new_state(state[id], inside, front);
        }
    }
    return dropped;
}
"""


def _host_lib(tmp_path):
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    return KB.host_harness(_HOST_HARNESS, tmp_path, {"host_camera_spheres": (None, [vp, vp, vp, i, vp, vp, i, d, vp]),
                                                     "host_render": (None, [vp, i, vp, i, i, i, d, i, vp, vp]),
                                                     "host_clear": (C.c_int64, [vp, vp, i, i, vp, vp, i, i, vp, i, d, d, i, vp])})


def _camera_rows(cameras):
    return np.ascontiguousarray(np.concatenate([np.stack([cameras[k] for k in ("fx", "fy", "cx", "cy")], -1), cameras["world_from_cam"]], 1))


def host_camera_spheres(lib, poses, local, link, cameras, config_of_view, pad):
    poses, local = np.ascontiguousarray(poses, np.float64), np.ascontiguousarray(local, np.float64).reshape(-1, 4)
    link, cfg, cam = np.ascontiguousarray(link, np.int32), np.ascontiguousarray(config_of_view, np.int32), _camera_rows(cameras)
    out = np.zeros((len(cam), len(local), 4))
    lib.host_camera_spheres(poses.ctypes.data, local.ctypes.data, link.ctypes.data, len(local), cam.ctypes.data, cfg.ctypes.data, len(cam), float(pad),
                            out.ctypes.data)
    return out


def host_render(lib, cam_spheres, cameras, H, W, t_min, cull):
    s, cam = np.ascontiguousarray(cam_spheres, np.float64), _camera_rows(cameras)
    t, which = np.zeros((len(cam), H, W)), np.zeros((len(cam), H, W), np.int32)
    lib.host_render(s.ctypes.data, s.shape[1], cam.ctypes.data, len(cam), H, W, float(t_min), int(cull), t.ctypes.data, which.ctypes.data)
    return t, which


def host_clear(lib, state, volumes, views, ranges, depth, near, t_near, cam_spheres, tol, begin, cull):
    """-> (the new states, the number of (run, view, sphere) triples the cull dropped)."""
    from omg_planner_amd import ops
    out = np.array(state, np.uint8)
    views, depth = np.ascontiguousarray(views, np.float64).reshape(-1, 16), np.ascontiguousarray(depth, np.float64)
    t_near, s = np.ascontiguousarray(t_near, np.float64), np.ascontiguousarray(cam_spheres, np.float64)
    rec = ops.surface_records([tuple(v[:4]) + (0,) for v in volumes])
    dropped = 0
    for m in range(len(volumes)):
        n = int(np.prod(volumes[m][3]))
        mine = np.ascontiguousarray(out[int(begin[m]): int(begin[m]) + n])
        dropped += lib.host_clear(C.byref(rec[m]), views.ctypes.data, int(ranges[m][0]), int(ranges[m][1]), depth.ctypes.data, t_near.ctypes.data,
                                  depth.shape[1], depth.shape[2], s.ctypes.data, s.shape[1], float(near), float(tol), int(cull), mine.ctypes.data)
        out[int(begin[m]): int(begin[m]) + n] = mine
    return out, dropped


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@KB.requires_host_cxx
def test_kernel_body_compiled_for_the_host_equals_the_specification(tmp_path):
    """csrc/omg_robot_filter_body.h is what a thread of the two kernels does for its sphere, its pixel and its node; compiled for
    the host without contraction it gives the specification's bits on the edge cases and on the seeded batch (N = 1, 7 and one
    more than the staging chunk), with either cull on and off.  The culls do drop something: otherwise they prove nothing."""
    from omg_planner_amd import _lib
    assert _lib.CONSTANTS["OMGX_ROBOT_SPHERE_CHUNK"] == RC.CHUNK and _lib.CONSTANTS["OMGX_ROBOT_MAX_SPHERES"] >= 2048
    lib = _host_lib(tmp_path)
    from omg_planner_amd import robot_filter as rf
    e = RC.render_edge_launch()
    want_cs = rf.camera_spheres(e["link_poses"], e["local"], e["link"], e["cameras"], e["config_of_view"], 0.0)
    want = rf.render_spheres(want_cs, e["cameras"], e["H"], e["W"], RC.RENDER_T_MIN)
    cs = host_camera_spheres(lib, e["link_poses"], e["local"], e["link"], e["cameras"], e["config_of_view"], 0.0)
    assert _same(cs, want_cs)
    for cull in (0, 1):
        got = host_render(lib, cs, e["cameras"], e["H"], e["W"], RC.RENDER_T_MIN, cull)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), cull
    b = RC.clear_edge_batch()
    for cull in (0, 1):
        got, _ = host_clear(lib, b["state"], b["volumes"], RC.clear_views(), b["ranges"], RC.CLEAR_DEPTH, RC.CLEAR_NEAR, RC.CLEAR_T_NEAR,
                            RC.CLEAR_SPHERES, RC.CLEAR_TOL, b["begin"], cull)
        assert _same(got, b["want"]), cull
    for N in RC.BATCH_N:
        c = RC.batch(N)
        cs = host_camera_spheres(lib, c["link_poses"], c["local"], c["link"], c["cameras"], c["config_of_view"], RC.BATCH_PAD)
        assert _same(cs, c["cam_spheres"]), N
        for cull in (0, 1):
            t, which = host_render(lib, cs, c["cameras"], RC.BATCH_H, RC.BATCH_W, RC.BATCH_T_MIN, cull)
            assert _same(t, c["t_near"]) and _same(which, c["sphere"]), (N, cull)
            got, dropped = host_clear(lib, c["state"], RC.BATCH_VOLUMES, c["views"], RC.BATCH_RANGES, c["depth"], RC.BATCH_NEAR, c["t_near"], cs,
                                      RC.BATCH_TOL, c["begin"], cull)
            assert _same(got, c["want"]), (N, cull)
            assert (dropped > 0) == (cull == 1), (N, cull, dropped)
        # the batch is worth its name: hits and misses, explained pixels, nodes freed by either rule, a camera inside the arm
        changed = c["want"] != c["state"]
        print("N", N, "hit pixels", int(np.isfinite(c["t_near"]).sum()), "of", c["t_near"].size, "explained",
              int(rf.explained(c["depth"], c["t_near"], RC.BATCH_TOL).sum()), "states changed", int(changed.sum()))
        assert np.isfinite(c["t_near"]).any() and np.isinf(c["t_near"]).any() and changed.any()
        assert (c["t_near"][2] == RC.BATCH_T_MIN).any()  # the third camera stands inside a sphere
        assert ((c["state"] == RC.S) & changed).any() and ((c["state"] == RC.U) & changed).any()
        assert (c["want"] == RC.GUARD).sum() == (c["state"] == RC.GUARD).sum() and not ((c["state"] == RC.F) & changed).any()


@KB.requires_host_cxx
def test_fuzz_generator_against_the_body_compiled_for_the_host(tmp_path):
    """The generator of tests/fuzz/fuzz_robot_filter.py without a GPU: the draws of the GPU test's seed through the body header on
    the host equal the specification, and between them they reach no sphere and more than a chunk of them, both culls, empty view
    ranges, a 1 x 1 image and a camera inside a sphere."""
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("fuzz_robot_filter", Path(__file__).resolve().parent / "fuzz" / "fuzz_robot_filter.py")
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    lib = _host_lib(tmp_path)
    rng = np.random.default_rng(fuzz.SMOKE_SEED)
    counts, culls, empty, tiny, inside, changed = set(), set(), 0, 0, 0, 0
    for _ in range(fuzz.SMOKE_TRIALS):
        c = fuzz.draw(rng)
        cs, t_near, which, depth, want = fuzz.specification(c)
        got_cs = host_camera_spheres(lib, c["poses"], c["local"], c["link"], c["cams"], c["cfg"], c["pad"])
        t, n = host_render(lib, got_cs, c["cams"], c["H"], c["W"], c["t_min"], c["cull"])
        assert _same(got_cs, cs) and _same(t, t_near) and _same(n, which), (c["N"], c["H"], c["W"])
        got, _ = host_clear(lib, c["state"], c["volumes"], c["views"], c["ranges"], depth, c["near"], t_near, cs, c["tol"], c["begin"], c["cull"])
        assert _same(got, want), (c["N"], [v[3] for v in c["volumes"]], c["ranges"])
        counts.add(c["N"]), culls.add(c["cull"])
        empty += sum(r[1] == 0 for r in c["ranges"])
        tiny += (c["H"], c["W"]) == (1, 1)
        inside += int((t_near == c["t_min"]).any())
        changed += int((want != c["state"]).sum())
    print("sphere counts", sorted(counts), "empty ranges", empty, "1 x 1 images", tiny, "cameras inside a sphere", inside, "states changed", changed)
    assert 0 in counts and max(counts) > RC.CHUNK and culls == {False, True} and empty > 0 and tiny > 0 and inside > 0 and changed > 1000


# ---------------------------------------------------------------------------------------------------------------------
# 3. the path in numpy
# ---------------------------------------------------------------------------------------------------------------------
def test_filtered_carve_equals_the_arm_free_carve_away_from_the_arm():
    """fusion_cases' scene with an arm of six spheres (radius 0.025) composited into the three images as min(t_scene, t_arm); the
    filter knows the spheres at radius + 0.01.  Carving the filtered depth and then clear_states gives the states of carving the
    arm-free images, except on the exempt nodes: inside a padded sphere, or projecting onto an explained pixel of a view that
    sees them (there the arm hides the scene).  A pixel that is not explained shows the scene as the arm-free image does: the bare
    arm lies behind its padded entry, so min() took the scene.  No node within r + pad of a centre is SURFACE afterwards; the
    same carve without the filter has SURFACE nodes there, which is the failure the feature removes."""
    from omg_planner_amd import fusion, robot_filter as rf
    a = RC.scene_with_arm()
    vols, ranges, views = [FC.SCENE_VOLUME], [(0, 3)], a["views"]
    assert (a["t_arm"] < a["t_scene"]).sum() > 100  # the arm is in the images
    mask = rf.explained(a["t_arm"], a["t_near"], RC.ARM_TOL)
    filtered = rf.filter_depth(a["t_arm"], a["t_near"], RC.ARM_TOL)
    assert (filtered[mask] == 0.0).all() and _same(filtered[~mask], a["t_arm"][~mask]) and _same(a["t_arm"][~mask], a["t_scene"][~mask])
    carved = fusion.carve_views(vols, views, ranges, filtered, FC.BAND, FC.NEAR)
    got = rf.clear_states(carved, vols, views, ranges, a["t_arm"], FC.NEAR, a["t_near"], a["cam_spheres"], RC.ARM_TOL)
    clean = FC.scene_states(3).ravel()
    p = fusion.node_points(np.array(FC.ORIGIN), FC.DELTA, 0.5, FC.DIMS)
    exempt = np.zeros(len(p), bool)
    for v in range(3):
        q = [((views[v][4 + 4 * k] * p[:, 0] + views[v][5 + 4 * k] * p[:, 1]) + views[v][6 + 4 * k] * p[:, 2]) + views[v][7 + 4 * k] for k in range(3)]
        c, r = np.floor((views[v][0] * (q[0] / q[2]) + views[v][2]) + 0.5), np.floor((views[v][1] * (q[1] / q[2]) + views[v][3]) + 0.5)
        seen = (q[2] > FC.NEAR) & (c >= 0) & (c <= FC.W - 1) & (r >= 0) & (r <= FC.H - 1)
        exempt |= seen & mask[v][np.where(seen, r, 0).astype(int), np.where(seen, c, 0).astype(int)]
    dist = np.linalg.norm(p[:, None, :] - RC.ARM_CENTRES[None], axis=2).min(1)
    in_arm = dist <= RC.ARM_RADIUS + RC.ARM_PAD - 1e-12
    exempt |= dist <= RC.ARM_RADIUS + RC.ARM_PAD + 1e-12
    print("exempt nodes", int(exempt.sum()), "of", len(p), "inside the padded arm", int(in_arm.sum()))
    assert exempt.sum() <= len(p) // 4 and in_arm.sum() > 100
    assert np.array_equal(got[~exempt], clean[~exempt])
    assert (got[in_arm] == fusion.FREE).all()
    unfiltered = fusion.carve_views(vols, views, ranges, a["t_arm"], FC.BAND, FC.NEAR)
    assert (unfiltered[in_arm] == fusion.SURFACE).sum() > 20 and (clean[in_arm] == fusion.SURFACE).sum() == 0
    assert (got == fusion.SURFACE).sum() > 500  # the scene is still there


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_specification_argument_errors():
    from omg_planner_amd import robot_filter as rf
    poses, cam = np.tile(np.eye(4), (2, 10, 1, 1)), _identity_cameras(2)
    good = dict(link_poses=poses, local=[(0.0, 0.0, 2.0, 0.5)], link=[0], cameras=cam, config_of_view=[0, 1], pad=0.0)
    bad_pose = poses.copy()
    bad_pose[1, 9, 3, 3] = NAN
    bad_cam, zero_f = cam.copy(), cam.copy()
    bad_cam["world_from_cam"][1, 11], zero_f["fy"][0] = INF, 0.0
    for change in (dict(local=[(0.0, NAN, 2.0, 0.5)]), dict(local=[(0.0, 0.0, 2.0, INF)]), dict(local=[(0.0, 0.0, 2.0, -0.5)]), dict(link=[10]),
                   dict(link=[-1]), dict(link=[0, 1]), dict(link_poses=bad_pose), dict(link_poses=poses[:, :9]), dict(cameras=bad_cam),
                   dict(cameras=zero_f), dict(cameras=np.zeros((2, 16))), dict(config_of_view=[0, 2]), dict(config_of_view=[-1, 0]),
                   dict(config_of_view=[0]), dict(pad=NAN), dict(pad=INF), dict(pad=-0.01)):
        with pytest.raises(ValueError):
            rf.camera_spheres(**{**good, **change})
    cs = rf.camera_spheres(**good)
    for change in (dict(H=0), dict(W=0), dict(t_min=NAN), dict(t_min=-1.0), dict(t_min=INF), dict(cam_spheres=cs[:1]), dict(cam_spheres=cs[:, :, :3]),
                   dict(cam_spheres=np.where(cs == 2.0, NAN, cs)), dict(cam_spheres=np.where(cs == 0.5, -0.5, cs)), dict(cameras=bad_cam)):
        with pytest.raises(ValueError):
            rf.render_spheres(**{**dict(cam_spheres=cs, cameras=cam, H=2, W=2, t_min=0.0), **change})
    vol = FC.line_volume([1.0, 2.0])
    ok = dict(state=np.array([2, 2], np.uint8), volumes=[vol], views=RC.clear_views(), view_range=[(0, 2)], depth=RC.CLEAR_DEPTH, near=1.0,
              t_near=RC.CLEAR_T_NEAR, cam_spheres=RC.CLEAR_SPHERES, tol=0.25)
    assert rf.clear_states(**ok).tolist() == [2, 0]
    bad_s, neg_s, bad_v, zero_v = RC.CLEAR_SPHERES.copy(), RC.CLEAR_SPHERES.copy(), RC.clear_views(), RC.clear_views()
    bad_s[1, 1, 0], neg_s[0, 0, 3], bad_v[1, 9], zero_v[0, 0] = NAN, -1.0, INF, 0.0
    for change in (dict(near=NAN), dict(tol=INF), dict(cam_spheres=bad_s), dict(cam_spheres=neg_s), dict(cam_spheres=RC.CLEAR_SPHERES[:1]),
                   dict(t_near=RC.CLEAR_T_NEAR[:1]), dict(depth=RC.CLEAR_DEPTH[:1]), dict(t_near=RC.CLEAR_T_NEAR[:, :, :3]),
                   dict(depth=RC.CLEAR_DEPTH[:, :1]), dict(views=bad_v), dict(views=zero_v), dict(view_range=[(0, 3)]), dict(view_range=[(-1, 1)]),
                   dict(view_range=[(0, 1), (0, 1)]), dict(state=np.array([2], np.uint8)), dict(state_begin=[-1]), dict(state_begin=[1]),
                   dict(volumes=[vol[:1] + (0.0,) + vol[2:]])):
        with pytest.raises(ValueError):
            rf.clear_states(**{**ok, **change})


def _volumes(M=2, **over):
    from omg_planner_amd import _lib
    rec = (_lib.Mesh * M)()
    for m in range(M):
        r = rec[m]
        r.origin[:], r.delta, r.sample_offset, r.dims[:] = [0.0, 0.0, 0.0], 0.01, 0.5, [4, 5, 6 + m]
        r.out_offset, r.first_workgroup = 1000 * m, m
    for k, val in over.items():
        if k in ("origin", "dims"):
            getattr(rec[M - 1], k)[:] = val
        else:
            setattr(rec[M - 1], k, val)
    return rec


def test_c_abi_argument_checks_without_gpu():
    """Every OMGX_ERR_INVALID / OMGX_ERR_UNSUPPORTED case of the two entry points is decided on the host copies before any HIP
    call: the device pointers below are never dereferenced."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    assert lib.omgx_abi_version() == 14 and len(_lib.STRUCTS) == 8
    INV, UNS, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED, _lib.OMGX_OK
    arr = lambda a: C.c_void_p(a.ctypes.data)
    d = C.c_void_p(4096)
    cams = _identity_cameras(2)

    def render(spheres=((0.0, 0.0, 2.0, 0.5),) * 3, links=(0, 4, 9), poses=None, cams=cams, cfg=(0, 1), N=None, Cn=None, V=None, H=4, W=5, pad=0.0,
               t_min=0.0, **ptr):
        local, link = np.ascontiguousarray(spheres, np.float64), np.ascontiguousarray(links, np.int32)
        poses = np.ascontiguousarray(np.tile(np.eye(4), (2, 10, 1, 1)) if poses is None else poses)
        cameras, cfg = np.ascontiguousarray(cams), np.ascontiguousarray(cfg, np.int32)
        p = dict(local=d, link=d, link_poses=d, cameras=d, config_of_view=d, cam_spheres=d, t_near=d, sphere=d, h_local=arr(local), h_link=arr(link),
                 h_link_poses=arr(poses), h_cameras=arr(cameras), h_config_of_view=arr(cfg))
        p.update(ptr)
        return lib.omgx_render_spheres(p["local"], p["h_local"], p["link"], p["h_link"], len(link) if N is None else N, p["link_poses"],
                                       p["h_link_poses"], len(poses) if Cn is None else Cn, p["cameras"], p["h_cameras"], p["config_of_view"],
                                       p["h_config_of_view"], len(cameras) if V is None else V, H, W, pad, t_min, 1, p["cam_spheres"], p["t_near"],
                                       p["sphere"], None)

    for k in ("local", "h_local", "link", "h_link", "link_poses", "h_link_poses", "cameras", "h_cameras", "config_of_view", "h_config_of_view",
              "cam_spheres", "t_near", "sphere"):
        assert render(**{k: None}) == INV, k
    assert render(V=0) == OK and render(V=0, cameras=None, h_cameras=None, config_of_view=None, h_config_of_view=None, t_near=None, sphere=None) == OK
    assert render(N=-1) == INV and render(Cn=-1) == INV and render(V=-1) == INV and render(H=0) == INV and render(W=0) == INV
    for bad in (NAN, INF, -INF, -0.5):
        assert render(pad=bad) == INV and render(t_min=bad) == INV
    for col in range(4):
        for bad in (NAN, INF) + ((-1.0,) if col == 3 else ()):
            s = np.array([(0.0, 0.0, 2.0, 0.5)] * 3)
            s[2, col] = bad
            assert render(spheres=s) == INV, (col, bad)
    for link in ((0, 4, 10), (-1, 4, 9)):
        assert render(links=link) == INV
    for at in ((0, 0, 0, 0), (1, 9, 3, 3), (1, 5, 1, 2)):
        poses = np.tile(np.eye(4), (2, 10, 1, 1))
        poses[at] = NAN
        assert render(poses=poses) == INV, at
    for name in ("fx", "fy", "cx", "cy"):
        for bad in (NAN, INF) + ((0.0,) if name in ("fx", "fy") else ()):
            c = cams.copy()
            c[name][1] = bad
            assert render(cams=c) == INV, (name, bad)
    c = cams.copy()
    c["world_from_cam"][0, 7] = NAN
    assert render(cams=c) == INV
    assert render(cfg=(0, 2)) == INV and render(cfg=(-1, 0)) == INV and render(Cn=0, link_poses=None, h_link_poses=None) == INV
    # limits, reported after every invalid argument
    many = _lib.CONSTANTS["OMGX_ROBOT_MAX_SPHERES"] + 1
    assert render(spheres=np.tile((0.0, 0.0, 2.0, 0.5), (many, 1)), links=np.zeros(many, np.int32)) == UNS
    assert render(spheres=np.tile((0.0, 0.0, 2.0, -0.5), (many, 1)), links=np.zeros(many, np.int32)) == INV
    assert render(H=1 << 16, W=1 << 16) == UNS and render(cams=_identity_cameras(65536), cfg=np.zeros(65536, np.int32)) == UNS

    good_views = np.stack([FC.view(2.0, 3.0, 1.0, 1.0)] * 3)
    vpc = lambda x: C.cast(x, C.c_void_p)

    def clear(rec=None, M=None, views=good_views, V=None, ranges=None, begin=(0, 120), H=4, W=5, spheres=None, N=None, near=0.05, tol=0.01,
              state_elems=1 << 20, **ptr):
        rec = _volumes() if rec is None else rec
        views = np.ascontiguousarray(views, np.float64)
        ranges = np.ascontiguousarray([(0, 3), (1, 2)] + [(0, 1)] * (len(rec) - 2) if ranges is None else ranges, np.int32)
        begin = np.ascontiguousarray(begin, np.int64)
        spheres = np.ascontiguousarray(np.tile((0.0, 0.0, 2.0, 0.5), (len(views), 2, 1)) if spheres is None else spheres, np.float64)
        p = dict(volumes=d, views=d, view_range=d, state_begin=d, depth=d, t_near=d, cam_spheres=d, state=d, h_views=arr(views), h_view_range=arr(ranges),
                 h_state_begin=arr(begin), h_volumes=vpc(rec), h_cam_spheres=arr(spheres))
        p.update(ptr)
        return lib.omgx_clear_robot(p["volumes"], p["h_volumes"], len(rec) if M is None else M, p["views"], p["h_views"], len(views) if V is None else V,
                                    p["view_range"], p["h_view_range"], p["state_begin"], p["h_state_begin"], p["depth"], p["t_near"], H, W,
                                    p["cam_spheres"], p["h_cam_spheres"], spheres.shape[1] if N is None else N, near, tol, 1, p["state"], state_elems, None)

    for k in ("volumes", "h_volumes", "views", "h_views", "view_range", "h_view_range", "state_begin", "h_state_begin", "depth", "t_near", "cam_spheres",
              "state"):
        assert clear(**{k: None}) == INV, k
    assert clear(M=0) == OK and clear(M=0, volumes=None, h_volumes=None, state=None) == OK
    assert clear(M=-1) == INV and clear(V=-1) == INV and clear(N=-1) == INV and clear(state_elems=-1) == INV and clear(H=0) == INV and clear(W=0) == INV
    for bad in (NAN, INF, -INF):
        assert clear(near=bad) == INV and clear(tol=bad) == INV
    for col in range(4):
        for bad in (NAN, INF) + ((-0.5,) if col == 3 else ()):
            s = np.tile((0.0, 0.0, 2.0, 0.5), (3, 2, 1))
            s[2, 1, col] = bad
            assert clear(spheres=s) == INV, (col, bad)
    for col in range(16):
        v = good_views.copy()
        v[2, col] = NAN
        assert clear(views=v) == INV, col
    v = good_views.copy()
    v[1, 1] = 0.0
    assert clear(views=v) == INV
    for ranges in (((0, 4), (1, 2)), ((0, 3), (3, 1)), ((-1, 2), (1, 2)), ((0, 3), (1, -1))):
        assert clear(ranges=ranges) == INV, ranges
    for bad_rec in (_volumes(dims=[0, 4, 4]), _volumes(delta=0.0), _volumes(sample_offset=0.25), _volumes(origin=[NAN, 0, 0]), _volumes(first_workgroup=2)):
        assert clear(rec=bad_rec) == INV
    assert clear(begin=(-1, 120)) == INV and clear(begin=(0, 119)) == INV and clear(state_elems=120 + 139) == INV
    assert clear(rec=_volumes(1, dims=[2048, 1024, 1024]), begin=(0,), ranges=[(0, 1)], state_elems=1 << 40) == UNS
    assert clear(H=1 << 15, W=1 << 15) == UNS and clear(N=many, h_cam_spheres=None) == UNS and clear(N=many, h_cam_spheres=None, begin=(0, 119)) == INV


def test_wrapper_checks_without_gpu():
    """RobotSpheres' and the wrappers' own refusals come before anything touches a device."""
    import torch
    from omg_planner_amd import _lib, camera, ops, pipeline
    import inspect
    E = _lib.OmgHipError
    for bad in (dict(local=[(0.0, 0.0, NAN, 0.1)], link=[0]), dict(local=[(0.0, 0.0, 0.0, -0.1)], link=[0]), dict(local=[(0.0, 0.0, 0.0, 0.1)], link=[10]),
                dict(local=[(0.0, 0.0, 0.0, 0.1)], link=[0, 1])):
        with pytest.raises(E):
            ops.RobotSpheres(device="cpu", **bad)
    with pytest.raises(E, match=r"\[10,P,3\]"):
        ops.RobotSpheres.from_points(np.zeros((9, 4, 3)), 0.04, device="cpu")
    with pytest.raises(E, match="one value per link"):
        ops.RobotSpheres.from_points(np.zeros((10, 4, 3)), [0.04, 0.05], device="cpu")
    s = ops.RobotSpheres.from_points(np.arange(120.0).reshape(10, 4, 3), np.arange(10) * 0.01, device="cpu")
    assert s.N == 40 and s.h_link.tolist() == np.repeat(np.arange(10), 4).tolist() and s.h_local[5].tolist() == [15.0, 16.0, 17.0, 0.01]
    with pytest.raises(E, match="device tensor"):
        ops.render_spheres(s, torch.zeros((1, 10, 4, 4), dtype=torch.float64), _identity_cameras(), [0], 4, 4)
    vols = [((0.0, 0.0, 0.0), 0.01, "centre", (4, 4, 4), 0)]
    depth = torch.zeros((1, 4, 4), dtype=torch.float64)
    with pytest.raises(E, match="near and tol must be finite"):
        ops.clear_robot(torch.zeros(64, dtype=torch.uint8), None, vols, [FC.view()], [(0, 1)], depth, 0.05, depth, torch.zeros((1, 1, 4), dtype=torch.float64), NAN)
    with pytest.raises(E, match="device tensor"):
        ops.clear_robot(torch.zeros(64, dtype=torch.uint8), None, vols, [FC.view()], [(0, 1)], depth, 0.05, depth, torch.zeros((1, 1, 4), dtype=torch.float64), 0.01)
    with pytest.raises(E, match="RobotView"):
        ops._robot_step(object(), depth, [FC.view()], [(0, 1)], 0.05)
    same, step = ops._robot_step(None, depth, [FC.view()], [(0, 1)], 0.05)
    assert same is depth and step is None  # no robot: the call's own depth, no step
    for fn in (ops.DeviceScenes.fuse_obstacles, ops.DeviceScenes.integrate_obstacles, ops.DeviceScenes.segment_obstacles, camera.Observation.fuse_obstacles,
               camera.Observation.integrate_obstacles, camera.Observation.segment_obstacles, pipeline.plan_observed, pipeline.plan_on_unknown_support):
        assert inspect.signature(fn).parameters["robot"].default is None, fn
    assert inspect.signature(camera.Observation.fit_supports).parameters["skip"].default is None and hasattr(camera.Observation, "robot_view")


# ---------------------------------------------------------------------------------------------------------------------
# 5. registers
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_robot_filter_kernels_do_not_spill(tmp_path):
    """The compiler's resource remarks for csrc/omg_robot_filter.hip: neither kernel uses scratch or spills.  Registers, LDS and
    occupancy are printed, not pinned (the LDS is the staged chunk: 5 and 4 doubles per sphere, and the four waves' counts)."""
    seen = KB.kernel_resources("omg_robot_filter.hip", tmp_path)
    assert len(seen) == 2
    for part in ("k_render_spheres", "k_clear_robot"):
        v = KB.one(seen, part)
        print(part, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (part, v)
