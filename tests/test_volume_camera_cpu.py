"""The depth camera on the SDF pool without a GPU: volume_camera.render_volumes against written answers at
the edges of its rule, csrc/omg_volume_camera_body.h compiled for the host against the specification bit for bit, the analytic
sphere with derived bounds, the surface-nets route it stands beside, every refused argument (specification, C ABI, wrappers) and
the compiler's resource figures of the kernel."""
from __future__ import annotations

import ctypes as C
import types

import numpy as np
import pytest

from tests import kernel_build as KB
from tests import volume_camera_cases as VC

INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# 1. written answers
# ---------------------------------------------------------------------------------------------------------------------
def test_edges_of_the_rule_against_the_written_answers():
    from omg_planner_amd import volume_camera as vc
    groups = VC.edge_groups()
    assert sum(len(idx) for _, idx in groups) == len(VC.EDGE_CASES) == 18 and len(groups) == 5
    for args, idx in groups:
        objects, begin, pool, cameras, visible, _ = VC.edge_batch(idx)
        t, inst, normal, steps = vc.render_volumes(objects, begin, pool, cameras, 1, 1, visible=visible, **args)
        VC.edge_check(idx, t, inst, normal, steps)


def test_the_shared_trilinear_body_leaves_value_gradient_as_it_was():
    """registration.value_gradient now calls registration.trilinear: on a random volume its value equals the eight-corner formula
    written out here, and points outside give zeros."""
    from omg_planner_amd import registration as reg
    rng = np.random.default_rng(3)
    data = rng.normal(size=(4, 5, 6)).astype(np.float32)
    obj = VC.record(data.shape, (0.0, 0.0, 0.0), 0.5, 0)
    q = rng.uniform(-0.2, 3.2, (200, 3))
    inside, v, g = reg.value_gradient(obj, data.ravel(), q)
    assert inside.any() and not inside.all() and (v[~inside] == 0).all() and (g[~inside] == 0).all()
    u = q[inside] * 2.0 - 0.5
    i = u.astype(int)
    f = u - i
    c = lambda a, b, d: data[i[:, 0] + a, i[:, 1] + b, i[:, 2] + d].astype(np.float64)
    z = lambda a, b: c(a, b, 0) + f[:, 2] * (c(a, b, 1) - c(a, b, 0))
    y = lambda a: z(a, 0) + f[:, 1] * (z(a, 1) - z(a, 0))
    assert np.array_equal(v[inside], y(0) + f[:, 0] * (y(1) - y(0))) and np.array_equal(g[inside, 0], (y(1) - y(0)) * 2.0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the kernel body compiled for the host: the kernel's loop, pixel by pixel
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include "omg_volume_camera_body.h"
struct rec { float pose_inv[12], lo[3], hi[3]; int32_t dim[3]; float delta, epsilon, padding_scale, clearance; int32_t disabled;
             int64_t grid_offset; double inv_extent[3]; float rb_c[3], rb_h[3], rb_r, rb_r2; double inv_delta; float inv_2eps, inv_eps; };
static_assert(sizeof(rec) == 184, "omgx_object");
extern "C" void host_render(const rec* objects, const int32_t* scene_begin, int S, const float* pool, int64_t pool_elems, const double* cameras,
                            const uint8_t* visible, int H, int W, double level, double t_min, double min_step, double relax, int max_steps,
                            double* t_out, int32_t* inst_out, double* normal_out, int32_t* steps_out) {
    for (int s = 0; s < S; ++s)
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const double* cam = cameras + 16 * s;
                const double dx = ((double)c - cam[2]) / cam[0], dy = ((double)r - cam[3]) / cam[1];
                double best = __builtin_inf(), n[3] = {0.0, 0.0, 0.0};
                int32_t inst = -1, samples = 0;
                for (int k = 0; k < scene_begin[s + 1] - scene_begin[s]; ++k) {
                    const rec& ob = objects[scene_begin[s] + k];
                    if (visible && !visible[scene_begin[s] + k]) continue;
                    if (!vcam_grid_usable(ob.dim, ob.grid_offset, pool_elems)) continue;
                    vcam_grid G;
                    vcam_set_grid(ob.lo, ob.dim, ob.inv_delta, ob.grid_offset, G);
                    double m[12], t0, t1, th;
                    vcam_object_from_camera(ob.pose_inv, cam + 4, m);
                    vcam_ray R;
                    vcam_make_ray(G, m, dx, dy, R);
                    if (!vcam_slab(G, R, t_min, t0, t1)) continue;
                    if (vcam_march(G, pool, R, t0, t1, level, min_step, relax, max_steps, th, samples) && th < best) {
                        best = th, inst = k;
                        vcam_normal(G, pool, R, m, th, n);
                    }
                }
                const int64_t at = ((int64_t)s * H + r) * W + c;
                t_out[at] = best, inst_out[at] = inst, steps_out[at] = samples;
                for (int j = 0; j < 3; ++j) normal_out[3 * at + j] = n[j];
            }
}
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    if KB.host_compiler() is None:
        pytest.skip("no C++ compiler")
    vp, dbl, i = C.c_void_p, C.c_double, C.c_int
    return KB.host_harness(_HOST_HARNESS, tmp_path_factory.mktemp("volume_camera_host"),
                           {"host_render": (None, [vp, vp, i, vp, C.c_int64, vp, vp, i, i, dbl, dbl, dbl, dbl, i, vp, vp, vp, vp])})


def host_render(lib, objects, begin, pool, cameras, visible, H, W, level, t_min, min_step, relax, max_steps):
    objects, begin, pool = np.ascontiguousarray(objects), np.ascontiguousarray(begin, np.int32), np.ascontiguousarray(pool, np.float32)
    cameras, S = np.ascontiguousarray(cameras, np.float64), len(begin) - 1
    visible = None if visible is None else np.ascontiguousarray(visible, np.uint8)
    t, inst = np.full((S, H, W), 7.0), np.full((S, H, W), 77, np.int32)
    normal, steps = np.full((S, H, W, 3), 7.0), np.full((S, H, W), 77, np.int32)
    lib.host_render(objects.ctypes.data, begin.ctypes.data, S, pool.ctypes.data, len(pool), cameras.ctypes.data,
                    None if visible is None else visible.ctypes.data, H, W, level, t_min, min_step, relax, max_steps, t.ctypes.data, inst.ctypes.data,
                    normal.ctypes.data, steps.ctypes.data)
    return t, inst, normal, steps


@KB.requires_host_cxx
def test_the_kernel_body_on_the_host_equals_the_specification(host_lib):
    from omg_planner_amd import volume_camera as vc
    for args, idx in VC.edge_groups():
        objects, begin, pool, cameras, visible, _ = VC.edge_batch(idx)
        got = host_render(host_lib, objects, begin, pool, cameras, visible, 1, 1, **args)
        VC.edge_check(idx, *got)
        assert VC.same_images(got, vc.render_volumes(objects, begin, pool, cameras, 1, 1, visible=visible, **args))
    (objects, begin, pool, cameras, visible), args, want = VC.random_batch()
    assert {tuple(r["dim"]) for r in objects} >= {(5, 9, 7), (2, 2, 2)} and (want[1] >= 0).sum() > 100 and len(np.unique(want[1])) == 4
    assert not np.isfinite(pool).all() and (visible == 0).any()
    assert VC.same_images(host_render(host_lib, objects, begin, pool, cameras, visible, 11, 13, **args), want)
    assert VC.same_images(host_render(host_lib, objects, begin, pool, cameras, None, 11, 13, **args),
                          vc.render_volumes(objects, begin, pool, cameras, 11, 13, **args))
    objects, begin, pool, cameras, want = VC.ragged_batch()
    assert VC.same_images(host_render(host_lib, objects, begin, pool, cameras, None, VC.RAGGED_H, VC.RAGGED_W, **VC.RAGGED_ARGS), want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the analytic sphere
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 16])
def test_analytic_sphere_within_the_derived_bounds(n):
    """|x| - R, R = 0.1, on n^3 samples over a 0.32 m cube, a 48 x 64 camera with f = 60 at (0.02, -0.01, -0.6) looking along +z,
    min_step = delta / 16, max_steps = 256, relax = 1.  The bounds are derived, not fitted: the trilinear error of a distance field
    is at most (delta^2 / 8) * sum |f_aa| <= 3 delta^2 / (8 R), over the cosine of incidence (>= 0.5): delta^2 / R with a third of
    margin; a trilinear gradient is piecewise constant along its own axis, each component off by at most delta / (2 R), the vector
    by (sqrt 3 / 2) delta / R to first order: delta / R.  Measured (printed below; DESIGN.md section 7m keeps them): 32^3: depth
    0.461 delta^2/R, normal 0.591 delta/R, the silhouette the analytic one; 16^3: 0.463 delta^2/R, 0.639 delta/R, 8 silhouette
    pixels differ, all within 0.037 delta of tangency.  No ray runs out of steps (at most 66 samples)."""
    H, W = 48, 64
    delta = VC.sphere_table(n)[3]
    cam, _ = VC.sphere_camera(H, W)
    t, inst, normal, steps = (x[0] for x in VC.sphere_render(n, H, W))
    hit_a, t_a, n_a, cos, closest = VC.sphere_analytic(cam[0], H, W)
    hit = inst == 0
    assert hit_a.sum() > 250 and steps.max() < 256 + 1 and np.array_equal(hit, np.isfinite(t))
    off = hit != hit_a
    print(f"n={n}: silhouette mismatches {int(off.sum())}, farthest from tangency {np.abs(closest - VC.SPHERE_R)[off].max(initial=0.0) / delta:.3f} delta")
    assert (np.abs(closest - VC.SPHERE_R)[off] <= 0.5 * delta).all()
    both = hit & hit_a & (cos >= 0.5)
    assert both.sum() > 200
    err_t = np.abs(t[both] - t_a[both]).max()
    angle = np.arccos(np.clip((normal * n_a).sum(-1), -1.0, 1.0))[both].max()
    print(f"n={n}: depth error {err_t / (delta * delta / VC.SPHERE_R):.3f} delta^2/R, normal error {angle / (delta / VC.SPHERE_R):.3f} delta/R, "
          f"most samples {int(steps.max())}")
    assert err_t <= delta * delta / VC.SPHERE_R
    assert angle <= delta / VC.SPHERE_R
    assert np.abs(np.linalg.norm(normal[hit], axis=-1) - 1.0).max() < 1e-12 and (normal[~hit] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the route it stands beside: surface nets and the triangle camera
# ---------------------------------------------------------------------------------------------------------------------
def test_against_surface_nets_and_the_triangle_camera():
    """scenes.surface_nets plus camera.render_depth on the 16^3 sphere at 24 x 32 (f = 30): a surface-nets vertex lies inside a
    crossing cell, hence within sqrt(3) delta of the level set, over the cosine (>= 0.5): 2 sqrt(3) delta.  Measured: 0.131 delta on
    the 60 pixels hit by both."""
    from omg_planner_amd import camera, scenes as sc
    H, W, n = 24, 32, 16
    objects, begin, pool, delta = VC.sphere_table(n)
    cam, cfw = VC.sphere_camera(H, W)
    t, inst, _, _ = VC.sphere_render(n, H, W)
    verts, faces, _ = sc.surface_nets(pool.reshape(n, n, n), objects[0]["lo"].astype(np.float64), float(objects[0]["delta"]), "centre", 0.0)
    records = camera.instance_records([(verts, faces)], [0], [np.eye(4)], [0], cfw)
    t_mesh, inst_mesh, _ = camera.render_depth([(verts, faces)], records, [0, 1], cam, H, W)
    _, _, _, cos, _ = VC.sphere_analytic(cam[0], H, W)
    both = (inst[0] == 0) & (inst_mesh[0] == 0) & (cos >= 0.5)
    assert both.sum() > 50
    worst = np.abs(t[0][both] - t_mesh[0][both]).max()
    print(f"largest difference to the mesh route {worst / delta:.3f} delta on {int(both.sum())} pixels")
    assert worst <= 2.0 * np.sqrt(3.0) * delta


# ---------------------------------------------------------------------------------------------------------------------
# 5. refused arguments
# ---------------------------------------------------------------------------------------------------------------------
def _good():
    objects, begin, pool, cameras, visible, _ = VC.edge_batch([1, 14])  # one object; two objects
    return dict(objects=objects, scene_begin=begin, pool=pool, cameras=cameras, H=2, W=3, visible=None, level=0.0, t_min=0.0, min_step=0.25,
                relax=1.0, max_steps=8)


def _bad_cases():
    """(what, the change of _good()): every argument error of the specification."""
    g = _good()
    rec = lambda **kw: _changed(g["objects"], 1, **kw)
    cam = lambda k, x: _with(g["cameras"], (1, k), x)
    return [("level", dict(level=np.nan)), ("t_min", dict(t_min=INF)), ("min_step", dict(min_step=np.nan)), ("relax", dict(relax=-INF)),
            ("t_min < 0", dict(t_min=-1e-9)), ("min_step <= 0", dict(min_step=0.0)), ("relax 0", dict(relax=0.0)), ("relax > 1", dict(relax=1.0 + 2.0 ** -52)),
            ("max_steps 0", dict(max_steps=0)), ("max_steps too large", dict(max_steps=4097)),
            ("dim < 2", dict(objects=rec(dim=(3, 1, 5)))), ("inv_delta zero", dict(objects=rec(inv_delta=0.0))),
            ("inv_delta negative", dict(objects=rec(inv_delta=-1.0))), ("inv_delta NaN", dict(objects=rec(inv_delta=np.nan))),
            ("inv_delta inf", dict(objects=rec(inv_delta=INF))), ("grid before the pool", dict(objects=rec(grid_offset=-1))),
            ("grid behind the pool", dict(objects=rec(grid_offset=len(g["pool"]) - 44))),
            ("scene_begin descending", dict(scene_begin=np.array([0, 2, 1], np.int32))), ("scene_begin negative", dict(scene_begin=np.array([-1, 1, 3], np.int32))),
            ("scene_begin behind the records", dict(scene_begin=np.array([0, 1, 4], np.int32))),
            ("camera NaN", dict(cameras=cam(9, np.nan))), ("camera inf", dict(cameras=cam(2, INF))), ("fx zero", dict(cameras=cam(0, 0.0))),
            ("fy zero", dict(cameras=cam(1, 0.0)))]


def _with(a, at, x):
    a = np.array(a, copy=True)
    a[at] = x
    return a


def _changed(objects, k, **fields):
    objects = objects.copy()
    for name, x in fields.items():
        objects[name][k] = x
    return objects


def test_specification_argument_errors():
    from omg_planner_amd import volume_camera as vc
    g = _good()
    vc.render_volumes(**g)
    for what, change in _bad_cases():
        with pytest.raises(ValueError):
            vc.render_volumes(**{**g, **change})
            pytest.fail(what)
    # an invisible object is not looked at; one outside every scene is not either
    bad = _changed(g["objects"], 1, dim=(3, 1, 5))
    vc.render_volumes(**{**g, "objects": bad, "visible": np.array([1, 0, 1], np.uint8)})
    vc.render_volumes(**{**g, "objects": bad, "scene_begin": np.array([0, 1, 1], np.int32)})
    for change in (dict(visible=np.ones(2, np.uint8)), dict(pool=g["pool"].astype(np.float64)), dict(H=0), dict(cameras=g["cameras"][:1]),
                   dict(objects=np.zeros(3))):
        with pytest.raises(ValueError):
            vc.render_volumes(**{**g, **change})


def test_c_abi_argument_checks_without_gpu():
    """Every OMGX_ERR_INVALID / OMGX_ERR_UNSUPPORTED case is decided on the host copies before any HIP call: the library loads
    without a GPU, and no device pointer below can be dereferenced."""
    from omg_planner_amd import _lib
    lib, vp, d = _lib.lib(), C.c_void_p, C.c_void_p(4096)
    g = _good()
    assert _lib.VOLUME_CAMERA_MAX_STEPS == 4096 and _lib.ABI_VERSION == 14

    def call(null=(), H=2, W=3, num_objects=None, num_scenes=None, pool_elems=None, h_visible=None, visible=None, **change):
        a = {**g, **change}
        objects, begin = np.ascontiguousarray(a["objects"]), np.ascontiguousarray(a["scene_begin"], np.int32)
        cameras = np.ascontiguousarray(a["cameras"], np.float64)
        p = dict(objects=d, h_objects=vp(objects.ctypes.data), scene_begin=d, h_scene_begin=vp(begin.ctypes.data), pool=d, cameras=d,
                 h_cameras=vp(cameras.ctypes.data), t_out=d, inst_out=d, normal_out=d, steps_out=d)
        p.update({k: None for k in null})
        hv = None if h_visible is None else vp(h_visible.ctypes.data)
        return lib.omgx_render_volumes(p["objects"], p["h_objects"], len(objects) if num_objects is None else num_objects, p["scene_begin"],
                                       p["h_scene_begin"], len(begin) - 1 if num_scenes is None else num_scenes, p["pool"],
                                       len(a["pool"]) if pool_elems is None else pool_elems, p["cameras"], p["h_cameras"], visible, hv, H, W,
                                       a["level"], a["t_min"], a["min_step"], a["relax"], a["max_steps"], p["t_out"], p["inst_out"], p["normal_out"],
                                       p["steps_out"], None)
    INVALID, UNSUPPORTED = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED
    for what, change in _bad_cases():
        assert call(**change) == INVALID, what
    for name in ("objects", "h_objects", "scene_begin", "h_scene_begin", "pool", "cameras", "h_cameras", "t_out", "inst_out"):
        assert call(null=(name,)) == INVALID, name
    flags = np.ones(3, np.uint8)
    assert call(h_visible=flags) == INVALID and call(visible=d) == INVALID  # both or neither
    assert call(H=0) == INVALID and call(W=0) == INVALID and call(num_objects=-1) == INVALID and call(num_scenes=-1) == INVALID
    assert call(pool_elems=-1) == INVALID and call(pool_elems=len(g["pool"]) - 4) == INVALID
    # legal without a launch: no scenes (nothing per scene is read), also with every pointer NULL
    assert call(num_scenes=0) == _lib.OMGX_OK
    assert lib.omgx_render_volumes(None, None, 0, None, None, 0, None, 0, None, None, None, None, 1, 1, 0.0, 0.0, 0.25, 1.0, 1, None, None, None, None,
                                   None) == _lib.OMGX_OK
    # an invalid argument is reported before an unsupported size
    many = 65536
    begin, cams = np.zeros(many + 1, np.int32), np.tile(g["cameras"][:1], (many, 1))
    assert call(scene_begin=begin, cameras=cams) == UNSUPPORTED
    assert call(scene_begin=begin, cameras=cams, relax=2.0) == INVALID
    assert call(H=16 * 4096, W=16 * 2048 + 1) == UNSUPPORTED and call(H=16 * 4096, W=16 * 2048 + 1, max_steps=0) == INVALID


def _stub_table(objects, begin, pool):
    import torch
    return types.SimpleNamespace(host_objects=np.ascontiguousarray(objects), host_scene_begin=np.ascontiguousarray(begin, np.int32),
                                 num_scenes=len(begin) - 1, pool=torch.from_numpy(np.ascontiguousarray(pool, np.float32)), device=torch.device("cpu"))


def test_wrapper_argument_errors_before_any_launch():
    """ops.render_volumes raises the specification's errors as OmgHipError from the table's host mirror before it touches the
    device: a stand-in table without a device is enough to see every one of them; so do VolumeCameraBatch's own."""
    pytest.importorskip("torch")
    from omg_planner_amd import _lib, ops
    g = _good()
    for what, change in _bad_cases():
        a = {**g, **change}
        with pytest.raises(_lib.OmgHipError):
            ops.render_volumes(_stub_table(a["objects"], a["scene_begin"], a["pool"]), a["cameras"], 2, 3, level=a["level"], t_min=a["t_min"],
                               min_step=a["min_step"], relax=a["relax"], max_steps=a["max_steps"])
            pytest.fail(what)
    table = _stub_table(g["objects"], g["scene_begin"], g["pool"])
    for kw in (dict(H=0, W=3), dict(H=2, W=-1), dict(H=2, W=3, visible=np.ones(2, np.uint8)), dict(H=2, W=3, out=(None, None, None, None))):
        with pytest.raises(_lib.OmgHipError):
            ops.render_volumes(table, g["cameras"], **kw)
    for cameras, labels in ((g["cameras"][:1], [0, 1, 1]), (_with(g["cameras"], (0, 0), 0.0), [0, 1, 1]), (g["cameras"], [0, 1]), (g["cameras"], [0, -1, 1])):
        with pytest.raises(_lib.OmgHipError):
            ops.VolumeCameraBatch(table, cameras, labels)


# ---------------------------------------------------------------------------------------------------------------------
# 6. what the compiler made of the kernel
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_kernel_uses_no_scratch(tmp_path):
    seen = KB.kernel_resources("omg_volume_camera.hip", tmp_path)
    v = KB.one(seen, "k_render_volumes")
    print(f"k_render_volumes: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, {v['Occupancy [waves/SIMD]']} waves per SIMD")
    assert len(seen) == 1 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["LDS Size [bytes/block]"] == 0
