"""CPU test: libomg_hip.so loads without a GPU and exports every function include/omg_hip.h declares
(no compute calls), the POD structs have the sizes the header documents, and the bindings the package derives from the header
(_header.parse) are what the C compiler reads there."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _declared_functions():
    text = (ROOT / "include" / "omg_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(omgx_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from omg_planner_amd import _lib
    names = _declared_functions()
    assert len(names) >= 12 and "omgx_sdf_loss_forward" in names
    lib = _lib.lib()
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert sorted(_lib.EXPORTS) == names  # the loader's list is the header's list
    assert sorted(_lib.FUNCTIONS) == names and len(names) == len(set(_lib.EXPORTS))  # every prototype is bound, none twice
    unbound = [n for n in names if getattr(lib, n).argtypes is None or getattr(lib, n).restype is not _lib.FUNCTIONS[n][0]]
    assert not unbound, unbound  # ctypes checks every call: no entry point is left without argtypes
    assert lib.omgx_abi_version() >= 1


def test_struct_layouts_match_header():
    from omg_planner_amd import _lib, scenes
    assert scenes.OBJECT_DTYPE.itemsize == 184
    assert scenes.OBJECT_DTYPE.fields["grid_offset"][1] == 104 and scenes.OBJECT_DTYPE.fields["inv_extent"][1] == 112
    assert C.sizeof(_lib.ChompParams) == 12 * 4 + 6 * 8 + 9 * 8 + 3 * 8   # ABI 7: three optional pose pointers at the end
    assert C.sizeof(_lib.LearnerParams) == 8 * 4 + 3 * 8 + 2 * 8          # ABI 7: goal pose table, end poses out
    from oracle import oracle as orc
    assert orc.lib().orc_sizeof_object() == 184 and orc.lib().orc_sizeof_params() == C.sizeof(_lib.ChompParams)


def test_workspace_and_aux_sizes_without_gpu():
    from omg_planner_amd import _lib
    lib = _lib.lib()
    assert lib.omgx_chomp_aux_doubles(30) == 30 * 9 + 30 * 10 + 30 * 9 + 31
    # ABI 10: the kinematics pre-pass's scratch — per goal 10 links x 9 doubles x (n + 1) configurations + 10 x n mask words
    assert lib.omgx_goalset_workspace_bytes(100, 64, 30, 15) == 100 * 64 * (90 * 31 * 8 + 300 * 4)
    assert lib.omgx_goalset_workspace_bytes(1, 1, 1, 15) == 1488 and lib.omgx_goalset_workspace_bytes(0, 64, 30, 15) == 0
    assert lib.omgx_fk_sdf_workspace_bytes(100, 30, 15) >= 100 * 10 * 32 * 12 * 8
    assert lib.omgx_fk_sdf_workspace_bytes(0, 30, 15) == 0


def test_robot_blob_layout():
    from omg_planner_amd import robot as rb
    m = rb.PandaModel(seed=0)
    b = m.blob()
    P = m.points_per_link
    assert b.size == 528 + 30 * P + 356 + 30 * P
    np.testing.assert_array_equal(b[:160].reshape(10, 4, 4), m.pose_0)
    np.testing.assert_array_equal(b[528:528 + 30 * P].reshape(10, P, 3), m.collision_points)
    # derived joint-0 matrices reproduce pose_0[0] @ Rz(q) @ Rx(0)
    D = 528 + 30 * P
    U, V, W = b[D:D + 9].reshape(3, 3), b[D + 9:D + 18].reshape(3, 3), b[D + 18:D + 27].reshape(3, 3)
    q = 0.37
    Rz = np.array([[np.cos(q), -np.sin(q), 0], [np.sin(q), np.cos(q), 0], [0, 0, 1]])
    np.testing.assert_allclose(np.cos(q) * U + np.sin(q) * V + W, m.pose_0[0][:3, :3] @ Rz, atol=1e-15)


def test_goalset_parts_and_tiled_argument_checks_without_gpu():
    """Host logic of the latency-mode launch (no GPU needed: argument errors are reported before anything is launched).
    omgx_goalset_parts: the largest power of two <= goal_parts that leaves every workgroup at least 4 of the window's
    ceil(n / 4) x 5 tiles."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    want = {(30, 4): 4, (30, 8): 8, (30, 1): 1, (30, 2): 2, (12, 8): 2, (13, 4): 4, (8, 4): 2, (5, 8): 2, (4, 8): 1, (1, 8): 1, (64, 8): 8}
    for (n, p), np_ in want.items():
        assert lib.omgx_goalset_parts(n, p) == np_, (n, p)
        tiles = ((n + 3) // 4) * 5
        assert np_ == 1 or tiles // np_ >= 4
    assert lib.omgx_goalset_parts(0, 4) == 0 and lib.omgx_goalset_parts(30, 0) == 0 and lib.omgx_goalset_parts(30, 9) == 0
    d = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first

    def call(goal_parts=4, lg=10, cb=4, spread=1, goals=d, traj=d, G=64, n_rem=30):
        return lib.omgx_goalset_cost_layer_tiled(d, 15, d, d, d, d, 270, goals, 1, G, n_rem, 0.1, 0, d, d, traj, 30, 0, d, d, d, None, None,
                                                 goal_parts, lg, cb, spread, None, None, None)
    assert call(goal_parts=0) == _lib.OMGX_ERR_INVALID and call(goal_parts=9) == _lib.OMGX_ERR_INVALID
    assert call(lg=3) == _lib.OMGX_ERR_INVALID and call(lg=11) == _lib.OMGX_ERR_INVALID and call(cb=-1) == _lib.OMGX_ERR_INVALID
    # (goal_parts > 1 without `spread` is the batch kernel with split goals since ABI 8: omgx_goalset_cost_layer_parts)

    def parts(goal_parts=2, traj=d, sched=None, slen=0):
        return lib.omgx_goalset_cost_layer_parts(d, 15, d, d, d, d, 270, d, 1, 64, 30, 0.1, 0, d, d, traj, 30, 0, d, d, d, None, None,
                                                 sched, slen, None, goal_parts, None, None, None)
    assert parts(traj=None) == _lib.OMGX_ERR_INVALID and parts(goal_parts=0) == _lib.OMGX_ERR_INVALID and parts(goal_parts=16) == _lib.OMGX_ERR_INVALID
    assert parts(sched=d, slen=12) == _lib.OMGX_ERR_INVALID  # a schedule's length is a multiple of 8
    assert lib.omgx_goalset_schedule_parts(None, None, None, 4, 64, 3, 2, d, None) == _lib.OMGX_ERR_INVALID
    assert lib.omgx_goalset_schedule_parts(None, None, None, 4, 64, 2, 2, None, None) == _lib.OMGX_ERR_INVALID
    assert lib.omgx_goalset_schedule_ordered(None, None, None, 4, 64, 1, 2, 2, d, None) == _lib.OMGX_ERR_INVALID  # no such order
    assert lib.omgx_goalset_schedule_ordered(None, None, None, 4, 64, 3, 2, 1, d, None) == _lib.OMGX_ERR_INVALID
    assert call(goals=None, traj=None, G=0) == _lib.OMGX_ERR_INVALID
    assert call(goals=None) == _lib.OMGX_ERR_INVALID
    assert call(n_rem=0) == _lib.OMGX_ERR_UNSUPPORTED and call(n_rem=65) == _lib.OMGX_ERR_UNSUPPORTED
    assert lib.omgx_pose_table(None, 15, d, 4, d, None) == _lib.OMGX_ERR_INVALID and lib.omgx_pose_table(d, 15, d, 0, d, None) == _lib.OMGX_OK
    assert lib.omgx_pose_table(d, 99, d, 4, d, None) == _lib.OMGX_ERR_UNSUPPORTED and lib.omgx_pose_table(d, 15, d, -1, d, None) == _lib.OMGX_ERR_INVALID


def _c_compiler():
    for cc in (os.environ.get("CC"), "cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang"):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    raise RuntimeError("no C compiler (the oracle needs one too)")


def test_header_reader_agrees_with_the_compiler(tmp_path):
    """The independent check of _header.parse: a C program generated from the PARSED names includes omg_hip.h and prints what the
    compiler makes of it — every #define's value, every struct's sizeof and every field's offsetof and size — and all of it
    equals the constants and the ctypes structs the package works with."""
    from omg_planner_amd import _lib
    assert len(_lib.STRUCTS) == 8 and len(_lib.CONSTANTS) >= 50
    lines = [f'printf("{n} %lld\\n", (long long)({n}));' for n in _lib.CONSTANTS]
    for sname, st in _lib.STRUCTS.items():
        lines.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        lines += [f'printf("{sname}.{f} %zu %zu\\n", offsetof({sname}, {f}), sizeof((({sname}*)0)->{f}));' for f, _ in st._fields_]
    (tmp_path / "abi.c").write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"omg_hip.h\"\nint main(void) {\n" + "\n".join(lines)
                                    + "\nreturn 0;\n}\n")
    subprocess.run([_c_compiler(), "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")], check=True)
    out = subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = {row.split()[0]: tuple(int(v) for v in row.split()[1:]) for row in out if row}
    want = {n: (v,) for n, v in _lib.CONSTANTS.items()}
    for sname, st in _lib.STRUCTS.items():
        want[sname] = (C.sizeof(st),)
        want.update({f"{sname}.{f}": (getattr(st, f).offset, getattr(st, f).size) for f, _ in st._fields_})
    assert seen == want
    # the names the package exposes are those values
    assert (_lib.NUM_DOF, _lib.INFO_STRIDE, _lib.SCHEDULE_MAX_SCENES, _lib.SELECT_MAX_GOALS) == (
        seen["OMGX_NUM_DOF"][0], seen["OMGX_INFO_STRIDE"][0], seen["OMGX_SCHEDULE_MAX_SCENES"][0], seen["OMGX_SELECT_MAX_GOALS"][0])
    assert (_lib.OMGX_OK, _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_LAUNCH, _lib.OMGX_ERR_UNSUPPORTED) == (0, -1, -2, -3)
    assert (_lib.SCHEDULE_SCENE_MAJOR, _lib.SCHEDULE_LONGEST_FIRST, _lib.SCHEDULE_LONGEST_FIRST_MAX_ITEMS) == (0, 1, 8192)
    assert (_lib.MESH_SDF_NODES_PER_WORKGROUP, _lib.RAYCAST_RAYS_PER_WORKGROUP, _lib.RAYCAST_MAX_CHUNKS, _lib.CAMERA_PIXELS_PER_WORKGROUP) == (
        256, 256, 64, 256)
    assert _lib.ALG == {"FTL": 0, "FTC": 1, "Exp": 2, "MD": 3, "Proj": 4} and _lib.ABI_VERSION == 14
    # sizes the header documents, and the numpy records are the same structs
    sizes = {n: C.sizeof(st) for n, st in _lib.STRUCTS.items()}
    assert sizes == {"omgx_object": 184, "omgx_chomp_params": 192, "omgx_learner_params": 72, "omgx_plan_iter": 40, "omgx_mesh": 88,
                     "omgx_ray_work": 24, "omgx_camera": 136, "omgx_instance": 136}
    assert _lib.Mesh.dims.offset == 56 and _lib.Mesh.first_workgroup.offset == 48
    from omg_planner_amd import camera, scenes
    for dt, st in ((scenes.OBJECT_DTYPE, _lib.Object), (camera.CAMERA_DTYPE, _lib.Camera), (camera.INSTANCE_DTYPE, _lib.Instance)):
        assert dt.itemsize == C.sizeof(st) and list(dt.names) == [f for f, _ in st._fields_]
        assert all(dt.fields[f][1] == getattr(st, f).offset and dt.fields[f][0].itemsize == getattr(st, f).size for f in dt.names)
        assert np.zeros(2, dt).dtype == dt == np.dtype([(f, dt.fields[f][0].base, dt.fields[f][0].shape) for f in dt.names], align=True)


def test_signatures_pinned_literally():
    """A few signatures written out, so that a change of the type mapping cannot pass unnoticed."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    vp, i32, i64, f64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_float
    parts = lib.omgx_goalset_cost_layer_parts.argtypes
    assert list(parts) == [vp, i32, vp, vp, vp, vp, i64, vp, i32, i32, i32, f64, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp,
                           i32, vp, vp, vp] and len(parts) == 30
    assert [k for k, t in enumerate(parts) if t is i64] == [6] and [k for k, t in enumerate(parts) if t is f64] == [11]
    assert [k for k, t in enumerate(parts) if t is i32] == [1, 8, 9, 10, 12, 16, 17, 24, 26]
    lp, cp, it = C.POINTER(_lib.LearnerParams), C.POINTER(_lib.ChompParams), C.POINTER(_lib.PlanIter)
    plan = lib.omgx_plan_persistent.argtypes
    assert list(plan) == ([vp, i32, vp, vp, vp, vp, i32, i32, f64, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp] + [lp] + [vp] * 6 +
                          [cp] + [vp] * 7 + [it, vp, i32, vp, i64, i32, i32, vp]) and len(plan) == 44
    assert (plan[21], plan[28], plan[36]) == (lp, cp, it) and plan[37] is vp  # h_iters by reference, d_iters device memory
    assert list(lib.omgx_pixel_gather.argtypes) == [vp, i32, vp, i32, i32, i32, vp, vp, i32, vp, vp, i64, vp]
    assert list(lib.omgx_object_set_grid.argtypes) == [vp, vp, vp, vp, f32, i64, vp]
    assert list(lib.omgx_chomp_optimize.argtypes) == [vp, cp] + [vp] * 9 + [i32] + [vp] * 4 + [i32, vp]
    assert list(lib.omgx_device_arch.argtypes) == [C.c_char_p, i32] and lib.omgx_last_error.restype is C.c_char_p
    for name in ("omgx_abi_version", "omgx_device_cu_count", "omgx_last_error", "omgx_mesh_sdf_tile"):
        assert list(getattr(lib, name).argtypes) == []
    assert lib.omgx_goalset_workspace_bytes.restype is i64 and lib.omgx_mesh_sdf_tile.restype is i32 and lib.omgx_mesh_sdf.restype is C.c_int
    with pytest.raises(C.ArgumentError):  # a device pointer in an int32 slot is now an error, not a wild access
        lib.omgx_pose_table(vp(4096), vp(4096), vp(4096), 0, vp(4096), None)


_GOOD = """/* a header
 * of three lines */
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define OMGX_N 3
#define OMGX_M (1 << OMGX_N)   /* 8 */
typedef struct omgx_rec {
    float a[OMGX_N];      /* comment */
    int32_t b, c;
    const double* p;
    double d[OMGX_M + 1];
} omgx_rec; /* sizeof == 96 */
%s
int64_t omgx_bytes(int32_t n);
int omgx_run(const omgx_rec* h_rec, omgx_rec* recs, const float* x /* [n] */,
             float y, void* stream);
const char* omgx_text(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_reads_the_forms_the_header_uses():
    from omg_planner_amd import _header
    consts, structs, funcs = _header.parse(_GOOD % "")
    assert consts == {"OMGX_N": 3, "OMGX_M": 8}
    rec = structs["omgx_rec"]
    assert [(f, getattr(rec, f).offset, getattr(rec, f).size) for f, _ in rec._fields_] == [
        ("a", 0, 12), ("b", 12, 4), ("c", 16, 4), ("p", 24, 8), ("d", 32, 72)] and C.sizeof(rec) == 104
    assert list(funcs) == ["omgx_bytes", "omgx_run", "omgx_text"]
    assert funcs["omgx_bytes"] == (C.c_int64, [C.c_int32]) and funcs["omgx_text"] == (C.c_char_p, [])
    assert funcs["omgx_run"][0] is C.c_int and funcs["omgx_run"][1][1:] == [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    assert funcs["omgx_run"][1][0]._type_ is rec or funcs["omgx_run"][1][0] is C.c_void_p  # only the package's parameter blocks are typed


@pytest.mark.parametrize("what, text", [
    ("an unknown type", "int omgx_f(size_t n);"),
    ("an unknown type in a struct", "typedef struct omgx_s { int32_t n; long m; } omgx_s;"),
    ("a function-pointer argument", "int omgx_f(int32_t n, void (*done)(int32_t), void* stream);"),
    ("a nested struct", "typedef struct omgx_s { int32_t n; struct { double x; } in; } omgx_s;"),
    ("a struct held by value", "typedef struct omgx_s { omgx_rec r; } omgx_s;"),
    ("a prototype returning a struct", "omgx_rec omgx_f(int32_t n);"),
    ("a prototype returning a pointer", "float* omgx_f(int32_t n);"),
    ("a stray declaration", "extern int32_t omgx_counter;"),
    ("a function outside the omgx_ names", "int helper(int32_t n);"),
    ("a pointer to a pointer", "int omgx_f(double** rows);"),
    ("an array argument", "int omgx_f(double rows[3]);"),
    ("a macro with arguments", "#define OMGX_MAX(a, b) ((a) > (b) ? (a) : (b))"),
    ("a #define that is no integer", "#define OMGX_EPS 1e-6"),
    ("a #define of an unknown name", "#define OMGX_K (OMGX_UNKNOWN + 1)"),
    ("a declaration without its end", "int omgx_f(int32_t n)"),
])
def test_reader_refuses_what_it_does_not_understand(what, text):
    """Nothing is skipped: every line that is neither a #define, a struct of scalars, a prototype nor the bracket raises, and the
    error names the line (17 in _GOOD) and quotes it."""
    from omg_planner_amd import _header
    with pytest.raises(_header.HeaderError) as err:
        _header.parse(_GOOD % text)
    assert "line 17:" in str(err.value) and text.split(";")[0][:24] in str(err.value), (what, str(err.value))
