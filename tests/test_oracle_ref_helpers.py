"""CPU test: the oracle's trilinear value / central-difference gradient against THE REFERENCE'S OWN helpers —
layers/sdf_matching_loss_kernel.cu:15-86 (lerp, getValue, getValueInterpolated, getGradientInterpolated), compiled for the
host from the reference tree by `make -C oracle ref` into oracle/_ref/ (two builds: without and with FMA contraction).  What those
builds return on this module's seeded inputs is stored in tests/golden/ref_helpers.npz (`PYTHONPATH=. python tests/test_oracle_ref_helpers.py`
records it from oracle/_ref): the oracle is checked against the stored outputs, and wherever oracle/_ref is built the live helpers
must reproduce them bit for bit.

This pins the numerically delicate part of the SDF op (the -0.5 voxel-centre shift in double, truncation toward zero,
out-of-range 1.0, one-voxel central differences divided by delta in double).  The kernel body (.cu:96-195: pose transform,
hinge, rotate-back, reduction) is pinned by tests/test_oracle_ref_body.py, which runs the body's own text on the host."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as orc

REF_DIR = Path(__file__).resolve().parents[1] / "oracle" / "_ref"
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_helpers.npz"
BUILDS = {"libsdf_ref_helpers_fma.so": "fma", "libsdf_ref_helpers.so": "plain"}


def _load(name):
    """The reference's helpers built into oracle/_ref, or None where they are not built (no reference tree)."""
    p = REF_DIR / name
    if not p.exists():
        return None
    lib = C.CDLL(str(p))
    lib.ref_value_interpolated.restype = C.c_float
    lib.ref_value_interpolated.argtypes = [C.c_float] * 3 + [C.c_int] * 3 + [C.c_void_p]
    lib.ref_gradient_interpolated.restype = None
    lib.ref_gradient_interpolated.argtypes = [C.c_float] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_float, C.c_void_p]
    return lib


def _cases(rng, dims, n):
    d = np.array(dims, np.float32)
    g = rng.uniform(-2.5, 1.0, size=(n, 3)).astype(np.float32) + rng.uniform(0, 1, size=(n, 3)).astype(np.float32) * (d + 3.0)
    edge = np.array([[0.2, 3, 3], [-0.2, 3, 3], [-0.6, 3, 3], [0.5, 0.5, 0.5], [1.5, 1.5, 1.5], [d[0] - 0.5, 3, 3], [d[0] - 0.51, 3, 3],
                     [d[0] - 1.5, 3, 3], [3, d[1] - 0.49, 3], [3, 3, d[2] + 5], [1e9, 0, 0], [-1e9, 0, 0], [2.5, 2.5, 2.5]], np.float32)
    return np.concatenate([edge, g])


def _inputs():
    """(dims, delta, grid, query points) of the three seeded volumes."""
    rng = np.random.RandomState(0)
    for dims, delta in (((9, 7, 11), 0.05), ((16, 16, 16), 0.03125), ((5, 24, 6), 0.0117)):
        grid = rng.normal(0.05, 0.1, size=dims).astype(np.float32)
        yield dims, delta, grid, _cases(rng, dims, 4000)


def _evaluate(lib, prefix, dims, delta, grid, cases):
    """-> values [N] float32, gradients [N,3] float32 of `prefix`_value_interpolated / `prefix`_gradient_interpolated."""
    value, gradient = getattr(lib, f"{prefix}_value_interpolated"), getattr(lib, f"{prefix}_gradient_interpolated")
    gp = grid.ctypes.data_as(C.c_void_p)
    vals, grads = np.zeros(len(cases), np.float32), np.zeros((len(cases), 3), np.float32)
    for k, (gx, gy, gz) in enumerate(cases):
        vals[k] = value(gx, gy, gz, *dims, gp)
        gradient(gx, gy, gz, *dims, gp, delta, grads[k].ctypes.data_as(C.c_void_p))
    return vals, grads


@pytest.mark.parametrize("build,tol_ulps", [("libsdf_ref_helpers_fma.so", 0), ("libsdf_ref_helpers.so", 4)])
def test_value_and_gradient_match_the_reference_helpers(build, tol_ulps):
    ref = _load(build)
    fx = np.load(GOLDEN)
    key = BUILDS[build]
    o = orc.lib()
    o.orc_value_interpolated.restype = C.c_float
    o.orc_value_interpolated.argtypes = [C.c_float] * 3 + [C.c_int] * 3 + [C.c_void_p]
    o.orc_gradient_interpolated.restype = None
    o.orc_gradient_interpolated.argtypes = [C.c_float] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_float, C.c_void_p]
    worst_v = worst_g = 0
    for i, (dims, delta, grid, cases) in enumerate(_inputs()):
        assert np.array_equal(cases, fx[f"cases{i}"]) and np.array_equal(grid, fx[f"grid{i}"])  # the inputs the outputs belong to
        va, a3 = fx[f"{key}_value{i}"], fx[f"{key}_gradient{i}"]
        if ref is not None:  # the reference's helpers, live: the stored outputs are theirs
            lv, lg = _evaluate(ref, "ref", dims, delta, grid, cases)
            assert np.array_equal(lv.view(np.int32), va.view(np.int32)) and np.array_equal(lg.view(np.int32), a3.view(np.int32))
        vb, b3 = _evaluate(o, "orc", dims, delta, grid, cases)
        if tol_ulps == 0:
            bad = np.flatnonzero((va.view(np.int32) != vb.view(np.int32)) | (a3.view(np.int32) != b3.view(np.int32)).any(1))
            assert len(bad) == 0, (cases[bad[:3]], va[bad[:3]], vb[bad[:3]], a3[bad[:3]], b3[bad[:3]])
        else:  # without contraction lerp rounds twice: a few ulps of the value scale
            worst_v = max(worst_v, float(np.abs(va - vb).max()))
            worst_g = max(worst_g, float(np.abs(a3 - b3).max()))
    if tol_ulps:
        assert worst_v < 1e-7 and worst_g < 1e-4  # 1e-7 on values ~0.1; gradients are differences / delta (~1e-2)


if __name__ == "__main__":  # record tests/golden/ref_helpers.npz from the builds in oracle/_ref (`make -C oracle ref`)
    out = {}
    for build, key in BUILDS.items():
        lib = _load(build)
        if lib is None:
            raise SystemExit(f"{REF_DIR / build} is not built: `make -C oracle ref` needs the reference tree")
        for i, (dims, delta, grid, cases) in enumerate(_inputs()):
            out[f"cases{i}"], out[f"grid{i}"] = cases, grid
            out[f"{key}_value{i}"], out[f"{key}_gradient{i}"] = _evaluate(lib, "ref", dims, delta, grid, cases)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, sorted(out))
