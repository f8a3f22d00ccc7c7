"""tests/kernel_build.py itself: the device flags are the Makefile's, the resource reader and its selectors say what they found,
the host harness builds and runs, and a compile that fails says why."""
import ctypes as C
import subprocess

import pytest

from tests import kernel_build as KB


def test_device_flags_are_the_makefiles():
    flags = KB.device_flags()
    assert flags[-1] == "--cuda-device-only" and flags[-3].startswith("-I") and flags[-2].startswith("-I")
    assert flags[0].endswith("-arch=gfx950") and "-ffp-contract=off" in flags  # the target first, as on the Makefile's line
    dry = subprocess.run(["make", "-n", "-B", "-C", str(KB.CSRC), "build/omg_goal_select.o"], check=True, stdout=subprocess.PIPE, text=True).stdout
    line = next(ln for ln in dry.splitlines() if "omg_goal_select.hip" in ln).split()
    assert sorted(line[1:]) == sorted(flags[:-3] + ["-c", "omg_goal_select.hip", "-o", "build/omg_goal_select.o"])  # line[0]: the compiler


@KB.requires_hipcc
def test_kernel_resources_and_selectors(tmp_path):
    res = KB.kernel_resources("omg_goal_select.hip", tmp_path)
    v = KB.one(res, "k_select_goals")
    assert set(v) == set(KB.FIELDS) and len(KB.FIELDS) == 8 and all(type(x) is int for x in v.values())
    assert KB.matching(res, "k_select_goals") == {n: v for n in res if "k_select_goals" in n}
    for select in (KB.one, KB.matching):
        with pytest.raises(LookupError, match="k_select_goals"):
            select(res, "k_no_such_kernel")
    two = {"_Z3k_aPf": v, "_Z3k_bPf": v}
    assert KB.matching(two, "k_") == two and KB.one(two, "_Z3k_bPf") is v
    with pytest.raises(LookupError, match="2 kernels.*k_a.*k_b"):
        KB.one(two, "k_")


@KB.requires_host_cxx
def test_host_harness_builds_and_runs(tmp_path):
    lib = KB.host_harness('extern "C" double twice(double x) {\n    return 2.0 * x;\n}\n', tmp_path, {"twice": (C.c_double, [C.c_double])})
    assert lib.twice(1.25) == 2.5


@KB.requires_hipcc
@KB.requires_host_cxx
def test_a_failed_compile_says_why(tmp_path):
    with pytest.raises(RuntimeError, match="no_such_type_host"):
        KB.host_harness('extern "C" no_such_type_host f();\n', tmp_path)
    bad = tmp_path / "bad.hip"
    bad.write_text("__global__ void k_bad(no_such_type_device* p) {}\n")
    with pytest.raises(RuntimeError, match="no_such_type_device"):
        KB.kernel_resources(bad, tmp_path)
