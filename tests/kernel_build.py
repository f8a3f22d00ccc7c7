"""What the CPU tests of an op build without a GPU, in one place: the kernel body header compiled for the host (host_harness) and
the compiler's resource figures of a .hip file compiled for the device exactly as the product's objects are (kernel_resources,
with the selectors one / matching).  The device flags come from csrc/Makefile's `flags` target, not from a copy of them."""
from __future__ import annotations

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "omg-planner_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")  # every integer the kernel-resource-usage remark prints


def host_compiler():
    for cxx in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("c++"), shutil.which("g++")):
        if cxx and Path(cxx).exists():
            return cxx
    return None


requires_hipcc = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
requires_host_cxx = pytest.mark.skipif(host_compiler() is None, reason="no C++ compiler")


def _run(cmd):
    r = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(map(str, cmd))}\nexit status {r.returncode}\n{r.stderr}")
    return r


def device_flags():
    """The arguments the product's objects are compiled with (csrc/Makefile: --offload-arch, CXXFLAGS, EXTRA), device only."""
    return _run(["make", "-s", "--no-print-directory", "-C", CSRC, "flags"]).stdout.split() + [f"-I{ROOT / 'include'}", f"-I{CSRC}", "--cuda-device-only"]


def kernel_resources(hip_file, tmp_path):
    """{mangled kernel name: {field of FIELDS: int}} for every kernel of csrc/<hip_file>, from one device compile."""
    src = hip_file if Path(hip_file).is_absolute() else CSRC / hip_file
    r = _run([HIPCC, *device_flags(), "-c", "-Rpass-analysis=kernel-resource-usage", src, "-o", Path(tmp_path) / (Path(hip_file).stem + ".o")])
    res = {}
    for block in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        found = dict(re.findall(r"remark:\s+([^:\n]+): (\d+) \[", block))
        res[re.match(r"\S+", block).group(0)] = {k: int(found[k]) for k in FIELDS}
    return res


def matching(res, part):
    """The figures of every kernel whose name contains `part` (or is `part`), as {name: fields}: never empty."""
    hit = {n: v for n, v in res.items() if part in n}
    if not hit:
        raise LookupError(f"no kernel named like {part!r}; the file has {sorted(res)}")
    return hit


def one(res, part):
    """The figures of the single kernel whose name contains `part` (or is `part`: a whole mangled name)."""
    hit = matching(res, part)
    if len(hit) != 1:
        raise LookupError(f"{part!r} names {len(hit)} kernels, {sorted(hit)}; the file has {sorted(res)}")
    return next(iter(hit.values()))


def host_harness(source, tmp_path, restypes_argtypes=None):
    """`source` (a kernel body header behind extern "C" loops) compiled for the host without contraction, as a ctypes.CDLL;
    restypes_argtypes: {function: (restype, argtypes)}."""
    cpp, so = Path(tmp_path) / "h.cpp", Path(tmp_path) / "h.so"
    cpp.write_text(source)
    _run([host_compiler(), "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wno-unknown-pragmas", f"-I{CSRC}", cpp, "-o", so])
    lib = ctypes.CDLL(str(so))
    for name, (restype, argtypes) in (restypes_argtypes or {}).items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    return lib
