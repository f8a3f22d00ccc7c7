"""ctypes loader of libomg_hip.so (the hand-written gfx950 kernels + C ABI of include/omg_hip.h).

The bindings are not written here: constants, structs and every function's restype / argtypes come from the header itself
(_header.parse), so a new entry point is bound by declaring it there.

There is NO fallback: if the library is missing or a call fails, an exception is raised.  Nothing in
this package computes the hot path on the CPU.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

from . import _header

_CSRC = Path(__file__).resolve().parent / "csrc"
LIB_PATH = _CSRC / "libomg_hip.so"

# include/omg_hip.h is the only description of the ABI: its #defines, structs and prototypes, read once at import
CONSTANTS, STRUCTS, FUNCTIONS = _header.parse(_header.HEADER.read_text())
_K = {name[len("OMGX_"):]: value for name, value in CONSTANTS.items()}
OMGX_OK, OMGX_ERR_INVALID, OMGX_ERR_LAUNCH, OMGX_ERR_UNSUPPORTED = _K["OK"], _K["ERR_INVALID"], _K["ERR_LAUNCH"], _K["ERR_UNSUPPORTED"]
NUM_DOF, INFO_STRIDE = _K["NUM_DOF"], _K["INFO_STRIDE"]
SCHEDULE_MAX_SCENES = _K["SCHEDULE_MAX_SCENES"]
SCHEDULE_SCENE_MAJOR, SCHEDULE_LONGEST_FIRST = _K["SCHEDULE_SCENE_MAJOR"], _K["SCHEDULE_LONGEST_FIRST"]  # the order inside an XCD (omgx_goalset_schedule_ordered)
SCHEDULE_LONGEST_FIRST_MAX_ITEMS = _K["SCHEDULE_LONGEST_FIRST_MAX_ITEMS"]
SELECT_MAX_GOALS = _K["SELECT_MAX_GOALS"]
MESH_SDF_NODES_PER_WORKGROUP = _K["MESH_SDF_NODES_PER_WORKGROUP"]
RAYCAST_RAYS_PER_WORKGROUP, RAYCAST_MAX_CHUNKS = _K["RAYCAST_RAYS_PER_WORKGROUP"], _K["RAYCAST_MAX_CHUNKS"]
CAMERA_PIXELS_PER_WORKGROUP = _K["CAMERA_PIXELS_PER_WORKGROUP"]
SURFACE_NODES_PER_WORKGROUP = _K["SURFACE_NODES_PER_WORKGROUP"]
FUSION_NODES_PER_WORKGROUP, FUSION_MAX_RADIUS, FUSION_CHUNK = _K["FUSION_NODES_PER_WORKGROUP"], _K["FUSION_MAX_RADIUS"], _K["FUSION_CHUNK"]
SEGMENT_NODES_PER_WORKGROUP = _K["SEGMENT_NODES_PER_WORKGROUP"]
PLANE_PIXELS_PER_WORKGROUP, PLANE_STAGE_HYPOTHESES = _K["PLANE_PIXELS_PER_WORKGROUP"], _K["PLANE_STAGE_HYPOTHESES"]
PLANE_MAX_HYPOTHESES, PLANE_NODES_PER_WORKGROUP = _K["PLANE_MAX_HYPOTHESES"], _K["PLANE_NODES_PER_WORKGROUP"]
TSDF_NODES_PER_WORKGROUP = _K["TSDF_NODES_PER_WORKGROUP"]
VOLUME_CAMERA_MAX_STEPS = _K["VOLUME_CAMERA_MAX_STEPS"]
ALG = {"FTL": _K["ALG_FTL"], "FTC": _K["ALG_FTC"], "Exp": _K["ALG_EXP"], "MD": _K["ALG_MD"], "Proj": _K["ALG_PROJ"]}
ABI_VERSION = 14  # omgx_abi_version() of the library this package was written against

EXPORTS = list(FUNCTIONS)  # every symbol the header declares
ChompParams, LearnerParams, PlanIter = STRUCTS["omgx_chomp_params"], STRUCTS["omgx_learner_params"], STRUCTS["omgx_plan_iter"]
Object, Mesh, RayWork = STRUCTS["omgx_object"], STRUCTS["omgx_mesh"], STRUCTS["omgx_ray_work"]
Camera, Instance = STRUCTS["omgx_camera"], STRUCTS["omgx_instance"]


class OmgHipError(RuntimeError):
    pass


def build(force: bool = False) -> Path:
    """Compile csrc/*.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", str(_CSRC)] + (["-B"] if force else [])
    subprocess.run(args, check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise OmgHipError(f"{LIB_PATH} is missing: build it with `make -C {_CSRC}` "
                              "(or __graft_entry__.build()); there is no CPU fallback")
        try:
            # torch first: its HIP runtime must be the one in the process before this library binds to it (loaded the other way
            # round — build() followed by smoke() in one process — the two runtimes disagree and no device is found)
            import torch  # noqa: F401
        except ImportError:
            pass
        l = C.CDLL(str(LIB_PATH))
        for name, (restype, argtypes) in FUNCTIONS.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = restype, argtypes
        if l.omgx_abi_version() != ABI_VERSION:
            raise OmgHipError(f"{LIB_PATH} has ABI {l.omgx_abi_version()}, this package needs {ABI_VERSION}: rebuild it (make -C {_CSRC})")
        _lib = l
    return _lib


def check(rc: int, what: str) -> None:
    if rc == OMGX_OK:
        return
    if rc == OMGX_ERR_LAUNCH:
        raise OmgHipError(f"{what}: {lib().omgx_last_error().decode()}")
    names = {OMGX_ERR_INVALID: "invalid argument", OMGX_ERR_UNSUPPORTED: "size not supported by this build"}
    raise OmgHipError(f"{what}: {names.get(rc, rc)}")


def device_arch() -> str:
    buf = C.create_string_buffer(64)
    check(lib().omgx_device_arch(buf, 64), "omgx_device_arch")
    return buf.value.decode()
