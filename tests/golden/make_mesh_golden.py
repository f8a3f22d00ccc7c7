#!/usr/bin/env python3
"""Generate tests/golden/sdf_text_ramp.npz by RUNNING THE REFERENCE'S OWN READER on tests/golden/sdf_text_ramp.sdf.

Runs only in the build container (needs /root/reference; the tests read the committed .npz only):

    python tests/golden/make_mesh_golden.py

The input is a tiny hand-made text volume: a 2 x 3 x 4 ramp 0.125 * (x + 2 y + 6 z) - 0.5 with x running fastest, origin
(-0.01, 0.02, 0.125), delta 0.005 — every value a different number, so a reader that mixes up the axes cannot pass.  It is parsed
with SignedDensityField.from_sdf (omg/sdf_tools.py:169-185); the array it builds (data[x, y, z]), its origin and its delta are
recorded.  scene_io.read_sdf_text must reproduce that record (tests/test_mesh_sdf_cpu.py).

The reference module is imported as make_golden.py imports it on a CPU-only box: a `sys.modules` stub for IPython and
`torch.Tensor.cuda` patched to the identity (SignedDensityField.__init__ puts copies on the GPU, sdf_tools.py:31-35).
The fixture is data only; no reference source is stored.
"""
from __future__ import annotations

import importlib.util
import sys
import types
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent


def main():
    import torch
    sys.modules.setdefault("IPython", types.ModuleType("IPython"))
    torch.Tensor.cuda = lambda self, *a, **k: self
    spec = importlib.util.spec_from_file_location("ref_sdf_tools", REF / "omg" / "sdf_tools.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sdf = mod.SignedDensityField.from_sdf(str(OUT / "sdf_text_ramp.sdf"))
    np.savez(OUT / "sdf_text_ramp.npz", data=np.asarray(sdf.data, np.float64), origin=np.asarray(sdf.origin, np.float64),
             delta=np.float64(sdf.delta))
    print("wrote", OUT / "sdf_text_ramp.npz", sdf.data.shape, sdf.origin, sdf.delta)


if __name__ == "__main__":
    main()
