"""The generators of tests/fuzz/fuzz_mesh.py without a GPU: with the specification alone, few draws are rejected and every
listed choice occurs within a run of 40 trials."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest


@pytest.fixture(scope="module")
def fm():
    spec = importlib.util.spec_from_file_location("fuzz_mesh", Path(__file__).resolve().parent / "fuzz" / "fuzz_mesh.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("seed", [12345, 7])
def test_generators_reject_little_and_cover_every_choice(fm, seed):
    rng = np.random.RandomState(seed)
    draws = fm.Draws()
    cases = {name: [] for name, _ in fm.SECTIONS}
    for _ in range(40):
        for name, fn in fm.SECTIONS:
            cases[name].append(draws.draw(name, fn, rng))
    print(draws)
    assert draws.share() <= fm.MAX_REJECTED, str(draws)
    assert all(draws.drawn[name] >= 40 for name, _ in fm.SECTIONS)
    sdf, ray, grasp, render = (cases[k] for k in ("sdf", "raycast", "grasp", "render"))
    assert {c["M"] for c in sdf} == set(fm.SDF_BATCHES) and {c["M"] for c in ray} == set(fm.RAY_BATCHES)
    assert {c["chunks"] for c in ray} == set(fm.CHUNKS)
    assert {n for c in ray for n in c["counts"]} == set(fm.RAY_COUNTS)
    assert {k for c in ray for k in c["kinds"]} == set(fm.RAY_KINDS)
    assert {c["t_min"] for c in ray} == set(fm.T_MINS) and {c["tol"] for c in ray} == set(fm.TOLS)
    for group in (sdf, ray, grasp):
        assert {m[2] for c in group for m in c["meshes"]} == {True, False}                      # closed and open meshes
    assert {v[2] for c in sdf for v in c["vols"]} == {"centre", "node"} == {v[2] for c in grasp for v in c["vols"]}
    dims = {v[4] for c in sdf for v in c["vols"]}
    assert (1, 1, 1) in dims and any(d[:2] == (1, 1) and d[2] > 1 for d in dims) and any(min(d) > 1 for d in dims)
    assert any(not any(v[5] for v in c["vols"]) for c in sdf)                                   # a batch on the default layouts
    assert max(len(m[1]) for c in sdf for m in c["meshes"]) <= fm.MAX_FACES and max(int(np.prod(d)) for d in dims) <= fm.MAX_NODES
    assert all(len(set(c["offsets"])) == c["M"] for c in sdf) and all(min(c["offsets"]) > 0 for c in grasp)
    assert {c["A"] for c in grasp} == {1, 3, 8} and {len(c["probe"]) for c in grasp} == {1, 17, 100}
    assert {c["clearance"] for c in grasp} == {0.0, 0.004} and len({c["max_width"] for c in grasp}) == 3
    assert len({c["min_width"] for c in grasp}) == 3 and len({c["pad_depth"] for c in grasp}) == 3 and len({c["cone"] for c in grasp}) == 3
    assert all(64 <= len(x[0]) <= 300 for c in grasp for x in c["contacts"])
    assert {c["S"] for c in render} == {1, 2, 5} and {c["cull"] for c in render} == {True, False} == {c["want_face"] for c in render}
    assert any(c["mirrored"] for c in render) and any(min(c["H"], c["W"]) < 16 for c in render) and any(max(c["H"], c["W"]) > 32 for c in render)
    assert any(c["H"] % 16 and c["W"] % 16 for c in render) and {int(n) for c in render for n in np.diff(c["inst_begin"])} >= {0, 8}
    dets = [np.linalg.det(np.asarray(p)[:3, :3]) for c in render for ps in c["poses"] for p in ps]
    assert min(dets) < 0 < max(dets)
    assert {c["t_min"] for c in render} == set(fm.T_MINS) and {c["tol"] for c in render} == set(fm.TOLS)
