"""bench.py's result line on the GPU: a plain run times exactly --steps steps and carries the headline alone; --dump-outputs writes
what the last timed step computed, the same from run to run and the same as the engine driven in-process; --full carries the
rest (roofline, the regions' spread, the parity sample)."""
from __future__ import annotations

import copy
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = Path(__file__).resolve().parents[1]
SHAPE = ["--gpus", "1", "--scenes", "6", "--goals", "8", "--grid", "24"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _line(args, timeout=600):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(dev, tmp_path):
    steps, warmup = 7, 2
    a = _line([*SHAPE, "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "a")])
    b = _line([*SHAPE, "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "b")])
    for j in (a, b):
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(j)
        assert j["steps"] == steps and j["warmup"] == warmup and j["unit"] == "iterations/s" and j["higher_is_better"] is True
        assert j["ms_per_step"] > 0 and j["value"] == pytest.approx(6 * 1e3 / j["ms_per_step"], rel=1e-9)
        assert not {"roofline", "regions", "parity_sample", "cpu_baseline", "ms_per_plan", "collective"} & set(j)
    names = sorted(p.stem for p in (tmp_path / "a").glob("*.npy"))
    assert names == sorted(p.stem for p in (tmp_path / "b").glob("*.npy"))
    assert {"traj", "info", "goal_idx", "goal_cost", "final_costs"} <= set(names)
    total = 0
    for k in names:
        x, y = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y, equal_nan=True), k
        total += x.nbytes
    assert total <= 64 << 20
    # the same workload driven here: warmup + steps iterations of the pinned-window step -> the same bits
    import bench
    from omg_planner_amd.engine import ChompEngine
    cfg, model, batch, start, goals = bench.build_workload(6, 8, 30, 24, seed0=0, share_grids=False, device=dev)
    eng = ChompEngine.auto(model, batch, copy.deepcopy(cfg), start, goals, layout_scenes=6, device=dev, ol_alg="MD")
    eng.pose_hand_over(True)
    for _ in range(warmup + steps):
        eng.t = 0
        eng.iterate(0)
    costs = eng.final_costs()
    torch.cuda.synchronize()
    got = {"traj": eng.traj, "info": eng.info, "goal_idx": eng.goal_idx, "goal_cost": eng.goal_cost_total(), "final_costs": costs}
    for k, v in got.items():
        assert np.array_equal(np.load(tmp_path / "a" / f"{k}.npy"), v.cpu().numpy().astype(np.load(tmp_path / "a" / f"{k}.npy").dtype)), k
    assert a["config"]["layout"] == dict(eng.layout_used, pipeline=a["config"]["pipeline_parts"], evaluated_for_scenes=6)


def test_full_line_keeps_the_rest(dev):
    j = _line([*SHAPE, "--steps", "5", "--warmup", "1", "--full", "--no-plan", "--no-cpu-baseline"], timeout=900)
    assert j["steps"] == 5 and j["ms_per_step"] > 0 and j["regions"] >= 5  # a region of a few ms: more regions for the spread
    lo, hi = j["ms_per_step_spread"]
    assert lo <= j["ms_per_step"] <= hi and lo <= j["ms_per_step_median_region"] <= hi
    assert j["roofline"]["launches"] > 0 and j["roofline"]["avg_launch_ms"] > 0
    assert j["parity_sample"]["ok"] is True
