"""ChompEngine._learner_params without a device: the record of the engine's rule is strict — a rule without a learner ("Baseline") is a
KeyError for every caller that means to run the learner — and the record run_persistent() builds for a launch that never selects a goal
names a rule by code instead (the launch does not read it).  On a stand-in engine holding what the method touches."""
from __future__ import annotations

from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")

from omg_planner_amd import _lib  # noqa: E402
from omg_planner_amd.config import Config  # noqa: E402
from omg_planner_amd.engine import ChompEngine  # noqa: E402


def _engine(alg, t=3):
    cfg = Config(timesteps=30, use_standoff=False)
    cfg.optim_steps = 9
    return SimpleNamespace(cfg=cfg, ol_alg=alg, G=6, n=30, t=t, c=1, use_standoff=False, eta=0.25, latency=False, goal_parts=1, _poses_on=False)


def test_the_record_of_a_rule_without_a_learner_is_refused():
    with pytest.raises(KeyError):
        ChompEngine._learner_params(_engine("Baseline"))
    assert "Baseline" not in _lib.ALG and "Proj" in _lib.ALG


@pytest.mark.parametrize("alg", ["Baseline", "Proj", "MD"])
def test_the_record_of_a_launch_that_never_selects(alg):
    p = ChompEngine._learner_params(_engine(alg), alg=_lib.ALG["Proj"])
    assert p.alg == _lib.ALG["Proj"]
    assert (p.num_goals, p.n_waypoints, p.constraint_num, p.use_standoff) == (6, 30, 1, 0)
    assert p.start_idx == min(int((3 / 9) * 30), 29) and p.eta == 0.25 and p.cost_parts == 0
    assert not p.goal_pose_table and not p.end_poses_out


@pytest.mark.parametrize("alg", ["FTL", "FTC", "Exp", "MD", "Proj"])
def test_the_record_of_a_rule_names_the_rule(alg):
    assert ChompEngine._learner_params(_engine(alg)).alg == _lib.ALG[alg]
