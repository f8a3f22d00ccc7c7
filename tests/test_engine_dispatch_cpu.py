"""ChompEngine._dispatch_rule, the dispatch-schedule policy of a goal-set launch as a function of plain values, against a
restatement of the code it was lifted from: the lines of ChompEngine.update_goal() that used to hold the policy, run here on a
stand-in engine whose build_schedule() and goal-set launch only record how they were called.  The full product of the
function's inputs, and two consequences by name."""
from __future__ import annotations

import itertools
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")

from omg_planner_amd.engine import ChompEngine  # noqa: E402

MIN = ChompEngine.MEASURE_MIN_ITEMS
BOOLS = (False, True)
# auto_schedule, masked, measured, np_is_max, has_schedule, sched_np_ok | reschedule_every | launches | items | sched_age
ROWS = list(itertools.product(BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, (0, 1, 3), (1, 2, 3), (MIN - 1, MIN), (None, 0, 1, 3)))


class _Engine(SimpleNamespace):
    """What the restated lines touch of an engine."""
    MEASURE_MIN_ITEMS = MIN

    def _np(self, n_rem):
        return self.NP

    def _mask(self):
        return "mask" if self._masked else None

    def build_schedule(self, active=None, uniform=False, parts=1):
        self.builds.append((active, uniform, parts))
        self._sched_np = parts  # as the engine's does
        return f"schedule {len(self.builds)}"


def _restated(self, ops, n_rem, traj_start):
    """engine.py, ChompEngine.update_goal(), the branch of the fused batch-layout launch before the policy moved — as it stood."""
    self._gs_launches += 1
    NP = self._np(n_rem)
    self._parts_last = NP
    use_sched = self.auto_schedule and (not self._masked or (self._measured and bool(self.reschedule_every)))
    measure = use_sched and not self._measured and self._gs_launches >= 2 and self.S * self.G * NP >= self.MEASURE_MIN_ITEMS and NP == self._parts_max
    if use_sched and self._masked:
        if self._sched_age is None or self._sched_age >= self.reschedule_every or self._sched_np != NP:
            self.schedule = self.build_schedule(active=self._mask(), parts=NP, uniform=(NP != self._parts_max or not self._measured))
            self._sched_age = 0
        self._sched_age += 1
    if use_sched and (self.schedule is None or self._sched_np != NP):
        # nothing measured yet, or the window has shrunk to another number of parts per goal (the last few iterations
        # of a plan): the items in scene-major order, equal counts per XCD
        self.schedule = self.build_schedule(uniform=True, parts=NP)
    ops.goalset_cost_layer(self.robot, self.P, self.scenes, traj_start, self.cv_goals, n_rem, self.cfg.time_interval,
                           self.traj, (self.pot, self.pgrad, self.col), soften_fingers=False,
                           layer_soften_fingers=self.cfg.uncheck_finger_collision == -1,
                           out=(self.goal_cost, self.goal_col), active=self._mask(), goal_count=self.goal_count,
                           schedule=self.schedule if use_sched else None, work=self.work[: self.S * self.G * NP] if measure else None,
                           goal_parts=self.goal_parts, layer_poses=self.wp_pose if self._poses_on else None,
                           prepass=self.prepass)
    if measure:
        self._measured = True
        self.schedule = self.build_schedule(parts=NP)


def _parent(auto, masked, measured, np_is_max, has_schedule, sched_np_ok, every, launches, items, age):
    """The restated lines on a stand-in engine in the state the inputs describe -> (use, rebuild, measure, sched_age)."""
    NP = 1
    e = _Engine(NP=NP, S=items, G=1, auto_schedule=auto, _masked=masked, _measured=measured, reschedule_every=every, _gs_launches=launches - 1,
                _parts_max=NP if np_is_max else 2, schedule="schedule 0" if has_schedule else None, _sched_np=NP if sched_np_ok else 2,
                _sched_age=age, work=list(range(items * NP)), builds=[], _poses_on=False, goal_parts=1, prepass=False, wp_pose=None,
                robot=None, P=0, scenes=None, cv_goals=None, traj=None, pot=None, pgrad=None, col=None, goal_cost=None, goal_col=None, goal_count=None,
                cfg=SimpleNamespace(time_interval=0.1, uncheck_finger_collision=0))
    launch = {}
    ops = SimpleNamespace(goalset_cost_layer=lambda *a, **kw: launch.update(kw, builds_before=len(e.builds)))
    _restated(e, ops, 8, None)
    before, after = e.builds[: launch["builds_before"]], e.builds[launch["builds_before"]:]
    assert len(before) <= 1
    kinds = {(None, True, NP): "uniform", ("mask", True, NP): "masked-uniform", ("mask", False, NP): "masked-measured"}
    rebuild = kinds[before[0]] if before else None
    measure = launch["work"] is not None
    assert after == ([(None, False, NP)] if measure else []) and e._measured == (measured or measure)
    assert launch["work"] is None or len(launch["work"]) == items * NP
    if launch["schedule"] is not None:  # the launch takes the schedule at hand after the rebuild, built for its part count
        assert launch["schedule"] == e.schedule if not measure else launch["schedule"] == f"schedule {len(before)}"
    return launch["schedule"] is not None, rebuild, measure, e._sched_age


def _rule(auto, masked, measured, np_is_max, has_schedule, sched_np_ok, every, launches, items, age):
    use, rebuild, measure, new_age = ChompEngine._dispatch_rule(auto, masked, measured, every, launches, items, MIN, np_is_max, has_schedule, sched_np_ok, age)
    return bool(use), rebuild, bool(measure), new_age


def test_the_rule_is_the_policy_update_goal_held():
    assert len(ROWS) == 2 ** 6 * 3 * 3 * 2 * 4
    wrong = [row for row in ROWS if _rule(*row) != _parent(*row)]
    assert not wrong, (len(wrong), wrong[:5])


def test_a_masked_launch_never_measures():
    for row in ROWS:
        if row[1]:
            assert not _rule(*row)[2], row


def test_an_engine_below_its_first_part_count_is_never_asked_to_measure():
    """NP != _parts_max and nothing measured: the launch does not measure, whatever the launch count and the item count — the
    case in which the engine once kept leaving its prepared calls for a measurement that could not happen."""
    for row in ROWS:
        auto, masked, measured, np_is_max = row[:4]
        if not np_is_max and not measured:
            assert not _rule(*row)[2], row
