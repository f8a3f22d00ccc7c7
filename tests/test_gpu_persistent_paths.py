"""The persistent planner launch (ChompEngine.run_persistent, omgx_plan_persistent, csrc/omg_persist.h) on the paths the other tests leave
out: rules that never select a goal, a launch that lasts longer than the bound of its waits, the status outside join(), scene counts at
the rings' capacity.  The reference is always the path the launch replaces — K calls of iterate() on a twin engine — and every tensor of
_CMP, Learner.t and Optimizer.step are compared bit for bit."""
from __future__ import annotations

import pytest

torch = pytest.importorskip("torch")

from test_gpu_round6 import _CMP, _pair, _same  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ready(*engines):
    for e in engines:
        e.select_initial_goal()
        e.pose_hand_over(True)


# ------------------------------------------------------------------------------------------------
# A. rules whose goal is fixed before planning: no iteration of the launch selects
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("alg", ["Baseline", "Proj"])
def test_fixed_goal_rules_through_the_persistent_launch(dev, alg, early_stop):
    """"Baseline" and "Proj" with cfg.goal_set_proj: every iteration of the plan is a fixed-goal one (layer + step), the launch gets a
    learner record whose rule it never reads — "Baseline" has no code among the learner's rules — and the goal select_initial_goal()
    fixed (for "Baseline" cfg.goal_idx = 4, not the default's goal 0) is still the goal afterwards."""
    over = {"optim_steps": 9, "extra_smooth_steps": 6, "goal_set_proj": True}
    if alg == "Baseline":
        over["goal_idx"] = 4
    S = 3
    a, b = _pair(dev, S, 6, 30, alg, cfg_over=over)
    _ready(a, b)
    chosen = b.goal_idx.clone()
    if alg == "Baseline":
        assert a.cfg.goal_idx == b.cfg.goal_idx == 4 and bool((chosen == 4).all())
    ts = list(range(15))
    for t in ts:
        a.iterate(t, early_stop=early_stop)
    b.run_persistent(ts, early_stop=early_stop)
    _same(a, b)
    assert torch.equal(a.active, b.active)
    st = b.persistent_status()
    assert st["failure"] == 0 and st["scenes_planned"] == S, st
    assert torch.equal(b.goal_idx, chosen) and torch.equal(a.goal_idx, chosen)


# ------------------------------------------------------------------------------------------------
# B. a launch that lasts longer than the bound of its waits
# ------------------------------------------------------------------------------------------------
LONG_K = 21865  # ceil(3.0 s / 0.13721 ms): see the test's docstring


def test_a_launch_longer_than_the_wait_bound(dev):
    """Every wait inside the launch is bounded by 2 s; a healthy launch that lasts longer must not run into that bound (omg_persist.h,
    out_of_patience: the bound counts from the plan's last progress).  One scene, two goals, 30 waypoints, 4 obstacles, "Proj" — eight
    workgroups, five items per iteration, so three workgroups at least have nothing to do at any time.  Measured on the MI355X: 500
    iterations of this plan in one launch take 68.6 ms, 0.13721 ms per iteration; K = ceil(3.0 s / 0.13721 ms) = 21 865 iterations (the
    launch allows 65 535), and that launch took 2.97 s: one and a half times the bound.  The twin's 21 865 iterate() calls take 0.8 s.
    (With the bound counted from the start of a claim attempt, as it was before, this launch passed as well: every workgroup took an
    activation off the ring often enough to restart its clock.  The test holds the long launch; it does not tell the two bounds apart.)

    cfg.cost_schedule_boost = 1: with the default's 1.02 the smoothness weight is 0.1 * 1.02 ** k, the costs are infinite after 500
    iterations and the trajectory is NaN before iteration 1000 — on both paths, but NaN is not equal to NaN.  With the weights stationary
    the plan converges and stays finite, which the test asserts, so that `equal` means something."""
    S, K = 1, LONG_K
    assert K <= 65535  # omgx_plan_persistent's own limit: an activation word holds 16 bits of the iteration
    a, b = _pair(dev, S, 2, 30, "Proj", objects=4, cfg_over={"cost_schedule_boost": 1.0})
    _ready(a, b)
    b.run_persistent(range(K))
    for t in range(K):
        a.iterate(t)
    _same(a, b)  # (join() inside raises OmgHipError when a wait of the launch ran out)
    st = b.persistent_status()
    assert st["failure"] == 0 and st["scenes_finished"] == S and st["activations"] == S * K, st
    for k in _CMP:
        assert bool(torch.isfinite(getattr(b, k).double()).all()), k


# ------------------------------------------------------------------------------------------------
# C. the status path
# ------------------------------------------------------------------------------------------------
def test_status_before_the_first_launch_is_a_clear_error(dev):
    """No launch, no status: a ValueError that says so (not an AttributeError from inside), and join() has nothing to look at."""
    a, _ = _pair(dev, 1, 2, 12, "MD", objects=3, grid=20)
    with pytest.raises(ValueError, match="no persistent launch"):
        a.persistent_status()
    a.join()


def _same_on_the_current_stream(a, b):
    """_same() without its device-wide synchronize: every tensor comes down through the current stream alone."""
    for k in _CMP:
        x, y = getattr(a, k).cpu(), getattr(b, k).cpu()
        assert torch.equal(x, y), (k, float((x.double() - y.double()).abs().max()))
    assert a.t == b.t and a.step_count == b.step_count


def test_join_waits_for_the_stream_the_launch_went_to(dev):
    """run_persistent under torch.cuda.stream(side), join() with the default stream current: join() waits for the launch where it was
    enqueued, and what is read next through the default stream — no synchronize in between — is what the launch left."""
    S, K = 6, 12
    a, b = _pair(dev, S, 16, 30, "MD")
    _ready(a, b)
    for t in range(K):
        a.iterate(t)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))  # the engine's tensors were prepared on the default stream
    with torch.cuda.stream(side):
        b.run_persistent(range(K))
    assert torch.cuda.current_stream(dev) != side
    b.join()
    _same_on_the_current_stream(a, b)
    st = b.persistent_status()
    assert st["failure"] == 0 and st["scenes_finished"] == S and st["activations"] == S * K, st


def test_no_pipelined_iteration_after_a_failed_launch(dev, monkeypatch):
    """A launch whose status says failure must stop the engine's NEXT call, whichever it is — also an iterate() that goes to pipeline
    parts built earlier, which calls no join().  No launch fails here: a healthy one, and a status that reports failure code 3 in its
    place."""
    from omg_planner_amd import _lib, ops
    S = 4
    a, b = _pair(dev, S, 8, 30, "MD")
    a.pipeline = b.pipeline = 2
    _ready(a, b)
    for e in (a, b):
        e.iterate(0)  # builds the two parts
    assert b._parts is not None and len(b._parts) == 2
    a.iterate(1)
    a.iterate(2)
    b.run_persistent([1, 2])
    b.join()
    _same(a, b)
    assert not b._forked
    b.run_persistent([3])  # healthy; its status has not been looked at
    torch.cuda.synchronize()
    before = b.traj.clone()
    real = ops.plan_persistent_status
    monkeypatch.setattr(ops, "plan_persistent_status", lambda ws, n: dict(real(ws, n), failure=3))
    with pytest.raises(_lib.OmgHipError, match="failure code 3"):
        b.iterate(4)
    torch.cuda.synchronize()
    assert torch.equal(b.traj, before)
    monkeypatch.undo()
    a.iterate(3)
    _same(a, b)  # and nothing else was touched: the engines still agree
    b.iterate(4)
    a.iterate(4)
    _same(a, b)


# ------------------------------------------------------------------------------------------------
# D. scene counts at the rings' capacity
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_wg", [0, 16])
@pytest.mark.parametrize("S", [64, 128])
def test_scene_counts_that_fill_the_rings(dev, S, max_wg):
    """The activation ring and the update rings hold S rounded up to 64 words: with 64 and 128 scenes every slot is in use at the
    start of the launch and the first activation of iteration 1 goes where scene 0's was."""
    K = 6
    a, b = _pair(dev, S, 2, 12, "MD", objects=3, grid=20)
    _ready(a, b)
    for t in range(K):
        a.iterate(t)
    b.run_persistent(range(K), max_workgroups=max_wg)
    _same(a, b)
    st = b.persistent_status()
    assert st["failure"] == 0 and st["activations"] == S * K, st
