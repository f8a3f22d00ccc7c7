"""Generate tests/golden/ik_*.npz: the reference's own Planner.solve_and_process_ik / solve_goal_set_ik (omg/planner.py:17-86,
239-455) on stub Planner / target objects, with the CPU restatement's NR_JL solve (tests/ik_restatement.py) plugged in as
cfg.ROBOT.inverse_kinematics — PyKDL is not available, as make_golden.py plugs the oracle in as omg_cuda.

Runs only where the reference tree is present (never on the GPU machine):  python tests/golden/make_ik_golden.py [case ...]

* a real mat2quat / quat2mat (transforms3d's) is installed into omg.util: with the stubbed transforms3d, safemat2quat would
  silently return the identity quaternion (util.py:105-112);
* the ik_parallel path's multiprocessing.Pool(4) is replaced by an in-process map with the same call order (its outputs are
  concatenated in order either way), so the restatement's records see every solve;
* every case asserts that no recorded decision sits near its threshold — residual vs eps, iterations vs max_iter, the Frobenius
  diff vs 2, the filter's angle vs 120 degrees and the hand x axis vs -0.3 — and that no chain's result moves by more than 1e-9
  when its targets are taken as matrices instead of through the quaternion (a chain near a singular configuration amplifies
  that rounding), and draws new grasps until all hold, so that the fixtures pin count and order exactly.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parents[1]))

import make_golden as mg  # noqa: E402
import ik_restatement as ikr  # noqa: E402

# "near": a residual within 0.1 % of eps (a chain stable to 1e-9 moves its residual by ~1e-9 = 0.1 % of eps), a diff / angle /
# downward value within 1e-6 of its threshold, relatively
RES_MARGIN, REL_MARGIN = 1e-3, 1e-6


class SerialPool:
    def __init__(self, processes=None):
        pass

    def map(self, f, items):
        return [f(x) for x in items]

    def terminate(self):
        pass


def yaw_pose(x, y, z, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    P = np.eye(4)
    P[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    P[:3, 3] = [x, y, z]
    return P


def make_grasps(model, obj, rng, G, unreachable=0):
    """Hand poses of random configurations within the limits whose hand sits within 25 cm of the object, in the object frame;
    `unreachable` of them moved 2 m away."""
    from omg_planner_amd import scenes as sc
    q, pos, _, tree = sc._reach_pool(model)
    idx = np.array(tree.query_ball_point(obj[:3, 3], 0.25))
    pick = rng.choice(idx, G, replace=False)
    R, t, _, _ = ikr.hand_kinematics(model, q[pick, :7])
    H = np.tile(np.eye(4), (G, 1, 1))
    H[:, :3, :3], H[:, :3, 3] = R, t
    if unreachable:
        H[rng.choice(G, unreachable, replace=False), 0, 3] += 2.0
    return np.linalg.inv(obj) @ H


def near_threshold_report(model, kin, targets, seeds, use_standoff, attached, start, cfg):
    """Worst relative distance of any decision to its threshold (smaller = nearer)."""
    worst = {}
    res = np.concatenate(kin.record) if kin.record else np.zeros(1)
    worst["residual"] = float(np.min(np.abs(res / ikr.EPS - 1.0)))
    it = np.array(kin.iters)
    succ = it[it < ikr.MAX_ITER]
    worst["iters"] = float(ikr.MAX_ITER - 1 - (succ.max() if succ.size else 0))  # must stay >= 1 (a success at <= 98 updates)
    diffs, reach_all, perturb = [], [], 0.0
    T = targets.shape[1]
    kdl = targets.copy()  # the targets as the reference hands them to KDL (pack_pose -> quaternion): rounding apart from `targets`
    for g in range(targets.shape[0]):
        for k in range(T):
            kdl[g, k, :3, :3] = ikr.kdl_target(targets[g, k])
    K = len(seeds)
    for g in range(targets.shape[0]):
        outs = []  # per variant: (accepted [K], solutions [K, T, 7]) — all seeds of the grasp at once
        for tg in (targets[g], kdl[g]):
            if not use_standoff:
                q, ok, _ = ikr.solve(model, np.repeat(tg[:1, :3, :3], K, 0), np.repeat(tg[:1, :3, 3], K, 0), seeds)
                outs.append((ok, q[:, None]))
                continue
            q, alive, _ = ikr.solve(model, np.repeat(tg[T - 1:, :3, :3], K, 0), np.repeat(tg[T - 1:, :3, 3], K, 0), seeds)
            sols = []
            for k in range(T):
                q, ok, _ = ikr.solve(model, np.repeat(tg[k:k + 1, :3, :3], K, 0), np.repeat(tg[k:k + 1, :3, 3], K, 0), q)
                alive = alive & ok
                sols.append(q)
            outs.append((alive, np.stack(sols, 1)))
        # a chain whose result moves with the rounding of its target is as fragile as a decision near its threshold
        if not np.array_equal(outs[0][0], outs[1][0]):
            perturb = np.inf
        elif outs[0][0].any():
            perturb = max(perturb, float(np.abs(outs[0][1][outs[0][0]] - outs[1][1][outs[0][0]]).max()))
        for j in np.nonzero(outs[0][0])[0]:
            if not use_standoff:
                reach_all.append(np.concatenate([outs[0][1][j, 0], [0.04, 0.04]])[None])
                continue
            sols = list(outs[0][1][j])
            tr = np.stack(sols if attached else sols[::-1])
            diffs.append(np.linalg.norm(np.diff(tr, axis=0)))
            reach_all.append(np.concatenate([tr, np.full((T, 2), 0.04)], axis=1))
    worst["perturb"] = perturb
    worst["diff"] = float(np.min(np.abs(np.array(diffs) / 2.0 - 1.0))) if diffs else 1.0
    if reach_all and not attached:
        rk = np.stack(reach_all)
        flipped = rk.copy()
        j = flipped[..., -3]
        flipped[..., -3] = np.where(j < 0, j + np.pi, np.where(j > 0, j - np.pi, j))
        rk = np.concatenate([rk, flipped])
        end = rk[:, -1]
        if use_standoff:
            t = np.linspace(0, 1, 7)[1:-1]
            pts = (end[:, None] - start[None, None]) * t[None, :, None] + start[None, None]
        else:
            pts = end[:, None]
        Rs = ikr.hand_kinematics(model, start[None, :7])[0][0]
        R = ikr.hand_kinematics(model, pts.reshape(-1, 9)[:, :7])[0]
        tr = np.trace(R @ Rs.T, axis1=1, axis2=2)
        ang = np.degrees(np.arccos(np.clip((tr - 1) / 2, -1, 1)))
        worst["angle"] = float(np.min(np.abs(ang / cfg.target_hand_filter_angle - 1.0)))
        xz = R[:, 2, 0] / np.linalg.norm(R[:, :, 0], axis=-1)
        worst["downward"] = float(np.min(np.abs(xz / -0.3 - 1.0)))
    return worst


CASES = [
    # name, use_standoff, attached, ik_parallel, z_upsample, y_upsample, one_trial, obj_coord, G, unreachable
    ("standoff_par", 1, 0, 1, 0, 0, 0, 1, 10, 0),
    ("standoff_seq", 1, 0, 0, 0, 0, 0, 1, 10, 0),
    ("nostandoff_seq", 0, 0, 0, 0, 0, 0, 1, 10, 0),
    ("attached_seq", 1, 1, 0, 0, 0, 0, 1, 6, 0),
    ("zup_seq", 1, 1, 0, 1, 0, 0, 1, 1, 0),
    ("yup_par", 1, 0, 1, 0, 1, 0, 1, 2, 0),
    ("onetrial_seq", 1, 0, 0, 0, 0, 1, 1, 10, 0),
    ("world_par", 1, 0, 1, 0, 0, 0, 0, 10, 0),
    ("unreachable_seq", 1, 0, 0, 0, 0, 0, 1, 10, 4),
]


def run_case(case, config, util, pl, kin_ref, model, seed):
    name, use_standoff, attached, parallel, z_up, y_up, one_trial, obj_coord, G, unreach = case
    rng = np.random.RandomState(seed)
    cfg = config.cfg
    cfg.use_standoff, cfg.ik_parallel, cfg.y_upsample, cfg.silent = bool(use_standoff), bool(parallel), bool(y_up), True
    cfg.increment_iks = False
    cfg.ik_seed_num = 4 if z_up else 12  # 50 rotated poses x 5 seeds keep the placement case's one-at-a-time solves affordable
    kin = ikr.Kinematics(model)
    cfg.ROBOT = kin
    obj = yaw_pose(rng.uniform(0.4, 0.6), rng.uniform(-0.2, 0.2), rng.uniform(0.1, 0.3), rng.uniform(-np.pi, np.pi))
    obj7 = util.pack_pose(obj)
    obj_used = util.unpack_pose(obj7)
    pg = make_grasps(model, obj_used, rng, G, unreach)
    if z_up:  # a placement: the inverse of a hand pose relative to the object, one of it (load_grasp_set)
        pg = pg[:1]
    if not obj_coord:
        pg = obj_used @ pg
    start = np.array([0.0, -1.285, 0.0, -2.356, 0.0, 1.571, 0.785, 0.04, 0.04]) + np.r_[rng.normal(0, 0.1, 7), 0, 0]
    captured = []
    orig = pl.solve_one_pose_ik

    def capture(inp):
        captured.append(np.array(inp[1]))
        return orig(inp)

    pl.solve_one_pose_ik = capture
    pl.multiprocessing.Pool = SerialPool
    planner = object.__new__(pl.Planner)
    planner.cfg = cfg
    planner.traj = types.SimpleNamespace(start=start)
    planner.env = types.SimpleNamespace(robot=types.SimpleNamespace(robot_kinematics=kin_ref))
    target = types.SimpleNamespace(pose=obj7, attached=bool(attached), name="obj", reach_grasps=[], grasps=[])
    try:
        if one_trial:
            reach, grasps = planner.solve_goal_set_ik(target, planner.env, pg.copy(), one_trial=True, z_upsample=bool(z_up),
                                                      y_upsample=bool(y_up), obj_coord=bool(obj_coord))
            stage = "solve"
        else:
            planner.solve_and_process_ik(target, pg.copy(), bool(z_up), obj_coord=bool(obj_coord))
            reach, grasps = target.reach_grasps, target.grasps
            stage = "process"
    finally:
        pl.solve_one_pose_ik = orig
    T = cfg.reach_tail_length
    targets = np.stack(captured) if captured else np.zeros((0, T, 4, 4))
    seeds = ikr.ANCHOR_SEEDS[:cfg.ik_seed_num]
    seeds = start[None, :7] if one_trial else np.concatenate([start[None, :7], seeds])
    worst = near_threshold_report(model, ikr.Kinematics(model), targets, seeds, use_standoff, attached, start, cfg)
    for key, v in near_threshold_report(model, kin, np.zeros((0, T, 4, 4)), seeds, use_standoff, attached, start, cfg).items():
        worst[key] = max(worst.get(key, v), v) if key == "perturb" else min(worst.get(key, v), v)
    reach = np.array(reach, np.float64)
    grasps = np.array(grasps, np.float64)
    if use_standoff:
        reach = reach.reshape(-1, T, 9)
    else:
        reach = reach.reshape(-1, 9)
    grasps = grasps.reshape(-1, 9)
    data = dict(pose_grasp=pg, obj_pose7=obj7, object_pose=obj_used, start=start, targets=targets, reach_grasps=reach, grasps=grasps,
                use_standoff=use_standoff, attached=attached, ik_parallel=parallel, z_upsample=z_up, y_upsample=y_up,
                one_trial=one_trial, obj_coord=obj_coord, stage=stage, reach_tail_length=T, standoff_dist=cfg.standoff_dist,
                ik_seed_num=cfg.ik_seed_num)
    return data, worst


def main():
    config, cost, optimizer, util, rk = mg.load_reference()
    import importlib
    util.mat2quat = ikr.mat2quat
    from omg_planner_amd.goal_ik import quat2mat
    util.quat2mat = quat2mat
    pl = importlib.import_module("omg.planner")
    from omg_planner_amd import robot as rb
    model = rb.PandaModel()
    kin_ref = mg.make_kinematics(rk)
    # arguments: case names to (re)generate (all by default); "--attempt N" tries only attempt N of each (attempts are independent:
    # several can run side by side, and the fixture is the lowest attempt that passes — what a plain run finds first)
    args = sys.argv[1:]
    attempts = range(20)
    if "--attempt" in args:
        i = args.index("--attempt")
        attempts = [int(args[i + 1])]
        del args[i:i + 2]
    only = set(args)
    for case in CASES:
        if only and case[0] not in only:
            continue
        for attempt in attempts:
            data, worst = run_case(case, config, util, pl, kin_ref, model, 1000 * (CASES.index(case) + 1) + attempt)
            ok = worst["residual"] > RES_MARGIN and worst["iters"] >= 1 and worst["diff"] > REL_MARGIN and worst["perturb"] <= 1e-9 \
                and worst.get("angle", 1.0) > REL_MARGIN and worst.get("downward", 1.0) > REL_MARGIN
            if ok:
                break
            print(case[0], "attempt", attempt, "near a threshold:", worst)
        else:
            raise RuntimeError(f"{case[0]}: every attempt had a decision near its threshold")
        np.savez_compressed(HERE / (f"ik_{case[0]}.npz" if len(attempts) > 1 else f"ik_{case[0]}.attempt{attempt}.npz"), **data)
        print(case[0], "grasps", data["grasps"].shape, "reach", data["reach_grasps"].shape, "targets", data["targets"].shape, worst)


if __name__ == "__main__":
    main()
