"""Goal-set IK on the device: grasp poses -> (standoff) goal sets, batched over scenes.

The stage of the reference's goal-set pipeline between the grasp poses (Planner.load_grasp_set / load_goal_from_external,
omg/planner.py:176-186, 457-500) and Planner.setup_goal_set (goalset.py here):

* pose preparation  (Planner.solve_goal_set_ik, planner.py:296-358): object frame, z / y upsampling, standoff poses — torch f64;
* the IK            (solve_one_pose_ik, planner.py:17-86, over KDL's NR_JL solver) — omgx_goal_ik, one lane per (grasp, seed);
* compaction        successes in (grasp, seed) order per scene — a prefix sum over the accepted chains;
* post-processing   (Planner.solve_and_process_ik, planner.py:239-294): the wrist-flip augmentation and the hand-rotation filter,
                    the filter's kinematics on omgx_forward_kinematics.

``solve_goal_sets`` is the batched API: its outputs are what ``goalset.goal_collision_stats`` / ``select_goals`` and
``ChompEngine(..., goal_counts=...)`` take.  ``solve_goal_set_ik`` / ``solve_and_process_ik`` are drop-ins with the reference's
signatures.  The reference's ``ik_parallel`` quirk (its pool never solves a target's last grasp) is kept behind
``parallel`` (default cfg.ik_parallel); ``increment_iks`` is refused (it draws from np.random).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from . import robot as rb

FINGER = 0.04
# omg/util.py:19-35, arm joints (radians)
ANCHOR_SEEDS = np.array([
    [2.5, 0.23, -2.89, -1.69, 0.056, 1.46, -1.27], [2.8, 0.23, -2.89, -1.69, 0.056, 1.46, -1.27],
    [2, 0.23, -2.89, -1.69, 0.056, 1.46, -1.27], [2.5, 0.83, -2.89, -1.69, 0.056, 1.46, -1.27],
    [0.049, 1.22, -1.87, -0.67, 2.12, 0.99, -0.85], [-2.28, -0.43, 2.47, -1.35, 0.62, 2.28, -0.27],
    [-2.02, -1.29, 2.20, -0.83, 0.22, 1.18, 0.74], [-2.2, 0.03, -2.89, -1.69, 0.056, 1.46, -1.27],
    [-2.5, -0.71, -2.73, -0.82, -0.7, 0.62, -0.56], [-2, -0.71, -2.73, -0.82, -0.7, 0.62, -0.56],
    [-2.66, -0.55, 2.06, -1.77, 0.96, 1.77, -1.35], [1.51, -1.48, -1.12, -1.55, -1.57, 1.15, 0.24],
    [-2.61, -0.98, 2.26, -0.85, 0.61, 1.64, 0.23]])
STATUS_ACCEPTED, STATUS_REJECTED = 0, -1  # omgx_goal_ik status; j > 0: solve j - 1 failed


def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])


def prepare_poses(pose_grasp, object_pose, obj_coord=True, z_upsample=False, y_upsample=False, reach_tail_length=5,
                  standoff_dist=0.08, use_standoff=True, device=None):
    """planner.py:316-358 for one target: pose_grasp [G,4,4], object_pose [4,4] -> standoff poses [G', T, 4, 4] float64 (torch, on
    `device`), k = 0 the grasp itself; T = 1 without standoff.  z_upsample: 50 rotations about the object's z through its origin,
    np.matmul(global_rot_z, poses) (so G must be 1 or 50, as in the reference); y_upsample: 10 tilts about the finger contact
    0.13 m along z, grasp-major."""
    dev = device if device is not None else (pose_grasp.device if isinstance(pose_grasp, torch.Tensor) else "cpu")
    f64 = dict(dtype=torch.float64, device=dev)
    g = torch.as_tensor(pose_grasp, **f64).reshape(-1, 4, 4)
    obj = torch.as_tensor(object_pose, **f64)
    g = torch.matmul(obj, g) if obj_coord else g.clone()
    if z_upsample:
        rz = torch.as_tensor(np.stack([_rot_z(a) for a in np.linspace(-np.pi, np.pi, 50)]), **f64)
        g = g.clone()
        g[:, :3, 3] = g[:, :3, 3] - obj[:3, 3]
        g = torch.matmul(rz, g)
        g[:, :3, 3] += obj[:3, 3]
    if y_upsample:
        ry = torch.as_tensor(np.stack([_rot_y(a) for a in np.linspace(-np.pi / 4, np.pi / 4, 10)]), **f64)
        finger = g[:, :3, 2] * 0.13 + g[:, :3, 3]                                   # R . (0, 0, 0.13) + t
        local = torch.matmul(g[:, :3, :3], ry[:, None, :3, :3])                       # [10, G, 3, 3]
        delta = local[..., 2] * 0.13
        out = g[:, None].repeat(1, 10, 1, 1)
        out[:, :, :3, 3] = (finger[None] - delta).transpose(0, 1)
        out[:, :, :3, :3] = local.transpose(0, 1)
        g = out.reshape(-1, 4, 4)
    T = int(reach_tail_length) if use_standoff else 1
    st = torch.eye(4, **f64).repeat(T, 1, 1)
    if use_standoff:
        st[:, 2, 3] = torch.as_tensor(-standoff_dist * np.linspace(0, 1, T, endpoint=False), **f64)
    return torch.matmul(g[:, None], st[None])  # [G', T, 4, 4]: standoff_grasp_global transposed


def pose_rows(poses: torch.Tensor) -> torch.Tensor:
    """[..., 4, 4] -> [..., 12]: rotation rows, translation (the omgx_pose_table layout omgx_goal_ik reads)."""
    return torch.cat([poses[..., :3, :3].reshape(*poses.shape[:-2], 9), poses[..., :3, 3]], dim=-1).contiguous()


def ik_seeds(start, ik_seed_num=12, one_trial=False):
    """[traj.start[:7]] + util_anchor_seeds[:ik_seed_num, :7] (planner.py:314-320); one_trial: the start only."""
    start = np.asarray(start, np.float64)[:7]
    return start[None].copy() if one_trial else np.concatenate([start[None], ANCHOR_SEEDS[:ik_seed_num]], axis=0)


_ROBOT_CACHE: dict = {}


def _robot_blob(model, device):
    key = (id(model), str(device))
    hit = _ROBOT_CACHE.get(key)
    if hit is None or hit[0] is not model:
        hit = (model, ops.robot_blob(model, device))
        _ROBOT_CACHE[key] = hit
    return hit[1]


def _flat_targets(grasp_poses, object_poses, cfg, obj_coord, z_upsample, y_upsample, device):
    parts, begin = [], [0]
    for s, pg in enumerate(grasp_poses):
        pg = np.asarray(pg, np.float64).reshape(-1, 4, 4) if not isinstance(pg, torch.Tensor) else pg
        if pg.shape[0] == 0:
            begin.append(begin[-1])
            continue
        p = prepare_poses(pg, object_poses[s], obj_coord, z_upsample, y_upsample, cfg.reach_tail_length, cfg.standoff_dist,
                          cfg.use_standoff, device)
        parts.append(pose_rows(p))
        begin.append(begin[-1] + p.shape[0])
    T = int(cfg.reach_tail_length) if cfg.use_standoff else 1
    tg = torch.cat(parts) if parts else torch.zeros((0, T, 12), dtype=torch.float64, device=device)
    return tg.contiguous(), np.asarray(begin, np.int64)


def _check_cfg(cfg):
    if getattr(cfg, "increment_iks", False):
        raise ValueError("increment_iks = True is not supported: it draws extra seeds from np.random (planner.py:367-374, 437-442)")


def solve_raw(model, grasp_poses, object_poses, starts, cfg, attached=False, obj_coord=True, z_upsample=False, y_upsample=None,
              one_trial=False, parallel=None, device="cuda:0", max_iter=100, eps=1e-6, pinv_eps=1e-5, accept_diff=2.0):
    """Pose preparation + omgx_goal_ik + compaction: Planner.solve_goal_set_ik for S targets at once.
    Returns a namespace: goals [M,9], reach [M,T,9] (T = 1 without standoff) in the reference's order, scene [M] (int64), counts [S],
    failed [S] (grasps without an accepted chain: the reference's `failed_ik`), and the raw kernel outputs (status, solutions)."""
    _check_cfg(cfg)
    y_upsample = cfg.y_upsample if y_upsample is None else y_upsample
    parallel = cfg.ik_parallel if parallel is None else parallel
    S = len(grasp_poses)
    object_poses = np.asarray(object_poses, np.float64).reshape(S, 4, 4)
    starts = np.asarray(starts, np.float64).reshape(S, -1)
    targets, begin = _flat_targets(grasp_poses, object_poses, cfg, obj_coord, z_upsample, y_upsample, device)
    seeds = torch.as_tensor(np.stack([ik_seeds(starts[s], cfg.ik_seed_num, one_trial) for s in range(S)]) if S else
                            np.zeros((0, 1, 7)), dtype=torch.float64, device=device).contiguous()
    status, sols, _ = ops.goal_ik(_robot_blob(model, device), model.points_per_link, targets, begin, seeds, cfg.use_standoff,
                                  attached, max_iter, eps, pinv_eps, accept_diff)
    N, K = status.shape
    bt = torch.as_tensor(begin, device=device)
    grasp_scene = torch.repeat_interleave(torch.arange(S, device=device), bt[1:] - bt[:-1])      # [N]
    solved = torch.ones(N, dtype=torch.bool, device=device)
    if parallel:  # range(i, min(i + 4, num - 1)): the last grasp of every target is never solved
        last = bt[1:][bt[1:] > bt[:-1]] - 1
        solved[last] = False
    acc = (status == STATUS_ACCEPTED) & solved[:, None]
    failed = torch.zeros(S, dtype=torch.int64, device=device).index_add_(0, grasp_scene, (solved & ~acc.any(1)).long())
    idx = acc.reshape(-1).nonzero().squeeze(1)                                          # the prefix sum over accepted chains
    sel = sols.reshape(N * K, *sols.shape[2:])[idx]                                     # [M, T, 7] in pose order
    T = sel.shape[1]
    fingers = torch.full((sel.shape[0], T, 2), FINGER, dtype=torch.float64, device=device)
    if cfg.use_standoff:
        reach = torch.cat([sel if attached else sel.flip(1), fingers], dim=-1)
        goals = torch.cat([sel[:, T - 1], fingers[:, 0]], dim=-1)  # standoff_iks[0] after the reversal / [-1] attached: pose T-1
    else:
        reach = torch.cat([sel, fingers], dim=-1)
        goals = reach[:, 0].clone()
    scene = grasp_scene[idx // K]
    counts = torch.bincount(scene, minlength=S)
    return SimpleNamespace(goals=goals, reach=reach, scene=scene, counts=counts, failed=failed, status=status, solutions=sols,
                           begin=begin)


def flip_grasp(grasps, padding=0.2):
    """Planner.flip_grasp (planner.py:224-237) on [..., 9] tensors: joint 7 (index -3) +pi where negative, -pi where positive;
    the mask keeps flips strictly inside +-(2.8973 - padding)."""
    g = grasps.clone()
    j = g[..., -3]
    g[..., -3] = torch.where(j < 0, j + np.pi, torch.where(j > 0, j - np.pi, j))
    lim = (g[..., -3] < 2.8973 - padding) & (g[..., -3] > -2.8973 + padding)
    return g, lim


def _hand_rotation(model, device, configs):
    poses, _, _ = ops.forward_kinematics(_robot_blob(model, device), model.points_per_link, configs.contiguous(), want_joint_info=False)
    return poses[:, 7, :3, :3]


def post_process(model, raw, starts, cfg, attached=False, device="cuda:0"):
    """solve_and_process_ik's augmentation and filter (planner.py:249-294) for every scene at once.  Returns (goals [M2,9],
    reach [M2,T,9], scene [M2]) in the reference's order: per scene its goals, then their kept flips, minus the filtered."""
    goals, reach, scene = raw.goals, raw.reach, raw.scene
    M = goals.shape[0]
    if M == 0 or attached:
        return goals, reach, scene
    order_key = scene * (2 * M) + torch.arange(M, device=device)
    if cfg.augment_flip_grasp:
        fg, mask = flip_grasp(goals, cfg.soft_joint_limit_padding)
        fr, _ = flip_grasp(reach, cfg.soft_joint_limit_padding)
        keep = mask.nonzero().squeeze(1)
        goals = torch.cat([goals, fg[keep]])
        reach = torch.cat([reach, fr[keep]])
        scene_f = scene[keep]
        order_key = torch.cat([order_key, scene_f * (2 * M) + M + keep])
        scene = torch.cat([scene, scene_f])
        perm = torch.argsort(order_key)
        goals, reach, scene = goals[perm], reach[perm], scene[perm]
    if cfg.remove_flip_grasp:
        starts_t = torch.as_tensor(np.asarray(starts, np.float64), device=device)
        start_R = _hand_rotation(model, device, starts_t)[scene]                           # [M2,3,3]
        if cfg.use_standoff:
            n = 5
            t = torch.as_tensor(np.linspace(0, 1, n + 2)[1:-1], dtype=torch.float64, device=device)
            s0 = starts_t[scene][:, None]
            g1 = reach[:, -1][:, None]
            interp = (g1 - s0) * t[None, :, None] + s0                                    # scipy interp1d "linear" on x = (0, 1)
            R = _hand_rotation(model, device, interp.reshape(-1, 9)).reshape(-1, n, 3, 3)
        else:
            R = _hand_rotation(model, device, goals).reshape(-1, 1, 3, 3)
        Rd = torch.matmul(R, start_R[:, None].transpose(-1, -2))
        tr = Rd[..., 0, 0] + Rd[..., 1, 1] + Rd[..., 2, 2]
        angle = torch.abs(torch.arccos((tr - 1) / 2)) * 180 / np.pi
        rot = angle > cfg.target_hand_filter_angle                                          # NaN compares False: kept
        x = R[..., :3, 0]
        xz = x[..., 2] / torch.sqrt((x * x).sum(-1))
        drop = (rot | (xz < -0.3)).any(-1)
        keep = (~drop).nonzero().squeeze(1)
        goals, reach, scene = goals[keep], reach[keep], scene[keep]
    return goals, reach, scene


def _pad(goals, reach, scene, S, device):
    counts = torch.bincount(scene, minlength=S) if scene.numel() else torch.zeros(S, dtype=torch.int64, device=device)
    G = int(counts.max().item()) if S else 0
    first = torch.cumsum(counts, 0) - counts
    slot = torch.arange(scene.numel(), device=device) - first[scene]
    gs = torch.zeros((S, G, 9), dtype=torch.float64, device=device)
    rs = torch.zeros((S, G) + tuple(reach.shape[1:]), dtype=torch.float64, device=device)
    gs[scene, slot] = goals
    rs[scene, slot] = reach
    return gs, rs, counts


def solve_goal_sets(model, grasp_poses, object_poses, starts, cfg, attached=False, obj_coord=True, z_upsample=False, y_upsample=None,
                    one_trial=False, parallel=None, device="cuda:0", max_iter=100, eps=1e-6, pinv_eps=1e-5, accept_diff=2.0):
    """Goal sets of S scenes from their grasp poses, on the device.

    model: PandaModel; grasp_poses: S arrays [G_s,4,4] (ragged, G_s may be 0) in the object frame (obj_coord) or the world's;
    object_poses [S,4,4]; starts [S,9] (traj.start: the first seed and the filter's reference); cfg: Config (use_standoff,
    reach_tail_length, standoff_dist, ik_seed_num, ik_parallel, y_upsample, augment_flip_grasp, remove_flip_grasp,
    target_hand_filter_angle, soft_joint_limit_padding).
    Returns (goal_set [S,G,9], reach_grasps [S,G,T,9], goal_counts [S] int64, failed [S] int64), padded with zeros beyond
    goal_counts[s]; T = reach_tail_length with standoff, 1 without."""
    raw = solve_raw(model, grasp_poses, object_poses, starts, cfg, attached, obj_coord, z_upsample, y_upsample, one_trial, parallel,
                    device, max_iter, eps, pinv_eps, accept_diff)
    goals, reach, scene = post_process(model, raw, starts, cfg, attached, device)
    gs, rs, counts = _pad(goals, reach, scene, len(grasp_poses), device)
    return gs, rs, counts, raw.failed


# ---- drop-ins with the reference's signatures -------------------------------------------------------------------

def quat2mat(q):
    """transforms3d.quaternions.quat2mat (w, x, y, z), as omg.util.unpack_pose uses it."""
    w, x, y, z = q
    Nq = w * w + x * x + y * y + z * z
    if Nq < np.finfo(np.float64).eps:
        return np.eye(3)
    s = 2.0 / Nq
    X, Y, Z = x * s, y * s, z * s
    wX, wY, wZ = w * X, w * Y, w * Z
    xX, xY, xZ = x * X, x * Y, x * Z
    yY, yZ, zZ = y * Y, y * Z, z * Z
    return np.array([[1.0 - (yY + zZ), xY - wZ, xZ + wY], [xY + wZ, 1.0 - (xX + zZ), yZ - wX], [xZ - wY, yZ + wX, 1.0 - (xX + yY)]])


def unpack_pose(pose):
    out = np.eye(4)
    out[:3, :3] = quat2mat(pose[3:])
    out[:3, 3] = pose[:3]
    return out


def _model_for(planner):
    m = getattr(planner, "_goal_ik_model", None)
    if m is None:
        m = rb.PandaModel(soft_joint_limit_padding=planner.cfg.soft_joint_limit_padding)
        planner._goal_ik_model = m
    return m


def _device_for(planner):
    return getattr(planner, "goal_ik_device", "cuda:0")


def solve_goal_set_ik(planner, target_obj, env, pose_grasp, one_trial=False, z_upsample=False, y_upsample=False, obj_coord=True):
    """Planner.solve_goal_set_ik (planner.py:296-455) on the device: (reach_goal_set, standoff_goal_set) as lists of numpy arrays."""
    cfg = planner.cfg
    dev = _device_for(planner)
    raw = solve_raw(_model_for(planner), [np.asarray(pose_grasp, np.float64)], unpack_pose(np.asarray(target_obj.pose))[None],
                    np.asarray(planner.traj.start, np.float64)[None], cfg, bool(target_obj.attached), obj_coord, z_upsample,
                    y_upsample, one_trial, cfg.ik_parallel, dev)
    reach = raw.reach.cpu().numpy()
    if not cfg.use_standoff:
        reach = reach[:, 0]
    return list(reach), list(raw.goals.cpu().numpy())


def solve_and_process_ik(planner, target_obj, pose_grasp, z_upsample, obj_coord=True):
    """Planner.solve_and_process_ik (planner.py:239-294) on the device: sets target_obj.reach_grasps / grasps / grasp_potentials
    with the reference's container types (arrays after the flip step, lists after the filter)."""
    cfg = planner.cfg
    dev = _device_for(planner)
    model = _model_for(planner)
    attached = bool(target_obj.attached)
    raw = solve_raw(model, [np.asarray(pose_grasp, np.float64)], unpack_pose(np.asarray(target_obj.pose))[None],
                    np.asarray(planner.traj.start, np.float64)[None], cfg, attached, obj_coord, z_upsample, cfg.y_upsample, False,
                    cfg.ik_parallel, dev)
    start = np.asarray(planner.traj.start, np.float64)[None]
    goals, reach, _ = post_process(model, raw, start, cfg, attached, dev)
    reach = reach.cpu().numpy()
    if not cfg.use_standoff:
        reach = reach[:, 0]
    goals = goals.cpu().numpy()
    target_obj.grasp_potentials = []
    if cfg.remove_flip_grasp and len(goals) > 0 and not attached:
        target_obj.reach_grasps, target_obj.grasps = list(reach), list(goals)
    else:
        target_obj.reach_grasps, target_obj.grasps = reach, goals
