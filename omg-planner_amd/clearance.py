"""Plan clearance: how far the arm's spheres stay from the volumes of a scene table along a plan, at the waypoints and between
them.  The specification of omgx_sphere_clearance / omgx_self_clearance (include/omg_hip.h section 24; csrc/omg_clearance_body.h
follows it operation by operation) and of DeviceScenes.plan_clearance's report, in plain numpy.

CHOMP's own evidence (OMGX_INFO_COLLIDE) is a hinge on 15 points per link at the n waypoints.  Between two waypoints the hand
moves centimetres, so a thin obstacle can lie between them.  Here the plan is sampled K times per segment in joint space
(dense_configs), the arm's spheres (ops.RobotSpheres, the links of omgx_forward_kinematics) are moved to every sample
(world_spheres), and every sphere is held against the trilinear interpolant of every used record's volume (sphere_clearance:
volume_camera.sample, the lines registration.value_gradient and the depth camera read).  Outside a grid the value at the nearest
point of the grid minus the distance to it is a Lipschitz lower bound; further than `beyond` from a grid the volume says nothing.
self_clearance holds the spheres of one sample against one another.  plan_report turns the samples into a statement about the
whole motion:

  A sphere centre on link l moves at most len_l = sum_j rho[l][j] * |dq_j| over a linear joint-space segment (reach_table: a
  point's speed is at most sum_j |qdot_j| * its distance from the axis of joint j).  With K samples per segment every point of
  the motion lies within half = (len_l / K) / 2 of a sample.  The margin of a sample is its clearance with every radius grown by
  half + slack.  A segment is CERTIFIED when the margin of all its K + 1 samples is > 0 and r_max + max_l half + slack <= beyond
  (so that a pair left out because it is further than `beyond` from the grid is free as well: an object lies inside its grid).
  If every used record's volume is within `slack` of a lower bound of the true distance to its object, a certified segment
  touches no used object anywhere along it.  `slack` is the caller's statement about their volumes (fused volumes measure to
  voxel centres: at most (sqrt 3 / 2) delta coarse; analytic and mesh volumes are exact at the samples and off by the
  interpolation error between them).  Not certified is not "collides": take a larger K.

Everything is float64, every operation rounded on its own, dot products written (a*x + b*y) + c*z, with + - * /, sqrt, comparisons
and float-to-int conversion only, so that the device can equal the bits.  Rejections are negated comparisons: NaN falls on the
"no" side.  Not part of the contract: capsules and link meshes, per-scene sphere sets (a grasped object's spheres go on link 7
of the one RobotSpheres), swept volumes of the obstacles, time parameterisation, conservative advancement.
"""
from __future__ import annotations

import numpy as np

from . import _lib, robot_filter as _rf, volume_camera as _vc

NUM_LINKS, NUM_DOF = 10, 9
MAX_SELF = _lib.CONSTANTS["OMGX_CLEARANCE_MAX_SELF"]  # the most spheres of self_clearance


def dense_configs(traj, K: int) -> np.ndarray:
    """traj [S,n,9], K >= 1 -> q [S,T,9], T = (n-1)*K + 1.  Sample i*K + k (0 <= k < K) is a + (b - a) * (k / K) with
    a = traj[s,i], b = traj[s,i+1]; for k = 0 it is a itself, and the last sample is traj[s,n-1] itself."""
    traj, K = np.asarray(traj, np.float64), int(K)
    if traj.ndim != 3 or traj.shape[2] != NUM_DOF or traj.shape[1] < 1:
        raise ValueError(f"traj must be [S,n,{NUM_DOF}] with n >= 1, got {traj.shape}")
    if K < 1:
        raise ValueError(f"K must be >= 1, got {K}")
    S, n = traj.shape[:2]
    q = np.empty((S, (n - 1) * K + 1, NUM_DOF))
    a, b = traj[:, :-1, None, :], traj[:, 1:, None, :]
    w = (np.arange(K, dtype=np.float64) / float(K)).reshape(1, 1, K, 1)
    with np.errstate(all="ignore"):
        seg = a + (b - a) * w
    seg[:, :, 0, :] = traj[:, :-1]
    q[:, :-1] = seg.reshape(S, (n - 1) * K, NUM_DOF)
    q[:, -1] = traj[:, -1]
    return q


def reach_table(model, local, link, finger_travel: float) -> np.ndarray:
    """rho [10,9]: rho[l][j] bounds the distance of any sphere centre on link l from the axis of joint j; 0 where joint j does not
    move link l.  a_i = |pose_0[i][:3,3]|; c_l = the largest |center_offset[l] applied to the local centre| over the spheres of
    link l (0 without spheres).  Revolute j <= 6, l >= j: sum_{i=j+1..min(l,6)} a_i + [l>=7] a_7 + [l>=8] (a_l + finger_travel) +
    c_l.  The prismatic fingers: rho[8][7] = rho[9][8] = 1.  finger_travel: the largest |q_7|, |q_8| of the plans."""
    local, link = _rf._spheres(local, link)
    finger_travel = float(finger_travel)
    if not (np.isfinite(finger_travel) and finger_travel >= 0):
        raise ValueError("finger_travel must be finite and not negative")
    a = np.linalg.norm(np.asarray(model.pose_0, np.float64)[:, :3, 3], axis=1)
    co = np.asarray(model.center_offset, np.float64)
    c = np.zeros(NUM_LINKS)
    for l in range(NUM_LINKS):
        p = local[link == l, :3]
        if len(p):
            c[l] = np.linalg.norm(p @ co[l, :3, :3].T + co[l, :3, 3], axis=1).max()
    rho = np.zeros((NUM_LINKS, NUM_DOF))
    for l in range(NUM_LINKS):
        for j in range(min(l, 6) + 1):
            r = sum(a[i] for i in range(j + 1, min(l, 6) + 1))
            if l >= 7:
                r += a[7]
            if l >= 8:
                r += a[l] + finger_travel
            rho[l, j] = r + c[l]
    rho[8, 7] = rho[9, 8] = 1.0
    return rho


def _poses(link_poses):
    poses = np.asarray(link_poses, np.float64)
    if poses.ndim != 4 or poses.shape[1:] != (NUM_LINKS, 4, 4):
        raise ValueError(f"link_poses must be [B,{NUM_LINKS},4,4], got {poses.shape}")
    return poses


def world_spheres(link_poses, local, link) -> np.ndarray:
    """The spheres of every configuration in the world -> [B,N,4]: with P = link_poses[b, link[n]] and p = local[n][:3],
    w_k = ((P[k,0]*p0 + P[k,1]*p1) + P[k,2]*p2) + P[k,3] (robot_filter.camera_spheres's w), and the radius unchanged."""
    local, link = _rf._spheres(local, link)
    poses = _poses(link_poses)
    out = np.zeros((len(poses), len(local), 4))
    p = local[:, :3]
    with np.errstate(all="ignore"):
        for b in range(len(poses)):
            P = poses[b, link]
            for k in range(3):
                out[b, :, k] = ((P[:, k, 0] * p[:, 0] + P[:, k, 1] * p[:, 1]) + P[:, k, 2] * p[:, 2]) + P[:, k, 3]
            out[b, :, 3] = local[:, 3]
    return out


def _pad(pad, B):
    if pad is None:
        return None
    pad = np.asarray(pad, np.float64)
    if pad.shape != (B, NUM_LINKS):
        raise ValueError(f"pad must be [{B},{NUM_LINKS}], got {pad.shape}")
    return pad


def _best(cand):
    """The replace rule over cand [N,K]: the smallest value, the lowest (n, k) on a tie; NaN and +inf never win -> (value, n, k)."""
    if cand.size == 0:
        return np.inf, -1, -1
    c = np.where(np.isnan(cand), np.inf, cand)
    at = int(np.argmin(c))  # (the first of the smallest in row-major order: the lowest (n, k))
    v = c.reshape(-1)[at]
    return (np.inf, -1, -1) if v == np.inf else (float(v), at // cand.shape[1], at % cand.shape[1])


def check_table(objects, scene_begin, pool_elems: int, visible):
    """The records, ranges and flags of sphere_clearance (ValueError) -> (objects, scene_begin int64 [S+1], used bool [n]).  A
    record is used when visible[k] != 0; visible None: when its `disabled` is 0.  A used record of a scene needs two samples per
    axis, a finite inv_delta > 0 and a grid inside the pool of pool_elems elements."""
    from . import scenes as _sc
    objects = np.asarray(objects)
    if objects.dtype != _sc.OBJECT_DTYPE or objects.ndim != 1:
        raise ValueError("objects must be a 1-d array of scenes.OBJECT_DTYPE records")
    begin = np.asarray(scene_begin, np.int64).reshape(-1)
    n = len(objects)
    if len(begin) < 1 or begin[0] < 0 or (np.diff(begin) < 0).any() or begin[-1] > n:
        raise ValueError(f"scene_begin must be [S+1], ascending, inside the {n} records")
    if visible is None:
        used = objects["disabled"] == 0
    else:
        used = np.asarray(visible).reshape(-1) != 0
        if len(used) != n:
            raise ValueError(f"visible must have one flag per record ({n}), got {len(used)}")
    at = np.arange(int(begin[0]), int(begin[-1]))
    at = at[used[at]]
    r = objects[at]
    dims, off = r["dim"].astype(np.int64), r["grid_offset"].astype(np.int64)
    with np.errstate(invalid="ignore"):
        bad = (dims < 2).any(axis=1) | ~(np.isfinite(r["inv_delta"]) & (r["inv_delta"] > 0))
    if bad.any():
        raise ValueError(f"object {int(at[bad][0])}: every axis needs two samples and inv_delta must be finite and positive")
    bad = (off < 0) | (off + dims.prod(axis=1) > int(pool_elems))
    if bad.any():
        raise ValueError(f"object {int(at[bad][0])}: the grid leaves the pool of {int(pool_elems)} elements")
    return objects, begin, used


def pair_distances(obj, pool, w):
    """One record against the centres w [n,3] -> (e [n], d [n]).  With P = pose_inv widened to float64:
    q_a = ((P[4a]*w0 + P[4a+1]*w1) + P[4a+2]*w2) + P[4a+3];  u_a = (q_a - float64(lo_a)) * inv_delta - 0.5;  c_a = u_a clamped as
    volume_camera.sample clamps it (!(u >= 0): 0; u > dim_a - 1: dim_a - 1);  x_a = u_a - c_a;
    e = sqrt((x0*x0 + x1*x1) + x2*x2) / inv_delta;  d = v(c) - e with v the interpolant of volume_camera.sample."""
    grid = _vc._Grid(obj)
    P = np.asarray(obj["pose_inv"], np.float32).astype(np.float64).reshape(12)
    with np.errstate(all="ignore"):
        q = [((P[4 * a] * w[:, 0] + P[4 * a + 1] * w[:, 1]) + P[4 * a + 2] * w[:, 2]) + P[4 * a + 3] for a in range(3)]
        u = [(q[a] - grid.lo[a]) * grid.inv_delta - 0.5 for a in range(3)]
        x = []
        for a in range(3):
            c = np.where(u[a] >= 0.0, u[a], 0.0)
            c = np.where(c > grid.hi[a], grid.hi[a], c)
            x.append(u[a] - c)
        e = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) / grid.inv_delta
        zero = np.zeros(len(w))
        v, _ = _vc.sample(grid, pool, u, [zero, zero, zero], 0.0)
        return e, v - e


def sphere_clearance(objects, scene_begin, pool, visible, scene_of_config, world, link, pad, beyond: float):
    """The clearance of B configurations -> (clear [B], clear_sphere [B], clear_object [B], margin [B], margin_sphere [B],
    margin_object [B]); float64 and int32; the margin outputs are None with pad=None.  Configuration b stands in scene
    scene_of_config[b]; world [B,N,4] (world_spheres); link [N]; pad [B,10] >= 0 or None; beyond finite, >= 0.  For sphere n and
    the scene's used records k = 0, 1, ... (pair_distances): the pair contributes iff e <= beyond; its candidates are d - r_n for
    clear and d - (r_n + pad[b][link_n]) for margin.  A candidate replaces the best iff it is < the best, or == the best with a
    smaller (n, k); NaN never wins; when nothing contributes the result is (+inf, -1, -1).  The object index is local to the
    scene."""
    pool = np.asarray(pool)
    if pool.dtype != np.float32 or pool.ndim != 1:
        raise ValueError("pool must be a 1-d float32 array")
    objects, begin, used = check_table(objects, scene_begin, pool.size, visible)
    world = np.asarray(world, np.float64)
    if world.ndim != 3 or world.shape[2] != 4:
        raise ValueError(f"world must be [B,N,4], got {world.shape}")
    B, N = world.shape[:2]
    link = np.asarray(link, np.int64).reshape(-1)
    if len(link) != N or (N and (link.min() < 0 or link.max() >= NUM_LINKS)):
        raise ValueError(f"link must be [{N}] in 0..{NUM_LINKS - 1}")
    cfg = np.asarray(scene_of_config, np.int64).reshape(-1)
    S = len(begin) - 1
    if len(cfg) != B or (B and (cfg.min() < 0 or cfg.max() >= S)):
        raise ValueError(f"scene_of_config must be [{B}] in [0, {S})")
    beyond = float(beyond)
    if not (np.isfinite(beyond) and beyond >= 0):
        raise ValueError("beyond must be finite and not negative")
    with np.errstate(invalid="ignore"):
        if N and not (world[:, :, 3] >= 0).all():
            raise ValueError("a radius is negative or not a number")
    pad = _pad(pad, B)
    clear, margin = np.full(B, np.inf), np.full(B, np.inf)
    who = np.full((4, B), -1, np.int32)
    for b in range(B):
        s = int(cfg[b])
        count = int(begin[s + 1] - begin[s])
        cand = np.full((N, count), np.inf)
        with np.errstate(all="ignore"):
            for k in range(count):
                o = int(begin[s]) + k
                if not used[o] or N == 0:
                    continue
                e, d = pair_distances(objects[o], pool, world[b, :, :3])
                cand[:, k] = np.where(e <= beyond, d, np.inf)  # (+inf never wins: left out)
            r = world[b, :, 3:4]
            clear[b], who[0, b], who[1, b] = _best(cand - r)
            if pad is not None:
                margin[b], who[2, b], who[3, b] = _best(cand - (r + pad[b, link][:, None]))
    if pad is None:
        return clear, who[0], who[1], None, None, None
    return clear, who[0], who[1], margin, who[2], who[3]


def self_clearance(world, link, pairs, pad=None):
    """The smallest gap between two spheres of one configuration -> (self_clear [B], i [B], j [B]).  Over i < j with
    pairs[link_i][link_j] != 0: dx = c_i - c_j, dist = sqrt((dx0*dx0 + dx1*dx1) + dx2*dx2),
    cand = dist - ((r_i + pad_i) + (r_j + pad_j)) with pad_n = pad[b][link_n] (0 with pad=None); the replace rule of
    sphere_clearance on (i, j); (+inf, -1, -1) without a pair.  N <= MAX_SELF."""
    world = np.asarray(world, np.float64)
    if world.ndim != 3 or world.shape[2] != 4:
        raise ValueError(f"world must be [B,N,4], got {world.shape}")
    B, N = world.shape[:2]
    if N > MAX_SELF:
        raise ValueError(f"self_clearance takes at most {MAX_SELF} spheres, got {N}")
    link = np.asarray(link, np.int64).reshape(-1)
    if len(link) != N or (N and (link.min() < 0 or link.max() >= NUM_LINKS)):
        raise ValueError(f"link must be [{N}] in 0..{NUM_LINKS - 1}")
    pairs = np.asarray(pairs)
    if pairs.shape != (NUM_LINKS, NUM_LINKS):
        raise ValueError(f"pairs must be [{NUM_LINKS},{NUM_LINKS}], got {pairs.shape}")
    pad = _pad(pad, B)
    out, wi, wj = np.full(B, np.inf), np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    on = (pairs[link][:, link] != 0) & (np.arange(N)[:, None] < np.arange(N)[None, :])
    for b in range(B):
        c = world[b]
        rp = c[:, 3] + (pad[b, link] if pad is not None else 0.0)
        with np.errstate(all="ignore"):
            dx = [c[:, None, a] - c[None, :, a] for a in range(3)]
            dist = np.sqrt((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2])
            cand = np.where(on, dist - (rp[:, None] + rp[None, :]), np.inf)
        out[b], wi[b], wj[b] = _best(cand)
    return out, wi, wj


def segment_halves(traj, K: int, rho) -> np.ndarray:
    """half [S,n-1,10]: len_l = sum over j = 0..8 in order of rho[l][j] * |traj[s,i+1][j] - traj[s,i][j]|, from the first term;
    half = (len_l / K) * 0.5."""
    traj, rho = np.asarray(traj, np.float64), np.asarray(rho, np.float64)
    if rho.shape != (NUM_LINKS, NUM_DOF):
        raise ValueError(f"rho must be [{NUM_LINKS},{NUM_DOF}], got {rho.shape}")
    dq = np.abs(traj[:, 1:] - traj[:, :-1])  # [S,n-1,9]
    length = rho[:, 0] * dq[:, :, 0:1]
    for j in range(1, NUM_DOF):
        length = length + rho[:, j] * dq[:, :, j:j + 1]
    return (length / float(int(K))) * 0.5


def sample_pads(half, K: int, slack: float) -> np.ndarray:
    """pad [S,T,10] of the samples of dense_configs: sample i*K + k has half[s,i] + slack for k > 0; at a waypoint (k = 0) the
    larger of the two adjacent segments' halves (the one there is at either end), + slack.  n = 1: slack alone."""
    half, K, slack = np.asarray(half, np.float64), int(K), float(slack)
    S, m = half.shape[:2]  # m = n - 1
    pad = np.zeros((S, m * K + 1, NUM_LINKS))
    if m:
        pad[:, :-1] = np.repeat(half, K, axis=1)
        way = half.copy()
        way[:, 1:] = np.maximum(half[:, 1:], half[:, :-1])
        pad[:, 0:-1:K] = way
        pad[:, -1] = half[:, -1]
    return pad + slack


def plan_report(traj, K: int, rho, r_max: float, slack: float, beyond: float, clear, margin) -> dict:
    """The per-segment and per-plan summary of clear, margin [S,T] (sphere_clearance on dense_configs(traj, K) with the pads of
    sample_pads) -> dict: half [S,n-1,10]; segment_margin [S,n-1]: the min of margin over the samples iK .. (i+1)K;
    certified [S,n-1] = (segment_margin > 0) & ((r_max + max_l half) + slack <= beyond); min_clearance [S]: the min of clear;
    collides [S]: some sample has clear < 0; first_hit [S] int64: the first such sample, or -1; plan_certified [S]: every segment
    certified (n = 1: the one sample's margin > 0 and r_max + slack <= beyond)."""
    traj, K = np.asarray(traj, np.float64), int(K)
    S, n = traj.shape[:2]
    clear, margin = np.asarray(clear, np.float64).reshape(S, -1), np.asarray(margin, np.float64).reshape(S, -1)
    T = (n - 1) * K + 1
    if clear.shape[1] != T or margin.shape[1] != T:
        raise ValueError(f"clear and margin must be [{S},{T}]")
    half = segment_halves(traj, K, rho)
    seg = np.minimum(margin[:, :-1].reshape(S, n - 1, K).min(axis=2) if n > 1 else np.zeros((S, 0)), margin[:, K::K][:, : n - 1])
    reach = (float(r_max) + (half.max(axis=2) if n > 1 else np.zeros((S, 0)))) + float(slack) <= float(beyond)
    certified = (seg > 0.0) & reach
    hit = clear < 0.0
    first = np.where(hit.any(axis=1), hit.argmax(axis=1), -1).astype(np.int64)
    whole = certified.all(axis=1) if n > 1 else (margin[:, 0] > 0.0) & (float(r_max) + float(slack) <= float(beyond))
    return dict(half=half, segment_margin=seg, certified=certified, min_clearance=clear.min(axis=1), collides=hit.any(axis=1),
                first_hit=first, plan_certified=whole)
