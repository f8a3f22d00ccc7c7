"""From grasp poses to plans for S grasping scenes on the device: the reference's PlanningScene.step (omg/core.py:694-699) after
Planner.__init__'s goal pipeline (planner.py:104-115) — IK (`goal_ik.solve_goal_sets`), the scene table
(`ops.DeviceScenes.from_scenes`), the goal-set set-up (`goalset.setup_goal_sets`), grasp_init's goal set (planner.py:188-199)
and the batched planner (`ChompEngine`).

Grasping only: the engine holds one robot blob for all scenes, so it cannot carry per-scene attached-object points; a scene
whose objects include an attached one is refused.

Deviation kept from the engine (not from this module): with ol_alg "Baseline" the initial goal is cfg.goal_idx (or goal 0),
where the reference's Learner.__init__ (online_learner.py:94-102) takes argmin(cost_vector) whenever reach grasps exist.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, goal_ik, goalset, ops
from .engine import ChompEngine


@dataclass
class GraspPlans:
    """What plan_grasps returns (device tensors unless noted).  Rows of scenes that were not planned hold zeros (traj), NaN
    (info) and -1 (goal_idx)."""
    traj: torch.Tensor            # [S, n, 9] f64: the final trajectories
    info: torch.Tensor            # [S, 16] f64: the final info rows (ChompEngine.plan)
    goal_idx: torch.Tensor        # [S] int32: the goal each plan ends at, an index into goal_set
    goal_set: torch.Tensor        # [S, K, 9] f64: the goal sets planned towards (grasp_init: reach[:, :, -1] under use_standoff)
    grasps: torch.Tensor          # [S, K, 9] f64: the selected goals (setup_goal_sets), padded with zeros
    reach_grasps: torch.Tensor    # [S, K, T, 9] f64
    potentials: torch.Tensor      # [S, K] f32
    goal_counts: np.ndarray       # [S] int64 (host): goals per scene after the draw
    num_free: np.ndarray          # [S] (host): goals that passed the collision filter
    num_candidates: np.ndarray    # [S] (host): goals the draw chose from (0: "IK FAIL")
    planned: np.ndarray           # [S] bool (host): False for scenes without goals ("planning not run")
    engine: "ChompEngine | None"  # the engine over the planned scenes (None when no scene was planned)


def plan_grasps(model, scenes, grasp_poses, starts, cfg, ol_alg=None, rng=np.random, obj_coord=True, device="cuda:0",
                layout_scenes: "int | None" = None) -> GraspPlans:
    """Plans for S grasping scenes from their grasp poses.

    model: PandaModel; scenes: S scenes.Scene (the target object of each gives the object pose); grasp_poses: S arrays [G_s,4,4]
    (ragged, may be empty) in the target's frame (obj_coord) or the world's; starts [S,9]; cfg: Config.  ol_alg: default
    cfg.ol_alg.  rng: the stream the goal draw consumes (np.random, as the reference).  Scenes whose goal sets come out empty are
    not planned (the reference prints "planning not run"); the engine runs over the other scenes with its layout evaluated for
    `layout_scenes` (default S), so a goal-less scene changes no other scene's bits."""
    dev = torch.device(device)
    S = len(scenes)
    if any(ob.attached for sc_ in scenes for ob in sc_.objects):
        raise ValueError("plan_grasps plans grasps only: a scene with an attached object needs per-scene robot points")
    if len(grasp_poses) != S:
        raise ValueError("grasp_poses must hold one array per scene")
    starts = np.ascontiguousarray(np.asarray(starts, np.float64).reshape(S, 9))
    objs = np.stack([np.asarray(sc_.objects[sc_.target_idx].pose_mat, np.float64) for sc_ in scenes]) if S else np.zeros((0, 4, 4))
    gs, rs, counts, _ = goal_ik.solve_goal_sets(model, grasp_poses, objs, starts, cfg, attached=False, obj_coord=obj_coord, device=dev)
    table = ops.DeviceScenes.from_scenes(scenes, cfg.layer_kwargs(), device=dev)
    robot = ops.robot_blob(model, dev)
    grasps, reach, pot, k, nfree, ncand = goalset.setup_goal_sets(robot, model.points_per_link, table, gs, rs, counts, cfg, rng=rng)
    goals = reach[:, :, -1].contiguous() if (cfg.goal_set_proj and cfg.use_standoff) else grasps
    planned = k > 0
    idx = np.flatnonzero(planned)
    if not getattr(cfg, "silent", False):
        for s in np.flatnonzero(~planned):
            print(f"scene {s}: planning not run...")
    n = cfg.timesteps
    traj = torch.zeros((S, n, 9), dtype=torch.float64, device=dev)
    info = torch.full((S, _lib.INFO_STRIDE), float("nan"), dtype=torch.float64, device=dev)
    goal_idx = torch.full((S,), -1, dtype=torch.int32, device=dev)
    eng = None
    if idx.size:
        sub = table if idx.size == S else ops.DeviceScenes.from_scenes([scenes[i] for i in idx], cfg.layer_kwargs(), device=dev)
        sel = torch.from_numpy(idx).to(dev)
        kw = dict(reach_grasps=reach.index_select(0, sel).cpu().numpy()) if cfg.use_standoff else {}
        eng = ChompEngine.auto(model, sub, cfg, starts[idx], goals.index_select(0, sel).cpu().numpy(),
                               layout_scenes=S if layout_scenes is None else int(layout_scenes), for_plan=True,
                               goal_counts=k[idx], device=dev, ol_alg=ol_alg or cfg.ol_alg, **kw)
        out = eng.plan()
        traj.index_copy_(0, sel, eng.traj)
        info.index_copy_(0, sel, out)
        goal_idx.index_copy_(0, sel, eng.goal_idx)
    return GraspPlans(traj, info, goal_idx, goals, grasps, reach, pot, k, nfree, ncand, planned, eng)


def plan_meshes(model, scenes, meshes, starts, cfg, n_rays: int = 512, n_angles: int = 8, ol_alg=None, rng=np.random,
                grasp_rng=None, max_grasps=None, device="cuda:0", layout_scenes: "int | None" = None, **grasp_kwargs):
    """Plans for S grasping scenes from the triangle meshes of their targets: grasps.sample_grasp_sets on the device (one ray-cast
    launch and one pose launch for all scenes, the target's own volume as the gripper check), then plan_grasps unchanged.

    meshes: S (verts, faces) in the frame of the target object's volume (scenes[s].objects[target_idx].sdf, voxel centres).
    grasp_rng: the stream the sampler consumes (default np.random.RandomState(0)), or a list of S; rng: the stream plan_grasps'
    goal draw consumes.  grasp_kwargs: sample_grasp_sets' parameters (cone, max_width, clearance, probe, chunks, ...).  The
    targets' volumes are uploaded for the sampler and again by plan_grasps for its scene table (it builds its own).
    -> (GraspPlans, grasp poses: S arrays [G_s,4,4] in the targets' frames)."""
    from . import grasps as _gr
    if len(meshes) != len(scenes):
        raise ValueError("meshes must hold one (verts, faces) per scene")
    grids = [sc_.objects[sc_.target_idx].sdf for sc_ in scenes]
    sets = _gr.sample_grasp_sets(meshes, grids, n_rays, n_angles, np.random.RandomState(0) if grasp_rng is None else grasp_rng,
                                 max_grasps=max_grasps, device=device, **grasp_kwargs)
    return plan_grasps(model, scenes, sets, starts, cfg, ol_alg=ol_alg, rng=rng, obj_coord=True, device=device, layout_scenes=layout_scenes), sets


def plan_volumes(model, scenes, starts, cfg, level: float = 0.0, n_rays: int = 512, n_angles: int = 8, ol_alg=None, rng=np.random,
                 grasp_rng=None, max_grasps=None, device="cuda:0", layout_scenes: "int | None" = None, **grasp_kwargs):
    """plan_meshes without meshes: the targets exist only as distance volumes.  The scene table is built
    (ops.DeviceScenes.from_scenes), the level set {v = level} of every target's volume is extracted from the table's own pool on
    the device (DeviceScenes.object_surfaces) and downloaded once, grasps.sample_grasp_sets samples grasps on those meshes with
    the same pool as the gripper check, then plan_grasps unchanged (it builds its own table).  level: 0 for a signed volume; a
    small radius for a target that is the unsigned distance to an observed cloud (ops.point_cloud_sdf).  A target whose surface
    is empty or leaves its grid (open edges: the mesh is not closed there) is refused, by scene.  The other arguments are
    plan_meshes'.  -> (GraspPlans, grasp poses: S arrays [G_s,4,4] in the targets' frames, meshes: S (verts, faces) on the host)."""
    from . import grasps as _gr
    dev = torch.device(device)
    if any(ob.attached for sc_ in scenes for ob in sc_.objects):
        raise ValueError("plan_volumes plans grasps only: a scene with an attached object needs per-scene robot points")
    table = ops.DeviceScenes.from_scenes(scenes, cfg.layer_kwargs(), device=dev)
    targets = [int(sc_.target_idx) for sc_ in scenes]
    verts, faces, vrows, frows, open_edges = table.object_surfaces([(s, t) for s, t in enumerate(targets)], level)
    bad = [f"scene {s}: the target's surface at level {level} " + ("is empty" if frows[s, 1] == 0 else f"leaves its grid ({int(open_edges[s])} open edges)")
           for s in range(len(scenes)) if frows[s, 1] == 0 or open_edges[s] > 0]
    if bad:
        raise ValueError("; ".join(bad))
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    meshes = [(hv[vrows[s, 0]: vrows[s, 0] + vrows[s, 1]], hf[frows[s, 0]: frows[s, 0] + frows[s, 1]]) for s in range(len(scenes))]
    sets = _gr.sample_grasp_sets(meshes, table, n_rays, n_angles, np.random.RandomState(0) if grasp_rng is None else grasp_rng,
                                 max_grasps=max_grasps, targets=targets, device=dev, **grasp_kwargs)
    plans = plan_grasps(model, scenes, sets, starts, cfg, ol_alg=ol_alg, rng=rng, obj_coord=True, device=device, layout_scenes=layout_scenes)
    return plans, sets, meshes


def plan_observed(model, scenes, obs, obstacles, layouts, band: float, near: float, reach: float, seeds, min_nodes: int, starts, cfg,
                  connectivity: int = 6, margin=None, free_mask=None, device="cuda:0", robot=None, **plan_kwargs):
    """plan_volumes from depth images alone: no instance labels, no target volume from a file.  obs: a camera.Observation of the
    S scenes (only its depth images and cameras are used); obstacles [S]: the object of each scene that stands for everything
    observed, at the pose of the layout's frame, as the target (scene.target_idx) should be; layouts, band, near, reach, seeds,
    min_nodes, connectivity, margin, free_mask, robot: camera.Observation.segment_obstacles' (robot: the arm in the images,
    camera.Observation.robot_view's result).  A table built from the scenes is segmented
    on the device, the two small volumes of every scene are downloaded into the scenes' SdfGrids (the target's crop, the layout
    without the target), then plan_volumes unchanged (plan_kwargs: its other arguments).
    -> (GraspPlans, grasp poses, meshes, the chosen records [S,8])."""
    from . import fusion as _fu, scenes as _sc, segmentation as _sg
    dev = torch.device(device)
    S = len(scenes)
    tp = [(s, int(scenes[s].target_idx)) for s in range(S)]
    op = [(s, int(o)) for s, o in enumerate(obstacles)]
    # room for every scene's two new volumes: the layout, and a crop that is at most the layout grown by the margin
    grow = 2 * (max(_fu.obstacle_radius(reach, float(delta)) for _, delta, _ in layouts) + 1 if margin is None else int(margin))
    reserve = sum(int(np.prod(dims)) + int(np.prod(np.asarray(dims, np.int64) + grow)) for _, _, dims in layouts)
    table = ops.DeviceScenes.from_scenes(scenes, cfg.layer_kwargs(), device=dev, share_grids=False, reserve_voxels=reserve)
    radius, records, _ = obs.segment_obstacles(table, tp, op, layouts, band, near, reach, seeds, min_nodes, connectivity, margin, free_mask,
                                                robot=robot)
    for s, (origin, delta, _) in enumerate(layouts):
        crop = _sg.crop_layout((origin, delta), records[s], radius + 1 if margin is None else int(margin))
        # (origins and delta as the host knows them in float64, not the records' float32 limits)
        for (_, o), org in ((tp[s], crop[0]), (op[s], np.asarray(origin, np.float64))):
            scenes[s].objects[o].sdf = _sc.SdfGrid(table.volume(s, o).cpu().numpy(), org, float(delta))
    plans, sets, meshes = plan_volumes(model, scenes, starts, cfg, device=device, **plan_kwargs)
    return plans, sets, meshes, records


def plan_on_unknown_support(model, scenes, obs, obstacles, supports, layouts, support_layouts, band: float, near: float, reach: float, seeds,
                            min_nodes: int, starts, cfg, triples, tol: float, up_world=None, cos_min: float = -1.0, refine: int = 2,
                            connectivity: int = 6, margin=None, device="cuda:0", robot=None, **plan_kwargs):
    """plan_observed on a support nobody has modelled: from depth images and seed points alone.  The support's plane is fitted to
    every scene's depth image (camera.Observation.fit_supports: triples, tol, up_world, cos_min, refine), its pixels are the
    free_mask that plan_observed takes in place of explained_mask's rendering of a known table, and its half-space becomes the
    volume of supports[s], an object of scene s at the pose of the layout's frame (support_layouts: one (origin [3], delta,
    dims [3]) per scene, voxel centres, in that frame), so that the masked-out support is still an obstacle: the volume is
    written on the device (ops.DeviceScenes.plane_obstacles) and downloaded into the object's SdfGrid as plan_observed downloads
    its two.  Then plan_observed, unchanged.  A scene without a plane is refused.  robot: the
    arm in the images (camera.Observation.robot_view's result): its pixels take no part in the fit, and plan_observed gets it.
    -> (GraspPlans, grasp poses, meshes, the chosen records [S,8], the ops.PlaneFit)."""
    from . import scenes as _sc
    dev = torch.device(device)
    sp = [(s, int(o)) for s, o in enumerate(supports)]
    fit, mask = obs.fit_supports(triples, tol, up_world, cos_min, refine, skip=None if robot is None else robot.mask)
    table = ops.DeviceScenes.from_scenes(scenes, cfg.layer_kwargs(), device=dev, share_grids=False,
                                         reserve_voxels=sum(int(np.prod(dims)) for _, _, dims in support_layouts))
    table.plane_obstacles(sp, obs.support_planes(table, sp, fit), support_layouts)
    for (s, o), (origin, delta, _) in zip(sp, support_layouts):
        scenes[s].objects[o].sdf = _sc.SdfGrid(table.volume(s, o).cpu().numpy(), np.asarray(origin, np.float64), float(delta))
    plans, sets, meshes, records = plan_observed(model, scenes, obs, obstacles, layouts, band, near, reach, seeds, min_nodes, starts, cfg, connectivity,
                                                 margin, free_mask=mask, device=device, robot=robot, **plan_kwargs)
    return plans, sets, meshes, records, fit


def check_plans(model, table, plans: GraspPlans, spheres, substeps: int, skip_targets: bool = True, fingers_touch: bool = True, targets=None,
                **kw) -> "ops.PlanClearance":
    """Are the plans free of the scenes they were planned in, or of a newer table of the same scenes, at the waypoints and between
    them?  DeviceScenes.plan_clearance (clearance.py says what is computed and what a certificate means) on the rows with
    plans.planned -> ops.PlanClearance over all S rows; a row that was not planned says nothing (+inf, -1, False).

    table: an ops.DeviceScenes of the S scenes; spheres: ops.RobotSpheres on the links of forward_kinematics; substeps: samples per
    segment.  The used records are the enabled ones (`disabled` 0 in the table's host mirror), minus each scene's target when
    skip_targets is set: a grasp ends at the target, so its last samples touch it.  targets: one object index per scene, or the
    scenes themselves (their target_idx); needed with skip_targets and to tell which object the plan's end touches.  The arm's own
    links are held against one another by ops.default_self_pairs(fingers_touch) unless pairs= is given (pairs=False: not at all).
    A grasped object is the caller's to add: its spheres go on link 7 of `spheres` (one sphere set for all scenes: per-scene sets
    are not supported).  kw: plan_clearance's slack, beyond, rho, cull; without rho, spheres.reach_table(model) is used."""
    S = table.num_scenes
    if plans.traj.shape[0] != S or len(plans.planned) != S:
        raise ValueError(f"the table has {S} scenes, the plans {plans.traj.shape[0]}")
    visible = table.host_objects["disabled"] == 0
    if skip_targets:
        if targets is None:
            raise ValueError("skip_targets needs targets: one object index per scene, or the scenes")
        for s, t in enumerate(targets):
            visible[table._index(s, int(getattr(t, "target_idx", t)))] = False
    pairs = kw.pop("pairs", None)
    pairs = ops.default_self_pairs(fingers_touch) if pairs is None else None if pairs is False else pairs
    if kw.get("rho") is None and getattr(spheres, "rho", None) is None:
        spheres.reach_table(model)
    idx = np.flatnonzero(np.asarray(plans.planned, bool))
    sel = torch.from_numpy(idx).to(table.device)
    robot = plans.engine.robot if getattr(plans.engine, "robot", None) is not None else ops.robot_blob(model, table.device)
    out = table.plan_clearance(spheres, robot, model.points_per_link, plans.traj.index_select(0, sel).contiguous(), substeps,
                               visible=visible.astype(np.uint8), pairs=pairs, scene_of_plan=idx, **kw)
    return out if len(idx) == S else out.scattered(S, sel)
