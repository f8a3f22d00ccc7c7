"""Tensor-level wrappers over the C ABI.  torch owns device memory and streams; all compute is in
libomg_hip.so.  Every function enqueues on torch's current stream and returns without syncing."""
from __future__ import annotations

import ctypes as C
import time
from collections import Counter

import numpy as np
import torch

from . import _lib, scenes as _sc
from ._lib import ChompParams, LearnerParams, check

_ws_cache: dict = {}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _lib.OmgHipError(f"{name} must be a device tensor (the reference asserts CHECK_CUDA, omg_layers.cpp:5)")
    if not t.is_contiguous():
        raise _lib.OmgHipError(f"{name} must be contiguous (CHECK_CONTIGUOUS, omg_layers.cpp:6)")
    if t.dtype != dtype:
        raise _lib.OmgHipError(f"{name} must be {dtype}, got {t.dtype}")


def _tensor(t, name: str, dtype, shape, dev) -> torch.Tensor:
    """t as it is if it is a contiguous device tensor of `dtype` on `dev` with `shape` (None: a free dimension, or any shape)."""
    if not isinstance(t, torch.Tensor):
        raise _lib.OmgHipError(f"{name} must be a tensor")
    _need(t, dtype, name)
    shape = (None,) * t.dim() if shape is None else shape
    if t.device != dev or t.dim() != len(shape) or any(w is not None and n != w for n, w in zip(t.shape, shape)):
        want = ", ".join("*" if w is None else str(w) for w in shape)
        raise _lib.OmgHipError(f"{name} must be [{want}] on {dev}, got {tuple(t.shape)} on {t.device}")
    return t


def _nonneg_finite(**named) -> None:
    if not all(np.isfinite(float(x)) and float(x) >= 0 for x in named.values()):
        raise _lib.OmgHipError(f"{' and '.join(named)} must be finite and not negative")


def _workspace(nbytes: int, device) -> torch.Tensor:
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def _kin_workspace(prepass, S: int, G: int, n_remaining: int, P: int, device):
    """Scratch of the kinematics pre-pass (omgx_goalset_workspace_bytes): None without it, the caller's own uint8 tensor, or the
    cached buffer of this (device, current stream) pair (`_workspace`: launches on different streams get different buffers)."""
    if prepass is None or prepass is False:
        return None
    need = _lib.lib().omgx_goalset_workspace_bytes(S, G, int(n_remaining), P)
    if isinstance(prepass, torch.Tensor):
        if not prepass.is_cuda or prepass.numel() * prepass.element_size() < need or not prepass.is_contiguous():
            raise _lib.OmgHipError(f"the pre-pass workspace must be a contiguous device tensor of at least {need} bytes")
        return prepass
    return _workspace(need, device)


def _eta(eta, S):
    if eta is not None and not (eta.is_cuda and eta.dtype == torch.float64 and eta.is_contiguous() and eta.numel() == S):
        raise _lib.OmgHipError("eta must be a contiguous float64 device tensor [S]")
    return eta


def _i32n(t, n, name):
    """Optional contiguous 4-byte integer device tensor of n elements (int32 schedules, uint32-as-int32 work counters)."""
    if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and (n is None or t.numel() == n)):
        raise _lib.OmgHipError(f"{name} must be a contiguous int32 device tensor" + (f" of {n} elements" if n is not None else ""))
    return t


def _active(active, S):
    if active is not None and not (active.is_cuda and active.dtype == torch.int32 and active.is_contiguous() and active.numel() == S):
        raise _lib.OmgHipError("active must be a contiguous int32 device tensor [S]")
    return active


def _traj_start(traj_start):
    """traj_start [S,9] float64, a strided row view such as traj[:, k] included -> (pointer, row stride in doubles)."""
    if not (traj_start.is_cuda and traj_start.dtype == torch.float64 and traj_start.dim() == 2 and traj_start.shape[1] == 9
            and traj_start.stride(1) == 1 and (traj_start.shape[0] == 1 or traj_start.stride(0) >= 9)):
        raise _lib.OmgHipError("traj_start must be a float64 device tensor [S,9] with unit inner stride")
    return _ptr(traj_start), traj_start.stride(0) if traj_start.shape[0] > 1 else 9


def _layer(S: int, P: int, traj, layer_out, layer_poses=None):
    """The trajectory layer of a launch, checked: traj [S,n,9] f64, layer_out = (potentials [S,n,10,P], grads [S,n,10,P,3], collides
    [S,n,10,P]) f32, layer_poses [S,n,10,12] f64 or None -> pointers (traj, n, potentials, grads, collides, layer_poses).
    traj None: a launch without the layer (layer_out is not looked at, layer_poses is an error)."""
    n, ptrs = 0, (None, None, None)
    if traj is not None:
        _need(traj, torch.float64, "traj")
        for n_, t in zip(("layer potentials", "layer grads", "layer collides"), layer_out):
            _need(t, torch.float32, n_)
        lp, lg, lc = layer_out
        n = traj.shape[1]
        if traj.shape[0] != S or lp.numel() != S * n * 10 * P or lg.numel() != 3 * lp.numel() or lc.numel() != lp.numel():
            raise _lib.OmgHipError("layer outputs must be [S,n,10,P], [S,n,10,P,3], [S,n,10,P]")
        ptrs = (_ptr(lp), _ptr(lg), _ptr(lc))
    if layer_poses is not None:
        _need(layer_poses, torch.float64, "layer_poses")
        if traj is None or layer_poses.numel() != S * n * 120:
            raise _lib.OmgHipError("layer_poses must be [S,n,10,12] and needs the trajectory layer")
    return (_ptr(traj), n, *ptrs, _ptr(layer_poses))


def _goal_out(goal_out, need: int):
    """(goal_cost, collides) f32 of at least `need` = S * G * parts elements each, checked -> their pointers."""
    for n_, t in zip(("goal_cost", "goal collides"), goal_out):
        _need(t, torch.float32, n_)
        if t.numel() < need:
            raise _lib.OmgHipError(f"{n_} must hold S * G * parts = {need} elements")
    return _ptr(goal_out[0]), _ptr(goal_out[1])


def _iteration_tensors(S: int, goal_set, reach, state, goal_idx, cost_vector, start, end, goal_rows, goal_point, step_out, active, goal_count,
                       eta, scene_flags=None):
    """The learner's and the step's tensors of an iteration (omgx_goal_update_optimize, omgx_plan_persistent), checked: all but the
    trajectory and its layer (`_layer`) and the goal costs (`_goal_out`)."""
    for n_, t in (("goal_set", goal_set), ("state", state), ("start", start), ("end", end), ("goal", goal_rows), ("goal_point", goal_point),
                  *zip(("grad", "cost_traj", "info"), step_out)):
        _need(t, torch.float64, n_)
    for n_, t in (("reach", reach), ("cost_vector", cost_vector)):
        if t is not None:
            _need(t, torch.float64, n_)
    if goal_idx.dtype != torch.int32 or not goal_idx.is_cuda or goal_idx.numel() != S:
        raise _lib.OmgHipError("goal_idx must be an int32 device tensor [S]")
    if scene_flags is not None and (scene_flags.dtype != torch.int32 or scene_flags.numel() < S or not scene_flags.is_cuda):
        raise _lib.OmgHipError("scene_flags must be an int32 device tensor [S]")
    _active(active, S); _active(goal_count, S); _eta(eta, S)


def _schedule_args(schedule, work, items: int):
    """(schedule, schedule_len, work) of a goal-set launch over `items` workgroups: checked int32 device tensors or None."""
    work = None if work is None else _ptr(_i32n(work, items, "work"))
    if schedule is None:
        return None, 0, work
    return _ptr(_i32n(schedule, None, "schedule")), schedule.numel(), work


class _GoalsetArgs:
    """The argument lists of omgx_goalset_cost_layer, _parts and _tiled from one set of checked pointers.  The three entry points
    share robot .. goal collides and traj .. goal_count; they differ in where the pre-pass workspace goes and in what follows
    goal_count, which is what their methods below add.  start = (traj_start, its row stride), active and stream change per launch."""

    def __init__(self, robot, P, scenes: "DeviceScenes", goals, S, G, dt, soften_fingers, goal_out, layer, layer_soften_fingers, goal_count, kin_ws):
        traj, n, lp, lg, lc, self.poses = layer
        self.scene = (_ptr(robot), int(P), _ptr(scenes.objects), _ptr(scenes.scene_begin), _ptr(scenes.pool))
        self.goals = (_ptr(goals), S, G)
        self.cost = (float(dt), int(bool(soften_fingers)), *goal_out)
        self.layer = (traj, n, int(bool(layer_soften_fingers)), lp, lg, lc)
        self.items, self.goal_count, self.ws = S * G, _ptr(goal_count), _ptr(kin_ws)

    def _args(self, start, n_remaining, ws, active, tail, stream):
        return (*self.scene, *start, *self.goals, n_remaining, *self.cost, *ws, *self.layer, active, self.goal_count, *tail, stream)

    def whole(self, start, n_remaining, active, schedule, work, stream):
        """omgx_goalset_cost_layer: the workspace after the goal outputs, the dispatch schedule last."""
        return self._args(start, n_remaining, (self.ws,), active, _schedule_args(schedule, work, self.items), stream)

    def parts(self, start, n_remaining, active, schedule, work, NP, goal_parts, poses, stream):
        """omgx_goalset_cost_layer_parts: the schedule over the (scene, goal, part) items, then goal_parts, layer_poses, workspace."""
        return self._args(start, n_remaining, (), active, (*_schedule_args(schedule, work, self.items * NP), goal_parts, poses, self.ws), stream)

    def tiled(self, start, n_remaining, active, tiling, poses, stream):
        """omgx_goalset_cost_layer_tiled: (goal_parts, layer_link_groups, layer_config_block, spread), then layer_poses, workspace."""
        return self._args(start, n_remaining, (), active, (*tiling, poses, self.ws), stream)


def sdf_loss_forward(pose_init, sdf_grids, sdf_limits, points, epsilons, padding_scales, clearances, disables):
    """omg_cuda.sdf_loss_forward (layers/omg_layers.cpp:24-49): -> [potentials[N], potential_grads[N,3], collides[N]]."""
    for n, t in (("pose_init", pose_init), ("sdf_grids", sdf_grids), ("sdf_limits", sdf_limits), ("points", points),
                 ("epsilons", epsilons), ("padding_scales", padding_scales), ("clearances", clearances), ("disables", disables)):
        _need(t, torch.float32, n)
    N, O = points.shape[0], pose_init.shape[0]
    pot = torch.empty(N, dtype=torch.float32, device=points.device)
    grad = torch.empty((N, 3), dtype=torch.float32, device=points.device)
    col = torch.empty(N, dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        check(_lib.lib().omgx_sdf_loss_forward(_ptr(pose_init), _ptr(sdf_grids), _ptr(sdf_limits), _ptr(points),
                                               _ptr(epsilons), _ptr(padding_scales), _ptr(clearances), _ptr(disables),
                                               N, O, _ptr(pot), _ptr(grad), _ptr(col), _stream()), "omgx_sdf_loss_forward")
    return [pot, grad, col]


def _masked_depth(depth: torch.Tensor, free_mask) -> torch.Tensor:
    """depth [V,H,W] float64 on the device with the pixels of free_mask (a bool tensor of its shape, on its device; or None) set
    to +inf, as a new tensor: the caller's images are not changed."""
    _need(depth, torch.float64, "depth")
    if free_mask is None:
        return depth
    if (not isinstance(free_mask, torch.Tensor) or free_mask.dtype != torch.bool or free_mask.shape != depth.shape
            or free_mask.device != depth.device):
        raise _lib.OmgHipError("free_mask must be a bool tensor of depth's shape, on its device")
    return torch.where(free_mask, torch.full_like(depth, float("inf")), depth).contiguous()


class PoolSlots:
    """Which part of the SDF pool each object's volume may use, as offsets and element counts.  Identical volumes are stored once
    (scenes.pack_table(share_grids=True), scene_io); a slot several objects share is never written in place (copy-on-write)."""

    def __init__(self, offsets, sizes, used: int, capacity: int):
        self.offset = [int(o) for o in offsets]  # where object i's volume lies
        self.cap = [int(n) for n in sizes]       # elements object i may use there
        self.refs = Counter(self.offset)
        self.free = []       # [(offset, capacity)] slots no object points at any more: reused before the reserve is touched
        self.pending = {}    # object -> (offset, capacity) offered, not yet committed
        self.used, self.capacity = int(used), int(capacity)  # the reserve is [used, capacity)

    def offer(self, i: int, n: int) -> int:
        """Offset for object i's NEXT volume of n elements: its own slot if n fits and nobody shares it, else the first free slot
        that fits, else the reserve.  Nothing changes for i before commit(i); an offer never committed returns to the free list."""
        old = self.pending.pop(i, None)
        if old is not None and old[0] != self.offset[i]:
            self.free.append(old)
        off, cap = self.offset[i], self.cap[i]
        if n > cap or self.refs[off] > 1:
            for k, (_, fc) in enumerate(self.free):
                if fc >= n:
                    off, cap = self.free.pop(k)
                    break
            else:
                if self.used + n > self.capacity:
                    raise _lib.OmgHipError(f"the SDF pool has no room for {n} more voxels: build DeviceScenes with reserve_voxels")
                off, cap = self.used, n
                self.used += n
        self.pending[i] = (off, cap)
        return off

    def commit(self, i: int) -> int:
        """Object i moves into the slot it was offered; the slot it leaves behind is free once no object uses it."""
        off, cap = self.pending.pop(i)
        old = self.offset[i]
        if off != old:
            self.refs[old] -= 1
            if self.refs[old] <= 0:
                del self.refs[old]
                self.free.append((old, self.cap[i]))
            self.refs[off] += 1
            self.offset[i], self.cap[i] = off, cap
        return off


class DeviceScenes:
    """Scene table resident in HBM: object records, scene_begin, SDF pool (see scenes.SceneBatch) — and the ways to change it
    while it stays there (include/omg_hip.h section 8): `set_object_pose` (a 48-byte write), `replace_grid` (a volume that is
    already on the device, its influence region fitted on the device), `grid_slot` (where omgx_point_cloud_sdf can write a new
    volume directly).  Every change is ordered on torch's current stream; launches enqueued behind it see the new scene, and a
    ChompEngine built on these scenes plans again without being rebuilt (it holds pointers, not copies).
    `reserve_voxels`: spare float32 elements at the end of the pool for volumes that outgrow their slot (the pool is never
    reallocated: engines and prepared launches keep its address).
    DeviceScenes(batch) and from_scenes own their pool; over_pool borrows one (poses may change, volumes may not); scene_range is a
    view of some scenes for launches (nothing may change)."""

    def __init__(self, batch, device="cuda:0", reserve_voxels: int = 0, *, _fields=None):
        if _fields is not None:  # from_scenes, over_pool, scene_range
            return self._set(*_fields)
        dev = torch.device(device)
        used = int(np.asarray(batch.pool).size)
        pool = torch.empty(used + max(int(reserve_voxels), 0), dtype=torch.float32, device=dev)
        pool[:used].copy_(torch.from_numpy(np.ascontiguousarray(batch.pool, np.float32).reshape(-1)))
        self._set(np.ascontiguousarray(batch.objects).copy(), batch.scene_begin, pool, used, dev)

    def _set(self, rec, scene_begin, pool, pool_used, device, shared=None):
        """Every field of a DeviceScenes.  rec: the host mirror of the records (the region fields of a device-fitted object are
        stale until sync_host()); pool_used None: the pool is not ours; shared: (objects, scene_begin, slots) of the table this one views."""
        assert rec.dtype == _sc.OBJECT_DTYPE
        self.device, self.pool, self.host_objects = torch.device(device), pool, rec
        self.host_scene_begin = np.ascontiguousarray(scene_begin, np.int32)
        self.num_scenes = len(self.host_scene_begin) - 1
        self._view, self._scratch = shared is not None, None
        if self._view:
            self.objects, self.scene_begin, self._slots = shared
        else:
            self.objects = torch.from_numpy(rec.view(np.uint8).copy()).to(self.device)
            self.scene_begin = torch.from_numpy(self.host_scene_begin).to(self.device)
            self._slots = None if pool_used is None else PoolSlots(rec["grid_offset"], rec["dim"].astype(np.int64).prod(axis=1), pool_used, pool.numel())

    @property
    def pool_used(self) -> int:  # elements of the pool that hold volumes: what lies behind them is the reserve
        return self.pool.numel() if self._slots is None else self._slots.used

    def _changing(self, volumes: bool = False):  # called first by every method that changes the table
        if self._view:
            raise _lib.OmgHipError("a scene range is for launches: change the scenes through the table the engine was built on")
        if volumes and self._slots is None:
            raise _lib.OmgHipError("these scenes address a pool that belongs to somebody else: its volumes are not replaced through them")

    @classmethod
    def from_scenes(cls, scenes, cfg_kwargs=None, device="cuda:0", share_grids: bool = True, reserve_voxels: int = 0,
                    timing: "dict | None" = None) -> "DeviceScenes":
        """First build of a batch WITHOUT a host pass over the voxels (Env.combine_sdfs, omg/core.py:366-411; scenes.pack_table is
        the host-side specification): the records are written on the host from the scenes' poses / limits / thresholds (a few
        hundred bytes per object, scenes.ragged_records), every distinct volume goes to the pool with one copy, and ALL influence
        regions are fitted on the device in seven launches (omgx_fit_influence_regions) — volumes and thresholds that occur several
        times are fitted once.  share_grids: a volume referenced by several objects (the same ndarray) is stored once.  The device
        records equal scenes.pack_table(scenes, cfg_kwargs, ragged=True, share_grids=share_grids) field for field; the host
        mirror's region fields are the loose ones until sync_host()."""
        t0 = time.perf_counter()
        dev = torch.device(device)
        rec, begins, chunks, used = _sc.ragged_records(scenes, cfg_kwargs, share_grids)
        t1 = time.perf_counter()
        with torch.cuda.device(dev):
            pool = torch.empty(used + int(reserve_voxels), dtype=torch.float32, device=dev)
            for off, data in chunks:
                src = torch.from_numpy(np.ascontiguousarray(data, np.float32).reshape(-1))
                pool[off: off + src.numel()].copy_(src, non_blocking=True)
            self = cls(None, _fields=(rec, begins, pool, used, dev))
        t2 = time.perf_counter()
        self.fit_all()
        if timing is not None:
            torch.cuda.synchronize(dev)
            t3 = time.perf_counter()
            timing.update(records_ms=(t1 - t0) * 1e3, upload_ms=(t2 - t1) * 1e3, fit_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3)
        return self

    @classmethod
    def over_pool(cls, records, scene_begin, pool: torch.Tensor, what: str = "the pool", device="cuda") -> "DeviceScenes":
        """Records (OBJECT_DTYPE, e.g. scenes.table_from_padded) around a pool that belongs to somebody else, addressed IN PLACE: a
        contiguous float32 tensor of any shape on a `device` kind of device; records and scene_begin go where it lives.  Objects
        can be moved and the mirror read back; the volumes are not ours to replace: grid_slot and replace_grid refuse."""
        if not (pool.device.type == torch.device(device).type and pool.dtype == torch.float32 and pool.is_contiguous()):
            raise _lib.OmgHipError(f"{what} must be a contiguous float32 device tensor")
        return cls(None, _fields=(np.ascontiguousarray(records).copy(), scene_begin, pool.reshape(-1), None, pool.device))

    def scene_range(self, lo: int, hi: int) -> "DeviceScenes":
        """Scenes [lo, hi) as a table for launches (the engine's pipeline parts): the same record buffer, host mirror and pool, both
        scene_begin cut to rows lo .. hi (object offsets stay absolute).  It cannot diverge from this table: every mutating method raises."""
        if not 0 <= lo <= hi <= self.num_scenes:
            raise IndexError(f"scenes [{lo}, {hi}) of {self.num_scenes}")
        shared = (self.objects, self.scene_begin[lo: hi + 1], self._slots)
        return DeviceScenes(None, _fields=(self.host_objects, self.host_scene_begin[lo: hi + 1], self.pool, None, self.device, shared))

    def fit_all(self) -> int:
        """Fit the influence region of every record the kernels cull for (scenes.culled), on the device, in seven launches
        (omgx_fit_influence_regions); records with the same volume CONTENT (omgx_volume_hashes: private copies of one model in many
        scenes count as one), dims, voxel size and thresholds are fitted once.  Returns the number of distinct fits."""
        self._changing()
        rec = self.host_objects
        w = (rec["hi"].astype(np.float32) - rec["lo"].astype(np.float32)).astype(np.float32)
        l = _lib.lib()
        with torch.cuda.device(self.device):  # 128-bit content hashes of all volumes: one launch, one small download
            d_hash = torch.empty((len(rec), 2), dtype=torch.int64, device=self.device)
            check(l.omgx_volume_hashes(_ptr(self.objects), len(rec), _ptr(self.pool), _ptr(d_hash), _stream()), "omgx_volume_hashes")
            hashes = d_hash.cpu().numpy()
        copy_src = np.full(len(rec), -1, np.int32)
        leaders, first = [], {}
        for o in np.flatnonzero(_sc.culled(rec)):
            r = rec[o]
            key = (hashes[o].tobytes(), r["dim"].tobytes(), w[o].tobytes(), float(r["epsilon"]), float(r["clearance"]))
            lead = first.setdefault(key, int(o))
            copy_src[o] = lead
            if lead == o:
                leaders.append(int(o))
        if not leaders:
            return 0
        fit_list = np.array(leaders, np.int32)
        nvox = rec["dim"][fit_list].astype(np.int64).prod(axis=1)
        need_off = np.concatenate([[0], np.cumsum(nvox)[:-1]]).astype(np.int64)
        nbytes = int(l.omgx_regions_scratch_bytes(len(fit_list), int(nvox.sum())))
        with torch.cuda.device(self.device):
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            d_fit = torch.from_numpy(fit_list).to(self.device)
            d_off = torch.from_numpy(need_off).to(self.device)
            d_src = torch.from_numpy(copy_src).to(self.device)
            check(l.omgx_fit_influence_regions(_ptr(self.objects), len(rec), _ptr(self.pool), _ptr(d_fit), _ptr(d_off), len(fit_list),
                                               int(nvox.max()), _ptr(d_src), _ptr(scratch), _stream()), "omgx_fit_influence_regions")
            scratch.record_stream(torch.cuda.current_stream(self.device))
        return len(fit_list)

    def _index(self, scene: int, obj: int) -> int:
        lo, hi = int(self.host_scene_begin[scene]), int(self.host_scene_begin[scene + 1])
        if not 0 <= obj < hi - lo:
            raise IndexError(f"scene {scene} has {hi - lo} objects")
        return lo + obj

    def _rows(self, pairs, unique=None) -> list:
        """The record rows of the (scene, obj) `pairs`.  unique: None, or the error to raise for a pair that is named twice."""
        rows = [self._index(int(s), int(o)) for s, o in np.asarray(pairs, np.int64).reshape(-1, 2)]
        if unique is not None and len(set(rows)) != len(rows):
            raise unique("a (scene, obj) pair is named twice")
        return rows

    def _writer_rows(self, pairs, layouts):
        """What an obstacle writer starts with -> (the pairs' rows, the layouts as a list): one layout per pair, no pair twice."""
        self._changing(volumes=True)
        pairs, layouts = np.asarray(pairs, np.int64).reshape(-1, 2), list(layouts)
        if len(layouts) != len(pairs) or not len(pairs):
            raise _lib.OmgHipError(f"{len(pairs)} pairs need as many layouts, and at least one")
        return self._rows(pairs, unique=_lib.OmgHipError), layouts

    def _record_ptr(self, idx: int) -> C.c_void_p:
        return C.c_void_p(self.objects.data_ptr() + idx * self.host_objects.dtype.itemsize)

    def set_object_pose(self, scene: int, obj: int, pose_mat) -> None:
        """Move an object: pose_mat [4,4] (object -> world; numpy or a device tensor).  The record's pose rows become
        se3_inverse(pose_mat) in float32 (omg/util.py:129-135, what Cost.compute_obstacle_cost_layer rebuilds per call,
        omg/cost.py:303-316); its influence region lives in object coordinates and stays."""
        self._changing()
        idx = self._index(scene, obj)
        if isinstance(pose_mat, torch.Tensor):
            P = pose_mat.to(device=self.device, dtype=torch.float64)
            R, t = P[:3, :3], P[:3, 3]
            inv = torch.cat([R.T, -(R.T @ t)[:, None]], dim=1).to(torch.float32).contiguous()  # [3,4]
            self.host_objects[idx]["pose_inv"] = inv.cpu().numpy().ravel()
        else:
            inv_h = _sc.se3_inverse(np.asarray(pose_mat, np.float64))[:3, :4]
            self.host_objects[idx]["pose_inv"] = inv_h.ravel()
            inv = torch.from_numpy(np.ascontiguousarray(inv_h, np.float32)).to(self.device, non_blocking=True)
        off = idx * self.host_objects.dtype.itemsize
        self.objects[off: off + 48].copy_(inv.reshape(-1).view(torch.uint8))

    def set_object_poses(self, indices, poses) -> None:
        """Move several objects at once: indices [n,2] (scene, obj) pairs, no pair twice; poses [n,4,4] (object -> world; numpy, or
        a tensor, which is brought to the host first).  The batched form of set_object_pose: the same float32 rows
        (scenes.se3_inverse of every pose), ONE upload and ONE scatter into the record buffer on the device, one update of the
        host mirror; record bytes and mirror end up as after set_object_pose(scene, obj, pose) with every pose given as a numpy
        array.  (set_object_pose inverts a TENSOR pose on the device with torch, whose rounding of R^T t is its own; here a
        tensor takes the numpy path, so the equality is with set_object_pose's numpy path whatever the input type.)"""
        self._changing()
        pairs = np.asarray(indices, np.int64).reshape(-1, 2)
        if isinstance(poses, torch.Tensor):
            poses = poses.detach().cpu().numpy()
        poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        if len(poses) != len(pairs):
            raise ValueError(f"{len(pairs)} pairs but {len(poses)} poses")
        idx = np.array(self._rows(pairs, unique=ValueError), np.int64)
        if not len(idx):
            return
        inv = np.stack([_sc.se3_inverse(P)[:3, :4] for P in poses]).reshape(-1, 12).astype(np.float32)
        self.host_objects["pose_inv"][idx] = inv
        rows = self.objects.view(-1, self.host_objects.dtype.itemsize)
        d_inv = torch.from_numpy(inv.view(np.uint8).reshape(-1, 48)).to(self.device, non_blocking=True)
        rows[:, :48].index_copy_(0, torch.from_numpy(idx).to(self.device, non_blocking=True), d_inv)

    def grid_slot(self, scene: int, obj: int, shape) -> torch.Tensor:
        """A float32 [X,Y,Z] view into the pool where the object's NEXT volume can be written in place (e.g. by
        point_cloud_sdf(out=...)), chosen by PoolSlots.offer.  Nothing about the object changes until replace_grid is given the view.
        Sizing the reserve: one extra volume per object whose cloud extents grow from frame to frame (a slot that is outgrown
        is reused by the next volume that fits it), plus one per object that shares its volume and will be changed."""
        self._changing(volumes=True)
        return self._pool_view(self._slots.offer(self._index(scene, obj), int(np.prod(shape))), shape)

    def replace_grid(self, scene: int, obj: int, grid: torch.Tensor, origin, delta: float, fit: str = "device") -> None:
        """Give an object a new volume that is already on the device: grid [X,Y,Z] float32 (a view from grid_slot: used in place;
        anything else is copied into the pool, device to device), origin = min corner [3], delta = voxel size.  The record's
        limits follow like scenes.pack_table writes them; the influence region is fitted ON THE DEVICE (fit="device":
        omgx_fit_influence_region, the algorithm of scenes.influence_rbox) or left loose (fit="loose": the grid with 1.5 voxels
        of slack — same results, more exact lookups)."""
        self._changing(volumes=True)
        if fit not in ("device", "loose"):
            raise ValueError("fit must be 'device' or 'loose'")
        _need(grid, torch.float32, "grid")
        if grid.dim() != 3:
            raise _lib.OmgHipError("grid must be [X,Y,Z]")
        self._replace(self._index(scene, obj), grid, origin, delta, fit)

    def _replace(self, idx: int, grid: torch.Tensor, origin, delta: float, fit: str) -> None:
        shape = tuple(int(d) for d in grid.shape)
        n = int(np.prod(shape))
        pend = self._slots.pending.get(idx)
        if pend is not None and n <= pend[1] and grid.data_ptr() == self.pool.data_ptr() + 4 * pend[0]:
            slot = grid  # the view grid_slot handed out, filled in place
        else:
            slot = self._pool_view(self._slots.offer(idx, n), shape)
            slot.copy_(grid)
        rec = self.host_objects[idx]
        rec["grid_offset"] = self._slots.commit(idx)
        lo, hi = _sc.grid_limits(origin, shape, delta)
        dims = np.array(shape, np.int32)
        rec["lo"], rec["hi"], rec["dim"], rec["delta"] = lo, hi, dims, np.float32(delta)
        _sc.finish_records(self.host_objects[idx: idx + 1])  # host mirror: derived constants + the loose region
        l = _lib.lib()
        vp = C.c_void_p
        with torch.cuda.device(self.device):
            check(l.omgx_object_set_grid(self._record_ptr(idx), lo.ctypes.data_as(vp), hi.ctypes.data_as(vp), dims.ctypes.data_as(vp),
                                         float(np.float32(delta)), int(rec["grid_offset"]), _stream()), "omgx_object_set_grid")
            if fit == "device":
                need = int(l.omgx_region_scratch_bytes(*shape))
                if self._scratch is None or self._scratch.numel() < need:
                    self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
                check(l.omgx_fit_influence_region(self._record_ptr(idx), C.c_void_p(slot.data_ptr()), dims.ctypes.data_as(vp),
                                                  lo.ctypes.data_as(vp), hi.ctypes.data_as(vp), float(rec["epsilon"]), float(rec["clearance"]),
                                                  _ptr(self._scratch), _stream()), "omgx_fit_influence_region")

    def _offer(self, rows, layouts):
        """A slot of the pool for the next volume of every record row -> the layouts (origin [3], delta, dims [3]) as surface_records takes
        them: voxel centres, at the slots' offsets.  A writer refuses what it can refuse BEFORE this, launches into the pool, then _adopt."""
        return [(origin, delta, "centre", dims, self._slots.offer(i, int(np.prod(dims)))) for i, (origin, delta, dims) in zip(rows, layouts)]

    def _adopt(self, rows, volumes) -> None:  # the offered slots, written by now, become the rows' volumes, fitted on the device
        for i, (origin, delta, _, dims, off) in zip(rows, volumes):
            self._replace(i, self._pool_view(off, dims), origin, float(delta), "device")

    def _pool_view(self, off: int, dims) -> torch.Tensor:
        dims = tuple(int(d) for d in dims)
        return self.pool[off: off + int(np.prod(dims))].view(dims)

    def volume(self, scene: int, obj: int) -> torch.Tensor:
        """The object's volume as it lies in the pool: a float32 [X,Y,Z] view, from the host mirror's offset and dims."""
        rec = self.host_objects[self._index(scene, obj)]
        return self._pool_view(int(rec["grid_offset"]), rec["dim"])

    def surface_records(self, indices):
        """The volumes of the objects `indices` (rows of the record table) as omgx_mesh records for omgx_surface_count /
        omgx_surface_gather: origin = the record's lo, its delta and dim, voxel centres, out_offset = its grid_offset in the pool,
        first_workgroup the prefix table.  From the host mirror: nothing is downloaded."""
        rec = self.host_objects
        idx = [int(i) for i in indices]
        if any(not 0 <= i < len(rec) for i in idx):
            raise IndexError(f"object rows must lie in [0, {len(rec)})")
        return surface_records([(rec["lo"][i].astype(np.float64), float(rec["delta"][i]), "centre", rec["dim"][i], int(rec["grid_offset"][i])) for i in idx])

    def object_surfaces(self, pairs=None, level: float = 0.0):
        """The level set of the volumes of the (scene, object) `pairs` (default: every object) as triangle meshes, read IN PLACE
        from the pool (ops.surface_meshes: nothing is uploaded but the records) -> (verts [V,3] float64 and faces [F,3] int32 on the
        device, vert_rows [n,2] and face_rows [n,2] = (begin, count) per pair, open_edges [n]; host int64).  Objects that share a
        volume (share_grids) are extracted once and name the same rows.  Coordinates are in the object's own frame, like its volume."""
        idx = list(range(len(self.host_objects))) if pairs is None else self._rows(pairs)
        rec, first, which = self.host_objects, {}, []
        for i in idx:
            key = (int(rec["grid_offset"][i]), rec["dim"][i].tobytes(), rec["lo"][i].tobytes(), rec["delta"][i].tobytes())
            which.append(first.setdefault(key, len(first)))
        if not idx:
            z = np.zeros((0, 2), np.int64)
            return (torch.empty((0, 3), dtype=torch.float64, device=self.device), torch.empty((0, 3), dtype=torch.int32, device=self.device), z, z.copy(),
                    np.zeros(0, np.int64))
        leaders = [idx[which.index(u)] for u in range(len(first))]
        verts, faces, vrows, frows, open_edges = surface_meshes(self.pool, self.surface_records(leaders), level)
        return verts, faces, vrows[which], frows[which], open_edges[which]

    def fuse_obstacles(self, pairs, depth: torch.Tensor, views, view_range, layouts, band: float, near: float, reach: float,
                       unknown_occupied: bool = True, free_mask: "torch.Tensor | None" = None, robot: "RobotView | None" = None) -> int:
        """The observed obstacle volumes of the (scene, obj) `pairs` from depth views, written straight into the pool: ONE carve
        launch and three transform launches for all pairs (carve_views, distance_transform), then grid_slot's slot becomes the
        object's volume through replace_grid(fit="device"), object by object.  layouts: one (origin [3], delta, dims [3]) per pair,
        voxel centres, in the object's own frame; views [V,16] (fusion.view_rows with cam_from_grid = cam_from_world times the
        object's pose) and view_range [n,2] as carve_views takes them; depth [V,H,W] float64 on the device.  reach: the distance up
        to which the cost reads the volume (epsilon + clearance): radius = ceil(reach / delta + 0.5) + 1 of the finest layout, so
        the saturation lies beyond it.  free_mask: a bool tensor [V,H,W]; its pixels are set to +inf first (the target's pixels:
        the reference's "non-target points only").  robot: a RobotView whose images belong to the views, one by one (the arm as
        the same cameras see it): the pixels it explains are set to 0.0, no information, before the carve, and clear_robot frees
        the arm's nodes between the carve and the transform (_robot_step).  Returns the radius."""
        from . import fusion as _fu
        rows, layouts = self._writer_rows(pairs, layouts)
        _nonneg_finite(reach=reach)
        # everything that can be refused is refused here, before grid_slot offers a slot: the radius, the layouts, the views
        _, views = _carve_arguments([(origin, delta, "centre", dims) for origin, delta, dims in layouts], views, view_range, depth, band, near, None)
        radius = _fusion_radius(max(_fu.obstacle_radius(reach, float(delta)) for _, delta, _ in layouts))
        depth, clear = _robot_step(robot, _masked_depth(depth, free_mask), views, None, near)
        volumes = self._offer(rows, layouts)
        fuse_views(volumes, views, None, depth, band, near, radius, unknown_occupied, out=self.pool, clear=clear)
        self._adopt(rows, volumes)
        return radius

    def integrate_obstacles(self, pairs, tsdf_volumes: "TsdfVolumes | None", depth: torch.Tensor, views, view_range, layouts, trunc: float,
                            near: float, reach: float, unknown_occupied: bool = True, min_weight: float = 1.0, wmax: float = float("inf"),
                            weights=None, free_mask: "torch.Tensor | None" = None, robot: "RobotView | None" = None):
        """fuse_obstacles with weighted TSDF fusion (fuse_tsdf; tsdf.fuse is the specification): the volumes of the (scene, obj)
        `pairs` have their zero level on the observed surface, between the nodes, not `band` in front of it on voxel faces; with
        a finite wmax old frames fade, so that an object that was taken away becomes free again.  pairs, depth, views,
        view_range, layouts, near, reach, unknown_occupied, free_mask and robot as fuse_obstacles takes them (clear_robot runs
        on the states of this frame's arm, between tsdf_states and the transform: the pairs themselves keep what they saw);
        trunc: the truncation (a few voxels, a few sigma of the sensor); weights: one per view.  tsdf_volumes: None for the first frame, or what an
        earlier call returned: this frame is added to the same pairs (its layouts, trunc, near and wmax must be the call's).
        One integrate launch, then states, the three transform launches and the blend for all pairs, written straight into
        grid_slot's slots, which become the objects' volumes through replace_grid(fit="device").  Everything that can be
        refused is refused before a slot is offered.  Returns (radius, the TsdfVolumes)."""
        from . import fusion as _fu
        rows, layouts = self._writer_rows(pairs, layouts)
        _nonneg_finite(reach=reach)
        min_weight = _tsdf_positive("min_weight", min_weight)
        volumes = [(origin, delta, "centre", dims) for origin, delta, dims in layouts]
        _, views, _, trunc, wmax = _tsdf_arguments(volumes, views, view_range, depth, trunc, near, weights, wmax, None)
        radius = _fusion_radius(max(_fu.obstacle_radius(reach, float(delta)) for _, delta, _ in layouts))
        depth, clear = _robot_step(robot, _masked_depth(depth, free_mask), views, None, near)
        if depth.device != self.pool.device:
            raise _lib.OmgHipError(f"depth must be on {self.pool.device}, got {depth.device}")
        if tsdf_volumes is None:
            tsdf_volumes = TsdfVolumes(volumes, trunc, near, wmax, device=depth.device)
        else:
            same = isinstance(tsdf_volumes, TsdfVolumes) and len(tsdf_volumes.rec) == len(layouts) and all(
                np.array_equal(a[0], np.asarray(b[0], np.float64).reshape(-1)) and a[1] == float(b[1]) and a[2] == tuple(int(d) for d in b[2])
                for a, b in zip(tsdf_volumes.layouts(), layouts))
            if not same or (tsdf_volumes.trunc, tsdf_volumes.near, tsdf_volumes.wmax) != (trunc, float(near), wmax):
                raise _lib.OmgHipError("tsdf_volumes were started with other layouts, or another trunc, near or wmax")
            if tsdf_volumes.device != depth.device:
                raise _lib.OmgHipError(f"tsdf_volumes are on {tsdf_volumes.device}, depth on {depth.device}")
        placed = self._offer(rows, layouts)
        tsdf_volumes.integrate(depth, views, None, weights)
        tsdf_volumes.signed(radius, unknown_occupied, min_weight, out=self.pool, offsets=[v[4] for v in placed], clear=clear)
        self._adopt(rows, placed)
        return radius, tsdf_volumes

    def segment_obstacles(self, target_pairs, obstacle_pairs, depth: torch.Tensor, views, view_range, layouts, band: float, near: float,
                          reach: float, seeds, min_nodes: int, connectivity: int = 6, margin: "int | None" = None,
                          free_mask: "torch.Tensor | None" = None, robot: "RobotView | None" = None):
        """fuse_obstacles without labels: per scene n the layout (origin [3], delta, dims [3]: voxel centres, in the frame both of
        the scene's pairs stand in) is carved from its views, the SURFACE nodes are labelled (label_components), the target is the
        component nearest to seeds[n] (a point of the layout's frame, converted to index units on the host;
        segmentation.pick_component among the components of at least min_nodes nodes), its crop in mode 0 becomes the volume of
        target_pairs[n] and the whole layout in mode 1 the volume of obstacle_pairs[n], both through grid_slot and
        replace_grid(fit="device").  One carve launch, one labelling and one set of crop and transform launches for all scenes;
        two small downloads (counts, records).  margin: nodes around the target's box (default radius + 1, so that the target's
        zero level closes inside its crop); free_mask and robot as fuse_obstacles takes them (camera.explained_mask: the
        support; the arm is cleared before the labelling, so that it is no component).
        -> (radius, the chosen records [n,8] int32, the Components).  segmentation.segment_views is the specification."""
        from . import fusion as _fu, segmentation as _sg
        self._changing(volumes=True)
        tp, op = np.asarray(target_pairs, np.int64).reshape(-1, 2), np.asarray(obstacle_pairs, np.int64).reshape(-1, 2)
        layouts = list(layouts)
        n = len(layouts)
        seeds = np.asarray(seeds, np.float64).reshape(-1, 3)
        if not n or len(tp) != n or len(op) != n or len(seeds) != n:
            raise _lib.OmgHipError(f"{n} layouts need as many target pairs, obstacle pairs and seeds, and at least one")
        rows = self._rows(np.concatenate([tp, op]), unique=_lib.OmgHipError)  # the targets' rows, then the obstacles'
        _nonneg_finite(reach=reach)
        if not np.isfinite(seeds).all() or int(min_nodes) < 1 or (margin is not None and int(margin) < 0):
            raise _lib.OmgHipError("seeds must be finite, min_nodes at least 1 and margin not negative")
        _segment_arguments(1, connectivity)
        volumes = [(origin, delta, "centre", dims) for origin, delta, dims in layouts]
        batch, views = _carve_arguments(volumes, views, view_range, depth, band, near, None)  # (one batch of each for every stage)
        radius = _fusion_radius(max(_fu.obstacle_radius(reach, float(delta)) for _, delta, _ in layouts))
        margin = radius + 1 if margin is None else int(margin)
        depth, clear = _robot_step(robot, _masked_depth(depth, free_mask), views, None, near)
        state, _ = carve_views(batch, views, None, depth, band, near)
        if clear is not None:
            clear(state, None, batch)
        comps = label_components(state, None, batch, 1, connectivity)
        try:  # (a scene without a component of min_nodes nodes is refused here: no slot has been offered yet)
            ranks = [_sg.pick_component(comps.of(m), _sg.point_to_index(volumes[m], seeds[m]), min_nodes) for m in range(n)]
        except ValueError as e:
            raise _lib.OmgHipError(str(e)) from None
        chosen = [int(comps.comp_begin[m]) + ranks[m] for m in range(n)]
        crops = [c for m in range(n) for c in (_sg.crop_layout(layouts[m], comps.records[chosen[m]], margin), tuple(layouts[m]) + ((0, 0, 0),))]
        picks = [(k // 2,) + tuple(first) + (chosen[k // 2], k % 2, 0, 0) for k, (_, _, _, first) in enumerate(crops)]
        rows = [r for both in zip(rows[:n], rows[n:]) for r in both]  # (per scene: the target's crop in mode 0, then the whole layout in mode 1)
        outs = self._offer(rows, [c[:3] for c in crops])
        component_volumes(state, comps, picks, outs, radius, True, out=self.pool)
        self._adopt(rows, outs)
        return radius, comps.records[chosen].copy(), comps

    def plane_obstacles(self, pairs, planes, layouts) -> None:
        """The half-space volumes of fitted supports as the volumes of the (scene, obj) `pairs`, written straight into the pool:
        a support that plane_mask took out of the depth images would otherwise be space the planner believes is free.  planes
        [n,4] on the host, each in its object's own frame (camera.Observation.support_planes), the normal towards the free side;
        layouts: one (origin [3], delta, dims [3]) per pair, voxel centres, in the object's frame.  grid_slot, ONE launch
        (plane_volumes), then replace_grid(fit="device") object by object, as fuse_obstacles does it; everything that can be
        refused is refused before a slot is offered."""
        rows, layouts = self._writer_rows(pairs, layouts)
        _plane_volume_arguments([(origin, delta, "centre", dims) for origin, delta, dims in layouts], planes)
        volumes = self._offer(rows, layouts)
        plane_volumes(volumes, planes, out=self.pool)
        self._adopt(rows, volumes)

    def sync_host(self) -> np.ndarray:
        """Bring the host mirror of the records up to date with the device (one small copy; tests, oracle comparisons)."""
        self.host_objects[:] = self.objects.cpu().numpy().view(self.host_objects.dtype)  # in place: scene ranges share the mirror
        return self.host_objects

    def host_batch(self):
        """The scenes as they are on the device now, as a host SceneBatch (records + pool copied back): for oracle checks."""
        return _sc.SceneBatch(self.sync_host().copy(), self.host_scene_begin.copy(), self.pool[: self.pool_used].cpu().numpy())

    def plan_clearance(self, spheres: "RobotSpheres", robot_blob, P: int, traj: torch.Tensor, substeps: int, slack: float = 0.0,
                       beyond: float = 0.1, visible=None, pairs=None, rho=None, scene_of_plan=None, cull: bool = True) -> "PlanClearance":
        """Are the plans traj [S',n,9] free of this table's volumes, at the waypoints and between them?  clearance.py is the
        specification (its docstring says what the certificate means and what `slack` states): dense_configs with K = substeps,
        ONE forward_kinematics call, ONE sphere_clearance launch with the pads of clearance.sample_pads, with `pairs` [10,10] ONE
        self_clearance launch with the same pads, then clearance.plan_report in torch: the same bits throughout, and no host
        sync on the way.  Plan s stands in scene scene_of_plan[s] (host integers; default: plan s in scene s, S' = num_scenes).
        visible: one flag per record or None (the enabled records).  rho [10,9]: clearance.reach_table (default: the one
        spheres.reach_table() computed).  Ordered on torch's current stream."""
        dev = self.device
        _tensor(traj, "traj", torch.float64, (None, None, 9), dev)
        S, n = int(traj.shape[0]), int(traj.shape[1])
        K = int(substeps)
        rho = getattr(spheres, "rho", None) if rho is None else rho
        if rho is None:
            raise _lib.OmgHipError("rho is needed for the certificate: clearance.reach_table, or spheres.reach_table(model) once")
        rho = np.ascontiguousarray(rho, np.float64)
        if rho.shape != (10, 9) or not np.isfinite(rho).all() or (rho < 0).any():
            raise _lib.OmgHipError("rho must be [10,9], finite and not negative")
        if K < 1 or n < 1:
            raise _lib.OmgHipError(f"substeps and the number of waypoints must be >= 1, got {K} and {n}")
        _nonneg_finite(slack=slack, beyond=beyond)
        sop = np.arange(S) if scene_of_plan is None else np.asarray(scene_of_plan, np.int64).reshape(-1)
        if len(sop) != S or (S and (sop.min() < 0 or sop.max() >= self.num_scenes)):
            raise _lib.OmgHipError(f"scene_of_plan must be {S} scenes in [0, {self.num_scenes})")
        T = (n - 1) * K + 1
        q = dense_configs(traj, K)
        d_rho = _upload(rho, dev)
        dq = (traj[:, 1:] - traj[:, :-1]).abs()  # clearance.segment_halves, operation for operation
        length = d_rho[:, 0] * dq[:, :, 0:1]
        for j in range(1, 9):
            length = length + d_rho[:, j] * dq[:, :, j:j + 1]
        half = (length / torch.full((1,), float(K), dtype=torch.float64, device=dev)) * 0.5  # (a tensor as divisor: dense_configs says why)
        pad = torch.zeros((S, T, 10), dtype=torch.float64, device=dev)  # clearance.sample_pads
        if n > 1:
            pad[:, :-1] = half.repeat_interleave(K, dim=1)
            way = half.clone()
            way[:, 1:] = torch.maximum(half[:, 1:], half[:, :-1])
            pad[:, 0:-1:K] = way
            pad[:, -1] = half[:, -1]
        pad = pad + float(slack)
        poses = forward_kinematics(robot_blob, P, q.reshape(S * T, 9), want_joint_info=False)[0] if S else q.new_empty((0, 10, 4, 4))
        out = sphere_clearance(self, spheres, poses, np.repeat(sop, T), visible=visible, pad=pad.reshape(S * T, 10), beyond=beyond, cull=cull,
                               want_world=pairs is not None)
        clear, margin = out[0].reshape(S, T), out[3].reshape(S, T)
        own = (None, None, None) if pairs is None else tuple(x.reshape(S, T) for x in self_clearance(out[6], spheres, pairs, pad=pad.reshape(S * T, 10)))
        r_max = float(spheres.h_local[:, 3].max()) if spheres.N else 0.0
        if n > 1:  # clearance.plan_report
            seg = torch.minimum(margin[:, :-1].reshape(S, n - 1, K).amin(dim=2), margin[:, K::K][:, : n - 1])
            certified = (seg > 0.0) & ((r_max + half.amax(dim=2)) + float(slack) <= float(beyond))
            whole = certified.all(dim=1)
        else:
            seg, certified = margin[:, :0], torch.zeros((S, 0), dtype=torch.bool, device=dev)
            whole = (margin[:, 0] > 0.0) & (r_max + float(slack) <= float(beyond))
        hit = clear < 0.0
        collides = hit.any(dim=1)
        first = torch.where(collides, hit.to(torch.uint8).argmax(dim=1), torch.full_like(collides, -1, dtype=torch.int64))
        return PlanClearance(K=K, q=q, clear=clear, clear_sphere=out[1].reshape(S, T), clear_object=out[2].reshape(S, T), margin=margin,
                             margin_sphere=out[4].reshape(S, T), margin_object=out[5].reshape(S, T), self_clear=own[0], self_i=own[1],
                             self_j=own[2], half=half, segment_margin=seg, certified=certified, min_clearance=clear.amin(dim=1),
                             collides=collides, first_hit=first, plan_certified=whole)


def robot_blob(model, device="cuda:0") -> torch.Tensor:
    return torch.from_numpy(model.blob()).to(device)


def fk_sdf(robot: torch.Tensor, P: int, scenes: DeviceScenes, joints: torch.Tensor, soften_fingers=False,
           want_grad=True, want_col=True, out=None, arc_length=0, arc_start=None, dt=0.1):
    """joints [S,C,9] f64 -> potentials [S,C,10,P], grads [S,C,10,P,3] | None, collides [S,C,10,P] | None.
    arc_length > 0: groups of arc_length waypoints, potentials weighted by the float32 point speed."""
    _need(joints, torch.float64, "joints")
    S, Cn = joints.shape[0], joints.shape[1]
    dev = joints.device
    if out is None:
        pot = torch.empty((S, Cn, 10, P), dtype=torch.float32, device=dev)
        grad = torch.empty((S, Cn, 10, P, 3), dtype=torch.float32, device=dev) if want_grad else None
        col = torch.empty((S, Cn, 10, P), dtype=torch.float32, device=dev) if want_col else None
    else:
        pot, grad, col = out
    l = _lib.lib()
    with torch.cuda.device(dev):
        ws = _workspace(l.omgx_fk_sdf_workspace_bytes(S, Cn, P), dev)
        if arc_length > 0:
            _need(arc_start, torch.float64, "arc_start")
        check(l.omgx_fk_sdf(_ptr(robot), P, _ptr(scenes.objects), _ptr(scenes.scene_begin), _ptr(scenes.pool),
                            _ptr(joints), S, Cn, int(bool(soften_fingers)), int(arc_length), _ptr(arc_start), float(dt),
                            _ptr(pot), _ptr(grad), _ptr(col), _ptr(ws), _stream()), "omgx_fk_sdf")
    return pot, grad, col


def goalset_cost(robot, P, scenes: DeviceScenes, traj_start, goals, n_remaining, dt, soften_fingers=False,
                 want_potentials=False, out=None, active=None, goal_count=None, prepass=False):
    """traj_start [S,9], goals [S,G,9] f64 -> goal_cost [S,G] f32, collides [S,G] f32, potentials [S,G,n,10,P] | None.
    traj_start may be a strided row view such as traj[:, k] of a contiguous [S,n,9] tensor (no copy is made).
    active / goal_count [S] int32 (optional, not with want_potentials): scenes with 0 and the padding goals of a ragged
    goal set are skipped; their outputs keep their previous contents.
    prepass: the goals' kinematics and row masks as a launch of their own (k_goalset_kin, ABI 10) through a scratch workspace
    — same bits, two launches; a torch tensor of omgx_goalset_workspace_bytes is taken as that workspace."""
    ts, ts_stride = _traj_start(traj_start)
    _need(goals, torch.float64, "goals")
    S, G = goals.shape[0], goals.shape[1]
    dev = goals.device
    if out is None:
        cost = torch.empty((S, G), dtype=torch.float32, device=dev)
        col = torch.empty((S, G), dtype=torch.float32, device=dev)
    else:
        cost, col = out
    pots = torch.empty((S, G, n_remaining, 10, P), dtype=torch.float32, device=dev) if want_potentials else None
    cost_p, col_p = _goal_out((cost, col), S * G)
    l = _lib.lib()
    with torch.cuda.device(dev):
        ws = _kin_workspace(prepass, S, G, n_remaining, P, dev) if not want_potentials else None
        check(l.omgx_goalset_cost(_ptr(robot), P, _ptr(scenes.objects), _ptr(scenes.scene_begin), _ptr(scenes.pool),
                                  ts, ts_stride, _ptr(goals), S, G, n_remaining, float(dt), int(bool(soften_fingers)),
                                  cost_p, _ptr(pots), col_p, _ptr(ws), _ptr(_active(active, S)), _ptr(_active(goal_count, S)),
                                  _stream()), "omgx_goalset_cost")
    return cost, col, pots


def goalset_cost_layer(robot, P, scenes: DeviceScenes, traj_start, goals, n_remaining, dt, traj, layer_out, soften_fingers=False,
                       layer_soften_fingers=False, out=None, active=None, goal_count=None, schedule=None, work=None, goal_parts=1,
                       layer_poses=None, prepass=False):
    """goalset_cost (cost only) + fk_sdf(traj) in one launch (omgx_goalset_cost_layer).  traj [S,n,9] f64;
    layer_out = (potentials [S,n,10,P], grads [S,n,10,P,3], collides [S,n,10,P]) float32, written in place.
    active [S] int32 (optional): scenes with 0 are skipped, their outputs keep their previous contents.
    goal_parts > 1 (omgx_goalset_cost_layer_parts): a goal's tiles dealt over NP = goalset_parts(n_remaining, goal_parts) workgroups
    of the batch kernel; `out` must then hold S * G * NP elements each and receives [S][G][NP] PARTIAL sums, schedule / work count
    the S * G * NP (scene, goal, part) items.  prepass: see goalset_cost.  Returns (cost, collides) as given / allocated."""
    start = _traj_start(traj_start)
    _need(goals, torch.float64, "goals")
    S, G = goals.shape[0], goals.shape[1]
    layer = _layer(S, P, traj, layer_out, layer_poses)
    dev = goals.device
    NP = goalset_parts(n_remaining, goal_parts) if int(goal_parts) != 1 else 1
    if NP < 1:
        raise _lib.OmgHipError("goal_parts must be 1, 2, 4 or 8")
    if out is None:
        cost = torch.empty((S, G) if NP == 1 else (S, G, NP), dtype=torch.float32, device=dev)
        col = torch.empty((S, G) if NP == 1 else (S, G, NP), dtype=torch.float32, device=dev)
    else:
        cost, col = out
    l = _lib.lib()
    with torch.cuda.device(dev):
        g = _GoalsetArgs(robot, P, scenes, goals, S, G, dt, soften_fingers, _goal_out((cost, col), S * G * NP), layer, layer_soften_fingers,
                         _active(goal_count, S), _kin_workspace(prepass, S, G, n_remaining, P, dev))
        active = _ptr(_active(active, S))
        if int(goal_parts) != 1 or layer_poses is not None:
            check(l.omgx_goalset_cost_layer_parts(*g.parts(start, n_remaining, active, schedule, work, NP, int(goal_parts), g.poses, _stream())),
                  "omgx_goalset_cost_layer_parts")
        else:
            check(l.omgx_goalset_cost_layer(*g.whole(start, n_remaining, active, schedule, work, _stream())), "omgx_goalset_cost_layer")
    return cost, col


def goalset_parts(n_remaining: int, goal_parts: int) -> int:
    """Workgroups per goal of goalset_cost_layer_tiled for a window of n_remaining configurations (omgx_goalset_parts)."""
    return int(_lib.lib().omgx_goalset_parts(int(n_remaining), int(goal_parts)))


def goalset_cost_layer_tiled(robot, P, scenes: DeviceScenes, traj_start, goals, n_remaining, dt, traj, layer_out, out,
                             soften_fingers=False, layer_soften_fingers=False, active=None, goal_count=None, goal_parts=4,
                             layer_link_groups=10, layer_config_block=16, spread=True, layer_poses=None, prepass=False):
    """The goal-set batch and / or the trajectory layer cut into many small workgroups (omgx_goalset_cost_layer_tiled: latency
    mode for one or a few scenes).  goals None: only the layer; traj None: only the batch.  out = (cost, collides): float32
    device tensors with at least S * G * goalset_parts(n_remaining, goal_parts) elements, written as [S][G][parts] PARTIAL sums
    (the learner adds them: LearnerParams.cost_parts).  layer_poses: optional float64 [S,n,10,12] receiving the waypoints' link
    poses (ChompParams.waypoint_poses of the step that follows).  Returns the number of parts per goal."""
    dev = (goals if goals is not None else traj).device
    S = (goals if goals is not None else traj).shape[0]
    G, start, parts, goal_out = 0, (None, 9), 1, (None, None)
    if goals is not None:
        start = _traj_start(traj_start)
        _need(goals, torch.float64, "goals")
        G = goals.shape[1]
        parts = goalset_parts(n_remaining, goal_parts)
        if parts < 1:
            raise _lib.OmgHipError("goal_parts must be 1, 2, 4 or 8")
        goal_out = _goal_out(out, S * G * parts)
    else:
        n_remaining, prepass = 1, None
    layer = _layer(S, P, traj, layer_out, layer_poses)
    with torch.cuda.device(dev):
        g = _GoalsetArgs(robot, P, scenes, goals, S, G, dt, soften_fingers, goal_out, layer, layer_soften_fingers, _active(goal_count, S),
                         _kin_workspace(prepass, S, G, n_remaining, P, dev))
        tiling = (int(goal_parts), int(layer_link_groups), int(layer_config_block), int(bool(spread)))
        check(_lib.lib().omgx_goalset_cost_layer_tiled(*g.tiled(start, int(n_remaining), _ptr(_active(active, S)), tiling, g.poses, _stream())),
              "omgx_goalset_cost_layer_tiled")
    return parts


def goalset_schedule(work, num_scenes: int, num_goals: int, active=None, goal_count=None, slack: int = 2, out=None, device=None,
                     parts: int = 1, longest_first: bool = False):
    """Dispatch order for goalset_cost_layer (omgx_goalset_schedule): int32 device tensor [omgx_goalset_schedule_len].
    work: int32/uint32 device tensor [S*G] of durations (None: all items weigh the same).  Asynchronous, one small launch.
    The result lives on the device of `out`, else of the first tensor given, else `device`.
    parts > 1 (omgx_goalset_schedule_parts): the items are the S * G * parts (scene, goal, part) workgroups of a launch with
    split goals; work [S*G*parts]; goal_count still counts goals.
    longest_first (omgx_goalset_schedule_ordered): inside an XCD the items run by decreasing work across its scenes — for launches of
    a round or two of the chip's workgroup slots (falls back to the scene-major order above 8192 items)."""
    l = _lib.lib()
    parts = int(parts)
    n = int(l.omgx_goalset_schedule_len(num_scenes, num_goals * parts, slack))
    if out is None:
        for t in (work, active, goal_count):
            if t is not None:
                device = t.device
                break
        if device is None:
            raise _lib.OmgHipError("goalset_schedule needs a device: pass work, active, goal_count, out or device")
        out = torch.empty(n, dtype=torch.int32, device=device)
    _i32n(out, n, "schedule")
    _i32n(work, num_scenes * num_goals * parts, "work")
    with torch.cuda.device(out.device):
        if longest_first:
            check(l.omgx_goalset_schedule_ordered(_ptr(work), _ptr(_active(active, num_scenes)), _ptr(_active(goal_count, num_scenes)),
                                                  num_scenes, num_goals, parts, slack, _lib.SCHEDULE_LONGEST_FIRST, _ptr(out), _stream()),
                  "omgx_goalset_schedule_ordered")
        elif parts != 1:
            check(l.omgx_goalset_schedule_parts(_ptr(work), _ptr(_active(active, num_scenes)), _ptr(_active(goal_count, num_scenes)),
                                                num_scenes, num_goals, parts, slack, _ptr(out), _stream()), "omgx_goalset_schedule_parts")
        else:
            check(l.omgx_goalset_schedule(_ptr(work), _ptr(_active(active, num_scenes)), _ptr(_active(goal_count, num_scenes)), num_scenes,
                                          num_goals, slack, _ptr(out), _stream()), "omgx_goalset_schedule")
    return out


def forward_kinematics(robot, P, joints, want_joint_info=True):
    """joints [B,9] f64 -> link poses [B,10,4,4], joint origins [B,10,3] | None, joint axes [B,10,3] | None."""
    _need(joints, torch.float64, "joints")
    B, dev = joints.shape[0], joints.device
    poses = torch.empty((B, 10, 4, 4), dtype=torch.float64, device=dev)
    org = torch.empty((B, 10, 3), dtype=torch.float64, device=dev) if want_joint_info else None
    ax = torch.empty((B, 10, 3), dtype=torch.float64, device=dev) if want_joint_info else None
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_forward_kinematics(_ptr(robot), P, _ptr(joints), B, _ptr(poses), _ptr(org), _ptr(ax), _stream()),
              "omgx_forward_kinematics")
    return poses, org, ax


def pose_table(robot, P, configs: torch.Tensor, out: "torch.Tensor | None" = None) -> torch.Tensor:
    """configs [..., 9] f64 -> link poses [..., 10, 12] f64 in the step's own layout (omgx_pose_table: rotation rows, translation;
    before center_offset): what ChompParams.start_poses / end_poses and LearnerParams.goal_pose_table point at."""
    _need(configs, torch.float64, "configs")
    N = configs.numel() // 9
    if out is None:
        out = torch.empty(tuple(configs.shape[:-1]) + (10, 12), dtype=torch.float64, device=configs.device)
    else:
        _need(out, torch.float64, "poses")
        if out.numel() != N * 120:
            raise _lib.OmgHipError("poses must hold 120 doubles per configuration")
    with torch.cuda.device(configs.device):
        check(_lib.lib().omgx_pose_table(_ptr(robot), P, _ptr(configs), N, _ptr(out), _stream()), "omgx_pose_table")
    return out


def goal_ik(robot, P, targets: torch.Tensor, grasp_begin, seeds: torch.Tensor, use_standoff: bool = True, attached: bool = False,
            max_iter: int = 100, eps: float = 1e-6, pinv_eps: float = 1e-5, accept_diff: float = 2.0, want_iterations: bool = False):
    """omgx_goal_ik: targets [N,T,12] f64 (omgx_pose_table layout; T = 1 without standoff), grasp_begin [S+1] (host ints: scene s owns
    grasps grasp_begin[s]:grasp_begin[s+1]), seeds [S,K,7] f64 -> (status [N,K] int32, solutions [N,K,T,7] f64 in pose order,
    iterations [N,K,1+T] / [N,K,1] int32 | None).  Enqueued on the current stream."""
    _need(targets, torch.float64, "targets")
    _need(seeds, torch.float64, "seeds")
    dev = targets.device
    if targets.dim() != 3 or targets.shape[2] != 12:
        raise _lib.OmgHipError("targets must be [N, T, 12]")
    N, T = int(targets.shape[0]), int(targets.shape[1])
    h_begin = np.ascontiguousarray(np.asarray(grasp_begin, dtype=np.int32))
    S = h_begin.size - 1
    if S < 0 or seeds.dim() != 3 or seeds.shape[0] != S or seeds.shape[2] != 7:
        raise _lib.OmgHipError("seeds must be [S, K, 7] with S = len(grasp_begin) - 1")
    K = int(seeds.shape[1])
    d_begin = torch.from_numpy(h_begin).to(dev)
    status = torch.empty((N, K), dtype=torch.int32, device=dev)
    sols = torch.empty((N, K, T, 7), dtype=torch.float64, device=dev)
    its = torch.empty((N, K, 1 + T if use_standoff else 1), dtype=torch.int32, device=dev) if want_iterations else None
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_goal_ik(_ptr(robot), P, _ptr(targets), _ptr(d_begin), h_begin.ctypes.data_as(C.c_void_p), S, N,
                                      _ptr(seeds), K, T, int(bool(use_standoff)), int(bool(attached)), int(max_iter), float(eps),
                                      float(pinv_eps), float(accept_diff), _ptr(status), _ptr(sols), _ptr(its), _stream()),
              "omgx_goal_ik")
    return status, sols, its


def select_goals(goals: torch.Tensor, goal_count, collide: "torch.Tensor | None" = None, allow_collision_point=5,
                 filter_diversity: bool = True):
    """omgx_select_goals: the collision threshold and the greedy diversity filter of Planner.setup_goal_set (planner.py:526-575)
    for S scenes.  goals [S,G,9] f64, scene s owning rows [0, goal_count[s]); goal_count: S host integers (checked here), or an
    integer device tensor (checked on the device: a scene out of [0, G] reports -1 in both counts); collide [S,G] f32
    (goalset.goal_collision_stats) or None: no collision filter.
    -> (candidates [S,G] int32: the rows the reference's `indexes` name, in order, valid in [0, num_candidates[s]);
    num_candidates [S] int32, 0 = "IK FAIL"; num_free [S] int32), on the device.  Enqueued on the current stream."""
    if not isinstance(goals, torch.Tensor) or goals.dim() != 3 or goals.shape[2] != 9:
        raise _lib.OmgHipError("goals must be a [S, G, 9] tensor")
    if goals.dtype != torch.float64:
        raise _lib.OmgHipError(f"goals must be torch.float64, got {goals.dtype}")
    S, G = int(goals.shape[0]), int(goals.shape[1])
    if G > _lib.SELECT_MAX_GOALS:
        raise _lib.OmgHipError(f"at most {_lib.SELECT_MAX_GOALS} goals per scene")
    h_count = d_count = None
    if isinstance(goal_count, torch.Tensor) and goal_count.is_cuda:
        if tuple(goal_count.shape) != (S,) or goal_count.dtype not in (torch.int32, torch.int64):
            raise _lib.OmgHipError("goal_count must hold S integers")
        d_count = goal_count.to(torch.int32).contiguous()
    else:
        gc = np.asarray(goal_count.numpy() if isinstance(goal_count, torch.Tensor) else goal_count)
        if gc.shape != (S,) or (S and not np.issubdtype(gc.dtype, np.integer)):
            raise _lib.OmgHipError("goal_count must hold S integers")
        if S and (gc.min() < 0 or gc.max() > G):
            raise _lib.OmgHipError(f"goal_count must lie in [0, {G}]")
        h_count = np.ascontiguousarray(gc, dtype=np.int32)
    if collide is not None:
        if not isinstance(collide, torch.Tensor) or tuple(collide.shape) != (S, G):
            raise _lib.OmgHipError("collide must be a [S, G] tensor")
        if collide.dtype != torch.float32:
            raise _lib.OmgHipError(f"collide must be torch.float32, got {collide.dtype}")
    allow = float(allow_collision_point)
    if allow != allow:
        raise _lib.OmgHipError("allow_collision_point is NaN")
    _need(goals, torch.float64, "goals")
    if collide is not None:
        _need(collide, torch.float32, "collide")
    dev = goals.device
    if d_count is None:
        d_count = torch.from_numpy(h_count).to(dev)
    cand = torch.empty((S, G), dtype=torch.int32, device=dev)
    counts = torch.empty((2, S), dtype=torch.int32, device=dev)
    l = _lib.lib()
    with torch.cuda.device(dev):
        ws = _workspace(l.omgx_select_goals_workspace_bytes(S, G), dev) if filter_diversity else None
        check(l.omgx_select_goals(_ptr(goals), _ptr(d_count), None if h_count is None else h_count.ctypes.data_as(C.c_void_p),
                                  S, G, _ptr(collide), allow, int(bool(filter_diversity)), _ptr(cand), _ptr(counts[0]),
                                  _ptr(counts[1]), _ptr(ws), _stream()), "omgx_select_goals")
    return cand, counts[0], counts[1]


def chomp_optimize(robot, params: ChompParams, traj, start, end, goal, goal_point, pot, pgrad, col, active=None, out=None,
                   aux=None, stop_on_terminate=False):
    """In-place step on traj [S,n,9] f64 -> grad [S,n,9], cost_traj [S,n], info [S,16] (f64).
    aux: optional [S, omgx_chomp_aux_doubles(n)] f64 receiving obs_grad | obs_cost | smooth_grad | smooth_loss."""
    for n_, t in (("traj", traj), ("start", start), ("end", end), ("goal", goal), ("goal_point", goal_point)):
        _need(t, torch.float64, n_)
    for n_, t in (("potentials", pot), ("grads", pgrad), ("collides", col)):
        _need(t, torch.float32, n_)
    S, n = traj.shape[0], traj.shape[1]
    dev = traj.device
    if out is None:
        grad = torch.empty((S, n, 9), dtype=torch.float64, device=dev)
        cost_traj = torch.empty((S, n), dtype=torch.float64, device=dev)
        info = torch.zeros((S, _lib.INFO_STRIDE), dtype=torch.float64, device=dev)
    else:
        grad, cost_traj, info = out
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_chomp_optimize(_ptr(robot), C.byref(params), _ptr(traj), _ptr(start), _ptr(end), _ptr(goal),
                                             _ptr(goal_point), _ptr(pot), _ptr(pgrad), _ptr(col), _ptr(active), S,
                                             _ptr(grad), _ptr(cost_traj), _ptr(info), _ptr(aux), int(bool(stop_on_terminate)),
                                             _stream()), "omgx_chomp_optimize")
    return grad, cost_traj, info


def learner_state(S: int, G: int, device, goal_count=None) -> torch.Tensor:
    """Initial Learner state [S, 7G+10] f64: sum_costs 0 | p 1/G | experts_p 1/G | q 1/5 | experts_costs 0
    (Learner.__init__, omg/online_learner.py:66-95).  goal_count [S] (ragged goal sets padded to G): scene s holds
    1 / goal_count[s] in its first goal_count[s] entries and 0 in the padding."""
    st = np.zeros((S, 7 * G + 10), np.float64)  # built on the host: one upload instead of four first-use torch kernels
    if goal_count is None:
        st[:, G:7 * G] = 1.0 / G
    else:
        cnt = np.asarray(goal_count, np.float64).reshape(S, 1)
        row = np.where(np.arange(G)[None, :] < cnt, 1.0 / cnt, 0.0)
        st[:, G:7 * G] = np.tile(row, (1, 6))
    st[:, 7 * G:7 * G + 5] = 0.2
    return torch.from_numpy(st).to(device)


def goal_update(params: LearnerParams, traj, goal_set, reach, goal_cost, state, goal_idx, end, goal_rows, goal_point,
                cost_vector=None, active=None, goal_count=None, eta=None):
    """Learner.update_goal for S scenes in one launch (omgx_goal_update); all outputs are written in place.
    active [S] int32 (optional): scenes with 0 keep goal, outputs and state."""
    _need(traj, torch.float64, "traj")
    _need(goal_set, torch.float64, "goal_set")
    _need(state, torch.float64, "state")
    if goal_idx.dtype != torch.int32:
        raise _lib.OmgHipError("goal_idx must be int32")
    with torch.cuda.device(traj.device):
        check(_lib.lib().omgx_goal_update(C.byref(params), _ptr(traj), _ptr(goal_set), _ptr(reach), _ptr(goal_cost), _ptr(state),
                                          traj.shape[0], _ptr(goal_idx), _ptr(end), _ptr(goal_rows), _ptr(goal_point),
                                          _ptr(cost_vector), _ptr(_active(active, traj.shape[0])),
                                          _ptr(_active(goal_count, traj.shape[0])), _ptr(_eta(eta, traj.shape[0])), _stream()), "omgx_goal_update")


def goal_update_optimize(lparams: LearnerParams, goal_set, reach, goal_cost, state, goal_idx, robot, params: ChompParams, traj,
                         start, end, goal, goal_point, pot, pgrad, col, active=None, out=None, aux=None, cost_vector=None,
                         scene_flags=None, ticket=0, stop_on_terminate=False, goal_count=None, eta=None):
    """goal_update followed by chomp_optimize in one launch (omgx_goal_update_optimize): same results as the two calls."""
    S, n = traj.shape[0], traj.shape[1]
    dev = traj.device
    if out is None:
        grad = torch.empty((S, n, 9), dtype=torch.float64, device=dev)
        cost_traj = torch.empty((S, n), dtype=torch.float64, device=dev)
        info = torch.zeros((S, _lib.INFO_STRIDE), dtype=torch.float64, device=dev)
    else:
        grad, cost_traj, info = out
    _layer(S, params.n_points, traj, (pot, pgrad, col))
    _iteration_tensors(S, goal_set, reach, state, goal_idx, cost_vector, start, end, goal, goal_point, (grad, cost_traj, info), active,
                       goal_count, eta, scene_flags)
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_goal_update_optimize(C.byref(lparams), _ptr(goal_set), _ptr(reach), _ptr(goal_cost), _ptr(state),
                                                   _ptr(goal_idx), _ptr(cost_vector), _ptr(robot), C.byref(params), _ptr(traj),
                                                   _ptr(start), _ptr(end), _ptr(goal), _ptr(goal_point), _ptr(pot), _ptr(pgrad),
                                                   _ptr(col), _ptr(active), S, _ptr(grad), _ptr(cost_traj), _ptr(info), _ptr(aux),
                                                   _ptr(scene_flags), int(ticket), int(bool(stop_on_terminate)),
                                                   _ptr(goal_count), _ptr(eta), _stream()),
              "omgx_goal_update_optimize")
    return grad, cost_traj, info


class IterationCalls:
    """The two launches of a planner iteration (omgx_goalset_cost_layer with traj_start = traj[:, k], then
    omgx_goal_update_optimize) with their tensor arguments checked and converted ONCE: a steady-state iteration passes ~60
    pointers whose values never change, and re-checking / re-wrapping them costs the host more than the launches
    themselves (48 -> 27 us per iteration; it matters when the iteration is short: small batches, the late iterations of a
    plan, the engine's two-stream pipeline).  Same entry points, same argument meaning as goalset_cost_layer() and
    goal_update_optimize(); whoever rebinds one of the tensors builds a new object (ChompEngine keys it on their identities)."""

    def __init__(self, robot, P, scenes: DeviceScenes, goals, dt, traj, layer_out, goal_out, goal_set, reach, state, goal_idx,
                 start, end, goal_rows, goal_point, step_out, cost_vector, active, goal_count=None, eta=None, scene_flags=None,
                 layer_soften_fingers=False, tiling=None, layer_poses=None, goal_parts=1, prepass=False):
        _need(goals, torch.float64, "goals")
        S, G = goals.shape[0], goals.shape[1]
        layer = _layer(S, P, traj, layer_out, layer_poses)
        n = layer[1]
        # tiling = (goal_parts, layer_link_groups, layer_config_block, spread): the launches go through omgx_goalset_cost_layer_tiled
        # (latency mode), goal_cost / collides then hold [S][G][parts] partial sums
        self._tiling = None if tiling is None else tuple(int(v) for v in tiling)
        # goal_parts > 1 without a tiling: the batch kernel with split goals (omgx_goalset_cost_layer_parts), schedules over (scene, goal, part)
        self._goal_parts = int(goal_parts) if self._tiling is None else 1
        max_parts = self._tiling[0] if self._tiling is not None else self._goal_parts
        goal_ptrs = _goal_out(goal_out, S * G * (goalset_parts(n, max_parts) if max_parts != 1 else 1))
        _iteration_tensors(S, goal_set, reach, state, goal_idx, cost_vector, start, end, goal_rows, goal_point, step_out, active, goal_count,
                           eta, scene_flags)
        self.S, self.G, self.n, self.P, self.dt = S, G, n, int(P), float(dt)
        self.device = traj.device
        self._dev_index = traj.device.index if traj.device.index is not None else torch.cuda.current_device()
        self._traj_addr = traj.data_ptr()
        l = _lib.lib()
        self._f_gs, self._f_up = l.omgx_goalset_cost_layer, l.omgx_goal_update_optimize
        self._f_gst = l.omgx_goalset_cost_layer_tiled
        self._f_gsp = l.omgx_goalset_cost_layer_parts
        # prepass: the goals' kinematics as a launch of their own (k_goalset_kin) through a workspace this object owns — launches of
        # different IterationCalls may run at once on different streams
        self.kin_workspace = (torch.empty(max(16, l.omgx_goalset_workspace_bytes(S, G, n, self.P)), dtype=torch.uint8, device=traj.device)
                              if prepass else None)
        self._gs = _GoalsetArgs(robot, P, scenes, goals, S, G, dt, False, goal_ptrs, layer, layer_soften_fingers, goal_count, self.kin_workspace)
        self._layer_alone = _GoalsetArgs(robot, P, scenes, None, S, 0, dt, False, (None, None), layer, layer_soften_fingers, None, None)
        p = _ptr
        self._active_p = p(active)
        traj_p, _n, lp, lg, lc, _poses = layer
        grad, cost_traj, info = step_out
        self._up_a = (p(goal_set), p(reach), goal_ptrs[0], p(state), p(goal_idx), p(cost_vector), p(robot))
        self._up_b = (traj_p, p(start), p(end), p(goal_rows), p(goal_point), lp, lg, lc, p(active), S, p(grad), p(cost_traj), p(info), None)
        self._flags, self._eta = p(scene_flags), p(eta)
        self.use_layer_poses = False  # set per launch by the owner: only while the step that follows takes the poses

    def goalset_layer(self, start_idx: int, masked: bool, schedule, work, stream):
        """omgx_goalset_cost_layer for traj_start = traj[:, start_idx], n_remaining = n - start_idx.  schedule / work: checked
        int32 device tensors or None; stream: a HIP stream handle (int)."""
        g, start, n_remaining = self._gs, (C.c_void_p(self._traj_addr + 72 * start_idx), self.n * 9), self.n - start_idx
        active, poses, stream = self._active_p if masked else None, g.poses if self.use_layer_poses else None, C.c_void_p(stream)
        if self._tiling is not None:
            if schedule is not None or work is not None:
                raise _lib.OmgHipError("a tiled goal-set launch takes no dispatch schedule")
            self._call(self._f_gst, g.tiled(start, n_remaining, active, self._tiling, poses, stream))
        elif self._goal_parts > 1 or self.use_layer_poses:
            NP = goalset_parts(n_remaining, self._goal_parts) if self._goal_parts > 1 else 1
            self._call(self._f_gsp, g.parts(start, n_remaining, active, schedule, work, NP, self._goal_parts, poses, stream))
        else:
            self._call(self._f_gs, g.whole(start, n_remaining, active, schedule, work, stream))

    def _call(self, fn, args):
        if torch.cuda.current_device() == self._dev_index:
            check(fn(*args), fn.__name__)
        else:
            with torch.cuda.device(self.device):
                check(fn(*args), fn.__name__)

    # (goal_parts, layer_link_groups, layer_config_block, spread) of a layer-ONLY launch in the batch layout (the smoothing iterations of a
    # plan): any split gives the same bits (every element is computed on its own).  Five workgroups per scene (2 links x all waypoints)
    # take 38 us on a chip they fill to a third; TEN (one link each) shorten the launch: plan of 100 scenes 9.06 -> 8.73 ms, with early
    # stop 7.88 -> 7.62 (round 6; config blocks on top: nothing; 13 x 128 and 16 x 64: within the noise either way).  An experiment
    # overrides the rule by setting this attribute, e.g. (1, 5, 0, 0).
    LAYER_ONLY_TILING = None

    def _layer_only_tiling(self):
        if self.LAYER_ONLY_TILING is not None:
            return self.LAYER_ONLY_TILING
        S = getattr(self, "batch_scenes", self.S)  # set by the engine (a pipeline part's calls know the batch)
        if self.n > 32:
            # Long plans (50 waypoints, a dozen objects): a piece of 2 links x all waypoints is 70 us of work and a batch of 16 scenes has 80 of
            # them on 1 280 slots.  About 1 100 pieces in all, ten link groups x blocks of waypoints: plan of 16 x 64 x 50 x 13 objects 9.94 ->
            # 8.85 ms, 8 x 64 x 50 7.92 -> 6.86, 32 x 64 x 50 13.41 -> 12.22, 100 x 64 x 50 13.23 -> 12.79
            blocks = max(1, min(7, round(110.0 / max(S, 1))))
            return (1, 10, 0 if blocks == 1 else -(-self.n // blocks), 0)
        return (1, 10, 0, 0) if S >= 32 else (1, 10, 8, 0)  # small batches: 40 pieces per scene (13 x 128: plan 4.72 -> 4.48 by the pieces, 4.26 with the phase as one part)

    def layer_only(self, stream):
        """The SDF layer of the current trajectories alone (omgx_goalset_cost_layer_tiled with num_goals = 0): what omgx_fk_sdf
        computes for the step, with this object's tiling (latency mode) or five workgroups per scene (batch layout)."""
        g = self._layer_alone
        tl = self._tiling if self._tiling is not None else self._layer_only_tiling()
        self._call(self._f_gst, g.tiled((None, 9), 1, None, tl, g.poses if self.use_layer_poses else None, C.c_void_p(stream)))

    def step(self, params: ChompParams, stop_on_terminate: bool, stream):
        """omgx_chomp_optimize on the layer outputs this object's launches write."""
        robot = self._up_a[6]
        traj, start, end, goal_rows, goal_point, lp, lg, lc, active, S, grad, cost_traj, info, _aux = self._up_b
        args = (robot, C.byref(params), traj, start, end, goal_rows, goal_point, lp, lg, lc, active, S, grad, cost_traj, info, None,
                int(bool(stop_on_terminate)), C.c_void_p(stream))
        self._call(_lib.lib().omgx_chomp_optimize, args)

    def goal_update(self, lparams: LearnerParams, stream):
        """omgx_goal_update alone (the learner without the step) on the goal costs the last goalset_layer() left."""
        goal_set, reach, cost, state, goal_idx, cost_vector, _robot = self._up_a
        traj, _start, end, goal_rows, goal_point = self._up_b[:5]
        args = (C.byref(lparams), traj, goal_set, reach, cost, state, self.S, goal_idx, end, goal_rows, goal_point, cost_vector,
                None, self._gs.goal_count, self._eta, C.c_void_p(stream))
        self._call(_lib.lib().omgx_goal_update, args)

    def update(self, lparams: LearnerParams, params: ChompParams, split: bool, ticket: int, stop_on_terminate: bool, stream):
        """omgx_goal_update_optimize."""
        args = (C.byref(lparams), *self._up_a, C.byref(params), *self._up_b, self._flags if split else None, int(ticket),
                int(bool(stop_on_terminate)), self._gs.goal_count, self._eta, C.c_void_p(stream))
        self._call(self._f_up, args)


def plan_persistent(robot, P, scenes: DeviceScenes, goals, dt, traj, layer_out, layer_poses, goal_out, lparams: LearnerParams, goal_set, reach,
                    state, goal_idx, cost_vector, params: ChompParams, start, end, goal_rows, goal_point, step_out, iters, d_iters, workspace,
                    active=None, goal_count=None, eta=None, soften_fingers=False, layer_soften_fingers=False, max_workgroups=0, update_cus=-1):
    """omgx_plan_persistent: len(iters) iterations of the planner loop (omg/planner.py:612-630) for every scene in ONE launch
    (csrc/omg_persist.h) on the current stream.  iters: a ctypes array of _lib.PlanIter (host); d_iters: a uint8 device tensor holding the
    same bytes; workspace: uint8 device tensor of omgx_plan_persistent_workspace_bytes(S, n).  The same tensors as
    goalset_cost_layer() + goal_update_optimize(); the pose hand-over (params.start_poses / end_poses, lparams.goal_pose_table /
    end_poses_out, layer_poses) is required."""
    _need(goals, torch.float64, "goals")
    S, G = goals.shape[0], goals.shape[1]
    if layer_poses is None:
        raise _lib.OmgHipError("plan_persistent needs layer_poses (the pose hand-over)")
    traj_p, n, lp, lg, lc, poses = _layer(S, P, traj, layer_out, layer_poses)
    cost, col = _goal_out(goal_out, S * G)
    _iteration_tensors(S, goal_set, reach, state, goal_idx, cost_vector, start, end, goal_rows, goal_point, step_out, active, goal_count, eta)
    grad, cost_traj, info = step_out
    K = len(iters)
    if not (d_iters.is_cuda and d_iters.dtype == torch.uint8 and d_iters.numel() >= K * C.sizeof(_lib.PlanIter)):
        raise _lib.OmgHipError("d_iters must be a uint8 device tensor holding the iteration table")
    l = _lib.lib()
    need = l.omgx_plan_persistent_workspace_bytes(S, n)
    if not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.numel() >= need):
        raise _lib.OmgHipError(f"workspace must be a uint8 device tensor of {need} bytes")
    with torch.cuda.device(traj.device):
        check(l.omgx_plan_persistent(_ptr(robot), int(P), _ptr(scenes.objects), _ptr(scenes.scene_begin), _ptr(scenes.pool), _ptr(goals), S, G,
                                     float(dt), int(bool(soften_fingers)), cost, col, traj_p, n, int(bool(layer_soften_fingers)),
                                     lp, lg, lc, poses, _ptr(active), _ptr(goal_count),
                                     C.byref(lparams), _ptr(goal_set), _ptr(reach), _ptr(state), _ptr(goal_idx), _ptr(cost_vector), _ptr(eta),
                                     C.byref(params), _ptr(start), _ptr(end), _ptr(goal_rows), _ptr(goal_point), _ptr(grad), _ptr(cost_traj), _ptr(info),
                                     iters, _ptr(d_iters), K, _ptr(workspace), workspace.numel(), int(max_workgroups), int(update_cus), _stream()),
              "omgx_plan_persistent")


def plan_persistent_status(workspace, num_scenes: int) -> dict:
    """{"failure", "scenes_finished", "scenes_planned", "activations"} of the last omgx_plan_persistent on `workspace` (synchronises)."""
    st = (C.c_int32 * 4)()
    with torch.cuda.device(workspace.device):
        check(_lib.lib().omgx_plan_persistent_status(_ptr(workspace), int(num_scenes), st, _stream()), "omgx_plan_persistent_status")
    return {"failure": int(st[0]), "scenes_finished": int(st[1]), "scenes_planned": int(st[2]), "activations": int(st[3])}


def point_cloud_sdf(points: torch.Tensor, grid_resolution: float = 0.02, margin: float = 0.24, out: "torch.Tensor | None" = None):
    """PointEnv.compute_sdf_from_points (omg/core.py:426-457) on the device: points [N,3] f64 (robot base frame) ->
    (grid float32 [X,Y,Z] of nearest-point distances, origin [3] float64 numpy, resolution).  The workspace bounds
    are the cloud's bounding box +- margin and the nodes np.arange(lo, hi, resolution), as in the reference.
    out: optional contiguous float32 device tensor with X*Y*Z elements (e.g. a slice of env.sdf_torch) written IN PLACE
    through its raw pointer; its autograd version counter is bumped so that caches keyed on it (Cost's object table and
    influence boxes) notice.  A caller that writes such a volume through the C ABI itself must do the same
    (torch.autograd.graph.increment_version) or call Cost.invalidate()."""
    _need(points, torch.float64, "points")
    lo = points.min(0).values.cpu().numpy() - margin
    hi = points.max(0).values.cpu().numpy() + margin
    dims = np.array([len(np.arange(lo[a], hi[a], grid_resolution)) for a in range(3)], np.int32)
    if out is None:
        out = torch.empty(tuple(int(d) for d in dims), dtype=torch.float32, device=points.device)
    else:
        _need(out, torch.float32, "out")
        if out.numel() != int(dims.prod()):
            raise _lib.OmgHipError(f"out must hold {int(dims.prod())} elements (grid {tuple(int(d) for d in dims)})")
        torch.autograd.graph.increment_version(out)
    origin = np.ascontiguousarray(lo, np.float64)
    with torch.cuda.device(points.device):
        check(_lib.lib().omgx_point_cloud_sdf(_ptr(points), points.shape[0], origin.ctypes.data_as(C.c_void_p),
                                              float(grid_resolution), dims.ctypes.data_as(C.c_void_p), _ptr(out),
                                              _stream()), "omgx_point_cloud_sdf")
    return out, origin, float(grid_resolution)


class MeshPool:
    """Host meshes [(verts [V,3] float, faces [F,3] int)] as omgx_mesh_sdf, omgx_mesh_raycast and omgx_grasp_poses take them:
    each cleaned (scenes.clean_mesh) and appended to `verts` [V,3] float64 and `faces` [F,3] int32, its rows of both in `rec`
    (omgx_mesh records).  Faces of zero area are dropped and counted in `dropped`, or rejected (drop_zero_area=False).  The
    volume fields of a record are set_volume's; first_workgroup is the caller's."""

    def __init__(self, meshes, drop_zero_area: bool):
        if len(meshes) < 1:
            raise _lib.OmgHipError("a batch of meshes needs at least one mesh")
        self.rec = (_lib.Mesh * len(meshes))()
        vs, fs, self.dropped = [], [], []
        v0 = f0 = 0
        for m, (verts, faces) in enumerate(meshes):
            try:
                verts, faces, dropped = _sc.clean_mesh(verts, faces)
            except ValueError as e:
                raise _lib.OmgHipError(f"mesh {m}: {e}") from None
            if dropped and not drop_zero_area:
                raise _lib.OmgHipError(f"mesh {m}: {dropped} faces of zero area (scenes.clean_mesh removes them; face indices stay as given here)")
            r = self.rec[m]
            r.vert_begin, r.vert_count, r.face_begin, r.face_count = v0, len(verts), f0, len(faces)
            v0, f0 = v0 + len(verts), f0 + len(faces)
            vs.append(verts), fs.append(faces), self.dropped.append(dropped)
        self.verts, self.faces = np.concatenate(vs), np.concatenate(fs)

    def set_volume(self, m: int, origin, delta, sample, dims, out_offset, padding=4):
        """The grid of mesh m's volume into its record: origin [3] and nodes per axis (both None: scenes.mesh_grid_layout with
        `padding`), node spacing, "centre" or "node", the element offset of the volume in its buffer -> (origin, dims)."""
        if sample not in _sc.MESH_SAMPLE_OFFSET:
            raise _lib.OmgHipError(f"mesh {m}: sample must be 'centre' or 'node', got {sample!r}")
        r = self.rec[m]
        origin, dims = _mesh_grid(self.verts[r.vert_begin: r.vert_begin + r.vert_count], delta, padding, origin, dims, m)
        if len(dims) != 3 or min(dims) < 1 or int(out_offset) < 0:
            raise _lib.OmgHipError(f"mesh {m}: the three dims must be >= 1 and the offset >= 0, got {dims} and {out_offset}")
        r.origin[:], r.delta, r.sample_offset, r.dims[:] = list(origin), float(delta), _sc.MESH_SAMPLE_OFFSET[sample], list(dims)
        r.out_offset = int(out_offset)
        return origin, dims

    def upload(self, device):
        """(vertex pool, face pool, records as bytes) on `device`; the records as they are now."""
        return (torch.from_numpy(self.verts).to(device), torch.from_numpy(self.faces).to(device),
                torch.from_numpy(np.frombuffer(self.rec, np.uint8).copy()).to(device))


def _mesh_grid(verts, delta, padding, origin, dims, m: int = 0):
    """(origin [3] float64, dims as ints) of mesh m's grid: as given, or scenes.mesh_grid_layout's around `verts`."""
    if not (float(delta) > 0 and np.isfinite(float(delta))):
        raise _lib.OmgHipError(f"mesh {m}: delta must be positive and finite, got {delta}")
    if (origin is None) != (dims is None):
        raise _lib.OmgHipError(f"mesh {m}: give origin and dims together")
    if origin is None:
        origin, dims = _sc.mesh_grid_layout(verts, float(delta), padding)
    return np.asarray(origin, np.float64).copy(), tuple(int(d) for d in dims)


def mesh_sdf_batch(meshes, delta, padding=4, sample="centre", origins=None, dims=None, out=None, out_offsets=None, device="cuda:0"):
    """Signed distance grids of M triangle meshes in ONE launch (omgx_mesh_sdf; scenes.mesh_sdf is the specification: the same
    float32 magnitudes bit for bit, the sign from the winding number's decision |w| > 0.5).
    meshes: a list of (verts [V,3] float, faces [F,3] int) on the host; delta / padding / sample: one value for all or a list
    with one per mesh; origins / dims: None (scenes.mesh_grid_layout per mesh) or lists with an explicit layout per mesh.
    out: None -> one flat float32 buffer holding the volumes back to back; or a contiguous float32 device tensor (the SDF
    pool, for instance) written IN PLACE at the element offsets `out_offsets` (one per mesh; the volumes must not overlap), its
    autograd version counter bumped like point_cloud_sdf does.
    -> (grids: M float32 [X,Y,Z] views into the buffer, origins: M float64 [3], deltas: M floats, dropped: M counts of zero-area
    faces left out).  Raises OmgHipError on indices outside a mesh's vertices, a mesh left without faces, a bad layout."""
    M = len(meshes)

    def per_mesh(x, name):
        if isinstance(x, (list, tuple)):
            if len(x) != M:
                raise _lib.OmgHipError(f"{name} must have one entry per mesh ({M}), got {len(x)}")
            return list(x)
        return [x] * M
    deltas, pads, samples = per_mesh(delta, "delta"), per_mesh(padding, "padding"), per_mesh(sample, "sample")
    if (origins is None) != (dims is None):
        raise _lib.OmgHipError("give origins and dims together")
    if origins is not None and (len(origins) != M or len(dims) != M):
        raise _lib.OmgHipError(f"origins and dims must have one entry per mesh ({M})")
    if out_offsets is not None and len(out_offsets) != M:
        raise _lib.OmgHipError(f"out_offsets must have one entry per mesh ({M})")
    mp = MeshPool(meshes, drop_zero_area=True)
    shapes, org = [], []
    wg = flat = 0
    for m in range(M):
        o, d = mp.set_volume(m, None if origins is None else origins[m], deltas[m], samples[m], None if dims is None else dims[m],
                             flat if out_offsets is None else out_offsets[m], pads[m])
        n = d[0] * d[1] * d[2]
        mp.rec[m].first_workgroup = wg  # the prefix table that maps a workgroup to its mesh
        wg += -(-n // _lib.MESH_SDF_NODES_PER_WORKGROUP)
        flat += n
        shapes.append(d), org.append(o)
    if out is None:
        if out_offsets is not None:
            raise _lib.OmgHipError("out_offsets needs out")
        out = torch.empty(flat, dtype=torch.float32, device=device)
    else:
        _need(out, torch.float32, "out")
        if out_offsets is None and M > 1:
            raise _lib.OmgHipError("out needs out_offsets (one element offset per mesh)")
        spans = sorted((int(mp.rec[m].out_offset), int(np.prod(shapes[m]))) for m in range(M))
        if spans[0][0] < 0 or spans[-1][0] + spans[-1][1] > out.numel() or any(spans[i][0] + spans[i][1] > spans[i + 1][0] for i in range(M - 1)):
            raise _lib.OmgHipError(f"the volumes (offset, elements) {spans} overlap or leave out ({out.numel()} elements)")
        torch.autograd.graph.increment_version(out)
    dev = out.device
    d_verts, d_faces, d_rec = mp.upload(dev)
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_mesh_sdf(_ptr(d_verts), _ptr(d_faces), _ptr(d_rec), C.cast(mp.rec, C.c_void_p), M, _ptr(out), _stream()),
              "omgx_mesh_sdf")
        for t in (d_verts, d_faces, d_rec):
            t.record_stream(torch.cuda.current_stream(dev))
    flat_out = out.reshape(-1)
    grids = [flat_out[int(mp.rec[m].out_offset): int(mp.rec[m].out_offset) + int(np.prod(shapes[m]))].view(shapes[m]) for m in range(M)]
    return grids, org, [float(x) for x in deltas], mp.dropped


def mesh_sdf(verts, faces, delta, padding=4, sample="centre", origin=None, dims=None, out=None, device="cuda:0"):
    """Signed distance grid of one triangle mesh on the device -> (grid float32 [X,Y,Z], origin [3] float64 numpy, delta).
    scenes.mesh_sdf with the same arguments is the specification.  out: a contiguous float32 device tensor with X*Y*Z elements,
    e.g. DeviceScenes.grid_slot(scene, obj, dims) with dims from scenes.mesh_grid_layout — written IN PLACE, ready for
    DeviceScenes.replace_grid(scene, obj, grid, origin, delta).  Faces of zero area are dropped (their number is logged at
    debug level; mesh_sdf_batch returns it)."""
    if out is not None:
        _need(out, torch.float32, "out")
        _, d = _mesh_grid(np.asarray(verts, np.float64), delta, padding, origin, dims)
        if out.numel() != d[0] * d[1] * d[2]:
            raise _lib.OmgHipError(f"out must hold {d[0] * d[1] * d[2]} elements (grid {d})")
    grids, org, deltas, dropped = mesh_sdf_batch([(verts, faces)], delta, padding, sample, None if origin is None else [origin],
                                                 None if dims is None else [dims], out=out, out_offsets=None if out is None else [0],
                                                 device=device)
    if dropped[0]:
        import logging
        logging.getLogger(__name__).debug("mesh_sdf: dropped %d faces of zero area", dropped[0])
    return grids[0], org[0], deltas[0]


def surface_records(volumes):
    """omgx_mesh records (a ctypes array) of the volumes [(origin [3], delta, "centre" or "node", dims [3], element offset in the
    pool)] for omgx_surface_count / omgx_surface_gather, first_workgroup filled in; the vert / face fields are left zero.  An array
    of records passes through a copy (its first_workgroup is rewritten)."""
    if isinstance(volumes, C.Array) and getattr(volumes, "_type_", None) is _lib.Mesh:
        rec = (_lib.Mesh * len(volumes))()
        C.memmove(rec, volumes, C.sizeof(rec))
    else:
        volumes = list(volumes)
        rec = (_lib.Mesh * len(volumes))()
        for m, (origin, delta, sample, dims, offset) in enumerate(volumes):
            if sample not in _sc.MESH_SAMPLE_OFFSET:
                raise _lib.OmgHipError(f"volume {m}: sample must be 'centre' or 'node', got {sample!r}")
            origin, dims = np.asarray(origin, np.float64).reshape(-1), [int(d) for d in np.asarray(dims).reshape(-1)]
            if len(origin) != 3 or len(dims) != 3 or min(dims) < 1 or int(offset) < 0:
                raise _lib.OmgHipError(f"volume {m}: origin [3], three dims >= 1 and an offset >= 0, got {origin}, {dims} and {offset}")
            if not (float(delta) > 0 and np.isfinite(float(delta)) and np.isfinite(origin).all()):
                raise _lib.OmgHipError(f"volume {m}: delta must be positive and finite and the origin finite, got {delta} and {origin}")
            r = rec[m]
            r.origin[:], r.delta, r.sample_offset, r.dims[:], r.out_offset = list(origin), float(delta), _sc.MESH_SAMPLE_OFFSET[sample], dims, int(offset)
    if len(rec) < 1:
        raise _lib.OmgHipError("a batch of volumes needs at least one volume")
    wg = 0
    for r in rec:
        r.first_workgroup = wg
        wg += -(-(int(r.dims[0]) * int(r.dims[1]) * int(r.dims[2])) // _lib.SURFACE_NODES_PER_WORKGROUP)
    return rec


def surface_meshes(pool: torch.Tensor, records_or_layouts, level: float = 0.0, out=None):
    """The level sets {v = level} of M volumes of `pool` as closed, outward-oriented triangle meshes, on the device
    (omgx_surface_count, omgx_surface_gather; scenes.surface_nets is the specification: the same float64 vertices bit for bit, the
    same faces in the same order).  pool: a contiguous float32 device tensor (the SDF pool, or any volume) read IN PLACE;
    records_or_layouts: what surface_records takes.  Count, ONE download of the counts, an exact allocation, gather.
    -> (verts [V_total,3] float64, faces [F_total,3] int32 with indices local to their mesh: device; vert_rows [M,2] and
    face_rows [M,2] = (begin, count) of mesh m's rows, open_edges [M]: host int64).  A mesh with open_edges > 0 left its grid and
    is not closed there.  out: (verts [cap,3], faces [cap,3]) of the caller's, written IN PLACE instead; rows beyond a cap are
    not written (the tables still tell what the mesh has).  The meshes lie back to back from row 0, in order."""
    _need(pool, torch.float32, "pool")
    level = float(level)
    if np.isnan(np.float32(level)):
        raise _lib.OmgHipError("level is NaN")
    rec = surface_records(records_or_layouts)
    M, dev, l, vp = len(rec), pool.device, _lib.lib(), C.c_void_p
    elems = int(pool.numel())
    for m, r in enumerate(rec):
        n = int(r.dims[0]) * int(r.dims[1]) * int(r.dims[2])
        if r.out_offset < 0 or r.out_offset + n > elems:
            raise _lib.OmgHipError(f"volume {m} (offset {r.out_offset}, {n} elements) leaves the pool of {elems}")
    if out is not None:
        for t, name, dt in ((out[0], "out[0]", torch.float64), (out[1], "out[1]", torch.int32)):
            _tensor(t, name, dt, (None, 3), dev)
    nbytes = int(l.omgx_surface_workspace_bytes(C.cast(rec, vp), M))
    check(min(nbytes, 0), "omgx_surface_workspace_bytes")
    with torch.cuda.device(dev):
        ws = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=dev)
        counts = torch.empty((M, 4), dtype=torch.int32, device=dev)
        d_rec = torch.from_numpy(np.frombuffer(rec, np.uint8).copy()).to(dev)
        check(l.omgx_surface_count(_ptr(pool), elems, _ptr(d_rec), C.cast(rec, vp), M, level, _ptr(ws), _ptr(counts), _stream()), "omgx_surface_count")
        h = counts.cpu().numpy().astype(np.int64)
        if h[:, :2].sum(0).max() > 0x7fffffff:
            raise _lib.OmgHipError("the meshes have more rows than int32 ranges address")
        vrows, frows = (np.stack([np.concatenate([[0], np.cumsum(h[:, col])[:-1]]), h[:, col]], -1) for col in (0, 1))
        for m, r in enumerate(rec):
            r.vert_begin, r.vert_count, r.face_begin, r.face_count = int(vrows[m, 0]), int(vrows[m, 1]), int(frows[m, 0]), int(frows[m, 1])
        if out is None:
            out = (torch.empty((int(h[:, 0].sum()), 3), dtype=torch.float64, device=dev), torch.empty((int(h[:, 1].sum()), 3), dtype=torch.int32, device=dev))
        verts, faces = out
        d_rec2 = torch.from_numpy(np.frombuffer(rec, np.uint8).copy()).to(dev)
        check(l.omgx_surface_gather(_ptr(pool), elems, _ptr(d_rec2), C.cast(rec, vp), M, level, _ptr(ws), _ptr(verts) if verts.shape[0] else None,
                                    int(verts.shape[0]), _ptr(faces) if faces.shape[0] else None, int(faces.shape[0]), _stream()), "omgx_surface_gather")
        for t in (ws, d_rec, d_rec2):
            t.record_stream(torch.cuda.current_stream(dev))
    return verts, faces, vrows, frows, h[:, 2].copy()


def surface_mesh(grid: torch.Tensor, origin, delta, sample: str = "centre", level: float = 0.0):
    """The level set of ONE volume, a contiguous float32 [X,Y,Z] device tensor whose sample (i,j,k) sits at
    origin + ((i,j,k) + offset) * delta -> (verts [V,3] float64, faces [F,3] int32 on the device, open_edges).
    scenes.surface_nets with the same arguments is the specification."""
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3:
        raise _lib.OmgHipError("grid must be a tensor [X,Y,Z]")
    verts, faces, _, _, open_edges = surface_meshes(grid, [(origin, delta, sample, tuple(grid.shape), 0)], level)
    return verts, faces, int(open_edges[0])


class _HostBatch:
    """Host arrays of a launch that go to a device once each, when a launch first needs them there.  _caches: one dict per array,
    device -> upload; on(dev) names the device that the arguments point into."""
    _dev = None

    def on(self, dev):
        self._dev = torch.device(dev)
        return self

    def _device(self, cache, host):  # the pointer to `host` on the device in use; None for an empty array, which is not uploaded
        if len(host) and self._dev not in cache:
            cache[self._dev] = _upload(host, self._dev)
        return _ptr(cache.get(self._dev))

    def release(self, *scratch) -> None:  # after a launch: the uploads, and the caller's scratch tensors, are in use by the current stream
        _release(self._dev, *(cache.get(self._dev) for cache in self._caches), *scratch)


class _VolumeBatch(_HostBatch):
    """The volumes of a launch over a ragged batch, checked on the host before any tensor is touched: rec (omgx_mesh records), nodes
    (int64 [M]), begin (state_begin int64 [M]) and M.  volumes: what surface_records takes (the prefix table is the same: 256 nodes
    per workgroup), or [] for an empty launch; a layout without its fifth field, the element offset in the pool, lies behind the
    layout before it (the first at 0).  The records and state_begin go to a device (on) once, when a launch first needs them there.
    like: a batch of the same volumes at other pool offsets, whose state_begin this one shares, uploads included."""

    def __init__(self, volumes, state_begin=None, like: "_VolumeBatch | None" = None):
        assert _lib.FUSION_NODES_PER_WORKGROUP == _lib.SURFACE_NODES_PER_WORKGROUP == _lib.PLANE_NODES_PER_WORKGROUP
        rec = volumes if isinstance(volumes, C.Array) else [tuple(v) for v in volumes]
        if not isinstance(rec, C.Array):
            at = 0
            for m, v in enumerate(rec):
                if len(v) == 4:
                    rec[m] = v + (at,)
                if len(rec[m]) != 5:
                    raise _lib.OmgHipError(f"volume {m}: (origin, delta, sample, dims[, offset]), got {len(v)} fields")
                at = int(rec[m][4]) + int(np.prod([int(d) for d in np.asarray(v[3]).reshape(-1)]))
        self.rec = surface_records(rec) if len(rec) else (_lib.Mesh * 0)()
        self.M = len(self.rec)
        self.nodes = np.array([int(r.dims[0]) * int(r.dims[1]) * int(r.dims[2]) for r in self.rec], np.int64)
        if like is not None:
            state_begin = like.begin
        self.begin = np.cumsum(self.nodes) - self.nodes if state_begin is None else np.ascontiguousarray(state_begin, np.int64).reshape(-1)
        if len(self.begin) != self.M:
            raise _lib.OmgHipError(f"state_begin must have one offset per volume ({self.M}), got {len(self.begin)}")
        self._caches = self._d_rec, self._d_begin = {}, {} if like is None else like._d_begin

    @classmethod
    def of(cls, volumes, state_begin=None) -> "_VolumeBatch":
        """A batch passes through as it is (with its own state_begin), anything else is made one."""
        return volumes if isinstance(volumes, cls) else cls(volumes, state_begin)

    def end(self) -> int:
        """Elements that the state ranges reach to: what sizes a new state buffer."""
        return int((self.begin + self.nodes).max()) if self.M else 0

    def pool_end(self) -> int:
        """Elements of the pool that the volumes reach to, 1 without any: what sizes a new pool."""
        return max([int(r.out_offset) + int(n) for r, n in zip(self.rec, self.nodes)], default=1)

    def host_args(self):
        """(h_volumes, num_volumes) of an entry point; no pointer for an empty batch."""
        return (C.cast(self.rec, C.c_void_p) if self.M else None, self.M)

    def volume_args(self):
        """(volumes, h_volumes, num_volumes) of an entry point."""
        return (self._device(self._d_rec, self.rec), *self.host_args())

    def begin_args(self):
        """(state_begin, h_state_begin) of an entry point."""
        return (self._device(self._d_begin, self.begin), C.c_void_p(self.begin.ctypes.data) if self.M else None)


class _ViewBatch(_HostBatch):
    """The views of a launch, checked on the host before any tensor is touched: h_views (float64 [V,16], fusion.view_rows), h_range
    (view_range, int32 [M,2]: first view and count per volume; set by of), V and the images' (H, W).  depth is only asked for its shape."""

    def __init__(self, views, depth):
        if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
            raise _lib.OmgHipError("depth must be a tensor [V,H,W]")
        self.V, self.H, self.W = (int(d) for d in depth.shape)
        self.h_views, self.h_range = np.ascontiguousarray(views, np.float64).reshape(-1, 16), None
        if len(self.h_views) != self.V:
            raise _lib.OmgHipError(f"{len(self.h_views)} views but {self.V} images")
        if not np.isfinite(self.h_views).all() or (self.h_views[:, :2] == 0).any():
            raise _lib.OmgHipError("a view is not finite or has a focal length of zero")
        self._caches = self._d_views, self._d_range = {}, {}

    @classmethod
    def of(cls, views, view_range, depth, M: int) -> "_ViewBatch":
        """The batch of views [V,16] and view_range [M,2] for depth [V,H,W] and M volumes.  A batch in the place of `views` passes
        through with its ranges and its uploads (view_range is not read), if its V, H, W and M are the call's."""
        self = views if isinstance(views, cls) else cls(views, depth)
        if self.h_range is None:
            h_range = np.asarray(view_range, np.int64).reshape(-1, 2)
            if len(h_range) != M or (h_range < 0).any() or (h_range.sum(1) > self.V).any():
                raise _lib.OmgHipError(f"view_range must be [{M},2] inside [0, {self.V}]")
            self.h_range = np.ascontiguousarray(h_range, np.int32)
        if len(self.h_range) != M or not isinstance(depth, torch.Tensor) or tuple(depth.shape) != (self.V, self.H, self.W):
            raise _lib.OmgHipError(f"these views are for {len(self.h_range)} volumes and depth [{self.V},{self.H},{self.W}]")
        return self

    def view_args(self):
        """(views, h_views, num_views, view_range, h_view_range) of an entry point; no pointer for an empty array."""
        return (self._device(self._d_views, self.h_views), C.c_void_p(self.h_views.ctypes.data) if self.V else None, self.V,
                self._device(self._d_range, self.h_range), C.c_void_p(self.h_range.ctypes.data) if len(self.h_range) else None)


def _upload(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy() if isinstance(a, C.Array) else np.ascontiguousarray(a)).to(dev)


def _record_bytes(a: np.ndarray, dev) -> torch.Tensor:
    """Records of a structured dtype as the bytes they are, on dev."""
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(dev)


def _release(dev, *scratch) -> None:
    """After the last launch that reads them: temporary uploads (None is skipped) are in use by dev's current stream."""
    for t in scratch:
        if t is not None:
            t.record_stream(torch.cuda.current_stream(dev))


def _fusion_radius(radius) -> int:
    radius = int(radius)
    if not 1 <= radius <= _lib.FUSION_MAX_RADIUS:
        raise _lib.OmgHipError(f"radius must lie in [1, {_lib.FUSION_MAX_RADIUS}], got {radius}")
    return radius


def _carve_arguments(volumes, views, view_range, depth, band, near, state_begin):
    """The host side of a carve launch, checked before anything touches the device, in this order: depth's shape and the views,
    band and near, the volumes, view_range -> (the _VolumeBatch, the _ViewBatch).  Batches pass through."""
    views = views if isinstance(views, _ViewBatch) else _ViewBatch(views, depth)
    if not (np.isfinite(float(band)) and np.isfinite(float(near))):
        raise _lib.OmgHipError("band and near must be finite")
    batch = _VolumeBatch.of(volumes, state_begin)
    return batch, _ViewBatch.of(views, view_range, depth, batch.M)


def carve_views(volumes, views, view_range, depth: torch.Tensor, band: float, near: float, state: "torch.Tensor | None" = None,
                state_begin=None, merge: bool = False):
    """The states (0 free, 1 surface, 2 unknown) of the nodes of M volumes from V depth views in ONE launch (omgx_carve_views;
    fusion.carve_views is the specification: the same bytes) -> (state uint8 on the device, state_begin [M] int64 numpy): volume
    m's node L at state[state_begin[m] + L].  volumes: what surface_records takes (the pool offset is not used here); views
    [V,16] float64 on the host (fusion.view_rows; or a _ViewBatch, which brings its view_range); view_range [M,2] host integers (first view, count; ranges may overlap);
    depth [V,H,W]: a contiguous float64 device tensor (render_depth's t), +inf as background.  state / state_begin: None -> a new
    buffer that reaches to the end of the last volume, filled with 2 (unknown) where no volume lies, as the specification's; or
    the caller's, written IN PLACE (elements outside every range are not touched).
    merge: the flags start from what `state` holds, so that carving the views A and merging the views B equals carving both.
    The host arguments are checked first, then the tensors: a refused call has touched nothing."""
    from . import fusion as _fu
    batch, vb = _carve_arguments(volumes, views, view_range, depth, band, near, state_begin)
    if state is None and merge:
        raise _lib.OmgHipError("merge needs the state of an earlier call")
    _need(depth, torch.float64, "depth")
    dev = depth.device
    if state is None:
        state = torch.full((max(batch.end(), 1),), _fu.UNKNOWN, dtype=torch.uint8, device=dev)
    _tensor(state, "state", torch.uint8, None, dev)
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_carve_views(*batch.on(dev).volume_args(), *vb.on(dev).view_args(), *batch.begin_args(), _ptr(depth) if vb.V else None,
                                          vb.H, vb.W, float(band), float(near), int(bool(merge)), _ptr(state), int(state.numel()), _stream()),
              "omgx_carve_views")
        batch.release(), vb.release()
    return state, batch.begin


def distance_transform(state: torch.Tensor, state_begin, volumes, radius: int, unknown_occupied: bool = True, out: "torch.Tensor | None" = None):
    """The signed float32 volumes of M volumes' states in three launches (omgx_distance_transform; fusion.distance_transform is
    the specification: the same bits) -> out: a contiguous float32 device tensor (the SDF pool, for instance) written IN PLACE
    at every volume's element offset (the fifth field of its layout; the volumes must not overlap), or None -> a new buffer
    that reaches to the end of the last volume, zero where no volume lies.  Volume m lies at out[offset : offset + X*Y*Z] as
    [X,Y,Z].  The host arguments are checked first, then the tensors."""
    radius = _fusion_radius(radius)
    batch = _VolumeBatch.of(volumes, state_begin)
    _need(state, torch.uint8, "state")
    dev, l = state.device, _lib.lib()
    if out is None:
        out = torch.zeros(batch.pool_end(), dtype=torch.float32, device=dev)
    _tensor(out, "out", torch.float32, None, dev)
    nbytes = int(l.omgx_distance_transform_workspace_bytes(*batch.host_args(), radius))
    check(min(nbytes, 0), "omgx_distance_transform_workspace_bytes")
    with torch.cuda.device(dev):
        ws = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=dev)
        check(l.omgx_distance_transform(_ptr(state), int(state.numel()), *batch.on(dev).begin_args(), *batch.volume_args(), radius,
                                        int(bool(unknown_occupied)), _ptr(ws), _ptr(out), int(out.numel()), _stream()), "omgx_distance_transform")
        batch.release(ws)
    return out


def fuse_views(volumes, views, view_range, depth: torch.Tensor, band: float, near: float, radius: int, unknown_occupied: bool = True,
               out: "torch.Tensor | None" = None, clear=None):
    """carve_views and distance_transform for M volumes, four launches in all (fusion.fuse_views is the specification) -> out,
    as distance_transform returns it.  The radius is checked before the carve launch.  clear: None, or a step between the two
    halves, clear(state, state_begin, volumes), that changes the state bytes in place (_robot_step)."""
    radius = _fusion_radius(radius)
    batch, vb = _carve_arguments(volumes, views, view_range, depth, band, near, None)  # (one batch of each: uploaded once for all stages)
    state, _ = carve_views(batch, vb, None, depth, band, near)
    if clear is not None:
        clear(state, None, batch)
    return distance_transform(state, None, batch, radius, unknown_occupied, out)


def _tsdf_positive(name: str, x, may_be_inf: bool = False) -> float:
    from . import tsdf as _ts
    try:  # (the specification's own check of trunc, wmax and min_weight, as this module's error)
        return _ts._positive(name, x, may_be_inf)
    except ValueError as e:
        raise _lib.OmgHipError(str(e)) from None


def _tsdf_arguments(volumes, views, view_range, depth, trunc, near, weights, wmax, state_begin):
    """The host side of an integrate launch, checked before anything touches the device: _carve_arguments' result and
    (weights float64 [V] or None, trunc, wmax)."""
    trunc, wmax = _tsdf_positive("trunc", trunc), _tsdf_positive("wmax", wmax, True)
    batch, vb = _carve_arguments(volumes, views, view_range, depth, 0.0, near, state_begin)
    h_w = None
    if weights is not None:
        h_w = np.ascontiguousarray(weights, np.float64).reshape(-1)
        if len(h_w) != vb.V or not np.isfinite(h_w).all() or (h_w < 0).any():
            raise _lib.OmgHipError(f"weights must be {vb.V} finite numbers >= 0")
    return batch, vb, h_w, trunc, wmax


def _tsdf_pair(tsdf, weight, dev=None):
    _need(tsdf, torch.float32, "tsdf")
    _need(weight, torch.float32, "weight")
    dev = tsdf.device if dev is None else dev
    if tsdf.device != dev or weight.device != dev or tsdf.numel() != weight.numel():
        raise _lib.OmgHipError(f"tsdf and weight must have the same number of elements on {dev}")


def tsdf_integrate(volumes, views, view_range, depth: torch.Tensor, trunc: float, near: float, weights=None, wmax: float = float("inf"),
                   tsdf: "torch.Tensor | None" = None, weight: "torch.Tensor | None" = None, state_begin=None, merge: bool = False):
    """The pairs (D: the averaged truncated distance, W: the accumulated weight) of the nodes of M volumes from V depth views in
    ONE launch (omgx_tsdf_integrate; tsdf.integrate is the specification: the same bits) -> (tsdf, weight: float32 on the
    device, state_begin [M] int64 numpy): volume m's node L at state_begin[m] + L of both.  volumes, views, view_range, depth and
    state_begin as carve_views takes them; weights: [V] host numbers >= 0 (None: 1.0 each); wmax caps W, so that old views fade.
    tsdf / weight: None -> new buffers that reach to the end of the last volume, zero where no volume lies; or the caller's,
    written IN PLACE.  merge: the pairs start from what the buffers hold (a further frame), otherwise from (0, 0).
    The host arguments are checked first, then the tensors: a refused call has touched nothing."""
    batch, vb, h_w, trunc, wmax = _tsdf_arguments(volumes, views, view_range, depth, trunc, near, weights, wmax, state_begin)
    if (tsdf is None) != (weight is None):
        raise _lib.OmgHipError("tsdf and weight come together")
    if tsdf is None and merge:
        raise _lib.OmgHipError("merge needs the pairs of an earlier call")
    _need(depth, torch.float64, "depth")
    dev, V = depth.device, vb.V
    if tsdf is None:
        n = max(batch.end(), 1)
        tsdf, weight = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    _tsdf_pair(tsdf, weight, dev)
    with torch.cuda.device(dev):
        d_w = _upload(h_w, dev) if h_w is not None and V else None
        check(_lib.lib().omgx_tsdf_integrate(*batch.on(dev).volume_args(), *vb.on(dev).view_args(), *batch.begin_args(), _ptr(depth) if V else None,
                                             vb.H, vb.W, _ptr(d_w), C.c_void_p(h_w.ctypes.data) if d_w is not None else None, trunc, float(near), wmax,
                                             int(bool(merge)), _ptr(tsdf), _ptr(weight), int(tsdf.numel()), _stream()), "omgx_tsdf_integrate")
        batch.release(d_w), vb.release()
    return tsdf, weight, batch.begin


def tsdf_states(tsdf: torch.Tensor, weight: torch.Tensor, state_begin, volumes, min_weight: float = 1.0,
                state: "torch.Tensor | None" = None) -> torch.Tensor:
    """The state bytes of the pairs in one launch (omgx_tsdf_states; tsdf.states is the specification): 2 (unknown) if
    !(W >= min_weight), else 1 (surface) if D < 0, else 0 (free), at the pairs' own offsets: carve_views' layout, so
    distance_transform, label_components and component_states take them as they are.  state: None -> a new buffer of the pairs'
    length, 2 where no volume lies; or the caller's uint8 tensor of that length, written IN PLACE inside the volumes' ranges."""
    from . import fusion as _fu
    min_weight = _tsdf_positive("min_weight", min_weight)
    batch = _VolumeBatch.of(volumes, state_begin)
    _tsdf_pair(tsdf, weight)
    dev = tsdf.device
    if state is None:
        state = torch.full((tsdf.numel(),), _fu.UNKNOWN, dtype=torch.uint8, device=dev)
    _need(state, torch.uint8, "state")
    if state.device != dev or state.numel() != tsdf.numel():
        raise _lib.OmgHipError(f"state must have the pairs' {tsdf.numel()} elements on {dev}")
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_tsdf_states(_ptr(tsdf), _ptr(weight), int(tsdf.numel()), *batch.on(dev).begin_args(), *batch.volume_args(), min_weight,
                                          _ptr(state), _stream()), "omgx_tsdf_states")
        batch.release()
    return state


def tsdf_blend(tsdf: torch.Tensor, weight: torch.Tensor, state_begin, volumes, trunc: float, min_weight: float, out: torch.Tensor) -> torch.Tensor:
    """The pairs blended into the volumes distance_transform wrote, IN PLACE in `out` (the SDF pool, for instance) at every
    volume's element offset, in one launch (omgx_tsdf_blend; tsdf.blend is the specification: the same bits): where
    W >= min_weight, out = D + (|D| / trunc) * (out - D) unless |D| >= trunc.  The zero level of the result is the TSDF's."""
    trunc, min_weight = _tsdf_positive("trunc", trunc), _tsdf_positive("min_weight", min_weight)
    batch = _VolumeBatch.of(volumes, state_begin)
    _tsdf_pair(tsdf, weight)
    dev = tsdf.device
    _tensor(out, "out", torch.float32, None, dev)
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_tsdf_blend(_ptr(tsdf), _ptr(weight), int(tsdf.numel()), *batch.on(dev).begin_args(), *batch.volume_args(), trunc,
                                         min_weight, _ptr(out), int(out.numel()), _stream()), "omgx_tsdf_blend")
        batch.release()
    return out


def _tsdf_signed(tsdf, weight, begin, volumes, trunc, radius, unknown_occupied, min_weight, out, clear=None):
    batch = _VolumeBatch.of(volumes, begin)  # (one batch: the records and state_begin go to the device once for the three)
    state = tsdf_states(tsdf, weight, None, batch, min_weight)
    if clear is not None:  # (fuse_views' optional step: the state bytes change before the transform reads them)
        clear(state, None, batch)
    out = distance_transform(state, None, batch, radius, unknown_occupied, out)
    return tsdf_blend(tsdf, weight, None, batch, trunc, min_weight, out)


def fuse_tsdf(volumes, views, view_range, depth: torch.Tensor, trunc: float, near: float, radius: int, unknown_occupied: bool = True,
              min_weight: float = 1.0, weights=None, wmax: float = float("inf"), out: "torch.Tensor | None" = None):
    """tsdf_integrate, tsdf_states, distance_transform and tsdf_blend for M volumes, six launches in all (tsdf.fuse is the
    specification) -> out, as distance_transform returns it (with out=pool: written in place, as fuse_views does).  The radius
    and min_weight are checked before the first launch."""
    radius, min_weight = _fusion_radius(radius), _tsdf_positive("min_weight", min_weight)
    tsdf, weight, begin = tsdf_integrate(volumes, views, view_range, depth, trunc, near, weights, wmax)
    return _tsdf_signed(tsdf, weight, begin, volumes, trunc, radius, unknown_occupied, min_weight, out)


class TsdfVolumes:
    """The pairs of M volumes kept on the device across frames: the records and state_begin (uploaded once), tsdf and weight
    (float32, zero at first).  volumes: what surface_records takes; trunc, near and wmax hold for every frame."""

    def __init__(self, volumes, trunc: float, near: float, wmax: float = float("inf"), device="cuda:0", state_begin=None):
        self.trunc, self.wmax, self.near = _tsdf_positive("trunc", trunc), _tsdf_positive("wmax", wmax, True), float(near)
        if not np.isfinite(self.near):
            raise _lib.OmgHipError("band and near must be finite")
        self.volumes = [tuple(v) for v in volumes]
        self._batch = _VolumeBatch(self.volumes, state_begin)
        self.rec, self.nodes, self.state_begin = self._batch.rec, self._batch.nodes, self._batch.begin
        if not len(self.rec):
            raise _lib.OmgHipError("TsdfVolumes needs at least one volume")
        self.device = torch.device(device)
        self.tsdf, self.weight = (torch.zeros(self._batch.end(), dtype=torch.float32, device=self.device) for _ in range(2))
        self._batch.on(self.device)
        self.frames = 0

    def layouts(self):
        """[(origin [3] float64, delta, dims)] of the volumes, for comparison with a caller's layouts."""
        return [(np.array(r.origin[:], np.float64), float(r.delta), tuple(int(d) for d in r.dims[:])) for r in self.rec]

    def integrate(self, depth: torch.Tensor, views, view_range, weights=None) -> "TsdfVolumes":
        """One more frame: depth [V,H,W], views [V,16] and view_range [M,2] as tsdf_integrate takes them.  The first call starts
        from (0, 0), every later one merges."""
        tsdf_integrate(self._batch, views, view_range, depth, self.trunc, self.near, weights, self.wmax, self.tsdf, self.weight, merge=self.frames > 0)
        self.frames += 1
        return self

    def states(self, min_weight: float = 1.0) -> torch.Tensor:
        """A new uint8 tensor of state bytes at state_begin (tsdf_states)."""
        return tsdf_states(self.tsdf, self.weight, None, self._batch, min_weight)

    def signed(self, radius: int, unknown_occupied: bool = True, min_weight: float = 1.0, out: "torch.Tensor | None" = None, offsets=None,
               clear=None):
        """The signed float32 volumes: states, distance_transform and tsdf_blend -> out, as distance_transform returns it.
        offsets: the volumes' element offsets in `out` for this call (a pool's slots change from frame to frame); default: the
        layouts' own.  clear: fuse_views' optional step between the states and the transform."""
        radius, min_weight = _fusion_radius(radius), _tsdf_positive("min_weight", min_weight)
        batch = self._batch
        if offsets is not None:
            if len(offsets) != batch.M:
                raise _lib.OmgHipError(f"{batch.M} volumes need as many offsets")
            batch = _VolumeBatch([v[:4] + (int(o),) for v, o in zip(self.volumes, offsets)], like=batch)  # (new records, the same state_begin)
        return _tsdf_signed(self.tsdf, self.weight, None, batch, self.trunc, radius, unknown_occupied, min_weight, out, clear)


class Components:
    """What label_components returns: labels (int32 on the device, one per state element), counts [M] and comp_begin [M+1]
    (host int64), records [C,8] (host int32; the same rows on the device as d_records), and the launch's volumes (rec) and
    state_begin, which component_states takes again."""

    def __init__(self, labels, counts, comp_begin, records, d_records, rec, begin, select, connectivity):
        self.labels, self.counts, self.comp_begin, self.records, self.d_records = labels, counts, comp_begin, records, d_records
        self.rec, self.begin, self.select, self.connectivity = rec, begin, select, connectivity
        self._batch = self._d_comp = None  # label_components' batch and comp_begin on the device: they serve component_states too

    def of(self, m: int) -> np.ndarray:
        """The records of volume m, in rank order."""
        return self.records[int(self.comp_begin[m]): int(self.comp_begin[m + 1])]


def _segment_arguments(select, connectivity):
    from . import segmentation as _sg
    if select not in (1, 2, 3):
        raise _lib.OmgHipError(f"select must be 1, 2 or 3, got {select!r}")
    if connectivity not in _sg.CONNECTIVITIES:
        raise _lib.OmgHipError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    return int(select), int(connectivity)


def label_components(state: torch.Tensor, state_begin, volumes, select: int = 1, connectivity: int = 6) -> Components:
    """The connected components of the foreground nodes of M volumes' states (carve_views' array and offsets), on the device
    (omgx_label_components, omgx_component_records; segmentation.label_components / component_records are the specification: the
    same integers) -> Components.  select bit 0: SURFACE nodes, bit 1: nodes that are neither FREE nor SURFACE; connectivity 6,
    18 or 26.  The same launches whatever the states hold; ONE download of the counts and one of the records.  The host
    arguments are checked first, then the tensor."""
    select, connectivity = _segment_arguments(select, connectivity)
    batch = _VolumeBatch.of(volumes, state_begin)
    _need(state, torch.uint8, "state")
    dev, vp, l, M, rec, begin = state.device, C.c_void_p, _lib.lib(), batch.M, batch.rec, batch.begin
    elems = int(state.numel())
    nbytes = int(l.omgx_label_workspace_bytes(*batch.host_args()))
    check(min(nbytes, 0), "omgx_label_workspace_bytes")
    with torch.cuda.device(dev):
        labels = torch.full((elems,), -1, dtype=torch.int32, device=dev) if M == 0 else torch.empty(elems, dtype=torch.int32, device=dev)
        if M == 0:
            return Components(labels, np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros((0, 8), np.int32),
                              torch.empty((0, 8), dtype=torch.int32, device=dev), rec, begin, select, connectivity)
        ws = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(M, dtype=torch.int32, device=dev)
        check(l.omgx_label_components(_ptr(state), elems, *batch.on(dev).begin_args(), *batch.volume_args(), select, connectivity, _ptr(ws), _ptr(labels),
                                      _ptr(counts), _stream()), "omgx_label_components")
        h_counts = counts.cpu().numpy().astype(np.int64)
        comp_begin = np.concatenate([[0], np.cumsum(h_counts)]).astype(np.int64)
        total = int(comp_begin[-1])
        d_records = torch.empty((total, 8), dtype=torch.int32, device=dev)
        d_comp = _upload(comp_begin, dev)
        check(l.omgx_component_records(_ptr(labels), elems, *batch.begin_args(), *batch.volume_args(), _ptr(d_comp), vp(comp_begin.ctypes.data),
                                       _ptr(d_records) if total else None, total, _stream()), "omgx_component_records")
        records = d_records.cpu().numpy()
        batch.release(ws, d_comp)
    comps = Components(labels, h_counts, comp_begin, records, d_records, rec, begin, select, connectivity)
    comps._batch, comps._d_comp = batch, d_comp
    return comps


def _component_arguments(components, picks, out_volumes, out_begin):
    """The host side of a component_states launch, checked before anything touches the device -> (picks int32 [K,8], the
    _VolumeBatch of the outputs)."""
    from . import segmentation as _sg
    if not isinstance(components, Components):
        raise _lib.OmgHipError("components must be what label_components returned")
    try:
        h_picks = np.ascontiguousarray(_sg.check_picks(picks, len(components.rec), components.comp_begin))
    except ValueError as e:
        raise _lib.OmgHipError(str(e)) from None
    outs = _VolumeBatch.of(out_volumes, out_begin)
    if outs.M != len(h_picks):
        raise _lib.OmgHipError(f"{len(h_picks)} picks need as many output volumes, got {outs.M}")
    return h_picks, outs


def component_states(state: torch.Tensor, components: Components, picks, out_volumes, out_begin=None, out: "torch.Tensor | None" = None):
    """The states of K cropped output volumes in ONE launch (omgx_component_states; segmentation.component_states is the
    specification: the same bytes) -> (out_state uint8 on the device, out_begin [K] int64 numpy).  state: the array that
    label_components labelled; picks [K,8] host integers (source volume, i0, j0, k0, component as a row of components.records,
    mode 0 the target alone / 1 everything but the target, 0, 0); out_volumes: what surface_records takes, one per pick.
    out / out_begin: None -> a new buffer, the outputs back to back, UNKNOWN where none lies; or the caller's, written IN PLACE."""
    from . import fusion as _fu
    h_picks, outs = _component_arguments(components, picks, out_volumes, out_begin)
    _need(state, torch.uint8, "state")
    dev, vp, K, ob = state.device, C.c_void_p, len(h_picks), outs.begin
    if int(state.numel()) != int(components.labels.numel()) or components.labels.device != dev:
        raise _lib.OmgHipError("state must be the array that label_components labelled")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.full((max(outs.end(), 1),), _fu.UNKNOWN, dtype=torch.uint8, device=dev)
        _tensor(out, "out", torch.uint8, None, dev)
        if K == 0:
            return out, ob
        src, comp_begin = (components._batch or _VolumeBatch(components.rec, components.begin)).on(dev), components.comp_begin
        d_comp, d_picks = _upload(comp_begin, dev) if components._d_comp is None else components._d_comp, _upload(h_picks, dev)
        check(_lib.lib().omgx_component_states(_ptr(state), int(state.numel()), *src.begin_args(), *src.volume_args(), _ptr(components.labels),
                                               _ptr(d_comp), vp(comp_begin.ctypes.data), _ptr(components.d_records), int(components.d_records.shape[0]),
                                               _ptr(d_picks), vp(h_picks.ctypes.data), *outs.on(dev).volume_args(), *outs.begin_args(), _ptr(out),
                                               int(out.numel()), _stream()), "omgx_component_states")
        src.release(d_comp, d_picks), outs.release()
    return out, ob


def component_volumes(state: torch.Tensor, components: Components, picks, out_volumes, radius: int, unknown_occupied: bool = True,
                      out: "torch.Tensor | None" = None):
    """component_states, then distance_transform of the K cropped states: four launches -> out as distance_transform returns it
    (output k at the element offset of its layout: the SDF pool, for instance).  The radius and the picks are checked before
    the first launch."""
    radius = _fusion_radius(radius)
    _, outs = _component_arguments(components, picks, out_volumes, None)  # (one batch of the outputs for both stages)
    cropped, _ = component_states(state, components, picks, outs)
    return distance_transform(cropped, None, outs, radius, unknown_occupied, out)


class PlaneFit:
    """What fit_planes returns.  On the device: planes [V,4] float64 (the final planes, four zeros without one), hypotheses
    [V,K,4], counts [V,K] int32 (-1: void), best [V] int32.  On the host (numpy): h_planes [V,4], h_best [V], ransac_counts [V]
    (the best hypothesis' count, 0 without), inliers [V] int32 (at the final plane), status [V] (planes.NO_PLANE, RANSAC_ONLY,
    REFINED), anchors [V,3]."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _plane_images(intrinsics, depth, skip, tol):
    """The host side of a launch over depth images, checked before anything touches the device -> (intrinsics float64 [V,4],
    V, H, W, tol).  depth and skip are only asked for their shape, type and place."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
        raise _lib.OmgHipError("depth must be a tensor [V,H,W]")
    V, H, W = (int(d) for d in depth.shape)
    k = np.asarray(intrinsics, np.float64)
    k = np.ascontiguousarray(np.broadcast_to(k, (V, 4)) if k.ndim == 1 and k.size == 4 else k.reshape(-1, 4))
    if len(k) != V or not np.isfinite(k).all() or (k[:, :2] == 0).any():
        raise _lib.OmgHipError(f"intrinsics must be [{V},4] (fx, fy, cx, cy), finite, the focal lengths not zero")
    if V and (H < 1 or W < 1):
        raise _lib.OmgHipError("the images are empty")
    tol = float(tol)
    _nonneg_finite(tol=tol)
    if skip is not None and (not isinstance(skip, torch.Tensor) or skip.dtype not in (torch.bool, torch.uint8) or skip.shape != depth.shape
                             or skip.device != depth.device):
        raise _lib.OmgHipError("skip must be a bool tensor of depth's shape, on its device")
    return k, V, H, W, tol


def _plane_skip(skip):
    return None if skip is None else (skip.contiguous().view(torch.uint8) if skip.dtype == torch.bool else skip.contiguous())


def _plane_rows(planes, V, dev, name="planes", cols=4):
    """planes [V,4] (or anchors [V,3]) as a contiguous float64 device tensor: a tensor is checked, a host array uploaded."""
    if isinstance(planes, torch.Tensor):
        _tensor(planes, name, torch.float64, (V, cols), dev)
        return planes
    h = np.ascontiguousarray(planes, np.float64)
    if h.shape != (V, cols):
        raise _lib.OmgHipError(f"{name} must be [{V},{cols}], got {h.shape}")
    return _upload(h, dev)


def plane_ransac(intrinsics, depth: torch.Tensor, triples, tol: float, min_nn: float = 1e-10, skip: "torch.Tensor | None" = None, up=None,
                 cos_min: float = -1.0):
    """One plane per pixel triple, its inlier count, and the best of every view, in three launches (omgx_plane_ransac;
    planes.ransac is the specification: the same bits) -> (planes [V,K,4] float64, counts [V,K] int32, best [V] int32,
    best_planes [V,4], anchors [V,3]) on depth's device.  intrinsics [4] or [V,4] and triples [V,K,3] (planes.draw_triples) are
    host arrays, up [3] or [V,3] too; depth [V,H,W]: a contiguous float64 device tensor; skip: a bool tensor of its shape.  The
    host arguments are checked first, then the tensors."""
    k, V, H, W, tol = _plane_images(intrinsics, depth, skip, tol)
    h_tri = np.asarray(triples)
    if h_tri.ndim != 3 or h_tri.shape[0] != V or h_tri.shape[2] != 3 or not np.issubdtype(h_tri.dtype, np.integer):
        raise _lib.OmgHipError(f"triples must be integers [{V},K,3]")
    K = int(h_tri.shape[1])
    if not 1 <= K <= _lib.PLANE_MAX_HYPOTHESES:
        raise _lib.OmgHipError(f"K must lie in [1, {_lib.PLANE_MAX_HYPOTHESES}], got {K}")
    if V and (h_tri.min() < 0 or h_tri.max() >= H * W):
        raise _lib.OmgHipError(f"a triple names a pixel outside [0, {H * W})")
    h_tri = np.ascontiguousarray(h_tri, np.int32)
    min_nn, cos_min = float(min_nn), float(cos_min)
    if not (np.isfinite(min_nn) and min_nn >= 0) or not -1.0 <= cos_min <= 1.0:
        raise _lib.OmgHipError("min_nn must be finite and not negative and cos_min lie in [-1, 1]")
    h_up = None
    if up is not None:
        h_up = np.asarray(up, np.float64)
        h_up = np.ascontiguousarray(np.broadcast_to(h_up, (V, 3)) if h_up.ndim == 1 and h_up.size == 3 else h_up.reshape(-1, 3))
        if len(h_up) != V or not np.isfinite(h_up).all():
            raise _lib.OmgHipError(f"up must be [{V},3] and finite")
    _need(depth, torch.float64, "depth")
    dev, vp = depth.device, C.c_void_p
    with torch.cuda.device(dev):
        planes = torch.empty((V, K, 4), dtype=torch.float64, device=dev)
        counts = torch.empty((V, K), dtype=torch.int32, device=dev)
        best = torch.empty(V, dtype=torch.int32, device=dev)
        best_planes, anchors = torch.empty((V, 4), dtype=torch.float64, device=dev), torch.empty((V, 3), dtype=torch.float64, device=dev)
        if V == 0:
            return planes, counts, best, best_planes, anchors
        d_k, d_tri, d_skip = _upload(k, dev), _upload(h_tri, dev), _plane_skip(skip)
        d_up = None if h_up is None else _upload(h_up, dev)
        check(_lib.lib().omgx_plane_ransac(_ptr(d_k), vp(k.ctypes.data), _ptr(depth), _ptr(d_skip), V, H, W, _ptr(d_tri), vp(h_tri.ctypes.data), K, tol,
                                           min_nn, _ptr(d_up), cos_min, _ptr(planes), _ptr(counts), _ptr(best), _ptr(best_planes), _ptr(anchors),
                                           _stream()), "omgx_plane_ransac")
        for t in (d_k, d_tri, d_skip, d_up):
            if t is not None:
                t.record_stream(torch.cuda.current_stream(dev))
    return planes, counts, best, best_planes, anchors


def plane_moments(intrinsics, depth: torch.Tensor, planes, anchors, tol: float, skip: "torch.Tensor | None" = None):
    """The inliers' count [V] int32 and sums [V,9] float64 about the anchors, in two launches (omgx_plane_moments;
    planes.moments is the specification: the same bits), on depth's device.  planes [V,4] and anchors [V,3]: float64 device
    tensors, or host arrays that are uploaded."""
    k, V, H, W, tol = _plane_images(intrinsics, depth, skip, tol)
    _need(depth, torch.float64, "depth")
    dev, vp, l = depth.device, C.c_void_p, _lib.lib()
    with torch.cuda.device(dev):
        d_planes, d_anchors = _plane_rows(planes, V, dev), _plane_rows(anchors, V, dev, "anchors", 3)
        count, sums = torch.empty(V, dtype=torch.int32, device=dev), torch.empty((V, 9), dtype=torch.float64, device=dev)
        if V == 0:
            return count, sums
        nbytes = int(l.omgx_plane_workspace_bytes(V, H, W))
        check(min(nbytes, 0), "omgx_plane_workspace_bytes")
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        d_k, d_skip = _upload(k, dev), _plane_skip(skip)
        check(l.omgx_plane_moments(_ptr(d_k), vp(k.ctypes.data), _ptr(depth), _ptr(d_skip), V, H, W, _ptr(d_planes), _ptr(d_anchors), tol, _ptr(ws),
                                   _ptr(count), _ptr(sums), _stream()), "omgx_plane_moments")
        for t in (ws, d_k, d_skip, d_planes, d_anchors):
            if t is not None:
                t.record_stream(torch.cuda.current_stream(dev))
    return count, sums


def fit_planes(intrinsics, depth: torch.Tensor, triples, tol: float, skip: "torch.Tensor | None" = None, up=None, cos_min: float = -1.0,
               min_nn: float = 1e-10, refine: int = 2) -> PlaneFit:
    """The dominant plane of every depth view (planes.fit_planes is the specification, and its host half, refine_plane, is the
    code that runs here too: the same planes bit for bit) -> PlaneFit.  plane_ransac, ONE small download of the best planes
    (with the counts), then per refinement round plane_moments at the current planes, a download of its 10 numbers per view and
    an upload of the refined planes; a last moment pass counts the inliers of the final planes.  Arguments: plane_ransac's."""
    from . import planes as _pl
    if int(refine) < 0:
        raise _lib.OmgHipError("refine must not be negative")
    hyp, counts, best, best_planes, anchors = plane_ransac(intrinsics, depth, triples, tol, min_nn, skip, up, cos_min)
    h_best, h_counts, h_anchors = best.cpu().numpy(), counts.cpu().numpy(), anchors.cpu().numpy()

    def moments_of(current):
        count, sums = plane_moments(intrinsics, depth, current, anchors, tol, skip)
        return count.cpu().numpy(), sums.cpu().numpy()

    final, inliers, status = _pl._fit_rounds(h_best, best_planes.cpu().numpy(), h_anchors, refine, moments_of)
    ransac_counts = np.array([h_counts[v, h_best[v]] if h_best[v] >= 0 else 0 for v in range(len(h_best))], np.int32)
    return PlaneFit(planes=_upload(final, depth.device), hypotheses=hyp, counts=counts, best=best, h_planes=final, h_best=h_best,
                    ransac_counts=ransac_counts, inliers=inliers, status=status, anchors=h_anchors)


def plane_mask(intrinsics, depth: torch.Tensor, planes, tol: float, skip: "torch.Tensor | None" = None) -> torch.Tensor:
    """The pixels on or behind the planes [V,4] (a device tensor, PlaneFit.planes, or a host array) in ONE launch
    (omgx_plane_mask; planes.plane_mask is the specification) -> a bool tensor of depth's shape on its device, directly usable
    as the free_mask of segment_obstacles, or as the skip of another fit."""
    k, V, H, W, tol = _plane_images(intrinsics, depth, skip, tol)
    _need(depth, torch.float64, "depth")
    dev, vp = depth.device, C.c_void_p
    with torch.cuda.device(dev):
        d_planes = _plane_rows(planes, V, dev)
        mask = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
        if V:
            d_k, d_skip = _upload(k, dev), _plane_skip(skip)
            check(_lib.lib().omgx_plane_mask(_ptr(d_k), vp(k.ctypes.data), _ptr(depth), _ptr(d_skip), V, H, W, _ptr(d_planes), tol, _ptr(mask), _stream()),
                  "omgx_plane_mask")
            for t in (d_k, d_skip, d_planes):
                if t is not None:
                    t.record_stream(torch.cuda.current_stream(dev))
    return mask.view(torch.bool)


def _plane_volume_arguments(volumes, planes):
    """The host side of plane_volumes, checked before anything touches the device -> (the _VolumeBatch, planes [M,4])."""
    batch = _VolumeBatch.of(volumes)
    h_planes = np.ascontiguousarray(planes, np.float64).reshape(-1, 4)
    if len(h_planes) != batch.M or not np.isfinite(h_planes).all():
        raise _lib.OmgHipError(f"{batch.M} volumes need as many planes [4], all finite")
    return batch, h_planes


def plane_volumes(volumes, planes, out: "torch.Tensor | None" = None, device="cuda:0") -> torch.Tensor:
    """The half-space volumes of M planes in ONE launch (omgx_plane_volumes; planes.halfspace_volume is the specification: the
    same bits): float32(n.p + off) at every node, positive on the camera's side of the plane.  volumes: what surface_records
    takes, the fifth field the element offset in `out` (without it: back to back); planes [M,4] on the host, in the grids'
    frames.  out: a contiguous float32 device tensor (the SDF pool) written IN PLACE, or None -> a new buffer on `device`."""
    batch, h_planes = _plane_volume_arguments(volumes, planes)
    if out is None:
        out = torch.zeros(batch.pool_end(), dtype=torch.float32, device=device)
    _need(out, torch.float32, "out")
    dev = out.device
    if batch.M == 0:
        return out
    with torch.cuda.device(dev):
        d_planes = _upload(h_planes, dev)
        check(_lib.lib().omgx_plane_volumes(*batch.on(dev).volume_args(), _ptr(d_planes), C.c_void_p(h_planes.ctypes.data), _ptr(out), int(out.numel()),
                                            _stream()), "omgx_plane_volumes")
        batch.release(d_planes)
    return out


class RayBatch:
    """Host side of a ragged ray batch over M meshes, shared by mesh_raycast_batch and grasp_poses: the meshes cleaned and pooled
    (vertex pool [V,3] float64, face pool [F,3] int32, omgx_mesh records), every mesh's rows of the ray arrays, and the work list
    (omgx_ray_work: one record per workgroup) on the host and on the device.

    meshes: a list of (verts [V,3], faces [F,3]) on the host; ray_counts: rays per mesh (0 is legal); ray_begins: the first row of
    each mesh's rays (default: back to back); num_rays: rows of the ray arrays (default: the end of the last range); chunks:
    workgroups that share the faces of one ray group (0: omgx_mesh_raycast_chunks decides from the compute units); layout: per
    mesh (origin [3], delta, sample, dims, element offset in the pool) of its volume, needed by grasp_poses only."""

    def __init__(self, meshes, ray_counts, ray_begins=None, num_rays=None, chunks: int = 0, device="cuda:0", layout=None):
        mp = MeshPool(meshes, drop_zero_area=False)  # dropping them here would renumber the faces the results name
        M = len(meshes)
        if len(ray_counts) != M or (ray_begins is not None and len(ray_begins) != M) or (layout is not None and len(layout) != M):
            raise _lib.OmgHipError(f"ray_counts, ray_begins and layout must have one entry per mesh ({M})")
        counts = [int(c) for c in ray_counts]
        if min(counts) < 0:
            raise _lib.OmgHipError("a ray count is negative")
        begins = [int(b) for b in ray_begins] if ray_begins is not None else [int(x) for x in np.concatenate([[0], np.cumsum(counts)[:-1]])]
        spans = sorted((b, c) for b, c in zip(begins, counts) if c > 0)
        end = max([b + c for b, c in spans], default=0)
        self.num_rays = end if num_rays is None else int(num_rays)
        if any(b < 0 for b in begins) or end > self.num_rays or any(spans[i][0] + spans[i][1] > spans[i + 1][0] for i in range(len(spans) - 1)):
            raise _lib.OmgHipError(f"the ray ranges (begin, count) {spans} overlap or leave the {self.num_rays} rows")
        if not 0 <= int(chunks) <= _lib.RAYCAST_MAX_CHUNKS:
            raise _lib.OmgHipError(f"chunks must lie in [0, {_lib.RAYCAST_MAX_CHUNKS}], got {chunks}")
        self.device = torch.device(device)
        self.num_meshes, self.ray_begin, self.ray_count, self.has_layout = M, begins, counts, layout is not None
        for m in range(M):
            mp.set_volume(m, *(((0.0, 0.0, 0.0), 1.0, "centre", (1, 1, 1), 0) if layout is None else layout[m]))
        self.rec, self.num_faces = mp.rec, len(mp.faces)
        groups = sum(-(-c // _lib.RAYCAST_RAYS_PER_WORKGROUP) for c in counts)
        if int(chunks) == 0 and groups > 0:
            with torch.cuda.device(self.device):
                self.chunks = int(_lib.lib().omgx_mesh_raycast_chunks(groups, max(r.face_count for r in self.rec), 0))
            check(min(self.chunks, 0), "omgx_mesh_raycast_chunks")
        else:
            self.chunks = max(int(chunks), 1)
        tile = int(_lib.lib().omgx_mesh_sdf_tile())
        work = []
        for m in range(M):
            nf = int(self.rec[m].face_count)
            tiles = -(-nf // tile)
            cut = [min(nf, tile * ((c * tiles) // self.chunks)) for c in range(self.chunks)] + [nf]
            for r0 in range(0, counts[m], _lib.RAYCAST_RAYS_PER_WORKGROUP):
                for c in range(self.chunks):
                    work.append((m, begins[m] + r0, min(_lib.RAYCAST_RAYS_PER_WORKGROUP, counts[m] - r0), cut[c], cut[c + 1] - cut[c], c))
        self.num_work = len(work)
        self.h_work = np.ascontiguousarray(np.array(work, np.int32).reshape(-1, 6))
        self.h_ray_begin, self.h_ray_count = np.array(begins, np.int32), np.array(counts, np.int32)
        self.verts, self.faces, self.d_rec = mp.upload(self.device)
        self.d_work = torch.from_numpy(self.h_work if self.num_work else np.zeros((1, 6), np.int32)).to(self.device)

    def _args(self):
        """(meshes, h_meshes, M, h_ray_begin, h_ray_count, work, h_work, num_work, chunks) as the entry points take them."""
        vp = C.c_void_p
        return (_ptr(self.d_rec), C.cast(self.rec, vp), self.num_meshes, vp(self.h_ray_begin.ctypes.data), vp(self.h_ray_count.ctypes.data),
                _ptr(self.d_work), vp(self.h_work.ctypes.data), self.num_work, self.chunks)

    def _rays(self, t, name, cols=3, dtype=torch.float64):
        return _tensor(t, name, dtype, (self.num_rays, cols) if cols else (self.num_rays,), self.device)


def mesh_raycast_batch(batch: RayBatch, origins: torch.Tensor, dirs: torch.Tensor, t_min: float = 1e-6, tol: float = 1e-9, out=None):
    """The nearest hit of every ray of a ragged batch with its own mesh, in ONE launch (omgx_mesh_raycast; grasps.mesh_raycast is
    the specification: the same float64 t bit for bit, the same face).  origins, dirs: [num_rays,3] float64 device tensors, mesh
    m's rays in rows [ray_begin[m], ray_begin[m] + ray_count[m]).  out: None or (t [num_rays] float64, face [num_rays] int32)
    written IN PLACE on those rows only.  -> (t, face); face is local to the mesh, (+inf, -1) is a miss; rows outside every
    range are left as they were (zeros in a fresh output)."""
    _nonneg_finite(t_min=t_min, tol=tol)
    batch._rays(origins, "origins"), batch._rays(dirs, "dirs")
    if out is None:
        out = (torch.zeros(batch.num_rays, dtype=torch.float64, device=batch.device), torch.zeros(batch.num_rays, dtype=torch.int32, device=batch.device))
    t, face = batch._rays(out[0], "out[0]", 0), batch._rays(out[1], "out[1]", 0, torch.int32)
    l = _lib.lib()
    ws = _workspace(int(l.omgx_mesh_raycast_workspace_bytes(batch.num_rays, batch.chunks)), batch.device) if batch.chunks > 1 else None
    a = batch._args()
    with torch.cuda.device(batch.device):
        check(l.omgx_mesh_raycast(_ptr(batch.verts), _ptr(batch.faces), *a, _ptr(origins), _ptr(dirs), batch.num_rays, float(t_min), float(tol),
                                  _ptr(t), _ptr(face), _ptr(ws), _stream()), "omgx_mesh_raycast")
    return t, face


def mesh_raycast(verts, faces, origins, dirs, t_min: float = 1e-6, tol: float = 1e-9, chunks: int = 0, device="cuda:0"):
    """Rays against one mesh on the device -> (t [N] float64, face [N] int32) device tensors; grasps.mesh_raycast with the same
    arguments is the specification.  origins, dirs: [N,3] on the host or float64 device tensors."""
    dev = torch.device(device)
    up = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)
    origins, dirs = up(origins), up(dirs)
    if origins.dim() != 2 or origins.shape[1:] != (3,) or origins.shape != dirs.shape:
        raise _lib.OmgHipError(f"origins and dirs must both be [N,3], got {tuple(origins.shape)} and {tuple(dirs.shape)}")
    return mesh_raycast_batch(RayBatch([(verts, faces)], [origins.shape[0]], chunks=chunks, device=dev), origins, dirs, t_min, tol)


def grasp_poses(batch: RayBatch, p1, n1, dirs, t, face2, normals, cs, probe, pool, max_width=0.08, min_width=0.005,
                cos_cone=float(np.cos(np.deg2rad(15.0))), pad_depth=0.088, clearance=0.0, out=None):
    """Hand poses of the contact pairs of a ragged batch in ONE launch (omgx_grasp_poses; grasps.grasp_poses is the specification:
    the same poses bit for bit, the same flags) -> (poses [num_rays,A,4,4] float64, valid [num_rays,A] uint8).
    batch: a RayBatch built with `layout` (where each mesh's volume lies in `pool`); p1, n1, dirs [num_rays,3], t [num_rays]
    float64, face2 [num_rays] int32: device tensors (mesh_raycast_batch's inputs and outputs); normals [F,3] float64 device tensor:
    unit face normals in the batch's face order; cs [A,2] (grasps.approach_angles) and probe [Q,3] on the host or the device;
    pool: contiguous float32 device tensor (the SDF pool or mesh_sdf_batch's buffer).  Rows outside every ray range are left as
    they were."""
    if not batch.has_layout:
        raise _lib.OmgHipError("grasp_poses needs a RayBatch with the layout of the volumes")
    dev = batch.device
    up = lambda x: x if isinstance(x, torch.Tensor) else _upload(np.asarray(x, np.float64), dev)
    cs, probe = _tensor(up(cs), "cs", torch.float64, (None, 2), dev), _tensor(up(probe), "probe", torch.float64, (None, 3), dev)
    _tensor(normals, "normals", torch.float64, (batch.num_faces, 3), dev)  # one per face of the batch
    if not 1 <= cs.shape[0] <= 65535:
        raise _lib.OmgHipError(f"cs must be [A,2] with 1 <= A <= 65535, got {tuple(cs.shape)}")
    _need(pool, torch.float32, "pool")
    for m in range(batch.num_meshes):
        r = batch.rec[m]
        if int(r.out_offset) + int(r.dims[0]) * int(r.dims[1]) * int(r.dims[2]) > pool.numel():
            raise _lib.OmgHipError(f"mesh {m}: its volume leaves the pool ({pool.numel()} elements)")
    if any(np.isnan(float(x)) for x in (max_width, min_width, cos_cone)) or not np.isfinite(float(pad_depth)) or not np.isfinite(float(clearance)):
        raise _lib.OmgHipError("max_width, min_width, cos_cone must not be NaN; pad_depth and clearance must be finite")
    batch._rays(p1, "p1"), batch._rays(n1, "n1"), batch._rays(dirs, "dirs"), batch._rays(t, "t", 0), batch._rays(face2, "face2", 0, torch.int32)
    A, N = int(cs.shape[0]), batch.num_rays
    if out is None:
        out = (torch.zeros((N, A, 4, 4), dtype=torch.float64, device=dev), torch.zeros((N, A), dtype=torch.uint8, device=dev))
    poses, valid = _tensor(out[0], "out[0]", torch.float64, (N, A, 4, 4), dev), _tensor(out[1], "out[1]", torch.uint8, (N, A), dev)
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_grasp_poses(*batch._args(), _ptr(p1), _ptr(n1), _ptr(dirs), _ptr(t), _ptr(face2), N, _ptr(normals), _ptr(cs), A,
                                          _ptr(probe), int(probe.shape[0]), _ptr(pool), pool.numel(), float(max_width), float(min_width),
                                          float(cos_cone), float(pad_depth), float(clearance), _ptr(poses), _ptr(valid), _stream()),
              "omgx_grasp_poses")
        _release(dev, cs, probe)
    return poses, valid


class CameraBatch:
    """Host side of a camera launch over S scenes, shared by render_depth and pixel_clouds: the meshes pooled (MeshPool: vertex
    pool [V,3] float64, face pool [F,3] int32, omgx_mesh records), the instance and camera records (omgx_instance, omgx_camera)
    on the host and on the device.

    meshes: the pool, a list of (verts [V,3], faces [F,3]) on the host; instances: camera.INSTANCE_DTYPE records
    (camera.instance_records); inst_begin [S+1]: scene s owns instances [inst_begin[s], inst_begin[s+1]); cameras [S,16]:
    fx, fy, cx, cy and the rows of world_from_cam (camera.camera_rows)."""

    def __init__(self, meshes, instances, inst_begin, cameras, device="cuda:0"):
        from . import camera as _cam
        mp = MeshPool(meshes, drop_zero_area=False)  # dropping them here would renumber the faces the face image names
        instances = np.ascontiguousarray(instances)
        if instances.dtype != _cam.INSTANCE_DTYPE or instances.ndim != 1:
            raise _lib.OmgHipError("instances must be a 1-d array of camera.INSTANCE_DTYPE records")
        for name in ("m", "centre", "q"):
            if not np.isfinite(instances[name]).all():
                raise _lib.OmgHipError(f"an instance's {name} is not finite")
        if len(instances) and (instances["label"].min() < 0 or instances["mesh"].min() < 0 or instances["mesh"].max() >= len(meshes)):
            raise _lib.OmgHipError(f"labels must be >= 0 and mesh indices inside the pool of {len(meshes)}")
        self.num_meshes = len(meshes)
        for m in range(self.num_meshes):
            mp.set_volume(m, (0.0, 0.0, 0.0), 1.0, "centre", (1, 1, 1), 0)  # no volume is read; the fields stay defined
        self.rec = mp.rec
        self._set_records(instances, inst_begin, cameras, None, torch.device(device))
        self.verts, self.faces, self.d_rec = mp.upload(self.device)

    def _set_records(self, instances, inst_begin, cameras, S, device):
        """What every kind of batch holds: the instance records as they are, the checked cameras [S,16] as omgx_camera records
        with their instance ranges, both on the host and on the device.  S: the scenes there must be, if known."""
        from . import camera as _cam
        try:
            cameras = _cam.check_camera_rows(cameras, S)
        except ValueError as e:
            raise _lib.OmgHipError(str(e)) from None
        S, I = len(cameras), len(instances)
        begin = np.asarray(inst_begin, np.int64).reshape(-1)
        if len(begin) != S + 1 or begin[0] < 0 or (np.diff(begin) < 0).any() or begin[-1] > I:
            raise _lib.OmgHipError(f"inst_begin must be [S+1] = [{S + 1}], ascending, inside the {I} instances")
        self.device, self.num_instances, self.num_scenes = device, I, S
        self.h_instances, self.h_inst_begin, self.h_cameras = instances, begin, _cam.camera_records(cameras, begin)
        self.d_instances, self.d_cameras = _record_bytes(self.h_instances, device), _record_bytes(self.h_cameras, device)
        return cameras

    def _records(self, host: bool = True):
        """(instances, [h_instances,] num_instances, cameras, [h_cameras,] num_scenes) as the entry points take them."""
        vp = C.c_void_p
        hi = (vp(self.h_instances.ctypes.data if self.num_instances else None),) if host else ()
        hc = (vp(self.h_cameras.ctypes.data if self.num_scenes else None),) if host else ()
        return (_ptr(self.d_instances), *hi, self.num_instances, _ptr(self.d_cameras), *hc, self.num_scenes)

    def _image(self, t, name, dtype, H=None, W=None):
        return _tensor(t, name, dtype, (self.num_scenes, H, W), self.device)


def _image_size(H, W):
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise _lib.OmgHipError(f"H and W must be >= 1, got {H} and {W}")
    return H, W


def render_depth(batch: CameraBatch, H: int, W: int, cull: bool = True, want_face: bool = True, t_min: float = 1e-6, tol: float = 1e-9,
                 out=None):
    """Depth, instance and face images of the batch's S scenes in ONE launch (omgx_render_depth; camera.render_depth is the
    specification: the same float64 t bit for bit, the same instance and face) -> (t [S,H,W] float64, inst [S,H,W] int32,
    face [S,H,W] int32 or None without want_face); background is (+inf, -1, -1).  out: None or (t, inst, face or None),
    contiguous device tensors written IN PLACE."""
    H, W = _image_size(H, W)
    _nonneg_finite(t_min=t_min, tol=tol)
    S, dev = batch.num_scenes, batch.device
    if out is None:
        out = (torch.empty((S, H, W), dtype=torch.float64, device=dev), torch.empty((S, H, W), dtype=torch.int32, device=dev),
               torch.empty((S, H, W), dtype=torch.int32, device=dev) if want_face else None)
    t, inst, face = out
    batch._image(t, "out[0]", torch.float64, H, W), batch._image(inst, "out[1]", torch.int32, H, W)
    if face is not None:
        batch._image(face, "out[2]", torch.int32, H, W)
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_render_depth(_ptr(batch.verts), _ptr(batch.faces), _ptr(batch.d_rec), C.cast(batch.rec, C.c_void_p),
                                           batch.num_meshes, *batch._records(), H, W, int(bool(cull)), float(t_min), float(tol), _ptr(t),
                                           _ptr(inst), _ptr(face), _stream()), "omgx_render_depth")
    return t, inst, face


def pixel_clouds(batch: CameraBatch, t: torch.Tensor, inst: torch.Tensor, cls: int, out: "torch.Tensor | None" = None):
    """The hit pixels of class `cls` (an instance label; < 0: every hit) of render_depth's images as world-frame points, in
    pixel order (omgx_pixel_count, omgx_pixel_gather; camera.pixel_clouds is the specification: the same float64 bit for bit)
    -> (points [N,3] float64 on the device, scene_begin [S+1] int64 numpy): scene s's cloud is points[scene_begin[s]:
    scene_begin[s+1]], a contiguous tensor as point_cloud_sdf takes it.  Count, ONE download of scene_begin, an exact
    allocation, gather.  out: a contiguous float64 [cap,3] device tensor written IN PLACE instead; rows >= cap are dropped."""
    batch._image(t, "t", torch.float64)
    H, W = int(t.shape[1]), int(t.shape[2])
    batch._image(inst, "inst", torch.int32, H, W)
    S, dev, l, cls = batch.num_scenes, batch.device, _lib.lib(), int(cls)
    if not -(1 << 31) <= cls < (1 << 31):
        raise _lib.OmgHipError(f"cls must fit int32, got {cls}")
    if out is not None:
        _tensor(out, "out", torch.float64, (None, 3), dev)
    ws = torch.empty(max(int(l.omgx_pixel_clouds_workspace_bytes(S, H, W)) // 4, 1), dtype=torch.int32, device=dev)
    begin = torch.empty(S + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(l.omgx_pixel_count(*batch._records(), H, W, _ptr(inst), cls, _ptr(ws), _ptr(begin), _stream()), "omgx_pixel_count")
        h_begin = begin.cpu().numpy().astype(np.int64)
        points = torch.empty((int(h_begin[-1]), 3), dtype=torch.float64, device=dev) if out is None else out
        check(l.omgx_pixel_gather(*batch._records(host=False), H, W, _ptr(t), _ptr(inst), cls, _ptr(ws), _ptr(points), int(points.shape[0]),
                                  _stream()), "omgx_pixel_gather")
    return points, h_begin


def register_clouds(scenes: DeviceScenes, pairs, poses0, points: torch.Tensor, ranges, stride: int = 1, trunc: float = 0.03,
                    lambda0: float = 2.0 ** -10, step_tol: float = 1e-6, max_passes: int = 30, out=None):
    """Refine the poses of M (scene, obj) instances against their clouds in ONE launch (omgx_register_clouds;
    registration.register_clouds is the specification: the same float64 bit for bit) -> (poses [M,12], stats [M,8]) float64 on
    the device.  pairs [M,2] (scene, obj) and ranges [M,2] (begin, end) rows of `points`: host integers; poses0 [M,12]: rows 0..2
    of world_from_obj, a float64 device tensor (or a host array, uploaded); points [N,3]: a contiguous float64 device tensor
    (pixel_clouds' points).  Ranges may be empty, overlap or be equal.  out: None or (poses, stats) written IN PLACE."""
    from . import registration as _reg
    dev = scenes.device
    # what does not depend on where a tensor lies comes first: the scalars, the index lists, the shapes, the ranges
    if int(stride) < 1 or not 0 <= int(max_passes) <= _reg.MAX_PASSES:
        raise _lib.OmgHipError(f"stride must be >= 1 and max_passes in [0, {_reg.MAX_PASSES}], got {stride} and {max_passes}")
    if not (np.isfinite(float(trunc)) and float(trunc) > 0 and np.isfinite(float(lambda0)) and float(lambda0) > 0):
        raise _lib.OmgHipError("trunc and lambda0 must be finite and positive")
    h_index = np.ascontiguousarray(scenes._rows(pairs), np.int32)
    M = len(h_index)
    h_ranges = np.asarray(ranges, np.int64).reshape(-1, 2)
    if len(h_ranges) != M:
        raise _lib.OmgHipError(f"ranges must be [{M},2], got {h_ranges.shape}")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise _lib.OmgHipError(f"points must be a tensor [N,3], got {tuple(getattr(points, 'shape', ()))}")
    N = int(points.shape[0])
    if M and ((h_ranges < 0).any() or (h_ranges > N).any() or (h_ranges[:, 1] < h_ranges[:, 0]).any()):
        raise _lib.OmgHipError(f"a range is outside [0, {N}] or ends before it begins")
    h_ranges = np.ascontiguousarray(h_ranges, np.int32)  # (inside [0, N], and N fits the int32 rows of pixel_clouds)
    if N > 0x7fffffff:
        raise _lib.OmgHipError(f"points has {N} rows: ranges are int32")
    if not isinstance(poses0, torch.Tensor):
        h_poses0 = np.ascontiguousarray(poses0, np.float64)
        if h_poses0.shape != (M, 12):
            raise _lib.OmgHipError(f"poses0 must be [{M},12], got {h_poses0.shape}")
        poses0 = torch.from_numpy(h_poses0).to(dev)
    if tuple(poses0.shape) != (M, 12):
        raise _lib.OmgHipError(f"poses0 must be [{M},12], got {tuple(poses0.shape)}")
    _tensor(points, "points", torch.float64, (None, 3), dev), _tensor(poses0, "poses0", torch.float64, (M, 12), dev)
    if out is None:
        out = (torch.empty((M, 12), dtype=torch.float64, device=dev), torch.empty((M, _reg.STATS), dtype=torch.float64, device=dev))
    poses, stats = _tensor(out[0], "out[0]", torch.float64, (M, 12), dev), _tensor(out[1], "out[1]", torch.float64, (M, _reg.STATS), dev)
    vp = C.c_void_p
    with torch.cuda.device(dev):
        d_index, d_ranges = torch.from_numpy(h_index).to(dev), torch.from_numpy(h_ranges).to(dev)
        check(_lib.lib().omgx_register_clouds(_ptr(scenes.objects), vp(scenes.host_objects.ctypes.data), len(scenes.host_objects), _ptr(scenes.pool),
                                              int(scenes.pool.numel()), _ptr(d_index), vp(h_index.ctypes.data if M else None), _ptr(poses0),
                                              _ptr(points) if N else None, N, _ptr(d_ranges), vp(h_ranges.ctypes.data if M else None), M,
                                              int(stride), float(trunc), float(lambda0), float(step_tol), int(max_passes), _ptr(poses), _ptr(stats),
                                              _stream()), "omgx_register_clouds")
    return poses, stats


class VolumeCameraBatch(CameraBatch):
    """What pixel_clouds needs of a CameraBatch for images rendered from a scene table's volumes (render_volumes): the host and
    device omgx_camera / omgx_instance records, ONE instance per object record of the table, in record order, so that a scene's
    instances are its objects and the instance image's k is the object index.  Only label, inst_begin and inst_count matter; no
    mesh is pooled.  cameras [S,16] (camera.camera_rows); labels: one per record (>= 0)."""

    def __init__(self, table: DeviceScenes, cameras, labels):
        from . import camera as _cam
        n = len(table.host_objects)
        labels = np.asarray(labels, np.int64).reshape(-1)
        if len(labels) != n or (n and labels.min() < 0):
            raise _lib.OmgHipError(f"labels must be {n} integers >= 0, one per object record")
        instances = np.zeros(n, _cam.INSTANCE_DTYPE)
        instances["label"] = labels
        self.num_meshes = 0
        self.cameras = self._set_records(instances, table.host_scene_begin, cameras, table.num_scenes, table.device)


def _volume_camera_arguments(table: DeviceScenes, cameras, H, W, visible, level, t_min, min_step, relax, max_steps):
    """render_volumes' checks that need no device: the specification's own (volume_camera.check_scalars / check_table on the
    table's host mirror), as OmgHipError -> (H, W, cameras [S,16], visible uint8 [n] or None)."""
    from . import volume_camera as _vc
    H, W = _image_size(H, W)
    try:
        _vc.check_scalars(level, t_min, min_step, relax, max_steps)
        _, _, cameras, vis = _vc.check_table(table.host_objects, table.host_scene_begin, int(table.pool.numel()), cameras, visible)
    except ValueError as e:
        raise _lib.OmgHipError(str(e)) from None
    # (flags for no records at all are no flags: an empty tensor has no address to pass beside the host's)
    return H, W, np.ascontiguousarray(cameras), None if visible is None or not len(vis) else np.ascontiguousarray(vis, np.uint8)


def render_volumes(table: DeviceScenes, cameras, H: int, W: int, visible=None, level: float = 0.0, t_min: float = 1e-6,
                   min_step: "float | None" = None, relax: float = 1.0, max_steps: "int | None" = None, want_normals: bool = False,
                   want_steps: bool = False, out=None):
    """Depth, object and normal images of the table's S scenes in ONE launch, straight from the records and the pool as they stand
    on the device (omgx_render_volumes; volume_camera.render_volumes is the specification: the same float64 t and normal bit for
    bit, the same inst and steps) -> (t [S,H,W] float64, inst [S,H,W] int32, normal [S,H,W,3] float64 or None, steps [S,H,W] int32
    or None); background is (+inf, -1, (0,0,0)).  A pose written on the device (set_object_poses, register_clouds' write-back) is
    seen without sync_host: the host mirror is used for the checks of dims and offsets only.  cameras [S,16]: camera.camera_rows;
    visible: one flag per object record of the table, or None (all); a scene_range view renders its scenes.  out: None or
    (t, inst, normal or None, steps or None), contiguous device tensors written IN PLACE.  Ordered on torch's current stream."""
    from . import volume_camera as _vc
    min_step = _vc.MIN_STEP if min_step is None else min_step
    max_steps = _vc.DEFAULT_STEPS if max_steps is None else max_steps
    H, W, h_cameras, h_visible = _volume_camera_arguments(table, cameras, H, W, visible, level, t_min, min_step, relax, max_steps)
    S, dev = table.num_scenes, table.device
    if out is None:
        out = (torch.empty((S, H, W), dtype=torch.float64, device=dev), torch.empty((S, H, W), dtype=torch.int32, device=dev),
               torch.empty((S, H, W, 3), dtype=torch.float64, device=dev) if want_normals else None,
               torch.empty((S, H, W), dtype=torch.int32, device=dev) if want_steps else None)
    t, inst, normal, steps = out
    for x, name, dtype, shape in ((t, "out[0]", torch.float64, (S, H, W)), (inst, "out[1]", torch.int32, (S, H, W)),
                                  (normal, "out[2]", torch.float64, (S, H, W, 3)), (steps, "out[3]", torch.int32, (S, H, W))):
        if x is not None or name in ("out[0]", "out[1]"):
            _tensor(x, name, dtype, shape, dev)
    vp = C.c_void_p
    h_begin = np.ascontiguousarray(table.host_scene_begin, np.int32)
    with torch.cuda.device(dev):
        d_cameras, d_visible = _upload(h_cameras, dev), None if h_visible is None else _upload(h_visible, dev)
        n = len(table.host_objects)
        check(_lib.lib().omgx_render_volumes(_ptr(table.objects) if n else None, vp(table.host_objects.ctypes.data) if n else None, n,
                                             _ptr(table.scene_begin), vp(h_begin.ctypes.data), S, _ptr(table.pool) if table.pool.numel() else None,
                                             int(table.pool.numel()), _ptr(d_cameras) if S else None, vp(h_cameras.ctypes.data) if S else None,
                                             _ptr(d_visible), None if h_visible is None else vp(h_visible.ctypes.data), H, W, float(level),
                                             float(t_min), float(min_step), float(relax), int(max_steps), _ptr(t), _ptr(inst), _ptr(normal),
                                             _ptr(steps), _stream()), "omgx_render_volumes")
        _release(dev, d_cameras, d_visible)
    return t, inst, normal, steps


class RobotSpheres:
    """The arm as N padded spheres on the host and on the device (robot_filter.py): local [N,4] float64, a centre in the frame of
    link[n] (0..9, the links of forward_kinematics with center_offset applied: the frame of PandaModel.collision_points) and a
    radius, finite and >= 0."""

    def __init__(self, local, link, device="cuda:0"):
        from . import robot_filter as _rf
        try:
            h_local, h_link = _rf._spheres(local, link)
        except ValueError as e:
            raise _lib.OmgHipError(str(e)) from None
        self.h_local, self.h_link = np.ascontiguousarray(h_local), np.ascontiguousarray(h_link, np.int32)
        self.N, self.device = len(self.h_link), torch.device(device)
        self.local, self.link = torch.from_numpy(self.h_local).to(self.device), torch.from_numpy(self.h_link).to(self.device)

    @classmethod
    def from_points(cls, collision_points, radius, device="cuda:0") -> "RobotSpheres":
        """One sphere per collision point: collision_points [10,P,3]; radius: a scalar or one value per link."""
        pts = np.asarray(collision_points, np.float64)
        if pts.ndim != 3 or pts.shape[0] != 10 or pts.shape[2] != 3:
            raise _lib.OmgHipError(f"collision_points must be [10,P,3], got {pts.shape}")
        try:
            r = np.broadcast_to(np.asarray(radius, np.float64).reshape(-1, 1), (10, pts.shape[1]))
        except ValueError:
            raise _lib.OmgHipError("radius must be a scalar or one value per link") from None
        return cls(np.concatenate([pts.reshape(-1, 3), r.reshape(-1, 1)], 1), np.repeat(np.arange(10), pts.shape[1]), device)

    def reach_table(self, model, finger_travel: "float | None" = None) -> np.ndarray:
        """clearance.reach_table for these spheres -> rho [10,9], kept as self.rho for DeviceScenes.plan_clearance.  finger_travel:
        default the larger of the fingers' joint limits."""
        from . import clearance as _cl
        if finger_travel is None:
            finger_travel = float(max(np.abs(model.joint_lower_limit[0, 7:]).max(), np.abs(model.joint_upper_limit[0, 7:]).max()))
        self.rho = _cl.reach_table(model, self.h_local, self.h_link, finger_travel)
        return self.rho


def _camera_records(cameras, dev):
    """(device records, host records) of a CameraBatch or of camera.CAMERA_DTYPE records on the host."""
    from . import camera as _cam
    if isinstance(cameras, CameraBatch):
        return cameras.d_cameras, cameras.h_cameras
    h = np.ascontiguousarray(cameras).reshape(-1)
    if h.dtype != _cam.CAMERA_DTYPE:
        raise _lib.OmgHipError("cameras must be camera.CAMERA_DTYPE records or a CameraBatch")
    return _record_bytes(h, dev), h


def render_spheres(spheres: RobotSpheres, link_poses: torch.Tensor, cameras, config_of_view, H: int, W: int, pad: float = 0.0,
                   t_min: float = 1e-6, cull: bool = True):
    """The arm's spheres as V cameras see them, in ONE launch (omgx_render_spheres; robot_filter.camera_spheres and render_spheres
    are the specification: the same bits) -> (t_near [V,H,W] float64, +inf where no sphere is seen; sphere [V,H,W] int32, -1
    there; cam_spheres [V,N,4] float64: centre in the camera's frame and radius + pad).  link_poses [C,10,4,4]: a float64 device
    tensor (forward_kinematics); cameras: V camera.CAMERA_DTYPE records on the host, or a CameraBatch (its own records, already on
    the device); config_of_view [V] host integers in 0..C-1.  The poses are downloaded once for the checks (one small copy that
    waits for the stream).  cull=False walks every sphere in every wave: the same bits."""
    from . import robot_filter as _rf
    H, W = _image_size(H, W)
    _tensor(link_poses, "link_poses", torch.float64, (None, 10, 4, 4), spheres.device)
    dev, N, Cn, vp = spheres.device, spheres.N, int(link_poses.shape[0]), C.c_void_p
    d_cam, h_cam = _camera_records(cameras, dev)
    V = len(h_cam)
    h_cfg = np.ascontiguousarray(np.asarray(config_of_view, np.int64).reshape(-1), np.int32)
    h_poses = np.ascontiguousarray(link_poses.cpu().numpy())
    _nonneg_finite(t_min=t_min)
    try:  # (the specification's own checks, as this module's error; nothing has touched the device's memory yet)
        _rf.camera_spheres(h_poses, np.zeros((0, 4)), np.zeros(0, np.int64), h_cam, h_cfg, pad)
    except ValueError as e:
        raise _lib.OmgHipError(str(e)) from None
    t_near = torch.empty((V, H, W), dtype=torch.float64, device=dev)
    which = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    cam_spheres = torch.empty((V, N, 4), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        d_cfg = _upload(h_cfg, dev)
        check(_lib.lib().omgx_render_spheres(_ptr(spheres.local) if N else None, vp(spheres.h_local.ctypes.data) if N else None,
                                             _ptr(spheres.link) if N else None, vp(spheres.h_link.ctypes.data) if N else None, N,
                                             _ptr(link_poses) if Cn else None, vp(h_poses.ctypes.data) if Cn else None, Cn,
                                             _ptr(d_cam) if V else None, vp(h_cam.ctypes.data) if V else None, _ptr(d_cfg) if V else None,
                                             vp(h_cfg.ctypes.data) if V else None, V, H, W, float(pad), float(t_min), int(bool(cull)),
                                             _ptr(cam_spheres) if V and N else None, _ptr(t_near) if V else None, _ptr(which) if V else None,
                                             _stream()), "omgx_render_spheres")
        _release(dev, d_cfg, d_cam)
    return t_near, which, cam_spheres


def clear_robot(state: torch.Tensor, state_begin, volumes, views, view_range, depth: torch.Tensor, near: float, t_near: torch.Tensor,
                cam_spheres: torch.Tensor, tol: float, cull: bool = True, h_cam_spheres=None) -> torch.Tensor:
    """The arm taken out of the states of M volumes, IN PLACE, in ONE launch (omgx_clear_robot; robot_filter.clear_states is the
    specification: the same bytes): a node inside a sphere of one of its volume's views becomes FREE, an UNKNOWN node between the
    camera and the arm too.  state, state_begin, volumes, views, view_range, depth and near as carve_views takes them (depth:
    the images BEFORE filter_depth); t_near [V,H,W] and cam_spheres [V,N,4]: render_spheres' for the same views.  h_cam_spheres:
    cam_spheres on the host, if the caller has them; otherwise they are downloaded once for the checks.  cull=False stages every
    sphere for every run of nodes: the same bytes."""
    batch, vb = _carve_arguments(volumes, views, view_range, depth, 0.0, near, state_begin)
    if not np.isfinite(float(tol)):
        raise _lib.OmgHipError("near and tol must be finite")
    _need(depth, torch.float64, "depth")
    dev, vp, V, H, W = depth.device, C.c_void_p, vb.V, vb.H, vb.W
    _tensor(t_near, "t_near", torch.float64, (V, H, W), dev), _tensor(cam_spheres, "cam_spheres", torch.float64, (V, None, 4), dev)
    N = int(cam_spheres.shape[1])
    h_sph = np.ascontiguousarray(cam_spheres.cpu().numpy() if h_cam_spheres is None else h_cam_spheres, np.float64)
    if h_sph.shape != (V, N, 4) or not np.isfinite(h_sph).all() or (h_sph[:, :, 3] < 0).any():
        raise _lib.OmgHipError("a sphere is not finite or has a negative radius")
    _tensor(state, "state", torch.uint8, None, dev)
    with torch.cuda.device(dev):
        check(_lib.lib().omgx_clear_robot(*batch.on(dev).volume_args(), *vb.on(dev).view_args(), *batch.begin_args(), _ptr(depth) if V else None,
                                          _ptr(t_near) if V else None, H, W, _ptr(cam_spheres) if V and N else None,
                                          vp(h_sph.ctypes.data) if V and N else None, N, float(near), float(tol), int(bool(cull)), _ptr(state),
                                          int(state.numel()), _stream()), "omgx_clear_robot")
        batch.release(), vb.release()
    return state


class RobotView:
    """What the arm looks like to V cameras (camera.Observation.robot_view): t_near [V,H,W] float64 and sphere [V,H,W] int32
    (render_spheres), cam_spheres [V,N,4] on the device and on the host, tol, and mask = explained(depth, t_near, tol): the
    pixels that show the arm, or what the arm hides.  As the `robot` of fuse_obstacles, integrate_obstacles and segment_obstacles
    its images belong to the call's views, one by one (take gathers them)."""

    def __init__(self, t_near, sphere, cam_spheres, tol: float, mask=None, h_cam_spheres=None):
        if not np.isfinite(float(tol)):
            raise _lib.OmgHipError("near and tol must be finite")
        self.t_near, self.sphere, self.cam_spheres, self.tol, self.mask = t_near, sphere, cam_spheres, float(tol), mask
        self.h_cam_spheres = np.ascontiguousarray(cam_spheres.cpu().numpy()) if h_cam_spheres is None else h_cam_spheres

    def explained(self, depth: torch.Tensor) -> torch.Tensor:
        """robot_filter.explained on the device, elementwise: t_near < inf and depth >= t_near - tol."""
        if depth.shape != self.t_near.shape or depth.device != self.t_near.device:
            raise _lib.OmgHipError(f"depth must be {list(self.t_near.shape)} on {self.t_near.device}, as the images of the arm")
        return (self.t_near < float("inf")) & (depth >= self.t_near - self.tol)

    def filter_depth(self, depth: torch.Tensor) -> torch.Tensor:
        """A new tensor: depth with the explained pixels set to 0.0, no information (robot_filter.filter_depth)."""
        return torch.where(self.explained(depth), torch.zeros_like(depth), depth).contiguous()

    def take(self, index) -> "RobotView":
        """The view whose image k is this one's image index[k]: a gather on the device."""
        index = np.asarray(index, np.int64).reshape(-1)
        at = torch.from_numpy(index.copy()).to(self.t_near.device)
        return RobotView(self.t_near[at].contiguous(), self.sphere[at].contiguous(), self.cam_spheres[at].contiguous(), self.tol,
                         None if self.mask is None else self.mask[at].contiguous(), np.ascontiguousarray(self.h_cam_spheres[index]))

    def filtered(self, obs):
        """A new camera.Observation whose t is 0.0 and whose inst is -1 on the mask."""
        from . import camera as _cam
        mask = self.explained(obs.t)
        return _cam.Observation(obs.batch, torch.where(mask, torch.zeros_like(obs.t), obs.t).contiguous(),
                                torch.where(mask, torch.full_like(obs.inst, -1), obs.inst).contiguous(), obs.face, obs.normals)


def _robot_step(robot: "RobotView | None", depth: torch.Tensor, views, view_range, near: float):
    """The self-filter's two halves for a call that turns depth views into states (fuse_obstacles, integrate_obstacles,
    segment_obstacles) -> (the depth to carve or integrate, clear).  Without a robot: the depth as it is and None, so that the
    call launches what it launched before.  With one: the explained pixels set to 0.0, and clear(state, state_begin, volumes),
    which runs clear_robot on the state bytes, with the images before the filter, before anything reads them."""
    if robot is None:
        return depth, None
    if not isinstance(robot, RobotView):
        raise _lib.OmgHipError("robot must be a RobotView (camera.Observation.robot_view)")
    _need(depth, torch.float64, "depth")
    filtered = robot.filter_depth(depth)
    # (what clear_robot would refuse is refused here, before the caller takes a slot of the pool)
    V, s, h = int(depth.shape[0]), robot.cam_spheres, robot.h_cam_spheres
    _need(robot.t_near, torch.float64, "robot.t_near"), _need(s, torch.float64, "robot.cam_spheres")
    if s.device != depth.device or s.dim() != 3 or s.shape[0] != V or s.shape[2] != 4 or tuple(h.shape) != tuple(s.shape):
        raise _lib.OmgHipError(f"robot.cam_spheres must be [{V},N,4] on {depth.device} and on the host, got {tuple(s.shape)} on {s.device}")
    if not np.isfinite(h).all() or (h[:, :, 3] < 0).any() or not np.isfinite(float(near)):
        raise _lib.OmgHipError("a sphere is not finite or has a negative radius, or near is not finite")

    def clear(state, state_begin, volumes):
        return clear_robot(state, state_begin, volumes, views, view_range, depth, near, robot.t_near, robot.cam_spheres, robot.tol,
                           h_cam_spheres=robot.h_cam_spheres)
    return filtered, clear


def _sensor_table(radius, table, sigma_px, dev):
    """(R, the spatial table on the host, the same on dev): the caller's, or a Gaussian of sigma_px pixels through numpy."""
    from . import sensor as _sn
    try:
        R, h_table = _sn.check_table(_sn.gaussian_table(radius, sigma_px) if table is None else table, radius)
    except ValueError as e:
        raise _lib.OmgHipError(str(e)) from None
    return R, h_table, _upload(h_table, dev)


def condition_depth(frames: torch.Tensor, scale: float, z_min: float, z_max: float, tau, min_support: int = 3, radius: int = 3, table=None,
                    sigma_px: float = 2.0, range_scale: float = 3.0, out=None):
    """A sensor's frames as clean depth images, V views in ONE launch (omgx_depth_condition; sensor.condition_depth is the
    specification: the same float64 bit for bit, the same flags) -> (depth [V,H,W] float64: 0.0 where there is no return or a flying
    pixel, the bilateral filter of the rest; flags [V,H,W] uint8: sensor.KEPT, NO_RETURN, FLYING).  frames [V,H,W]: a contiguous
    uint16 device tensor (z = raw * scale) or a float64 one (z as given: a rendered image, +inf as no return); tau = (t0, t1, t2):
    the noise scale (t0 + t1*z) + t2*z*z; table: the (2*radius+1)^2 spatial weights on the host, or None for a Gaussian of sigma_px
    pixels (sensor.gaussian_table).  out: None or (depth, flags) written IN PLACE; depth may not be `frames`."""
    from . import sensor as _sn
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint16, torch.float64):
        raise _lib.OmgHipError("frames must be a uint16 or float64 tensor [V,H,W]")
    _tensor(frames, "frames", frames.dtype, (None, None, None), frames.device)
    dev, (V, H, W) = frames.device, (int(d) for d in frames.shape)
    if V:
        _image_size(H, W)
    try:
        _sn.check_condition(np.zeros((0, 1, 1), np.uint16), scale, z_min, z_max, tau, min_support, 0, [1.0], range_scale)
        t0, t1, t2 = _sn.check_tau(tau)
    except ValueError as e:
        raise _lib.OmgHipError(str(e)) from None
    if out is None:
        out = (torch.empty((V, H, W), dtype=torch.float64, device=dev), torch.empty((V, H, W), dtype=torch.uint8, device=dev))
    depth, flags = _tensor(out[0], "out[0]", torch.float64, (V, H, W), dev), _tensor(out[1], "out[1]", torch.uint8, (V, H, W), dev)
    with torch.cuda.device(dev):
        R, h_table, d_table = _sensor_table(radius, table, sigma_px, dev)
        check(_lib.lib().omgx_depth_condition(_ptr(frames) if V else None, _sn.UINT16 if frames.dtype == torch.uint16 else _sn.FLOAT64, float(scale),
                                              V, H, W, float(z_min), float(z_max), t0, t1, t2, int(min_support), R, _ptr(d_table),
                                              C.c_void_p(h_table.ctypes.data), float(range_scale), _ptr(depth) if V else None,
                                              _ptr(flags) if V else None, _stream()), "omgx_depth_condition")
        _release(dev, d_table)
    return depth, flags


def depth_normals(depth: torch.Tensor, intrinsics, tau, cos_min: float = 0.0, flags: "torch.Tensor | None" = None, want_cosine: bool = False,
                  out=None):
    """Normal maps of V conditioned depth images in ONE launch (omgx_depth_normals; sensor.depth_normals is the specification: the
    same float64 bit for bit) -> (normals [V,H,W,3] float64: unit, in the camera's frame, facing the camera as render_volumes' are,
    zeros without one; depth_out [V,H,W]: depth with the grazing pixels (cos < cos_min) set to 0.0; flags [V,H,W] uint8: sensor.KEPT,
    KEPT | NO_NORMAL, GRAZING, or what `flags` says where nothing is there; cosine [V,H,W] or None).  depth: a contiguous float64
    device tensor, a pixel is there if > 0; intrinsics [V,4] on the host: fx, fy, cx, cy (Observation.intrinsics); tau as
    condition_depth takes it; flags: condition_depth's, or None.  out: None or (normals, depth_out, flags_out, cosine or None)
    written IN PLACE; flags_out may be `flags`, depth_out may not be `depth`."""
    from . import sensor as _sn
    _tensor(depth, "depth", torch.float64, (None, None, None), depth.device if isinstance(depth, torch.Tensor) else None)
    dev, (V, H, W) = depth.device, (int(d) for d in depth.shape)
    if V:
        _image_size(H, W)
    try:
        _, h_k, (t0, t1, t2), cos_min, _ = _sn.check_normals(np.zeros((V, 1, 1)), intrinsics, tau, cos_min, None)
    except ValueError as e:
        raise _lib.OmgHipError(str(e)) from None
    if flags is not None:
        _tensor(flags, "flags", torch.uint8, (V, H, W), dev)
    if out is None:
        out = (torch.empty((V, H, W, 3), dtype=torch.float64, device=dev), torch.empty((V, H, W), dtype=torch.float64, device=dev),
               torch.empty((V, H, W), dtype=torch.uint8, device=dev), torch.empty((V, H, W), dtype=torch.float64, device=dev) if want_cosine else None)
    normals, depth_out, flags_out, cosine = out
    _tensor(normals, "out[0]", torch.float64, (V, H, W, 3), dev), _tensor(depth_out, "out[1]", torch.float64, (V, H, W), dev)
    _tensor(flags_out, "out[2]", torch.uint8, (V, H, W), dev)
    if cosine is not None:
        _tensor(cosine, "out[3]", torch.float64, (V, H, W), dev)
    with torch.cuda.device(dev):
        d_k = _upload(h_k, dev)
        check(_lib.lib().omgx_depth_normals(_ptr(depth) if V else None, _ptr(flags) if V else None, _ptr(d_k) if V else None,
                                            C.c_void_p(h_k.ctypes.data) if V else None, V, H, W, t0, t1, t2, cos_min, _ptr(normals) if V else None,
                                            _ptr(depth_out) if V else None, _ptr(flags_out) if V else None, _ptr(cosine) if V else None,
                                            _stream()), "omgx_depth_normals")
        _release(dev, d_k)
    return normals, depth_out, flags_out, cosine


class FrameBatch(CameraBatch):
    """The batch of an observation made of sensor frames alone (camera.observe_frames): the cameras [S,16] (camera.camera_rows) as
    host and device records, and no instance, no mesh: every scene's instance range is empty."""
    frames_only = True

    def __init__(self, cameras, device="cuda:0"):
        from . import camera as _cam
        self.num_meshes = 0
        cameras = np.asarray(cameras, np.float64)
        self.cameras = self._set_records(np.zeros(0, _cam.INSTANCE_DTYPE), np.zeros(len(cameras) + 1, np.int64), cameras, None, torch.device(device))


def track_workspace_bytes(V: int, H: int, W: int, stride: int = 1) -> int:
    """The bytes track_cameras needs as its workspace for V views of H x W (omgx_track_workspace_bytes)."""
    nbytes = int(_lib.lib().omgx_track_workspace_bytes(int(V), int(H), int(W), int(stride)))
    if nbytes < 0:
        check(nbytes, "omgx_track_workspace_bytes")
    return nbytes


def track_cameras(live_depth: torch.Tensor, live_normals: "torch.Tensor | None", model_depth: torch.Tensor, model_normals: torch.Tensor, intrinsics,
                  poses0=None, stride: int = 1, dist_max: float = 0.05, cos_min: float = 0.7, lambda0: float = 2.0 ** -10, step_tol: float = 1e-6,
                  max_passes: int = 12, workspace: "torch.Tensor | None" = None, out=None):
    """Align V live depth frames to V model renderings by projective point-to-plane ICP (omgx_track_cameras; tracking.track_cameras
    is the specification: the same float64 bit for bit) -> (poses [V,12]: the rows [R t] of model_cam_from_live_cam, stats [V,8]:
    registration's columns) float64 on the device.  live_depth [V,H,W] (not > 0: no information) and live_normals [V,H,W,3] or None
    (depth_normals' outputs), model_depth [V,H,W] (+inf: background) and model_normals [V,H,W,3] (render_volumes' t and normal):
    contiguous float64 device tensors; intrinsics [V,4] on the host: fx, fy, cx, cy of both images; poses0 [V,12]: a float64
    device tensor (never downloaded), a host array (uploaded), or None: identity.  One init launch and max_passes + 1 times a pass
    and a step launch on torch's current stream, no host sync: a view that has stopped costs workgroups that return at once.
    workspace: None or a uint8 device tensor of at least track_workspace_bytes(V, H, W, stride); out: None or (poses, stats)
    written IN PLACE; out[0] may be poses0."""
    from . import tracking as _tr
    # what does not depend on where a tensor lies comes first: the scalars and the shapes
    try:
        _tr.check_scalars(stride, dist_max, cos_min, lambda0, step_tol, max_passes)
    except ValueError as e:
        raise _lib.OmgHipError(str(e)) from None
    if not isinstance(live_depth, torch.Tensor) or live_depth.dim() != 3:
        raise _lib.OmgHipError(f"live_depth must be a tensor [V,H,W], got {tuple(getattr(live_depth, 'shape', ()))}")
    V, H, W = (int(d) for d in live_depth.shape)
    if V:
        _image_size(H, W)
    images = [("live_depth", live_depth, (V, H, W)), ("model_depth", model_depth, (V, H, W)), ("model_normals", model_normals, (V, H, W, 3))]
    if live_normals is not None:
        images.append(("live_normals", live_normals, (V, H, W, 3)))
    for name, t, shape in images:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise _lib.OmgHipError(f"{name} must be a tensor {list(shape)}, got {list(getattr(t, 'shape', ()))}")
    h_k = np.ascontiguousarray(intrinsics, np.float64)
    if h_k.shape != (V, 4) or not np.isfinite(h_k).all() or (h_k[:, :2] == 0).any():
        raise _lib.OmgHipError(f"intrinsics must be [{V},4], finite, with no focal length of zero")
    dev = live_depth.device
    if poses0 is None or not isinstance(poses0, torch.Tensor):
        h_poses0 = np.ascontiguousarray(np.tile(_tr.IDENTITY, (V, 1)) if poses0 is None else poses0, np.float64)
        if h_poses0.shape != (V, 12):
            raise _lib.OmgHipError(f"poses0 must be [{V},12], got {h_poses0.shape}")
        poses0 = torch.from_numpy(h_poses0) if dev.type == "cpu" else torch.from_numpy(h_poses0).to(dev)
    if tuple(poses0.shape) != (V, 12):
        raise _lib.OmgHipError(f"poses0 must be [{V},12], got {tuple(poses0.shape)}")
    for name, t, shape in images:
        _tensor(t, name, torch.float64, shape, dev)
    _tensor(poses0, "poses0", torch.float64, (V, 12), dev)
    if out is None:
        out = (torch.empty((V, 12), dtype=torch.float64, device=dev), torch.empty((V, _tr.STATS), dtype=torch.float64, device=dev))
    poses, stats = _tensor(out[0], "out[0]", torch.float64, (V, 12), dev), _tensor(out[1], "out[1]", torch.float64, (V, _tr.STATS), dev)
    need = track_workspace_bytes(V, H, W, stride)
    if workspace is None:
        workspace = _workspace(need, dev)
    _tensor(workspace, "workspace", torch.uint8, (None,), dev)
    if workspace.numel() < need:
        raise _lib.OmgHipError(f"workspace has {workspace.numel()} bytes, {need} are needed")
    with torch.cuda.device(dev):
        d_k = _upload(h_k, dev)
        check(_lib.lib().omgx_track_cameras(_ptr(d_k) if V else None, C.c_void_p(h_k.ctypes.data) if V else None, _ptr(live_depth) if V else None,
                                            _ptr(live_normals) if V else None, _ptr(model_depth) if V else None, _ptr(model_normals) if V else None,
                                            V, H, W, int(stride), _ptr(poses0) if V else None, float(dist_max), float(cos_min), float(lambda0),
                                            float(step_tol), int(max_passes), _ptr(workspace) if V else None, int(workspace.numel()),
                                            _ptr(poses) if V else None, _ptr(stats) if V else None, _stream()), "omgx_track_cameras")
        _release(dev, d_k)
    return poses, stats


def dense_configs(traj: torch.Tensor, K: int) -> torch.Tensor:
    """clearance.dense_configs on the device (the same bits): traj [S,n,9] float64 -> q [S,(n-1)*K+1,9].  Sample i*K + k is
    a + (b - a) * (k / K), every operation rounded on its own (plain operators: no addcmul, no lerp); k = 0 and the last sample are
    the waypoints themselves."""
    if not isinstance(traj, torch.Tensor) or traj.dim() != 3 or traj.shape[2] != 9 or traj.dtype != torch.float64:
        raise _lib.OmgHipError("traj must be a float64 tensor [S,n,9]")
    S, n, K = int(traj.shape[0]), int(traj.shape[1]), int(K)
    if K < 1 or n < 1:
        raise _lib.OmgHipError(f"K and the number of waypoints must be >= 1, got {K} and {n}")
    q = torch.empty((S, (n - 1) * K + 1, 9), dtype=torch.float64, device=traj.device)
    a, b = traj[:, :-1, None, :], traj[:, 1:, None, :]
    # (a tensor divided by a tensor: dividing by a Python number may be done as a product with its reciprocal, which rounds otherwise)
    w = (torch.arange(K, dtype=torch.float64, device=traj.device) / torch.full((K,), float(K), dtype=torch.float64, device=traj.device)).reshape(1, 1, K, 1)
    seg = (b - a) * w
    seg = a + seg
    seg[:, :, 0, :] = traj[:, :-1]
    q[:, :-1] = seg.reshape(S, (n - 1) * K, 9)
    q[:, -1] = traj[:, -1]
    return q


def sphere_clearance(table: DeviceScenes, spheres: RobotSpheres, link_poses: torch.Tensor, scene_of_config, visible=None, pad=None,
                     beyond: float = 0.1, cull: bool = True, want_world: bool = False):
    """The clearance of B configurations of the arm from the volumes of their scenes, in ONE launch, straight from the records and
    the pool as they stand on the device (omgx_sphere_clearance; clearance.world_spheres and sphere_clearance are the
    specification: the same bits) -> (clear [B] float64, clear_sphere [B] int32, clear_object [B] int32, margin, margin_sphere,
    margin_object (None with pad=None), world [B,N,4] float64 or None).  link_poses [B,10,4,4]: a float64 device tensor
    (forward_kinematics), not downloaded; scene_of_config [B] host integers; visible: one flag per record of the table, or None
    (the records whose `disabled` is 0); pad [B,10]: a float64 device tensor or None; beyond: how far outside a grid its volume
    still speaks.  The host mirror is used for the checks of dims and offsets only.  cull=False walks every record in every wave:
    the same bits.  Ordered on torch's current stream."""
    from . import clearance as _cl
    dev, N, vp = table.device, spheres.N, C.c_void_p
    _tensor(link_poses, "link_poses", torch.float64, (None, 10, 4, 4), dev)
    B = int(link_poses.shape[0])
    h_cfg = np.ascontiguousarray(np.asarray(scene_of_config, np.int64).reshape(-1), np.int32)
    S, n = table.num_scenes, len(table.host_objects)
    h_begin = np.ascontiguousarray(table.host_scene_begin, np.int32)
    _nonneg_finite(beyond=beyond)
    if len(h_cfg) != B or (B and (h_cfg.min() < 0 or h_cfg.max() >= S)):
        raise _lib.OmgHipError(f"scene_of_config must be {B} scenes in [0, {S})")
    if spheres.device != dev:
        raise _lib.OmgHipError(f"the spheres are on {spheres.device}, the table on {dev}")
    if pad is not None:
        _tensor(pad, "pad", torch.float64, (B, 10), dev)
    try:  # (the specification's own checks of the table, as this module's error; nothing has touched the device's memory yet)
        _cl.check_table(table.host_objects, h_begin, int(table.pool.numel()), visible)
        h_visible = None if visible is None else np.ascontiguousarray(np.asarray(visible).reshape(-1) != 0, np.uint8)
    except ValueError as e:
        raise _lib.OmgHipError(str(e)) from None
    if h_visible is not None and not n:
        h_visible = None  # (flags for no records at all are no flags: an empty tensor has no address to pass beside the host's)
    f64 = lambda: torch.empty((B,), dtype=torch.float64, device=dev)
    i32 = lambda: torch.empty((B,), dtype=torch.int32, device=dev)
    clear, cs, co = f64(), i32(), i32()
    margin, ms, mo = (f64(), i32(), i32()) if pad is not None else (None, None, None)
    world = torch.empty((B, N, 4), dtype=torch.float64, device=dev) if want_world else None
    with torch.cuda.device(dev):
        d_cfg, d_visible = _upload(h_cfg, dev) if B else None, None if h_visible is None else _upload(h_visible, dev)
        check(_lib.lib().omgx_sphere_clearance(_ptr(table.objects) if n else None, vp(table.host_objects.ctypes.data) if n else None, n,
                                               _ptr(table.scene_begin), vp(h_begin.ctypes.data), S, _ptr(table.pool) if table.pool.numel() else None,
                                               int(table.pool.numel()), _ptr(d_visible), None if h_visible is None else vp(h_visible.ctypes.data),
                                               _ptr(d_cfg), vp(h_cfg.ctypes.data) if B else None, B, _ptr(link_poses) if B else None,
                                               _ptr(spheres.local) if N else None, vp(spheres.h_local.ctypes.data) if N else None,
                                               _ptr(spheres.link) if N else None, vp(spheres.h_link.ctypes.data) if N else None, N,
                                               _ptr(pad) if B else None, float(beyond), int(bool(cull)), _ptr(clear) if B else None,
                                               _ptr(cs) if B else None, _ptr(co) if B else None, _ptr(margin) if B else None, _ptr(ms) if B else None,
                                               _ptr(mo) if B else None, _ptr(world) if B and N else None, _stream()), "omgx_sphere_clearance")
        _release(dev, d_cfg, d_visible)
    return clear, cs, co, margin, ms, mo, world


def default_self_pairs(fingers_touch: bool = True) -> np.ndarray:
    """pairs [10,10] uint8 for self_clearance: the links whose spheres are held against one another.  A link is not held
    against itself, its neighbour in the chain (they share a joint), or, from link 6 on, anything rigidly fixed to it: the hand
    (7) on link 6 and the fingers (8, 9) on the hand.  fingers_touch: the two fingers may meet (they close on an object)."""
    pairs = np.zeros((10, 10), np.uint8)
    for i in range(10):
        for j in range(i + 1, 10):
            pairs[i, j] = pairs[j, i] = j - i >= 2 and i < 6
    pairs[8, 9] = pairs[9, 8] = 0 if fingers_touch else 1
    return pairs


def self_clearance(world: torch.Tensor, spheres: RobotSpheres, pairs, pad=None):
    """The smallest gap between two spheres of each of B configurations, in ONE launch (omgx_self_clearance;
    clearance.self_clearance is the specification: the same bits) -> (self_clear [B] float64, i [B] int32, j [B] int32).  world
    [B,N,4]: sphere_clearance's (want_world=True); pairs [10,10] host flags: which links are held against which; pad [B,10]: a
    float64 device tensor or None.  At most clearance.MAX_SELF spheres."""
    dev, N, vp = spheres.device, spheres.N, C.c_void_p
    _tensor(world, "world", torch.float64, (None, N, 4), dev)
    B = int(world.shape[0])
    h_pairs = np.ascontiguousarray(np.asarray(pairs) != 0, np.uint8)
    if h_pairs.shape != (10, 10):
        raise _lib.OmgHipError(f"pairs must be [10,10], got {h_pairs.shape}")
    if N > _lib.CONSTANTS["OMGX_CLEARANCE_MAX_SELF"]:
        raise _lib.OmgHipError(f"self_clearance takes at most {_lib.CONSTANTS['OMGX_CLEARANCE_MAX_SELF']} spheres, got {N}")
    if pad is not None:
        _tensor(pad, "pad", torch.float64, (B, 10), dev)
    out = torch.empty((B,), dtype=torch.float64, device=dev)
    wi, wj = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        d_pairs = _upload(h_pairs, dev)
        check(_lib.lib().omgx_self_clearance(_ptr(world) if B and N else None, B, _ptr(spheres.link) if N else None,
                                             vp(spheres.h_link.ctypes.data) if N else None, N, _ptr(d_pairs), _ptr(pad) if B else None,
                                             _ptr(out) if B else None, _ptr(wi) if B else None, _ptr(wj) if B else None, _stream()),
              "omgx_self_clearance")
        _release(dev, d_pairs)
    return out, wi, wj


class PlanClearance:
    """What DeviceScenes.plan_clearance returns (device tensors; clearance.py names every field).  Per sample [S,T], T = (n-1)*K+1:
    q [S,T,9]; clear, clear_sphere, clear_object; margin, margin_sphere, margin_object; self_clear, self_i, self_j (None without
    pairs).  Per segment [S,n-1]: half [S,n-1,10], segment_margin, certified.  Per plan [S]: min_clearance, collides, first_hit
    (a sample index or -1), plan_certified.  K: the samples per segment."""
    SAMPLE = ("clear", "clear_sphere", "clear_object", "margin", "margin_sphere", "margin_object", "self_clear", "self_i", "self_j")
    FILL = dict(q=0.0, clear=float("inf"), margin=float("inf"), self_clear=float("inf"), half=0.0, segment_margin=float("inf"), certified=False,
                min_clearance=float("inf"), collides=False, first_hit=-1, plan_certified=False)  # (every index: -1)

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def scattered(self, S: int, rows: torch.Tensor) -> "PlanClearance":
        """The same report over S plans with this one's plans at `rows`; the other rows say nothing: +inf, -1, False."""
        out = {}
        for name, x in self.__dict__.items():
            if not isinstance(x, torch.Tensor):
                out[name] = x
                continue
            full = torch.full((S,) + tuple(x.shape[1:]), self.FILL.get(name, -1), dtype=x.dtype, device=x.device)
            out[name] = full.index_copy_(0, rows, x)
        return PlanClearance(**out)
