"""Randomised differential test (GPU vs the numpy specification) of omgx_render_spheres / omgx_clear_robot, bit for bit:
ops.render_spheres and ops.clear_robot against robot_filter.camera_spheres, render_spheres and clear_states on random draws: 0..300
spheres (radius 0 included) on random links, 1..3 configurations of random link poses, 1..4 cameras of which one may stand inside a
sphere, images from 1 x 1 to 40 x 33 whose depths include NaN, inf, zero and negative values and values within tol of the arm, 1..3
volumes with dims 1..40 and both sample offsets, view ranges that alias or are empty, states between guard bytes, and either cull
on or off.  draw() needs neither torch nor a GPU; torch and ops are imported inside main.

    python tests/fuzz/fuzz_robot_filter.py [trials] [seed]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from omg_planner_amd import camera, fusion, robot_filter as rf

GUARD_STATE = 0xAB
SMOKE_SEED, SMOKE_TRIALS = 31, 12  # the short run of the test suite


def random_rigid(rng, reach):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    m = np.eye(4)
    m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    m[:3, 3] = rng.uniform(-reach, reach, 3)
    return m


def draw(rng):
    N = int(rng.choice([0, 1, 2, 5, 40, 255, 256, 257, 300]))
    Cn, V, M = int(rng.integers(1, 4)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
    H, W = (1, 1) if rng.random() < 0.1 else (int(rng.integers(1, 41)), int(rng.integers(1, 34)))
    local = np.concatenate([rng.uniform(-0.05, 0.05, (N, 3)), rng.uniform(0.0, 0.07, (N, 1)) * (rng.random((N, 1)) < 0.9)], 1)
    link = rng.integers(0, 10, N)
    poses = np.stack([np.stack([random_rigid(rng, 0.15) for _ in range(10)]) for _ in range(Cn)])
    cfg = rng.integers(0, Cn, V)
    rows, views = np.zeros((V, 16)), np.zeros((V, 16))
    for v in range(V):
        world_from_cam = random_rigid(rng, 0.0)
        if N and rng.random() < 0.3:  # on a sphere's centre: inside it unless its radius is 0
            n = int(rng.integers(N))
            world_from_cam[:3, 3] = (poses[cfg[v], link[n]] @ np.append(local[n, :3], 1.0))[:3]
        else:
            world_from_cam[:3, 3] = -world_from_cam[:3, 2] * rng.uniform(0.2, 0.8) + rng.normal(scale=0.03, size=3)
        f = float(rng.uniform(0.5, 2.0) * max(H, W))
        k = (f, f * rng.uniform(0.8, 1.25), (W - 1) / 2 + rng.normal(), (H - 1) / 2 + rng.normal())
        rows[v] = np.concatenate([k, world_from_cam[:3].ravel()])
        views[v] = fusion.view_rows(k, np.linalg.inv(world_from_cam))  # (the grid frame is the world frame)
    cams = camera.camera_records(rows)
    volumes, begin, at = [], [], int(rng.integers(0, 5))
    for _ in range(M):
        dims = tuple(int(d) for d in (rng.integers(1, 41, 3) if rng.random() < 0.5 else rng.integers(1, 9, 3)))
        delta = float(rng.uniform(0.004, 0.02))
        origin = -0.5 * delta * np.array(dims) + rng.normal(scale=0.03, size=3)
        volumes.append((origin, delta, "centre" if rng.random() < 0.5 else "node", dims))
        begin.append(at)
        at += int(np.prod(dims)) + int(rng.integers(0, 5))
    ranges = []
    for _ in range(M):
        first = int(rng.integers(0, V + 1))
        ranges.append((first, int(rng.integers(0, V - first + 1))))
    state = np.full(at, GUARD_STATE, np.uint8)
    for b, v in zip(begin, volumes):
        n = int(np.prod(v[3]))
        state[b: b + n] = rng.choice(np.array([0, 1, 2, 7], np.uint8), size=n, p=[0.2, 0.3, 0.45, 0.05])
    return dict(N=N, local=local, link=link, poses=poses, cfg=cfg, cams=cams, views=views, H=H, W=W, volumes=volumes, begin=np.array(begin, np.int64),
                ranges=ranges, state=state, pad=float(rng.uniform(0.0, 0.02)), t_min=float(rng.choice([0.0, 1e-6, 0.05])),
                near=float(rng.uniform(0.0, 0.3)), tol=float(rng.uniform(0.0, 0.03)), cull=bool(rng.integers(2)), depth_seed=int(rng.integers(1 << 30)))


def depth_images(c, t_near):
    """Depths around the arm's, with values that carry no information."""
    rng = np.random.default_rng(c["depth_seed"])
    depth = rng.uniform(0.1, 1.0, t_near.shape)
    close = np.isfinite(t_near) & (rng.random(t_near.shape) < 0.6)
    depth[close] = (t_near + rng.uniform(-0.05, 0.05, t_near.shape))[close]
    kind = rng.random(t_near.shape)
    for lo, hi, val in ((0.0, 0.04, np.nan), (0.04, 0.15, np.inf), (0.15, 0.18, 0.0), (0.18, 0.21, -0.5), (0.21, 0.23, -np.inf)):
        depth[(kind >= lo) & (kind < hi)] = val
    return depth


def specification(c):
    """-> (cam_spheres, t_near, sphere, depth, states)."""
    cs = rf.camera_spheres(c["poses"], c["local"], c["link"], c["cams"], c["cfg"], c["pad"])
    t_near, which = rf.render_spheres(cs, c["cams"], c["H"], c["W"], c["t_min"])
    depth = depth_images(c, t_near)
    want = rf.clear_states(c["state"], c["volumes"], c["views"], c["ranges"], depth, c["near"], t_near, cs, c["tol"], state_begin=c["begin"])
    return cs, t_near, which, depth, want


def check(c, torch, ops, dev):
    """-> (errors, pixels and nodes compared)."""
    cs, t_near, which, depth, want = specification(c)
    spheres = ops.RobotSpheres(c["local"], c["link"], dev)
    poses = torch.from_numpy(c["poses"]).to(dev)
    g_t, g_n, g_cs = ops.render_spheres(spheres, poses, c["cams"], c["cfg"], c["H"], c["W"], pad=c["pad"], t_min=c["t_min"], cull=c["cull"])
    torch.cuda.synchronize()
    state = torch.from_numpy(c["state"].copy()).to(dev)
    ops.clear_robot(state, c["begin"], c["volumes"], c["views"], c["ranges"], torch.from_numpy(depth).to(dev), c["near"], g_t, g_cs, c["tol"], cull=c["cull"])
    torch.cuda.synchronize()
    what = f"(N={c['N']}, V={len(c['cams'])}, image {c['H']} x {c['W']}, dims {[v[3] for v in c['volumes']]}, ranges {c['ranges']}, cull={c['cull']})"
    errs = []
    for name, got, ref in (("cam_spheres", g_cs, cs), ("t_near", g_t, t_near), ("sphere", g_n, which), ("states", state, want)):
        got = got.cpu().numpy()
        if got.shape != ref.shape or got.tobytes() != np.ascontiguousarray(ref).tobytes():
            errs.append(f"{name} differ {what}")
    return errs, t_near.size + sum(int(np.prod(v[3])) for v in c["volumes"])


def main(trials=None, seed=None):
    import torch
    from omg_planner_amd import ops
    trials = int(trials if trials is not None else (sys.argv[1] if len(sys.argv) > 1 else 30))
    seed = int(seed if seed is not None else (sys.argv[2] if len(sys.argv) > 2 else 0))
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda:0")
    bad, total, t0 = 0, 0, time.time()
    for k in range(trials):
        c = draw(rng)
        try:
            errs, n = check(c, torch, ops, dev)
        except Exception as e:  # noqa: BLE001
            # not a mismatch: the device may have faulted, so nothing more is started on it
            print(f"trial {k}: STOP exception {type(e).__name__}: {e}; {trials - k - 1} trials not run", flush=True)
            return 2
        total += n
        if errs:
            bad += 1
            print(f"trial {k}: FAIL " + "; ".join(errs), flush=True)
    print(f"{trials - bad}/{trials} trials agree; {total} pixels and nodes compared bit for bit; seed {seed}; {time.time() - t0:.0f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
