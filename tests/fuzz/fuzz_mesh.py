"""Randomised differential test (GPU vs the numpy specifications) of the mesh entry points, bit for bit:
  1. ops.mesh_sdf_batch      against scenes.mesh_sdf      (1..20 meshes in one launch, volumes at shuffled offsets of one buffer)
  2. ops.mesh_raycast_batch  against grasps.mesh_raycast  (ragged ray batches, every chunk split, t_min and tol off their defaults)
  3. ops.grasp_poses         against grasps.grasp_poses   (volumes in a pool at non-zero offsets, widths, pad depth and cone drawn)
  4. ops.render_depth / ops.pixel_clouds against camera.render_depth / camera.pixel_clouds (mirrored and scaled instances)
Every trial runs the four sections, each on a draw of its own.  A draw whose specification alone makes it useless (a node on the
surface, an open mesh with too many undecided signs, a render without hits or without background) is rejected, counted and drawn
again; a run whose rejected share exceeds MAX_REJECTED fails.  The draw_* generators need neither torch nor a GPU
(tests/test_fuzz_mesh_cpu.py runs them alone); torch and ops are imported inside main.

    python tests/fuzz/fuzz_mesh.py [trials] [seed]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from omg_planner_amd import camera as cam, grasps as gr, scenes as sc
from tests import camera_cases as CC, grasp_cases as GC, mesh_cases as MC

MAX_REJECTED = 0.05
SDF_BATCHES = (1, 2, 5, 20)
RAY_BATCHES = (1, 2, 4, 9)
RAY_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 300)
CHUNKS = (0, 1, 2, 3, 7, 16)
T_MINS = (0.0, 1e-6, 1e-3, 0.05)
TOLS = (0.0, 1e-9, 1e-3)
RAY_KINDS = ("mixed", "crack", "outward")
IMAGE_SIDES = (1, 2, 5, 9, 15, 16, 17, 24, 31, 32, 33, 40)
MAX_FACES, MAX_NODES, MAX_RAYS, MAX_SIDE = 1280, 3000, 300, 40


def draw_mesh(rng, max_level, closed=None):
    """The box or an icosphere of level 1..max_level with an anisotropic scale and a rotation about its centre, up to 1.5 m from
    the origin; closed, or cut to 1..F of its faces in permuted order -> (verts, faces, closed)."""
    level = int(rng.randint(0, max_level + 1))
    v, f = MC.box_mesh(MC.BOX_HALF) if level == 0 else MC.icosphere(level)
    c = v.mean(0)
    R = MC.pose(rng.uniform(-np.pi, np.pi, 3))[:3, :3]
    shift = rng.normal(size=3)
    shift *= rng.uniform(0.0, 1.5) / np.linalg.norm(shift)
    v = ((v - c) * rng.uniform(0.5, 2.0, 3)) @ R.T + c + shift
    closed = bool(rng.rand() < 0.5) if closed is None else closed
    if not closed:
        f = f[rng.permutation(len(f))[: int(rng.randint(1, len(f) + 1))]]
    return np.ascontiguousarray(v), np.ascontiguousarray(f, np.int32), closed


def _levels(M):
    """The largest icosphere level of a batch of M meshes, so that the faces of a batch (the specification's cost) stay bounded."""
    return 3 if M == 1 else 2 if M <= 2 else 1


def spec_sdf(v, f, delta, padding, sample, origin, dims):
    """scenes.mesh_sdf with the distances and winding numbers it computed on the way -> (SdfGrid, d, w)."""
    seen, inner = {}, sc.mesh_distance_winding

    def recording(*a):
        seen["dw"] = inner(*a)
        return seen["dw"]
    sc.mesh_distance_winding = recording
    try:
        grid = sc.mesh_sdf(v, f, delta, padding, sample, origin, dims)
    finally:
        sc.mesh_distance_winding = inner
    return (grid, *seen["dw"])


def _volume(rng, v, cells, explicit=True):
    """(delta, padding, sample, origin, dims, explicit) of a mesh's volume: mesh_grid_layout's with about `cells` cells along the
    longest side, or (with `explicit`, one in six each) a single node and a column along z."""
    ext = float((v.max(0) - v.min(0)).max())
    delta = ext / rng.uniform(cells - 0.5, cells + 0.5)
    padding, sample = int(rng.randint(0, 3)), ("centre", "node")[int(rng.randint(0, 2))]
    kind = rng.rand() if explicit else 1.0
    if kind < 1 / 6:
        return delta, 0, sample, v.mean(0) + rng.uniform(-1.0, 1.0, 3) * ext, (1, 1, 1), True
    if kind < 2 / 6:
        n = int(rng.randint(2, 301))
        return 2.0 * ext / n, 0, sample, v.mean(0) + rng.uniform(-0.3, 0.3, 3) * ext - (0.0, 0.0, ext), (1, 1, n), True
    origin, dims = sc.mesh_grid_layout(v, delta, padding)
    return delta, padding, sample, origin, tuple(int(x) for x in dims), False


def _layouts(vols):
    """(origins, dims) as ops.mesh_sdf_batch takes them: None, None when every volume of the batch has mesh_grid_layout's."""
    if not any(v[5] for v in vols):
        return None, None
    return [v[3] for v in vols], [v[4] for v in vols]


def _sdf_useless(closed, d, w):
    """The reason the specification alone gives to throw a volume away, or None."""
    gap = np.abs(np.abs(w) - 0.5)
    if d.min() <= 0.0:
        return "a node on the surface"
    if closed and gap.min() <= 0.4:
        return "a closed mesh with an unclear winding number"
    if not closed and (gap <= 1e-3).sum() > 0.005 * len(w):
        return "more than 0.5 % of the nodes undecided"
    return None


def draw_sdf(rng, tally):
    """Section 1: M meshes with a volume each, at shuffled offsets of one buffer.  A draw here is one mesh with its volume: a
    useless one is drawn again (at most 50 times) and the batch keeps its size."""
    M = int(SDF_BATCHES[rng.randint(0, len(SDF_BATCHES))])
    cells = {1: 9, 2: 7, 5: 5, 20: 3}[M]
    meshes, vols, specs = [], [], []
    for _ in range(M):
        for attempt in range(50):
            v, f, closed = draw_mesh(rng, _levels(M))
            vol = _volume(rng, v, cells)
            assert len(f) <= MAX_FACES and int(np.prod(vol[4])) <= MAX_NODES
            grid, d, w = spec_sdf(v, f, *vol[:5])
            if tally(_sdf_useless(closed, d, w)) is None:
                break
        else:
            raise RuntimeError("section sdf: 50 draws in a row rejected")
        meshes.append((v, f, closed)), vols.append(vol), specs.append((grid, d, w))
    sizes = [int(np.prod(vol[4])) for vol in vols]
    offsets, at = [0] * M, int(rng.randint(0, 40))
    for m in rng.permutation(M):
        offsets[m] = at
        at += sizes[m] + int(rng.randint(0, 50))
    return dict(M=M, meshes=meshes, vols=vols, specs=specs, offsets=offsets, total=at + int(rng.randint(0, 40)))


def _rays(rng, v, f, count, kind):
    seed = int(rng.randint(0, 1 << 30))
    if kind == "mixed":
        return GC.mixed_rays(v, f, count, seed)
    if kind == "outward":
        o, d = GC.outward_rays(v, f, count, seed)
        return np.ascontiguousarray(o.reshape(count, 3)), np.ascontiguousarray(d.reshape(count, 3))
    c = v.mean(0)                                                   # from the middle through vertices and points of edges
    _, d, _ = GC.sphere_crack_rays(v - c, f, limit=count)
    return np.ascontiguousarray(np.tile(c, (count, 1))), np.ascontiguousarray(d.reshape(count, 3))


def draw_raycast(rng, tally):
    """Section 2: M meshes with 0..300 rays each at scattered rows of the ray arrays (never rejected)."""
    M = int(RAY_BATCHES[rng.randint(0, len(RAY_BATCHES))])
    meshes = [draw_mesh(rng, _levels(M)) for _ in range(M)]
    counts = [int(RAY_COUNTS[rng.randint(0, len(RAY_COUNTS))]) for _ in range(M)]
    kinds = [RAY_KINDS[rng.randint(0, 3)] for _ in range(M)]
    rays = [_rays(rng, v, f, n, k) for (v, f, _), n, k in zip(meshes, counts, kinds)]
    begins, at = [0] * M, int(rng.randint(0, 9))
    for m in rng.permutation(M):
        begins[m] = at
        at += counts[m] + int(rng.randint(0, 9))
    assert max(counts) <= MAX_RAYS
    tally(None)
    return dict(M=M, meshes=meshes, counts=counts, kinds=kinds, rays=rays, begins=begins, num_rays=at + int(rng.randint(0, 9)),
                chunks=int(CHUNKS[rng.randint(0, len(CHUNKS))]), t_min=float(T_MINS[rng.randint(0, len(T_MINS))]),
                tol=float(TOLS[rng.randint(0, len(TOLS))]))


def draw_grasp(rng, tally):
    """Section 3: 1..3 meshes with a volume and 64..300 surface samples and ray directions each (the specification's own chain),
    the pose arguments drawn around their defaults (never rejected: the volumes come from the device)."""
    M = int(rng.randint(1, 4))
    cone = float(np.deg2rad(rng.choice([15.0, 5.0, 30.0])))
    meshes, vols, contacts = [], [], []
    for _ in range(M):
        v, f, closed = draw_mesh(rng, 2 if M == 1 else 1)
        v, f = gr.outward_mesh(v, f)
        vol = _volume(rng, v, 8, explicit=False)
        n = int(rng.randint(64, 301))
        p1, _, n1 = gr.surface_samples(v, f, n, rng)
        contacts.append((p1, n1, gr.ray_directions(n1, cone, rng)))
        meshes.append((v, f, closed)), vols.append(vol)
    tally(None)
    probe = gr.default_probe()
    q = int(rng.choice([1, 17, len(probe)]))
    sizes = [int(np.prod(vol[4])) for vol in vols]
    offsets, at = [0] * M, int(rng.randint(1, 40))
    for m in rng.permutation(M):
        offsets[m] = at
        at += sizes[m] + int(rng.randint(0, 50))
    return dict(M=M, meshes=meshes, vols=vols, contacts=contacts, offsets=offsets, total=at, cone=cone, A=int(rng.choice([1, 3, 8])),
                probe=np.ascontiguousarray(probe[np.sort(rng.permutation(len(probe))[:q])]), clearance=float(rng.choice([0.0, 0.004])),
                max_width=float(rng.choice([0.08, 0.05, 0.12])), min_width=float(rng.choice([0.005, 0.0, 0.02])),
                pad_depth=float(rng.choice([0.088, 0.05, 0.1])), chunks=int(CHUNKS[rng.randint(0, len(CHUNKS))]))


def draw_render(rng, tally):
    """Section 4: S scenes of H x W pixels with 0..8 instances of the box and icosphere(1) each at scaled and (one in four)
    mirrored poses with z in [-0.1, 0.9]; the first scene's first instance sits in front of the camera so that a render is seldom
    all background."""
    for attempt in range(50):
        case = _render_case(rng)
        hit = case["spec"][1] >= 0
        if tally("a render of one kind of pixel" if case["H"] * case["W"] > 1 and (hit.all() or not hit.any()) else None) is None:
            return case
    raise RuntimeError("section render: 50 draws in a row rejected")


def _render_case(rng):
    S = int(rng.choice([1, 2, 5]))
    H, W = (int(IMAGE_SIDES[rng.randint(0, len(IMAGE_SIDES))]) for _ in range(2))
    meshes = [CC.BOX, MC.icosphere(1)]
    scenes, mirrored = [], False
    for s in range(S):
        f = rng.uniform(0.4, 1.0) * max(H, W)
        intr = (f, rng.uniform(0.8, 1.2) * f, rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H)
        cfw = MC.pose(rng.uniform(-1.0, 1.0, 3), rng.uniform(-0.5, 0.5, 3))
        items = []
        for i in range(max(int(rng.randint(0, 9)), int(s == 0))):
            anchor = s == 0 and i == 0
            at = CC.at_pixel(intr, H, W, *(rng.uniform(0.35, 0.65, 2) if anchor else rng.uniform(-0.2, 1.2, 2)), 1.0)
            z = rng.uniform(0.35, 0.6) if anchor else rng.uniform(-0.1, 0.9)
            P = MC.pose(rng.uniform(-np.pi, np.pi, 3), (at[0] * abs(z), at[1] * abs(z), z))
            scale = rng.uniform(0.8, 1.6, 3) if anchor else rng.uniform(0.5, 2.5, 3) * min(1.0, max(abs(z), 0.01) / 0.6)   # small when close
            if rng.rand() < 0.25:
                scale[int(rng.randint(0, 3))] *= -1.0
                mirrored = True
            P[:3, :3] = P[:3, :3] * scale
            items.append((int(rng.randint(0, 2)), np.linalg.inv(cfw) @ P, int(rng.randint(0, 3))))
        scenes.append((intr, cfw, items))
    case = dict(CC.build(meshes, scenes, H, W), S=S, mirrored=mirrored, cull=bool(rng.rand() < 0.5), want_face=bool(rng.rand() < 0.5),
                t_min=float(T_MINS[rng.randint(0, len(T_MINS))]), tol=float(TOLS[rng.randint(0, len(TOLS))]), cls=int(rng.randint(0, 3)))
    assert max(H, W) <= MAX_SIDE
    case["spec"] = cam.render_depth(case["meshes"], case["instances"], case["inst_begin"], case["cameras"], H, W, case["cull"], case["t_min"],
                                    case["tol"])
    return case


SECTIONS = (("sdf", draw_sdf), ("raycast", draw_raycast), ("grasp", draw_grasp), ("render", draw_render))


class Draws:
    """Draws and rejected draws of a run, per section."""

    def __init__(self):
        self.drawn = {name: 0 for name, _ in SECTIONS}
        self.rejected = {name: 0 for name, _ in SECTIONS}
        self.reasons = {}

    def draw(self, name, fn, rng):
        """A useful case of a section; fn reports every draw it makes, with the reason it rejected it or None."""
        def tally(reason):
            self.drawn[name] += 1
            if reason is not None:
                self.rejected[name] += 1
                self.reasons[reason] = self.reasons.get(reason, 0) + 1
            return reason
        return fn(rng, tally)

    def share(self):
        return sum(self.rejected.values()) / max(sum(self.drawn.values()), 1)

    def __str__(self):
        return f"{sum(self.rejected.values())}/{sum(self.drawn.values())} draws rejected ({100.0 * self.share():.1f} %) {self.reasons}"


# ---------------------------------------------------------------------------------------------------------------------
# the device against the specification
# ---------------------------------------------------------------------------------------------------------------------
def check_sdf(case, torch, ops, dev):
    errs = []
    M = case["M"]
    sentinel = torch.arange(case["total"], dtype=torch.float32, device=dev) * 0.25 + 1000.0
    buf = sentinel.clone()
    vols = case["vols"]
    grids, origins, _, dropped = ops.mesh_sdf_batch([m[:2] for m in case["meshes"]], [v[0] for v in vols], [v[1] for v in vols], [v[2] for v in vols],
                                                    *_layouts(vols), out=buf, out_offsets=case["offsets"])
    torch.cuda.synchronize()
    written = np.zeros(case["total"], bool)
    for m in range(M):
        want, d, w = case["specs"][m]
        got = grids[m].cpu().numpy()
        n = got.size
        written[case["offsets"][m]: case["offsets"][m] + n] = True
        if dropped[m] or got.shape != want.data.shape or not np.array_equal(origins[m], want.origin):
            errs.append(f"sdf mesh {m}/{M}: layout differs")
            continue
        if not np.array_equal(np.abs(got).view(np.uint32), np.abs(want.data).view(np.uint32)):
            errs.append(f"sdf mesh {m}/{M}: {int((np.abs(got) != np.abs(want.data)).sum())} of {n} magnitudes differ")
        decided = (d > 0.0) & (np.abs(np.abs(w) - 0.5) > 1e-3)
        if not np.array_equal(np.signbit(got).ravel()[decided], np.signbit(want.data).ravel()[decided]):
            errs.append(f"sdf mesh {m}/{M}: signs differ on decided nodes")
    keep = torch.from_numpy(~written).to(dev)
    if not torch.equal(buf[keep], sentinel[keep]):
        errs.append("sdf: the gaps between the volumes changed")
    return errs, sum(int(np.prod(v[4])) for v in vols)


def check_raycast(case, torch, ops, dev):
    errs = []
    N, M = case["num_rays"], case["M"]
    rng = np.random.RandomState(N)
    o, d = rng.normal(size=(N, 3)), rng.normal(size=(N, 3))               # the rows nobody owns hold rays too
    for m in range(M):
        b, n = case["begins"][m], case["counts"][m]
        o[b: b + n], d[b: b + n] = case["rays"][m]
    batch = ops.RayBatch([m[:2] for m in case["meshes"]], case["counts"], case["begins"], N, chunks=case["chunks"], device=dev)
    t = torch.full((N,), -7.0, dtype=torch.float64, device=dev)
    face = torch.full((N,), -9, dtype=torch.int32, device=dev)
    ops.mesh_raycast_batch(batch, torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), case["t_min"], case["tol"], out=(t, face))
    torch.cuda.synchronize()
    t, face = t.cpu().numpy(), face.cpu().numpy()
    owned = np.zeros(N, bool)
    for m in range(M):
        b, n = case["begins"][m], case["counts"][m]
        owned[b: b + n] = True
        want_t, want_f = gr.mesh_raycast(*case["meshes"][m][:2], *case["rays"][m], case["t_min"], case["tol"])
        if not (np.array_equal(t[b: b + n].view(np.int64), want_t.view(np.int64)) and np.array_equal(face[b: b + n], want_f)):
            errs.append(f"raycast mesh {m}/{M} ({n} {case['kinds'][m]} rays, chunks {case['chunks']} -> {batch.chunks}, t_min {case['t_min']}, "
                        f"tol {case['tol']}): {int((face[b: b + n] != want_f).sum())} faces differ")
    if not ((t[~owned] == -7.0).all() and (face[~owned] == -9).all()):
        errs.append("raycast: a row outside every range was written")
    return errs, sum(case["counts"])


def check_grasp(case, torch, ops, dev):
    errs = []
    M, vols = case["M"], case["vols"]
    pool = torch.full((case["total"],), 1000.0, dtype=torch.float32, device=dev)
    meshes = [m[:2] for m in case["meshes"]]
    grids, origins, _, _ = ops.mesh_sdf_batch(meshes, [v[0] for v in vols], [v[1] for v in vols], [v[2] for v in vols], *_layouts(vols),
                                              out=pool, out_offsets=case["offsets"])
    counts = [len(c[0]) for c in case["contacts"]]
    layout = [(origins[m], vols[m][0], vols[m][2], vols[m][4], case["offsets"][m]) for m in range(M)]
    batch = ops.RayBatch(meshes, counts, chunks=case["chunks"], device=dev, layout=layout)
    hits = [gr.mesh_raycast(*meshes[m], case["contacts"][m][0], case["contacts"][m][2]) for m in range(M)]   # the specification's chain
    normals = [gr.face_normals(*meshes[m])[0] for m in range(M)]
    to = lambda xs: torch.from_numpy(np.ascontiguousarray(np.concatenate(xs))).to(dev)
    cs = gr.approach_angles(case["A"])
    poses, valid = ops.grasp_poses(batch, to([c[0] for c in case["contacts"]]), to([c[1] for c in case["contacts"]]), to([c[2] for c in case["contacts"]]),
                                   to([h[0] for h in hits]), to([h[1] for h in hits]), to(normals), cs, case["probe"], pool, case["max_width"],
                                   case["min_width"], float(np.cos(case["cone"])), case["pad_depth"], case["clearance"])
    torch.cuda.synchronize()
    poses, valid = poses.cpu().numpy(), valid.cpu().numpy()
    at = 0
    for m in range(M):
        p1, n1, d = case["contacts"][m]
        grid = sc.SdfGrid(grids[m].cpu().numpy(), origins[m], vols[m][0])
        want_p, want_v, _ = gr.grasp_poses(p1, n1, d, hits[m][0], hits[m][1], normals[m], cs, grid, case["probe"], case["max_width"], case["min_width"],
                                           case["cone"], case["pad_depth"], case["clearance"], vols[m][2])
        got_p, got_v = poses[at: at + counts[m]], valid[at: at + counts[m]]
        at += counts[m]
        if not np.array_equal(got_p.view(np.int64), np.ascontiguousarray(want_p).view(np.int64)):
            errs.append(f"grasp mesh {m}/{M}: poses differ")
        if not np.array_equal(got_v.astype(bool), want_v):
            errs.append(f"grasp mesh {m}/{M}: {int((got_v.astype(bool) != want_v).sum())} valid flags differ")
    return errs, int(valid.sum())


def check_render(case, torch, ops, dev):
    errs = []
    H, W = case["H"], case["W"]
    b = ops.CameraBatch(case["meshes"], case["instances"], case["inst_begin"], case["cameras"], device=dev)
    got = ops.render_depth(b, H, W, cull=case["cull"], want_face=case["want_face"], t_min=case["t_min"], tol=case["tol"])
    torch.cuda.synchronize()
    want = case["spec"]
    if not np.array_equal(got[0].cpu().numpy().view(np.int64), want[0].view(np.int64)):
        errs.append(f"render {case['S']}x{H}x{W} cull {case['cull']}: depths differ")
    if not np.array_equal(got[1].cpu().numpy(), want[1]):
        errs.append(f"render {case['S']}x{H}x{W} cull {case['cull']}: instances differ")
    if (got[2] is None) != (not case["want_face"]) or (got[2] is not None and not np.array_equal(got[2].cpu().numpy(), want[2])):
        errs.append(f"render {case['S']}x{H}x{W} cull {case['cull']}: faces differ")
    if errs:
        return errs, 0                                                  # the clouds are taken from the device's images
    for cls in (case["cls"], -1):
        per = cam.pixel_clouds(want[0], want[1], CC.labels(case), case["inst_begin"], case["cameras"], cls)
        points, begin = ops.pixel_clouds(b, got[0], got[1], cls)
        torch.cuda.synchronize()
        flat = np.concatenate(per)
        if begin.tolist() != np.concatenate([[0], np.cumsum([len(x) for x in per])]).tolist():
            errs.append(f"clouds class {cls}: scene_begin differs")
        elif not np.array_equal(points.cpu().numpy().view(np.int64), flat.view(np.int64)):
            errs.append(f"clouds class {cls}: points differ")
    return errs, case["S"] * H * W


CHECKS = dict(sdf=check_sdf, raycast=check_raycast, grasp=check_grasp, render=check_render)


def main(trials=None, seed=None):
    import torch
    from omg_planner_amd import ops
    trials = int(trials if trials is not None else (sys.argv[1] if len(sys.argv) > 1 else 40))
    rng = np.random.RandomState(int(seed if seed is not None else (sys.argv[2] if len(sys.argv) > 2 else 0)))
    dev = torch.device("cuda:0")
    draws, bad, t0 = Draws(), 0, time.time()
    work = {name: 0 for name, _ in SECTIONS}
    for k in range(trials):
        errs = []
        for name, fn in SECTIONS:
            try:
                e, n = CHECKS[name](draws.draw(name, fn, rng), torch, ops, dev)
                errs += e
                work[name] += n
            except Exception as e:  # noqa: BLE001
                errs.append(f"{name}: exception {type(e).__name__}: {e}")
        if errs:
            bad += 1
            print(f"trial {k}: FAIL " + "; ".join(errs), flush=True)
    too_many = draws.share() > MAX_REJECTED
    if too_many:
        print(f"FAIL more than {100 * MAX_REJECTED:.0f} % of the draws rejected")
    print(f"{trials - bad}/{trials} trials agree; {work['sdf']} nodes, {work['raycast']} rays, {work['grasp']} valid grasps, {work['render']} pixels "
          f"compared bit for bit; {draws}; {time.time() - t0:.0f} s")
    return 1 if bad or too_many else 0


if __name__ == "__main__":
    sys.exit(main())
