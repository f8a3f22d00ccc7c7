"""CPU tests of grasp sampling (omg-planner_amd/grasps.py, csrc/omg_grasp.hip): the specification against
geometry, the tie and crack rules, the pose construction, the gripper filter on known shapes, csrc/omg_grasp_body.h compiled for
the host against the specification bit for bit, every argument error of the C ABI, and the kernels' register budget."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import grasp_cases as GC
from tests import kernel_build as KB
from tests import mesh_cases as MC

CONE = np.deg2rad(15.0)


@pytest.fixture(scope="module")
def G():
    from omg_planner_amd import grasps
    return grasps


# ---------------------------------------------------------------------------------------------------------------------
# 1-3: the ray cast
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("posed", [False, True])
def test_ray_cast_against_the_box(G, posed):
    pose = GC.BOX_POSE if posed else None
    v, f = MC.box_mesh(MC.BOX_HALF, pose)
    o, d, want, opposite = GC.box_inward_rays(pose)
    t, face = G.mesh_raycast(v, f, o, d)
    assert t.dtype == np.float64 and face.dtype == np.int32
    assert np.abs(t - want).max() <= 1e-12
    assert ((face == opposite[:, 0]) | (face == opposite[:, 1])).all()
    # t_min excludes the face a ray starts on (that is why the hits above are the opposite faces), and anything nearer
    t2, face2 = G.mesh_raycast(v, f, o, d, t_min=0.11)
    near = want < 0.11                                    # the 0.10 and 0.06 slabs; the 0.16 one is still hit
    assert np.isinf(t2[near]).all() and (face2[near] == -1).all() and (face2[~near] == face[~near]).all() and (~near).sum() == 16


def _lowest_nearest(G, v, f, o, d, incident):
    """The face the tie rule promises for every ray: of the faces incident to its crack, the lowest index among those whose own
    t is the smallest (each face of the mesh cast alone, against all rays)."""
    alone = np.stack([G.mesh_raycast(v, f[[j]], o, d)[0] for j in range(len(f))])  # [F, N]
    want = np.empty(len(o), np.int32)
    for i, fs in enumerate(incident):
        fs = sorted(fs)
        ts = alone[fs, i]
        want[i] = fs[int(np.flatnonzero(ts == ts.min())[0])]
    return want


def test_cracks_and_ties(G):
    """Rays through the shared diagonal of each box quad, and through vertices and edges of an icosphere: no ray falls between
    two triangles, and of equal hits the lower face index is returned.  (Where two neighbours' t differ in the last bits — the
    posed box, the sphere — the nearer one is returned, as t < best says; the rule is then checked on the faces that do tie.)
    With tol = 0 some of these rays do fall through; nothing is asserted on that case."""
    v, f = MC.box_mesh(MC.BOX_HALF)
    o, d, quad = GC.box_diagonal_rays()
    t, face = G.mesh_raycast(v, f, o, d)
    assert (face == quad[:, 0]).all()                    # exact ties on the axis-aligned box: the lower index, every time
    assert np.abs(t - 0.05).max() <= 1e-16
    top = quad[:, 0] == 10                               # the 99 rays down the top face's diagonal, cast from the bottom face
    start = o[top].copy()
    start[:, 2] = -MC.BOX_HALF[2]
    t_in, face_in = G.mesh_raycast(v, f, start, -d[top])
    assert len(np.unique(t_in)) == 1 and abs(t_in[0] - 0.06) <= np.spacing(0.06) and (face_in == 10).all()  # one value, all 99 (the double above 0.06)
    vp, fp = MC.box_mesh(MC.BOX_HALF, GC.BOX_POSE)
    o, d, quad = GC.box_diagonal_rays(GC.BOX_POSE)
    t, face = G.mesh_raycast(vp, fp, o, d)
    assert (face >= 0).all() and np.abs(t - 0.05).max() <= 1e-12
    assert (face == _lowest_nearest(G, vp, fp, o, d, [list(q) for q in quad])).all()
    sv, sf = MC.icosphere(2)
    o, d, incident = GC.sphere_crack_rays(sv, sf)
    t, face = G.mesh_raycast(sv, sf, o, d)
    assert len(o) == 162 + 3 * 480 and (face >= 0).all() and np.isfinite(t).all()
    assert all(face[i] in incident[i] for i in range(len(o)))
    assert (face == _lowest_nearest(G, sv, sf, o, d, incident)).all()


def test_misses_and_parallels(G):
    sv, sf = MC.icosphere(2)
    o, d = GC.outward_rays(sv, sf)
    t, face = G.mesh_raycast(sv, sf, o, d)
    assert np.isposinf(t).all() and (face == -1).all()
    v, f = GC.two_boxes()
    t, face = G.mesh_raycast(v, f, *GC.PLANE_RAY)      # in the plane of faces 10, 11 (and parallel to 8, 9 and four of the second box)
    assert not np.isnan(t).any() and abs(t[0] - 0.45) <= 1e-15 and face[0] in (12, 13)
    # a mesh that is nothing but faces parallel to the ray: a miss, not a NaN
    t, face = G.mesh_raycast(v, f[[8, 9, 10, 11]], *GC.PLANE_RAY)
    assert np.isposinf(t).all() and (face == -1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4: poses
# ---------------------------------------------------------------------------------------------------------------------
def _free_grid():
    from omg_planner_amd import scenes as sc
    return sc.SdfGrid(np.ones((2, 2, 2), np.float32), np.zeros(3), 0.01)


def _directions():
    rng = np.random.RandomState(3)
    d = rng.normal(size=(200, 3))
    d /= np.sqrt((d * d).sum(1))[:, None]
    s2, s3 = np.sqrt(0.5), np.sqrt(1.0 / 3.0)
    special = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1],            # exact axes
               [s2, s2, 0], [0, s2, -s2], [s2, 0, s2], [s3, s3, s3], [-s3, s3, -s3],              # two or three equal smallest
               [0.6, 0.6, np.sqrt(0.28)], [0.8, 0.0, 0.6], [np.sqrt(0.28), -0.6, 0.6]]
    return np.concatenate([np.array(special, np.float64), d])


def test_pose_construction(G):
    d = _directions()
    N = len(d)
    rng = np.random.RandomState(4)
    p1 = rng.uniform(-0.4, 0.4, (N, 3))
    t = rng.uniform(0.01, 0.08, N)
    pad = 0.088
    poses, valid, width = G.grasp_poses(p1, -d, d, t, np.arange(N, dtype=np.int32), d, G.approach_angles(8), _free_grid(),
                                        G.default_probe(), cone=CONE, pad_depth=pad)
    assert poses.shape == (N, 8, 4, 4) and valid.all() and np.array_equal(width, t)
    R, o = poses[:, :, :3, :3], poses[:, :, :3, 3]
    assert np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max() <= 1e-14
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-14
    assert np.array_equal(R[:, :, :, 1].view(np.uint64), np.broadcast_to(d[:, None, :], (N, 8, 3)).copy().view(np.uint64))  # y is d, bit for bit
    m = p1 + (0.5 * t)[:, None] * d
    assert np.abs((R @ np.array([0.0, 0.0, pad])) + o - m[:, None, :]).max() <= 1e-15
    assert np.array_equal(poses[:, :, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (N, 8, 4)))
    # the eight approach directions of a pair turn about the closing axis
    z = R[:, :, :, 2]
    assert np.abs((z * d[:, None, :]).sum(-1)).max() <= 1e-15 and np.abs((z[:, 0] * z[:, 2]).sum(-1)).max() <= 1e-15
    # a ray that is not antipodal: zeros, invalid
    f2 = np.arange(N, dtype=np.int32)
    f2[::3] = -1
    t2 = t.copy()
    t2[1::3] = np.inf
    poses, valid, _ = G.grasp_poses(p1, -d, d, t2, f2, d, G.approach_angles(4), _free_grid(), G.default_probe())
    bad = (f2 < 0) | np.isinf(t2)
    assert not valid[bad].any() and (poses[bad] == 0).all() and valid[~bad].all() and np.isfinite(poses).all()


def test_nearest_sample_lookup_and_clearance(G):
    """One probe point against a volume with a single negative sample, for both sample conventions."""
    from omg_planner_amd import scenes as sc
    data = np.ones((4, 5, 6), np.float32)
    data[2, 3, 1] = -1.0
    data[0, 0, 0] = 0.004
    grid = sc.SdfGrid(data, np.array([0.1, -0.2, 0.3]), 0.02)
    d = np.array([[0.0, 1.0, 0.0]])
    for sample, off in (("centre", 0.5), ("node", 0.0)):
        z = G.grasp_poses(np.zeros((1, 3)), -d, d, [0.05], [0], d, G.approach_angles(1), grid, np.zeros((1, 3)), sample=sample)[0][0, 0, :3, 2]
        # the hand's origin o = m - pad_depth * z is put on the point looked up; the probe is the single point (0, 0, 0)
        def at(ijk, frac, clearance=0.0):
            w = grid.origin + (np.array(ijk) + off + np.array(frac)) * grid.delta
            p1 = w - 0.5 * 0.05 * d[0] + 0.088 * z
            return bool(G.grasp_poses(p1[None], -d, d, [0.05], [0], d, G.approach_angles(1), grid, np.zeros((1, 3)), clearance=clearance,
                                      sample=sample)[1][0, 0])
        assert not at((2, 3, 1), (0.0, 0.0, 0.0)) and not at((2, 3, 1), (0.4, -0.4, 0.4)) and at((2, 3, 1), (0.6, 0.0, 0.0))
        assert at((2, 3, 2), (0.0, 0.0, 0.0)) and at((0, 0, 0), (0.0, 0.0, 0.0)) and not at((0, 0, 0), (0.0, 0.0, 0.0), clearance=0.005)
        assert at((-3, 3, 1), (0.0, 0.0, 0.0)) and at((2, 30, 1), (0.0, 0.0, 0.0))  # outside the grid: free


# ---------------------------------------------------------------------------------------------------------------------
# 5: the filter on known shapes
# ---------------------------------------------------------------------------------------------------------------------
_CHAIN = {}


def chain(name):
    """mesh -> volume (scenes.mesh_sdf, delta 0.005) -> 512 rays, 8 angles, 15 degrees: computed once per shape."""
    from omg_planner_amd import grasps as G, scenes as sc
    if name not in _CHAIN:
        v, f = {"box": lambda: MC.box_mesh(MC.BOX_HALF), "posed_box": lambda: MC.box_mesh(MC.BOX_HALF, GC.BOX_POSE),
                "large_sphere": lambda: MC.icosphere(1, 0.06), "small_sphere": lambda: MC.icosphere(2, 0.025)}[name]()
        grid = sc.mesh_sdf(v, f, 0.005)
        v, f = G.outward_mesh(v, f)
        rng = np.random.RandomState(0)
        p1, _, n1 = G.surface_samples(v, f, 512, rng)
        d = G.ray_directions(n1, CONE, rng)
        t, f2 = G.mesh_raycast(v, f, p1, d)
        nrm = G.face_normals(v, f)[0]
        poses, valid, width = G.grasp_poses(p1, n1, d, t, f2, nrm, G.approach_angles(8), grid, G.default_probe(), cone=CONE)
        _CHAIN[name] = dict(v=v, f=f, grid=grid, p1=p1, n1=n1, d=d, t=t, f2=f2, nrm=nrm, poses=poses, valid=valid, width=width)
    return _CHAIN[name]


@pytest.mark.parametrize("name", ["box", "posed_box"])
def test_filter_on_the_box(name):
    c = chain(name)
    valid, poses = c["valid"], c["poses"]
    assert valid.sum() > 0
    zaxis = (GC.BOX_POSE if name == "posed_box" else np.eye(4))[:3, :3]
    y = poses[valid][:, :3, 1] @ zaxis                     # the closing axes in the box's own frame
    cos15 = np.cos(CONE)
    assert (np.abs(y[:, 2]) >= cos15 - 1e-12).all()        # within 15 degrees of the box's +-z
    assert (np.abs(y[:, 0]) < 0.5).all() and (np.abs(y[:, 1]) < 0.5).all()  # none along x or y: 0.10 and 0.16 exceed max_width
    w = c["width"][valid.any(1)]
    assert (w >= 0.06 - 1e-12).all() and (w <= 0.06 / cos15 + 1e-12).all()
    # surface points lie on the mesh, directions inside the cone
    assert np.abs(np.sqrt((c["d"] ** 2).sum(1)) - 1).max() <= 1e-15 and (-(c["d"] * c["n1"]).sum(1) >= cos15 - 1e-12).all()


def test_filter_on_spheres():
    assert chain("large_sphere")["valid"].sum() == 0       # every chord along a normal is 0.12 > max_width
    assert not (chain("large_sphere")["poses"] != 0).any()
    assert chain("small_sphere")["valid"].sum() > 0


def test_sample_grasps_chain_and_rng_order(G):
    c = chain("box")
    got = G.sample_grasps(*MC.box_mesh(MC.BOX_HALF), c["grid"], 512, 8, np.random.RandomState(0), cone=CONE)
    assert np.array_equal(got, c["poses"][c["valid"]])     # (ray, angle) order
    rng = np.random.RandomState(0)
    some = G.sample_grasps(*MC.box_mesh(MC.BOX_HALF), c["grid"], 512, 8, rng, cone=CONE, max_grasps=10)
    ref = np.random.RandomState(0)
    ref.random_sample((512, 3)), ref.random_sample((512, 2))
    keep = np.sort(ref.choice(len(got), 10, replace=False))
    assert np.array_equal(some, got[keep]) and rng.random_sample() == ref.random_sample()
    # a mesh whose faces point inwards gives the same grasps; cone = 0 gives exactly -n
    flipped = G.sample_grasps(*MC.box_mesh(MC.BOX_HALF, flip=True), c["grid"], 512, 8, np.random.RandomState(0), cone=CONE)
    assert np.array_equal(flipped, got)
    assert np.array_equal(G.ray_directions(c["n1"], 0.0, np.random.RandomState(1)), -c["n1"])
    probe = G.default_probe()
    assert probe.shape == (100, 3) and np.abs(probe[:, 1]).max() == 0.050 and probe[:, 2].max() == 0.098 and probe[:, 2].min() == 0.048


# ---------------------------------------------------------------------------------------------------------------------
# 6: the kernel bodies compiled for the host
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include "omg_grasp_body.h"
extern "C" void host_raycast(const double* verts, const int32_t* faces, int nf, const double* o, const double* d, int n, double t_min,
                             double tol, double* t_out, int32_t* f_out) {
    for (int i = 0; i < n; ++i) {
        double best = __builtin_inf();
        int32_t face = -1;
        for (int q = 0; q < nf; ++q) {
            double T[9];
            for (int c = 0; c < 3; ++c)
                for (int a = 0; a < 3; ++a) T[c * 3 + a] = verts[faces[q * 3 + c] * 3 + a];
            mesh_raycast_pair(o[i * 3], o[i * 3 + 1], o[i * 3 + 2], d[i * 3], d[i * 3 + 1], d[i * 3 + 2], T, q, t_min, -tol, 1.0 + tol, best, face);
        }
        t_out[i] = best;
        f_out[i] = face;
    }
}
extern "C" void host_poses(const double* p1, const double* n1, const double* d, const double* t, const int32_t* f2, int n,
                           const double* normals, const double* cs, int A, const double* probe, int Q, const double* origin, double delta,
                           double sample_offset, const int32_t* dims, const float* vol, double max_width, double min_width,
                           double cos_cone, double pad_depth, double clearance, double* poses, uint8_t* valid) {
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < A; ++a) {
            grasp_frame F;
            const int fn = f2[i] < 0 ? 0 : f2[i];
            bool ok = grasp_pose_pair(p1[i * 3], p1[i * 3 + 1], p1[i * 3 + 2], n1[i * 3], n1[i * 3 + 1], n1[i * 3 + 2], d[i * 3], d[i * 3 + 1],
                                      d[i * 3 + 2], t[i], f2[i], normals[fn * 3], normals[fn * 3 + 1], normals[fn * 3 + 2], cs[a * 2],
                                      cs[a * 2 + 1], max_width, min_width, cos_cone, pad_depth, F);
            double* P = poses + ((long)i * A + a) * 16;
            for (int k = 0; k < 16; ++k) P[k] = 0.0;
            valid[(long)i * A + a] = 0;
            if (!ok) continue;
            for (int q = 0; q < Q && ok; ++q)
                ok = !grasp_probe_collides(F, probe[q * 3], probe[q * 3 + 1], probe[q * 3 + 2], origin, delta, sample_offset, dims, vol, (float)clearance);
            P[0] = F.xx, P[1] = F.yx, P[2] = F.zx, P[3] = F.ox, P[4] = F.xy, P[5] = F.yy, P[6] = F.zy, P[7] = F.oy;
            P[8] = F.xz, P[9] = F.yz, P[10] = F.zz, P[11] = F.oz, P[15] = 1.0;
            valid[(long)i * A + a] = ok;
        }
}
"""


@KB.requires_host_cxx
def test_kernel_bodies_compiled_for_the_host_equal_the_specification(G, tmp_path):
    """csrc/omg_grasp_body.h is what the kernels do per (ray, face) pair, per (ray, angle) pair and per probe point; compiled for
    the host without contraction it gives the specification's t as uint64 bits and its face on 2 000 (ray, face set) cases, and
    the poses as bits with the same flags."""
    lib = KB.host_harness(_HOST_HARNESS, tmp_path)
    vp, dbl = C.c_void_p, C.c_double
    lib.host_raycast.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, dbl, dbl, vp, vp]
    lib.host_poses.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, dbl, dbl, vp, vp, dbl, dbl, dbl, dbl, dbl, vp, vp]
    ico3 = MC.icosphere(3, 0.06, (0.003, -0.002, 0.001))
    sets = [MC.box_mesh(MC.BOX_HALF), MC.box_mesh(MC.BOX_HALF, GC.BOX_POSE), MC.icosphere(2), (ico3[0], ico3[1][:257]), GC.two_boxes()]
    cases = 0
    for k, (v, f) in enumerate(sets):
        v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int32)
        o, d = GC.mixed_rays(v, f, 380, seed=k)
        extra = [GC.box_diagonal_rays()[:2], GC.box_diagonal_rays(GC.BOX_POSE)[:2], GC.sphere_crack_rays(v, f, 100)[:2] if k == 2 else None,
                 None, GC.PLANE_RAY][k]
        if extra is not None:
            o, d = np.ascontiguousarray(np.concatenate([o, extra[0]])), np.ascontiguousarray(np.concatenate([d, extra[1]]))
        for tol in (1e-9, 0.0):
            t, face = G.mesh_raycast(v, f, o, d, tol=tol)
            ht, hf = np.zeros(len(o)), np.zeros(len(o), np.int32)
            lib.host_raycast(v.ctypes.data, f.ctypes.data, len(f), o.ctypes.data, d.ctypes.data, len(o), 1e-6, tol, ht.ctypes.data, hf.ctypes.data)
            assert np.array_equal(ht.view(np.uint64), t.view(np.uint64)) and np.array_equal(hf, face), (k, tol)
        cases += len(o)
        assert (face >= 0).any() and (face < 0).any()
    assert cases >= 2000
    for name, sample, clearance, probe in (("box", "centre", 0.0, G.default_probe()), ("posed_box", "node", 0.004, G.default_probe()),
                                           ("small_sphere", "centre", 0.002, G.default_probe()[:1]), ("large_sphere", "centre", 0.0, G.default_probe())):
        c = chain(name)
        cs = G.approach_angles(8)
        poses, valid, _ = G.grasp_poses(c["p1"], c["n1"], c["d"], c["t"], c["f2"], c["nrm"], cs, c["grid"], probe, cone=CONE, clearance=clearance, sample=sample)
        N = len(c["t"])
        hp, hv = np.full((N, 8, 4, 4), 7.0), np.full((N, 8), 7, np.uint8)
        data = np.ascontiguousarray(c["grid"].data, np.float32)
        dims = np.array(data.shape, np.int32)
        origin = np.ascontiguousarray(c["grid"].origin, np.float64)
        f2 = np.ascontiguousarray(c["f2"], np.int32)
        lib.host_poses(c["p1"].ctypes.data, c["n1"].ctypes.data, c["d"].ctypes.data, c["t"].ctypes.data, f2.ctypes.data, N, c["nrm"].ctypes.data,
                       cs.ctypes.data, 8, probe.ctypes.data, len(probe), origin.ctypes.data, float(c["grid"].delta),
                       {"centre": 0.5, "node": 0.0}[sample], dims.ctypes.data, data.ctypes.data, 0.08, 0.005, float(np.cos(CONE)), 0.088, clearance,
                       hp.ctypes.data, hv.ctypes.data)
        assert np.array_equal(hp.view(np.uint64), poses.view(np.uint64)) and np.array_equal(hv.astype(bool), valid), name


# ---------------------------------------------------------------------------------------------------------------------
# 7: argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _mesh_records(M=2, **over):
    from omg_planner_amd import _lib
    rec = (_lib.Mesh * M)()
    for m in range(M):
        r = rec[m]
        r.origin[:], r.delta, r.sample_offset, r.dims[:] = [0.0, 0.0, 0.0], 0.01, 0.5, [5, 6, 7]
        r.out_offset, r.first_workgroup = 210 * m, 0
        r.vert_begin, r.vert_count, r.face_begin, r.face_count = 8 * m, 8, 300 * m, 300
    for k, val in over.items():
        if k in ("origin", "dims"):
            getattr(rec[M - 1], k)[:] = val
        else:
            setattr(rec[M - 1], k, val)
    return rec


def _work(counts=(300, 5), begins=(0, 300), chunks=2, faces=300):
    rows = []
    for m, (n, b) in enumerate(zip(counts, begins)):
        for r0 in range(0, n, 256):
            cut = [0, 256, faces][:chunks] + [faces] if chunks > 1 else [0, faces]
            for c in range(chunks):
                rows.append([m, b + r0, min(256, n - r0), cut[c], cut[c + 1] - cut[c], c])
    return np.ascontiguousarray(np.array(rows, np.int32).reshape(-1, 6))


def test_c_abi_argument_checks_without_gpu():
    """Every OMGX_ERR_INVALID / OMGX_ERR_UNSUPPORTED case of the three entry points is decided on the host copies before any HIP
    call."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    assert C.sizeof(_lib.RayWork) == 24 and _lib.RAYCAST_RAYS_PER_WORKGROUP == 256 == lib.omgx_mesh_sdf_tile()
    INV, UNS, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED, _lib.OMGX_OK
    assert lib.omgx_mesh_raycast_workspace_bytes(1000, 1) == 0 and lib.omgx_mesh_raycast_workspace_bytes(1000, 7) == 7 * 1000 * 12
    assert lib.omgx_mesh_raycast_workspace_bytes(-1, 2) == INV and lib.omgx_mesh_raycast_workspace_bytes(10, -1) == INV
    assert lib.omgx_mesh_raycast_workspace_bytes(10, 65) == INV
    assert lib.omgx_mesh_raycast_chunks(10, 300, 3) == 3 and lib.omgx_mesh_raycast_chunks(0, 300, 0) == 1
    assert lib.omgx_mesh_raycast_chunks(10, 300, -1) == INV and lib.omgx_mesh_raycast_chunks(-1, 300, 1) == INV
    assert lib.omgx_mesh_raycast_chunks(10, 0, 1) == INV and lib.omgx_mesh_raycast_chunks(10, 300, 65) == INV
    d = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    rb, rc = np.array([0, 300], np.int32), np.array([300, 5], np.int32)

    def ray(rec=None, M=2, verts=d, faces=d, meshes=d, host=True, begins=rb, counts=rc, work=d, h_work=None, chunks=2, origins=d, dirs=d,
            N=305, t_min=1e-6, tol=1e-9, t=d, face=d, ws=d):
        rec = _mesh_records(max(M, 1)) if rec is None else rec
        h_work = _work() if h_work is None else h_work
        return lib.omgx_mesh_raycast(verts, faces, meshes, C.cast(rec, C.c_void_p) if host else None, M,
                                     None if begins is None else begins.ctypes.data, None if counts is None else counts.ctypes.data, work,
                                     h_work.ctypes.data if len(h_work) else None, len(h_work), chunks, origins, dirs, N, t_min, tol, t, face, ws, None)
    for k in ("verts", "faces", "meshes", "begins", "counts", "work", "origins", "dirs", "t", "face", "ws"):
        assert ray(**{k: None}) == INV, k
    assert ray(host=False) == INV and ray(M=0) == INV and ray(M=-1) == INV and ray(N=-1) == INV and ray(N=304) == INV
    assert ray(chunks=-1) == INV and ray(chunks=65) == INV and ray(chunks=3) == INV and ray(chunks=1) == INV  # the list is for 2
    for bad in (-1e-6, float("nan"), float("inf")):
        assert ray(t_min=bad) == INV and ray(tol=bad) == INV
    assert ray(_mesh_records(face_count=0)) == INV and ray(_mesh_records(vert_count=0)) == INV
    assert ray(_mesh_records(vert_begin=-1)) == INV and ray(_mesh_records(face_begin=-1)) == INV
    assert ray(counts=np.array([300, -1], np.int32)) == INV and ray(begins=np.array([-1, 300], np.int32)) == INV
    assert ray(counts=np.array([300, 6], np.int32)) == INV               # the list does not cover the rays
    assert ray(begins=np.array([0, 299], np.int32), h_work=_work(begins=(0, 299))) == INV   # two meshes share row 299
    assert ray(h_work=_work()[:-1]) == INV and ray(h_work=_work()[:-2]) == INV and ray(h_work=np.concatenate([_work(), _work()[-2:]])) == INV
    for col, val in ((0, 1), (1, 1), (2, 255), (3, 1), (4, 255), (5, 1)):   # one wrong field of the first record
        w = _work()
        w[0, col] = val
        assert ray(h_work=w) == INV, col
    w = _work()
    w[1, 4] = 43                                                         # the face ranges stop short of the mesh
    assert ray(h_work=w) == INV
    w = _work()
    w[[0, 1]] = w[[1, 0]]                                                # chunks out of order
    assert ray(h_work=w) == INV
    w = _work()
    w[1, 4] = -1
    assert ray(h_work=w) == INV
    # nothing to do: no ray in any mesh
    assert ray(counts=np.array([0, 0], np.int32), h_work=np.zeros((0, 6), np.int32), work=None, origins=None, dirs=None, t=None, face=None) == OK

    pool = 420

    def pose(rec=None, M=2, meshes=d, host=True, begins=rb, counts=rc, work=d, h_work=None, chunks=2, N=305, A=8, Q=100, probe=d, cs=d,
             normals=d, pool_ptr=d, pool_elems=pool, widths=(0.08, 0.005, 0.96, 0.088, 0.0), ptrs=None):
        rec = _mesh_records(max(M, 1)) if rec is None else rec
        h_work = _work() if h_work is None else h_work
        p = dict(p1=d, n1=d, dirs=d, t=d, face2=d, poses=d, valid=d)
        p.update(ptrs or {})
        return lib.omgx_grasp_poses(meshes, C.cast(rec, C.c_void_p) if host else None, M, None if begins is None else begins.ctypes.data,
                                    None if counts is None else counts.ctypes.data, work, h_work.ctypes.data if len(h_work) else None,
                                    len(h_work), chunks, p["p1"], p["n1"], p["dirs"], p["t"], p["face2"], N, normals, cs, A, probe, Q, pool_ptr,
                                    pool_elems, *widths, p["poses"], p["valid"], None)
    for k in ("meshes", "begins", "counts", "work", "cs", "normals", "probe", "pool_ptr"):
        assert pose(**{k: None}) == INV, k
    for k in ("p1", "n1", "dirs", "t", "face2", "poses", "valid"):
        assert pose(ptrs={k: None}) == INV, k
    assert pose(host=False) == INV and pose(M=0) == INV and pose(N=-1) == INV and pose(N=304) == INV and pose(Q=-1) == INV
    assert pose(A=0) == INV and pose(A=-1) == INV and pose(A=65536) == INV and pose(chunks=0) == INV and pose(chunks=-1) == INV and pose(chunks=3) == INV
    for bad in ([0, 6, 7], [5, -1, 7], [5, 6, 0]):
        assert pose(_mesh_records(dims=bad)) == INV, bad
    for bad in (0.0, -0.01, float("inf"), float("nan")):
        assert pose(_mesh_records(delta=bad)) == INV, bad
    for bad in (0.25, 1.0, float("nan")):
        assert pose(_mesh_records(sample_offset=bad)) == INV, bad
    assert pose(_mesh_records(origin=[0.0, float("inf"), 0.0])) == INV and pose(_mesh_records(out_offset=-1)) == INV
    assert pose(_mesh_records(face_count=0)) == INV and pose(_mesh_records(face_begin=-1)) == INV
    assert pose(pool_elems=419) == INV and pose(pool_elems=-1) == INV        # the second volume leaves the pool
    assert pose(_mesh_records(dims=[2048, 2048, 513]), pool_elems=1 << 40) == UNS
    mixed = _mesh_records(delta=0.0)                                         # mesh 0 too big, mesh 1 invalid: the first mesh decides
    mixed[0].dims[:] = [2048, 2048, 513]
    assert pose(mixed, pool_elems=1 << 40) == UNS
    assert pose(mixed, pool_elems=pool) == UNS                               # and within a mesh, before the pool's bounds
    nan = float("nan")
    for i in range(5):
        w = [0.08, 0.005, 0.96, 0.088, 0.0]
        w[i] = nan
        assert pose(widths=tuple(w)) == INV, i
    assert pose(counts=np.array([300, 6], np.int32)) == INV and pose(h_work=_work()[:-1]) == INV
    assert pose(begins=np.array([0, 299], np.int32), h_work=_work(begins=(0, 299))) == INV
    assert pose(counts=np.array([0, 0], np.int32), h_work=np.zeros((0, 6), np.int32), work=None, ptrs=dict(p1=None, poses=None)) == OK
    assert pose(Q=0, probe=None, counts=np.array([0, 0], np.int32), h_work=np.zeros((0, 6), np.int32)) == OK  # an empty probe is legal


def test_wrapper_checks_without_gpu(G):
    from omg_planner_amd import _lib, ops
    v, f = MC.box_mesh(MC.BOX_HALF)
    E = _lib.OmgHipError
    bad = f.copy()
    bad[3, 1] = 8
    with pytest.raises(E, match="indices"):
        ops.RayBatch([(v, bad)], [4], chunks=1, device="cpu")
    with pytest.raises(E, match="zero area"):  # dropping them would renumber the faces that the results name
        ops.RayBatch([(v, np.concatenate([f[:3], [[0, 0, 1]], f[3:]]))], [4], chunks=1, device="cpu")
    with pytest.raises(E):
        ops.RayBatch([], [], chunks=1, device="cpu")
    with pytest.raises(E):
        ops.RayBatch([(v, f)], [4, 4], chunks=1, device="cpu")
    with pytest.raises(E, match="negative"):
        ops.RayBatch([(v, f)], [-1], chunks=1, device="cpu")
    with pytest.raises(E, match="overlap"):
        ops.RayBatch([(v, f), (v, f)], [4, 4], ray_begins=[0, 3], chunks=1, device="cpu")
    with pytest.raises(E, match="overlap"):
        ops.RayBatch([(v, f)], [4], ray_begins=[2], num_rays=5, chunks=1, device="cpu")
    with pytest.raises(E, match="chunks"):
        ops.RayBatch([(v, f)], [4], chunks=65, device="cpu")
    with pytest.raises(E):
        ops.RayBatch([(v, f)], [4], chunks=1, device="cpu", layout=[(np.zeros(3), 0.0, "centre", (4, 4, 4), 0)])
    with pytest.raises(E):
        ops.RayBatch([(v, f)], [4], chunks=1, device="cpu", layout=[(np.zeros(3), 0.01, "corner", (4, 4, 4), 0)])
    with pytest.raises(E):
        ops.RayBatch([(v, f)], [4], chunks=1, device="cpu", layout=[(np.zeros(3), 0.01, "centre", (4, 0, 4), 0)])
    # the work list of a forced split: 2 ray groups x 3 chunks over 600 faces in whole tiles, in the order the entry points check
    sv, sf = MC.icosphere(3)
    b = ops.RayBatch([(v, f), (sv, sf[:600])], [0, 300], ray_begins=[7, 20], num_rays=400, chunks=3, device="cpu")
    assert b.chunks == 3 and b.num_work == 6 and b.num_faces == 612
    assert b.h_work.tolist() == [[1, 20, 256, 0, 256, 0], [1, 20, 256, 256, 256, 1], [1, 20, 256, 512, 88, 2],
                                 [1, 276, 44, 0, 256, 0], [1, 276, 44, 256, 256, 1], [1, 276, 44, 512, 88, 2]]
    import torch
    with pytest.raises(E, match="device tensor"):
        ops.mesh_raycast_batch(b, torch.zeros((400, 3), dtype=torch.float64), torch.zeros((400, 3), dtype=torch.float64))
    with pytest.raises(E, match="layout"):
        ops.grasp_poses(b, *([None] * 9))
    with pytest.raises(E, match="finite"):
        ops.mesh_raycast_batch(b, None, None, t_min=-1.0)
    with pytest.raises(ValueError):
        G.sample_grasp_sets([(v, f)], [None, None], 4, 2, np.random.RandomState(0))


# ---------------------------------------------------------------------------------------------------------------------
# 8: registers
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_grasp_kernels_do_not_spill(tmp_path):
    """The compiler's resource remarks for csrc/omg_grasp.hip: no kernel uses scratch, and k_mesh_raycast keeps a ray's state and a
    face's nine coordinates in few enough registers for at least four waves per SIMD (65 VGPRs, seven)."""
    seen = KB.kernel_resources("omg_grasp.hip", tmp_path)
    kernels = {k: KB.one(seen, k) for k in ("k_mesh_raycast_reduce", "k_grasp_poses")}
    kernels["k_mesh_raycast"] = KB.one({n: v for n, v in seen.items() if "reduce" not in n}, "k_mesh_raycast")
    for k, v in kernels.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    assert kernels["k_mesh_raycast"]["Occupancy [waves/SIMD]"] >= 4 and kernels["k_mesh_raycast"]["VGPRs"] <= 128, kernels
