"""CPU tests of plan clearance (omg-planner_amd/clearance.py, csrc/omg_clearance.hip): the specification at
its edges as answers worked out by hand; csrc/omg_clearance_body.h compiled for the host, walked as the kernels walk it, equals
the specification bit for bit with and without the cull; the reach table bounds the path of every sphere centre; dense_configs;
the tunnelling case by the specification alone; every argument error of the specification, of the C ABI and of the wrappers;
the kernels use no scratch."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import clearance_cases as CC
from tests import kernel_build as KB

INF, NAN = CC.INF, CC.NAN


# ---------------------------------------------------------------------------------------------------------------------
# 1. the specification at its edges
# ---------------------------------------------------------------------------------------------------------------------
def test_sphere_edge_cases_as_known_answers():
    from omg_planner_amd import clearance as cl
    objects, begin, pool, launches = CC.edge_launch()
    for L in launches:
        world = cl.world_spheres(L["poses"], L["local"], L["link"])
        assert CC.same(world[0], L["local"])  # identity poses
        got = cl.sphere_clearance(objects, begin, pool, None, L["cfg"], world, L["link"], L["pad"], L["beyond"])
        assert tuple(None if x is None else x[0].item() for x in got) == L["want"], L["what"]
        assert got[0].dtype == np.float64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    # no sphere, and no configuration
    got = cl.sphere_clearance(objects, begin, pool, None, [0, 1], np.zeros((2, 0, 4)), [], np.zeros((2, 10)), 0.5)
    assert all(CC.same(g, w) for g, w in zip(got, [np.full(2, INF), np.full(2, -1, np.int32), np.full(2, -1, np.int32)] * 2))
    assert [len(x) for x in cl.sphere_clearance(objects, begin, pool, None, [], np.zeros((0, 3, 4)), [0, 1, 2], np.zeros((0, 10)), 0.5)] == [0] * 6


def test_self_edge_cases_as_known_answers():
    from omg_planner_amd import clearance as cl
    for what, sph, links, pairs, pad, want in CC.SELF_CASES:
        got = cl.self_clearance(np.array([sph], np.float64), links, pairs, None if pad is None else np.array([pad]))
        assert tuple(x[0].item() for x in got) == want, what
    got = cl.self_clearance(np.zeros((2, 0, 4)), [], np.ones((10, 10)), None)
    assert got[0].tolist() == [INF, INF] and got[1].tolist() == [-1, -1] and got[2].tolist() == [-1, -1]


def test_dense_configs():
    from omg_planner_amd import clearance as cl
    rng = np.random.default_rng(3)
    traj = rng.uniform(-2.0, 2.0, (3, 5, 9))
    traj[0, 1, 2], traj[1, 0, 0] = -0.0, -0.0  # a + (b - a) * 0 would turn -0.0 into +0.0
    for K in (1, 2, 7):
        q = cl.dense_configs(traj, K)
        assert q.shape == (3, 4 * K + 1, 9) and CC.same(q[:, ::K], traj)  # k = 0 returns the waypoint's bits, the last sample too
        for k in range(1, K):
            assert CC.same(q[:, k::K][:, :4], traj[:, :-1] + (traj[:, 1:] - traj[:, :-1]) * (k / K)), (K, k)
    assert CC.same(cl.dense_configs(traj, 1), traj)  # K = 1 is the identity
    assert CC.same(cl.dense_configs(traj[:, :1], 4), traj[:, :1])  # n = 1: T = 1
    assert cl.dense_configs(np.zeros((0, 3, 9)), 2).shape == (0, 5, 9)
    for bad in (dict(traj=traj, K=0), dict(traj=traj[:, :, :8], K=1), dict(traj=traj[0], K=1), dict(traj=traj[:, :0], K=1)):
        with pytest.raises(ValueError):
            cl.dense_configs(**bad)


def test_sample_pads_and_plan_report_on_written_numbers():
    """Two segments of one plan, K = 2, one link's half written by hand: half = (1, 3) on link 0; the pads of the five samples are
    (1, 1, 3, 3, 3) + slack; the margins (5, 4, 3, 0.5, 2) give segment margins (3, 0.5)."""
    from omg_planner_amd import clearance as cl
    half = np.zeros((1, 2, 10))
    half[0, :, 0] = (1.0, 3.0)
    pad = cl.sample_pads(half, 2, 0.25)
    assert pad[0, :, 0].tolist() == [1.25, 1.25, 3.25, 3.25, 3.25] and (pad[0, :, 1:] == 0.25).all()
    assert cl.sample_pads(np.zeros((2, 0, 10)), 3, 0.5).tolist() == [[[0.5] * 10]] * 2
    rho = np.zeros((10, 9))
    rho[0, 0], rho[0, 8] = 2.0, 1.0
    traj = np.zeros((1, 3, 9))
    traj[0, 1, 0], traj[0, 2, 0], traj[0, 2, 8] = 2.0, -2.0, 4.0  # len_0 = 2*2 = 4 and 2*4 + 1*4 = 12: half = (4/2)/2, (12/2)/2
    clear, margin = np.array([[5.0, 4.0, -1.0, -2.0, 2.0]]), np.array([[5.0, 4.0, 3.0, 0.5, 2.0]])
    r = cl.plan_report(traj, 2, rho, 0.5, 0.25, 4.0, clear, margin)
    assert r["half"][0, :, 0].tolist() == [1.0, 3.0] and r["segment_margin"].tolist() == [[3.0, 0.5]]
    assert r["certified"].tolist() == [[True, True]] and r["plan_certified"].tolist() == [True]  # 0.5 + 3 + 0.25 <= 4
    assert r["collides"].tolist() == [True] and r["first_hit"].tolist() == [2] and r["min_clearance"].tolist() == [-2.0]
    r = cl.plan_report(traj, 2, rho, 0.5, 0.25, 3.5, clear, margin)  # the second segment's reach leaves `beyond`
    assert r["certified"].tolist() == [[True, False]] and r["plan_certified"].tolist() == [False]
    r = cl.plan_report(traj, 2, rho, 0.5, 0.25, 4.0, np.abs(clear), np.array([[5.0, 4.0, 0.0, 0.5, 2.0]]))  # a margin of 0 is not > 0
    assert r["certified"].tolist() == [[False, False]] and r["collides"].tolist() == [False] and r["first_hit"].tolist() == [-1]


# ---------------------------------------------------------------------------------------------------------------------
# 2. csrc/omg_clearance_body.h on the host
# ---------------------------------------------------------------------------------------------------------------------
_HOST_HARNESS = r"""
#include "omg_clearance_body.h"
static void butterfly(clear_best* m) {  // wave_best: lane l takes lane l ^ s, s = 32 .. 1
    for (int s = 32; s >= 1; s >>= 1) {
        clear_best next[64];
        for (int l = 0; l < 64; ++l) next[l] = m[l], clear_take(next[l], m[l ^ s].v, m[l ^ s].a, m[l ^ s].b);
        for (int l = 0; l < 64; ++l) m[l] = next[l];
    }
}
// Configuration by configuration as a wave of k_sphere_clearance walks it: chunks of 256 spheres, 64 lanes on the spheres
// j0 + lane of a chunk, the records in order, the cull as one vote of the 64 lanes -> the number of (64 spheres, record) skips.
extern "C" int64_t host_sphere_clearance(const omgx_object* objects, int num_objects, const int32_t* scene_begin, int S, const float* pool,
                                         int64_t pool_elems, const uint8_t* visible, const int32_t* cfg, int B, const double* poses,
                                         const double* local, const int32_t* link, int N, const double* pad, double beyond, int cull,
                                         double* clear, int32_t* cs, int32_t* co, double* margin, int32_t* ms, int32_t* mo, double* world) {
    int64_t skipped = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int first = scene_begin[cfg[b]], count = scene_begin[cfg[b] + 1] - first;
        clear_best bc[64], bm[64];
        for (int l = 0; l < 64; ++l) bc[l] = clear_none(), bm[l] = clear_none();
        for (int n0 = 0; n0 < N; n0 += 256) {
            const int cnt = N - n0 < 256 ? N - n0 : 256;
            for (int j0 = 0; j0 < cnt; j0 += 64) {
                double w[64][3], r[64], rm[64];
                int n[64];
                bool valid[64];
                for (int l = 0; l < 64; ++l) {
                    valid[l] = j0 + l < cnt;
                    n[l] = n0 + (valid[l] ? j0 + l : cnt - 1);
                    clear_world(poses + (b * 10 + link[n[l]]) * 16, local + (int64_t)n[l] * 4, w[l]);
                    r[l] = local[(int64_t)n[l] * 4 + 3];
                    rm[l] = pad ? r[l] + pad[b * 10 + link[n[l]]] : r[l];
                    if (valid[l] && world) for (int k = 0; k < 4; ++k) world[(b * N + n[l]) * 4 + k] = k < 3 ? w[l][k] : r[l];
                }
                for (int k = 0; k < count; ++k) {
                    const omgx_object& ob = objects[first + k];
                    if (!clear_record_used(ob, visible, first + k, pool_elems)) continue;
                    vcam_grid G;
                    vcam_set_grid(ob.lo, ob.dim, ob.inv_delta, ob.grid_offset, G);
                    vcam_ray R[64];
                    double e[64];
                    bool reach[64], any = false;
                    for (int l = 0; l < 64; ++l) e[l] = clear_reach(G, ob.pose_inv, w[l], R[l]), reach[l] = valid[l] && e[l] <= beyond, any = any || reach[l];
                    if (cull && !any) {
                        ++skipped;
                        continue;
                    }
                    for (int l = 0; l < 64; ++l) {
                        const double d = vcam_sample<false>(G, pool, R[l], 0.0, nullptr) - e[l];
                        if (reach[l]) clear_take(bc[l], d - r[l], n[l], k), clear_take(bm[l], d - rm[l], n[l], k);
                    }
                }
            }
        }
        butterfly(bc), butterfly(bm);
        clear[b] = bc[0].v, cs[b] = bc[0].a, co[b] = bc[0].b;
        if (margin) margin[b] = bm[0].v, ms[b] = bm[0].a, mo[b] = bm[0].b;
    }
    return skipped;
}
// As k_self_clearance: thread t of 256 takes j = i + 1 + t, i + 1 + t + 256, ...; four butterflies, then the waves in order.
extern "C" void host_self_clearance(const double* world, int B, const int32_t* link, int N, const uint8_t* pairs, const double* pad, double* out,
                                    int32_t* wi, int32_t* wj) {
    double* sp = new double[(N > 0 ? N : 1) * 4];
    for (int64_t b = 0; b < B; ++b) {
        for (int n = 0; n < N; ++n) {
            const double* c = world + (b * N + n) * 4;
            sp[n * 4] = c[0], sp[n * 4 + 1] = c[1], sp[n * 4 + 2] = c[2], sp[n * 4 + 3] = c[3] + (pad ? pad[b * 10 + link[n]] : 0.0);
        }
        clear_best best[256];
        for (int t = 0; t < 256; ++t) {
            best[t] = clear_none();
            for (int i = 0; i + 1 < N; ++i)
                for (int j = i + 1 + t; j < N; j += 256)
                    if (pairs[link[i] * 10 + link[j]]) clear_take(best[t], clear_gap(sp + i * 4, sp + j * 4), i, j);
        }
        clear_best m = clear_none();
        for (int w = 0; w < 4; ++w) butterfly(best + 64 * w), clear_take(m, best[64 * w].v, best[64 * w].a, best[64 * w].b);
        out[b] = m.v, wi[b] = m.a, wj[b] = m.b;
    }
    delete[] sp;
}
"""


def _host_lib(tmp_path):
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    return KB.host_harness(_HOST_HARNESS, tmp_path, {
        "host_sphere_clearance": (C.c_int64, [vp, i, vp, i, vp, C.c_int64, vp, vp, i, vp, vp, vp, i, vp, d, i, vp, vp, vp, vp, vp, vp, vp]),
        "host_self_clearance": (None, [vp, i, vp, i, vp, vp, vp, vp, vp])})


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host_sphere(lib, c, cull, pad="own"):
    """-> (the six outputs, world, the skips)."""
    pad = c["pad"] if isinstance(pad, str) else pad
    objects, begin, pool = np.ascontiguousarray(c["objects"]), np.ascontiguousarray(c["begin"], np.int32), np.ascontiguousarray(c["pool"], np.float32)
    cfg, poses, local = np.ascontiguousarray(c["cfg"], np.int32), np.ascontiguousarray(c["poses"], np.float64), np.ascontiguousarray(c["local"], np.float64)
    link = np.ascontiguousarray(c["link"], np.int32)
    vis = None if c.get("visible") is None else np.ascontiguousarray(c["visible"], np.uint8)
    B, N = len(cfg), len(link)
    out = [np.full(B, -77.25), np.full(B, -5, np.int32), np.full(B, -5, np.int32)]
    out += [np.full(B, -77.25), np.full(B, -5, np.int32), np.full(B, -5, np.int32)] if pad is not None else [None, None, None]
    world = np.full((B, N, 4), -77.25)
    skips = lib.host_sphere_clearance(_p(objects), len(objects), _p(begin), len(begin) - 1, _p(pool), pool.size, _p(vis), _p(cfg), B, _p(poses), _p(local),
                                      _p(link), N, _p(pad), float(c["beyond"]), int(cull), *[_p(x) for x in out], _p(world))
    return tuple(out), world, skips


def host_self(lib, world, link, pairs, pad):
    world, link = np.ascontiguousarray(world, np.float64), np.ascontiguousarray(link, np.int32)
    pairs = np.ascontiguousarray(pairs, np.uint8)
    B, N = world.shape[:2]
    out, wi, wj = np.full(B, -77.25), np.full(B, -5, np.int32), np.full(B, -5, np.int32)
    lib.host_self_clearance(_p(world), B, _p(link), N, _p(pairs), _p(pad), _p(out), _p(wi), _p(wj))
    return out, wi, wj


@KB.requires_host_cxx
def test_kernel_body_compiled_for_the_host_equals_the_specification(tmp_path):
    """csrc/omg_clearance_body.h is what a lane of the two kernels does for its sphere, its pair and its merge; compiled for the
    host without contraction and walked in the kernels' order it gives the specification's bits: on the edge cases; on N in
    {0, 1, 63, 64, 65, 257} x B in {1, 4, 5, 17} x S in {1, 3} over volumes of (2,2,2), (5,9,7), (33,17,9) in a ragged pool with
    NaN between them, a scene without objects, a disabled and an invisible record; with the cull on and off.  The cull does skip
    something: otherwise it proves nothing."""
    from omg_planner_amd import _lib
    assert _lib.CONSTANTS["OMGX_ROBOT_SPHERE_CHUNK"] == 256 and _lib.CONSTANTS["OMGX_CLEARANCE_MAX_SELF"] == 1024
    lib = _host_lib(tmp_path)
    objects, begin, pool, launches = CC.edge_launch()
    for L in launches:
        for cull in (0, 1):
            got, world, _ = host_sphere(lib, dict(L, objects=objects, begin=begin, pool=pool), cull)
            assert tuple(None if x is None else x[0].item() for x in got) == L["want"] and CC.same(world[0], L["local"]), (L["what"], cull)
    skipped, reached, nobody, objects_won = 0, 0, 0, set()
    for key in CC.BATCHES:
        c = CC.batch(*key)
        for cull in (0, 1):
            got, world, skips = host_sphere(lib, c, cull)
            assert CC.same_results(got, c["want"]) and CC.same(world, c["world"]), (key, cull)
            assert cull or skips == 0
            skipped += skips
        got, _, _ = host_sphere(lib, c, 1, pad=None)  # without pads: no margin, the same clear
        assert CC.same_results(got, c["want"][:3] + (None, None, None)), key
        reached += int((c["want"][1] >= 0).sum())
        nobody += int((c["want"][1] < 0).sum())
        objects_won |= set(c["want"][2].tolist())
        if key[0]:  # the margin is never above the clearance, and somewhere the pads move the argmin
            assert (c["want"][3] <= c["want"][0]).all()
    moved = sum(int((CC.batch(*k)["want"][1] != CC.batch(*k)["want"][4]).sum()) for k in CC.BATCHES)
    print("skips", skipped, "configurations with an answer", reached, "without", nobody, "objects that won", sorted(objects_won), "argmin moved by pads", moved)
    assert skipped > 100 and reached > 100 and nobody > 20 and objects_won >= {-1, 0, 1, 2} and moved > 0
    for what, sph, links, pairs, pad, want in CC.SELF_CASES:
        got = host_self(lib, np.array([sph], np.float64), links, pairs, None if pad is None else np.array([pad]))
        assert tuple(x[0].item() for x in got) == want, what
    for N in CC.SELF_N:
        c = CC.self_batch(N)
        assert CC.same_results(host_self(lib, c["world"], c["link"], c["pairs"], c["pad"]), c["want"]), N
        assert CC.same_results(host_self(lib, c["world"], c["link"], c["pairs"], None), c["want_bare"]), N
        assert N < 65 or ((c["want"][1] >= 0).all() and (c["want"][0] < c["want_bare"][0]).all())


@KB.requires_host_cxx
def test_fuzz_generator_against_the_body_compiled_for_the_host(tmp_path):
    """The draws of the GPU test's seed through the body header on the host equal the specification, and between them they reach
    no sphere and more than a wave of them, both culls, scenes without objects, pads and none, and voxels that are not finite."""
    lib = _host_lib(tmp_path)
    rng = np.random.default_rng(CC.FUZZ_SEED)
    counts, culls, empty, bare, odd, answers = set(), set(), 0, 0, 0, 0
    for _ in range(CC.FUZZ_TRIALS):
        c = CC.draw(rng)
        world, want, want_self = CC.specification(c)
        got, got_world, _ = host_sphere(lib, c, c["cull"])
        assert CC.same_results(got, want) and CC.same(got_world, world), (c["N"], c["B"], c["S"])
        if c["N"] <= 1024:
            assert CC.same_results(host_self(lib, world, c["link"], c["pairs"], c["pad"]), want_self)
        counts.add(c["N"]), culls.add(c["cull"])
        empty += int((np.diff(c["begin"]) == 0).sum())
        bare += c["pad"] is None
        odd += int((~np.isfinite(c["pool"])).sum())
        answers += int((want[1] >= 0).sum())
    print("sphere counts", sorted(counts), "empty scenes", empty, "trials without pads", bare, "voxels not finite", odd, "answers", answers)
    assert min(counts) <= 1 and max(counts) > 256 and len(counts) > 8 and culls == {0, 1} and empty > 0 and 0 < bare < CC.FUZZ_TRIALS and odd > 100 and answers > 50


# ---------------------------------------------------------------------------------------------------------------------
# 3. the reach table
# ---------------------------------------------------------------------------------------------------------------------
def test_reach_table_bounds_the_path_of_every_centre():
    """Over 300 seeded linear joint-space segments inside the joint limits, with 15 random centres per link within 8 cm: the
    length of each centre's path over 33 samples (oracle.fk) is at most len_l = sum_j rho[l][j] * |dq_j|.  A condition, not a
    measurement; the largest ratio is printed."""
    from omg_planner_amd import clearance as cl, robot as rb
    from oracle import oracle as orc
    model = rb.PandaModel(seed=0)
    rng = np.random.default_rng(7)
    lo, hi = model.joint_lower_limit[0], model.joint_upper_limit[0]
    local = np.concatenate([rng.uniform(-0.08, 0.08, (150, 3)), np.zeros((150, 1))], 1)
    link = np.repeat(np.arange(10), 15)
    travel = float(max(abs(lo[7:]).max(), abs(hi[7:]).max()))
    rho = cl.reach_table(model, local, link, travel)
    assert rho.shape == (10, 9) and (rho >= 0).all() and rho[8, 7] == 1.0 and rho[9, 8] == 1.0
    assert all(rho[l, j] == 0 for l in range(10) for j in range(9) if (j <= 6 and j > min(l, 6)) or (j == 7 and l != 8) or (j == 8 and l != 9))
    a, b = rng.uniform(lo, hi, (300, 9)), rng.uniform(lo, hi, (300, 9))
    single = rng.integers(0, 9, 100)  # the first 100: one joint alone (the bound is tight by construction)
    for k in range(100):
        keep = b[k, single[k]]
        b[k] = a[k]
        b[k, single[k]] = keep
    w = np.linspace(0.0, 1.0, 33)
    q = a[:, None, :] + (b - a)[:, None, :] * w[None, :, None]  # [300,33,9]
    poses = orc.fk(model.blob(), q.reshape(-1, 9))[0]
    world = cl.world_spheres(poses, local, link)[:, :, :3].reshape(300, 33, 150, 3)
    path = np.linalg.norm(np.diff(world, axis=1), axis=3).sum(axis=1)  # [300,150]
    bound = (np.abs(b - a) @ rho.T)[:, link]  # [300,150]
    ratio = path / np.maximum(bound, 1e-300)
    print("largest path / bound", ratio.max(), "per link", np.round(ratio.reshape(300, 10, 15).max(axis=(0, 2)), 5))
    assert (path <= bound * (1 + 1e-12)).all()
    assert ratio.max() > 0.9  # the bound is not idle
    for bad in (dict(finger_travel=NAN), dict(finger_travel=-0.01), dict(link=link[:5]), dict(local=np.full((150, 4), NAN))):
        with pytest.raises(ValueError):
            cl.reach_table(**{**dict(model=model, local=local, link=link, finger_travel=travel), **bad})


# ---------------------------------------------------------------------------------------------------------------------
# 4. tunnelling
# ---------------------------------------------------------------------------------------------------------------------
def test_a_plate_between_two_waypoints_by_the_specification_alone():
    """A 2 cm plate on a 1 cm grid stands in the plane the hand sweeps through while joint 0 turns by 1 rad between two waypoints;
    a sphere of 2 cm sits at the hand's frame.  K = 1: no sample collides (CHOMP's own evidence says free) and the segment is not
    certified.  K = 16: collides, first_hit strictly inside.  The same motion with the plate lifted 15 cm (9 cm clear of its
    edge): not certified at K = 1, certified at K = 16, and never colliding."""
    k_few, k_many = CC.PLATE_K
    few, _ = CC.plate_report(k_few)
    many, out = CC.plate_report(k_many)
    print("K", k_few, {k: v.tolist() for k, v in few.items() if k != "half"})
    print("K", k_many, {k: v.tolist() for k, v in many.items() if k != "half"})
    assert few["collides"].tolist() == [False, False] and few["certified"].tolist() == [[False], [False]] and (few["min_clearance"] > 0.03).all()
    assert many["collides"].tolist() == [True, False] and 0 < many["first_hit"][0] < k_many and many["first_hit"][1] == -1
    assert many["certified"].tolist() == [[False], [True]] and many["plan_certified"].tolist() == [False, True]
    assert many["min_clearance"][0] < -0.02 and many["segment_margin"][0, 0] < 0 < many["segment_margin"][1, 0]
    assert (out[2].reshape(2, -1) == 0).all() and (out[1].reshape(2, -1) == 0).all()  # the one sphere, the one object


# ---------------------------------------------------------------------------------------------------------------------
# 5. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_specification_argument_errors():
    from omg_planner_amd import clearance as cl
    objects, begin, pool, _ = CC.table(3)
    world = np.zeros((2, 3, 4))
    good = dict(objects=objects, scene_begin=begin, pool=pool, visible=None, scene_of_config=[0, 2], world=world, link=[0, 5, 9], pad=None, beyond=0.1)
    assert cl.sphere_clearance(**good)[3] is None
    short, neg_r, nan_r = objects.copy(), world.copy(), world.copy()
    short["dim"][1] = (5, 1, 7)
    neg_r[1, 2, 3], nan_r[0, 0, 3] = -0.1, NAN
    out_of_pool, bad_delta = objects.copy(), objects.copy()
    out_of_pool["grid_offset"][2], bad_delta["inv_delta"][0] = pool.size - 10, NAN
    for change in (dict(beyond=NAN), dict(beyond=-0.1), dict(beyond=INF), dict(scene_of_config=[0, 3]), dict(scene_of_config=[-1, 0]),
                   dict(scene_of_config=[0]), dict(link=[0, 5, 10]), dict(link=[0, 5]), dict(link=[-1, 0, 0]), dict(world=world[:, :, :3]),
                   dict(world=neg_r), dict(world=nan_r), dict(pad=np.zeros((2, 9))), dict(pad=np.zeros((3, 10))), dict(visible=[1, 1, 1]),
                   dict(scene_begin=[0, 3, 2, 5]), dict(scene_begin=[0, 3, 3, 6]), dict(scene_begin=[-1, 3, 3, 5]), dict(objects=short),
                   dict(objects=out_of_pool), dict(objects=bad_delta), dict(objects=np.zeros(5)), dict(pool=pool.astype(np.float64))):
        with pytest.raises(ValueError):
            cl.sphere_clearance(**{**good, **change})
    # what is not used is not looked at: the broken record invisible
    assert cl.sphere_clearance(**{**good, **dict(objects=short, visible=[1, 0, 1, 1, 1])})[0].shape == (2,)
    for change in (dict(link=[0, 1]), dict(link=[0, 1, 10]), dict(pairs=np.ones((9, 10))), dict(pad=np.zeros((2, 9))), dict(world=np.zeros((1, 1025, 4)), link=[0] * 1025)):
        with pytest.raises(ValueError):
            cl.self_clearance(**{**dict(world=world, link=[0, 1, 2], pairs=np.ones((10, 10)), pad=None), **change})
    with pytest.raises(ValueError):
        cl.plan_report(np.zeros((1, 3, 9)), 2, np.zeros((10, 9)), 0.0, 0.0, 0.1, np.zeros((1, 4)), np.zeros((1, 5)))
    with pytest.raises(ValueError):
        cl.segment_halves(np.zeros((1, 3, 9)), 2, np.zeros((9, 10)))


def test_c_abi_argument_checks_without_gpu():
    """Every OMGX_ERR_INVALID / OMGX_ERR_UNSUPPORTED case of the two entry points is decided on the host copies before any HIP
    call: the device pointers below are never dereferenced."""
    from omg_planner_amd import _lib
    lib = _lib.lib()
    assert lib.omgx_abi_version() == 14 and len(_lib.STRUCTS) == 8
    INV, UNS, OK = _lib.OMGX_ERR_INVALID, _lib.OMGX_ERR_UNSUPPORTED, _lib.OMGX_OK
    d = C.c_void_p(4096)
    objects0, begin0, pool0, _ = CC.table(3)

    def sphere(objects=objects0, begin=begin0, pool_elems=pool0.size, flags=None, cfg=(0, 1, 2, 2), spheres=((0.0, 0.0, 0.1, 0.05),) * 3, links=(0, 4, 9),
               beyond=0.1, n=None, S=None, B=None, N=None, margins=True, **ptr):
        objects, begin = np.ascontiguousarray(objects), np.ascontiguousarray(begin, np.int32)
        cfg, local, link = np.ascontiguousarray(cfg, np.int32), np.ascontiguousarray(spheres, np.float64), np.ascontiguousarray(links, np.int32)
        vis = None if flags is None else np.ascontiguousarray(flags, np.uint8)
        m = d if margins else None
        p = dict(objects=d, scene_begin=d, pool=d, visible=None if vis is None else d, scene_of_config=d, link_poses=d, local=d, link=d, pad=m, clear=d,
                 clear_sphere=d, clear_object=d, margin=m, margin_sphere=m, margin_object=m, world_out=d, h_objects=_p(objects), h_scene_begin=_p(begin),
                 h_visible=_p(vis), h_scene_of_config=_p(cfg), h_local=_p(local), h_link=_p(link))
        p.update(ptr)
        return lib.omgx_sphere_clearance(p["objects"], p["h_objects"], len(objects) if n is None else n, p["scene_begin"], p["h_scene_begin"],
                                         len(begin) - 1 if S is None else S, p["pool"], pool_elems, p["visible"], p["h_visible"], p["scene_of_config"],
                                         p["h_scene_of_config"], len(cfg) if B is None else B, p["link_poses"], p["local"], p["h_local"], p["link"],
                                         p["h_link"], len(link) if N is None else N, p["pad"], beyond, 1, p["clear"], p["clear_sphere"], p["clear_object"],
                                         p["margin"], p["margin_sphere"], p["margin_object"], p["world_out"], None)

    for k in ("objects", "h_objects", "scene_begin", "h_scene_begin", "pool", "scene_of_config", "h_scene_of_config", "link_poses", "local", "h_local", "link",
              "h_link", "clear", "clear_sphere", "clear_object", "pad", "margin", "margin_sphere", "margin_object"):
        assert sphere(**{k: None}) == INV, k
    assert sphere(flags=[1] * 5, h_visible=None) == INV and sphere(flags=[1] * 5, visible=None) == INV  # both or neither
    assert sphere(margins=False, margin=d) == INV and sphere(margins=False, pad=d) == INV
    assert sphere(B=0) == OK and sphere(B=0, scene_of_config=None, h_scene_of_config=None, link_poses=None, clear=None, clear_sphere=None, clear_object=None) == OK
    assert sphere(B=0, beyond=NAN) == INV  # refused even when nothing would run
    assert sphere(n=-1) == INV and sphere(S=-1) == INV and sphere(B=-1) == INV and sphere(N=-1) == INV and sphere(pool_elems=-1) == INV
    for bad in (NAN, INF, -INF, -0.5):
        assert sphere(beyond=bad) == INV, bad
    for col in range(4):
        for bad in (NAN, INF) + ((-1.0,) if col == 3 else ()):
            s = np.array([(0.0, 0.0, 0.1, 0.05)] * 3)
            s[2, col] = bad
            assert sphere(spheres=s) == INV, (col, bad)
    assert sphere(links=(0, 4, 10)) == INV and sphere(links=(-1, 4, 9)) == INV
    assert sphere(cfg=(0, 3)) == INV and sphere(cfg=(-1, 0)) == INV and sphere(S=0, B=1) == INV
    assert sphere(begin=(0, 3, 2, 5)) == INV and sphere(begin=(0, 3, 3, 6)) == INV and sphere(begin=(-1, 3, 3, 5)) == INV
    for field, value, index in (("dim", (1, 9, 7), 1), ("inv_delta", 0.0, 0), ("inv_delta", NAN, 2), ("inv_delta", INF, 2), ("inv_delta", -1.0, 4),
                                ("grid_offset", -1, 0), ("grid_offset", pool0.size - 10, 2)):
        bad = objects0.copy()
        bad[field][index] = value
        assert sphere(objects=bad) == INV, (field, value)
        assert sphere(objects=bad, flags=[k != index for k in range(5)], B=0) == OK and sphere(objects=bad, begin=(0, 0, 0, 0), B=0) == OK  # not used: not looked at
        assert sphere(objects=bad, B=0) == INV
    bad = objects0.copy()
    bad["dim"][3] = (0, 0, 0)  # the disabled record: used only when the flags say so
    assert sphere(objects=bad, B=0) == OK and sphere(objects=bad, flags=[1] * 5, B=0) == INV
    assert sphere(pool_elems=int(objects0["grid_offset"].max())) == INV
    many = _lib.CONSTANTS["OMGX_ROBOT_MAX_SPHERES"] + 1
    assert sphere(spheres=np.tile((0.0, 0.0, 0.1, 0.05), (many, 1)), links=np.zeros(many, np.int32)) == UNS
    assert sphere(spheres=np.tile((0.0, 0.0, 0.1, -0.05), (many, 1)), links=np.zeros(many, np.int32)) == INV  # limits after every invalid argument

    def own(links=(0, 4, 9), B=2, N=None, **ptr):
        link = np.ascontiguousarray(links, np.int32)
        p = dict(world=d, link=d, h_link=_p(link), pairs=d, pad=d, self_clear=d, sphere_i=d, sphere_j=d)
        p.update(ptr)
        return lib.omgx_self_clearance(p["world"], B, p["link"], p["h_link"], len(link) if N is None else N, p["pairs"], p["pad"], p["self_clear"],
                                       p["sphere_i"], p["sphere_j"], None)

    for k in ("world", "link", "h_link", "pairs", "self_clear", "sphere_i", "sphere_j"):
        assert own(**{k: None}) == INV, k
    assert own(B=0) == OK and own(B=0, world=None, pairs=None, self_clear=None, sphere_i=None, sphere_j=None) == OK
    assert own(B=-1) == INV and own(N=-1) == INV and own(links=(0, 10, 1)) == INV and own(links=(0, -1, 1)) == INV
    assert own(links=np.zeros(1025, np.int32)) == UNS and own(links=np.full(1025, 10, np.int32)) == INV and own(links=np.zeros(1025, np.int32), B=0) == UNS


def test_wrapper_checks_without_gpu():
    """The wrappers' own refusals come before anything touches a device."""
    import inspect
    import torch
    from omg_planner_amd import _lib, ops, pipeline
    E = _lib.OmgHipError
    with pytest.raises(E, match=r"\[S,n,9\]"):
        ops.dense_configs(torch.zeros((2, 3, 8), dtype=torch.float64), 2)
    with pytest.raises(E, match=">= 1"):
        ops.dense_configs(torch.zeros((2, 3, 9), dtype=torch.float64), 0)
    q = ops.dense_configs(torch.arange(54, dtype=torch.float64).reshape(2, 3, 9), 4)  # plain tensor operators: the host will do
    from omg_planner_amd import clearance as cl
    assert CC.same(q.numpy(), cl.dense_configs(np.arange(54.0).reshape(2, 3, 9), 4))
    s = ops.RobotSpheres([(0.0, 0.0, 0.0, 0.01)] * 2, [0, 7], device="cpu")
    with pytest.raises(E, match="device tensor"):
        ops.self_clearance(torch.zeros((1, 2, 4), dtype=torch.float64), s, np.ones((10, 10)))
    pairs = ops.default_self_pairs()
    assert pairs.shape == (10, 10) and (pairs == pairs.T).all() and not pairs.diagonal().any() and pairs[0, 2] and not pairs[0, 1]
    assert not pairs[8, 9] and ops.default_self_pairs(False)[8, 9] and not pairs[6, 7] and not pairs[7, 8] and pairs[5, 7] and pairs[3, 9]
    from omg_planner_amd import robot as rb
    rho = s.reach_table(rb.PandaModel(seed=0))
    assert rho.shape == (10, 9) and s.rho is rho
    sig = inspect.signature(ops.DeviceScenes.plan_clearance).parameters
    assert (sig["slack"].default, sig["beyond"].default, sig["visible"].default, sig["pairs"].default, sig["rho"].default) == (0.0, 0.1, None, None, None)
    sig = inspect.signature(pipeline.check_plans).parameters
    assert sig["skip_targets"].default is True and sig["fingers_touch"].default is True
    sig = inspect.signature(ops.sphere_clearance).parameters
    assert (sig["visible"].default, sig["pad"].default, sig["beyond"].default, sig["cull"].default, sig["want_world"].default) == (None, None, 0.1, True, False)


# ---------------------------------------------------------------------------------------------------------------------
# 6. registers
# ---------------------------------------------------------------------------------------------------------------------
@KB.requires_hipcc
def test_clearance_kernels_do_not_spill(tmp_path):
    """The compiler's resource remarks for csrc/omg_clearance.hip: neither kernel uses scratch or spills.  Registers, LDS and
    occupancy are printed, not pinned (the LDS is the staged chunk, and the self op's spheres: 32 KB and their links)."""
    seen = KB.kernel_resources("omg_clearance.hip", tmp_path)
    assert len(seen) == 2
    for part in ("k_sphere_clearance", "k_self_clearance"):
        v = KB.one(seen, part)
        print(part, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (part, v)
