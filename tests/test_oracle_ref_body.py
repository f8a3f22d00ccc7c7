"""CPU test: the oracle's SDF op against THE REFERENCE'S OWN kernel body — layers/sdf_matching_loss_kernel.cu:96-195
(SDFdistanceForward and sum_gradients, with the helpers of lines 15-86 and the loop macro of 11-13), cut out of the reference
tree at build time and compiled for the host behind oracle/ref_body_wrapper.cpp by `make -C oracle ref` into
oracle/_ref/libsdf_ref_body.so.  What that library returns on this module's seeded inputs is stored in
tests/golden/ref_sdf_body.npz (`PYTHONPATH=. python tests/test_oracle_ref_body.py` records it): the oracle is checked against
the stored outputs bit for bit, and wherever oracle/_ref is built the live library must reproduce them bit for bit.

This pins the body's text: every index, cast, literal promotion, comparison, branch, `continue` and operand order.  It cannot
pin Eigen's and Sophus' own arithmetic (restated in the wrapper's two modes: the float32 matrix product the kernels use, and
the quaternion round trip of the oracle's SOPHUS MODE), what nvcc would contract inside them, or the atomic reduction order.

The inputs are ones on which the reference text has defined behaviour: finite points whose grid coordinates stay far inside
the int range of the casts at .cu:39-41.  NaN, inf and 3e9 stay with tests/test_gpu_parity.py (oracle against kernel only).

The stored file holds outputs and a SHA-256 of each block's regenerated input bytes, not the inputs.  The quaternion-mode
outputs are stored as the XOR of their bits with the matrix-mode outputs (mostly zero: it compresses)."""
import ctypes as C
import hashlib
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as orc

REF_LIB = Path(__file__).resolve().parents[1] / "oracle" / "_ref" / "libsdf_ref_body.so"
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_sdf_body.npz"
MODES = {"matrix": 0, "quaternion": 1}
F32 = np.float32
ARG_NAMES = ("pose", "grids", "lim", "pts", "eps", "pad", "clr", "dis")


# ------------------------------------------------------------------------------------------------
# the reference body, live
# ------------------------------------------------------------------------------------------------
def load_ref():
    """The reference's kernel body built into oracle/_ref, or None where it is not built (no reference tree)."""
    if not REF_LIB.exists():
        return None
    lib = C.CDLL(str(REF_LIB))
    lib.ref_sdf_loss_forward.restype = C.c_int
    lib.ref_sdf_loss_forward.argtypes = [C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_int] + [C.c_void_p] * 6
    lib.ref_quaternion_branch.restype = C.c_int
    lib.ref_quaternion_branch.argtypes = [C.c_void_p]
    return lib


def run_ref(lib, mode, pose, grids, lim, pts, eps, pad, clr, dis):
    """-> potentials [N], gradients [N,3], collides [N], and the per-pair arrays [N,O], [N,O,3], [N,O] (float32)."""
    a = [np.ascontiguousarray(x, F32) for x in (pose, grids, lim, pts, eps, pad, clr, dis)]
    N, O = len(a[3]), len(a[0])
    # filled with a marker: the entry itself must zero them like at::zeros (.cu:225-231)
    out = [np.full(s, 7.0, F32) for s in ((N,), (N, 3), (N,), (N, O), (N, O, 3), (N, O))]
    rc = lib.ref_sdf_loss_forward(MODES[mode], *[x.ctypes.data_as(C.c_void_p) for x in a], N, O, *[x.ctypes.data_as(C.c_void_p) for x in out])
    assert rc == 0
    return tuple(out)


def ref_single_object_sum(lib, mode, objs, pts):
    """The in-object-order float32 sum of single-object reference-body calls — one call per object with its OWN grid, since
    one call cannot take unequal dims.  objs: (pose [4,4], grid [X,Y,Z], limits [10], eps, pad, clr, disabled) per object.
    The per-pair outputs are added to +0 in object order, exactly what the launcher's reduction does (.cu:248-258)."""
    N = len(pts)
    acc = [np.zeros(N, F32), np.zeros((N, 3), F32), np.zeros(N, F32)]
    for pose, grid, lim, eps, pad, clr, dis in objs:
        one = run_ref(lib, mode, pose[None], grid[None], lim[None], pts, [eps], [pad], [clr], [dis])
        acc = [x + y for x, y in zip(acc, one[:3])]
    return acc


# ------------------------------------------------------------------------------------------------
# seeded inputs: named blocks
# ------------------------------------------------------------------------------------------------
def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _axis_angle(axis, th):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _pose(R=np.eye(3), t=(0, 0, 0)):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T.astype(F32)


def _pose_about(lim, R, dt):
    """A pose that turns the world about the centre c of the volume `lim`: u = R (p - c) + c + dt, so the rotated volume stays
    where the points are."""
    c = 0.5 * (lim[0:3].astype(np.float64) + lim[3:6].astype(np.float64))
    return _pose(R, c - R @ c + dt)


def _limits(lo, extent, dims, delta):
    lo = np.asarray(lo, F32)
    return np.array([*lo, *(lo + np.asarray(extent, F32)), *dims, delta], F32)


def grid_coords(lim, pts):
    """Grid coordinates (.cu:140-142) of object-frame points, in numpy float32 — the test's own statement of the expression."""
    lo, hi, d = lim[0:3].astype(F32), lim[3:6].astype(F32), lim[6:9].astype(np.int32).astype(F32)
    return (pts.astype(F32) - lo) / (hi - lo) * d


def _face_points(lim, dims, rng):
    """Object-frame points (identity pose) that walk every axis across the places where the lookup changes its mind: grid
    coordinate 0.5 (first voxel centre), d - 0.5 (last centre: x1 leaves the range), d - 1.5; 13 neighbouring float32 values
    around each, so that the exact value (where float32 reaches it) and both sides are met; inside (-0.5, 0.5), where the cast
    truncates toward zero and the cell is in range with a negative weight; and up to one voxel outside, where only some of the
    central-difference neighbours are in range.  The other two coordinates sit at generic places inside the volume."""
    lo, hi = lim[0:3].astype(np.float64), lim[3:6].astype(np.float64)
    out = []
    for ax in range(3):
        d = dims[ax]
        targets = [0.5, d - 0.5, d - 1.5, 1.5, -0.5, d + 0.5, -0.45, -0.2, 0.0, 0.2, 0.45, 0.7, 1.2, -0.7, -1.2, -1.6, d - 1.2, d - 0.7, d - 0.2,
                   d + 0.3, d + 0.7]
        for k, g in enumerate(targets):
            base = rng.uniform(1.6, np.array(dims) - 1.6)  # generic interior grid coordinates of the other two axes
            p = (lo + base / np.array(dims) * (hi - lo)).astype(F32)
            c = F32(lo[ax] + g / d * (hi[ax] - lo[ax]))
            walk = [c]
            if k < 6:  # 0, +-1 .. 4, +-8, +-16 float32 steps: a step of p is a fraction of a step of the grid coordinate
                for n in (-16, -8, -4, -3, -2, -1, 1, 2, 3, 4, 8, 16):
                    walk.append((c.view(np.int32) + np.int32(n if c > 0 else -n)).view(F32))
            for v in walk:
                q = p.copy()
                q[ax] = v
                out.append(q)
    # corners: every axis near a face at once
    for sx in (0.2, dims[0] - 0.2, -0.7):
        for sy in (0.45, dims[1] - 1.2, dims[1] + 0.3):
            for sz in (0.0, dims[2] - 0.7, -1.2):
                out.append((lo + np.array([sx, sy, sz]) / np.array(dims) * (hi - lo)).astype(F32))
    return np.array(out, F32)


def _box_points(lim, rng, n, grow=0.35):
    lo, hi = lim[0:3].astype(np.float64), lim[3:6].astype(np.float64)
    return rng.uniform(lo - grow * (hi - lo), hi + grow * (hi - lo), size=(n, 3)).astype(F32)


def _one_volume(dims, rng, delta=None):
    """Limits whose extent is no power of two (so (u - lo) / (hi - lo) * d rounds) and a rough random volume."""
    ext = np.array(dims) * np.array([0.0117, 0.0093, 0.0131])
    lim = _limits([-0.0713, -0.1191, 0.0377], ext, dims, 0.0117 if delta is None else delta)
    return lim, rng.normal(0.05, 0.1, size=dims).astype(F32)


def _exact_face_points(dims, rng):
    """Points for a volume with lo = 0 and a voxel of 2^-6: p = g / 64 is exact, and fl(fl(g / d) * d) == g, so the grid
    coordinates 0.5, d - 0.5 and d - 1.5 are met EXACTLY; one float32 either side of each as well."""
    out = []
    for ax in range(3):
        for g in (0.5, dims[ax] - 0.5, dims[ax] - 1.5):
            c = F32(g / 64.0)
            for v in (np.nextafter(c, F32(-1)), c, np.nextafter(c, F32(9))):
                q = (rng.uniform(1.6, np.array(dims) - 1.6) / 64.0).astype(F32)
                q[ax] = v
                out.append(q)
    return np.array(out, F32)


def _faces_block(seed, dims, delta):
    rng = np.random.RandomState(seed)
    lim, grid = _one_volume(dims, rng, delta)
    lim_exact = _limits([0, 0, 0], np.array(dims) / 64.0, dims, delta)
    pts = np.concatenate([_face_points(lim, dims, rng), _exact_face_points(dims, rng)])
    # object 0: identity pose, the points are object-frame coordinates exactly.  Object 1: the same volume rotated and shifted
    # (the faces are then met at rounded places).  Object 2: epsilon >= 1, the out-of-range 1.0 is inside the hinge.
    # Object 3: identity pose and limits in which the faces' grid coordinates are exact (_exact_face_points).
    pose = np.stack([_pose(), _pose_about(lim, _rot(rng), rng.uniform(-0.01, 0.01, 3)), _pose(), _pose()])
    return dict(pose=pose, grids=np.stack([grid] * 4), lim=np.stack([lim] * 3 + [lim_exact]), pts=pts, eps=F32([0.2, 0.15, 1.5, 0.25]),
                pad=F32([1.0, 2.5, 0.75, 1.0]), clr=F32([0.01, 0.0, 0.02, 0.01]), dis=F32([0, 0, 0, 0]))


def _const_block(seed, value, eps, pad, clr):
    """Constant volumes: the interpolated value equals the constant wherever every weight is in [0, 1] ..."""
    rng = np.random.RandomState(seed)
    dims = (5, 24, 6)
    lim, _ = _one_volume(dims, rng)
    O = len(eps)
    grids = np.stack([np.full(dims, v, F32) for v in np.broadcast_to(F32(value), (O,))])
    pts = np.concatenate([_face_points(lim, dims, rng), _box_points(lim, rng, 300), _box_points(lim, rng, 100, grow=-0.33)])
    pose = np.stack([_pose()] + [_pose_about(lim, _rot(rng), rng.uniform(-0.01, 0.01, 3)) for _ in range(O - 1)])
    return dict(pose=pose, grids=grids, lim=np.stack([lim] * O), pts=pts, eps=F32(eps), pad=F32(pad), clr=F32(clr), dis=np.zeros(O, F32))


def _params_block(seed):
    rng = np.random.RandomState(seed)
    dims = (9, 7, 11)
    lim, _ = _one_volume(dims, rng, delta=0.031)  # delta different from the voxel size
    eps = F32([1e-6, 0.0, -0.1, 1.0, 2.5, 0.2, 0.2, 0.2, 0.2, 0.2, 0.3])
    pad = F32([1.0, 2.0, 3.0, 0.5, 1.5, 0.0, 1e4, 1.0, 1.0, 1.0, 1.0])
    dis = F32([0, 0, 0, 0, 0, 0, 0, -1.0, 0.5, 1.0, 0.0])  # the test is `> 0`: -1 and 0 are enabled, 0.5 and 1 disabled
    clr = F32([0.01, 0.0, -0.05, 0.3, 1.5, 0.01, 0.01, 0.01, 0.01, 0.01, -0.02])
    O = len(eps)
    grids = rng.normal(0.03, 0.08, size=(O, *dims)).astype(F32)
    pose = np.stack([_pose()] + [_pose_about(lim, _rot(rng), rng.uniform(-0.01, 0.01, 3)) for _ in range(O - 1)])
    pts = np.concatenate([_face_points(lim, dims, rng), _box_points(lim, rng, 400)])
    return dict(pose=pose, grids=grids, lim=np.stack([lim] * O), pts=pts, eps=eps, pad=pad, clr=clr, dis=dis)


def _single_param_block(seed, eps, pad=1.0, clr=0.01):
    """One object, so that the per-point output shows one parameter's effect alone."""
    rng = np.random.RandomState(seed)
    dims = (9, 7, 11)
    lim, grid = _one_volume(dims, rng, delta=0.031)
    pts = np.concatenate([_face_points(lim, dims, rng), _box_points(lim, rng, 300)])
    return dict(pose=_pose_about(lim, _rot(rng), rng.uniform(-0.01, 0.01, 3))[None], grids=grid[None], lim=lim[None], pts=pts, eps=F32([eps]), pad=F32([pad]),
                clr=F32([clr]), dis=F32([0]))


POSE_BRANCHES = (0, 1, 2, 0, 1, 2, 3, 3, 3, 0)  # branch of Eigen's matrix -> quaternion assignment per object: 3 = trace > 0, else pivot


def _poses_block(seed, fourth_row=False):
    rng = np.random.RandomState(seed)
    dims = (9, 7, 11)
    lim, _ = _one_volume(dims, rng)
    Rs = [np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1]),       # half turns about x, y, z
          _axis_angle([1, 0.02, -0.03], np.pi - 0.01), _axis_angle([0.01, 1, 0.02], np.pi - 0.02), _axis_angle([-0.02, 0.03, 1], np.pi + 0.015),
          _rot(np.random.RandomState(11)), _axis_angle([1, 2, 3], 0.4), _axis_angle([0, 0, 1], 1.9),  # float32-rounded rotations, trace > 0
          _axis_angle([3, 1, 1], 2.2)]                                                     # 1 + 2 cos < 0: no half turn, pivot x
    O = len(Rs)
    pose = np.stack([_pose_about(lim, R, rng.uniform(-0.02, 0.02, 3)) for R in Rs])
    if fourth_row:  # never read beyond the constructor (.cu:121-126)
        pose[:, 3, :] = np.random.RandomState(seed + 1).uniform(-3, 3, size=(O, 4)).astype(F32)
    grids = rng.normal(0.04, 0.08, size=(O, *dims)).astype(F32)
    pts = _box_points(lim, rng, 700, grow=0.3)
    return dict(pose=pose, grids=grids, lim=np.stack([lim] * O), pts=pts, eps=np.full(O, 0.2, F32), pad=rng.uniform(0.5, 2, O).astype(F32),
                clr=np.full(O, 0.01, F32), dis=np.zeros(O, F32))


def _shape_block(O, N):
    rng = np.random.RandomState(1000 * O + N)
    dims = (6, 5, 7)
    lim, _ = _one_volume(dims, rng)
    pose = np.stack([_pose_about(lim, _rot(rng), rng.uniform(-0.01, 0.01, 3)) for _ in range(O)])
    return dict(pose=pose, grids=rng.normal(0.05, 0.1, size=(O, *dims)).astype(F32), lim=np.stack([lim] * O),
                pts=_box_points(lim, rng, N, grow=0.2), eps=rng.uniform(0.05, 0.3, O).astype(F32), pad=rng.uniform(0.5, 3, O).astype(F32),
                clr=rng.uniform(-0.02, 0.05, O).astype(F32), dis=(rng.uniform(size=O) < 0.2).astype(F32))


def _tabletop_block():
    """A few thousand random points through a tabletop-like arrangement, in the reference's padded layout."""
    from omg_planner_amd import scenes as sc
    from tests import helpers as H
    scene = sc.make_tabletop_scene(5, grid=16, table_grid=(24, 16, 8))
    for ob in scene.objects[:-1]:  # pulled together and sunk into the table: points inside two volumes at once
        ob.pose_mat[:3, 3] = [0.5 + 0.35 * (ob.pose_mat[0, 3] - 0.5), 0.35 * ob.pose_mat[1, 3], 0.07]
    grids, lim = sc.pack_padded(scene.objects)
    pose, eps, pad, clr, dis = sc.layer_params(scene, **H.LAYER_CFG)
    rng = np.random.RandomState(77)  # two thirds around the objects, one third through and beyond the table's volume
    pts = np.concatenate([rng.uniform([0.3, -0.2, -0.02], [0.7, 0.2, 0.2], size=(2000, 3)), rng.uniform([-0.5, -0.7, -0.4], [1.5, 0.7, 0.9], size=(1000, 3))]).astype(F32)
    return dict(pose=pose, grids=grids, lim=lim, pts=pts, eps=eps, pad=pad, clr=clr, dis=dis)


def blocks():
    """name -> inputs of the reference's op, in the order of ARG_NAMES."""
    b = {}
    b["faces_5_24_6"] = _faces_block(1, (5, 24, 6), 0.0117)
    b["faces_9_7_11"] = _faces_block(2, (9, 7, 11), 0.05)
    eps3, clr3 = [0.2, 0.1, 0.05], [0.01, 0.0, 0.02]
    b["const_zero"] = _const_block(3, 0.0, eps3, [2.0, 0.5, 3.0], clr3)                # value == 0: the `<= 0` branch
    b["const_epsilon"] = _const_block(4, eps3, eps3, [2.0, 0.5, 3.0], [0.01, 0.3, 0.02])  # value == eps: second branch, zero factor
    b["const_clearance"] = _const_block(5, [0.0075, 0.25, -0.5], [0.2, 0.2, 0.2], [1.0, 1.0, 1.0], [0.0075, 0.25, -0.5])  # value < clr is false
    b["negative_clearance"] = _single_param_block(6, eps=0.2, clr=-0.03)
    b["tiny_positive"] = _const_block(7, [1e-30, 1e-38, 1e-12], eps3, [3.0, 0.25, 7.0], clr3)  # just above 0: the potential jumps
    b["params"] = _params_block(8)
    b["epsilon_1e-6"] = _single_param_block(9, eps=1e-6)
    b["epsilon_zero"] = _single_param_block(10, eps=0.0, pad=2.0)
    b["epsilon_negative"] = _single_param_block(11, eps=-0.1, pad=2.0, clr=-0.05)
    b["epsilon_one"] = _single_param_block(12, eps=1.0, pad=0.5)
    b["epsilon_large"] = _single_param_block(13, eps=2.5, pad=1.5, clr=1.5)
    b["padding_zero"] = _single_param_block(14, eps=0.2, pad=0.0)
    b["padding_large"] = _single_param_block(15, eps=0.2, pad=1e4)
    b["delta_not_voxel"] = _single_param_block(16, eps=0.3)
    dis = _params_block(17)
    dis["dis"] = F32([1, 0.5, 2, 1e-30, 1, 1, 3, 1, 0.5, 1, 1])
    b["all_disabled"] = dis
    b["poses"] = _poses_block(18)
    b["poses_fourth_row"] = _poses_block(18, fourth_row=True)
    for O in (1, 5, 13, 41):
        for N in (1, 63, 65):
            b[f"shape_O{O}_N{N}"] = _shape_block(O, N)
    b["random_tabletop"] = _tabletop_block()
    return b


def args_of(blk):
    return [blk[k] for k in ARG_NAMES]


def input_hash(blk):
    h = hashlib.sha256()
    for k in ARG_NAMES:
        a = np.ascontiguousarray(blk[k], F32)
        h.update(k.encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------
# stored outputs
# ------------------------------------------------------------------------------------------------
OUT_NAMES = ("potentials", "gradients", "collides")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def stored_outputs(fx, name, mode):
    """The reference body's (potentials, gradients, collides) of a block as recorded in tests/golden/ref_sdf_body.npz."""
    out = [fx[f"{name}/{k}"] for k in OUT_NAMES]
    if mode == "quaternion":
        out = [(_bits(m) ^ fx[f"{name}/q_xor_{k}"]).view(F32) for m, k in zip(out, OUT_NAMES)]
    return out


def load_golden():
    """The stored outputs — a checkout without them is broken: fail, do not skip."""
    assert GOLDEN.exists(), f"{GOLDEN} is missing: it is committed, record it again with `python tests/test_oracle_ref_body.py`"
    with np.load(GOLDEN, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def record(lib):
    out = {}
    for name, blk in blocks().items():
        m = run_ref(lib, "matrix", *args_of(blk))[:3]
        q = run_ref(lib, "quaternion", *args_of(blk))[:3]
        out[f"{name}/sha256"] = np.array(input_hash(blk))
        for k, a, b in zip(OUT_NAMES, m, q):
            out[f"{name}/{k}"] = a
            out[f"{name}/q_xor_{k}"] = _bits(a) ^ _bits(b)
    out["random_tabletop/pair_potentials"] = run_ref(lib, "matrix", *args_of(blocks()["random_tabletop"]))[3]
    out["poses/branches"] = np.array([lib.ref_quaternion_branch(np.ascontiguousarray(p, F32).ctypes.data_as(C.c_void_p)) for p in blocks()["poses"]["pose"]], np.int32)
    return out


def assert_same_bits(got, want, what, pts=None):
    for k, g, w in zip(OUT_NAMES, got, want):
        g, w = np.ascontiguousarray(g, F32), np.ascontiguousarray(w, F32)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.argwhere(_bits(g) != _bits(w))
        if len(bad):
            i = tuple(bad[0])
            raise AssertionError(f"{what}: {k} differs in {len(bad)} of {g.size} elements; first at {i}: got {g[i]!r}, reference {w[i]!r}"
                                 + (f", point {pts[i[0]]!r}" if pts is not None else ""))


@pytest.fixture(scope="module")
def fx():
    return load_golden()


@pytest.fixture(scope="module")
def all_blocks():
    return blocks()


BLOCK_NAMES = list(blocks())


# ------------------------------------------------------------------------------------------------
# the stored outputs are the reference's, on these inputs
# ------------------------------------------------------------------------------------------------
def test_stored_outputs_belong_to_these_inputs(fx, all_blocks):
    assert sorted({k.split("/")[0] for k in fx}) == sorted(all_blocks)
    for name, blk in all_blocks.items():
        assert str(fx[f"{name}/sha256"]) == input_hash(blk), name
    assert GOLDEN.stat().st_size < 256 * 1024


@pytest.mark.parametrize("mode", list(MODES))
def test_live_reference_body_reproduces_the_stored_outputs(fx, all_blocks, mode):
    lib = load_ref()
    if lib is None:
        pytest.skip("oracle/_ref/libsdf_ref_body.so is not built (`make -C oracle ref` needs the reference tree)")
    for name, blk in all_blocks.items():
        assert_same_bits(run_ref(lib, mode, *args_of(blk))[:3], stored_outputs(fx, name, mode), f"{name} [{mode}]", blk["pts"])
    assert np.array_equal(_bits(run_ref(lib, "matrix", *args_of(all_blocks["random_tabletop"]))[3]), _bits(fx["random_tabletop/pair_potentials"]))
    got = [lib.ref_quaternion_branch(np.ascontiguousarray(p, F32).ctypes.data_as(C.c_void_p)) for p in all_blocks["poses"]["pose"]]
    assert got == list(fx["poses/branches"])


# ------------------------------------------------------------------------------------------------
# every block hits what its name says — asserted on the REFERENCE's outputs (and on the test's own float32 grid coordinates)
# ------------------------------------------------------------------------------------------------
def _in_range(g, dims):
    """Centre lookup in range (.cu:39-48), from float32 grid coordinates: base = trunc(g - 0.5 in double)."""
    b = np.trunc(g.astype(np.float64) - 0.5)
    return ((b >= 0) & (b + 1 < np.array(dims))).all(-1)


def test_face_blocks_meet_the_faces(fx, all_blocks):
    for name, dims in (("faces_5_24_6", (5, 24, 6)), ("faces_9_7_11", (9, 7, 11))):
        blk = all_blocks[name]
        g, ge = grid_coords(blk["lim"][0], blk["pts"]), grid_coords(blk["lim"][3], blk["pts"])  # objects 0 and 3 have the identity pose
        for ax in range(3):
            for what, t in (("first centre", 0.5), ("last centre", dims[ax] - 0.5), ("last cell", dims[ax] - 1.5)):
                near = g[np.abs(g[:, ax] - t) < 1e-4, ax]   # limits that round: both sides
                assert (near < F32(t)).any() and (near > F32(t)).any(), (name, ax, what)
                near = ge[np.abs(ge[:, ax] - t) < 1e-4, ax]  # exact limits: the value itself and both sides
                assert (near == F32(t)).any() and (near < F32(t)).any() and (near > F32(t)).any(), (name, ax, what)
            s = g[:, ax].astype(np.float64) - 0.5
            assert ((s > -1) & (s < 0)).sum() >= 5, (name, ax, "truncation toward zero with a negative weight")
            assert ((s <= -1) & (s > -2)).any() and ((s >= dims[ax] - 1) & (s < dims[ax])).any(), (name, ax, "one voxel outside")
        pot = stored_outputs(fx, name, "matrix")[0]
        inr = _in_range(g, dims)
        assert inr.any() and (~inr).any()
        # object 2 has epsilon 1.5: the out-of-range 1.0 is inside its hinge, so EVERY point has a potential
        assert (pot > 0).all(), name


def _const_expect(fx, all_blocks, name):
    blk = all_blocks[name]
    return blk, stored_outputs(fx, name, "matrix")


def test_constant_blocks_sit_on_the_branch_boundaries(fx, all_blocks):
    lib = load_ref()
    # per object (needs the live per-pair arrays); the stored per-point sums are checked below without them
    if lib is not None:
        for name in ("const_zero", "const_epsilon", "const_clearance", "tiny_positive"):
            blk = all_blocks[name]
            pp, pg, pc = run_ref(lib, "matrix", *args_of(blk))[3:]
            g0 = grid_coords(blk["lim"][0], blk["pts"])
            deep = ((g0 > 1.6) & (g0 < np.array(blk["grids"].shape[1:]) - 1.6)).all(-1)  # object 0 (identity pose): the whole stencil is inside
            assert deep.sum() > 20
            e, p = blk["eps"][0], blk["pad"][0]
            if name == "const_zero":      # -value + 0.5 * eps in double; value 0 < clearance
                assert (pp[deep, 0] == F32(0.5 * np.float64(e))).all() and (pc[deep, 0] == 1).all()
            if name == "const_epsilon":   # (value - eps) == 0: a potential of exactly 0, and value 0.2 >= clearance
                assert (pp[deep, 0] == 0).all() and (pc[deep, 0] == 0).all() and (pg[deep, 0] == 0).all()
            if name == "const_clearance":  # value == clearance: `<` is false
                assert (pc[deep] == 0).all()
            if name == "tiny_positive":   # (0, eps] branch at value ~ 0: eps / 2 * padding_scale, not eps / 2
                assert np.allclose(pp[deep, 0], 0.5 * e * p, rtol=1e-6) and p != 1
    blk, (pot, grad, col) = _const_expect(fx, all_blocks, "const_zero")
    assert (pot > 0).mean() > 0.3 and col.max() == 2  # value 0 < clearance for objects 0 and 2; object 1 has clearance 0
    blk, (pot, grad, col) = _const_expect(fx, all_blocks, "const_clearance")
    g0 = grid_coords(blk["lim"][0], blk["pts"])
    assert (col[((g0 > 1.6) & (g0 < np.array([5, 24, 6]) - 1.6)).all(-1)] == 0).all()
    blk, (pot, grad, col) = _const_expect(fx, all_blocks, "negative_clearance")
    assert 0 < (col > 0).mean() < 0.5 and (pot[col > 0] > F32(0.03 + 0.1) - 1e-6).all()  # value < -0.03: potential -value + eps / 2


def test_parameter_blocks_do_what_their_names_say(fx, all_blocks):
    def out(name):
        return stored_outputs(fx, name, "matrix")
    def inside(name):
        blk = all_blocks[name]
        R, t = blk["pose"][0, :3, :3].astype(np.float64), blk["pose"][0, :3, 3].astype(np.float64)
        g = grid_coords(blk["lim"][0], (blk["pts"].astype(np.float64) @ R.T + t).astype(F32))
        d = np.array(blk["grids"].shape[1:])
        return ((g > 0.6) & (g < d - 0.6)).all(-1), ((g < -1.6) | (g > d + 0.6)).any(-1)
    pot, grad, col = out("epsilon_1e-6")
    assert 0 < (pot > 0).mean() < 0.6
    pot, grad, col = out("epsilon_zero")  # 1 / (2 * 0) is never used: only value <= 0 contributes, with potential -value
    assert 0 < (pot > 0).mean() < 0.6 and np.isfinite(pot).all() and np.isfinite(grad).all()
    pot, grad, col = out("epsilon_negative")
    # .cu:158-160: EVERY value <= 0 takes the first branch, whatever epsilon is: values in (-0.05, 0] give -value + eps / 2 < 0
    assert (pot < 0).sum() >= 5 and (pot > 0).sum() >= 5
    for name, e in (("epsilon_one", 1.0), ("epsilon_large", 2.5)):
        pot, grad, col = out(name)
        ins, far = inside(name)
        blk = all_blocks[name]
        want = F32(1) / (F32(2) * F32(e)) * (F32(1) - F32(e)) * (F32(1) - F32(e)) * blk["pad"][0]
        assert far.sum() > 20 and (pot[far] == want).all(), name   # out of range: value 1.0, inside the hinge
        assert (grad[far] == 0).all()
    assert (out("epsilon_large")[0] > 0).all()
    assert (out("epsilon_large")[2][inside("epsilon_large")[1]] == 1).all()  # 1.0 < clearance 1.5: points outside the volume collide
    pot, grad, col = out("padding_zero")
    assert (pot > 0).any() and ((pot == 0) & (col == 0)).any()
    assert out("padding_large")[0].max() > 10 and (out("padding_large")[1] != 0).any()
    pot, grad, col = out("all_disabled")
    assert not pot.any() and not grad.any() and not col.any()
    # disables 0, -1 enabled; 0.5, 1 disabled: the block's sum equals the sum over the enabled objects only
    lib = load_ref()
    if lib is not None:
        blk = all_blocks["params"]
        pp, pg, pc = run_ref(lib, "matrix", *args_of(blk))[3:]
        on = blk["dis"] <= 0
        assert list(on) == [True] * 8 + [False, False, True]
        assert not pp[:, ~on].any() and not pg[:, ~on].any() and not pc[:, ~on].any()
        assert all(pp[:, o].any() for o in np.flatnonzero(on))


def test_pose_block_takes_every_quaternion_branch(fx, all_blocks):
    assert tuple(fx["poses/branches"]) == POSE_BRANCHES
    assert set(POSE_BRANCHES) == {0, 1, 2, 3}
    for k in OUT_NAMES:  # the fourth row is never used
        assert np.array_equal(_bits(fx[f"poses/{k}"]), _bits(fx[f"poses_fourth_row/{k}"])), k
        assert np.array_equal(fx[f"poses/q_xor_{k}"], fx[f"poses_fourth_row/q_xor_{k}"]), k
    assert fx["poses/q_xor_potentials"].any()  # the two modes do differ on this block
    assert not np.array_equal(all_blocks["poses"]["pose"][:, 3], all_blocks["poses_fourth_row"]["pose"][:, 3])


# Shares of the random block's points, measured on the reference body's outputs when tests/golden/ref_sdf_body.npz was recorded
# (the recorder prints them); asserted as floors, so that a change of the generator cannot quietly empty a branch.
RANDOM_SHARES = {"nonpositive_branch": 0.075, "band_branch": 0.735, "beyond_epsilon": 0.265, "outside_every_volume": 0.194, "collides_gt_1": 0.0406}


def random_block_shares(blk, pot, col, pair_pot):
    """Shares of the points of the random block, from the reference body's per-point outputs and per-pair potentials [N,O].
    With padding_scale 1 a pair's branch shows in its potential: -value + eps / 2 >= eps / 2 in the `<= 0` branch,
    (value - eps)^2 / (2 eps) < eps / 2 in the (0, eps] branch.  `outside` (clearly outside every volume) comes from the test's own grid coordinates."""
    assert (blk["pad"] == 1).all()
    nonpos = (pair_pot > 0) & (pair_pot >= F32(0.5) * blk["eps"][None])
    band = (pair_pot > 0) & ~nonpos
    outside = np.ones(len(blk["pts"]), bool)
    for o in range(len(blk["pose"])):
        R, t = blk["pose"][o, :3, :3].astype(np.float64), blk["pose"][o, :3, 3].astype(np.float64)
        g = grid_coords(blk["lim"][o], (blk["pts"].astype(np.float64) @ R.T + t).astype(F32))
        d = np.array(blk["grids"].shape[1:])
        outside &= ((g < -0.5 - 1e-3) | (g > d - 0.5 + 1e-3)).any(-1)  # in range is (-0.5, d - 0.5): truncation toward zero; 1e-3 absorbs rounding
    assert not pot[outside].any() and not col[outside].any()
    return dict(nonpositive_branch=float(nonpos.any(1).mean()), band_branch=float(band.any(1).mean()), beyond_epsilon=float((pot == 0).mean()),
                outside_every_volume=float(outside.mean()), collides_gt_1=float((col > 1).mean()))


def test_random_block_coverage(fx, all_blocks):
    blk = all_blocks["random_tabletop"]
    pot, grad, col = stored_outputs(fx, "random_tabletop", "matrix")
    s = random_block_shares(blk, pot, col, fx["random_tabletop/pair_potentials"])
    for k, floor in RANDOM_SHARES.items():
        assert s[k] >= floor > 0, (k, s)


# ------------------------------------------------------------------------------------------------
# the oracle against the reference body
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BLOCK_NAMES)
def test_oracle_matches_reference_body_matrix_mode(fx, all_blocks, name):
    blk = all_blocks[name]
    assert not orc.sophus_mode()
    assert_same_bits(orc.sdf_loss_forward(*args_of(blk)), stored_outputs(fx, name, "matrix"), f"{name} [matrix]", blk["pts"])
    lib = load_ref()
    if lib is None:
        return
    # per pair: the reference's [N,O] arrays against single-object oracle calls.  Both sides are added to +0 first, as the
    # launcher's reduction does: the body stores -0 gradients where (value - eps) == 0, which no per-point output can show.
    pp, pg, pc = run_ref(lib, "matrix", *args_of(blk))[3:]
    for o in range(len(blk["pose"])):
        one = orc.sdf_loss_forward(blk["pose"][o:o + 1], blk["grids"][o:o + 1], blk["lim"][o:o + 1], blk["pts"], blk["eps"][o:o + 1],
                                   blk["pad"][o:o + 1], blk["clr"][o:o + 1], blk["dis"][o:o + 1])
        assert_same_bits(one, (pp[:, o] + F32(0), pg[:, o] + F32(0), pc[:, o] + F32(0)), f"{name} [matrix] object {o}", blk["pts"])


@pytest.mark.parametrize("name", BLOCK_NAMES)
def test_oracle_matches_reference_body_quaternion_mode(fx, all_blocks, name):
    blk = all_blocks[name]
    orc.set_sophus_mode(True)
    try:
        got = orc.sdf_loss_forward(*args_of(blk))
    finally:
        orc.set_sophus_mode(False)
    assert_same_bits(got, stored_outputs(fx, name, "quaternion"), f"{name} [quaternion]", blk["pts"])


# ------------------------------------------------------------------------------------------------
# the ragged-pool path (orc_fk_sdf over the engine's object table) against per-object reference-body sums
# ------------------------------------------------------------------------------------------------
# the third: clearances below the epsilons too, so that nothing but the `value <= 0` rule keeps the band (epsilon, 0] alive in
# the influence regions
TABLETOP_CFGS = (dict(epsilon=0.2), dict(epsilon=1.25), dict(epsilon=-0.05, target_epsilon=-0.02, clearance=-0.1, target_clearance=-0.08))


def tabletop_scenes():
    """Three tabletop scenes with unequal dims per object and the layer parameters of each: the reference's defaults; epsilon
    1.25 on every object but the target, so that the reference's out-of-range 1.0 lies inside the hinge; and negative epsilons,
    where only the `value <= 0` branch is left (.cu:158) and values in (epsilon, 0] still count."""
    from omg_planner_amd import scenes as sc
    from tests import helpers as H
    scenes = [sc.make_tabletop_scene(s, grid=24, table_grid=(40, 28, 12)) for s in (3, 4, 3)]
    return scenes, [dict(H.LAYER_CFG, **c) for c in TABLETOP_CFGS]


def tabletop_batch():
    """tabletop_scenes() as one engine table (ragged pool, influence regions fitted on the host)."""
    from omg_planner_amd import scenes as sc
    parts = [sc.pack_table([s], c) for s, c in zip(*tabletop_scenes())]
    rec = np.concatenate([p.objects for p in parts])
    begin = np.cumsum([0] + [len(p.objects) for p in parts]).astype(np.int32)
    for k, off in enumerate(np.cumsum([0] + [p.pool.size for p in parts[:-1]])):
        rec["grid_offset"][begin[k]: begin[k + 1]] += off
    return sc.SceneBatch(rec, begin, np.concatenate([p.pool for p in parts]))


def tabletop_joints(model, S, Cn, seed=5):
    """Configurations around a table-top pre-grasp with the shoulder pushed 0.7 rad forward: the arm dips into the objects and
    the table, so that points lie inside volumes (value <= 0) and collide."""
    from omg_planner_amd import scenes as sc
    rng = np.random.RandomState(seed)
    q = np.stack([sc.make_goal_set(s, Cn) for s in range(S)])
    q[:, :, :7] += rng.normal(0, 0.3, size=(S, Cn, 7))
    q[:, :, 1] += 0.7
    return np.clip(q, model.joint_lower_limit[0], model.joint_upper_limit[0])


def reference_table_sums(lib, mode, batch, scene, pts):
    """Per-object reference-body sums over the records of one scene of the engine's table, at float32 points [N,3]."""
    objs = []
    for r in batch.objects[batch.scene_begin[scene]: batch.scene_begin[scene + 1]]:
        d = r["dim"]
        pose = np.eye(4, dtype=F32)
        pose[:3] = r["pose_inv"].reshape(3, 4)
        grid = batch.pool[int(r["grid_offset"]): int(r["grid_offset"]) + int(d.prod())].reshape(tuple(d))
        objs.append((pose, grid, np.array([*r["lo"], *r["hi"], *d, r["delta"]], F32), r["epsilon"], r["padding_scale"], r["clearance"], F32(r["disabled"])))
    return ref_single_object_sum(lib, mode, objs, pts)


def test_ragged_pool_path_matches_per_object_reference_sums():
    """The points are float32(config_points): orc_points_of_config and orc_fk_sdf run the same orc_fk / orc_point code, and
    the narrowing is the same (float) cast, so they are reproduced bit for bit from config_points."""
    lib = load_ref()
    if lib is None:
        pytest.skip("oracle/_ref/libsdf_ref_body.so is not built (`make -C oracle ref` needs the reference tree)")
    from omg_planner_amd import robot as rb
    m = rb.PandaModel(seed=3)
    P, blob = m.points_per_link, m.blob()
    batch = tabletop_batch()
    S, Cn = 3, 6
    joints = tabletop_joints(m, S, Cn)
    pot, grad, col = orc.fk_sdf(blob, P, batch, joints)
    hit = seen = 0
    for s in range(S):
        assert len({tuple(d) for d in batch.objects["dim"][batch.scene_begin[s]: batch.scene_begin[s + 1]]}) > 1  # unequal dims
        for c in range(Cn):
            pts = orc.config_points(blob, P, joints[s, c]).reshape(-1, 3).astype(F32)
            want = reference_table_sums(lib, "matrix", batch, s, pts)
            assert_same_bits((pot[s, c].reshape(-1), grad[s, c].reshape(-1, 3), col[s, c].reshape(-1)), want, f"scene {s} configuration {c}", pts)
            hit += int((want[0] > 0).sum())
            if s == 2:
                seen += regions_hold_every_contribution(lib, batch, s, pts)
    assert hit > 200 and seen > 20 and (col[0] > 0).sum() > 20
    assert (pot[1] > 0).all()      # scene 1: epsilon 1.25, every point has a potential
    assert (pot[2] < 0).sum() > 20  # scene 2: negative epsilon, values in (epsilon / 2, 0]


def regions_hold_every_contribution(lib, batch, scene, pts):
    """Every point to which an object of the scene adds anything lies inside that record's influence region (include/omg_hip.h:
    sum_k max(|t_k - c_k| - h_k, 0)^2 <= R^2 in offset-from-lo coordinates) — the kernels skip the points outside it."""
    seen = 0
    for r in batch.objects[batch.scene_begin[scene]: batch.scene_begin[scene + 1]]:
        if r["disabled"] > 0:
            continue
        T = r["pose_inv"].reshape(3, 4).astype(np.float64)
        t = pts.astype(np.float64) @ T[:, :3].T + T[:, 3] - r["lo"].astype(np.float64)
        d = np.maximum(np.abs(t - r["rb_c"]) - r["rb_h"], 0.0)
        inside = (d * d).sum(1) <= float(r["rb_r2"])
        pose = np.eye(4, dtype=F32)
        pose[:3] = r["pose_inv"].reshape(3, 4)
        dim = r["dim"]
        grid = batch.pool[int(r["grid_offset"]): int(r["grid_offset"]) + int(dim.prod())].reshape(tuple(dim))
        p1, g1, c1 = run_ref(lib, "matrix", pose[None], grid[None], np.array([[*r["lo"], *r["hi"], *dim, r["delta"]]], F32), pts, [r["epsilon"]],
                             [r["padding_scale"]], [r["clearance"]], [0])[:3]
        adds = (p1 != 0) | (c1 != 0) | (g1 != 0).any(1)
        assert not (adds & ~inside).any(), (r["epsilon"], pts[adds & ~inside][:3])
        seen += int(adds.sum())
    return seen


if __name__ == "__main__":  # record tests/golden/ref_sdf_body.npz from oracle/_ref/libsdf_ref_body.so (`make -C oracle ref`)
    lib = load_ref()
    if lib is None:
        raise SystemExit(f"{REF_LIB} is not built: `make -C oracle ref` needs the reference tree")
    out = record(lib)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, GOLDEN.stat().st_size, "bytes,", len(blocks()), "blocks,", sum(len(b["pts"]) for b in blocks().values()), "points")
    blk = blocks()["random_tabletop"]
    pot, grad, col, pp = run_ref(lib, "matrix", *args_of(blk))[:4]
    print("random_tabletop shares:", random_block_shares(blk, pot, col, pp), "nonzero potential", float((pot != 0).mean()), "collides", float((col > 0).mean()))
