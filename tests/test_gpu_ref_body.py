"""GPU tests (-m gpu): the HIP SDF kernels against THE REFERENCE'S OWN kernel body (layers/sdf_matching_loss_kernel.cu:96-195
compiled for the host, see tests/test_oracle_ref_body.py and oracle/ref_body_wrapper.cpp) — directly, not through the oracle.

The stored outputs tests/golden/ref_sdf_body.npz are always there; the two tests that need the live library
oracle/_ref/libsdf_ref_body.so skip where it is not built.  The reference body runs in its matrix mode, the arithmetic of
the kernels (R p + t and R^T v as fma chains); everything is compared bit for bit except the engine's table path, whose
points come from the device's own float64 FK (see that test)."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_oracle_ref_body as RB

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NO_LIB = "oracle/_ref/libsdf_ref_body.so is not built (`make -C oracle ref` needs the reference tree)"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    from omg_planner_amd import _lib
    assert _lib.device_arch().startswith("gfx950"), _lib.device_arch()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return RB.load_golden()


@pytest.fixture(scope="module")
def all_blocks():
    return RB.blocks()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run_op(dev, args):
    from omg_planner_amd import ops
    got = ops.sdf_loss_forward(*[_t(np.ascontiguousarray(a, np.float32), dev) for a in args])
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


@pytest.mark.parametrize("name", RB.BLOCK_NAMES)
def test_padded_op_matches_reference_body(dev, fx, all_blocks, name):
    """omgx_sdf_loss_forward on every block of the CPU module against the stored matrix-mode outputs, bit for bit."""
    blk = all_blocks[name]
    assert str(fx[f"{name}/sha256"]) == RB.input_hash(blk)
    RB.assert_same_bits(_run_op(dev, RB.args_of(blk)), RB.stored_outputs(fx, name, "matrix"), f"{name} [kernel]", blk["pts"])


def test_padded_op_full_size_matches_live_reference_body(dev):
    """200 000 random points through the cost_topk300 scene — the inputs of test_sdf_loss_forward_bit_exact_vs_oracle with its
    non-finite and out-of-int-range rows replaced by finite ones — against the live library."""
    lib = RB.load_ref()
    if lib is None:
        pytest.skip(NO_LIB)
    fixture = H.load("cost_topk300.npz")
    poses, eps, pad, clr, dis = H.layer_params_from(fixture)
    rng = np.random.RandomState(0)
    pts = rng.uniform([-0.4, -0.8, -0.3], [1.2, 0.8, 1.2], size=(200_000, 3)).astype(np.float32)
    pts[:8] = [[1e4, 0, 0], [-1e4, 0, 0], [300.0, 1, 1], [0.5, 0.0, 0.02], [0, -1e3, 0], [50.0, 50.0, 50.0], [0.5, 0.0, 0.02], [-0.3, -0.3, -0.3]]
    args = (poses, fixture["sdf"], fixture["limits"], pts, eps, pad, clr, dis)
    want = RB.run_ref(lib, "matrix", *args)[:3]
    RB.assert_same_bits(_run_op(dev, args), want, "cost_topk300, 200 000 points", pts)
    assert (want[0] > 0).mean() > 0.05 and want[2].sum() > 100  # both hinge branches, as in the oracle's test


def _device_tables(dev):
    """The tabletop batch on the device twice: packed with host-fitted influence regions, and scene by scene with the regions
    fitted on the device (from_scenes takes one set of layer parameters per call)."""
    from omg_planner_amd import ops
    batch = RB.tabletop_batch()
    yield "host-fitted", batch, [(ops.DeviceScenes(batch, dev), slice(0, batch.num_scenes))]
    yield "device-fitted", batch, [(ops.DeviceScenes.from_scenes([s], c, dev), slice(k, k + 1)) for k, (s, c) in enumerate(zip(*RB.tabletop_scenes()))]


def test_engine_table_path_matches_per_object_reference_sums(dev):
    """omgx_fk_sdf — ragged pool, influence regions, culling — on the tabletop batch of the CPU module (one scene with epsilon
    1.25, where the reference's out-of-range 1.0 is inside the hinge and nothing may be culled; one with negative epsilons)
    against the in-object-order sums of single-object reference-body runs.

    The reference sums are taken at float32(the oracle's float64 points).  The device computes its own float64 FK, whose last
    ulp can differ and then flips a float32 point by one ulp, so — as in test_fk_sdf_matches_oracle, whose bounds these are —
    at least 99.9 % of the elements must be bit-equal and the rest within 5e-6 (potentials, collides) / 5e-4 (gradients)."""
    lib = RB.load_ref()
    if lib is None:
        pytest.skip(NO_LIB)
    from omg_planner_amd import ops, robot as rb
    from oracle import oracle as orc
    m = rb.PandaModel(seed=3)
    P, blob = m.points_per_link, m.blob()
    S, Cn = 3, 6
    joints = RB.tabletop_joints(m, S, Cn)
    for label, batch, tables in _device_tables(dev):
        want = [np.zeros((S, Cn, 10 * P), np.float32), np.zeros((S, Cn, 10 * P, 3), np.float32), np.zeros((S, Cn, 10 * P), np.float32)]
        for s in range(S):
            for c in range(Cn):
                pts = orc.config_points(blob, P, joints[s, c]).reshape(-1, 3).astype(np.float32)
                for w, r in zip(want, RB.reference_table_sums(lib, "matrix", batch, s, pts)):
                    w[s, c] = r
        got = [np.zeros_like(w) for w in want]
        for ds, sl in tables:
            out = ops.fk_sdf(ops.robot_blob(m, dev), P, ds, _t(joints[sl], dev))
            torch.cuda.synchronize()
            for g, o in zip(got, out):
                g[sl] = o.cpu().numpy().reshape(g[sl].shape)
        for name, g, w in zip(RB.OUT_NAMES, got, want):
            for s in range(S):
                same = (g[s].view(np.uint32) == w[s].view(np.uint32)).mean()
                print(f"{label} scene {s} {name}: bit-equal share {same:.6f}, max abs difference {np.abs(g[s] - w[s]).max():.3g}")
                assert same > 0.999, (label, s, name, same)
                np.testing.assert_allclose(g[s], w[s], rtol=0, atol=5e-4 if name == "gradients" else 5e-6, err_msg=f"{label} scene {s} {name}")
        assert (want[0][0] > 0).sum() > 200 and (want[2][0] > 0).sum() > 20
        assert (want[0][1] > 0).all()       # epsilon 1.25: every point has a potential, far from every volume too
        assert (want[0][2] < 0).sum() > 20  # negative epsilon: values in (epsilon / 2, 0]
