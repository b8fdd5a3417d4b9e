"""GPU: GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> on the device -- ProjForm::Rows2Fisheye, k_lin_proj_fisheye and
k_error_proj_fisheye -- against the reference's recorded answers (tests/golden/fisheye_mixed.npz, fisheye_example.npz:
tests/golden/make_golden_fisheye.py).

Tolerances are the project's, as stated at the top of tests/test_gpu_parity.py, in the norm of tests/stereo_support.rel: records
<= 1e-12, Hessian diagonal / gradient <= 1e-10, the step of a damped solve <= 1e-7, errors <= 1e-9, LM trajectories the identical
accept / reject sequence with per-iteration errors <= 1e-6, final values <= 1e-5.  fisheye_mixed records trace_stable = 1 (the
reference takes the same accept / reject sequence under the reversed elimination ordering), so the identical sequence is demanded."""
import numpy as np
import pytest

from gtsam_amd.params import LevenbergMarquardtParams as LMP
from gtsam_amd.problem import NOISE_ISOTROPIC
from tests import fisheye_support as FS
from tests.fisheye_support import rel
from tests.test_gpu_stereo import check_solves, check_trajectory, run_two_shards

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gtsam_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def mixed():
    g = FS.fixture("fisheye_mixed")
    return FS.problem_of(g), g["values0"], g


# ---- 1. fixture parity and the branch rows ------------------------------------------------------------------------------------
def test_error_records_diagonal_gradient_vs_reference(gpu, mixed):
    p, v0, g = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    print("error", e, float(g["error"]))
    assert abs(e - float(g["error"])) <= 1e-9 * float(g["error"])
    dev.linearize()
    for ft in (1, 2, 3):
        J = dev.jacobians(ft)
        assert J.shape == g[f"jac{ft}"].shape
        print("records", ft, rel(J, g[f"jac{ft}"]))
        assert rel(J, g[f"jac{ft}"]) <= 1e-12, ft
    hd, grad = dev.hessian_diagonal(), dev.gradient()
    print("diagonal", rel(hd, g["hessian_diagonal"]), "gradient", rel(grad, g["gradient"]))
    assert rel(hd, g["hessian_diagonal"]) <= 1e-10
    assert rel(grad, g["gradient"]) <= 1e-10
    assert dev.reduced_dim == 6 * 11 and dev.jacobians(4).shape == (0, 30)
    dev.close()


def test_branch_rows(gpu, mixed):
    """The on-axis and Taylor rows to 1e-12; the row of the landmark behind its camera has 18 Jacobian entries that are == 0.0 and
    the residual 2 fx / sigma."""
    p, v0, g = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    J = dev.jacobians(1)
    dev.close()
    scale = np.abs(g["jac1"][:, 18:]).max()
    for b in ("on_axis", "taylor"):
        k = int(g["branch_" + b])
        assert np.abs(J[k] - g["jac1"][k]).max() <= 1e-12 * max(scale, np.abs(g["jac1"][k]).max()), b
    k = int(g["branch_on_axis"])
    K = FS.calib9(p)[p.proj_calib[k]]
    assert np.array_equal(J[k, 12:18].reshape(2, 3), np.array([[K[0], K[2]], [0.0, K[1]]]) @ np.array([[0.125, 0, 0], [0, 0.125, 0]]))
    k = int(g["branch_behind"])
    b = -2.0 * FS.calib9(p)[p.proj_calib[k], 0] / float(p.noise_data[p.noise_off[p.proj_noise[k]]])
    assert np.all(J[k, :18] == 0.0) and np.array_equal(J[k, 18:], [b, b])


# ---- 2. damped solves and trajectories ------------------------------------------------------------------------------------------
def test_damped_solves_vs_reference(gpu, mixed):
    p, v0, g = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    check_solves(dev, g)
    dev.close()


def test_lm_trajectory_vs_reference(gpu, mixed):
    from gtsam_amd.optimizer import DeviceLevenbergMarquardt
    p, v0, g = mixed
    opt = DeviceLevenbergMarquardt(p, v0, LMP())
    opt.optimize()
    check_trajectory(opt, g)
    opt.dev.close()


def test_fisheye_example_reproduces_the_reference(gpu):
    """examples/FisheyeExample.cpp under LM with default parameters: the reference's iteration count, accept / reject sequence,
    per-iteration errors and final values; a consistent scene, so both reach zero error to rounding -- the final errors agree to 1e-9
    of the scale the run started from.  Then the same through the public Python surface."""
    from gtsam_amd import api as A
    from gtsam_amd import datasets as D
    from gtsam_amd.optimizer import DeviceLevenbergMarquardt
    g = FS.fixture("fisheye_example")
    p, v0 = FS.problem_of(g), g["values0"]
    opt = DeviceLevenbergMarquardt(p, v0, LMP())
    assert abs(opt.error() - float(g["error"])) <= 1e-9 * float(g["error"])
    opt.optimize()
    ref, tr = g["trace"], np.array(opt.trace)[:, :3]
    print("example trace", tr, ref)
    assert opt.iterations() == int(g["iterations"]) and tr.shape == ref.shape and np.array_equal(tr[:, 0], ref[:, 0])
    assert rel(tr[:, 1], ref[:, 1]) <= 1e-6 and np.allclose(tr[:, 2], ref[:, 2], rtol=1e-6, atol=0)
    assert abs(opt.error() - float(g["final_error"])) <= 1e-9 * float(g["error"]) and opt.error() <= 1e-15 and float(g["final_error"]) <= 1e-15
    assert rel(opt.values_packed(), g["final_values"]) <= 1e-5
    opt.dev.close()
    graph, initial = D.fisheye_example_graph()
    lm = A.LevenbergMarquardtOptimizer(graph, initial)
    result = lm.optimize()
    assert lm.iterations() == int(g["iterations"])
    packed = np.concatenate([result.at(k).packed() if hasattr(result.at(k), "packed") else result.at(k) for k in result.keys()])
    assert rel(packed, g["final_values"]) <= 1e-5
    lm._opt.dev.close()


# ---- 3. chunk and block boundaries ----------------------------------------------------------------------------------------------
def trimmed(g, n):
    """n projection factors of the fixture, a fisheye factor at both ends of the range -- the first n, the last of them replaced by
    factor n where that one is no fisheye factor -- and a prior AT the initial value on every pose and landmark (zero residual: the
    priors add nothing to the error or the gradient, and keep the system definite).  Returns (Problem, the factors' indices)."""
    full = FS.problem_of(g)
    fish = FS.is_fisheye(full)
    idx = np.arange(n)
    if not fish[idx[-1]]:
        idx[-1] = n
    assert fish[idx[0]] and fish[idx[-1]]
    p = FS.problem_of(g, between_v1=[], between_v2=[], between_z=[], between_noise=[], prior_var=[], prior_off=[], prior_data=[], prior_noise=[])
    for f, w in (("proj_pose", 1), ("proj_point", 1), ("proj_z", 2), ("proj_noise", 1), ("proj_calib", 1), ("proj_sensor", 1)):
        setattr(p, f, getattr(p, f).reshape(-1, w)[idx].reshape(-1).copy())
    n6 = p.add_noise(NOISE_ISOTROPIC, 6, [0.1]); n3 = p.add_noise(NOISE_ISOTROPIC, 3, [0.1])
    off = p.val_offsets()
    for v in range(p.n_vars):
        p.add_prior(v, g["values0"][off[v]:off[v + 1]], n6 if p.var_type[v] == 0 else n3)
    return p, idx


# k_lin_proj_fisheye: 64 observations per wavefront chunk, 256 per workgroup; k_error_proj_fisheye: 256 per workgroup
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_chunk_boundaries(gpu, mixed, n):
    """One lane, the last lane of a wavefront chunk, a full chunk, one past it, one past a 256-thread workgroup.  The range mixes the
    four calibrations, so every wavefront takes both sides of the model dispatch."""
    _, v0, g = mixed
    p, idx = trimmed(g, n)
    if n >= 4:
        assert all(set(FS.models(p)[p.proj_calib[c:c + 64]]) == {0, 1} for c in range(0, n - 3, 64))
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    dev.linearize()
    J = dev.jacobians(1)
    grad = dev.gradient()
    rc, out = dev.try_lambda(1e-3, False)
    dev.close()
    assert J.shape == (n, 20)
    print("n", n, "records", rel(J, g["jac1"][idx]))
    assert rel(J, g["jac1"][idx]) <= 1e-12
    Jh, eh = FS.evaluate(p, v0)
    assert rel(J, Jh) <= 1e-12
    want_e, want_g = FS.sums_from_records(p, J)
    print("error", e, want_e, eh.sum(), "gradient", rel(grad, want_g))
    assert abs(e - want_e) <= 1e-9 * want_e and abs(e - eh.sum()) <= 1e-9 * want_e
    assert rel(grad, want_g) <= 1e-10
    assert rc == 0 and abs(out[0] - 0.5 * float(J[:, 18:].ravel() @ J[:, 18:].ravel())) <= 1e-9 * out[0]


# ---- 4. PCG, 5. sharding, 6. reproducibility (the assertions of tests/test_gpu_sam3d.py section 5) --------------------------------
def test_pcg_equals_direct_solve(gpu, mixed):
    p, v0, _ = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    rc, out = dev.try_lambda(1e-3, False)
    d = dev.delta().copy()
    rc2, out2, its = dev.try_lambda_pcg(1e-3, False, max_iterations=5000, min_iterations=1, epsilon_rel=1e-13, epsilon_abs=1e-26)
    d2 = dev.delta().copy()
    dev.close()
    assert rc == rc2 == 0 and its > 1
    assert rel(d2, d) <= 1e-7, rel(d2, d)


def test_two_shards_equal_one(gpu, mixed):
    """Landmark factors follow their landmark; the form of the range comes from the whole graph's model list on either shard."""
    from gtsam_amd.optimizer import DeviceLevenbergMarquardt
    p, v0, _ = mixed
    single = DeviceLevenbergMarquardt(p, v0, LMP())
    single.dev.linearize()
    rc1, out1 = single.dev.try_lambda(1e-3, False)
    d1 = single.dev.delta()
    single.optimize()

    def body(rank, allreduce):
        opt = DeviceLevenbergMarquardt(p, v0, LMP(), shard=rank, n_shards=2, allreduce=allreduce)
        opt.dev.linearize()
        rc, out = opt.dev.try_lambda(1e-3, False)
        d = opt.dev.delta()
        opt.optimize()
        return rc, out, d, np.array(opt.trace)[:, :3], opt.values_packed(), opt.dev.structure_hash()

    res = run_two_shards(body)
    ref = np.array(single.trace)[:, :3]
    for rc, out, d, trace, vals, h in res:
        assert rc == rc1 and h == single.dev.structure_hash()
        assert np.abs(d - d1).max() <= 1e-9 * np.abs(d1).max()
        assert np.allclose(out[:3], out1[:3], rtol=1e-9)
        assert trace.shape == ref.shape and np.array_equal(trace[:, 0], ref[:, 0])
        assert np.abs(trace[:, 1] - ref[:, 1]).max() <= 1e-7 * np.abs(ref[:, 1]).max()
        assert np.abs(vals - single.values_packed()).max() <= 1e-6 * np.abs(vals).max()
    assert np.array_equal(res[0][4], res[1][4])


def test_two_shards_pcg_equal_one(gpu, mixed):
    p, v0, _ = mixed
    cg = dict(max_iterations=300, min_iterations=1, epsilon_rel=1e-10, epsilon_abs=1e-14)

    def solve(dev):
        dev.set_values(v0)
        dev.linearize()
        rc, out, its = dev.try_lambda_pcg(1e-3, False, **cg)
        return rc, out, its, dev.delta().copy()

    single = gpu.DeviceGraph(p)
    rc1, out1, its1, d1 = solve(single)
    single.close()
    assert rc1 == 0 and its1 > 1

    def body(rank, allreduce):
        dev = gpu.DeviceGraph(p, shard=rank, n_shards=2, allreduce=allreduce)
        r = solve(dev)
        dev.close()
        return r

    res = run_two_shards(body)
    for rc, out, its, d in res:
        assert rc == 0 and abs(its - its1) <= 1
        assert np.abs(d - d1).max() <= 1e-7 * np.abs(d1).max()
        assert np.allclose(out[:3], out1[:3], rtol=1e-8)
    assert np.array_equal(res[0][3], res[1][3])


def test_two_runs_identical_bits(gpu, mixed):
    p, v0, _ = mixed

    def run():
        dev = gpu.DeviceGraph(p)
        dev.set_values(v0)
        e = dev.error()
        dev.linearize()
        rc, out = dev.try_lambda(1e-3, False)
        rc2, out2 = dev.try_lambda(1e-4, True)
        r = (e, rc, out.copy(), rc2, out2.copy(), dev.delta().copy(), dev.jacobians(1).copy(), dev.hessian_diagonal().copy(), dev.gradient().copy())
        dev.close()
        return r

    a, b = run(), run()
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))
