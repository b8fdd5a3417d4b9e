"""GPU: planar landmark SLAM -- Point2 landmarks and BearingRangeFactor / RangeFactor / BearingFactor <Pose2, Point2> (gtsam/sam) on the
device against the reference's recorded answers (tests/golden/planar_mixed.npz, planar_slam.npz: tests/golden/make_golden_planar.py).

Tolerances are the project's, as stated at the top of tests/test_gpu_stereo.py, in the norm of tests/stereo_support.rel: records
<= 1e-12, Hessian diagonal / gradient <= 1e-10, the step of a damped solve <= 1e-7, errors <= 1e-9, LM trajectories the identical
accept / reject sequence with per-iteration errors <= 1e-6, final values <= 1e-5.  Both fixtures record trace_stable = 1 (the
reference takes the same accept / reject sequence under the reversed elimination ordering), so the identical sequence is demanded.
At the C ABI a POINT2 holds three storage doubles (x, y, 0) and three tangent entries (dx, dy, 0): every third entry the library
returns must be == 0.0, not small."""
import numpy as np
import pytest

from gtsam_amd.params import LevenbergMarquardtParams as LMP
from gtsam_amd.problem import NOISE_ISOTROPIC
from tests import planar_support as PL
from tests.planar_support import rel
from tests.test_gpu_stereo import check_solves, check_trajectory

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
    g = PL.fixture("planar_mixed")
    return PL.problem_of(g), g["values0"], g


@pytest.fixture(scope="module")
def slam():
    g = PL.fixture("planar_slam")
    return PL.problem_of(g), g["values0"], g


# ---- 1. fixture parity ------------------------------------------------------------------------------------------------------
def test_error_records_diagonal_gradient_vs_reference(gpu, mixed):
    p, v0, g = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    assert abs(e - float(g["error"])) <= 1e-9 * float(g["error"])
    dev.linearize()
    for ft in (7, 2, 3, 6):
        J = dev.jacobians(ft)
        assert J.shape == g[f"jac{ft}"].shape
        assert rel(J, g[f"jac{ft}"]) <= 1e-12, ft
    assert dev.jacobians(5).shape == (0, 30) and dev.jacobians(1).shape == (0, 20)
    hd, grad = dev.hessian_diagonal(), dev.gradient()
    assert rel(hd, g["hessian_diagonal"]) <= 1e-10
    assert rel(grad, g["gradient"]) <= 1e-10
    third = PL.third_entries(p)
    assert third.size == 33 and np.all(hd[third] == 0.0) and np.all(grad[third] == 0.0) and np.all(dev.graph_gradient()[third] == 0.0)
    dev.close()


def test_damped_solves_and_the_padding_vs_reference(gpu, mixed):
    """Two damped solves (the second with diagonalDamping) against the reference; every POINT2's third tangent / storage entry is
    exactly 0 after linearise, after each lambda try and after accept."""
    p, v0, g = mixed
    third = PL.third_entries(p)
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    assert np.all(dev.values()[third] == 0.0) and np.all(dev.hessian_diagonal()[third] == 0.0)
    check_solves(dev, g)
    for lam, dd in ((1e-3, False), (1e-4, True), (7.0, True), (1e-9, False)):
        rc, out = dev.try_lambda(lam, dd)
        assert rc == 0
        d, t = dev.delta(), dev.trial_values()
        assert np.all(d[third] == 0.0) and np.all(t[third] == 0.0), (lam, dd)
        assert np.abs(d).max() > 0 and np.all(np.isfinite(d))
    dev.accept()
    assert np.all(dev.values()[third] == 0.0)
    dev.linearize()
    assert np.all(dev.hessian_diagonal()[third] == 0.0) and np.all(dev.gradient()[third] == 0.0)
    dev.close()


@pytest.mark.parametrize("name", PL.FIXTURES)
def test_lm_trajectory_vs_reference(gpu, name):
    from gtsam_amd.optimizer import DeviceLevenbergMarquardt
    g = PL.fixture(name)
    p, v0 = PL.problem_of(g), g["values0"]
    opt = DeviceLevenbergMarquardt(p, v0, LMP())
    n_poses = int((p.var_type == PL.POSE2).sum())
    # a landmark seen by planar factors alone is eliminated as a landmark: the reduced system is the poses
    assert opt.dev.reduced_dim == 3 * n_poses and opt.dev.dim_size == 3 * p.n_vars
    opt.optimize()
    check_trajectory(opt, g)
    assert np.all(opt.values_packed()[PL.third_entries(p)] == 0.0)
    opt.dev.close()


def test_planar_slam_records_sums_and_solves(gpu, slam):
    p, v0, g = slam
    assert p.n_sam2 == 1080 and p.n_vars == 160 and p.n_between == 39 and p.n_prior == 1
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    assert abs(dev.error() - float(g["error"])) <= 1e-9 * float(g["error"])
    dev.linearize()
    assert rel(dev.jacobians(7), g["jac7"]) <= 1e-12
    assert rel(dev.hessian_diagonal(), g["hessian_diagonal"]) <= 1e-10
    assert rel(dev.gradient(), g["gradient"]) <= 1e-10
    check_solves(dev, g)
    dev.close()


# ---- 2. branch rows ---------------------------------------------------------------------------------------------------------
def test_branch_rows_and_zero_entries(gpu, mixed):
    """The recorded branch factors give the fixture's records; a landmark on the pose has a bearing row with a zero Jacobian; the rows
    a factor does not have and A2's third column are exactly 0."""
    p, v0, g = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    J = dev.jacobians(7)
    dev.close()
    scale = np.abs(g["jac7"][:, 18:]).max()
    for name in ("branch_same", "branch_bearing_zero", "branch_range_zero", "branch_wrap"):
        k = int(g[name])
        assert np.abs(J[k] - g["jac7"][k]).max() <= 1e-12 * max(scale, np.abs(g["jac7"][k]).max()), name
    k = int(g["branch_bearing_zero"])
    assert np.all(J[k, :18] == 0.0) and J[k, 18] != 0.0
    k = int(g["branch_range_zero"])
    inv_sigma = 1.0 / float(p.noise_data[p.noise_off[p.sam2_noise[k]]])
    assert np.array_equal(J[k, 9:11], [inv_sigma, inv_sigma]) and np.array_equal(J[k, :3], [-inv_sigma, -inv_sigma, 0.0])
    k = int(g["branch_same"])
    assert J[k, 18] == 0.0                       # (contraction is off on the device: the product h^-1 z of equal rotations has s = 0 exactly)
    k = int(g["branch_wrap"])
    assert abs(g["probe"][k, 6]) > np.pi and abs(J[k, 18]) * float(p.noise_data[p.noise_off[p.sam2_noise[k]]]) < 0.1
    mask = PL.unused_entries(p)
    assert mask.any(1).all() and np.all(J[mask] == 0.0)
    assert set(p.sam2_kind) == {0, 1, 2}


# ---- 3. chunk boundaries ----------------------------------------------------------------------------------------------------
def trimmed(g, n):
    """The first n planar factors of the fixture and a prior AT the initial value on every pose (zero residual: the priors add nothing
    to the error or the gradient, and keep the reduced system definite; a landmark that the n factors do not fix is held by the damping
    term of the try)."""
    p = PL.problem_of(g, between_v1=[], between_v2=[], between_z=[], between_noise=[], prior_var=[], prior_off=[], prior_data=[], prior_noise=[],
                      pose_partial_kind=[], pose_partial_var=[], pose_partial_z=[], pose_partial_noise=[])
    for f, w in (("sam2_kind", 1), ("sam2_pose", 1), ("sam2_point", 1), ("sam2_z", 3), ("sam2_noise", 1)):
        setattr(p, f, getattr(p, f)[:w * n].copy())
    n3 = p.add_noise(NOISE_ISOTROPIC, 3, [0.1])
    off = p.val_offsets()
    for v in np.flatnonzero(p.var_type == PL.POSE2):
        p.add_prior(int(v), g["values0"][off[v]:off[v + 1]], n3)
    return p


@pytest.fixture(scope="module")
def full_records(gpu, slam):
    p, v0, _ = slam
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    J = dev.jacobians(7)
    dev.close()
    J.setflags(write=False)
    return J


# k_lin_planar / k_error_planar: 64 factors per wavefront, 256 per workgroup; k_obs_E / k_obs_v: grid1(n / 4 + 1) workgroups of 256
# observations, a second workgroup from n = 1024 on
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_chunk_boundaries(gpu, slam, full_records, n):
    """The records of the first n factors are, bit for bit, those of the same factors inside the full graph, and equal the
    host-compiled evaluators to the records' tolerance (not bit for bit: cos, sin and atan2 of the device's and the host's maths
    libraries are each within an ulp of the exact value, not of each other); error, gradient and the linear error of a try are the
    sums of those records."""
    p_full, v0, g = slam
    p = trimmed(g, n)
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    dev.linearize()
    J = dev.jacobians(7)
    grad, hd = dev.gradient(), dev.hessian_diagonal()
    rc, out = dev.try_lambda(1.0, False)
    d = dev.delta()
    dev.close()
    assert J.shape == (n, 21) and np.array_equal(J, full_records[:n])
    Jh, eh = PL.evaluate(p, v0)
    assert rel(J, Jh) <= 1e-12
    assert np.all(J[PL.unused_entries(p)] == 0.0)
    want_e = PL.error_of_records(p, J, p.sam2_noise)
    assert abs(e - want_e) <= 1e-9 * want_e and abs(e - eh.sum()) <= 1e-9 * want_e
    prior_hd = np.zeros_like(hd); prior_hd[np.repeat(p.var_type == PL.POSE2, 3)] = 100.0
    assert rel(grad, PL.gradient_of_records(p, J)) <= 1e-10
    assert rel(hd, prior_hd + PL.gradient_of_records(p, np.concatenate([J[:, :18] ** 2, np.ones((n, 3))], 1))) <= 1e-10
    third = PL.third_entries(p)
    assert rc == 0 and abs(out[0] - 0.5 * float(J[:, 18:].ravel() @ J[:, 18:].ravel())) <= 1e-9 * out[0]
    assert np.all(d[third] == 0.0) and np.all(grad[third] == 0.0) and np.all(hd[third] == 0.0) and np.all(np.isfinite(d))


# ---- 4. the reference's example ---------------------------------------------------------------------------------------------
def test_planar_slam_example_converges_to_its_recorded_values(gpu, mixed):
    """examples/PlanarSLAMExample.cpp through the public Python surface: BearingRangeFactor2D -> LevenbergMarquardtOptimizer; the user
    sees 2-vectors."""
    from gtsam_amd import api as A
    from gtsam_amd import datasets as D
    _, _, g = mixed
    graph, initial = D.planar_slam_example()
    lm = A.LevenbergMarquardtOptimizer(graph, initial)
    assert abs(lm.error() - float(g["ex_error"])) <= 1e-9 * float(g["ex_error"])
    result = lm.optimize()
    assert lm.iterations() == int(g["ex_iterations"])
    assert lm.error() <= 1e-18 and float(g["ex_final_error"]) <= 1e-18          # a consistent toy: both reach zero to rounding
    L, X = A.symbol_shorthand.L, A.symbol_shorthand.X
    assert result.at(L(1)).shape == (2,) and result.at(L(2)).shape == (2,)
    packed = np.concatenate([np.append(result.at(L(j)), 0.0) for j in (1, 2)] + [result.at(X(i)).packed() for i in (1, 2, 3)])
    assert np.abs(packed - g["ex_final_values"]).max() <= 1e-5 * np.abs(g["ex_final_values"]).max()
    assert np.abs(packed - [2, 2, 0, 4, 2, 0, 0, 0, 0, 2, 0, 0, 4, 0, 0]).max() <= 1e-6
    lm._opt.dev.close()


def test_pcg_is_refused_on_a_planar_graph(gpu, mixed):
    p, v0, _ = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    with pytest.raises(gpu.GtsamAmdError, match="planar graph"):
        dev.try_lambda_pcg(1e-3, False)
    dev.close()
