"""GPU: PoseTranslationPrior / PoseRotationPrior <Pose3 | Pose2> (gtsam/slam) on the device against the reference's recorded answers
(tests/golden/pose_partial_graph3d.npz, pose_partial_vo.npz, pose_partial_graph2d.npz: tests/golden/make_golden_pose_partial.py).

Tolerances are the project's, as stated at the top of tests/test_gpu_stereo.py, in the norm of tests/stereo_support.rel: records
<= 1e-12, Hessian diagonal / gradient <= 1e-10, the step of a damped solve <= 1e-7, errors <= 1e-9, LM trajectories the identical
accept / reject sequence with per-iteration errors <= 1e-6, final values <= 1e-5.  Every fixture records trace_stable = 1 (the
reference takes the same accept / reject sequence under the reversed elimination ordering), so the identical sequence is demanded.
No graph here has a full PriorFactor: the gauge is fixed by the partial priors alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gtsam_amd.params import LevenbergMarquardtParams as LMP
from tests import pose_partial_support as PS
from tests.pose_partial_support import rel
from tests.step_recording import record_step
from tests.test_gpu_stereo import check_solves, check_trajectory, run_two_shards

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gtsam_amd import lib
    lib.load()
    return lib


def case(name):
    g = PS.fixture(name)
    return PS.problem_of(g), g["values0"], g


# ---- 1. fixture parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PS.FIXTURES)
def test_error_records_diagonal_gradient_vs_reference(gpu, name):
    p, v0, g = case(name)
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    assert abs(e - float(g["error"])) <= 1e-9 * float(g["error"])
    dev.linearize()
    types = [ft for ft in (6, 2, 1) if f"jac{ft}" in g]
    assert 6 in types and 2 in types and (1 in types) == (name == "pose_partial_vo")      # all factor types present
    for ft in types:
        J = dev.jacobians(ft)
        assert J.shape == g[f"jac{ft}"].shape
        assert rel(J, g[f"jac{ft}"]) <= 1e-12, ft
    J6, J3 = dev.jacobians(6), dev.jacobians(3)
    assert J3.shape == (0, 90)                           # GTG_FAC_PRIOR: the caller's PriorFactors and nothing else
    assert np.all(J6[PS.unused_entries(p)] == 0.0)       # the rows a factor does not have are exactly 0
    assert rel(dev.hessian_diagonal(), g["hessian_diagonal"]) <= 1e-10
    dev.close()


@pytest.mark.parametrize("name", PS.FIXTURES)
def test_gradient_vs_reference(gpu, name):
    """The reference's -gradientAtZero of the linearised graph, <= 1e-10: gtg_get_graph_gradient.  In the smart-VO fixture the
    reference's smart factors are Hessian factors with their landmark eliminated, so their poses' blocks carry
    F^T b - F^T E (E^T E)^-1 E^T b; gtg_get_gradient returns J^T b of the records BEFORE the hidden landmarks are eliminated (measured on
    the MI355X: 1.3e-2 from the reference on pose_partial_vo, equal on the two pose graphs), which is why the smart fixtures of
    tests/golden/make_golden_smart_pose.py record no gradient.  Without smart factors the two getters return the same bits."""
    p, v0, g = case(name)
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    got, plain = dev.graph_gradient(), dev.gradient()
    dev.close()
    print(name, "gradient vs reference:", rel(got, g["gradient"]), "J^T b before elimination:", rel(plain, g["gradient"]))
    assert rel(got, g["gradient"]) <= 1e-10
    if p.n_smart == 0:
        assert np.array_equal(got, plain)
    else:
        lm = np.repeat(p.var_type == 2, [3 if t == 2 else 6 for t in p.var_type])
        assert np.array_equal(got[lm], plain[lm]) and not np.array_equal(got[~lm], plain[~lm])    # the explicit landmarks keep J^T b


@pytest.mark.parametrize("name", PS.FIXTURES)
def test_damped_solves_vs_reference(gpu, name):
    p, v0, g = case(name)
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    check_solves(dev, g)
    dev.close()


@pytest.mark.parametrize("name", PS.FIXTURES)
def test_lm_trajectory_vs_reference(gpu, name):
    from gtsam_amd.optimizer import DeviceLevenbergMarquardt
    p, v0, g = case(name)
    opt = DeviceLevenbergMarquardt(p, v0, LMP())
    opt.optimize()
    check_trajectory(opt, g)
    assert g["trace"][-1, 1] < g["trace"][0, 1]
    opt.dev.close()


def test_branch_and_wrap_rows(gpu):
    """The recorded branch factors of SO3::Logmap and the Pose2 rotation prior across the +-pi cut give the fixture's b."""
    p, v0, g = case("pose_partial_graph3d")
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    J = dev.jacobians(6)
    dev.close()
    scale = np.abs(g["jac6"][:, 81:]).max()
    assert set(g["rot_branch"][g["rot_branch"] >= 0]) == {0, 1, 2}
    for branch in (0, 1, 2):
        rows = np.flatnonzero(g["rot_branch"] == branch)
        assert np.abs(J[rows, 81:] - g["jac6"][rows, 81:]).max() <= 1e-12 * scale, branch
    rot = p.pose_partial_kind == 1
    sig_free = J[rot][:, :18].reshape(-1, 3, 6)          # H = [I | 0] whitened: the translation columns stay exactly 0
    assert np.all(sig_free[:, :, 3:] == 0.0)
    p, v0, g = case("pose_partial_graph2d")
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    J = dev.jacobians(6)
    dev.close()
    k = int(g["wrap"]); nz = int(p.pose_partial_noise[k])
    sigma = 1.0 if p.noise_kind[nz] == 0 else float(p.noise_data[p.noise_off[nz]])
    assert abs(-J[k, 81] * sigma - (2 * np.pi - 6.2)) <= 1e-12      # 0.083, not -6.2
    assert abs(J[k, 81] - g["jac6"][k, 81]) <= 1e-12 * np.abs(g["jac6"][:, 81:]).max()


def test_python_surface_runs_the_same_trajectory(gpu):
    """PoseTranslationPrior2D / PoseRotationPrior2D -> extract -> LevenbergMarquardtOptimizer, the way user code reads."""
    from gtsam_amd import api as A
    g = PS.fixture("pose_partial_graph2d")
    graph, initial, _ = PS.scene("pose_partial_graph2d")
    lm = A.LevenbergMarquardtOptimizer(graph, initial)
    result = lm.optimize()
    assert lm.iterations() == int(g["iterations"])
    tr = np.array(lm._opt.trace)[:, :3]
    assert tr.shape == g["trace"].shape and np.array_equal(tr[:, 0], g["trace"][:, 0]) and rel(tr[:, 1], g["trace"][:, 1]) <= 1e-6
    packed = np.concatenate([result.at(k).packed() for k in result.keys()])
    assert rel(packed, g["final_values"]) <= 1e-5
    lm._opt.dev.close()


# ---- 2. PCG, sharding, host analysis (the assertions of tests/test_gpu_sam3d.py) ----------------------------------------------
def test_pcg_equals_direct_solve(gpu):
    p, v0, _ = case("pose_partial_graph3d")
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


@pytest.mark.parametrize("name", ["pose_partial_graph3d", "pose_partial_vo"])
def test_two_shards_equal_one(gpu, name):
    """The partial priors are dealt round-robin like the other non-landmark factors: tolerances of tests/test_gpu_sharding.py for its
    small cases."""
    from gtsam_amd.optimizer import DeviceLevenbergMarquardt
    p, v0, g = case(name)
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
    single.dev.close()


_STEP_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from gtsam_amd import lib as L
from tests import pose_partial_support as PS
g = PS.fixture("pose_partial_vo")
dev = L.DeviceGraph(PS.problem_of(g))
dev.set_values(g["values0"])
e = dev.error()
dev.linearize()
rc, out = dev.try_lambda(1e-3, True)
np.savez(%(out)r, e=e, rc=rc, out=out, delta=dev.delta(), hash=dev.structure_hash(), hd=dev.hessian_diagonal(), grad=dev.gradient(), jac6=dev.jacobians(6))
dev.close()
"""


def step_in_child(tmp_path, tag, env_extra):
    out = str(tmp_path / f"step_{tag}.npz")
    env = dict(os.environ); env.pop("GTG_HOST_ANALYSIS", None); env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _STEP_CHILD % {"root": ROOT, "out": out}], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def test_host_analysis_equals_device_analysis(gpu, tmp_path):
    a = step_in_child(tmp_path, "device", {})
    b = step_in_child(tmp_path, "host", {"GTG_HOST_ANALYSIS": "1"})
    assert int(a["rc"]) == int(b["rc"]) == 0 and int(a["hash"]) == int(b["hash"])
    for k in ("e", "delta", "out", "hd", "grad", "jac6"):
        assert np.array_equal(a[k], b[k]), k


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------
def upload_error(gpu, cp):
    """The text gtg_upload_problem leaves for this C struct (it must refuse)."""
    lib = gpu.load()
    h = C.c_void_p()
    assert lib.gtg_create(C.byref(h), 0) == 0
    rc = lib.gtg_upload_problem(h, C.byref(cp), 0, 1)
    msg = lib.gtg_last_error().decode()
    lib.gtg_destroy(h)
    assert rc < 0, "the upload was accepted"
    return msg


def test_upload_refusals_by_message(gpu):
    p, v0, g = case("pose_partial_vo")
    T = int(np.flatnonzero(p.pose_partial_kind == 0)[0]); R = int(np.flatnonzero(p.pose_partial_kind == 1)[0])
    point = int(np.flatnonzero(p.var_type == 2)[0])

    def broken(field, index, value):
        q = PS.problem_of(g)
        a = getattr(q, field).copy(); a[index] = value
        setattr(q, field, a)
        return upload_error(gpu, q.to_ctypes())

    assert "unknown pose_partial_kind" in broken("pose_partial_kind", T, 2)
    assert "unknown pose_partial_kind" in broken("pose_partial_kind", R, -1)
    assert "PoseTranslationPrior: its key must be a POSE3 or POSE2 variable" in broken("pose_partial_var", T, point)
    assert "PoseRotationPrior: its key must be a POSE3 or POSE2 variable" in broken("pose_partial_var", R, p.n_vars)
    assert "PoseTranslationPrior: its key must be a POSE3 or POSE2 variable" in broken("pose_partial_var", T, -1)
    n2 = int(np.flatnonzero(p.noise_dim == 2)[0]); n6 = int(np.flatnonzero(p.noise_dim == 6)[0])
    assert "PoseTranslationPrior: NoiseModel has wrong dimension" in broken("pose_partial_noise", T, n2)
    assert "PoseRotationPrior: NoiseModel has wrong dimension" in broken("pose_partial_noise", R, n6)
    assert "PoseRotationPrior: NoiseModel has wrong dimension" in broken("pose_partial_noise", R, p.noise_kind.size)
    # Pose2: a translation prior has two rows, a rotation prior one
    p2, _, g2 = case("pose_partial_graph2d")
    q = PS.problem_of(g2)
    T2 = int(np.flatnonzero(q.pose_partial_kind == 0)[0]); R2 = int(np.flatnonzero(q.pose_partial_kind == 1)[0])
    a = q.pose_partial_noise.copy(); a[T2] = q.pose_partial_noise[R2]; q.pose_partial_noise = a
    assert "PoseTranslationPrior: NoiseModel has wrong dimension" in upload_error(gpu, q.to_ctypes())
    # n_pose_partial > 0 with a table missing
    for name in ("pose_partial_kind", "pose_partial_var", "pose_partial_z", "pose_partial_noise"):
        cp = PS.problem_of(g).to_ctypes()
        setattr(cp, name, C.cast(None, type(getattr(cp, name))))
        assert "partial pose prior tables missing" in upload_error(gpu, cp), name
    # and the unbroken tables upload
    dev = gpu.DeviceGraph(PS.problem_of(g))
    dev.close()


# ---- 4. the paths without partial priors are untouched ----------------------------------------------------------------------
def test_a_graph_without_partial_priors_gives_the_records_it_gave(gpu):
    """sam3d_mixed with empty partial tables (count 0, NULL pointers): bit-equal to the recording made on the MI355X with an earlier
    library (tests/golden/sam3d_mixed_step_parent.npz, the recording tests/test_gpu_sam3d.py holds the same step to), and
    gtg_get_jacobians(GTG_FAC_POSE_PARTIAL) returns nothing."""
    g = PS.fixture("sam3d_mixed")
    p = PS.problem_of(g)
    assert p.n_pose_partial == 0 and p.n_prior > 0
    rec = dict(np.load(os.path.join(ROOT, "tests", "golden", "sam3d_mixed_step_parent.npz")))
    got = record_step(gpu, p, g["values0"], jac_types=(1, 2, 3, 4, 5))
    assert set(got) == set(rec)
    for k in got:
        assert np.array_equal(np.asarray(got[k]), rec[k]), k
    dev = gpu.DeviceGraph(p)
    dev.set_values(g["values0"])
    dev.linearize()
    assert dev.jacobians(6).shape == (0, 90) and dev.jacobians(3).shape == (p.n_prior, 90)
    dev.close()


def test_full_priors_and_partial_priors_side_by_side(gpu):
    """A PriorFactor<Pose3> in front of the partial priors: GTG_FAC_PRIOR returns the one record, GTG_FAC_POSE_PARTIAL the fixture's, and
    the error is the fixture's plus the prior's 0.5 |b|^2."""
    from gtsam_amd.problem import NOISE_ISOTROPIC
    p, v0, g = case("pose_partial_graph3d")
    n6 = p.add_noise(NOISE_ISOTROPIC, 6, [0.5])
    prior = np.array(v0[12:24]); prior[9:] += [0.3, -0.2, 0.1]
    p.add_prior(1, prior, n6)
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    dev.linearize()
    J3, J6 = dev.jacobians(3), dev.jacobians(6)
    dev.close()
    assert J3.shape == (1, 90) and rel(J6, g["jac6"]) <= 1e-12
    assert np.array_equal(J3[0, :36].reshape(6, 6), np.eye(6) / 0.5)
    want = float(g["error"]) + 0.5 * float(J3[0, 81:87] @ J3[0, 81:87])
    assert abs(e - want) <= 1e-9 * want
