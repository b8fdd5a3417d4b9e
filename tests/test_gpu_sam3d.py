"""GPU: BearingRangeFactor / RangeFactor / BearingFactor <Pose3, Point3> (gtsam/sam) on the device against the reference's recorded
answers (tests/golden/sam3d_mixed.npz, sam3d_slam.npz: tests/golden/make_golden_sam3d.py).

Tolerances are the project's, as stated at the top of tests/test_gpu_stereo.py, in the norm of tests/stereo_support.rel: records
<= 1e-12, Hessian diagonal / gradient <= 1e-10, the step of a damped solve <= 1e-7, errors <= 1e-9, LM trajectories the identical
accept / reject sequence with per-iteration errors <= 1e-6, final values <= 1e-5.  Both fixtures record trace_stable = 1 (the
reference takes the same accept / reject sequence under the reversed elimination ordering), so the identical sequence is demanded."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gtsam_amd.params import LevenbergMarquardtParams as LMP
from gtsam_amd.problem import NOISE_ISOTROPIC
from tests import sam_support as SS
from tests.sam_support import rel
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


@pytest.fixture(scope="module")
def mixed():
    g = SS.fixture("sam3d_mixed")
    return SS.problem_of(g), g["values0"], g


# ---- 1. fixture parity ------------------------------------------------------------------------------------------------------
def test_error_records_diagonal_gradient_vs_reference(gpu, mixed):
    p, v0, g = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    assert abs(e - float(g["error"])) <= 1e-9 * float(g["error"])
    dev.linearize()
    for ft in (5, 4, 1, 2, 3):
        J = dev.jacobians(ft)
        assert J.shape == g[f"jac{ft}"].shape
        assert rel(J, g[f"jac{ft}"]) <= 1e-12, ft
    assert rel(dev.hessian_diagonal(), g["hessian_diagonal"]) <= 1e-10
    assert rel(dev.gradient(), g["gradient"]) <= 1e-10
    dev.close()


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


# ---- 2. branch rows ---------------------------------------------------------------------------------------------------------
def test_branch_rows_and_zero_rows(gpu, mixed):
    """The recorded branch factors (bit-equal bearing, opposite bearing, axis tie, best axis x / y / z) give the fixture's b; the rows
    a range-only or bearing-only factor does not use are exactly 0."""
    p, v0, g = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    J = dev.jacobians(5)
    dev.close()
    scale = np.abs(g["jac5"][:, 27:]).max()
    for name in ("branch_same", "branch_opposite", "branch_tie", "axis_x", "axis_y", "axis_z"):
        k = int(g[name])
        assert np.abs(J[k, 27:] - g["jac5"][k, 27:]).max() <= 1e-12 * scale, name
        assert rel(J[k], g["jac5"][k]) <= 1e-12, name
    k = int(g["branch_opposite"])
    sigma = float(p.noise_data[p.noise_off[p.sam_noise[k]]])
    assert np.allclose(J[k, 27:29], [np.pi / sigma, 0.0], rtol=1e-15, atol=0)
    k = int(g["branch_same"])
    assert np.all(J[k, 27:29] == 0.0)
    A1, A2, b = J[:, :18].reshape(-1, 3, 6), J[:, 18:27].reshape(-1, 3, 3), J[:, 27:]
    rng_only, brg_only = p.sam_kind == 1, p.sam_kind == 2
    assert rng_only.any() and brg_only.any()
    assert np.all(A1[rng_only, 1:] == 0.0) and np.all(A2[rng_only, 1:] == 0.0) and np.all(b[rng_only, 1:] == 0.0)
    assert np.all(A1[brg_only, 2] == 0.0) and np.all(A2[brg_only, 2] == 0.0) and np.all(b[brg_only, 2] == 0.0)


# ---- 3. chunk boundaries ----------------------------------------------------------------------------------------------------
N_MONO_FRONT, N_STEREO_FRONT = 20, 17      # the 37 camera observations in front of the sam sub-range


def trimmed(g, n_sam, front):
    """The first n_sam sam factors of the fixture behind `front` (0 or 37) of its monocular / stereo factors, and a prior AT the
    initial value on every pose and landmark (zero residual: the priors add nothing to the error or the gradient, and keep the
    system definite)."""
    n_mono, n_stereo = (N_MONO_FRONT, N_STEREO_FRONT) if front else (0, 0)
    assert front in (0, N_MONO_FRONT + N_STEREO_FRONT)
    p = SS.problem_of(g, between_v1=[], between_v2=[], between_z=[], between_noise=[], prior_var=[], prior_off=[], prior_data=[], prior_noise=[])
    for f, w in (("proj_pose", 1), ("proj_point", 1), ("proj_z", 2), ("proj_noise", 1), ("proj_calib", 1), ("proj_sensor", 1)):
        setattr(p, f, getattr(p, f)[:w * n_mono].copy())
    for f, w in (("stereo_pose", 1), ("stereo_point", 1), ("stereo_z", 3), ("stereo_noise", 1), ("stereo_calib", 1), ("stereo_sensor", 1)):
        setattr(p, f, getattr(p, f)[:w * n_stereo].copy())
    for f, w in (("sam_kind", 1), ("sam_pose", 1), ("sam_point", 1), ("sam_z", 4), ("sam_noise", 1)):
        setattr(p, f, getattr(p, f)[:w * n_sam].copy())
    n6 = p.add_noise(NOISE_ISOTROPIC, 6, [0.1]); n3 = p.add_noise(NOISE_ISOTROPIC, 3, [0.1])
    off = p.val_offsets()
    for v in range(p.n_vars):
        p.add_prior(v, g["values0"][off[v]:off[v + 1]], n6 if p.var_type[v] == 0 else n3)
    return p


def sums_from_records(p, J5, J4, J1):
    """error and gradient J^T b of the sam / stereo / monocular factors from their whitened records (numpy, float64 sums)."""
    grad = np.zeros(int(p.dim_offsets()[-1])); doff = p.dim_offsets()
    err = 0.0
    for J, rows, pose, point, nzs in ((J5, 3, p.sam_pose, p.sam_point, p.sam_noise), (J4, 3, p.stereo_pose, p.stereo_point, p.stereo_noise),
                                      (J1, 2, p.proj_pose, p.proj_point, p.proj_noise)):
        for k in range(J.shape[0]):
            A1 = J[k, :6 * rows].reshape(rows, 6); A2 = J[k, 6 * rows:9 * rows].reshape(rows, 3); b = J[k, 9 * rows:]
            grad[doff[pose[k]]:doff[pose[k]] + 6] += A1.T @ b
            grad[doff[point[k]]:doff[point[k]] + 3] += A2.T @ b
            nz = int(nzs[k]); bb = float(b @ b); kk = float(p.noise_robust_param[nz])
            if p.noise_robust[nz] == 2:      # Huber: the record's b is sqrt(w) r with w = k / |r| outside the quadratic zone: |b|^2 = k |r|
                err += 0.5 * bb if bb <= kk * kk else kk * (bb / kk - kk / 2)
            elif p.noise_robust[nz] == 3:    # Cauchy: w = k^2 / (k^2 + |r|^2), so |r|^2 = |b|^2 k^2 / (k^2 - |b|^2); loss k^2 / 2 log1p(|r|^2 / k^2)
                err += 0.5 * kk * kk * np.log1p(bb / (kk * kk - bb))
            else:
                assert p.noise_robust[nz] == 0
                err += 0.5 * bb
    return err, grad


@pytest.mark.parametrize("front", [0, 37])
@pytest.mark.parametrize("n_sam", [1, 63, 64, 65, 257])
def test_chunk_boundaries(gpu, mixed, n_sam, front):
    """64 observations per wavefront, 256 per workgroup: the sam sub-range cut at 1, 63, 64, 65 and 257 factors, starting at
    observation 0 and at observation 37 (20 monocular and 17 stereo factors in front: off a multiple of 64).  The fixture's sam
    factors cycle through the three kinds, so every wavefront holds all of them."""
    _, v0, g = mixed
    p = trimmed(g, n_sam, front)
    if n_sam >= 3:
        assert all(set(p.sam_kind[c:c + 64]) == {0, 1, 2} for c in range(0, n_sam - 2, 64))
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    dev.linearize()
    J5, J4, J1 = dev.jacobians(5), dev.jacobians(4), dev.jacobians(1)
    grad = dev.gradient()
    rc, out = dev.try_lambda(1e-3, False)
    dev.close()
    assert J5.shape == (n_sam, 30) and J4.shape == (p.n_stereo, 30) and J1.shape == (p.n_proj, 20) and p.n_stereo + p.n_proj == front
    assert rel(J5, g["jac5"][:n_sam]) <= 1e-12
    if front:
        assert rel(J4, g["jac4"][:p.n_stereo]) <= 1e-12 and rel(J1, g["jac1"][:p.n_proj]) <= 1e-12
    want_e, want_g = sums_from_records(p, J5, J4, J1)
    assert abs(e - want_e) <= 1e-9 * want_e
    assert rel(grad, want_g) <= 1e-10
    assert rc == 0 and abs(out[0] - 0.5 * sum(float(J[:, -r:].ravel() @ J[:, -r:].ravel()) for J, r in ((J5, 3), (J4, 3), (J1, 2)))) <= 1e-9 * out[0]


# ---- 4. landmark SLAM without a camera --------------------------------------------------------------------------------------
def test_sam3d_slam(gpu):
    from gtsam_amd.optimizer import DeviceLevenbergMarquardt
    g = SS.fixture("sam3d_slam")
    p, v0 = SS.problem_of(g), g["values0"]
    n_poses = int((p.var_type == 0).sum())
    assert p.n_sam == 3000 and p.n_proj == 0 and p.n_stereo == 0 and p.calib.size == 0 and n_poses == 40 and p.n_vars == 340
    opt = DeviceLevenbergMarquardt(p, v0, LMP())
    # landmarks seen by bearing / range factors alone are eliminated as landmarks: the reduced system is the poses
    assert opt.dev.dim_size == 6 * n_poses + 3 * (p.n_vars - n_poses) and opt.dev.reduced_dim == 6 * n_poses
    h = opt.dev.structure_hash()
    assert h != 0
    assert abs(opt.error() - float(g["error"])) <= 1e-9 * float(g["error"])
    opt.dev.linearize()
    assert rel(opt.dev.jacobians(5), g["jac5"]) <= 1e-12
    assert rel(opt.dev.hessian_diagonal(), g["hessian_diagonal"]) <= 1e-10
    assert rel(opt.dev.gradient(), g["gradient"]) <= 1e-10
    check_solves(opt.dev, g)
    opt.optimize()
    check_trajectory(opt, g)
    opt.dev.close()
    # the same through the public Python surface: BearingRangeFactor3D / RangeFactor3D / BearingFactor3D -> LevenbergMarquardtOptimizer
    from gtsam_amd import api as A
    from gtsam_amd import datasets as D
    graph, initial = D.landmark_slam3d_graph()
    lm = A.LevenbergMarquardtOptimizer(graph, initial)
    assert lm._opt.dev.structure_hash() == h and lm._opt.dev.reduced_dim == 6 * n_poses
    result = lm.optimize()
    assert lm.iterations() == int(g["iterations"])
    tr = np.array(lm._opt.trace)[:, :3]
    assert tr.shape == g["trace"].shape and np.array_equal(tr[:, 0], g["trace"][:, 0]) and rel(tr[:, 1], g["trace"][:, 1]) <= 1e-6
    assert abs(lm.error() - g["trace"][-1, 1]) <= 1e-6 * g["trace"][-1, 1]
    packed = np.concatenate([result.at(k).packed() if hasattr(result.at(k), "packed") else result.at(k) for k in result.keys()])
    assert rel(packed, g["final_values"]) <= 1e-5
    lm._opt.dev.close()


# ---- 5. PCG, sharding, host analysis, reproducibility (the assertions of tests/test_gpu_stereo.py) ---------------------------
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
    """Landmark factors follow their landmark: tolerances of tests/test_gpu_sharding.py for its small cases."""
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


_STEP_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from gtsam_amd import lib as L
from tests import sam_support as SS
g = SS.fixture("sam3d_mixed")
dev = L.DeviceGraph(SS.problem_of(g))
dev.set_values(g["values0"])
dev.linearize()
rc, out = dev.try_lambda(1e-3, True)
np.savez(%(out)r, rc=rc, out=out, delta=dev.delta(), hash=dev.structure_hash(), hd=dev.hessian_diagonal(), grad=dev.gradient())
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
    for k in ("delta", "out", "hd", "grad"):
        assert np.array_equal(a[k], b[k]), k


def test_two_runs_identical_bits(gpu, mixed):
    p, v0, _ = mixed

    def run():
        dev = gpu.DeviceGraph(p)
        dev.set_values(v0)
        e = dev.error()
        dev.linearize()
        rc, out = dev.try_lambda(1e-3, False)
        rc2, out2 = dev.try_lambda(1e-4, True)
        r = (e, rc, out.copy(), rc2, out2.copy(), dev.delta().copy(), dev.jacobians(5).copy(), dev.jacobians(4).copy(), dev.hessian_diagonal().copy(),
             dev.gradient().copy())
        dev.close()
        return r

    a, b = run(), run()
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ---- 6. the paths without sam factors are untouched -------------------------------------------------------------------------
def test_three_row_step_without_sam_factors_equals_the_parent_commits(gpu):
    """stereo_mixed (three-row records, n_sam = 0) takes the kernels it took before: its records, sums, two damped steps and a PCG
    step are bit-equal to a recording made on the MI355X with the library of the parent commit
    (tests/golden/stereo_mixed_step_parent.npz).  The two-row path has the same test in tests/test_gpu_stereo.py
    (projection_small_step_parent.npz), which stays as it is."""
    rec = dict(np.load(os.path.join(ROOT, "tests", "golden", "stereo_mixed_step_parent.npz")))
    g = SS.fixture("stereo_mixed")
    got = record_step(gpu, SS.problem_of(g), g["values0"], jac_types=(1, 2, 3, 4))
    assert set(got) == set(rec)
    for k in got:
        assert np.array_equal(np.asarray(got[k]), rec[k]), k


def test_three_row_step_with_sam_factors_equals_the_parent_commits(gpu, mixed):
    """sam3d_mixed (40 monocular + 90 stereo + 301 bearing / range observations: both sub-range boundaries and the end inside a
    64-factor chunk, two workgroups, robust rows) through k_lin_rows3<true> / k_error_rows3<true>: bit-equal to a recording made on the
    MI355X with the library of the commit before the two kernels became instantiations (tests/golden/sam3d_mixed_step_parent.npz;
    recorded twice in two processes, every key agreed)."""
    p, v0, _ = mixed
    rec = dict(np.load(os.path.join(ROOT, "tests", "golden", "sam3d_mixed_step_parent.npz")))
    got = record_step(gpu, p, v0, jac_types=(1, 2, 3, 4, 5))
    assert set(got) == set(rec)
    for k in got:
        assert np.array_equal(np.asarray(got[k]), rec[k]), k
