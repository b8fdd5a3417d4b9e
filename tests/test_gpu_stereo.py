"""GPU: GenericStereoFactor<Pose3, Point3> on the device against the reference's recorded answers (tests/golden/stereo_mixed.npz,
stereo_vo_large.npz: tests/golden/make_golden_stereo.py).

Tolerances are the project's (tests/test_gpu_parity.py): records <= 1e-12 relative, Hessian diagonal / gradient <= 1e-10, the step
of a damped solve <= 1e-7 (max-norm, relative), errors <= 1e-9, LM trajectories the identical accept / reject sequence with
per-iteration errors <= 1e-6, final values <= 1e-5.  Both fixtures record trace_stable = 1 (the reference takes the same
accept / reject sequence under the reversed elimination ordering), so the identical sequence is demanded."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from gtsam_amd.params import LevenbergMarquardtParams as LMP
from gtsam_amd.problem import NOISE_ISOTROPIC
from tests import problems as PB
from tests import stereo_support as S
from tests.step_recording import record_step
from tests.stereo_support import rel

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
    g = S.fixture("stereo_mixed")
    return S.problem_of(g), g["values0"], g


# ---- 1. fixture parity ------------------------------------------------------------------------------------------------------
def test_error_records_diagonal_gradient_vs_reference(gpu, mixed):
    p, v0, g = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    assert abs(e - float(g["error"])) <= 1e-9 * float(g["error"])
    dev.linearize()
    for ft in (4, 1, 2, 3):
        J = dev.jacobians(ft)
        assert J.shape == g[f"jac{ft}"].shape
        assert rel(J, g[f"jac{ft}"]) <= 1e-12, ft
    assert rel(dev.hessian_diagonal(), g["hessian_diagonal"]) <= 1e-10
    assert rel(dev.gradient(), g["gradient"]) <= 1e-10
    dev.close()


def check_solves(dev, g):
    for i in range(2):
        lam, dd = float(g[f"solve{i}_lambda"]), bool(g[f"solve{i}_diag"])
        rc, out = dev.try_lambda(lam, dd)
        assert rc == int(g[f"solve{i}_status"]) == 0
        assert rel(dev.delta(), g[f"solve{i}_delta"]) <= 1e-7, (i, rel(dev.delta(), g[f"solve{i}_delta"]))
        le = g[f"solve{i}_linerr"]
        assert abs(out[0] - le[0]) <= 1e-9 * abs(le[0])
        assert abs(out[1] - le[1]) <= 1e-7 * max(abs(le[1]), 1e-12 * abs(le[0]))
        assert rel(dev.trial_values(), g[f"solve{i}_retract"]) <= 1e-7
        te = float(g[f"solve{i}_trial_error"])
        if out[0] - out[1] >= 0:
            assert abs(out[2] - te) <= 1e-6 * abs(te)


def test_damped_solves_vs_reference(gpu, mixed):
    p, v0, g = mixed
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    check_solves(dev, g)
    dev.close()


def check_trajectory(opt, g):
    ref = g["trace"]
    tr = np.array(opt.trace)[:, :3]
    assert int(g["trace_stable"]) == 1
    assert tr.shape == ref.shape and np.array_equal(tr[:, 0], ref[:, 0]), (tr, ref)
    assert rel(tr[:, 1], ref[:, 1]) <= 1e-6
    assert np.allclose(tr[:, 2], ref[:, 2], rtol=1e-6, atol=0)
    assert opt.iterations() == int(g["iterations"])
    assert rel(opt.values_packed(), g["final_values"]) <= 1e-5


def test_lm_trajectory_vs_reference(gpu, mixed):
    from gtsam_amd.optimizer import DeviceLevenbergMarquardt
    p, v0, g = mixed
    opt = DeviceLevenbergMarquardt(p, v0, LMP())
    opt.optimize()
    check_trajectory(opt, g)
    opt.dev.close()


# ---- 2. cheirality ----------------------------------------------------------------------------------------------------------
def test_cheirality_rows(gpu, mixed):
    """The landmark behind its camera: zero Jacobians, b = -whiten(Vector3::Constant(2 fx)) (StereoFactor.h:144-153)."""
    p, v0, g = mixed
    k = int(g["behind"])
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    J = dev.jacobians(4)
    dev.close()
    zero = np.flatnonzero(np.abs(J[:, :27]).sum(1) == 0)
    assert k in zero and np.array_equal(zero, np.flatnonzero(np.abs(g["jac4"][:, :27]).sum(1) == 0))
    for f in zero:
        nz = int(p.stereo_noise[f]); o = int(p.noise_off[nz]); nd = S.device_noise_data(p)
        r = np.full(3, 2.0 * p.calib.reshape(-1, 5)[p.stereo_calib[f], 0])
        w = {0: r, 1: r * nd[o], 2: r * nd[o:o + 3], 3: nd[o:o + 9].reshape(3, 3) @ r}[int(p.noise_kind[nz])]
        if p.noise_robust[nz]:      # Huber, Block scheme: the record scaled by sqrt(weight(|whitened b|))
            d = np.linalg.norm(w); kk = float(p.noise_robust_param[nz])
            w = w * np.sqrt(1.0 if d <= kk else kk / d)
        assert rel(J[f, 27:], -w) <= 1e-12


# ---- 3. chunk boundaries ----------------------------------------------------------------------------------------------------
def trimmed(g, n_stereo, n_mono):
    """The first n_stereo stereo factors of the fixture behind its first n_mono monocular ones, and a prior AT the initial value on
    every pose and landmark (zero residual: the priors add nothing to the error or the gradient, and keep the system definite)."""
    p = S.problem_of(g, between_v1=[], between_v2=[], between_z=[], between_noise=[], prior_var=[], prior_off=[], prior_data=[], prior_noise=[])
    for f, w in (("proj_pose", 1), ("proj_point", 1), ("proj_z", 2), ("proj_noise", 1), ("proj_calib", 1), ("proj_sensor", 1)):
        setattr(p, f, getattr(p, f)[:w * n_mono].copy())
    for f, w in (("stereo_pose", 1), ("stereo_point", 1), ("stereo_z", 3), ("stereo_noise", 1), ("stereo_calib", 1), ("stereo_sensor", 1)):
        setattr(p, f, getattr(p, f)[:w * n_stereo].copy())
    n6 = p.add_noise(NOISE_ISOTROPIC, 6, [0.1]); n3 = p.add_noise(NOISE_ISOTROPIC, 3, [0.1])
    off = p.val_offsets()
    for v in range(p.n_vars):
        p.add_prior(v, g["values0"][off[v]:off[v + 1]], n6 if p.var_type[v] == 0 else n3)
    return p


def sums_from_records(p, J4, J1):
    """error and gradient J^T b of the stereo / monocular factors from their whitened records (numpy, float64 sums)."""
    grad = np.zeros(int(p.dim_offsets()[-1])); doff = p.dim_offsets()
    err = 0.0
    for J, rows, pose, point, nzs in ((J4, 3, p.stereo_pose, p.stereo_point, p.stereo_noise), (J1, 2, p.proj_pose, p.proj_point, p.proj_noise)):
        for k in range(J.shape[0]):
            A1 = J[k, :6 * rows].reshape(rows, 6); A2 = J[k, 6 * rows:9 * rows].reshape(rows, 3); b = J[k, 9 * rows:]
            grad[doff[pose[k]]:doff[pose[k]] + 6] += A1.T @ b
            grad[doff[point[k]]:doff[point[k]] + 3] += A2.T @ b
            nz = int(nzs[k])
            if p.noise_robust[nz]:      # Huber: the record's b is sqrt(w) r with w = k / |r| outside the quadratic zone: |b|^2 = k |r|
                kk = float(p.noise_robust_param[nz]); bb = float(b @ b)
                err += 0.5 * bb if bb <= kk * kk else kk * (bb / kk - kk / 2)
            else:
                err += 0.5 * float(b @ b)
    return err, grad


@pytest.mark.parametrize("n_mono", [0, 37])
@pytest.mark.parametrize("n_stereo", [1, 63, 64, 65, 257])
def test_chunk_boundaries(gpu, mixed, n_stereo, n_mono):
    """64 observations per wavefront, 256 per workgroup: the stereo range cut at 1, 63, 64, 65 and 257 factors, starting at
    observation 0 and at observation 37 (off a multiple of 64)."""
    _, v0, g = mixed
    p = trimmed(g, n_stereo, n_mono)
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    dev.linearize()
    J4, J1 = dev.jacobians(4), dev.jacobians(1)
    grad = dev.gradient()
    rc, out = dev.try_lambda(1e-3, False)
    dev.close()
    assert J4.shape == (n_stereo, 30) and J1.shape == (n_mono, 20)
    assert rel(J4, g["jac4"][:n_stereo]) <= 1e-12
    if n_mono:
        assert rel(J1, g["jac1"][:n_mono]) <= 1e-12
    want_e, want_g = sums_from_records(p, J4, J1)
    assert abs(e - want_e) <= 1e-9 * want_e
    assert rel(grad, want_g) <= 1e-10
    assert rc == 0 and abs(out[0] - 0.5 * sum(float(J[:, -r:].ravel() @ J[:, -r:].ravel()) for J, r in ((J4, 3), (J1, 2)))) <= 1e-9 * out[0]


# ---- 4. PCG -----------------------------------------------------------------------------------------------------------------
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


# ---- 5. sharding ------------------------------------------------------------------------------------------------------------
def run_two_shards(body):
    from tests.test_gpu_sharding import TwoWaySum
    sumr = TwoWaySum()
    res = [None, None]

    def run(rank):
        try:
            res[rank] = body(rank, sumr.fn(rank))
        except Exception as e:  # noqa: BLE001
            res[rank] = e
            sumr.barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    for r in res:
        assert not isinstance(r, Exception), r
    return res


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


# ---- 6. host against device analysis ----------------------------------------------------------------------------------------
_STEP_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from gtsam_amd import lib as L
from tests import stereo_support as S
g = S.fixture("stereo_mixed")
dev = L.DeviceGraph(S.problem_of(g))
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


# ---- 7. two runs, identical bits --------------------------------------------------------------------------------------------
def test_two_runs_identical_bits(gpu, mixed):
    p, v0, _ = mixed

    def run():
        dev = gpu.DeviceGraph(p)
        dev.set_values(v0)
        e = dev.error()
        dev.linearize()
        rc, out = dev.try_lambda(1e-3, False)
        rc2, out2 = dev.try_lambda(1e-4, True)
        r = (e, rc, out.copy(), rc2, out2.copy(), dev.delta().copy(), dev.jacobians(4).copy(), dev.hessian_diagonal().copy(), dev.gradient().copy())
        dev.close()
        return r

    a, b = run(), run()
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ---- 8. examples/StereoVOExample_large.cpp ----------------------------------------------------------------------------------
def test_stereo_vo_large(gpu):
    from gtsam_amd.optimizer import DeviceLevenbergMarquardt
    g = S.fixture("stereo_vo_large")
    p, v0 = S.vo_problem()
    n_poses = int((p.var_type == 0).sum())
    assert p.n_stereo == 8189 and p.n_proj == 0 and n_poses == 26 and p.n_vars == 2660      # (the pose file lists 26 poses)
    opt = DeviceLevenbergMarquardt(p, v0, LMP())
    assert opt.dev.dim_size == 6 * n_poses + 3 * (p.n_vars - n_poses) and opt.dev.reduced_dim == 6 * n_poses
    h = opt.dev.structure_hash()
    assert h != 0
    assert abs(opt.error() - float(g["error"])) <= 1e-9 * float(g["error"])
    opt.dev.linearize()
    assert rel(opt.dev.jacobians(4)[g["jac4_rows"]], g["jac4"]) <= 1e-12
    assert rel(opt.dev.hessian_diagonal(), g["hessian_diagonal"]) <= 1e-10
    assert rel(opt.dev.gradient(), g["gradient"]) <= 1e-10
    check_solves(opt.dev, g)
    opt.optimize()
    check_trajectory(opt, g)
    opt.dev.close()
    # the same through the public Python surface: GenericStereoFactor3D -> LevenbergMarquardtOptimizer
    from gtsam_amd import api as A
    graph, initial = S.vo_graph()
    lm = A.LevenbergMarquardtOptimizer(graph, initial)
    assert lm._opt.dev.structure_hash() == h
    result = lm.optimize()
    assert lm.iterations() == int(g["iterations"])
    assert abs(lm.error() - g["trace"][-1, 1]) <= 1e-6 * g["trace"][-1, 1]
    packed = np.concatenate([result.at(k).packed() if hasattr(result.at(k), "packed") else result.at(k) for k in result.keys()])
    assert rel(packed, g["final_values"]) <= 1e-5
    lm._opt.dev.close()


# ---- 9. the path without stereo factors is untouched ------------------------------------------------------------------------
def test_no_stereo_step_equals_the_parent_commits(gpu):
    """projection_small (n_stereo = 0) takes the kernels it took before: its records, sums and two damped steps are bit-equal to a
    recording made on the MI355X with the library of the parent commit (tests/golden/projection_small_step_parent.npz)."""
    rec = dict(np.load(os.path.join(ROOT, "tests", "golden", "projection_small_step_parent.npz")))
    got = record_step(gpu, *PB.SYNTH["projection_small"](), jac_types=(1, 3))
    assert set(got) == set(rec)
    for k in got:
        assert np.array_equal(np.asarray(got[k]), rec[k]), k
