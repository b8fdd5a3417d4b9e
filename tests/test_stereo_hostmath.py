"""GenericStereoFactor<Pose3, Point3> on the CPU: stereo_linearize / stereo_error of gtsam_amd/csrc/factors.h compiled for the host
(tests/hostmath/hostmath_stereo.cpp) against the reference's records in the fixtures of tests/golden/make_golden_stereo.py.

Tolerances: records <= 1e-12 relative (the same formulas, rounding only); Jacobians against central differences of the evaluator's
own residual <= 1e-6 (step 1e-6 on entries of order 1e2 - 1e3: truncation h^2 and rounding eps / h both stay below that)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import stereo_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hm():
    so = os.path.join(ROOT, "tests", "_build", "libhostmath_stereo.so")
    src = os.path.join(ROOT, "tests", "hostmath", "hostmath_stereo.cpp")
    deps = [src, os.path.join(ROOT, "gtsam_amd", "csrc", "factors.h"), os.path.join(ROOT, "gtsam_amd", "csrc", "geom.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.hms_stereo.argtypes = [C.c_long] + [C.c_void_p] * 19
    lib.hms_proj_rows3.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p]
    assert lib.hms_record_size() == 30
    return lib


def evaluate(hm, p, values, rows=None):
    """(records, errors, whitened residuals) of the stereo factors `rows` of p at `values`."""
    rows = np.arange(p.n_stereo) if rows is None else np.asarray(rows)
    n = rows.size
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    pose, pt, nz, ci = i32(p.stereo_pose[rows]), i32(p.stereo_point[rows]), i32(p.stereo_noise[rows]), i32(p.stereo_calib[rows])
    si = i32(p.stereo_sensor[rows]) if p.stereo_sensor.size else np.full(n, -1, np.int32)
    z = np.ascontiguousarray(p.stereo_z.reshape(-1, 3)[rows])
    values = np.ascontiguousarray(values, np.float64)
    voff, nd = p.val_offsets(), S.device_noise_data(p)
    rk, rp = i32(p.noise_robust), np.ascontiguousarray(p.noise_robust_param, np.float64)
    sensor = np.ascontiguousarray(p.sensor if p.sensor.size else np.zeros(12))
    J, e, r = np.zeros((n, 30)), np.zeros(n), np.zeros((n, 3))
    hm.hms_stereo(n, pose.ctypes.data, pt.ctypes.data, z.ctypes.data, nz.ctypes.data, ci.ctypes.data, si.ctypes.data, p.calib.ctypes.data,
                  p.calib_baseline.ctypes.data, sensor.ctypes.data, values.ctypes.data, voff.ctypes.data, p.noise_kind.ctypes.data,
                  p.noise_off.ctypes.data, nd.ctypes.data, rk.ctypes.data, rp.ctypes.data, J.ctypes.data, e.ctypes.data, r.ctypes.data)
    return J, e, r


def test_records_equal_the_reference_on_stereo_mixed(hm):
    g = S.fixture("stereo_mixed")
    p = S.problem_of(g)
    J, e, _ = evaluate(hm, p, g["values0"])
    assert J.shape == g["jac4"].shape
    assert S.rel(J, g["jac4"]) <= 1e-12
    # every noise kind, the m-estimator, both calibrations and the sensor transform are among them
    assert set(p.noise_kind[p.stereo_noise]) == {0, 1, 2, 3} and (p.noise_robust[p.stereo_noise] == 2).any()
    assert len(set(p.stereo_calib)) == 2
    assert (p.stereo_sensor >= 0).any() and (p.stereo_sensor < 0).any()


def test_records_equal_the_reference_on_stereo_vo_large(hm):
    g = S.fixture("stereo_vo_large")
    p, v0 = S.vo_problem()
    assert np.array_equal(v0, g["values0"]) and p.n_stereo == 8189
    J, _, _ = evaluate(hm, p, v0, g["jac4_rows"])
    assert S.rel(J, g["jac4"]) <= 1e-12


def test_factor_errors_sum_to_the_graph_error_of_a_stereo_only_graph(hm):
    """stereo_vo_large is stereo factors and one prior whose residual is zero at the initial values."""
    g = S.fixture("stereo_vo_large")
    p, v0 = S.vo_problem()
    _, e, _ = evaluate(hm, p, v0)
    assert abs(e.sum() - float(g["error"])) <= 1e-9 * float(g["error"])


def test_cheirality_zero_jacobians_and_constant_residual(hm):
    g = S.fixture("stereo_mixed")
    p = S.problem_of(g)
    k = int(g["behind"])
    J, e, r = evaluate(hm, p, g["values0"], [k])
    fx = p.calib.reshape(-1, 5)[p.stereo_calib[k], 0]
    assert np.all(J[0, :27] == 0.0)
    # b = -whiten(2 fx 1) (times the m-estimator's weight where the factor has one): the reference's record, and the residual below
    if p.noise_robust[p.stereo_noise[k]] == 0:
        assert np.array_equal(J[0, 27:], -r[0])
    assert S.rel(J[0], g["jac4"][k]) <= 1e-12
    unwhitened = np.full(3, 2.0 * fx)
    nz = int(p.stereo_noise[k]); nd = S.device_noise_data(p); o = int(p.noise_off[nz])
    want = {0: unwhitened, 1: unwhitened * nd[o], 2: unwhitened * nd[o:o + 3], 3: nd[o:o + 9].reshape(3, 3) @ unwhitened}[int(p.noise_kind[nz])]
    assert np.allclose(r[0], want, rtol=1e-15, atol=0)


def test_skew_is_ignored(hm):
    g = S.fixture("stereo_mixed")
    p = S.problem_of(g)
    rows = np.flatnonzero(p.calib.reshape(-1, 5)[p.stereo_calib, 2] != 0.0)
    assert rows.size > 0, "the fixture has a Cal3_S2Stereo with skew"
    J0, e0, _ = evaluate(hm, p, g["values0"], rows)
    q = S.problem_of(g)
    c = q.calib.reshape(-1, 5).copy(); c[:, 2] = 0.0; q.calib = c.reshape(-1)
    J1, e1, _ = evaluate(hm, q, g["values0"], rows)
    assert np.array_equal(J0, J1) and np.array_equal(e0, e1)
    assert S.rel(J0, g["jac4"][rows]) <= 1e-12


def test_jacobians_against_central_differences(hm):
    """Unweighted factors in front of their camera (an m-estimator scales the record by a weight that is not part of the derivative)."""
    from oracle import gtsam_oracle as O
    g = S.fixture("stereo_mixed")
    p = S.problem_of(g)
    v0 = np.array(g["values0"])
    J, _, r0 = evaluate(hm, p, v0)
    plain = np.flatnonzero((p.noise_robust[p.stereo_noise] == 0) & (np.abs(J[:, :27]).sum(1) > 0))
    rows = np.concatenate([plain[:6], plain[plain.size // 2:plain.size // 2 + 6], plain[-6:]])
    assert (p.stereo_sensor[rows] >= 0).any() and (p.stereo_sensor[rows] < 0).any()
    voff, doff = p.val_offsets(), p.dim_offsets()
    h = 1e-6
    for k in rows:
        for var, col0, d in ((int(p.stereo_pose[k]), 0, 6), (int(p.stereo_point[k]), 18, 3)):
            A = J[k, col0:col0 + 3 * d].reshape(3, d)
            num = np.zeros((3, d))
            for c in range(d):
                res = []
                for sgn in (+1.0, -1.0):
                    delta = np.zeros(int(doff[-1])); delta[doff[var] + c] = sgn * h
                    res.append(evaluate(hm, p, O.retract(p, v0, delta), [k])[2][0])
                num[:, c] = (res[0] - res[1]) / (2 * h)
            assert np.abs(A - num).max() <= 1e-6 * max(1.0, np.abs(A).max()), (k, var)
        assert np.array_equal(J[k, 27:], -r0[k])


def test_monocular_record_in_the_three_row_layout(hm):
    """Beside stereo factors a monocular factor keeps its two rows, in the 30-double layout with a zero third row."""
    g = S.fixture("stereo_mixed")
    p = S.problem_of(g)
    v0, voff, nd = g["values0"], p.val_offsets(), S.device_noise_data(p)
    for k in (0, 1, p.n_proj - 1):
        K9 = np.zeros(9); K9[:5] = p.calib.reshape(-1, 5)[p.proj_calib[k]]
        if p.calib_distortion.size: K9[5:] = p.calib_distortion.reshape(-1, 4)[p.proj_calib[k]]
        pose = np.ascontiguousarray(v0[voff[p.proj_pose[k]]:][:12]); pt = np.ascontiguousarray(v0[voff[p.proj_point[k]]:][:3])
        z = np.ascontiguousarray(p.proj_z[2 * k:2 * k + 2]); nz = int(p.proj_noise[k])
        ndk = np.ascontiguousarray(nd[int(p.noise_off[nz]):][:4]) if p.noise_kind[nz] else np.zeros(1)
        J = np.zeros(30)
        hm.hms_proj_rows3(pose.ctypes.data, K9.ctypes.data, None, pt.ctypes.data, z.ctypes.data, int(p.noise_kind[nz]), ndk.ctypes.data, J.ctypes.data)
        ref = g["jac1"][k]
        assert np.all(J[12:18] == 0) and np.all(J[24:27] == 0) and J[29] == 0
        assert S.rel(np.concatenate([J[:12], J[18:24], J[27:29]]), ref) <= 1e-12
