"""BearingRangeFactor / RangeFactor / BearingFactor <Pose3, Point3> on the CPU: sam_linearize / sam_error of gtsam_amd/csrc/factors.h compiled
for the host (tests/hostmath/hostmath_sam.cpp) against the reference's records in the fixtures of tests/golden/make_golden_sam3d.py.

Tolerances: records <= 1e-12 and errors <= 1e-9 relative (the project's, tests/test_gpu_stereo.py).  Jacobians against central
differences of h <= 1e-7 max(1, |A|): step 1e-6 on entries of order 0.1 - 10, so the truncation (h^2 times a third derivative of order
1) is about 1e-12 and the rounding (eps |h(x)| / step with |h(x)| <= 20) about 4e-9; both stay below the bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sam_support as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hm():
    so = os.path.join(ROOT, "tests", "_build", "libhostmath_sam.so")
    src = os.path.join(ROOT, "tests", "hostmath", "hostmath_sam.cpp")
    deps = [src, os.path.join(ROOT, "gtsam_amd", "csrc", "factors.h"), os.path.join(ROOT, "gtsam_amd", "csrc", "geom.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.hmsam_factors.argtypes = [C.c_long] + [C.c_void_p] * 15
    lib.hmsam_unwhitened.argtypes = [C.c_int] + [C.c_void_p] * 4
    lib.hmsam_predict.argtypes = [C.c_void_p] * 3
    assert lib.hmsam_record_size() == 30
    return lib


def evaluate(hm, p, values, rows=None):
    """(records, errors, whitened residuals) of the sam factors `rows` of p at `values`."""
    rows = np.arange(p.n_sam) if rows is None else np.asarray(rows)
    n = rows.size
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    kind, pose, pt, nz = i32(p.sam_kind[rows]), i32(p.sam_pose[rows]), i32(p.sam_point[rows]), i32(p.sam_noise[rows])
    z = np.ascontiguousarray(p.sam_z.reshape(-1, 4)[rows])
    values = np.ascontiguousarray(values, np.float64)
    voff, nd = p.val_offsets(), SS.S.device_noise_data(p)
    rk, rp = i32(p.noise_robust), np.ascontiguousarray(p.noise_robust_param, np.float64)
    J, e, r = np.zeros((n, 30)), np.zeros(n), np.zeros((n, 3))
    hm.hmsam_factors(n, kind.ctypes.data, pose.ctypes.data, pt.ctypes.data, z.ctypes.data, nz.ctypes.data, values.ctypes.data, voff.ctypes.data,
                     p.noise_kind.ctypes.data, p.noise_off.ctypes.data, nd.ctypes.data, rk.ctypes.data, rp.ctypes.data, J.ctypes.data,
                     e.ctypes.data, r.ctypes.data)
    return J, e, r


def other_factors_error(g):
    """0.5 |b|^2 over the records of every factor that is not a sam factor (none of them has an m-estimator in these fixtures)."""
    p = SS.problem_of(g)
    for tab in (p.proj_noise, p.stereo_noise, p.between_noise, p.prior_noise):
        assert not p.noise_robust[tab].any()
    return sum(0.5 * float((g[f"jac{ft}"][:, o:] ** 2).sum()) for ft, o in ((1, 18), (2, 72), (3, 81), (4, 27)) if f"jac{ft}" in g)


@pytest.mark.parametrize("name", ["sam3d_mixed", "sam3d_slam"])
def test_records_and_error_equal_the_reference(hm, name):
    g = SS.fixture(name)
    p = SS.problem_of(g)
    J, e, _ = evaluate(hm, p, g["values0"])
    assert J.shape == g["jac5"].shape
    assert SS.rel(J, g["jac5"]) <= 1e-12
    assert abs(e.sum() + other_factors_error(g) - float(g["error"])) <= 1e-9 * float(g["error"])
    plain = p.noise_robust[p.sam_noise] == 0
    assert SS.rel(e[plain], 0.5 * (g["jac5"][plain, 27:] ** 2).sum(1)) <= 1e-9


def test_sam3d_mixed_holds_every_kind_noise_and_branch(hm):
    g = SS.fixture("sam3d_mixed")
    p = SS.problem_of(g)
    assert set(p.sam_kind) == {0, 1, 2} and p.n_proj and p.n_stereo and p.n_between and p.n_prior
    for kind, dim in ((0, 3), (1, 1), (2, 2)):
        nz = p.sam_noise[p.sam_kind == kind]
        assert set(p.noise_dim[nz]) == {dim} and set(p.noise_kind[nz]) == {0, 1, 2, 3}, kind
    assert set(p.noise_robust[p.sam_noise]) == {0, 2, 3}          # one Huber, one Cauchy
    J, _, _ = evaluate(hm, p, g["values0"])
    for name in ("same", "opposite", "tie", ):
        k = int(g["branch_" + name])
        assert SS.rel(J[k], g["jac5"][k]) <= 1e-12, name
    voff, v0 = p.val_offsets(), g["values0"]

    def predicted(k):
        out = np.zeros(10)
        T = np.ascontiguousarray(v0[voff[p.sam_pose[k]]:][:12]); pt = np.ascontiguousarray(v0[voff[p.sam_point[k]]:][:3])
        hm.hmsam_predict(T.ctypes.data, pt.ctypes.data, out.ctypes.data)
        return out
    k = int(g["branch_same"]); h = predicted(k)[:3]; z = p.sam_z.reshape(-1, 4)[k, :3]
    assert np.array_equal(h, z) and 1 - float(h @ z) ** 2 < np.finfo(float).eps and np.all(J[k, 27:29] == 0.0)
    k = int(g["branch_opposite"]); h = predicted(k)[:3]; z = p.sam_z.reshape(-1, 4)[k, :3]
    assert np.array_equal(h, -z) and p.sam_kind[k] == 2
    sigma = float(p.noise_data[p.noise_off[p.sam_noise[k]]])
    assert np.allclose(J[k, 27:29], [np.pi / sigma, 0.0], rtol=1e-15, atol=0) and np.array_equal(g["jac5"][k, 27:29], J[k, 27:29])
    k = int(g["branch_tie"]); h = np.abs(predicted(k)[:3])
    assert h[0] == h[1] < h[2]
    assert predicted(k)[3] == 0.0 and predicted(k)[4] != 0.0      # b1 = normalize(n x e_x): the tie goes to the x axis (`<=`, Unit3.cpp:72-81)
    for a, axis in enumerate("xyz"):
        k = int(g["axis_" + axis]); h = np.abs(predicted(k)[:3])
        assert np.argmin(h) == a and np.sum(h == h[a]) == 1 and p.sam_kind[k] != 1
        assert SS.rel(J[k], g["jac5"][k]) <= 1e-12, axis


def test_unused_rows_are_exactly_zero(hm):
    g = SS.fixture("sam3d_mixed")
    p = SS.problem_of(g)
    J, _, _ = evaluate(hm, p, g["values0"])
    A1, A2, b = J[:, :18].reshape(-1, 3, 6), J[:, 18:27].reshape(-1, 3, 3), J[:, 27:]
    rng_only, brg_only = p.sam_kind == 1, p.sam_kind == 2
    assert rng_only.any() and brg_only.any()
    assert np.all(A1[rng_only, 1:] == 0.0) and np.all(A2[rng_only, 1:] == 0.0) and np.all(b[rng_only, 1:] == 0.0)
    assert np.all(A1[brg_only, 2] == 0.0) and np.all(A2[brg_only, 2] == 0.0) and np.all(b[brg_only, 2] == 0.0)
    assert np.all(np.abs(A1[rng_only, 0]).sum(1) > 0) and np.all(np.abs(A1[brg_only, :2]).sum((1, 2)) > 0)
    ref = g["jac5"]      # (the reference's records, as the generator lays them out, agree)
    assert np.all(ref[rng_only][:, [6, 12, 21, 24, 28, 29]] == 0.0) and np.all(ref[brg_only][:, [12, 24, 29]] == 0.0)


def test_jacobians_against_central_differences_of_h(hm):
    """The unwhitened blocks are the derivatives of h alone: the bearing's in the basis of the UNPERTURBED prediction
    (B0^T (h(x+) - h(x-)) / 2 step), the range's plainly.  The chart derivative of Local is not in them."""
    from oracle import gtsam_oracle as O
    g = SS.fixture("sam3d_mixed")
    p = SS.problem_of(g)
    v0 = np.array(g["values0"])
    voff, doff = p.val_offsets(), p.dim_offsets()
    rows = np.concatenate([np.arange(9), [int(g[k]) for k in ("branch_same", "branch_opposite", "branch_tie", "axis_x", "axis_y", "axis_z")]])
    step = 1e-6

    def predict(values, k):
        out = np.zeros(10)
        T = np.ascontiguousarray(values[voff[p.sam_pose[k]]:][:12]); pt = np.ascontiguousarray(values[voff[p.sam_point[k]]:][:3])
        hm.hmsam_predict(T.ctypes.data, pt.ctypes.data, out.ctypes.data)
        return out
    for k in rows:
        kind = int(p.sam_kind[k])
        T = np.ascontiguousarray(v0[voff[p.sam_pose[k]]:][:12]); pt = np.ascontiguousarray(v0[voff[p.sam_point[k]]:][:3])
        z = np.ascontiguousarray(p.sam_z.reshape(-1, 4)[k]); J = np.zeros(30)
        hm.hmsam_unwhitened(kind, T.ctypes.data, pt.ctypes.data, z.ctypes.data, J.ctypes.data)
        h0 = predict(v0, k); B0 = h0[3:9].reshape(2, 3)
        for var, A, d in ((int(p.sam_pose[k]), J[:18].reshape(3, 6), 6), (int(p.sam_point[k]), J[18:27].reshape(3, 3), 3)):
            num_b, num_r = np.zeros((2, d)), np.zeros(d)
            for c in range(d):
                hs = []
                for sgn in (+1.0, -1.0):
                    delta = np.zeros(int(doff[-1])); delta[doff[var] + c] = sgn * step
                    hs.append(predict(O.retract(p, v0, delta), k))
                num_b[:, c] = B0 @ (hs[0][:3] - hs[1][:3]) / (2 * step)
                num_r[c] = (hs[0][9] - hs[1][9]) / (2 * step)
            want = {0: np.vstack([num_b, num_r]), 1: np.vstack([num_r, np.zeros((2, d))]), 2: np.vstack([num_b, np.zeros((1, d))])}[kind]
            assert np.abs(A - want).max() <= 1e-7 * max(1.0, np.abs(A).max()), (k, kind, var)


def test_range_derivative_falls_back_to_ones_on_the_pose(hm):
    """A landmark ON its pose's translation: norm3's derivative is (1, 1, 1) (Point3.cpp:44-47), so the range row is
    (1, 1, 1) D_local = [0 0 0 -1 -1 -1 | (1, 1, 1) R^T] and b = z - 0."""
    g = SS.fixture("sam3d_mixed")
    p = SS.problem_of(g)
    T = np.ascontiguousarray(g["values0"][p.val_offsets()[p.sam_pose[0]]:][:12])
    pt = np.ascontiguousarray(T[9:12].copy()); z = np.array([0.0, 0.0, 0.0, 2.5]); J = np.zeros(30)
    hm.hmsam_unwhitened(1, T.ctypes.data, pt.ctypes.data, z.ctypes.data, J.ctypes.data)
    R = T[:9].reshape(3, 3)
    assert np.array_equal(J[:6], [0.0, 0.0, 0.0, -1.0, -1.0, -1.0])
    assert np.allclose(J[18:21], np.ones(3) @ R.T, rtol=1e-15, atol=0)
    assert J[27] == 2.5 and np.all(J[6:18] == 0.0) and np.all(J[21:27] == 0.0) and np.all(J[28:] == 0.0)
    # just off the pose the general form is back: a unit row
    pt2 = np.ascontiguousarray(pt + np.array([1e-9, 0.0, 0.0]))
    hm.hmsam_unwhitened(1, T.ctypes.data, pt2.ctypes.data, z.ctypes.data, J.ctypes.data)
    assert abs(np.linalg.norm(J[18:21]) - 1.0) <= 1e-12
