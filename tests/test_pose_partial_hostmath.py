"""PoseTranslationPrior / PoseRotationPrior <Pose3 | Pose2> on the CPU: pose_partial_linearize / pose_partial_error of
gtsam_amd/csrc/factors.h compiled for the host (tests/hostmath/hostmath_pose_partial.cpp) against the reference's records in the fixtures
of tests/golden/make_golden_pose_partial.py.

Tolerances: records <= 1e-12 and errors <= 1e-9 relative (the project's, tests/test_gpu_stereo.py).  Translation Jacobians against
central differences of the residual <= 2e-8: t - z is LINEAR in the tangent step of both retractions (Pose3: t + R V(omega) v with
V(0) = I and no first- or second-order term in omega alone; Pose2: t + R(theta) (v0, v1)), so there is no truncation error; the rounding
error is 2 eps |t| / (2 step) per entry of r, with |t| <= 128 (asserted) and step 1e-5 that is 2.9e-9, times the 3 products of a row of
R^T in the comparison: 8.6e-9."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import pose_partial_support as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hm():
    so = os.path.join(ROOT, "tests", "_build", "libhostmath_pose_partial.so")
    src = os.path.join(ROOT, "tests", "hostmath", "hostmath_pose_partial.cpp")
    deps = [src, os.path.join(ROOT, "gtsam_amd", "csrc", "factors.h"), os.path.join(ROOT, "gtsam_amd", "csrc", "geom.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.hmpp_factors.argtypes = [C.c_long] + [C.c_void_p] * 14
    lib.hmpp_unwhitened.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3
    assert lib.hmpp_record_size() == 90
    return lib


def evaluate(hm, p, values):
    """(records, errors) of the partial priors of p at `values`."""
    n = p.n_pose_partial
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    kind, var, nz, vt = i32(p.pose_partial_kind), i32(p.pose_partial_var), i32(p.pose_partial_noise), i32(p.var_type)
    z = np.ascontiguousarray(p.pose_partial_z, np.float64)
    values = np.ascontiguousarray(values, np.float64)
    voff, nd = p.val_offsets(), PS.device_noise_data(p)
    rk, rp = i32(p.noise_robust), np.ascontiguousarray(p.noise_robust_param, np.float64)
    J, e = np.zeros((n, 90)), np.zeros(n)
    hm.hmpp_factors(n, kind.ctypes.data, var.ctypes.data, vt.ctypes.data, z.ctypes.data, nz.ctypes.data, values.ctypes.data, voff.ctypes.data,
                    p.noise_kind.ctypes.data, p.noise_off.ctypes.data, nd.ctypes.data, rk.ctypes.data, rp.ctypes.data, J.ctypes.data, e.ctypes.data)
    return J, e


def unwhitened(hm, p, values, k):
    v = int(p.pose_partial_var[k]); vt = int(p.var_type[v])
    x = np.ascontiguousarray(values[p.val_offsets()[v]:][:12 if vt == 0 else 3])
    z = np.ascontiguousarray(p.pose_partial_z[9 * k:9 * k + 9]); J = np.zeros(90)
    hm.hmpp_unwhitened(int(p.pose_partial_kind[k]), vt, x.ctypes.data, z.ctypes.data, J.ctypes.data)
    return J


def other_factors_error(g, p):
    """The graph's error without its partial priors: 0.5 |b|^2 over the between records (no m-estimator on them in these fixtures)."""
    assert not p.noise_robust[p.between_noise].any()
    return 0.5 * float((g["jac2"][:, 72:] ** 2).sum())


@pytest.mark.parametrize("name", PS.FIXTURES)
def test_records_equal_the_reference(hm, name):
    g = PS.fixture(name)
    p = PS.problem_of(g)
    J, e = evaluate(hm, p, g["values0"])
    assert J.shape == g["jac6"].shape and p.n_prior == 0
    assert PS.rel(J, g["jac6"]) <= 1e-12
    assert np.abs(J - g["jac6"]).max() <= 1e-12 * max(1.0, np.abs(g["jac6"]).max())
    plain = p.noise_robust[p.pose_partial_noise] == 0
    assert PS.rel(e[plain], 0.5 * (g["jac6"][plain, 81:] ** 2).sum(1)) <= 1e-9


@pytest.mark.parametrize("name", ["pose_partial_graph3d", "pose_partial_graph2d"])
def test_error_equals_the_reference(hm, name):
    """The pose graphs: between factors and partial priors are all there is, so the recorded graph error is checked whole (the Huber
    and the Cauchy factor included)."""
    g = PS.fixture(name)
    p = PS.problem_of(g)
    _, e = evaluate(hm, p, g["values0"])
    assert p.n_smart == 0 and p.n_proj == 0
    assert abs(e.sum() + other_factors_error(g, p) - float(g["error"])) <= 1e-9 * float(g["error"])


@pytest.mark.parametrize("name", PS.FIXTURES)
def test_rows_a_factor_does_not_have_are_exactly_zero(hm, name):
    g = PS.fixture(name)
    p = PS.problem_of(g)
    J, _ = evaluate(hm, p, g["values0"])
    mask = PS.unused_entries(p)
    assert mask.any(1).all() and np.all(J[mask] == 0.0) and np.all(g["jac6"][mask] == 0.0)
    R, d = PS.rows_of(p)
    for i in range(p.n_pose_partial):
        assert np.abs(J[i, :R[i] * d[i]]).sum() > 0


def test_graph3d_holds_every_case(hm):
    g = PS.fixture("pose_partial_graph3d")
    p = PS.problem_of(g)
    assert p.n_vars == 97 and p.n_pose_partial == 131 and p.n_between == 96 + 23 and p.n_prior == 0
    assert set(p.noise_kind[p.pose_partial_noise]) == {0, 1, 2, 3} and set(p.noise_robust[p.pose_partial_noise]) == {0, 2, 3}
    for k in (int(g["huber"]), int(g["outlier"])):
        assert p.pose_partial_kind[k] == 0 and p.noise_robust[p.pose_partial_noise[k]] != 0
    v, kk = p.pose_partial_var, p.pose_partial_kind
    assert any(np.sum((v == x) & (kk == 0)) >= 2 and np.sum((v == x) & (kk == 1)) >= 1 for x in range(p.n_vars))
    # the gross outlier: its whitened rhs was scaled down by the Cauchy weight
    k = int(g["outlier"])
    r = unwhitened(hm, p, g["values0"], k)[81:84]
    assert np.linalg.norm(r) > 20.0 and np.linalg.norm(g["jac6"][k, 81:84]) < 2.0


def test_every_branch_of_logmap_by_recorded_index(hm):
    """rot_branch is the reference's own trace: 0 Taylor, 1 acos, 2 near pi.  The thresholds are 1e-3 on tr + 1 and -1e-6 on tr - 3;
    no factor lies within a factor 2 of either, so rounding cannot switch a branch."""
    g = PS.fixture("pose_partial_graph3d")
    p = PS.problem_of(g)
    br, tr = g["rot_branch"], g["rot_trace"]
    rot = (p.pose_partial_kind == 1)
    assert np.array_equal(br >= 0, rot) and set(br[rot]) == {0, 1, 2}
    a, b = tr[rot] + 1.0, tr[rot] - 3.0
    assert not np.any((a > 0.5e-3) & (a < 2e-3)) and not np.any((b < -0.5e-6) & (b > -2e-6))
    J, _ = evaluate(hm, p, g["values0"])
    for branch in (0, 1, 2):
        rows = np.flatnonzero(br == branch)
        assert np.abs(J[rows] - g["jac6"][rows]).max() <= 1e-12 * max(1.0, np.abs(g["jac6"][rows]).max()), branch
    k = int(g["rot_taylor"]); v = int(p.pose_partial_var[k])
    assert br[k] == 0 and np.array_equal(g["values0"][12 * v:12 * v + 9], p.pose_partial_z[9 * k:9 * k + 9])
    assert np.abs(unwhitened(hm, p, g["values0"], k)[81:84]).max() <= 1e-15
    k = int(g["rot_near_pi"])
    angle = np.linalg.norm(unwhitened(hm, p, g["values0"], k)[81:84])
    assert br[k] == 2 and 0 < np.pi - angle < 1e-4
    assert p.noise_data[p.noise_off[p.pose_partial_noise[k]]] >= 1.0       # a loose sigma


def test_pose2_rotation_prior_across_the_cut(hm):
    g = PS.fixture("pose_partial_graph2d")
    p = PS.problem_of(g)
    k, v = int(g["wrap"]), int(g["wrap_pose"])
    assert p.pose_partial_var[k] == v and p.pose_partial_kind[k] == 1 and g["values0"][3 * v + 2] == -3.1
    assert np.arctan2(p.pose_partial_z[9 * k + 1], p.pose_partial_z[9 * k]) == pytest.approx(3.1, abs=1e-15)
    J = unwhitened(hm, p, g["values0"], k)
    assert abs(-J[81] - (2 * np.pi - 6.2)) <= 1e-14           # 0.083, not -6.2
    assert np.array_equal(J[:3], [0.0, 0.0, 1.0])
    Jw, _ = evaluate(hm, p, g["values0"])
    assert abs(Jw[k, 81] - g["jac6"][k, 81]) <= 1e-12


@pytest.mark.parametrize("name", ["pose_partial_graph3d", "pose_partial_graph2d"])
def test_translation_jacobians_against_central_differences(hm, name):
    from oracle import gtsam_oracle as O
    g = PS.fixture(name)
    p = PS.problem_of(g)
    v0 = np.array(g["values0"])
    voff, doff = p.val_offsets(), p.dim_offsets()
    step = 1e-5
    rows = np.flatnonzero(p.pose_partial_kind == 0)[:12]
    for k in rows:
        v = int(p.pose_partial_var[k]); vt = int(p.var_type[v])
        R, d = PS.ROWS[(0, vt)], PS.DIM[vt]
        t = v0[voff[v] + 9:voff[v] + 12] if vt == 0 else v0[voff[v]:voff[v] + 2]
        assert np.abs(t).max() <= 128.0
        A = unwhitened(hm, p, v0, k)[:R * d].reshape(R, d)
        num = np.zeros((R, d))
        for c in range(d):
            rs = []
            for sgn in (+1.0, -1.0):
                delta = np.zeros(int(doff[-1])); delta[doff[v] + c] = sgn * step
                rs.append(-unwhitened(hm, p, O.retract(p, v0, delta), k)[81:81 + R])
            num[:, c] = (rs[0] - rs[1]) / (2 * step)
        assert np.abs(A - num).max() <= 2e-8, (k, np.abs(A - num).max())
        # and the block is what the reference writes: R beside zeros (Pose3: [0 | R]; Pose2: [R(theta) | 0])
        if vt == 0:
            assert np.all(A[:, :3] == 0.0) and np.array_equal(A[:, 3:], v0[voff[v]:voff[v] + 9].reshape(3, 3))
        else:
            th = v0[voff[v] + 2]
            assert np.all(A[:, 2] == 0.0) and np.array_equal(A[:, :2], [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])


def test_rotation_jacobian_is_the_identity_block_not_the_derivative(hm):
    """PoseRotationPrior writes H = [I | 0] whatever the residual (slam/PoseRotationPrior.h:81-90).  The derivative of Logmap(Z^T R Exp(w))
    is the inverse right Jacobian of the residual r, I + skew(r) / 2 + ...: for the largest acos-branch residual of the fixture the
    numerical derivative differs from the identity by more than 0.2 |r|.  The evaluator restates the reference, not the derivative."""
    from oracle import gtsam_oracle as O
    g = PS.fixture("pose_partial_graph3d")
    p = PS.problem_of(g)
    v0 = np.array(g["values0"])
    doff = p.dim_offsets()
    want = np.hstack([np.eye(3), np.zeros((3, 3))])
    for k in np.flatnonzero(p.pose_partial_kind == 1):
        assert np.array_equal(unwhitened(hm, p, v0, k)[:18].reshape(3, 6), want), k
    g2 = PS.fixture("pose_partial_graph2d")
    p2 = PS.problem_of(g2)
    for k in np.flatnonzero(p2.pose_partial_kind == 1):
        assert np.array_equal(unwhitened(hm, p2, g2["values0"], k)[:3], [0.0, 0.0, 1.0]), k
    # the acos-branch factor with the largest residual (away from the cut at pi, where a difference quotient means nothing)
    k = int(max(np.flatnonzero(g["rot_branch"] == 1), key=lambda i: np.linalg.norm(unwhitened(hm, p, v0, i)[81:84])))
    v = int(p.pose_partial_var[k]); step = 1e-6
    num = np.zeros((3, 3))
    for c in range(3):
        rs = []
        for sgn in (+1.0, -1.0):
            delta = np.zeros(int(doff[-1])); delta[doff[v] + c] = sgn * step
            rs.append(-unwhitened(hm, p, O.retract(p, v0, delta), k)[81:84])
        num[:, c] = (rs[0] - rs[1]) / (2 * step)
    angle = np.linalg.norm(unwhitened(hm, p, v0, k)[81:84])
    assert angle > 0.05 and np.abs(num - np.eye(3)).max() > 0.2 * angle      # (the skew part of the inverse Jacobian is omega / 2)
