"""SmartProjectionPoseFactor<Cal3_S2> on the CPU: the pose forms of the device's triangulation (geom.h::smart_triangulate with the PoseCams
accessor) and of the at-infinity evaluators (factors.h::proj_linearize_at_infinity / proj_error_at_infinity) compiled for the host
(tests/hostmath/hostmath_smart_pose.cpp) against the real reference's per-factor TriangulationResult in the fixtures of
tests/golden/make_golden_smart_pose.py.

Tolerances: the status is equal, the point within 1e-9 relative (a DLT through a 4 x 4 eigen-decomposition instead of the reference's
SVD of the m x 4 matrix: rounding only, amplified by the conditioning of a track of a few degrees of parallax); the at-infinity
Jacobians against central differences of the evaluator's own residual <= 1e-6 (step 1e-6 on entries of order 1e2 - 1e3: truncation h^2
and rounding eps / h both stay below that -- the reasoning of tests/test_stereo_hostmath.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import smart_pose_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hm():
    so = os.path.join(ROOT, "tests", "_build", "libhostmath_smart_pose.so")
    src = os.path.join(ROOT, "tests", "hostmath", "hostmath_smart_pose.cpp")
    deps = [src, os.path.join(ROOT, "gtsam_amd", "csrc", "factors.h"), os.path.join(ROOT, "gtsam_amd", "csrc", "geom.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.hmsp_triangulate.argtypes = [C.c_int] + [C.c_void_p] * 8 + [C.c_double] * 3 + [C.c_void_p]
    lib.hmsp_camera.argtypes = [C.c_int] + [C.c_void_p] * 10
    lib.hmsp_backproject_at_infinity.argtypes = [C.c_void_p] * 4
    lib.hmsp_unit3_basis.argtypes = [C.c_void_p] * 3
    lib.hmsp_at_infinity.argtypes = [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3
    lib.hmsp_pose_retract.argtypes = [C.c_void_p] * 3
    assert lib.hmsp_record_size() == 20 and lib.hmsp_calib_stride() == 9
    return lib


def tables(p):
    sensor = np.ascontiguousarray(p.sensor if p.sensor.size else np.zeros(12))
    return S.device_calib(p), sensor, p.val_offsets()


def triangulate(hm, p, values, i):
    ids, z, ci, si = S.track(p, i)
    calib, sensor, voff = tables(p)
    m = ids.size
    cidx, sidx = np.full(m, ci, np.int32), np.full(m, si, np.int32)
    prm = p.smart_params.reshape(-1, 8)[i]
    pt = np.zeros(3)
    st = hm.hmsp_triangulate(m, ids.ctypes.data, cidx.ctypes.data, sidx.ctypes.data, calib.ctypes.data, sensor.ctypes.data, voff.ctypes.data,
                             values.ctypes.data, z.ctypes.data, prm[0], prm[1], prm[2], pt.ctypes.data)
    return st, pt


@pytest.mark.parametrize("name", S.FIXTURES)
def test_triangulation_status_and_point_equal_the_reference(hm, name):
    g, p, v0 = S.load(name)
    want_st, want_pt = g["tri_status"], g["tri_point"]
    for i in range(p.n_smart):
        st, pt = triangulate(hm, p, v0, i)
        assert st == want_st[i], (i, st, want_st[i])
        if st == S.VALID:
            assert S.rel(pt, want_pt[i]) <= 1e-9, (i, pt, want_pt[i])


def test_fixtures_hold_the_failing_statuses_they_claim():
    for name in S.FIXTURES[2:]:
        st = S.fixture(name)["tri_status"]
        assert (st == S.DEGENERATE).any() and (st == S.FAR_POINT).any() and (st == S.VALID).any()
    st = S.fixture("smart_pose_mixed")["tri_status"]
    assert all((st == s).any() for s in (S.VALID, S.DEGENERATE, S.OUTLIER, S.FAR_POINT))


def test_undistortion_round_trip_is_reproduced_not_skipped(hm):
    """CameraSet<PinholePose<Cal3_S2>> runs calibrate then uncalibrate of the same K on every pixel (triangulation.h:315-330): not the
    identity in floating point.  The accessor does the same arithmetic as Cal3_S2.cpp:44-69, here restated in numpy."""
    g, p, v0 = S.load("smart_pose_mixed")
    calib, sensor, voff = tables(p)
    differs = 0
    for i in range(0, p.n_smart, 7):
        ids, z, ci, si = S.track(p, i)
        cidx, sidx = np.full(ids.size, ci, np.int32), np.full(ids.size, si, np.int32)
        T, zu = np.zeros(12), np.zeros(2)
        hm.hmsp_camera(0, ids.ctypes.data, cidx.ctypes.data, sidx.ctypes.data, calib.ctypes.data, sensor.ctypes.data, voff.ctypes.data,
                       v0.ctypes.data, z.ctypes.data, T.ctypes.data, zu.ctypes.data)
        fx, fy, s, u0, v0_ = p.calib.reshape(-1, 5)[ci]
        du, dv = z[0] - u0, z[1] - v0_
        ify = (1 / fy) * dv
        x, y = (1 / fx) * (du - s * ify), ify
        assert np.array_equal(zu, [fx * x + s * y + u0, fy * y + v0_])
        differs += int(not np.array_equal(zu, z[:2]))
        # the camera pose is the composed world_P_sensor
        body = v0[voff[ids[0]]:][:12]
        R, t = body[:9].reshape(3, 3), body[9:]
        Rs, ts = sensor[12 * si:][:9].reshape(3, 3), sensor[12 * si:][9:12]
        assert si >= 0 and np.allclose(T[:9].reshape(3, 3), R @ Rs, rtol=0, atol=1e-15) and np.allclose(T[9:], t + R @ ts, rtol=0, atol=1e-14)
    assert differs > 0


@pytest.mark.parametrize("name", ["smart_pose_far_ignore", "smart_pose_mixed"])
def test_at_infinity_jacobians_against_central_differences(hm, name):
    """The 2 x 6 pose block (sensor chain rule included on smart_pose_mixed) and the 2 x 2 direction block of a failed track's
    measurements, against central differences of the evaluator's own whitened residual."""
    g, p, v0 = S.load(name)
    calib, sensor, voff = tables(p)
    failed = np.flatnonzero((g["tri_status"] != S.VALID) & (np.diff(p.smart_ptr) >= 2))[:4]
    assert failed.size >= 2
    h = 1e-6
    for i in failed:
        ids, z, ci, si = S.track(p, i)
        K9 = np.ascontiguousarray(calib[ci]); Sp = np.ascontiguousarray(sensor[12 * si:12 * si + 12]) if si >= 0 else None
        nz = int(p.smart_noise[i])
        nk = int(p.noise_kind[nz]); nd = np.array([1.0 / p.noise_data[int(p.noise_off[nz])]]) if nk == 1 else np.zeros(1)
        cidx, sidx = np.full(ids.size, ci, np.int32), np.full(ids.size, si, np.int32)
        T0, zu = np.zeros(12), np.zeros(2)
        hm.hmsp_camera(0, ids.ctypes.data, cidx.ctypes.data, sidx.ctypes.data, calib.ctypes.data, sensor.ctypes.data, voff.ctypes.data,
                       v0.ctypes.data, z.ctypes.data, T0.ctypes.data, zu.ctypes.data)
        d = np.zeros(3)
        hm.hmsp_backproject_at_infinity(T0.ctypes.data, K9.ctypes.data, z.ctypes.data, d.ctypes.data)
        assert abs(np.linalg.norm(d) - 1.0) <= 1e-15
        b1, b2 = np.zeros(3), np.zeros(3)
        hm.hmsp_unit3_basis(d.ctypes.data, b1.ctypes.data, b2.ctypes.data)

        def evaluate(pose, direction, zk):
            J, e = np.zeros(20), np.zeros(1)
            pose = np.ascontiguousarray(pose); direction = np.ascontiguousarray(direction); zk = np.ascontiguousarray(zk)
            ok = hm.hmsp_at_infinity(pose.ctypes.data, K9.ctypes.data, Sp.ctypes.data if Sp is not None else None, direction.ctypes.data,
                                     zk.ctypes.data, nk, nd.ctypes.data, J.ctypes.data, e.ctypes.data)
            return ok, J, e[0]
        for k in range(ids.size):
            pose = v0[voff[ids[k]]:][:12]; zk = z[2 * k:2 * k + 2]
            ok, J, e = evaluate(pose, d, zk)
            assert ok == 1
            r0 = -J[18:20]
            assert abs(e - 0.5 * r0 @ r0) <= 1e-15 * max(e, 1.0)
            A1, A2 = J[:12].reshape(2, 6), J[12:18].reshape(2, 3)
            assert np.all(A2[:, 2] == 0.0)
            if si < 0:
                assert np.all(A1[:, 3:] == 0.0)          # rotation only without a sensor offset
            num = np.zeros((2, 6))
            for c in range(6):
                res = []
                for sgn in (+1.0, -1.0):
                    xi = np.zeros(6); xi[c] = sgn * h
                    out = np.zeros(12)
                    hm.hmsp_pose_retract(np.ascontiguousarray(pose).ctypes.data, xi.ctypes.data, out.ctypes.data)
                    res.append(-evaluate(out, d, zk)[1][18:20])
                num[:, c] = (res[0] - res[1]) / (2 * h)
            assert np.abs(A1 - num).max() <= 1e-6 * max(1.0, np.abs(A1).max()), (i, k)
            num = np.zeros((2, 2))
            for c, b in enumerate((b1, b2)):
                res = []
                for sgn in (+1.0, -1.0):
                    dd = d + sgn * h * b
                    res.append(-evaluate(pose, dd / np.linalg.norm(dd), zk)[1][18:20])
                num[:, c] = (res[0] - res[1]) / (2 * h)
            assert np.abs(A2[:, :2] - num).max() <= 1e-6 * max(1.0, np.abs(A2).max()), (i, k)


def test_direction_behind_a_camera_is_reported(hm):
    g, p, v0 = S.load("smart_pose_far_ignore")
    calib, _, voff = tables(p)
    pose = np.ascontiguousarray(v0[:12])
    back = np.ascontiguousarray(-pose[:9].reshape(3, 3)[:, 2])       # against the optical axis
    J, e = np.ones(20), np.zeros(1)
    z = np.zeros(2); nd = np.zeros(1)
    assert hm.hmsp_at_infinity(pose.ctypes.data, np.ascontiguousarray(calib[0]).ctypes.data, None, back.ctypes.data, z.ctypes.data, 0, nd.ctypes.data,
                               J.ctypes.data, e.ctypes.data) == 0
    assert np.all(J == 0.0)
