"""TriangulationParameters::useLOST on the CPU: geom.h::triangulate_lost and the LOST forms of smart_triangulate compiled for the host
(tests/hostmath/hostmath_lost.cpp) against the reference's own known answers (geometry/tests/testTriangulation.cpp:96-157) and against the
real reference's per-factor TriangulationResult in the fixtures of tests/golden/make_golden_smart_lost.py.

Tolerances: the known answers as the reference's test states them (1e-12, 1e-4, 1e-3).  Against the fixtures the status is equal and a
VALID point lies within max(1e-12, 8 x tri_point_spread) relative, per track: tri_point_spread is the deviation of the reference's own
point when every input is moved by a relative 2^-52, and the factor 8 covers an arithmetic that differs in its order too (a QR written
out by hand against Eigen's).  Largest observed error / tolerance on the host: see DESIGN.md."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import smart_lost_support as S
from tests.smart_pose_support import device_calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hm():
    so = os.path.join(ROOT, "tests", "_build", "libhostmath_lost.so")
    src = os.path.join(ROOT, "tests", "hostmath", "hostmath_lost.cpp")
    deps = [src, os.path.join(ROOT, "gtsam_amd", "csrc", "factors.h"), os.path.join(ROOT, "gtsam_amd", "csrc", "geom.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.hml_linear_pose.argtypes = [C.c_int] + [C.c_void_p] * 8 + [C.c_double] * 2 + [C.c_void_p] * 2
    lib.hml_triangulate_pose.argtypes = [C.c_int] + [C.c_void_p] * 8 + [C.c_double] * 4 + [C.c_void_p] * 2
    lib.hml_triangulate_camera.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_double] * 3 + [C.c_int, C.c_double] + [C.c_void_p] * 2
    assert lib.hml_calib_stride() == 9
    return lib


# ---- the reference's own unit tests --------------------------------------------------------------------------------------------------
def ypr(y, p, r):
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]); Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def project(R, t, K, pt):
    q = R.T @ (np.asarray(pt) - t)
    u, v = q[0] / q[2], q[1] / q[2]
    return np.array([K[0] * u + K[2] * v + K[3], K[1] * v + K[4]])


def linear(hm, poses, K, zs, sigma, rank_tol=1e-9):
    """LOST (sigma > 0) or DLT of one track through PoseCams: poses = [(R, t)], one Cal3_S2 K, no sensor"""
    m = len(poses)
    values = np.concatenate([np.concatenate([R.reshape(-1), t]) for R, t in poses])
    voff = np.arange(m, dtype=np.int64) * 12
    calib = np.zeros(9); calib[:5] = K
    ids, ci, si = np.arange(m, dtype=np.int32), np.zeros(m, np.int32), np.full(m, -1, np.int32)
    z = np.ascontiguousarray(np.concatenate(zs)); rows, pt, sensor = np.zeros(8 * m), np.zeros(3), np.zeros(12)
    st = hm.hml_linear_pose(m, ids.ctypes.data, ci.ctypes.data, si.ctypes.data, calib.ctypes.data, sensor.ctypes.data, voff.ctypes.data,
                            values.ctypes.data, z.ctypes.data, rank_tol, sigma, rows.ctypes.data, pt.ctypes.data)
    return st, pt


def two_cameras():
    K = (1500.0, 1200.0, 0.1, 640.0, 480.0)
    R = ypr(-np.pi / 2, 0.0, -np.pi / 2)
    t1 = np.array([0.0, 0.0, 1.0])
    poses = [(R, t1), (R, t1 + R @ np.array([1.0, 0.0, 0.0]))]
    landmark = np.array([5.0, 0.5, 1.2])
    return K, poses, landmark, [project(Rk, tk, K, landmark) for Rk, tk in poses]


def test_two_cameras_using_lost_exact(hm):
    """testTriangulation.cpp:96-111"""
    K, poses, landmark, zs = two_cameras()
    st, pt = linear(hm, poses, K, zs, 1e-4)
    assert st == S.VALID and np.abs(pt - landmark).max() <= 1e-12, pt


def test_two_cameras_using_lost_noisy(hm):
    """testTriangulation.cpp:113-122"""
    K, poses, landmark, zs = two_cameras()
    zs = [zs[0] + [0.1, 0.5], zs[1] + [-0.2, 0.3]]
    st, pt = linear(hm, poses, K, zs, 1e-4)
    assert st == S.VALID and np.abs(pt - [4.995, 0.499167, 1.19814]).max() <= 1e-4, pt


def test_lost_beats_dlt_when_one_camera_is_much_closer(hm):
    """testTriangulation.cpp:125-157"""
    K = (1.0, 1.0, 0.0, 0.0, 0.0)
    poses = [(np.eye(3), np.zeros(3)), (np.eye(3), np.array([5.0, 0.0, -5.0]))]
    landmark = np.array([0.0, 0.0, 1.0])
    zs = [project(*poses[0], K, landmark) + [0.00817, 0.00977], project(*poses[1], K, landmark) + [-0.00610, 0.01969]]
    st, lost = linear(hm, poses, K, zs, 1e-2)
    assert st == S.VALID and np.abs(lost - [0.007, 0.011, 0.945]).max() <= 1e-3, lost
    st, dlt = linear(hm, poses, K, zs, 0.0)
    assert st == S.VALID
    assert np.linalg.norm(landmark - lost) <= np.linalg.norm(landmark - dlt)


# ---- the fixtures --------------------------------------------------------------------------------------------------------------------
def triangulate(hm, p, values, i, rank_tol=None, sigma=None):
    ids, z, ci, si = S.track(p, i)
    prm = p.smart_params.reshape(-1, 8)[i]
    rank_tol = prm[0] if rank_tol is None else rank_tol
    sigma = prm[7] if sigma is None else sigma
    m = ids.size
    voff = p.val_offsets()
    rows, pt = np.full(8 * m, np.nan), np.zeros(3)
    values = np.ascontiguousarray(values)
    if S.is_camera_type(p):
        st = hm.hml_triangulate_camera(m, ids.ctypes.data, voff.ctypes.data, values.ctypes.data, z.ctypes.data, rank_tol, prm[1], prm[2],
                                       int(prm[6]), sigma, rows.ctypes.data, pt.ctypes.data)
    else:
        calib = device_calib(p)
        sensor = np.ascontiguousarray(p.sensor if p.sensor.size else np.zeros(12))
        st = hm.hml_triangulate_pose(m, ids.ctypes.data, ci.ctypes.data, si.ctypes.data, calib.ctypes.data, sensor.ctypes.data, voff.ctypes.data,
                                     values.ctypes.data, z.ctypes.data, rank_tol, prm[1], prm[2], sigma, rows.ctypes.data, pt.ctypes.data)
    return st, pt


@pytest.mark.parametrize("name", S.FIXTURES)
def test_status_and_point_equal_the_reference(hm, name):
    g, p, v0 = S.load(name)
    tol = S.point_tolerance(g)
    worst = 0.0
    for i in range(p.n_smart):
        st, pt = triangulate(hm, p, v0, i)
        assert st == g["tri_status"][i], (i, st, g["tri_status"][i])
        if st == S.VALID:
            e = S.point_error(pt, g["tri_point"][i])[0]
            worst = max(worst, e / tol[i])
            assert e <= tol[i], (i, e, tol[i])
    print(f"{name}: largest error / tolerance {worst:.3g}")


@pytest.mark.parametrize("name", S.FIXTURES)
def test_fixtures_hold_the_paths_they_claim(name):
    g, p, _ = S.load(name)
    st, kind, m = g["tri_status"], g["lost_kind"], np.diff(p.smart_ptr)
    lost = p.smart_params.reshape(-1, 8)[:, 7] > 0
    assert int(g["trace_stable"]) == 1
    assert all(((st == s) & lost).any() for s in (S.VALID, S.DEGENERATE, S.OUTLIER, S.FAR_POINT))
    assert ((kind == 1) & (st == S.DEGENERATE)).any()                       # by rank
    assert ((kind == 2) & (m == 2) & (st == S.DEGENERATE)).any()            # by an exhausted partner search
    assert (S.lost_dlt_gap(g) > 1e-6).any()
    assert p.n_smart % 64 and int(p.smart_ptr[-1]) % 64
    assert ((p.smart_ptr[:-1] // 64 != (p.smart_ptr[1:] - 1) // 64) & (st == S.VALID) & lost).any()
    ratio = g["lost_pivots"][kind == 0] / g["lost_pivots"][kind == 0][:, :1]
    tol = p.smart_params.reshape(-1, 8)[kind == 0, :1]
    assert np.all(ratio >= 16 * tol) and np.all(g["lost_gaps"][(kind == 0) | (kind == 1)] >= 1e-6)
    if name == "smart_lost_pose":
        assert (~lost).any() and (p.smart_sensor >= 0).all()


def first_duplicated(p, i):
    """track i is three measurements whose first two are the same pixel"""
    ids, z, _, _ = S.track(p, i)
    return ids.size == 3 and np.array_equal(z[:2], z[2:4])


@pytest.mark.parametrize("name", S.FIXTURES)
def test_default_rank_tolerance_makes_every_lost_track_degenerate(hm, name):
    """rankTolerance = 1.0, the default of TriangulationParameters: the rank of ColPivHouseholderQR counts the pivots ABOVE threshold x the
    largest pivot, and none is: rank 0, as in the reference."""
    g, p, v0 = S.load(name)
    lost = np.flatnonzero((p.smart_params.reshape(-1, 8)[:, 7] > 0) & (np.diff(p.smart_ptr) >= 2))
    assert lost.size > 20
    for i in lost:
        assert triangulate(hm, p, v0, i, rank_tol=1.0)[0] == S.DEGENERATE, i


@pytest.mark.parametrize("name", S.FIXTURES)
def test_partner_search(hm, name):
    """Two coinciding measurements: no partner, DEGENERATE.  Three with the first camera duplicated: the search finds the third, VALID and
    the reference's point."""
    g, p, v0 = S.load(name)
    tol = S.point_tolerance(g)
    two = np.flatnonzero((g["lost_kind"] == 2) & (np.diff(p.smart_ptr) == 2))
    three = [i for i in range(p.n_smart) if g["lost_kind"][i] == 0 and first_duplicated(p, i)]
    assert two.size and three
    for i in two:
        _, z, _, _ = S.track(p, i)
        assert np.array_equal(z[:2], z[2:])
        assert triangulate(hm, p, v0, i)[0] == S.DEGENERATE
    for i in three:
        st, pt = triangulate(hm, p, v0, i)
        assert st == g["tri_status"][i] == S.VALID
        assert S.point_error(pt, g["tri_point"][i])[0] <= tol[i]


@pytest.mark.parametrize("name", ["smart_lost_cam", "smart_lost_pose", "smart_lost_rig"])
def test_sigma_scales_every_row_alike(hm, name):
    """sigma divides every weight q_i: 1e-4 and 1e-2 give the same statuses and, within the tolerance, the same points"""
    g, p, v0 = S.load(name)
    tol = S.point_tolerance(g)
    for i in np.flatnonzero(g["lost_kind"] >= 0):
        a, pa = triangulate(hm, p, v0, i, sigma=1e-4)
        b, pb = triangulate(hm, p, v0, i, sigma=1e-2)
        assert a == b == g["tri_status"][i], i
        if a == S.VALID:
            assert S.point_error(pa, g["tri_point"][i])[0] <= tol[i] and S.point_error(pb, g["tri_point"][i])[0] <= tol[i], i
