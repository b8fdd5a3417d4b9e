"""The two extractors against each other, on the CPU: the C++ shim (gtsam_amd/host, built against the real GTSAM of
oracle/_ref; graphs from the reference's shipped files through the reference's own loaders, tests/cpp/test_shim_extractor.cpp)
and the Python mirror (gtsam_amd/api.py / problem.py; the same files through gtsam_amd/io.py or the golden copies of what the
reference's loaders returned).  Both run under tools/hipstub, which hashes every host-to-device copy: equal records mean the
library was handed identical tables -- variable order, factor tables, shared noise rows (one row per distinct model, however
many objects), packed values -- and built the identical symbolic analysis from them."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402
from tests.conftest import data_dir  # noqa: E402

DATA = data_dir()
EXE = os.path.join(ROOT, "tests", "_build", "test_shim_extractor")

_CHILD = r'''
import ctypes, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from tools import host_profile as HP
from gtsam_amd import io, lib as L
from gtsam_amd.problem import NOISE_DIAGONAL, pose_graph_problem
from tests import problems as PB
from tests.conftest import load_golden
stub = ctypes.CDLL(HP.STUB)
stub.hipstub_h2d_record.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ulonglong)]
def records(p, v0):
    stub.hipstub_reset()
    g = L.DeviceGraph(p); g.set_values(np.ascontiguousarray(v0, np.float64))
    n = ctypes.c_longlong(); h = ctypes.c_ulonglong(); out = []
    for i in range(stub.hipstub_h2d_count()):
        stub.hipstub_h2d_record(i, ctypes.byref(n), ctypes.byref(h)); out.append("%%d:%%d" %% (n.value, h.value))
    g.close(); return out
res = {}
res["sfmexample_bal_dubrovnik_3_7"] = records(*PB.dubrovnik_sfmexample(load_golden("dubrovnik_3_7")))
res["pose2slam_w100"] = records(*PB.pose2_graph(load_golden("pose2_w100")))
# the reference's own loader through the oracle harness: bit-identical numbers to what the C++ side read (gtsam_amd/io.py
# agrees with it to 1e-14, tests/test_io.py, which is not enough for equal hashes)
from oracle import ref
d = ref.load_g2o3d(%(data)r + "pose3example.txt")
p = pose_graph_problem(len(d["vertex_keys"]), d["v1"], d["v2"], d["z"], d["noise_kind"], d["noise"])
p.add_prior(0, d["vertex_poses"][0], p.add_noise(NOISE_DIAGONAL, 6, np.sqrt([1e-6] * 3 + [1e-4] * 3)))
res["pose3slam_pose3example"] = records(p, d["vertex_poses"].reshape(-1))
# tests/cpp/test_shim_extractor.cpp, mixedEveryBranch(): the same graph from the same literals through the wrapped API's mirror
from gtsam_amd import api as A
C, P, X, Lm = A.symbol_shorthand.C, A.symbol_shorthand.P, A.symbol_shorthand.X, A.symbol_shorthand.L
Rz, Rx, Ry = A.Rot3([0, -1, 0, 1, 0, 0, 0, 0, 1]), A.Rot3([1, 0, 0, 0, 0, -1, 0, 1, 0]), A.Rot3([0, 0, 1, 0, 1, 0, -1, 0, 0])
X0, X1, X2 = A.Pose3(A.Rot3(), [0, 0, 0]), A.Pose3(Rz, [1, 2, -3]), A.Pose3(Rx, [-0.5, 4, 0.25])
T1, T2, T3 = A.Pose3(Rz, [1, 0, 0.5]), A.Pose3(Ry, [0, -2, 8]), A.Pose3(Rx, [0.125, 3, -1])
S1, S2 = A.Pose3(Ry, [0.5, 0, 0]), A.Pose3(Rz, [0, 0.25, -0.125])
Cam = A.PinholeCameraCal3Bundler
cam = [Cam(X1, A.Cal3Bundler(512, 0.25, -0.125, 0, 0)), Cam(T2, A.Cal3Bundler(256, 0, 0.5, 2, -4)),
       Cam(T3, A.Cal3Bundler(640, -0.0625, 0, 0, 0)), Cam(X2, A.Cal3Bundler(128, 0.5, 0.25, -1, 1))]
iv = A.Values()
for i in range(4): iv.insert(C(i), cam[i])
iv.insert(P(0), A.Point3(1, -2, 3)); iv.insert(P(1), A.Point3(0.5, 0.25, 16)); iv.insert(P(2), A.Point3(-4, 7, 9))
iv.insert(Lm(0), A.Point3(0.5, 0.25, -4)); iv.insert(Lm(1), A.Point3(2, 2, 32))
iv.insert(X(0), X0); iv.insert(X(1), X1); iv.insert(X(2), X2)
nm = A.noiseModel
nA, nA2 = nm.Isotropic.Sigma(2, 0.5), nm.Isotropic.Sigma(2, 0.5)
nH = nm.Robust.Create(nm.mEstimator.Huber.Create(1.5), nm.Isotropic.Sigma(2, 0.25))
nU = nm.Unit.Create(2)
R = 2.0 * np.eye(6); R[0, 1] = 0.5; R[0, 5] = -0.25; R[2, 3] = 1; R[4, 5] = 0.125
nG = nm.Gaussian.SqrtInformation(R)
sig = [0.5, 0.5, 0.5, 0.25, 0.25, 0.125]
nD, nD2 = nm.Diagonal.Sigmas(sig), nm.Diagonal.Sigmas(sig)
n9, n3, n3b, nS = nm.Isotropic.Sigma(9, 0.125), nm.Isotropic.Sigma(3, 0.5), nm.Isotropic.Sigma(3, 0.5), nm.Isotropic.Sigma(2, 2.0)
K1, K2 = A.Cal3_S2(500, 400, 0.5, 320, 240), A.Cal3_S2(250, 250, 0, 160, 120)
D1 = A.Cal3DS2(300, 350, 0.25, 100, 50, 0.125, -0.0625, 0.03125, 0.015625)
Sfm, Proj, ProjDS2, Btw = A.GeneralSFMFactorCal3Bundler, A.GenericProjectionFactorCal3_S2, A.GenericProjectionFactorCal3DS2, A.BetweenFactorPose3
SP, Smart = A.SmartProjectionParams, A.SmartProjectionFactorPinholeCameraCal3Bundler
g = A.NonlinearFactorGraph()
g.add(Sfm([1, 2], nA, C(0), P(0))); g.add(Sfm([-3, 4], nA, C(1), P(0))); g.add(Sfm([0.5, -1.5], nA, C(2), P(0)))
g.add(Sfm([8, -2], nA, C(0), P(1))); g.add(Sfm([2.25, 1], nH, C(1), P(1))); g.add(Sfm([-7, 3], nH, C(2), P(1)))
g.add(Sfm([4, 4], nA2, C(0), P(2))); g.add(Sfm([-0.75, 6], nA2, C(2), P(2)))
sp1 = SP(SP.JACOBIAN_Q, SP.HANDLE_INFINITY); sp1.setRankTolerance(4)
s1 = Smart(nA2, sp1); s1.add([1, 1], C(0)); s1.add([2, -1], C(1)); s1.add([-3, 0.5], C(2)); g.add(s1)
sp2 = SP(SP.JACOBIAN_SVD, SP.ZERO_ON_DEGENERACY, 0.125)
sp2.setRankTolerance(0.25); sp2.setLandmarkDistanceThreshold(64); sp2.setDynamicOutlierRejectionThreshold(8)
s2 = Smart(nA, sp2); s2.add([5, 2], C(3)); s2.add([-1, -2], C(0)); g.add(s2)
g.add(Proj([10, 20], nA, X(0), Lm(0), K1)); g.add(Proj([-5, 7.5], nA, X(1), Lm(0), K1, S1))
g.add(Proj([3, -4], nU, X(2), Lm(0), K2, S2)); g.add(ProjDS2([6.5, 1], nU, X(0), Lm(1), D1)); g.add(ProjDS2([-2, -8], nA, X(1), Lm(1), D1, S1))
g.add(Btw(X(0), X(1), T1, nG)); g.add(Btw(X(1), X(2), T2, nD)); g.add(Btw(X(0), X(2), T3, nG))
g.add(Btw(X(2), X(1), T1, nD2)); g.add(Btw(X(1), X(0), T2, nG))
g.addPriorPose3(X(0), X0, nD); g.addPriorPinholeCameraCal3Bundler(C(0), cam[0], n9)
g.addPriorPoint3(P(0), A.Point3(1, -2, 3), n3); g.addPriorPoint3(Lm(0), A.Point3(0.5, 0.25, -4), n3b)
s3 = Smart(nS); s3.add([0, 1], C(1)); s3.add([1, 0], C(2)); g.add(s3)
g.addPriorPose3(X(2), X2, nD2); g.add(Btw(X(2), X(0), T3, nG)); g.add(Proj([1.5, 2.5], nU, X(2), Lm(1), K2, S2))
g.add(Sfm([9, -9], nH, C(1), P(2))); g.add(Sfm([-6, 0.5], nA, C(3), P(2)))
assert g.size() == 30
pm, vm, _ = A.extract(g, iv)
res["mixed_every_branch"] = records(pm, vm)
print("RESULT " + json.dumps(res))
'''


def test_cpp_and_python_extractors_hand_the_library_identical_tables():
    if not (os.path.exists(EXE) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so"))):
        pytest.skip("shim extractor test / oracle/_ref not built")
    stub = HP.build_stub()
    env = dict(os.environ); env["LD_PRELOAD"] = stub
    r = subprocess.run([EXE, DATA], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    cpp = {}
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            parts = line.split()
            cpp[parts[1]] = parts[2:]
    # the extraction runs on host threads (a contiguous range of the graph each, tables concatenated in graph order, rows of the noise /
    # calibration tables handed out afterwards in first-occurrence order): the same tables for any thread count
    # (and the walk over the Values cut into key ranges -- three walkers over the two symbol ranges of the SfM example, over the plain
    # integer keys of the pose graphs: the same variable order)
    env_mt = dict(env); env_mt["GTG_HOST_THREADS"] = "5"; env_mt["GTG_EXTRACT_GRAIN"] = "3"; env_mt["GTG_VALUES_WALKERS"] = "3"
    r_mt = subprocess.run([EXE, DATA], env=env_mt, capture_output=True, text=True, timeout=300)
    assert r_mt.returncode == 0 and "ALL PASSED" in r_mt.stdout, r_mt.stdout[-2000:] + r_mt.stderr[-2000:]
    # (the records as a multiset per case: the library uploads the measurements and noise rows on a helper thread beside its analysis, so
    # the ORDER of the copies is not fixed)
    cases = lambda out: [(ln.split()[1], sorted(ln.split()[2:])) for ln in out.splitlines() if ln.startswith("CASE ")]
    assert cases(r_mt.stdout) == cases(r.stdout)
    py = HP.run_snippet(_CHILD % {"root": ROOT, "data": DATA})
    assert set(cpp) == set(py) == {"sfmexample_bal_dubrovnik_3_7", "pose2slam_w100", "pose3slam_pose3example", "mixed_every_branch"}
    for name in cpp:
        assert len(cpp[name]) > 30
        assert sorted(cpp[name]) == sorted(py[name]), name
