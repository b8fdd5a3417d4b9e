"""Shared by the Cal3Fisheye tests (tests/test_fisheye_*.py, tests/test_gpu_fisheye*.py): the fixtures of
tests/golden/make_golden_fisheye.py as Problems, loaded once per process and never modified, the host compile of the fisheye evaluators
(tests/hostmath/hostmath_fisheye.cpp) and what the tests compute from records."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from tests.stereo_support import device_noise_data, fixture, problem_of, rel  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("fisheye_mixed", "fisheye_example")
BRANCHES = ("on_axis", "taylor", "behind")
FISHEYE = 1                                              # GTG_CALIB_FISHEYE


@functools.lru_cache(maxsize=None)
def hostmath():
    so = os.path.join(ROOT, "tests", "_build", "libhostmath_fisheye.so")
    src = os.path.join(ROOT, "tests", "hostmath", "hostmath_fisheye.cpp")
    deps = [src, os.path.join(ROOT, "gtsam_amd", "csrc", "factors.h"), os.path.join(ROOT, "gtsam_amd", "csrc", "geom.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.hmfe_factors.argtypes = [C.c_long] + [C.c_void_p] * 18
    lib.hmfe_uncalibrate.argtypes = [C.c_void_p] * 4
    lib.hmfe_scaling.restype = C.c_double
    lib.hmfe_scaling.argtypes = [C.c_double]
    lib.hmfe_project.argtypes = [C.c_void_p] * 6
    assert lib.hmfe_record_size() == 20 and lib.hmfe_calib_stride() == 9
    return lib


def calib9(p):
    """The calib table as the device holds it: 9 doubles per row, fx fy s u0 v0 and the row of calib_distortion."""
    n = p.calib.size // 5
    K = np.zeros((n, 9))
    K[:, :5] = p.calib.reshape(n, 5)
    if p.calib_distortion.size:
        K[:, 5:] = p.calib_distortion.reshape(n, 4)
    return K


def models(p):
    """The model of every calib row (zeros for a Problem without a list)."""
    n = p.calib.size // 5
    return np.ascontiguousarray(p.calib_model if p.calib_model.size else np.zeros(n), np.int32)


def is_fisheye(p):
    """Per projection factor: its calib row is a Cal3Fisheye."""
    return models(p)[p.proj_calib] == FISHEYE


def evaluate(p, values, n=None):
    """(records [n, 20], errors [n]) of the first n projection factors of p at `values`, by the host-compiled evaluators."""
    hm = hostmath()
    n = p.n_proj if n is None else n
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    f64 = lambda a: np.ascontiguousarray(a, np.float64)
    pose, point, nz, cal = i32(p.proj_pose), i32(p.proj_point), i32(p.proj_noise), i32(p.proj_calib)
    sen = i32(p.proj_sensor if p.proj_sensor.size else np.full(p.n_proj, -1))
    z, K, m, S, values = f64(p.proj_z), f64(calib9(p)), models(p), f64(p.sensor if p.sensor.size else np.zeros(12)), f64(values)
    voff, nd = p.val_offsets(), device_noise_data(p)
    rk, rp = i32(p.noise_robust), f64(p.noise_robust_param)
    J, e = np.zeros((n, 20)), np.zeros(n)
    hm.hmfe_factors(n, pose.ctypes.data, point.ctypes.data, z.ctypes.data, nz.ctypes.data, cal.ctypes.data, sen.ctypes.data, K.ctypes.data,
                    m.ctypes.data, S.ctypes.data, values.ctypes.data, voff.ctypes.data, p.noise_kind.ctypes.data, p.noise_off.ctypes.data,
                    nd.ctypes.data, rk.ctypes.data, rp.ctypes.data, J.ctypes.data, e.ctypes.data)
    return J, e


def uncalibrate(K9, pn):
    """(pixel [2], d(pixel)/d(intrinsic point) [2, 2]) by the host-compiled fisheye_uncalibrate."""
    K9, pn = np.ascontiguousarray(K9, np.float64), np.ascontiguousarray(pn, np.float64)
    pi, D = np.zeros(2), np.zeros((2, 2))
    hostmath().hmfe_uncalibrate(K9.ctypes.data, pn.ctypes.data, pi.ctypes.data, D.ctypes.data)
    return pi, D


def project(T12, K9, pw):
    """(ok, pixel [2], Dpose [2, 6], Dpoint [2, 3]) by the host-compiled fisheye_project."""
    T12, K9, pw = (np.ascontiguousarray(a, np.float64) for a in (T12, K9, pw))
    pi, Dp, Dl = np.zeros(2), np.zeros((2, 6)), np.zeros((2, 3))
    ok = hostmath().hmfe_project(T12.ctypes.data, K9.ctypes.data, pw.ctypes.data, pi.ctypes.data, Dp.ctypes.data, Dl.ctypes.data)
    return bool(ok), pi, Dp, Dl


def sums_from_records(p, J):
    """(error, gradient J^T b) of projection factors from their whitened records (numpy, float64 sums): 0.5 |b|^2, the loss recovered
    for Huber and Cauchy."""
    doff = p.dim_offsets()
    grad = np.zeros(int(doff[-1]))
    err = 0.0
    for k in range(J.shape[0]):
        A1 = J[k, :12].reshape(2, 6); A2 = J[k, 12:18].reshape(2, 3); b = J[k, 18:]
        grad[doff[p.proj_pose[k]]:doff[p.proj_pose[k]] + 6] += A1.T @ b
        grad[doff[p.proj_point[k]]:doff[p.proj_point[k]] + 3] += A2.T @ b
        nz = int(p.proj_noise[k]); bb = float(b @ b); kk = float(p.noise_robust_param[nz])
        if p.noise_robust[nz] == 2:      # Huber: the record's b is sqrt(w) r with w = k / |r| outside the quadratic zone: |b|^2 = k |r|
            err += 0.5 * bb if bb <= kk * kk else kk * (bb / kk - kk / 2)
        elif p.noise_robust[nz] == 3:    # Cauchy: w = k^2 / (k^2 + |r|^2), so |r|^2 = |b|^2 k^2 / (k^2 - |b|^2); loss k^2 / 2 log1p(|r|^2 / k^2)
            err += 0.5 * kk * kk * np.log1p(bb / (kk * kk - bb))
        else:
            assert p.noise_robust[nz] == 0
            err += 0.5 * bb
    return err, grad


def extractor_cases():
    """(Problem, values) of the graphs both extractors are compared on: fisheye_mixed, and the FisheyeExample graph with its two priors
    moved behind the projection factors -- the text dump rebuilds a graph in the order projection, between, prior, and the noise table
    gets its rows in graph order."""
    from gtsam_amd import api as A
    from gtsam_amd import datasets as D
    g = fixture("fisheye_mixed")
    graph, initial = D.fisheye_example_graph()
    graph.factors = graph.factors[2:] + graph.factors[:2]
    p, v0, _ = A.extract(graph, initial)
    return [(problem_of(g), g["values0"]), (p, v0)]


TEXT_FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data", "noise_robust", "noise_robust_param",
               "proj_pose", "proj_point", "proj_z", "proj_noise", "proj_calib", "proj_sensor", "calib", "calib_distortion", "calib_model", "sensor",
               "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise")


def write_problem_text(path, p, values):
    """The dump tests/cpp/fisheye_graph_text.h reads: `name count` and the numbers (17 significant digits: exact round trip)."""
    with open(path, "w") as f:
        for name in TEXT_FIELDS + ("values",):
            a = np.asarray(values if name == "values" else getattr(p, name)).reshape(-1)
            f.write(f"{name} {a.size}\n" + " ".join(repr(float(x)) for x in a) + "\n")
