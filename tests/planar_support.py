"""Shared by the planar landmark SLAM tests (tests/test_planar_*.py, tests/test_gpu_planar*.py): the fixtures of
tests/golden/make_golden_planar.py as Problems, loaded once per process and never modified, the host compile of the planar evaluators
(tests/hostmath/hostmath_planar.cpp) and what the tests compute from records."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from tests.stereo_support import device_noise_data, fixture, problem_of, rel  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("planar_mixed", "planar_slam")
ROWS = {0: 2, 1: 1, 2: 1}                                 # sam kind -> rows of the factor
POINT2, POSE2 = 4, 3


def example_problem(g):
    """(Problem, initial values) of the PlanarSLAMExample graph a fixture carries (its ex_p_* arrays)."""
    from gtsam_amd.problem import Problem
    return Problem(**{k[5:]: np.array(v) for k, v in g.items() if k.startswith("ex_p_")}), g["ex_values0"]


@functools.lru_cache(maxsize=None)
def hostmath():
    so = os.path.join(ROOT, "tests", "_build", "libhostmath_planar.so")
    src = os.path.join(ROOT, "tests", "hostmath", "hostmath_planar.cpp")
    deps = [src, os.path.join(ROOT, "gtsam_amd", "csrc", "factors.h"), os.path.join(ROOT, "gtsam_amd", "csrc", "geom.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.hmpl_factors.argtypes = [C.c_long] + [C.c_void_p] * 14
    lib.hmpl_unwhitened.argtypes = [C.c_int] + [C.c_void_p] * 4
    assert lib.hmpl_record_size() == 21 and [lib.hmpl_rows(k) for k in (0, 1, 2)] == [2, 1, 1]
    return lib


def evaluate(p, values, n=None):
    """(records [n, 21], errors [n]) of the first n planar factors of p at `values`, by the host-compiled evaluators."""
    hm = hostmath()
    n = p.n_sam2 if n is None else n
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    kind, pose, point, nz = i32(p.sam2_kind), i32(p.sam2_pose), i32(p.sam2_point), i32(p.sam2_noise)
    z = np.ascontiguousarray(p.sam2_z, np.float64)
    values = np.ascontiguousarray(values, np.float64)
    voff, nd = p.val_offsets(), device_noise_data(p)
    rk, rp = i32(p.noise_robust), np.ascontiguousarray(p.noise_robust_param, np.float64)
    J, e = np.zeros((n, 21)), np.zeros(n)
    hm.hmpl_factors(n, kind.ctypes.data, pose.ctypes.data, point.ctypes.data, z.ctypes.data, nz.ctypes.data, values.ctypes.data, voff.ctypes.data,
                    p.noise_kind.ctypes.data, p.noise_off.ctypes.data, nd.ctypes.data, rk.ctypes.data, rp.ctypes.data, J.ctypes.data, e.ctypes.data)
    return J, e


def unwhitened(p, values, k):
    """The unwhitened record [H_pose 3x3 | H_point 3x3 | Local(h, z) 3] of planar factor k."""
    off = p.val_offsets()
    x = np.ascontiguousarray(values[off[p.sam2_pose[k]]:][:3]); l = np.ascontiguousarray(values[off[p.sam2_point[k]]:][:3])
    z = np.ascontiguousarray(p.sam2_z[3 * k:3 * k + 3]); J = np.zeros(21)
    hostmath().hmpl_unwhitened(int(p.sam2_kind[k]), x.ctypes.data, l.ctypes.data, z.ctypes.data, J.ctypes.data)
    return J


def unused_entries(p, n=None):
    """Boolean mask [n, 21] of the record entries a planar factor does not have: the rows beyond its own and A2's third column."""
    n = p.n_sam2 if n is None else n
    mask = np.zeros((n, 21), bool)
    for i in range(n):
        R = ROWS[int(p.sam2_kind[i])]
        mask[i, 3 * R:9] = True; mask[i, 9 + 3 * R:18] = True; mask[i, 18 + R:] = True
        mask[i, 11:18:3] = True
    return mask


def error_of_records(p, J, noise):
    """The error of factors from their whitened records' b (numpy, float64 sums): 0.5 |b|^2, the loss recovered for Huber and Cauchy."""
    err = 0.0
    for k in range(J.shape[0]):
        b = J[k, 18:]
        nz = int(noise[k]); bb = float(b @ b); kk = float(p.noise_robust_param[nz])
        if p.noise_robust[nz] == 2:      # Huber: the record's b is sqrt(w) r with w = k / |r| outside the quadratic zone: |b|^2 = k |r|
            err += 0.5 * bb if bb <= kk * kk else kk * (bb / kk - kk / 2)
        elif p.noise_robust[nz] == 3:    # Cauchy: w = k^2 / (k^2 + |r|^2), so |r|^2 = |b|^2 k^2 / (k^2 - |b|^2); loss k^2 / 2 log1p(|r|^2 / k^2)
            err += 0.5 * kk * kk * np.log1p(bb / (kk * kk - bb))
        else:
            assert p.noise_robust[nz] == 0
            err += 0.5 * bb
    return err


def gradient_of_records(p, J):
    """J^T b of planar records, in the padded tangent layout."""
    doff = p.dim_offsets()
    grad = np.zeros(int(doff[-1]))
    for k in range(J.shape[0]):
        A1 = J[k, :9].reshape(3, 3); A2 = J[k, 9:18].reshape(3, 3); b = J[k, 18:]
        grad[doff[p.sam2_pose[k]]:doff[p.sam2_pose[k]] + 3] += A1.T @ b
        grad[doff[p.sam2_point[k]]:doff[p.sam2_point[k]] + 3] += A2.T @ b
    return grad


def third_entries(p):
    """Indices, in the packed values / tangent vectors (the two layouts coincide in a planar graph), of every POINT2's third entry."""
    off = p.val_offsets()
    assert np.array_equal(off, p.dim_offsets())
    return off[:-1][p.var_type == POINT2] + 2


TEXT_FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data", "noise_robust", "noise_robust_param",
               "sam2_kind", "sam2_pose", "sam2_point", "sam2_z", "sam2_noise",
               "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise",
               "pose_partial_kind", "pose_partial_var", "pose_partial_z", "pose_partial_noise")


def write_problem_text(path, p, values):
    """The dump tests/cpp/planar_graph_text.h reads: `name count` and the numbers (17 significant digits: exact round trip)."""
    with open(path, "w") as f:
        for name in TEXT_FIELDS + ("values",):
            a = np.asarray(values if name == "values" else getattr(p, name)).reshape(-1)
            f.write(f"{name} {a.size}\n" + " ".join(repr(float(x)) for x in a) + "\n")
