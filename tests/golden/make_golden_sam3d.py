#!/usr/bin/env python3
"""tests/golden/make_golden_sam3d.py -- golden fixtures for BearingRangeFactor / RangeFactor / BearingFactor <Pose3, Point3> (gtsam/sam)
from the REAL reference.

Run in the build container only (needs the reference's sources and `make -C oracle ref`):

    python tests/golden/make_golden_sam3d.py

Compiles tests/golden/make_golden_sam3d.cpp against oracle/_ref into tests/_build/libgolden_sam3d.so and drives it through ctypes, in
the pattern of make_golden_stereo.py.  Every recorded number is computed by the reference's own code; the graphs come from
gtsam_amd/datasets.py through the API mirror's extractor, so the fixture's `p_*` arrays are the gtg_problem tables of
include/gtsam_amd.h.  The measured bearings are stored as the reference holds them: Unit3's constructor normalises what it is given,
so every bearing is passed through it twice: nearly all are then its fixed points (a few keep alternating between two
neighbouring doubles in one component, one ulp from what the reference then holds).

  sam3d_mixed.npz  datasets.sam3d_mixed_graph(): all three kinds beside monocular and stereo factors on shared landmarks, every noise
                   kind, Huber and Cauchy, one factor per branch of Unit3::localCoordinates / Unit3::basis.  Measurement noise:
                   0.004 rad on a bearing, 0.02 on a range (the dataset's defaults, seed 3).
  sam3d_slam.npz   datasets.landmark_slam3d_graph(): 40 poses, 300 landmarks, 3 000 bearing / range factors, no camera factor and
                   n_calib = 0; default LevenbergMarquardtParams.  Measurement noise: 0.005 rad, 0.03 (the defaults, seed 11).

Keys: those of the stereo fixtures (p_<field>, values0, error, jac1..jac4, hessian_diagonal, gradient, solve{i}_*, trace,
final_values, iterations, trace_reversed, trace_stable, solve0_delta_reversed) and jac5 = the sam factors in table order, 30 doubles
each in the layout of GTG_FAC_SAM.  sam3d_mixed also records the indices, among the sam factors, of its branch factors: branch_same,
branch_opposite, branch_tie (datasets.sam3d_mixed_graph) and axis_x, axis_y, axis_z (a bearing-carrying factor whose predicted
direction has its strictly smallest component on that axis).  Both fixtures must print trace_stable = 1; the generator fails otherwise.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from gtsam_amd import api as A  # noqa: E402
from gtsam_amd import datasets as D  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GTSAM_REF", "/root/reference")
LIB = os.path.join(ROOT, "tests", "_build", "libgolden_sam3d.so")
FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data", "noise_robust", "noise_robust_param",
          "proj_pose", "proj_point", "proj_z", "proj_noise", "proj_calib", "proj_sensor", "calib", "calib_distortion", "sensor",
          "stereo_pose", "stereo_point", "stereo_z", "stereo_noise", "stereo_calib", "stereo_sensor", "calib_baseline",
          "sam_kind", "sam_pose", "sam_point", "sam_z", "sam_noise",
          "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise")


def build_lib():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    ref_lib = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mavx2", "-mfma", "-w", "-shared", "-I" + os.path.join(ref_lib, "include"),
                    "-I" + REF, "-I" + os.path.join(REF, "gtsam", "3rdparty", "Eigen"), "-I" + os.path.join(REF, "gtsam", "3rdparty"),
                    "-I" + os.path.join(ROOT, "include"), "-o", LIB, os.path.join(HERE, "make_golden_sam3d.cpp"),
                    "-L" + ref_lib, "-lgtsam_ref", "-Wl,-rpath," + ref_lib], check=True)
    lib = C.CDLL(LIB)
    lib.sref_create.restype = C.c_void_p
    lib.sref_create.argtypes = [C.c_void_p]
    lib.sref_destroy.argtypes = [C.c_void_p]
    lib.sref_unit3.argtypes = [C.c_void_p, C.c_void_p]
    lib.sref_error.restype = C.c_double
    lib.sref_error.argtypes = [C.c_void_p, C.c_void_p]
    lib.sref_jacobians.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    lib.sref_hessian_diagonal_gradient.argtypes = [C.c_void_p] * 4
    lib.sref_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.sref_retract.argtypes = [C.c_void_p] * 4
    lib.sref_lm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def as_the_reference_holds(lib, p):
    """sam_z's bearings through the reference's Unit3 constructor, twice."""
    z = p.sam_z.reshape(-1, 4).copy()
    for row, kind in zip(z, p.sam_kind):
        if kind == 1:
            continue
        for _ in range(2):
            out = np.zeros(3)
            lib.sref_unit3(np.ascontiguousarray(row[:3]).ctypes.data, out.ctypes.data)
            row[:3] = out
    p.sam_z = z.reshape(-1)


def accept_sequence(trace):
    """What a trajectory did at every outer iteration: the inner iterations it spent there (1 = its first lambda was accepted)."""
    return np.diff(trace[:, 0]).astype(np.int64)


def record(lib, p, v0):
    cp = p.to_ctypes()
    h = lib.sref_create(C.addressof(cp))
    assert h, "the reference graph could not be built"
    v0 = np.ascontiguousarray(v0, np.float64)
    nd = int(p.dim_offsets()[-1])
    out = {"p_" + f: getattr(p, f) for f in FIELDS}
    out["values0"] = v0
    out["error"] = lib.sref_error(h, v0.ctypes.data)
    for ft, n, w in ((1, p.n_proj, 20), (2, p.n_between, 78), (3, p.n_prior, 90), (4, p.n_stereo, 30), (5, p.n_sam, 30)):
        if n:
            J = np.zeros((n, w))
            assert lib.sref_jacobians(h, v0.ctypes.data, ft, J.ctypes.data, J.size) == 0
            out[f"jac{ft}"] = J
    hd, gr = np.zeros(nd), np.zeros(nd)
    lib.sref_hessian_diagonal_gradient(h, v0.ctypes.data, hd.ctypes.data, gr.ctypes.data)
    out["hessian_diagonal"], out["gradient"] = hd, gr
    for i, (lam, dd) in enumerate(((1e-3, False), (1e-4, True))):
        delta, le = np.zeros(nd), np.zeros(2)
        rc = lib.sref_solve(h, v0.ctypes.data, lam, int(dd), 1e-6, 1e32, 0, delta.ctypes.data, le.ctypes.data)
        out[f"solve{i}_lambda"] = lam; out[f"solve{i}_diag"] = dd; out[f"solve{i}_status"] = rc
        out[f"solve{i}_delta"] = delta; out[f"solve{i}_linerr"] = le
        if rc == 0:
            tr = np.zeros_like(v0)
            lib.sref_retract(h, v0.ctypes.data, delta.ctypes.data, tr.ctypes.data)
            out[f"solve{i}_retract"] = tr; out[f"solve{i}_trial_error"] = lib.sref_error(h, tr.ctypes.data)
        if i == 0:
            d2 = np.zeros(nd)
            assert lib.sref_solve(h, v0.ctypes.data, lam, int(dd), 1e-6, 1e32, 1, d2.ctypes.data, le.copy().ctypes.data) == rc
            out["solve0_delta_reversed"] = d2
    runs = []
    for rev in (0, 1):
        trace, vals, nt = np.zeros((256, 3)), np.zeros_like(v0), C.c_int(0)
        it = lib.sref_lm(h, v0.ctypes.data, rev, vals.ctypes.data, 256, trace.ctypes.data, C.byref(nt))
        runs.append((trace[:nt.value].copy(), vals, it))
    out["trace"], out["final_values"], out["iterations"] = runs[0]
    out["trace_reversed"] = runs[1][0]
    a, b = accept_sequence(runs[0][0]), accept_sequence(runs[1][0])
    out["trace_stable"] = int(a.size == b.size and np.array_equal(a, b))
    lib.sref_destroy(h)
    return out


def axis_factors(p, v0):
    """The first bearing-carrying sam factor whose predicted direction has its strictly smallest component on x, on y and on z."""
    off = p.val_offsets()
    found = {}
    for k in range(p.n_sam):
        if p.sam_kind[k] == 1:
            continue
        T = v0[off[p.sam_pose[k]]:off[p.sam_pose[k]] + 12]; pt = v0[off[p.sam_point[k]]:off[p.sam_point[k]] + 3]
        q = np.abs(T[:9].reshape(3, 3).T @ (pt - T[9:]))
        a = int(np.argmin(q))
        if np.sum(q == q[a]) == 1:
            found.setdefault("xyz"[a], k)
    return found


def main():
    lib = build_lib()
    graph, initial, branch = D.sam3d_mixed_graph()
    p, v0, _ = A.extract(graph, initial)
    as_the_reference_holds(lib, p)
    out = record(lib, p, v0)
    for name, k in branch.items():
        out["branch_" + name] = k
    axes = axis_factors(p, v0)
    assert set(axes) == {"x", "y", "z"}, axes
    for a, k in axes.items():
        out["axis_" + a] = k
    np.savez_compressed(os.path.join(HERE, "sam3d_mixed.npz"), **out)
    print("sam3d_mixed:", p.n_sam, "sam,", p.n_stereo, "stereo,", p.n_proj, "projection factors; error", out["error"], "->", out["trace"][-1],
          "iterations", out["iterations"], "stable", out["trace_stable"], "solve status", out["solve0_status"], out["solve1_status"])
    print("  branch rows b:", {n: out["jac5"][k, 27:] for n, k in branch.items()}, "axes", axes)
    print(out["trace"]); print(out["trace_reversed"])
    assert out["trace_stable"] == 1

    graph, initial = D.landmark_slam3d_graph()
    p, v0, _ = A.extract(graph, initial)
    as_the_reference_holds(lib, p)
    assert p.calib.size == 0 and p.n_proj == 0 and p.n_stereo == 0
    out = record(lib, p, v0)
    np.savez_compressed(os.path.join(HERE, "sam3d_slam.npz"), **out)
    print("sam3d_slam:", p.n_sam, "sam factors,", p.n_vars, "variables; error", out["error"], "->", out["trace"][-1],
          "iterations", out["iterations"], "stable", out["trace_stable"])
    print(out["trace"]); print(out["trace_reversed"])
    assert out["trace_stable"] == 1
    for n in ("sam3d_mixed", "sam3d_slam"):
        print(n, os.path.getsize(os.path.join(HERE, n + ".npz")), "bytes")


if __name__ == "__main__":
    main()
