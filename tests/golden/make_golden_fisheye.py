#!/usr/bin/env python3
"""tests/golden/make_golden_fisheye.py -- golden fixtures for GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> from the REAL reference.

Run in the build container only (needs the reference's sources and `make -C oracle ref`):

    python tests/golden/make_golden_fisheye.py

Compiles tests/golden/make_golden_fisheye.cpp against oracle/_ref into tests/_build/libgolden_fisheye.so and drives it through ctypes,
in the pattern of make_golden_planar.py.  Every recorded number is computed by the reference's own code; the graphs come from
gtsam_amd/datasets.py through the API mirror's extractor, so the fixture's `p_*` arrays are the gtg_problem tables of
include/gtsam_amd.h and `p_calib_model` is what gtg_set_calibration_models takes.

  fisheye_mixed.npz    datasets.fisheye_mixed_graph(): two Cal3Fisheye (one skewed), a Cal3_S2 and a Cal3DS2, body_P_sensor on a third
                       of the factors, every noise kind, Huber and Cauchy, a between chain, a pose and a point prior, and one factor
                       per branch: branch_on_axis, branch_taylor, branch_behind (their indices among the projection factors).
  fisheye_example.npz  datasets.fisheye_example_graph(): the graph of examples/FisheyeExample.cpp under the reference's LM with default
                       LevenbergMarquardtParams.

The seed of the mixed graph is advanced until the reference's own run is stable under the reversed ordering (the same accept / reject
sequence), both damped solves succeed, the error falls, and no fisheye factor has r within a factor 2 of Scaling's threshold 1e-8
unless it was put into a branch on purpose; the generator fails if no seed of its range does.  The seed used is recorded (`seed`).

Keys: those of the planar fixtures (p_<field>, values0, error, jac1, jac2, jac3, hessian_diagonal, gradient, solve{i}_*, trace,
final_values, iterations, trace_reversed, trace_stable, solve0_delta_reversed) and probe = per projection factor (x, y, r, t, s) at
values0 for the rows of a Cal3Fisheye (zeros elsewhere and behind the camera).  fisheye_example.npz: p_<field>, values0, error, trace,
final_values, final_error, iterations.
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
LIB = os.path.join(ROOT, "tests", "_build", "libgolden_fisheye.so")
FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data", "noise_robust", "noise_robust_param",
          "proj_pose", "proj_point", "proj_z", "proj_noise", "proj_calib", "proj_sensor", "calib", "calib_distortion", "calib_model", "sensor",
          "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise")


def build_lib():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    ref_lib = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mavx2", "-mfma", "-w", "-shared", "-I" + os.path.join(ref_lib, "include"),
                    "-I" + REF, "-I" + os.path.join(REF, "gtsam", "3rdparty", "Eigen"), "-I" + os.path.join(REF, "gtsam", "3rdparty"),
                    "-I" + os.path.join(ROOT, "include"), "-o", LIB, os.path.join(HERE, "make_golden_fisheye.cpp"),
                    "-L" + ref_lib, "-lgtsam_ref", "-Wl,-rpath," + ref_lib], check=True)
    lib = C.CDLL(LIB)
    lib.fref_create.restype = C.c_void_p
    lib.fref_create.argtypes = [C.c_void_p, C.c_void_p]
    lib.fref_destroy.argtypes = [C.c_void_p]
    lib.fref_error.restype = C.c_double
    lib.fref_error.argtypes = [C.c_void_p, C.c_void_p]
    lib.fref_probe.argtypes = [C.c_void_p] * 3
    lib.fref_jacobians.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    lib.fref_hessian_diagonal_gradient.argtypes = [C.c_void_p] * 4
    lib.fref_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.fref_retract.argtypes = [C.c_void_p] * 4
    lib.fref_lm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def accept_sequence(trace):
    """What a trajectory did at every outer iteration: the inner iterations it spent there (1 = its first lambda was accepted)."""
    return np.diff(trace[:, 0]).astype(np.int64)


def open_ref(lib, p):
    cp = p.to_ctypes()
    model = np.ascontiguousarray(p.calib_model, np.int32)
    h = lib.fref_create(C.addressof(cp), model.ctypes.data if model.size else None)
    assert h, "the reference graph could not be built"
    return h, (cp, model)


def lm_run(lib, h, v0, rev):
    trace, vals, nt = np.zeros((256, 3)), np.zeros_like(v0), C.c_int(0)
    it = lib.fref_lm(h, v0.ctypes.data, rev, vals.ctypes.data, 256, trace.ctypes.data, C.byref(nt))
    return trace[:nt.value].copy(), vals, it


def record(lib, p, v0):
    h, keep = open_ref(lib, p)
    v0 = np.ascontiguousarray(v0, np.float64)
    nd = int(p.dim_offsets()[-1])
    out = {"p_" + f: getattr(p, f) for f in FIELDS}
    out["values0"] = v0
    out["error"] = lib.fref_error(h, v0.ctypes.data)
    probe = np.zeros((p.n_proj, 5))
    lib.fref_probe(h, v0.ctypes.data, probe.ctypes.data)
    out["probe"] = probe
    for ft, n, w in ((1, p.n_proj, 20), (2, p.n_between, 78), (3, p.n_prior, 90)):
        if n:
            J = np.zeros((n, w))
            assert lib.fref_jacobians(h, v0.ctypes.data, ft, J.ctypes.data, J.size) == 0
            out[f"jac{ft}"] = J
    hd, gr = np.zeros(nd), np.zeros(nd)
    lib.fref_hessian_diagonal_gradient(h, v0.ctypes.data, hd.ctypes.data, gr.ctypes.data)
    out["hessian_diagonal"], out["gradient"] = hd, gr
    for i, (lam, dd) in enumerate(((1e-3, False), (1e-4, True))):
        delta, le = np.zeros(nd), np.zeros(2)
        rc = lib.fref_solve(h, v0.ctypes.data, lam, int(dd), 1e-6, 1e32, 0, delta.ctypes.data, le.ctypes.data)
        out[f"solve{i}_lambda"] = lam; out[f"solve{i}_diag"] = dd; out[f"solve{i}_status"] = rc
        out[f"solve{i}_delta"] = delta; out[f"solve{i}_linerr"] = le
        if rc == 0:
            tr = np.zeros_like(v0)
            lib.fref_retract(h, v0.ctypes.data, delta.ctypes.data, tr.ctypes.data)
            out[f"solve{i}_retract"] = tr; out[f"solve{i}_trial_error"] = lib.fref_error(h, tr.ctypes.data)
        if i == 0:
            d2 = np.zeros(nd)
            assert lib.fref_solve(h, v0.ctypes.data, lam, int(dd), 1e-6, 1e32, 1, d2.ctypes.data, le.copy().ctypes.data) == rc
            out["solve0_delta_reversed"] = d2
    runs = [lm_run(lib, h, v0, rev) for rev in (0, 1)]
    out["trace"], out["final_values"], out["iterations"] = runs[0]
    out["trace_reversed"] = runs[1][0]
    a, b = accept_sequence(runs[0][0]), accept_sequence(runs[1][0])
    out["trace_stable"] = int(a.size == b.size and np.array_equal(a, b))
    lib.fref_destroy(h)
    return out


def near_threshold(p, probe, on_purpose=()):
    """The fisheye factors whose r lies within a factor 2 of Scaling's threshold 1e-8 at values0; factors put into a branch on purpose
    are exempt."""
    fish = p.calib_model[p.proj_calib] == 1
    return [(k, probe[k, 2]) for k in range(p.n_proj) if fish[k] and k not in on_purpose and 0.5e-8 <= probe[k, 2] <= 2e-8]


def conditions(p, out, on_purpose=()):
    """Why this seed cannot be recorded (an empty list: it can)."""
    why = []
    if out["trace_stable"] != 1:
        why.append("the trajectory depends on the ordering")
    if out["solve0_status"] != 0 or out["solve1_status"] != 0:
        why.append("a damped solve failed")
    if not out["trace"][-1, 1] < out["error"]:
        why.append("the error does not fall")
    bad = near_threshold(p, out["probe"], on_purpose)
    if bad:
        why.append(f"fisheye factors near the Taylor threshold: {bad}")
    return why


def example(lib):
    """The FisheyeExample graph: its tables, initial values, and the reference's own LM run with default parameters."""
    graph, initial = D.fisheye_example_graph()
    p, v0, _ = A.extract(graph, initial)
    h, keep = open_ref(lib, p)
    v0 = np.ascontiguousarray(v0, np.float64)
    out = {"p_" + f: getattr(p, f) for f in FIELDS}
    out["values0"] = v0
    out["error"] = lib.fref_error(h, v0.ctypes.data)
    out["trace"], out["final_values"], out["iterations"] = lm_run(lib, h, v0, 0)
    out["final_error"] = lib.fref_error(h, out["final_values"].ctypes.data)
    lib.fref_destroy(h)
    return out


def main():
    lib = build_lib()
    ex = example(lib)
    np.savez_compressed(os.path.join(HERE, "fisheye_example.npz"), **ex)
    print("FisheyeExample: error", ex["error"], "->", ex["final_error"], "in", ex["iterations"], "iterations")
    print(ex["trace"])
    seed0 = 0
    for seed in range(seed0, seed0 + 40):
        graph, initial, branch = D.fisheye_mixed_graph(seed=seed)
        p, v0, _ = A.extract(graph, initial)
        out = record(lib, p, v0)
        why = conditions(p, out, set(branch.values()))
        if not why:
            break
        print(f"fisheye_mixed: seed {seed} rejected:", "; ".join(why))
    else:
        raise SystemExit(f"fisheye_mixed: no seed in [{seed0}, {seed0 + 40}) meets the conditions")
    out["seed"] = seed
    for n, k in branch.items():
        out["branch_" + n] = k
    pr, J = out["probe"], out["jac1"]      # the branches are what they are named after
    k = branch["on_axis"]
    assert pr[k, 0] == 0.0 and pr[k, 1] == 0.0 and pr[k, 2] == 0.0 and J[k, :18].any(), "on_axis"
    k = branch["taylor"]
    assert 0.0 < pr[k, 2] < 0.5e-8, "taylor"
    k = branch["behind"]
    assert not J[k, :18].any() and J[k, 18] != 0.0 and not pr[k].any(), "behind"
    np.savez_compressed(os.path.join(HERE, "fisheye_mixed.npz"), **out)
    print(f"fisheye_mixed: seed {seed};", p.n_proj, "projection,", p.n_between, "between,", p.n_prior, "prior factors,", p.n_vars,
          "variables; models", p.calib_model, "error", out["error"], "->", out["trace"][-1], "iterations", out["iterations"], "stable",
          out["trace_stable"], "solve status", out["solve0_status"], out["solve1_status"])
    print("  branch records:", {n: out["jac1"][k] for n, k in branch.items()}, {n: pr[k] for n, k in branch.items()})
    print(out["trace"]); print(out["trace_reversed"])
    for n in ("fisheye_mixed", "fisheye_example"):
        print(n, os.path.getsize(os.path.join(HERE, n + ".npz")), "bytes")


if __name__ == "__main__":
    main()
