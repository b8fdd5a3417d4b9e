#!/usr/bin/env python3
"""tests/golden/make_golden_smart_rig.py -- golden fixtures for SmartProjectionRigFactor<PinholePose<Cal3_S2>> from the REAL reference.

Run in the build container only (needs the reference's sources and `make -C oracle ref`):

    python tests/golden/make_golden_smart_rig.py

Compiles tests/golden/make_golden_smart_rig.cpp against oracle/_ref into tests/_build/libgolden_smart_rig.so and drives it through
ctypes, after the pattern of make_golden_smart_pose.py.  Every recorded number is computed by the reference's own code; the graphs come
from gtsam_amd/datasets.py (SMART_RIG_SCENES) through the API mirror's extractor, so the fixture's `p_*` arrays are the gtg_problem
tables of include/gtsam_amd.h.

Keys: those of the smart-pose fixtures (p_<field>, seed, values0, error, tri_status / tri_point, hessian_diagonal,
solve{i}_lambda/_diag/_status/_delta/_linerr/_retract/_trial_error, ceres_trace / legacy_trace, ceres_values / legacy_values,
ceres_trace_reversed / legacy_trace_reversed, trace_stable, solve0_delta_reversed), with p_smart_meas_calib / p_smart_meas_sensor among
the tables.

Conditions checked here, on the CPU (they are not test tolerances): trace_stable == 1 for every fixture (the seed is advanced until it
holds); VALID, DEGENERATE and FAR_POINT tracks occur in both; on smart_rig_pair the reference's hessian_diagonal differs from the
per-observation formula diag(sum_o F_o^T F_o - sum_o E_o E_o^T) -- the reference's value plus the cross terms of every (pose, track)
group, computed here from the reference's own whitened F and E blocks -- by more than 1e-6 relative, so that a test can tell the two
apart; smart_rig_mixed has an OUTLIER track, a VALID track with a repeated key that crosses a 64-measurement boundary of the
projection range, track and measurement counts that are no multiples of 64, and a pose with more than 256 smart observations.
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
LIB = os.path.join(ROOT, "tests", "_build", "libgolden_smart_rig.so")
FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data", "noise_robust", "noise_robust_param",
          "proj_pose", "proj_point", "proj_z", "proj_noise", "proj_calib", "proj_sensor", "calib", "sensor",
          "smart_ptr", "smart_cam", "smart_z", "smart_noise", "smart_params", "smart_calib", "smart_sensor", "smart_meas_calib", "smart_meas_sensor",
          "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise")
VALID, DEGENERATE, BEHIND_CAMERA, OUTLIER, FAR_POINT = range(5)


def build_lib():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    ref_lib = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mavx2", "-mfma", "-w", "-shared", "-I" + os.path.join(ref_lib, "include"),
                    "-I" + REF, "-I" + os.path.join(REF, "gtsam", "3rdparty", "Eigen"), "-I" + os.path.join(REF, "gtsam", "3rdparty"),
                    "-I" + os.path.join(ROOT, "include"), "-o", LIB, os.path.join(HERE, "make_golden_smart_rig.cpp"),
                    "-L" + ref_lib, "-lgtsam_ref", "-Wl,-rpath," + ref_lib], check=True)
    lib = C.CDLL(LIB)
    lib.srref_create.restype = C.c_void_p
    lib.srref_create.argtypes = [C.c_void_p]
    lib.srref_destroy.argtypes = [C.c_void_p]
    lib.srref_error.restype = C.c_double
    lib.srref_error.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.srref_linearize_throws.argtypes = [C.c_void_p, C.c_void_p]
    lib.srref_triangulate.argtypes = [C.c_void_p] * 4
    lib.srref_hessian_diagonal.argtypes = [C.c_void_p] * 3
    lib.srref_cross_terms.argtypes = [C.c_void_p] * 3
    lib.srref_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.srref_retract.argtypes = [C.c_void_p] * 4
    lib.srref_lm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def accept_sequence(trace):
    """What a trajectory did at every outer iteration: the inner iterations it spent there (1 = its first lambda was accepted)."""
    return np.diff(trace[:, 0]).astype(np.int64)


def open_ref(lib, p):
    cp = p.to_ctypes()
    h = lib.srref_create(C.addressof(cp))
    assert h, "the reference graph could not be built"
    return h


def record(lib, p, v0):
    h = open_ref(lib, p)
    v0 = np.ascontiguousarray(v0, np.float64)
    nd = int(p.dim_offsets()[-1])
    out = {"p_" + f: getattr(p, f) for f in FIELDS}
    out["values0"] = v0
    threw = C.c_int(0)
    out["error"] = lib.srref_error(h, v0.ctypes.data, C.byref(threw))
    assert not threw.value
    st, pts = np.zeros(p.n_smart, np.int32), np.zeros((p.n_smart, 3))
    assert lib.srref_triangulate(h, v0.ctypes.data, st.ctypes.data, pts.ctypes.data) == 0
    out["tri_status"], out["tri_point"] = st, pts
    hd = np.zeros(nd)
    if lib.srref_hessian_diagonal(h, v0.ctypes.data, hd.ctypes.data) != 0:
        print("  linearize throws at values0"); lib.srref_destroy(h); return None
    out["hessian_diagonal"] = hd
    for i, (lam, dd) in enumerate(((1e-3, False), (1e-4, True))):
        delta, le = np.zeros(nd), np.zeros(2)
        rc = lib.srref_solve(h, v0.ctypes.data, lam, int(dd), 1e-6, 1e32, 0, delta.ctypes.data, le.ctypes.data)
        out[f"solve{i}_lambda"] = lam; out[f"solve{i}_diag"] = dd; out[f"solve{i}_status"] = rc
        out[f"solve{i}_delta"] = delta; out[f"solve{i}_linerr"] = le
        if rc == 0:
            tr = np.zeros_like(v0)
            lib.srref_retract(h, v0.ctypes.data, delta.ctypes.data, tr.ctypes.data)
            out[f"solve{i}_retract"] = tr; out[f"solve{i}_trial_error"] = lib.srref_error(h, tr.ctypes.data, C.byref(threw))
            assert not threw.value
        if i == 0:
            d2 = np.zeros(nd)
            assert lib.srref_solve(h, v0.ctypes.data, lam, int(dd), 1e-6, 1e32, 1, d2.ctypes.data, le.copy().ctypes.data) == rc
            out["solve0_delta_reversed"] = d2
    stable = True
    for tag, ceres in (("ceres", 1), ("legacy", 0)):
        runs = []
        for rev in (0, 1):
            trace, vals, nt = np.zeros((256, 3)), np.zeros_like(v0), C.c_int(0)
            if lib.srref_lm(h, v0.ctypes.data, ceres, rev, vals.ctypes.data, 256, trace.ctypes.data, C.byref(nt)) < 0:
                print("  the LM run throws:", tag, "reversed" if rev else ""); lib.srref_destroy(h); return None
            runs.append((trace[:nt.value].copy(), vals))
        out[tag + "_trace"], out[tag + "_values"] = runs[0]
        out[tag + "_trace_reversed"] = runs[1][0]
        a, b = accept_sequence(runs[0][0]), accept_sequence(runs[1][0])
        stable = stable and a.size == b.size and np.array_equal(a, b)
    out["trace_stable"] = int(stable)
    lib.srref_destroy(h)
    return out


def repeated(p):
    """per smart factor: it names a pose key more than once"""
    return np.array([np.unique(p.smart_cam[a:b]).size < b - a for a, b in zip(p.smart_ptr[:-1], p.smart_ptr[1:])])


def crosses_chunk(p, st):
    """a VALID track with a repeated key whose measurements lie on both sides of a 64-observation boundary of the projection range"""
    first = p.n_proj + p.smart_ptr[:-1]; last = p.n_proj + p.smart_ptr[1:] - 1
    return bool(np.any((st == VALID) & repeated(p) & (first // 64 != last // 64)))


def main():
    lib = build_lib()
    for name in D.SMART_RIG_SCENES:
        for seed in range(64):
            graph, initial, info = D.smart_rig_scene(name, seed)
            p, v0, _ = A.extract(graph, initial)
            out = record(lib, p, v0)
            if out is None:
                print(name, "seed", seed, "rejected: the reference throws a CheiralityException"); continue
            st = out["tri_status"]
            ok = out["trace_stable"] == 1 and out["solve0_status"] == 0 and out["solve1_status"] == 0
            ok = ok and all(np.any(st == s) for s in (VALID, DEGENERATE, FAR_POINT)) and np.any(repeated(p) & (st == VALID))
            if name == "smart_rig_pair":
                # what the per-observation formula would give: the reference's diagonal plus the cross terms of the repeated keys
                h = open_ref(lib, p)
                cross = np.zeros_like(out["hessian_diagonal"])
                assert lib.srref_cross_terms(h, np.ascontiguousarray(v0).ctypes.data, cross.ctypes.data) == 0
                lib.srref_destroy(h)
                gap = np.abs(cross).max() / np.abs(out["hessian_diagonal"]).max()
                print("  per-observation formula off by", gap, "relative")
                ok = ok and gap > 1e-6
            if name == "smart_rig_mixed":
                ok = ok and np.any(st == OUTLIER) and crosses_chunk(p, st) and np.bincount(p.smart_cam).max() > 256
                assert p.n_smart % 64 and (p.n_proj + int(p.smart_ptr[-1])) % 64 and int(p.smart_ptr[-1]) % 64
                assert np.any(p.smart_calib == -2) and np.any(p.smart_calib >= 0) and p.n_proj > 0 and p.n_between > 0
            if ok:
                break
            print(name, "seed", seed, "rejected: stable", out["trace_stable"], "status counts", np.bincount(st, minlength=5))
        else:
            raise SystemExit(name + ": no seed meets the conditions")
        out["seed"] = seed
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 512 * 1024
        print(name, "seed", seed, ":", p.n_smart, "smart factors,", int(p.smart_ptr[-1]), "measurements,", p.n_proj, "projection factors; status",
              np.bincount(st, minlength=5), "error", out["error"], "-> ceres", out["ceres_trace"][-1], "legacy", out["legacy_trace"][-1],
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
