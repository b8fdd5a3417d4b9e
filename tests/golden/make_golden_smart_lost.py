#!/usr/bin/env python3
"""tests/golden/make_golden_smart_lost.py -- golden fixtures for smart factors with TriangulationParameters::useLOST from the REAL reference.

Run in the build container only (needs the reference's sources and `make -C oracle ref`):

    python tests/golden/make_golden_smart_lost.py

Compiles tests/golden/make_golden_smart_lost.cpp against oracle/_ref into tests/_build/libgolden_smart_lost.so and drives it through
ctypes, after the pattern of make_golden_smart_rig.py.  Every recorded number is computed by the reference's own code; the graphs come
from gtsam_amd/datasets.py (SMART_LOST_SCENES) through the API mirror's extractor, so the fixture's `p_*` arrays are the gtg_problem
tables of include/gtsam_amd.h.  Fixtures: smart_lost_cam, smart_lost_cam_epi (camera-type, the second with enableEPI), smart_lost_pose
(pose-type with a body_P_sensor, LOST and DLT factors mixed), smart_lost_rig (rig-type, poses repeated inside tracks, a triangulation
noise model).

Keys: those of the smart-pose fixtures (p_<field>, seed, values0, error, tri_status / tri_point, hessian_diagonal,
solve{i}_lambda/_diag/_status/_delta/_linerr/_retract/_trial_error, ceres_trace / legacy_trace, ceres_values / legacy_values,
ceres_trace_reversed / legacy_trace_reversed, trace_stable, solve0_delta_reversed) and, per smart factor,
  lost_kind          0 triangulateLOST returns a point, 1 it throws on the rank, 2 it throws in the partner search, -1 a DLT factor or a
                     single measurement;
  lost_pivots        |R_11|, |R_22|, |R_33| of the generator's own Eigen::ColPivHouseholderQR of the matrix it rebuilds (kind 0 / 1);
  lost_gaps          at the first two pivot choices, (largest - next) / largest of the remaining column norms;
  tri_point_spread   the largest relative deviation (max |p' - p| / max |p|) of the reference's own point over 16 evaluations with every
                     pose (or camera) entry and every pixel multiplied by 1 +- 2^-52 at random;
  dlt_status / dlt_point   the reference's result for the same track with useLOST off.

Conditions enforced here, on the CPU (they are not test tolerances; the seed advances until they hold): trace_stable == 1; the rebuilt
system reproduces triangulateLOST's point (1e-9 relative) and its throw / no throw; every pivot ratio |R_kk| / |R_11| lies a factor 16
or more away from rankTolerance; every pivot choice has a gap of at least 1e-6; the perturbed evaluations keep every status; VALID,
DEGENERATE by rank, DEGENERATE by an exhausted partner search (two coinciding measurements), a VALID three-measurement track whose first
two measurements coincide, FAR_POINT and OUTLIER all occur; on some VALID track the LOST and the DLT point differ by more than 1e-6
relative; track and measurement counts are no multiples of 64 and a track crosses a 64-measurement boundary; smart_lost_pose mixes
LOST and DLT factors; smart_lost_rig repeats a pose inside a VALID track."""
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
LIB = os.path.join(ROOT, "tests", "_build", "libgolden_smart_lost.so")
FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data", "noise_robust", "noise_robust_param", "calib", "sensor",
          "smart_ptr", "smart_cam", "smart_z", "smart_noise", "smart_params", "smart_calib", "smart_sensor", "smart_meas_calib", "smart_meas_sensor",
          "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise")
VALID, DEGENERATE, BEHIND_CAMERA, OUTLIER, FAR_POINT = range(5)


def build_lib():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    ref_lib = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-mavx2", "-mfma", "-w", "-shared", "-I" + os.path.join(ref_lib, "include"),
                    "-I" + REF, "-I" + os.path.join(REF, "gtsam", "3rdparty", "Eigen"), "-I" + os.path.join(REF, "gtsam", "3rdparty"),
                    "-I" + os.path.join(ROOT, "include"), "-o", LIB, os.path.join(HERE, "make_golden_smart_lost.cpp"),
                    "-L" + ref_lib, "-lgtsam_ref", "-Wl,-rpath," + ref_lib], check=True)
    lib = C.CDLL(LIB)
    lib.slost_create.restype = C.c_void_p
    lib.slost_create.argtypes = [C.c_void_p]
    lib.slost_destroy.argtypes = [C.c_void_p]
    lib.slost_error.restype = C.c_double
    lib.slost_error.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.slost_triangulate.argtypes = [C.c_void_p] * 4
    lib.slost_system.argtypes = [C.c_void_p] * 6
    lib.slost_hessian_diagonal.argtypes = [C.c_void_p] * 3
    lib.slost_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.slost_retract.argtypes = [C.c_void_p] * 4
    lib.slost_lm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def accept_sequence(trace):
    """What a trajectory did at every outer iteration: the inner iterations it spent there (1 = its first lambda was accepted)."""
    return np.diff(trace[:, 0]).astype(np.int64)


def open_ref(lib, p):
    cp = p.to_ctypes()
    h = lib.slost_create(C.addressof(cp))
    assert h, "the reference graph could not be built"
    return h


def triangulate(lib, p, v0):
    h = open_ref(lib, p)
    st, pts = np.zeros(p.n_smart, np.int32), np.zeros((p.n_smart, 3))
    v0 = np.ascontiguousarray(v0, np.float64)
    assert lib.slost_triangulate(h, v0.ctypes.data, st.ctypes.data, pts.ctypes.data) == 0
    lib.slost_destroy(h)
    return st, pts


def with_fields(p, **fields):
    q = type(p)(**{f: np.array(getattr(p, f)) for f in p.__dataclass_fields__})
    for k, v in fields.items():
        setattr(q, k, v)
    return q


def spread(lib, p, v0, st, pts, rng):
    """tri_point_spread; None when a perturbed evaluation changes a status"""
    out = np.zeros(p.n_smart)
    scale = np.maximum(np.abs(pts).max(axis=1), 1e-300)
    for _ in range(16):
        flip = lambda a: a * (1.0 + rng.choice([-1.0, 1.0], a.shape) * 2.0 ** -52)
        st2, pts2 = triangulate(lib, with_fields(p, smart_z=flip(np.array(p.smart_z))), flip(np.array(v0)))
        if not np.array_equal(st2, st):
            return None
        out = np.maximum(out, np.abs(pts2 - pts).max(axis=1) / scale)
    return np.where(st == VALID, out, 0.0)


def record(lib, p, v0):
    h = open_ref(lib, p)
    v0 = np.ascontiguousarray(v0, np.float64)
    nd = int(p.dim_offsets()[-1])
    out = {"p_" + f: getattr(p, f) for f in FIELDS}
    out["values0"] = v0
    threw = C.c_int(0)
    out["error"] = lib.slost_error(h, v0.ctypes.data, C.byref(threw))
    if threw.value:
        lib.slost_destroy(h); return None
    st, pts = np.zeros(p.n_smart, np.int32), np.zeros((p.n_smart, 3))
    if lib.slost_triangulate(h, v0.ctypes.data, st.ctypes.data, pts.ctypes.data) != 0:
        lib.slost_destroy(h); return None
    out["tri_status"], out["tri_point"] = st, pts
    kind, piv, gaps, mis = np.zeros(p.n_smart, np.int32), np.zeros((p.n_smart, 3)), np.zeros((p.n_smart, 2)), np.zeros(p.n_smart)
    rc = lib.slost_system(h, v0.ctypes.data, kind.ctypes.data, piv.ctypes.data, gaps.ctypes.data, mis.ctypes.data)
    if rc == -9:
        lib.slost_destroy(h); return None
    assert rc == 0, ("the rebuilt LOST system and triangulateLOST disagree", rc)
    assert mis.max() <= 1e-9, ("the rebuilt LOST system does not reproduce triangulateLOST's point", mis.max())
    out["lost_kind"], out["lost_pivots"], out["lost_gaps"] = kind, piv, gaps
    hd = np.zeros(nd)
    if lib.slost_hessian_diagonal(h, v0.ctypes.data, hd.ctypes.data) != 0:
        print("  linearize throws at values0"); lib.slost_destroy(h); return None
    out["hessian_diagonal"] = hd
    for i, (lam, dd) in enumerate(((1e-3, False), (1e-4, True))):
        delta, le = np.zeros(nd), np.zeros(2)
        rc = lib.slost_solve(h, v0.ctypes.data, lam, int(dd), 1e-6, 1e32, 0, delta.ctypes.data, le.ctypes.data)
        out[f"solve{i}_lambda"] = lam; out[f"solve{i}_diag"] = dd; out[f"solve{i}_status"] = rc
        out[f"solve{i}_delta"] = delta; out[f"solve{i}_linerr"] = le
        if rc == 0:
            tr = np.zeros_like(v0)
            lib.slost_retract(h, v0.ctypes.data, delta.ctypes.data, tr.ctypes.data)
            out[f"solve{i}_retract"] = tr; out[f"solve{i}_trial_error"] = lib.slost_error(h, tr.ctypes.data, C.byref(threw))
            if threw.value:
                lib.slost_destroy(h); return None
        if i == 0:
            d2 = np.zeros(nd)
            assert lib.slost_solve(h, v0.ctypes.data, lam, int(dd), 1e-6, 1e32, 1, d2.ctypes.data, le.copy().ctypes.data) == rc
            out["solve0_delta_reversed"] = d2
    stable = True
    for tag, ceres in (("ceres", 1), ("legacy", 0)):
        runs = []
        for rev in (0, 1):
            trace, vals, nt = np.zeros((256, 3)), np.zeros_like(v0), C.c_int(0)
            if lib.slost_lm(h, v0.ctypes.data, ceres, rev, vals.ctypes.data, 256, trace.ctypes.data, C.byref(nt)) < 0:
                print("  the LM run throws:", tag, "reversed" if rev else ""); lib.slost_destroy(h); return None
            runs.append((trace[:nt.value].copy(), vals))
        out[tag + "_trace"], out[tag + "_values"] = runs[0]
        out[tag + "_trace_reversed"] = runs[1][0]
        a, b = accept_sequence(runs[0][0]), accept_sequence(runs[1][0])
        stable = stable and a.size == b.size and np.array_equal(a, b)
    out["trace_stable"] = int(stable)
    lib.slost_destroy(h)
    # the same tracks with useLOST off
    prm = np.array(p.smart_params).reshape(-1, 8); prm[:, 7] = 0.0
    out["dlt_status"], out["dlt_point"] = triangulate(lib, with_fields(p, smart_params=prm.reshape(-1)), v0)
    return out


def conditions(name, p, out, info):
    """None when the fixture meets every condition, else what it misses"""
    st, kind, piv, gaps = out["tri_status"], out["lost_kind"], out["lost_pivots"], out["lost_gaps"]
    prm = p.smart_params.reshape(-1, 8)
    what = np.array(info["kind"])
    m = np.diff(p.smart_ptr)
    if out["trace_stable"] != 1 or out["solve0_status"] != 0 or out["solve1_status"] != 0:
        return "unstable trace or a failed solve"
    built = kind >= 0
    built &= kind <= 1
    ratio = piv[built] / piv[built][:, :1]
    tol = prm[built, :1]
    if np.any((ratio < 16 * tol) & (ratio > tol / 16)):
        return "a pivot ratio within a factor 16 of rankTolerance"
    if np.any(gaps[built] < 1e-6):
        return "a tie between column norms"
    if not np.all((kind == 1) == ((what == "thin") & (prm[:, 7] > 0))):
        return "rank failures are not exactly the thin tracks"
    for s in (VALID, DEGENERATE, FAR_POINT, OUTLIER):
        if not np.any((st == s) & (prm[:, 7] > 0)):
            return f"status {s} missing among the LOST tracks"
    if not (np.any(kind == 1) and np.any((kind == 2) & (m == 2) & (what == "coincide")) and np.all(st[kind >= 1] == DEGENERATE)):
        return "both DEGENERATE paths must occur"
    if not np.all(st[(what == "dup_first") & (prm[:, 7] > 0)] == VALID):
        return "a duplicated-first-camera track is not VALID"
    both = (st == VALID) & (out["dlt_status"] == VALID) & (prm[:, 7] > 0)
    gap = np.abs(out["tri_point"] - out["dlt_point"]).max(axis=1) / np.maximum(np.abs(out["tri_point"]).max(axis=1), 1e-300)
    if not np.any(both & (gap > 1e-6)):
        return "LOST and DLT agree everywhere"
    n_meas = int(p.smart_ptr[-1])
    assert p.n_smart % 64 and n_meas % 64
    if not np.any((p.smart_ptr[:-1] // 64 != (p.smart_ptr[1:] - 1) // 64) & (st == VALID) & (prm[:, 7] > 0)):
        return "no VALID LOST track crosses a 64-measurement boundary"
    if name == "smart_lost_pose" and not (np.any(prm[:, 7] == 0) and np.any(prm[:, 7] > 0) and np.any(p.smart_sensor >= 0)):
        return "smart_lost_pose must mix LOST and DLT factors and have a body_P_sensor"
    if name == "smart_lost_rig":
        rep = np.array([np.unique(p.smart_cam[a:b]).size < b - a for a, b in zip(p.smart_ptr[:-1], p.smart_ptr[1:])])
        if not np.any(rep & (st == VALID) & (what == "random")):
            return "no VALID rig track repeats a pose"
    return None


def main():
    lib = build_lib()
    for name, spec in D.SMART_LOST_SCENES.items():
        for variant in [None] + list(spec["variants"]):
            full = name if variant is None else name + "_" + variant
            for seed in range(64):
                graph, initial, info = D.smart_lost_scene(name, seed, variant)
                p, v0, _ = A.extract(graph, initial)
                out = record(lib, p, v0)
                if out is None:
                    print(full, "seed", seed, "rejected: the reference throws"); continue
                why = conditions(name, p, out, info)
                if why is None:
                    sp = spread(lib, p, v0, out["tri_status"], out["tri_point"], np.random.default_rng(seed))
                    if sp is None:
                        why = "a status changes under a perturbation of 2^-52"
                if why is None:
                    break
                print(full, "seed", seed, "rejected:", why, "; status counts", np.bincount(out["tri_status"], minlength=5))
            else:
                raise SystemExit(full + ": no seed meets the conditions")
            out["tri_point_spread"] = sp
            out["seed"] = seed
            path = os.path.join(HERE, full + ".npz")
            np.savez_compressed(path, **out)
            assert os.path.getsize(path) < 512 * 1024
            print(full, "seed", seed, ":", p.n_smart, "smart factors,", int(p.smart_ptr[-1]), "measurements; status",
                  np.bincount(out["tri_status"], minlength=5), "lost kinds", np.bincount(out["lost_kind"] + 1, minlength=4),
                  "largest spread", sp.max(), "error", out["error"], "-> ceres", out["ceres_trace"][-1], "legacy", out["legacy_trace"][-1],
                  os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
