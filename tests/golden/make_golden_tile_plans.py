#!/usr/bin/env python3
"""Generator of tests/golden/tile_plans_parent.json: sizes and digests of the two tile schedules of the reduced-system Cholesky
(stream schedule: cholesky_plan(); dataflow schedule: df_plan() and the device tables df_device_tables()) as the library built them
BEFORE the planner moved into csrc/tile_plan.cpp.  tests/test_gpu_tile_plans.py holds every later build to these digests.

Run on the GPU with the library of the commit to pin (GTSAM_AMD_LIB names it):

    GTSAM_AMD_LIB=/path/to/parent/libgtsam_amd.so python tests/golden/make_golden_tile_plans.py

Every case is recorded twice, in two fresh processes; the recordings must agree key for key before the file is written."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "tile_plans_parent.json")

# case -> (workload of tools/host_profile.py::problem_for, environment of the upload)
CASES = {
    "bal60": ("bal:60:6000:7", {}),                                   # nt = 5, one chain, < 1024 tasks: the host resolve loop
    "sphere2500_nd": ("sphere2500", {}),                              # parts, several chains, the device resolve
    "sphere2500_one_part": ("sphere2500", {"GTG_ND_DEPTH": "0"}),     # one chain, banded: the pull rules
    "bal60_dense": ("bal:60:6000:7", {"GTG_DENSE_PLAN": "1"}),        # the dense plan
}
ENV_KEYS = ("GTG_ND_DEPTH", "GTG_DENSE_PLAN")


def _digest(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(case):
    """Upload only, no solve: the record of one case with the library that is loaded.  The caller's environment is put back."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from gtsam_amd import lib as L
    from tools import host_profile as HP
    workload, env = CASES[case]
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        problem, _ = HP.problem_for(workload)
        dev = L.DeviceGraph(problem)
        try:
            chol, df, tables = dev.cholesky_plan(), dev.df_plan(), dev.df_device_tables()
            rec = {"nt": int(chol["nt"]), "n_tasks": int(df["tasks"].shape[0]), "n_stored": int(chol["stored"].shape[0]),
                   "cholesky_flops": float(dev.cholesky_flops()).hex(), "cholesky_flops_executed": float(dev.cholesky_flops_executed()).hex(),
                   "structure_hash": dev.structure_hash()}
        finally:
            dev.close()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert df["nt"] == rec["nt"] and df["active"]
    rec["cholesky_plan"] = {k: _digest(v) for k, v in sorted(chol.items()) if k != "nt"}
    rec["df_plan"] = {k: _digest(df[k]) for k in ("tasks", "klist", "chain_off", "chain_tiles", "seq")}
    rec["df_device_tables"] = {k: _digest(v) for k, v in zip(("tasks", "steps", "chain"), tables)}
    return rec


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        print("TILEPLANS " + json.dumps({case: record(case) for case in CASES}, sort_keys=True), flush=True)
        sys.exit(0)
    runs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, check=True, timeout=600)
        runs.append(json.loads([line for line in r.stdout.splitlines() if line.startswith("TILEPLANS ")][-1][len("TILEPLANS "):]))
    assert runs[0] == runs[1], "two recordings of the same library differ"
    assert sorted(runs[0]) == sorted(CASES) and all(sorted(r) == sorted(runs[0]["bal60"]) for r in runs[0].values())
    with open(OUT, "w") as f:
        json.dump(runs[0], f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, "from", os.environ.get("GTSAM_AMD_LIB") or "the tree's library")
