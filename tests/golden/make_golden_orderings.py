#!/usr/bin/env python3
"""Generator of tests/golden/orderings_parent.json: the order of the reduced variables (reduced_order()), the layout it leads to
(structure_hash(), the reduced dimension) and the two flop counts (cholesky_flops(), cholesky_flops_block_level()) as the library
computed them BEFORE the ordering moved into csrc/ordering.cpp.  tests/test_gpu_orderings.py holds every later build to this record.

Run on the GPU with the library of the commit to pin (GTSAM_AMD_LIB names it):

    GTSAM_AMD_LIB=/path/to/parent/libgtsam_amd.so python tests/golden/make_golden_orderings.py

Every case is recorded twice, in two fresh processes; the recordings must agree key for key before the file is written."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "orderings_parent.json")

# case -> (workload of tools/host_profile.py::problem_for, environment of the upload)
CASES = {
    "bal60": ("bal:60:6000:7", {}),                                              # one part, reverse Cuthill-McKee on the device
    "bal60_host": ("bal:60:6000:7", {"GTG_HOST_ORDERING": "1"}),                 # the same order from the host unit
    "bal60_mindegree": ("bal:60:6000:7", {"GTG_ORDERING": "mindegree"}),
    "bal60_auto": ("bal:60:6000:7", {"GTG_ORDERING": "auto"}),                   # both orders scored at tile level
    "bal60_natural": ("bal:60:6000:7", {"GTG_ORDERING": "natural"}),             # the caller's order: the unit does not run
    "bal60_nd2": ("bal:60:6000:7", {"GTG_ND_DEPTH": "2"}),                       # below 256 reduced variables: one leaf
    "sphere2500": ("sphere2500", {}),                                            # nested dissection tried by the sparsity criterion
    "sphere2500_nd0": ("sphere2500", {"GTG_ND_DEPTH": "0"}),
    "sphere2500_nd2": ("sphere2500", {"GTG_ND_DEPTH": "2"}),                     # forced: kept whatever the chains gain
    "sphere2500_nd2_streams": ("sphere2500", {"GTG_ND_DEPTH": "2", "GTG_CHOL": "streams"}),
}
ENV_KEYS = ("GTG_HOST_ORDERING", "GTG_ORDERING", "GTG_ND_DEPTH", "GTG_CHOL")


def record(case):
    """Upload only, no solve: the record of one case with the library that is loaded.  The caller's environment is put back."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import numpy as np
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
            order = np.ascontiguousarray(dev.reduced_order(), dtype=np.int32)
            return {"reduced_order": hashlib.sha256(order.tobytes()).hexdigest(), "structure_hash": dev.structure_hash(),
                    "reduced_dim": int(dev.reduced_dim), "cholesky_flops": float(dev.cholesky_flops()).hex(),
                    "cholesky_flops_block_level": float(dev.cholesky_flops_block_level()).hex()}
        finally:
            dev.close()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        print("ORDERINGS " + json.dumps({case: record(case) for case in CASES}, sort_keys=True), flush=True)
        sys.exit(0)
    runs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, check=True, timeout=600)
        runs.append(json.loads([line for line in r.stdout.splitlines() if line.startswith("ORDERINGS ")][-1][len("ORDERINGS "):]))
    assert runs[0] == runs[1], "two recordings of the same library differ"
    assert sorted(runs[0]) == sorted(CASES) and all(sorted(r) == sorted(runs[0]["bal60"]) for r in runs[0].values())
    with open(OUT, "w") as f:
        json.dump(runs[0], f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, "from", os.environ.get("GTSAM_AMD_LIB") or "the tree's library")
