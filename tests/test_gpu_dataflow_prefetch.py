"""GPU: the bulk kernel of the dataflow Cholesky (csrc/chol_dataflow.hip) claims its next ticket and fetches that task's descriptor,
first step and first flag polls UNDER the current task.  A workgroup then holds two tickets; the smallest grids are where that can
go wrong (with one bulk workgroup every dependency of the held ticket sits in the same workgroup), a grid that is no divisor of
anything (7) and the default grid are the other cases.

Every case: two lambda tries with different lambda on ONE handle (the epoch in the flags carries over), `delta` of each try
bit-equal to the same tries under the stream schedule (GTG_CHOL=streams: per-column launches, same sums in the same order on one
chain), no dependency wait that ran into its bound and no repeated try.  Each case runs in a fresh child process: GTG_DF_GRID is
read once per process."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from gtsam_amd import datasets as D
from gtsam_amd import lib as L
from gtsam_amd.problem import bal_problem
if %(problem)r == "bal45":
    p, v0 = bal_problem(*D.synthetic_bal(45, 1500, seed=1, n_loops=1))      # 405 reduced dimensions: 4 tile columns, a band with fill
    diag = True
else:
    p, v0 = D.random_pose_graph(200, 60, seed=4)                            # 1200 dimensions, 10 tiles: several chain slots, lanes
    diag = False
lambdas = (1e-3, 7e-2)
out = {}
for sched in ("df", "streams"):
    os.environ["GTG_CHOL"] = sched                                          # (read per factorisation)
    dev = L.DeviceGraph(p); dev.set_values(v0); dev.linearize()
    deltas, rcs, kinds = [], [], []
    for lam in lambdas:
        rc, _ = dev.try_lambda(lam, diag)
        rcs.append(int(rc)); deltas.append(dev.delta().tobytes().hex())
        if sched == "df":
            c = dev.df_ctrl(); kinds.append([int(c[8]), int(c[15]), int(c[0])])   # first wait that gave up (0: none), repeated tries, tickets taken
    out[sched] = dict(rc=rcs, delta=deltas, ctrl=kinds, finite=bool(np.isfinite(dev.delta()).all()))
    if sched == "df":
        pl = dev.df_plan()
        out[sched].update(active=bool(pl["active"]), n_tasks=int(pl["tasks"].shape[0]), nt=int(pl["nt"]))
    dev.close()
print("RESULT " + json.dumps(out))
'''


def _run(problem, grid):
    env = dict(os.environ)
    env.pop("GTG_CHOL", None); env.pop("GTG_DF_GRID", None); env.pop("GTG_DF_SINGLE", None); env.pop("GTG_DF_TRACE", None)
    if grid is not None:
        env["GTG_DF_GRID"] = str(grid)
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "problem": problem}], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _check(o):
    assert o["df"]["active"], "the dataflow schedule must be the one that ran"
    assert o["df"]["rc"] == o["streams"]["rc"] == [0, 0]
    assert o["df"]["finite"] and o["streams"]["finite"]
    for kind, repeated, tickets in o["df"]["ctrl"]:
        assert kind == 0 and repeated == 0, ("a dependency wait ran into its bound", o["df"]["ctrl"])
        assert tickets >= o["df"]["n_tasks"]                                 # every ticket taken
    assert o["df"]["delta"][0] != o["df"]["delta"][1]                       # (two different systems)
    for i in range(2):
        assert o["df"]["delta"][i] == o["streams"]["delta"][i], ("try", i)


@pytest.mark.parametrize("grid", [1, 2, 7, None], ids=["grid1", "grid2", "grid7", "default"])
def test_prefetching_bulk_kernel_equals_stream_schedule_bal45(grid):
    o = _run("bal45", grid)
    assert o["df"]["nt"] == 4
    _check(o)


def test_prefetching_bulk_kernel_equals_stream_schedule_posegraph200():
    _check(_run("posegraph200", None))
