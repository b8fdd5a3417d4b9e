"""The bulk kernel's look-ahead (csrc/chol_dataflow.hip: a workgroup claims its next ticket before it has finished the current task
and fetches that task's descriptor, first step and first flag polls under it) on the host-thread emulation of
tests/test_dataflow_emulated.py -- the kernels' own source, one process per workgroup.

A workgroup now holds two tickets.  The smallest grids are where that can go wrong: with ONE bulk workgroup every dependency of the
held ticket sits in the same workgroup, which must run its tickets in order.  Pieces of one and of two steps make part_flag chains
that cross the task boundary at which the next ticket is held; one case has accumulator lanes; grids of tasks - 1, tasks and
tasks + 1 workgroups make claimed indices past the end of the list, which must be neither executed nor lost.  Every run must end
(each emulator process has a time limit; hitting it fails the test), the factor must pass the numpy check of the existing helper,
and it must be the same to the bit whatever the grid."""
import subprocess

import numpy as np
import pytest

from tests import test_dataflow_emulated as E

T = E.T
EMU_TIMEOUT_S = 600


@pytest.fixture(scope="module")
def exe():
    return E._build(E.EXE, [])


@pytest.fixture(autouse=True)
def _bounded_emulator(monkeypatch):
    """The helper's own limit is generous; a look-ahead that deadlocks should fail soon."""
    real = subprocess.run

    def run(cmd, *a, **kw):
        if isinstance(cmd, (list, tuple)) and cmd and str(cmd[0]).endswith("dataflow_emu"):
            kw["timeout"] = EMU_TIMEOUT_S
        return real(cmd, *a, **kw)
    monkeypatch.setattr(E.subprocess, "run", run)


def _bits(nt):
    S, X = E.factor.last
    return S.copy(), X.reshape(nt, T * T)[:, :14336].copy()   # (the rest of a diagonal tile's slot is scratch of the chain kernel)


@pytest.mark.parametrize("nt", [3, 4, 6])
@pytest.mark.parametrize("k_piece,k_final", [(1, 1), (2, 2)])
def test_lookahead_on_small_grids(exe, tmp_path, nt, k_piece, k_final):
    ref = None
    for n_bulk in (1, 2, 3):
        E.factor(exe, nt, n_bulk, k_piece, k_final, tmp_path)
        got = _bits(nt)
        if ref is None:
            ref = got
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), n_bulk


def _plan_with_lanes(orig):
    """plan_dense gives a tile accumulator lanes from 8 early pieces on (an 11-tile system, minutes of host threads).  The same rule
    from `lane_min` early pieces on, two lanes: early piece r accumulates in lane r mod 2 (lane 1 from zero, in a scratch slot behind
    the stored tiles), the final piece adds the lanes up in lane order."""
    def plan(nt, k_piece, k_final, lane_min=8, lane_max=8):
        P = orig(nt, k_piece, k_final, lane_min=10 ** 9)
        tasks = P["tasks"].copy(); lanes = {}; n_scratch = 0
        for t in tasks:
            if t[4] == t[5] - 1 and t[5] - 1 >= lane_min:
                lanes[(int(t[0]), int(t[1]))] = (2, P["n_slots"] + n_scratch); n_scratch += 1
        for t in tasks:
            if (int(t[0]), int(t[1])) in lanes:
                t[8], t[9] = lanes[(int(t[0]), int(t[1]))]
        P.update(tasks=tasks, lanes=lanes, n_scratch=n_scratch)
        return P
    return plan


@pytest.mark.parametrize("n_bulk", [1, 2])
def test_lookahead_with_accumulator_lanes(exe, tmp_path, monkeypatch, n_bulk):
    monkeypatch.setattr(E, "plan_dense", _plan_with_lanes(E.plan_dense))
    P = E.factor(exe, 6, n_bulk, 1, 1, tmp_path, lane_min=2)
    assert P["lanes"] and P["n_scratch"] > 0


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_lookahead_with_a_grid_around_the_task_count(exe, tmp_path, extra):
    """Two tile columns with the right-hand-side row: five tasks.  With as many workgroups as tasks (or one more) every workgroup's second
    claim -- and one workgroup's first -- is an index past the end."""
    n_tasks = len(E.plan_dense(2, 4, 4)["tasks"])
    assert n_tasks == 5
    E.factor(exe, 2, n_tasks + extra, 4, 4, tmp_path)
    S, X = _bits(2)
    E.factor(exe, 2, 1, 4, 4, tmp_path)
    S1, X1 = _bits(2)
    assert np.array_equal(S, S1) and np.array_equal(X, X1)
