"""GPU: the tile schedules of the reduced-system Cholesky (csrc/tile_plan.cpp: stream schedule, dataflow schedule, the tables resolved
to slots on the host or by chol_dataflow.hip::k_df_resolve) are, digest for digest, the ones the library built before the planner became
a unit of its own: tests/golden/tile_plans_parent.json, recorded on the MI355X with the parent commit's library by
tests/golden/make_golden_tile_plans.py.  Upload only, no solve; no tolerance."""
import json

import pytest

from tests.golden import make_golden_tile_plans as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with open(G.OUT) as f:
        return json.load(f)


def test_fixture_covers_every_case(parent):
    assert sorted(parent) == sorted(G.CASES)


@pytest.mark.parametrize("case", list(G.CASES))
def test_plans_equal_parent(case, parent):
    import torch
    assert torch.cuda.is_available()
    now, then = G.record(case), parent[case]
    print(case, {k: now[k] for k in ("nt", "n_tasks", "n_stored", "cholesky_flops", "cholesky_flops_executed", "structure_hash")})
    assert sorted(now) == sorted(then)
    for key in sorted(then):
        assert now[key] == then[key], (case, key, now[key], then[key])
