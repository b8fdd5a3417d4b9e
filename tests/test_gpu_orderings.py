"""GPU: the order of the reduced variables and what follows from it (layout hash, reduced dimension, flops over the stored tiles and at
block level) are, key for key, what the library computed before the ordering became a unit of its own (csrc/ordering.cpp):
tests/golden/orderings_parent.json, recorded on the MI355X with the parent commit's library by tests/golden/make_golden_orderings.py.
Device and host reverse Cuthill-McKee, minimum degree, the tile-level choice of `auto`, the caller's order, nested dissection tried,
forced and switched off, under both tile schedules.  Upload only, no solve; no tolerance."""
import json

import pytest

from tests.golden import make_golden_orderings as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with open(G.OUT) as f:
        return json.load(f)


def test_fixture_covers_every_case(parent):
    assert sorted(parent) == sorted(G.CASES)


@pytest.mark.parametrize("case", list(G.CASES))
def test_ordering_equals_parent(case, parent):
    import torch
    assert torch.cuda.is_available()
    now, then = G.record(case), parent[case]
    print(case, now)
    assert sorted(now) == sorted(then)
    for key in sorted(then):
        assert now[key] == then[key], (case, key, now[key], then[key])
