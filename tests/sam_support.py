"""Shared by the bearing / range tests (tests/test_sam_*.py, tests/test_gpu_sam*.py): the fixtures of tests/golden/make_golden_sam3d.py
as Problems, loaded once per process and never modified."""
import numpy as np

from tests import stereo_support as S
from tests.stereo_support import fixture, problem_of, rel  # noqa: F401


TEXT_FIELDS = S.TEXT_FIELDS[:S.TEXT_FIELDS.index("between_v1")] + ("sam_kind", "sam_pose", "sam_point", "sam_z", "sam_noise") + \
    S.TEXT_FIELDS[S.TEXT_FIELDS.index("between_v1"):]


def write_problem_text(path, p, values):
    """The dump tests/cpp/sam_graph_text.h reads: `name count` and the numbers (17 significant digits: exact round trip)."""
    with open(path, "w") as f:
        for name in TEXT_FIELDS + ("values",):
            a = np.asarray(values if name == "values" else getattr(p, name)).reshape(-1)
            f.write(f"{name} {a.size}\n" + " ".join(repr(float(x)) for x in a) + "\n")


def extractor_cases():
    """(Problem, values) of the graphs both extractors are compared on: sam3d_mixed (every table, shared rows, every kind) and
    sam3d_slam (3 000 factors: more than one extraction chunk, no calibration table)."""
    return [(problem_of(g), g["values0"]) for g in (fixture("sam3d_mixed"), fixture("sam3d_slam"))]
