"""Shared by the bearing / range tests (tests/test_sam_*.py, tests/test_gpu_sam*.py): the fixtures of tests/golden/make_golden_sam3d.py
as Problems, loaded once per process and never modified."""
import numpy as np

from tests import stereo_support as S
from tests.stereo_support import fixture, problem_of, rel  # noqa: F401


def stereo_mixed_step(lib):
    """Everything one linearisation and three lambda tries of stereo_mixed (a three-row graph WITHOUT sam factors) compute, for the
    bit comparison with the recording made with the parent commit's library (tests/golden/stereo_mixed_step_parent.npz)."""
    g = S.fixture("stereo_mixed")
    dev = lib.DeviceGraph(S.problem_of(g))
    dev.set_values(g["values0"])
    got = {"error": np.float64(dev.error())}
    dev.linearize()
    for ft in (1, 2, 3, 4):
        got[f"jac{ft}"] = dev.jacobians(ft)
    got["hessian_diagonal"], got["gradient"] = dev.hessian_diagonal(), dev.gradient()
    for i, (lam, dd) in enumerate(((1e-3, False), (1e-4, True))):
        rc, out = dev.try_lambda(lam, dd)
        got[f"rc{i}"], got[f"out{i}"], got[f"delta{i}"], got[f"trial{i}"] = np.int64(rc), out, dev.delta(), dev.trial_values()
    rc, out, its = dev.try_lambda_pcg(1e-3, False, max_iterations=300, min_iterations=1, epsilon_rel=1e-10, epsilon_abs=1e-14)
    got["rc_pcg"], got["out_pcg"], got["delta_pcg"], got["its_pcg"] = np.int64(rc), out, dev.delta(), np.int64(its)
    dev.close()
    return got


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
