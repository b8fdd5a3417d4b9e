"""Shared by the partial pose prior tests (tests/test_pose_partial_*.py, tests/test_gpu_pose_partial*.py): the fixtures of
tests/golden/make_golden_pose_partial.py as Problems, loaded once per process and never modified, and the scenes behind them."""
import functools

import numpy as np

from tests.stereo_support import device_noise_data, fixture, problem_of, rel  # noqa: F401

FIXTURES = ("pose_partial_graph3d", "pose_partial_vo", "pose_partial_graph2d")
ROWS = {(0, 0): 3, (1, 0): 3, (0, 3): 2, (1, 3): 1}       # (kind, variable type) -> rows of the factor
DIM = {0: 6, 3: 3}                                        # variable type -> tangent dimension


@functools.lru_cache(maxsize=None)
def scene(name):
    """(graph, initial values, info) of the scene a fixture was recorded on, at the fixture's seed."""
    from gtsam_amd import datasets as D
    build = {"pose_partial_graph3d": D.pose_partial_graph3d, "pose_partial_vo": D.pose_partial_vo_graph,
             "pose_partial_graph2d": D.pose_partial_graph2d}[name]
    return build(seed=int(fixture(name)["seed"]))


def rows_of(p):
    """Per partial prior: (rows, tangent dimension of its pose)."""
    vt = p.var_type[p.pose_partial_var]
    return np.array([ROWS[(int(k), int(t))] for k, t in zip(p.pose_partial_kind, vt)]), np.array([DIM[int(t)] for t in vt])


def unused_entries(p):
    """Boolean mask [n, 90] of the record entries a partial prior does not have: everything but its R x d block and its R rhs rows."""
    R, d = rows_of(p)
    mask = np.ones((p.n_pose_partial, 90), bool)
    for i in range(p.n_pose_partial):
        mask[i, :R[i] * d[i]] = False
        mask[i, 81:81 + R[i]] = False
    return mask


TEXT_FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data", "noise_robust", "noise_robust_param",
               "proj_pose", "proj_point", "proj_z", "proj_noise", "proj_calib", "proj_sensor", "calib", "sensor",
               "smart_ptr", "smart_cam", "smart_z", "smart_noise", "smart_params", "smart_calib", "smart_sensor",
               "between_v1", "between_v2", "between_z", "between_noise",
               "pose_partial_kind", "pose_partial_var", "pose_partial_z", "pose_partial_noise")


def write_problem_text(path, p, values, jac6=None):
    """The dump tests/cpp/pose_partial_graph_text.h reads: `name count` and the numbers (17 significant digits: exact round trip);
    jac6: the partial priors' records to carry along."""
    with open(path, "w") as f:
        for name in TEXT_FIELDS + ("values",) + (("jac6",) if jac6 is not None else ()):
            a = np.asarray(values if name == "values" else jac6 if name == "jac6" else getattr(p, name)).reshape(-1)
            f.write(f"{name} {a.size}\n" + " ".join(repr(float(x)) for x in a) + "\n")
