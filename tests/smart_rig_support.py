"""Shared by the SmartProjectionRigFactor<PinholePose<Cal3_S2>> tests (tests/test_smart_rig_*.py, tests/test_gpu_smart_rig*.py): the
fixtures of tests/golden/make_golden_smart_rig.py as Problems, loaded once per process and never modified."""
import functools

import numpy as np

from gtsam_amd.problem import SMART_RIG
from tests.stereo_support import fixture, problem_of, rel  # noqa: F401  (the same loaders: p_* arrays -> Problem)

FIXTURES = ("smart_rig_pair", "smart_rig_mixed")
VALID, DEGENERATE, BEHIND_CAMERA, OUTLIER, FAR_POINT = range(5)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return fixture(name)


def load(name):
    """(fixture, Problem, packed initial values)"""
    g = _fixture(name)
    return g, problem_of(g), np.array(g["values0"])


def repeated(p):
    """per smart factor: it names a pose key more than once"""
    return np.array([np.unique(p.smart_cam[a:b]).size < b - a for a, b in zip(p.smart_ptr[:-1], p.smart_ptr[1:])])


def as_pose_type(p):
    """p, whose rig-type tracks each look through ONE (calib row, sensor row) pair, with those tracks written as pose-type factors
    (smart_calib = the row, smart_sensor = the row): the same graph in the tables of SmartProjectionPoseFactor."""
    q = problem_of({"p_" + k: getattr(p, k) for k in TEXT_FIELDS})
    sc, ss = np.array(p.smart_calib), np.array(p.smart_sensor if p.smart_sensor.size else np.full(p.n_smart, -1, np.int32))
    for i in range(p.n_smart):
        if sc[i] != SMART_RIG:
            continue
        a, b = int(p.smart_ptr[i]), int(p.smart_ptr[i + 1])
        assert np.all(p.smart_meas_calib[a:b] == p.smart_meas_calib[a]) and np.all(p.smart_meas_sensor[a:b] == p.smart_meas_sensor[a])
        sc[i], ss[i] = p.smart_meas_calib[a], p.smart_meas_sensor[a]
    q.smart_calib, q.smart_sensor = sc.astype(np.int32), ss.astype(np.int32)
    q.smart_meas_calib = np.zeros(0, np.int32); q.smart_meas_sensor = np.zeros(0, np.int32)
    return q


def one_camera_per_track(p):
    """p with every rig-type track cut down to the sightings through the camera of its first measurement: a rig whose tracks never repeat
    a key (a camera sees a landmark once per pose); tracks left with one sighting stay (DEGENERATE)."""
    keep = np.ones(p.smart_cam.size, bool)
    for i in np.flatnonzero(p.smart_calib == SMART_RIG):
        a, b = int(p.smart_ptr[i]), int(p.smart_ptr[i + 1])
        keep[a:b] = (p.smart_meas_calib[a:b] == p.smart_meas_calib[a]) & (p.smart_meas_sensor[a:b] == p.smart_meas_sensor[a])
        assert np.unique(p.smart_cam[a:b][keep[a:b]]).size == keep[a:b].sum()
    counts = np.array([keep[int(a):int(b)].sum() for a, b in zip(p.smart_ptr[:-1], p.smart_ptr[1:])])
    q = problem_of({"p_" + k: getattr(p, k) for k in TEXT_FIELDS})
    q.smart_cam = p.smart_cam[keep]; q.smart_z = p.smart_z.reshape(-1, 2)[keep].reshape(-1)
    q.smart_meas_calib = p.smart_meas_calib[keep]; q.smart_meas_sensor = p.smart_meas_sensor[keep]
    q.smart_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return q


TEXT_FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data",
               "proj_pose", "proj_point", "proj_z", "proj_noise", "proj_calib", "proj_sensor", "calib", "sensor",
               "smart_ptr", "smart_cam", "smart_z", "smart_noise", "smart_params", "smart_calib", "smart_sensor",
               "smart_meas_calib", "smart_meas_sensor",
               "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise")


def write_problem_text(path, p, values):
    """The dump tests/cpp/smart_rig_graph_text.h reads: `name count` and the numbers (17 significant digits: exact round trip)."""
    with open(path, "w") as f:
        for name in TEXT_FIELDS + ("values",):
            a = np.asarray(values if name == "values" else getattr(p, name)).reshape(-1)
            f.write(f"{name} {a.size}\n" + " ".join(repr(float(x)) for x in a) + "\n")
