"""Shared by the useLOST tests (tests/test_smart_lost_*.py, tests/test_gpu_smart_lost*.py): the fixtures of
tests/golden/make_golden_smart_lost.py as Problems, loaded once per process and never modified."""
import functools

import numpy as np

from gtsam_amd.problem import SMART_RIG
from tests.stereo_support import fixture, problem_of, rel  # noqa: F401  (the same loaders: p_* arrays -> Problem)

FIXTURES = ("smart_lost_cam", "smart_lost_cam_epi", "smart_lost_pose", "smart_lost_rig")
VALID, DEGENERATE, BEHIND_CAMERA, OUTLIER, FAR_POINT = range(5)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return fixture(name)


def load(name):
    """(fixture, Problem, packed initial values)"""
    g = _fixture(name)
    return g, problem_of(g), np.array(g["values0"])


def is_camera_type(p):
    return p.smart_calib.size == 0


def track(p, i):
    """(variable ids, measurements 2 per row, calib index per measurement, sensor index per measurement) of smart factor i; the two
    index arrays are empty for a camera-type factor"""
    k0, k1 = int(p.smart_ptr[i]), int(p.smart_ptr[i + 1])
    ids, z = np.ascontiguousarray(p.smart_cam[k0:k1], np.int32), np.ascontiguousarray(p.smart_z[2 * k0:2 * k1])
    if is_camera_type(p):
        return ids, z, np.zeros(0, np.int32), np.zeros(0, np.int32)
    if p.smart_calib[i] == SMART_RIG:
        return ids, z, np.ascontiguousarray(p.smart_meas_calib[k0:k1], np.int32), np.ascontiguousarray(p.smart_meas_sensor[k0:k1], np.int32)
    si = int(p.smart_sensor[i]) if p.smart_sensor.size else -1
    return ids, z, np.full(k1 - k0, int(p.smart_calib[i]), np.int32), np.full(k1 - k0, si, np.int32)


def point_error(got, want):
    """per track: max |got - want| / max |want|"""
    got, want = np.asarray(got, np.float64).reshape(-1, 3), np.asarray(want, np.float64).reshape(-1, 3)
    return np.abs(got - want).max(axis=1) / np.maximum(np.abs(want).max(axis=1), 1e-300)


def point_tolerance(g):
    """per track: max(1e-12, 8 x tri_point_spread) -- the spread is the reference's own deviation under input perturbations of 2^-52; the
    factor 8 because the device's arithmetic differs in its order too, not only in the rounding of its inputs"""
    return np.maximum(1e-12, 8.0 * np.asarray(g["tri_point_spread"]))


def lost_dlt_gap(g):
    """per track: the relative distance between the reference's LOST and DLT points (0 where either has no point or the factor is DLT)"""
    both = (g["tri_status"] == VALID) & (g["dlt_status"] == VALID) & (g["lost_kind"] == 0)
    return np.where(both, point_error(g["tri_point"], np.where(both[:, None], g["dlt_point"], 1.0)), 0.0)


TEXT_FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data", "calib", "sensor",
               "smart_ptr", "smart_cam", "smart_z", "smart_noise", "smart_params", "smart_calib", "smart_sensor",
               "smart_meas_calib", "smart_meas_sensor",
               "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise")


def write_problem_text(path, p, values):
    """`name count` and the numbers (17 significant digits: exact round trip), the dump the C++ tests of this feature read"""
    with open(path, "w") as f:
        for name in TEXT_FIELDS + ("values",):
            a = np.asarray(values if name == "values" else getattr(p, name)).reshape(-1)
            f.write(f"{name} {a.size}\n" + " ".join(repr(float(x)) for x in a) + "\n")
