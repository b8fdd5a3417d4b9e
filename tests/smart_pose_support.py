"""Shared by the SmartProjectionPoseFactor<Cal3_S2> tests (tests/test_smart_pose_*.py, tests/test_gpu_smart_pose*.py): the fixtures of
tests/golden/make_golden_smart_pose.py as Problems, loaded once per process and never modified."""
import numpy as np

from tests.stereo_support import fixture, problem_of, rel  # noqa: F401  (the same loaders: p_* arrays -> Problem)

FIXTURES = ("smart_pose_example", "smart_pose_mixed", "smart_pose_far_ignore", "smart_pose_far_infinity", "smart_pose_far_jacobian_q")
VALID, DEGENERATE, BEHIND_CAMERA, OUTLIER, FAR_POINT = range(5)


def load(name):
    """(fixture, Problem, packed initial values)"""
    g = fixture(name)
    return g, problem_of(g), np.array(g["values0"])


def device_calib(p):
    """the calibration table as the device holds it: fx fy s u0 v0 + four distortion coefficients (zero for a Cal3_S2)"""
    c = np.zeros((p.calib.size // 5, 9))
    c[:, :5] = p.calib.reshape(-1, 5)
    return np.ascontiguousarray(c)


def track(p, i):
    """(pose ids, measurements 2 per row, calib index, sensor index) of smart factor i"""
    k0, k1 = int(p.smart_ptr[i]), int(p.smart_ptr[i + 1])
    si = int(p.smart_sensor[i]) if p.smart_sensor.size else -1
    return np.ascontiguousarray(p.smart_cam[k0:k1], np.int32), np.ascontiguousarray(p.smart_z[2 * k0:2 * k1]), int(p.smart_calib[i]), si


TEXT_FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data",
               "proj_pose", "proj_point", "proj_z", "proj_noise", "proj_calib", "proj_sensor", "calib", "sensor",
               "smart_ptr", "smart_cam", "smart_z", "smart_noise", "smart_params", "smart_calib", "smart_sensor",
               "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise")


def write_problem_text(path, p, values):
    """The dump tests/cpp/smart_pose_graph_text.h reads: `name count` and the numbers (17 significant digits: exact round trip)."""
    with open(path, "w") as f:
        for name in TEXT_FIELDS + ("values",):
            a = np.asarray(values if name == "values" else getattr(p, name)).reshape(-1)
            f.write(f"{name} {a.size}\n" + " ".join(repr(float(x)) for x in a) + "\n")
