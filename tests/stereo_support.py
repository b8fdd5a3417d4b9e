"""Shared by the stereo tests (tests/test_stereo_*.py, tests/test_gpu_stereo*.py): the fixtures of tests/golden/make_golden_stereo.py
as Problems, loaded once per process and never modified."""
import functools
import os

import numpy as np

from gtsam_amd.problem import NOISE_DIAGONAL, NOISE_GAUSSIAN, NOISE_ISOTROPIC, Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VO_FILES = ("VO_calibration.txt", "VO_camera_poses_large.txt", "VO_stereo_factors_large.txt")


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    for a in g.values():
        a.setflags(write=False)
    return g


def problem_of(g, **override):
    """The Problem behind a fixture's p_* arrays (fresh arrays: a test may trim its copy)."""
    fields = {k[2:]: np.array(v) for k, v in g.items() if k.startswith("p_")}
    fields.update(override)
    return Problem(**fields)


@functools.lru_cache(maxsize=None)
def vo_graph():
    """(graph, initial values) of examples/StereoVOExample_large.cpp through the API mirror, from tests/golden/data."""
    import gzip
    import shutil
    import tempfile
    from gtsam_amd import datasets as D
    with tempfile.TemporaryDirectory() as tmp:
        for n in VO_FILES:
            with gzip.open(os.path.join(GOLDEN, "data", n + ".gz"), "rb") as i, open(os.path.join(tmp, n), "wb") as o:
                shutil.copyfileobj(i, o)
        return D.stereo_vo_graph(*(os.path.join(tmp, n) for n in VO_FILES))


@functools.lru_cache(maxsize=None)
def vo_problem():
    """(Problem, packed initial values) of the VO graph; the fixture keeps every table but the measurements."""
    from gtsam_amd import api as A
    p, v0, _ = A.extract(*vo_graph())
    return p, v0


def device_noise_data(p):
    """noise_data as the device holds it: 1 / sigma, 1 / sigmas, R (csrc/upload.hip); offsets unchanged (Unit rows are empty)."""
    out = np.array(p.noise_data, np.float64)
    for i in range(p.noise_kind.size):
        o, d = int(p.noise_off[i]), int(p.noise_dim[i])
        if p.noise_kind[i] == NOISE_ISOTROPIC: out[o] = 1.0 / out[o]
        elif p.noise_kind[i] == NOISE_DIAGONAL: out[o:o + d] = 1.0 / out[o:o + d]
        elif p.noise_kind[i] == NOISE_GAUSSIAN: pass
    return out


def rel(a, b):
    """max |a - b| / max |b|: the measure of tests/test_gpu_parity.py"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


TEXT_FIELDS = ("var_type", "noise_kind", "noise_dim", "noise_off", "noise_data", "noise_robust", "noise_robust_param",
               "proj_pose", "proj_point", "proj_z", "proj_noise", "proj_calib", "proj_sensor", "calib", "calib_distortion", "sensor",
               "stereo_pose", "stereo_point", "stereo_z", "stereo_noise", "stereo_calib", "stereo_sensor", "calib_baseline",
               "between_v1", "between_v2", "between_z", "between_noise", "prior_var", "prior_off", "prior_data", "prior_noise")


def write_problem_text(path, p, values):
    """The dump tests/cpp/stereo_graph_text.h reads: `name count` and the numbers (17 significant digits: exact round trip)."""
    with open(path, "w") as f:
        for name in TEXT_FIELDS + ("values",):
            a = np.asarray(values if name == "values" else getattr(p, name)).reshape(-1)
            f.write(f"{name} {a.size}\n" + " ".join(repr(float(x)) for x in a) + "\n")


def extractor_cases():
    """(Problem, values) of the graphs both extractors are compared on: stereo_mixed (every table, shared rows) and the 8 189 stereo
    factors of the VO example (more than one extraction chunk)."""
    g = fixture("stereo_mixed")
    return [(problem_of(g), g["values0"]), vo_problem()]
