"""The Python mirror for Cal3Fisheye on the CPU: Cal3Fisheye / GenericProjectionFactorCal3Fisheye -> extract() gives the gtg_problem tables
the fixtures of tests/golden/make_golden_fisheye.py record (the reference's harness was fed exactly these), the model of a calib row
follows the CLASS of its calibration object, a graph without a fisheye calibration has no model list, and include/gtsam_amd.h declares
the setter and the two model values."""
import os
import re

import numpy as np

from gtsam_amd import api as A
from gtsam_amd import datasets as D
from gtsam_amd import lib, problem
from tests import fisheye_support as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_tables_equal(p, g):
    for f in FS.TEXT_FIELDS:
        a, b = getattr(p, f), g["p_" + f]
        assert a.dtype == b.dtype and np.array_equal(a, b), f


def test_extract_gives_the_recorded_tables_mixed():
    g = FS.fixture("fisheye_mixed")
    graph, initial, branch = D.fisheye_mixed_graph(seed=int(g["seed"]))
    p, v0, keys = A.extract(graph, initial)
    assert_tables_equal(p, g)
    assert np.array_equal(v0, g["values0"])
    assert {n: int(g["branch_" + n]) for n in FS.BRANCHES} == branch
    assert p.calib_model.dtype == np.int32 and p.calib_model.tolist() == [1, 0, 1, 0]
    assert p.n_stereo == 0 and p.n_smart == 0 and p.n_sam == 0 and p.n_sam2 == 0
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    assert keys[:36] == [L(j) for j in range(36)] and keys[36:] == [X(i) for i in range(11)]


def test_extract_gives_the_recorded_tables_example():
    g = FS.fixture("fisheye_example")
    graph, initial = D.fisheye_example_graph()
    p, v0, _ = A.extract(graph, initial)
    assert_tables_equal(p, g)
    assert np.array_equal(v0, g["values0"])
    assert p.n_proj == 64 and p.n_prior == 2 and p.calib_model.tolist() == [1]
    assert p.calib.tolist() == [278.66, 278.48, 0.0, 319.75, 241.96]                      # examples/FisheyeExample.cpp:64-66
    assert p.calib_distortion.tolist() == [-0.013721808247486035, 0.020727425669427896, -0.012786476702685545, 0.0025242267320687625]
    assert type(graph.factors[2]) is A.GenericProjectionFactorCal3Fisheye and type(graph.factors[0]) is A.PriorFactorPose3


def two_factor_graph(K1, K2):
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    m = A.noiseModel.Unit.Create(2)
    graph.add(D.type_of_projection(A, K1)(np.array([300.0, 200.0]), m, X(0), L(0), K1))
    graph.add(D.type_of_projection(A, K2)(np.array([310.0, 210.0]), m, X(0), L(0), K2))
    initial.insert(X(0), A.Pose3()); initial.insert(L(0), A.Point3(0.1, 0.2, 4.0))
    return A.extract(graph, initial)[0]


def test_a_cal3ds2_and_a_cal3fisheye_with_equal_numbers_get_two_rows():
    nums = (400.0, 410.0, 0.2, 300.0, 200.0, 0.05, -0.01, 0.001, -0.002)
    p = two_factor_graph(A.Cal3DS2(*nums), A.Cal3Fisheye(*nums))
    assert p.calib.size == 10 and np.array_equal(p.calib[:5], p.calib[5:]) and np.array_equal(p.calib_distortion[:4], p.calib_distortion[4:])
    assert p.proj_calib.tolist() == [0, 1] and p.calib_model.tolist() == [problem.CALIB_PINHOLE, problem.CALIB_FISHEYE]
    p = two_factor_graph(A.Cal3Fisheye(*nums), A.Cal3DS2(*nums))
    assert p.proj_calib.tolist() == [0, 1] and p.calib_model.tolist() == [1, 0]
    # equal objects of one class still share their row
    p = two_factor_graph(A.Cal3Fisheye(*nums), A.Cal3Fisheye(*nums))
    assert p.proj_calib.tolist() == [0, 0] and p.calib_model.tolist() == [1] and p.calib_distortion.tolist() == list(nums[5:])
    # a fisheye beside a plain Cal3_S2: the pinhole row's distortion row is zero
    p = two_factor_graph(A.Cal3_S2(*nums[:5]), A.Cal3Fisheye(*nums))
    assert p.calib_model.tolist() == [0, 1] and p.calib_distortion.tolist() == [0.0] * 4 + list(nums[5:])


def test_a_graph_without_fisheye_leaves_calib_model_empty():
    nums = (400.0, 410.0, 0.2, 300.0, 200.0, 0.05, -0.01, 0.001, -0.002)
    p = two_factor_graph(A.Cal3DS2(*nums), A.Cal3_S2(*nums[:5]))
    assert p.calib_model.size == 0 and p.calib_model.dtype == np.int32 and p.calib_distortion.size == 8
    graph, initial, _ = D.stereo_mixed_graph()
    q = A.extract(graph, initial)[0]
    assert q.calib_model.size == 0 and q.calib.size == 20
    assert problem.Problem(var_type=np.zeros(1, np.int32)).calib_model.size == 0


def test_calib_model_is_checked_against_the_calibration_table():
    nums = (400.0, 410.0, 0.2, 300.0, 200.0, 0.05, -0.01, 0.001, -0.002)
    p = two_factor_graph(A.Cal3DS2(*nums), A.Cal3Fisheye(*nums))
    p.calib_model = np.array([1], np.int32)
    try:
        p.to_ctypes()
    except ValueError as e:
        assert "calib_model" in str(e)
    else:
        raise AssertionError("a calib_model of the wrong length was accepted")


def test_cal3fisheye_uncalibrate_is_the_model():
    K = A.Cal3Fisheye(300.0, 295.0, 0.8, 320.0, 240.0, -0.02, 0.01, -0.005, 0.001)
    assert K.v.shape == (9,) and np.array_equal(K.uncalibrate([0.0, 0.0]), [320.0, 240.0])
    for pn in ([0.3, -0.2], [1e-9, 0.0], [2.0, 3.0]):
        want, _ = FS.uncalibrate(K.v, pn)
        assert np.abs(K.uncalibrate(pn) - want).max() <= 1e-12 * np.abs(want).max()


def test_header_declares_the_setter_and_the_models():
    hdr = open(os.path.join(ROOT, "include", "gtsam_amd.h")).read()
    assert re.search(r"int\s+gtg_set_calibration_models\s*\(\s*gtg_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*model\s*,\s*int32_t\s+n_calib\s*\)\s*;", hdr)
    assert re.search(r"GTG_CALIB_PINHOLE\s*=\s*0\b", hdr) and re.search(r"GTG_CALIB_FISHEYE\s*=\s*1\b", hdr)
    assert (problem.CALIB_PINHOLE, problem.CALIB_FISHEYE) == (0, 1)
    assert "gtg_set_calibration_models" in lib.SYMBOLS
    # the struct did not grow: the model list is not a field of gtg_problem
    assert not any("model" in f[0] for f in problem.gtg_problem._fields_ + problem.gtg_planar_table._fields_)
