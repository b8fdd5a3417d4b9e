"""The Python mirror of the wrapped API for stereo graphs (gtsam_amd/api.py: StereoPoint2, Cal3_S2Stereo, GenericStereoFactor3D):
what extract() makes of a small graph, and of the graphs behind the fixtures.  NonlinearFactorGraph.error runs on the device:
that part is marked gpu."""
import numpy as np
import pytest

from gtsam_amd import api as A
from gtsam_amd import datasets as D
from tests import stereo_support as S


def small_graph():
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    K = A.Cal3_S2Stereo(500.0, 510.0, 0.25, 320.0, 240.0, 0.2)
    K2 = A.Cal3_S2Stereo(400.0, 400.0, 0.0, 300.0, 200.0, 0.5)
    Km = A.Cal3_S2(450.0, 450.0, 0.0, 320.0, 240.0)
    n3, n2 = A.noiseModel.Isotropic.Sigma(3, 2.0), A.noiseModel.Isotropic.Sigma(2, 1.0)
    huber = A.noiseModel.Robust.Create(A.noiseModel.mEstimator.Huber.Create(1.5), A.noiseModel.Diagonal.Sigmas([1.0, 2.0, 3.0]))
    sensor = A.Pose3(A.Rot3(), [0.1, 0.0, 0.0])
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    graph.add(A.GenericStereoFactor3D(A.StereoPoint2(330.0, 310.0, 250.0), n3, X(0), L(0), K))
    graph.add(A.GenericProjectionFactorCal3_S2([321.0, 239.0], n2, X(1), L(0), Km))
    graph.add(A.GenericStereoFactor3D(A.StereoPoint2(300.0, 280.0, 230.0), huber, X(1), L(1), K2, sensor))
    graph.add(A.GenericStereoFactor3D(A.StereoPoint2(310.0, 290.0, 235.0), n3, X(1), L(0), K))
    graph.addPriorPose3(X(0), A.Pose3(), A.noiseModel.Isotropic.Sigma(6, 0.1))
    initial.insert(X(0), A.Pose3()); initial.insert(X(1), A.Pose3(A.Rot3(), [0.5, 0.0, 0.0]))
    initial.insert(L(0), A.Point3(0.1, 0.1, 5.0)); initial.insert(L(1), A.Point3(-0.3, 0.2, 6.0))
    return graph, initial


def test_extract_of_a_small_stereo_graph():
    graph, initial = small_graph()
    p, v0, keys = A.extract(graph, initial)
    assert keys == sorted(keys) and [chr(k >> 56) for k in keys] == ["l", "l", "x", "x"]      # Values order: landmarks, then poses
    assert p.var_type.tolist() == [2, 2, 0, 0] and v0.size == 3 + 3 + 12 + 12
    assert (p.n_stereo, p.n_proj, p.n_prior) == (3, 1, 1)
    assert p.stereo_pose.tolist() == [2, 3, 3] and p.stereo_point.tolist() == [0, 1, 0]
    assert p.stereo_z.tolist() == [330.0, 310.0, 250.0, 300.0, 280.0, 230.0, 310.0, 290.0, 235.0]
    # one calibration table for both factor types, rows in first-occurrence order; the baseline beside it (0 for the Cal3_S2)
    assert p.calib.reshape(-1, 5).tolist() == [[500.0, 510.0, 0.25, 320.0, 240.0], [450.0, 450.0, 0.0, 320.0, 240.0], [400.0, 400.0, 0.0, 300.0, 200.0]]
    assert p.calib_baseline.tolist() == [0.2, 0.0, 0.5] and p.calib_distortion.size == 0
    assert p.stereo_calib.tolist() == [0, 2, 0] and p.proj_calib.tolist() == [1]
    assert p.stereo_sensor.tolist() == [-1, 0, -1] and p.sensor.size == 12 and p.proj_sensor.tolist() == [-1]
    # shared noise rows: the two Isotropic(3, 2.0) factors name one row of dimension 3; the Huber row keeps its estimator
    assert p.stereo_noise[0] == p.stereo_noise[2] != p.stereo_noise[1]
    assert p.noise_dim[p.stereo_noise].tolist() == [3, 3, 3]
    assert p.noise_robust[p.stereo_noise].tolist() == [0, 2, 0] and p.noise_robust_param[p.stereo_noise[1]] == 1.5
    c = p.to_ctypes()
    assert c.n_stereo == 3 and c.n_calib == 3 and bool(c.calib_baseline) and bool(c.stereo_sensor)


def test_extract_checks_the_noise_dimension_and_unknown_types():
    graph, initial = small_graph()
    K = A.Cal3_S2Stereo(500.0, 510.0, 0.0, 320.0, 240.0, 0.2)
    graph.add(A.GenericStereoFactor3D(A.StereoPoint2(1, 2, 3), A.noiseModel.Isotropic.Sigma(2, 1.0), A.symbol_shorthand.X(0), A.symbol_shorthand.L(0), K))
    with pytest.raises(ValueError, match="NoiseModel has wrong dimension"):
        A.extract(graph, initial)


def test_fixture_problems_are_what_extract_returns():
    g = S.fixture("stereo_mixed")
    graph, initial, behind = D.stereo_mixed_graph()
    p, v0, _ = A.extract(graph, initial)
    assert behind == int(g["behind"]) and np.array_equal(v0, g["values0"])
    for k, want in g.items():
        if k.startswith("p_"):
            assert np.array_equal(getattr(p, k[2:]), want), k
    gv = S.fixture("stereo_vo_large")
    pv, vv = S.vo_problem()
    assert np.array_equal(vv, gv["values0"])
    for k, want in gv.items():
        if k.startswith("p_"):
            assert np.array_equal(getattr(pv, k[2:]), want), k


@pytest.mark.gpu
def test_graph_error_equals_the_reference():
    g = S.fixture("stereo_mixed")
    graph, initial, _ = D.stereo_mixed_graph()
    assert abs(graph.error(initial) - float(g["error"])) <= 1e-9 * float(g["error"])
    graph, initial = S.vo_graph()
    gv = S.fixture("stereo_vo_large")
    assert abs(graph.error(initial) - float(gv["error"])) <= 1e-9 * float(gv["error"])
