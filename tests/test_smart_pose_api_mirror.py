"""The Python mirror of the wrapped API for pose-type smart factors (gtsam_amd/api.py: SmartProjectionPose3Factor): what extract()
makes of a small graph and of the graphs behind the fixtures, and Problem.add_smart(..., calib, sensor)."""
import numpy as np
import pytest

from gtsam_amd import api as A
from gtsam_amd import datasets as D
from gtsam_amd.problem import NOISE_UNIT, VAR_POSE3, Problem
from tests import smart_pose_support as S


def small_graph():
    X = A.symbol_shorthand.X
    K, K2 = A.Cal3_S2(500.0, 510.0, 0.25, 320.0, 240.0), A.Cal3_S2(400.0, 400.0, 0.0, 300.0, 200.0)
    n2 = A.noiseModel.Isotropic.Sigma(2, 2.0)
    sensor = A.Pose3(A.Rot3(), [0.1, 0.0, 0.0])
    prm = A.SmartProjectionParams(A.SmartProjectionParams.JACOBIAN_Q, A.SmartProjectionParams.ZERO_ON_DEGENERACY)
    prm.setLandmarkDistanceThreshold(50.0); prm.setDynamicOutlierRejectionThreshold(3.0); prm.setRankTolerance(0.5)
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    f0 = A.SmartProjectionPose3Factor(n2, K)
    f0.add([321.0, 239.0], X(0)); f0.add([300.0, 238.0], X(1)); f0.add([280.0, 237.0], X(2))
    f1 = A.SmartProjectionPose3Factor(n2, K, sensor, prm)
    f1.add(A.Point2(100.0, 50.0), X(2)); f1.add(A.Point2(90.0, 51.0), X(0))
    f2 = A.SmartProjectionPose3Factor(n2, K2, A.Pose3(A.Rot3(), [0.1, 0.0, 0.0]))        # an equal sensor, another object
    f2.add([10.0, 20.0], X(1)); f2.add([11.0, 21.0], X(2))
    f3 = A.SmartProjectionPose3Factor(n2, A.Cal3_S2(500.0, 510.0, 0.25, 320.0, 240.0))    # an equal K, another object
    f3.add([1.0, 2.0], X(0)); f3.add([3.0, 4.0], X(1))
    for f in (f0, f1, f2, f3):
        graph.add(f)
    graph.addPriorPose3(X(0), A.Pose3(), A.noiseModel.Isotropic.Sigma(6, 0.1))
    for i in range(3):
        initial.insert(X(i), A.Pose3(A.Rot3(), [0.5 * i, 0.0, 0.0]))
    return graph, initial


def test_extract_round_trips_to_the_tables():
    graph, initial = small_graph()
    p, v0, keys = A.extract(graph, initial)
    assert p.var_type.tolist() == [VAR_POSE3] * 3 and v0.size == 36
    assert p.n_smart == 4 and p.smart_ptr.tolist() == [0, 3, 5, 7, 9]
    assert p.smart_cam.tolist() == [0, 1, 2, 2, 0, 1, 2, 0, 1]
    assert p.smart_z.tolist() == [321.0, 239.0, 300.0, 238.0, 280.0, 237.0, 100.0, 50.0, 90.0, 51.0, 10.0, 20.0, 11.0, 21.0, 1.0, 2.0, 3.0, 4.0]
    # K and sensor are deduplicated by value
    assert p.calib.reshape(-1, 5).tolist() == [[500.0, 510.0, 0.25, 320.0, 240.0], [400.0, 400.0, 0.0, 300.0, 200.0]]
    assert p.smart_calib.tolist() == [0, 0, 1, 0]
    assert p.sensor.size == 12 and p.smart_sensor.tolist() == [-1, 0, 0, -1]
    assert len(set(p.smart_noise.tolist())) == 1 and p.noise_dim[p.smart_noise[0]] == 2
    prm = p.smart_params.reshape(-1, 8)
    assert prm[1].tolist() == [0.5, 50.0, 3.0, 1e-5, 1.0, 2.0, 0.0, 0.0]
    c = p.to_ctypes()
    assert c.n_smart == 4 and c.n_calib == 2 and c.n_sensor == 1 and bool(c.smart_calib) and bool(c.smart_sensor) and c.n_proj == 0


def test_defaults_equal_smart_projection_params():
    """SmartProjectionParams() (slam/SmartFactorParams.h:58-66, geometry/triangulation.h:583-600): HESSIAN, IGNORE_DEGENERACY,
    rankTolerance 1, no distance / outlier threshold, retriangulationThreshold 1e-5, no EPI."""
    graph, initial = small_graph()
    p, _, _ = A.extract(graph, initial)
    assert p.smart_params.reshape(-1, 8)[0].tolist() == [1.0, -1.0, -1.0, 1e-5, 0.0, 0.0, 0.0, 0.0]
    f = A.SmartProjectionPose3Factor(A.noiseModel.Unit.Create(2), A.Cal3_S2())
    assert f.sensor is None and f.params.degeneracyMode == A.SmartProjectionParams.IGNORE_DEGENERACY
    assert f.params.linearizationMode == A.SmartProjectionParams.HESSIAN and f.calibration() is f.K
    q = Problem(var_type=np.full(2, VAR_POSE3, np.int32))
    q.calib = np.array([1.0, 1.0, 0.0, 0.0, 0.0])
    q.add_smart([0, 1], [0.0, 0.0, 1.0, 1.0], q.add_noise(NOISE_UNIT, 2), calib=0)
    assert q.smart_params.tolist() == [1.0, -1.0, -1.0, 1e-5, 0.0, 0.0, 0.0, 0.0] and q.smart_calib.tolist() == [0] and q.smart_sensor.tolist() == [-1]


def test_add_smart_keeps_camera_type_problems_as_they_were():
    q = Problem(var_type=np.full(2, 1, np.int32))
    q.add_smart([0, 1], [0.0, 0.0, 1.0, 1.0], q.add_noise(NOISE_UNIT, 2))
    assert q.smart_calib.size == 0 and q.smart_sensor.size == 0
    c = q.to_ctypes()
    assert not bool(c.smart_calib) and not bool(c.smart_sensor)
    q.smart_calib = np.array([0, 0], np.int32)
    with pytest.raises(ValueError, match="inconsistent smart factor tables"):
        q.to_ctypes()


def test_unknown_noise_dimension_is_refused():
    graph, initial = small_graph()
    f = A.SmartProjectionPose3Factor(A.noiseModel.Isotropic.Sigma(3, 1.0), A.Cal3_S2())
    f.add([0.0, 0.0], A.symbol_shorthand.X(0))
    graph.add(f)
    with pytest.raises(ValueError, match="NoiseModel has wrong dimension"):
        A.extract(graph, initial)


@pytest.mark.parametrize("name", S.FIXTURES)
def test_fixture_problems_are_what_extract_returns(name):
    g = S.fixture(name)
    graph, initial, _ = D.smart_pose_scene(name, int(g["seed"]))
    p, v0, _ = A.extract(graph, initial)
    assert np.array_equal(v0, g["values0"])
    for k, want in g.items():
        if k.startswith("p_"):
            assert np.array_equal(getattr(p, k[2:]), want), k
