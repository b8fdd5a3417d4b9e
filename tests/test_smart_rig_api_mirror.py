"""The API mirror of SmartProjectionRigFactor<PinholePose<Cal3_S2>> (gtsam_amd/api.py) on the CPU: constructor and add() errors as in the
reference (slam/SmartProjectionRigFactor.h:100-107, :148-159), the unique / non-unique key lists (:120-134), and the tables the
extractor makes of a graph -- one calib and one sensor row per (rig, camera), shared by every factor of the rig; an identity extrinsic
is no row (-1)."""
import numpy as np
import pytest

from gtsam_amd import api as A
from gtsam_amd import datasets as D
from gtsam_amd.problem import SMART_RIG, Problem

X = A.symbol_shorthand.X


def params():
    return A.SmartProjectionParams(degeneracyMode=A.SmartProjectionParams.ZERO_ON_DEGENERACY)


def rig2():
    cams = A.CameraSetPinholePoseCal3_S2()
    cams.push_back(A.PinholePoseCal3_S2(A.Pose3(), A.Cal3_S2(500, 510, 0.3, 320, 240)))
    cams.push_back(A.PinholePoseCal3_S2(A.Pose3(A.Rot3(), [0.5, 0.0, 0.0]), A.Cal3_S2(480, 490, 0.0, 300, 250)))
    return cams


def test_constructor_refuses_what_the_reference_refuses():
    model = A.noiseModel.Isotropic.Sigma(2, 1.0)
    for mode in (A.SmartProjectionParams.IGNORE_DEGENERACY, A.SmartProjectionParams.HANDLE_INFINITY):
        with pytest.raises(RuntimeError, match="degeneracyMode must be set to ZERO_ON_DEGENERACY"):
            A.SmartProjectionRigFactorPinholePoseCal3_S2(model, rig2(), A.SmartProjectionParams(degeneracyMode=mode))
    with pytest.raises(RuntimeError, match="degeneracyMode must be set to ZERO_ON_DEGENERACY"):
        A.SmartProjectionRigFactorPinholePoseCal3_S2(model, rig2())          # the default parameters are IGNORE_DEGENERACY
    for lin in (A.SmartProjectionParams.IMPLICIT_SCHUR, A.SmartProjectionParams.JACOBIAN_Q, A.SmartProjectionParams.JACOBIAN_SVD):
        with pytest.raises(RuntimeError, match="linearizationMode must be set to HESSIAN"):
            A.SmartProjectionRigFactorPinholePoseCal3_S2(model, rig2(), A.SmartProjectionParams(linearizationMode=lin, degeneracyMode=1))


def test_add_keeps_unique_keys_in_first_appearance_order_and_checks_the_vector_form():
    model = A.noiseModel.Isotropic.Sigma(2, 1.0)
    f = A.SmartProjectionRigFactorPinholePoseCal3_S2(model, rig2(), params())
    f.add([1.0, 2.0], X(3), 1)
    f.add([3.0, 4.0], X(1))                     # cameraId defaults to 0
    f.add([5.0, 6.0], X(3), 0)
    f.add([[7.0, 8.0], [9.0, 10.0]], [X(1), X(0)], [1, 1])
    assert f.nonUniqueKeys() == [X(3), X(1), X(3), X(1), X(0)] and f.keys() == [X(3), X(1), X(0)]
    assert f.cameraIds() == [1, 0, 0, 1, 1] and f.cameraRig().size() == 2
    with pytest.raises(RuntimeError, match="trying to add inconsistent inputs"):
        f.add([[1.0, 2.0]], [X(0), X(1)], [0, 0])
    with pytest.raises(RuntimeError, match="trying to add inconsistent inputs"):
        f.add([[1.0, 2.0], [1.0, 2.0]], [X(0), X(1)], [0])
    with pytest.raises(RuntimeError, match="camera rig includes multiple camera but add did not input cameraIds"):
        f.add([[1.0, 2.0], [1.0, 2.0]], [X(0), X(1)])
    one = A.CameraSetPinholePoseCal3_S2([A.PinholePoseCal3_S2()])
    g = A.SmartProjectionRigFactorPinholePoseCal3_S2(model, one, params())
    g.add([[1.0, 2.0], [1.0, 2.0]], [X(0), X(1)])          # a single camera needs no ids
    assert g.cameraIds() == [0, 0]
    assert len(f.zs) == 5                       # the refused calls added nothing


def test_extractor_shares_rows_per_rig_camera():
    model = A.noiseModel.Isotropic.Sigma(2, 1.5)
    rig, other = rig2(), rig2()
    graph, values = A.NonlinearFactorGraph(), A.Values()
    for i in range(3):
        values.insert(X(i), A.Pose3(A.Rot3(), [float(i), 0.0, 0.0]))
    f1 = A.SmartProjectionRigFactorPinholePoseCal3_S2(model, rig, params())
    for i, c in ((0, 0), (0, 1), (2, 1), (1, 0)):
        f1.add([10.0 * i, c], X(i), c)
    f2 = A.SmartProjectionRigFactorPinholePoseCal3_S2(model, rig, params())
    f2.add([1.0, 1.0], X(1), 1); f2.add([2.0, 2.0], X(2), 1)
    f3 = A.SmartProjectionRigFactorPinholePoseCal3_S2(model, other, params())      # another rig object: rows of its own
    f3.add([3.0, 3.0], X(0), 1); f3.add([4.0, 4.0], X(1), 0)
    for f in (f1, f2, f3):
        graph.add(f)
    p, v0, keys = A.extract(graph, values)
    assert p.n_smart == 3 and list(p.smart_ptr) == [0, 4, 6, 8] and list(p.smart_calib) == [SMART_RIG] * 3 and list(p.smart_sensor) == [-1] * 3
    assert list(p.smart_cam) == [0, 0, 2, 1, 1, 2, 0, 1]                        # the non-unique keys, in measurement order
    assert p.calib.size == 10                                                   # two distinct K, shared by value
    assert list(p.smart_meas_calib) == [0, 1, 1, 0, 1, 1, 1, 0]
    assert p.sensor.size == 24                                                  # camera 1 of each rig object; the identity camera has no row
    assert list(p.smart_meas_sensor) == [-1, 0, 0, -1, 0, 0, 1, -1]
    assert np.array_equal(p.sensor[:12], rig[1].pose().packed()) and np.array_equal(p.sensor[12:], other[1].pose().packed())
    prm = p.smart_params.reshape(-1, 8)
    assert np.all(prm[:, 4] == 1.0) and np.all(prm[:, 5] == 0.0)
    c = p.to_ctypes()
    assert bool(c.smart_meas_calib) and bool(c.smart_meas_sensor)
    f4 = A.SmartProjectionRigFactorPinholePoseCal3_S2(model, rig, params())
    f4.add([1.0, 1.0], X(0), 2)
    graph.add(f4)
    with pytest.raises(IndexError, match="camera id 2 outside the rig"):
        A.extract(graph, values)


def test_rig_and_pose_type_factors_share_the_tables():
    """the fixtures' scene: pose-type factors beside rig factors keep their per-factor rows; the per-measurement entries at their
    measurements are -1"""
    graph, initial, info = D.smart_rig_scene("smart_rig_mixed", 0)
    p, _, _ = A.extract(graph, initial)
    rig = p.smart_calib == SMART_RIG
    assert rig.any() and (~rig).any() and np.all(p.smart_calib[~rig] >= 0)
    assert p.smart_meas_calib.size == p.smart_cam.size == p.smart_meas_sensor.size
    per_meas = np.repeat(rig, np.diff(p.smart_ptr))
    assert np.all(p.smart_meas_calib[~per_meas] == -1) and np.all(p.smart_meas_calib[per_meas] >= 0)
    assert np.unique(np.stack([p.smart_meas_calib[per_meas], p.smart_meas_sensor[per_meas]]), axis=1).shape[1] == 3     # three cameras
    assert info["kind"].count("pose") == int((~rig).sum())
    graph, initial, _ = D.smart_rig_scene("smart_rig_pair", 1)
    p, _, _ = A.extract(graph, initial)
    assert set(p.smart_meas_sensor.tolist()) == {-1, 0} and p.calib.reshape(-1, 5)[0, 2] != 0.0       # camera 0: no extrinsic, skew


def test_add_smart_checks_the_rig_arguments():
    p = Problem(var_type=np.zeros(3, np.int32))
    n = p.add_noise(1, 2, [1.0])
    with pytest.raises(ValueError, match="meas_sensor without meas_calib"):
        p.add_smart([0, 1], [1.0, 2.0, 3.0, 4.0], n, meas_sensor=[-1, -1])
    with pytest.raises(ValueError, match="no calib / sensor of its own"):
        p.add_smart([0, 1], [1.0, 2.0, 3.0, 4.0], n, calib=0, meas_calib=[0, 0])
    with pytest.raises(ValueError, match="one calib and one sensor entry per measurement"):
        p.add_smart([0, 1], [1.0, 2.0, 3.0, 4.0], n, degeneracy_mode=1, meas_calib=[0])
