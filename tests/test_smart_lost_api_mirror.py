"""TriangulationParameters::useLOST in the API mirror (gtsam_amd/api.py, gtsam_amd/problem.py) on the CPU: SmartProjectionParams.useLOST /
setUseLOST / triangulationNoiseModel, the sigma triangulatePoint3 hands to triangulateLOST (geometry/triangulation.h:503: the mean of the
model's sigmas, 1e-4 without a model), slot 7 of smart_params for all three smart factor kinds, and the defaults: a graph that does not
use LOST gives the arrays it gave before.  The fixtures' tables are what the extractor makes of the scenes in gtsam_amd/datasets.py."""
import numpy as np
import pytest

from gtsam_amd import api as A
from gtsam_amd import datasets as D
from gtsam_amd.problem import Problem
from tests import smart_lost_support as S

X = A.symbol_shorthand.X
KINDS = ("camera", "pose", "rig")


def graph_of(kind, params):
    """two views of one track through a smart factor of the given kind"""
    model = A.noiseModel.Isotropic.Sigma(2, 1.0)
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    a, b = A.Pose3(), A.Pose3(A.Rot3(), [1.0, 0.0, 0.0])
    if kind == "camera":
        f = A.SmartProjectionFactorPinholeCameraCal3Bundler(model, params)
        initial.insert(X(0), A.PinholeCameraCal3Bundler(a, A.Cal3Bundler(500, 0, 0, 320, 240)))
        initial.insert(X(1), A.PinholeCameraCal3Bundler(b, A.Cal3Bundler(500, 0, 0, 320, 240)))
    else:
        initial.insert(X(0), a); initial.insert(X(1), b)
        if kind == "pose":
            f = A.SmartProjectionPose3Factor(model, A.Cal3_S2(500, 500, 0, 320, 240), None, params)
        else:
            f = A.SmartProjectionRigFactorPinholePoseCal3_S2(model, A.CameraSetPinholePoseCal3_S2([A.PinholePoseCal3_S2(A.Pose3(), A.Cal3_S2(500, 500, 0, 320, 240))]), params)
    f.add([320.0, 240.0], X(0)); f.add([220.0, 240.0], X(1))
    graph.add(f)
    return graph, initial


def params(**fields):
    prm = A.SmartProjectionParams(degeneracyMode=A.SmartProjectionParams.ZERO_ON_DEGENERACY)
    for k, v in fields.items():
        setattr(prm, k, v)
    return prm


def test_params_defaults_and_setter():
    prm = A.SmartProjectionParams()
    assert prm.useLOST is False and prm.triangulationNoiseModel is None and prm.enableEPI is False
    prm.setUseLOST(1)
    assert prm.useLOST is True and prm.lostSigma() == 1e-4


@pytest.mark.parametrize("kind", KINDS)
def test_slot_seven_is_written_for_every_kind(kind):
    nm = A.noiseModel
    p, _, _ = A.extract(*graph_of(kind, params()))
    assert p.smart_params.size == 8 and p.smart_params[7] == 0.0                      # the default: DLT, as before
    before = [1.0, -1.0, -1.0, 1e-5, 1.0, 0.0, 0.0, 0.0]                                 # the row this graph gave before LOST existed
    assert np.array_equal(p.smart_params, before)
    for model, sigma in ((None, 1e-4), (nm.Isotropic.Sigma(2, 0.25), 0.25), (nm.Diagonal.Sigmas([0.3, 0.5]), 0.4), (nm.Unit.Create(2), 1.0),
                         (nm.Gaussian.SqrtInformation(np.array([[2.0, 0.0], [0.0, 4.0]]), smart=False), 0.375)):
        q, _, _ = A.extract(*graph_of(kind, params(useLOST=True, triangulationNoiseModel=model)))
        assert q.smart_params[7] == pytest.approx(sigma, rel=1e-15), (kind, sigma)
        assert np.array_equal(q.smart_params[:7], before[:7])
    # a model without LOST changes nothing (the DLT does not read it)
    q, _, _ = A.extract(*graph_of(kind, params(triangulationNoiseModel=nm.Isotropic.Sigma(2, 0.25))))
    assert np.array_equal(q.smart_params, before)
    # Robust does not override sigmas(): the reference throws there
    robust = nm.Robust.Create(nm.mEstimator.Huber.Create(1.0), nm.Unit.Create(2))
    with pytest.raises(RuntimeError, match="sigmas"):
        A.extract(*graph_of(kind, params(useLOST=True, triangulationNoiseModel=robust)))


def test_add_smart_writes_the_slot_and_keeps_its_defaults():
    p = Problem(var_type=np.zeros(2, np.int32))
    ni = p.add_noise(0, 2, [])
    p.add_smart([0, 1], [1.0, 2.0, 3.0, 4.0], ni, calib=0)
    p.add_smart([0, 1], [1.0, 2.0, 3.0, 4.0], ni, calib=0, use_lost=True)
    p.add_smart([0, 1], [1.0, 2.0, 3.0, 4.0], ni, calib=0, use_lost=True, lost_sigma=0.5)
    p.add_smart([0, 1], [1.0, 2.0, 3.0, 4.0], ni, calib=0, lost_sigma=0.5)               # a sigma without use_lost: DLT
    assert np.array_equal(p.smart_params.reshape(-1, 8)[:, 7], [0.0, 1e-4, 0.5, 0.0])
    assert np.array_equal(p.smart_params.reshape(-1, 8)[0], [1.0, -1.0, -1.0, 1e-5, 0.0, 0.0, 0.0, 0.0])
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="lost_sigma"):
            p.add_smart([0, 1], [1.0, 2.0, 3.0, 4.0], ni, calib=0, use_lost=True, lost_sigma=bad)
    assert p.n_smart == 4


@pytest.mark.parametrize("name", S.FIXTURES)
def test_fixture_tables_are_the_extraction_of_the_dataset_scene(name):
    g, p, v0 = S.load(name)
    scene = "smart_lost_cam" if name.startswith("smart_lost_cam") else name
    variant = name[len(scene) + 1:] or None
    graph, initial, _ = D.smart_lost_scene(scene, int(g["seed"]), variant)
    q, w0, _ = A.extract(graph, initial)
    assert np.array_equal(w0, v0)
    for f in S.TEXT_FIELDS:
        assert np.array_equal(np.asarray(getattr(q, f)), np.asarray(getattr(p, f))), f
    prm = p.smart_params.reshape(-1, 8)
    assert np.all(prm[:, 6] == (1.0 if variant == "epi" else 0.0))
    assert set(prm[:, 7]) == {"smart_lost_pose": {0.0, 1e-4}, "smart_lost_rig": {0.4}}.get(name, {1e-4})
