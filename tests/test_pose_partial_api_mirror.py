"""The Python mirror of the wrapped API for partial pose priors (gtsam_amd/api.py: Rot2, PoseTranslationPrior3D / 2D,
PoseRotationPrior3D / 2D): what extract() makes of a small graph and of the graphs behind the fixtures of
tests/golden/make_golden_pose_partial.py, the errors of extract() and Problem.add_pose_partial, and the C struct of a problem with
and without such factors.  (The library's host side of the feature -- gtg_upload_problem with the table, its refusals -- is checked on
the GPU, tests/test_gpu_pose_partial.py.)"""
import ctypes as C

import numpy as np
import pytest

from gtsam_amd import api as A
from gtsam_amd.problem import POSE_PARTIAL_ROTATION, POSE_PARTIAL_TRANSLATION, VAR_POSE2, VAR_POSE3, Problem, gtg_problem
from tests import pose_partial_support as PS

X = A.symbol_shorthand.X
nm = A.noiseModel


def small_graph():
    n3, n2, n1 = nm.Diagonal.Sigmas([0.1, 0.2, 0.3]), nm.Isotropic.Sigma(2, 0.5), nm.Isotropic.Sigma(1, 0.05)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    graph.add(A.PoseTranslationPrior3D(X(0), A.Point3(1.0, 2.0, 3.0), n3))
    graph.add(A.PoseRotationPrior3D(X(0), A.Rot3(Rz), n3))
    graph.add(A.PoseTranslationPrior3D(X(1), A.Pose3(A.Rot3(Rz), [4.0, 5.0, 6.0]), nm.Unit.Create(3)))      # the pose's translation
    graph.add(A.PoseRotationPrior3D(X(1), A.Pose3(A.Rot3(Rz), [4.0, 5.0, 6.0]), n3))                        # the pose's rotation
    graph.add(A.PoseTranslationPrior2D(X(2), A.Point2(7.0, 8.0), n2))
    graph.add(A.PoseRotationPrior2D(X(2), 0.5, n1))
    graph.add(A.PoseTranslationPrior2D(X(2), A.Pose2(9.0, 10.0, 0.25), n2))
    graph.add(A.PoseRotationPrior2D(X(2), A.Pose2(9.0, 10.0, 0.25), n1))
    graph.add(A.PoseRotationPrior2D(X(2), A.Rot2.fromCosSin(0.0, 2.0), n1))                                 # normalised like the reference
    initial.insert(X(0), A.Pose3()); initial.insert(X(1), A.Pose3(A.Rot3(), [0.5, 0.0, 0.0])); initial.insert(X(2), A.Pose2(1.0, 2.0, 0.1))
    return graph, initial


def test_rot2_holds_cos_and_sin():
    r = A.Rot2(0.5)
    assert (r.c(), r.s()) == (float(np.cos(0.5)), float(np.sin(0.5))) and r.theta() == pytest.approx(0.5, abs=1e-16)
    assert (A.Rot2().c(), A.Rot2().s()) == (1.0, 0.0)
    n = A.Rot2.fromCosSin(0.0, 2.0)
    assert (n.c(), n.s()) == (0.0, 1.0)
    k = A.Rot2.fromCosSin(1.0 + 1e-12, 0.0)              # within 1e-10 of a unit vector: kept as given (Rot2.cpp:56-64)
    assert k.c() == 1.0 + 1e-12
    p = A.Pose2(1.0, 2.0, 0.3)
    assert np.array_equal(p.translation(), [1.0, 2.0]) and p.rotation().c() == float(np.cos(0.3))


def test_extract_of_a_small_graph():
    graph, initial = small_graph()
    p, v0, keys = A.extract(graph, initial)
    assert p.var_type.tolist() == [VAR_POSE3, VAR_POSE3, VAR_POSE2] and p.n_prior == 0 and p.n_pose_partial == 9
    T, R = POSE_PARTIAL_TRANSLATION, POSE_PARTIAL_ROTATION
    assert p.pose_partial_kind.tolist() == [T, R, T, R, T, R, T, R, R]
    assert p.pose_partial_var.tolist() == [0, 0, 1, 1, 2, 2, 2, 2, 2]
    z = p.pose_partial_z.reshape(-1, 9)
    rz = [0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert z[0].tolist() == [1.0, 2.0, 3.0] + [0.0] * 6 and z[1].tolist() == rz
    assert z[2].tolist() == [4.0, 5.0, 6.0] + [0.0] * 6 and z[3].tolist() == rz
    assert z[4].tolist() == [7.0, 8.0] + [0.0] * 7 and z[6].tolist() == [9.0, 10.0] + [0.0] * 7
    assert z[5].tolist() == [float(np.cos(0.5)), float(np.sin(0.5))] + [0.0] * 7
    assert z[7].tolist() == [float(np.cos(0.25)), float(np.sin(0.25))] + [0.0] * 7
    assert z[8].tolist() == [0.0, 1.0] + [0.0] * 7
    assert p.noise_dim[p.pose_partial_noise].tolist() == [3, 3, 3, 3, 2, 1, 2, 1, 1]
    # noise tables are shared: one row per distinct model
    nz = p.pose_partial_noise
    assert nz[0] == nz[1] == nz[3] and nz[4] == nz[6] and nz[5] == nz[7] == nz[8] and p.noise_kind.size == 4
    f = graph.factors[0]
    assert f.keys_ == (X(0),) and np.array_equal(f.measured(), [1.0, 2.0, 3.0])


@pytest.mark.parametrize("name", PS.FIXTURES)
def test_extract_reproduces_the_fixture_tables(name):
    g = PS.fixture(name)
    graph, initial, _ = PS.scene(name)
    p, v0, _ = A.extract(graph, initial)
    assert np.array_equal(v0, g["values0"])
    fields = [k[2:] for k in g if k.startswith("p_")]
    assert "pose_partial_z" in fields and "noise_data" in fields
    for f in fields:
        a, b = getattr(p, f), g["p_" + f]
        assert a.dtype == b.dtype and np.array_equal(a, b), f
    assert p.n_prior == 0 and p.n_pose_partial == g["jac6"].shape[0]
    # the noise table is shared among the factor families: fewer rows than factors that name one
    assert p.noise_kind.size < p.n_pose_partial + p.n_between


def test_extract_errors():
    graph, initial = small_graph()
    for bad, dim in ((A.PoseTranslationPrior3D(X(0), A.Point3(), nm.Unit.Create(2)), 2), (A.PoseRotationPrior3D(X(0), A.Rot3(), nm.Unit.Create(6)), 6),
                     (A.PoseTranslationPrior2D(X(2), A.Point2(), nm.Unit.Create(3)), 3), (A.PoseRotationPrior2D(X(2), 0.0, nm.Unit.Create(3)), 3)):
        g2 = A.NonlinearFactorGraph(); g2.add(bad)
        with pytest.raises(ValueError, match="NoiseModel has wrong dimension"):
            A.extract(g2, initial)
    for bad, what in ((A.PoseTranslationPrior3D(X(2), A.Point3(), nm.Unit.Create(3)), "not a Pose3"), (A.PoseRotationPrior3D(X(2), A.Rot3(), nm.Unit.Create(3)), "not a Pose3"),
                      (A.PoseTranslationPrior2D(X(0), A.Point2(), nm.Unit.Create(2)), "not a Pose2"), (A.PoseRotationPrior2D(X(1), 0.0, nm.Unit.Create(1)), "not a Pose2")):
        g2 = A.NonlinearFactorGraph(); g2.add(bad)
        with pytest.raises(ValueError, match=what):
            A.extract(g2, initial)
    g2 = A.NonlinearFactorGraph(); g2.add(A.PoseTranslationPrior3D(X(7), A.Point3(), nm.Unit.Create(3)))
    with pytest.raises(KeyError, match="ValuesKeyDoesNotExist"):
        A.extract(g2, initial)


def test_add_pose_partial_argument_checks():
    p = Problem(var_type=np.array([VAR_POSE3, VAR_POSE2, 2], np.int32))
    n3 = p.add_noise(0, 3)
    with pytest.raises(ValueError, match="unknown partial pose prior kind"):
        p.add_pose_partial(2, 0, [0.0] * 3, n3)
    for var in (2, 3, -1):
        with pytest.raises(ValueError, match="POSE3 or POSE2"):
            p.add_pose_partial(POSE_PARTIAL_TRANSLATION, var, [0.0] * 3, n3)
    for kind, var, n in ((POSE_PARTIAL_TRANSLATION, 0, 2), (POSE_PARTIAL_ROTATION, 0, 3), (POSE_PARTIAL_TRANSLATION, 1, 3), (POSE_PARTIAL_ROTATION, 1, 1)):
        with pytest.raises(ValueError, match="measurement doubles"):
            p.add_pose_partial(kind, var, [0.0] * n, n3)
    assert p.n_pose_partial == 0
    p.add_pose_partial(POSE_PARTIAL_ROTATION, 1, [0.6, 0.8], p.add_noise(0, 1))
    p.add_pose_partial(POSE_PARTIAL_TRANSLATION, 0, [1.0, 2.0, 3.0], n3)
    assert p.n_pose_partial == 2 and p.pose_partial_z.tolist() == [0.6, 0.8] + [0.0] * 7 + [1.0, 2.0, 3.0] + [0.0] * 6
    assert p.pose_partial_kind.dtype == np.int32 and p.pose_partial_var.tolist() == [1, 0]


def test_to_ctypes_with_and_without_the_table():
    assert [f[0] for f in gtg_problem._fields_][-5:] == ["n_pose_partial", "pose_partial_kind", "pose_partial_var", "pose_partial_z", "pose_partial_noise"]
    g = PS.fixture("pose_partial_graph2d")
    cp = PS.problem_of(g).to_ctypes()
    assert cp.n_pose_partial == g["jac6"].shape[0]
    assert cp.pose_partial_kind[0] == g["p_pose_partial_kind"][0] and cp.pose_partial_z[1] == g["p_pose_partial_z"][1]
    assert cp.pose_partial_noise[cp.n_pose_partial - 1] == g["p_pose_partial_noise"][-1] and cp.pose_partial_var[3] == g["p_pose_partial_var"][3]
    # a problem without such factors: the count 0 and the four pointers NULL
    plain = PS.problem_of(PS.fixture("sam3d_mixed"))
    cp = plain.to_ctypes()
    assert plain.n_pose_partial == 0 and cp.n_pose_partial == 0
    for name in ("pose_partial_kind", "pose_partial_var", "pose_partial_z", "pose_partial_noise"):
        assert not getattr(cp, name), name
        assert C.cast(getattr(cp, name), C.c_void_p).value is None
    bad = PS.problem_of(g)
    bad.pose_partial_z = bad.pose_partial_z[:-1]
    with pytest.raises(ValueError, match="inconsistent partial pose prior tables"):
        bad.to_ctypes()
