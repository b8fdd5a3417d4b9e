"""The Python mirror of the wrapped API for bearing / range graphs (gtsam_amd/api.py: Unit3, BearingRange3D, BearingRangeFactor3D,
RangeFactor3D, BearingFactor3D): what extract() makes of a small graph and of the graphs behind the fixtures; and, in a child process
under tools/hipstub (a dry-run HIP runtime: host code only, no kernel runs), gtg_upload_problem with the sam table: sizes, the landmark
split, two shards, every refusal with its message, and a problem without the table."""
import os
import sys

import numpy as np
import pytest

from gtsam_amd import api as A
from gtsam_amd import datasets as D
from gtsam_amd.problem import SAM_BEARING, SAM_BEARING_RANGE, SAM_RANGE
from tests import sam_support as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402


def small_graph():
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    nm = A.noiseModel
    n3, n1, n2 = nm.Diagonal.Sigmas([0.01, 0.01, 0.1]), nm.Isotropic.Sigma(1, 0.1), nm.Isotropic.Sigma(2, 0.01)
    cauchy = nm.Robust.Create(nm.mEstimator.Cauchy.Create(0.5), nm.Isotropic.Sigma(1, 0.1))
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    graph.add(A.BearingRangeFactor3D(X(0), L(0), A.Unit3(0.0, 0.0, 2.0), 5.0, n3))
    graph.add(A.RangeFactor3D(X(1), L(0), 5.5, n1))
    graph.add(A.BearingFactor3D(X(1), L(1), A.Unit3(np.array([3.0, 0.0, 4.0])), n2))
    graph.add(A.RangeFactor3D(X(0), L(1), 6.5, cauchy))
    graph.add(A.BearingRangeFactor3D(X(1), L(1), A.Unit3(1.0, 0.0, 0.0), 6.0, n3))
    graph.addPriorPose3(X(0), A.Pose3(), nm.Isotropic.Sigma(6, 0.1))
    initial.insert(X(0), A.Pose3()); initial.insert(X(1), A.Pose3(A.Rot3(), [0.5, 0.0, 0.0]))
    initial.insert(L(0), A.Point3(0.1, 0.1, 5.0)); initial.insert(L(1), A.Point3(-0.3, 0.2, 6.0))
    return graph, initial


def test_unit3_normalises_and_bearing_range_holds_both():
    u = A.Unit3(3.0, 0.0, 4.0)
    assert np.array_equal(u.point3(), np.array([3.0, 0.0, 4.0]) / 5.0) and np.array_equal(A.Unit3(np.array([0.0, 2.0, 0.0])).unitVector(), [0.0, 1.0, 0.0])
    assert np.array_equal(A.Unit3().point3(), [1.0, 0.0, 0.0])                 # the default direction (Unit3.h)
    br = A.BearingRange3D(u, 2.5)
    assert br.bearing() is u and br.range() == 2.5
    f = A.BearingRangeFactor3D(1, 2, u, 2.5, A.noiseModel.Unit.Create(3))
    assert f.measured().range() == 2.5 and f.measured().bearing() is u and f.keys_ == (1, 2)
    assert A.RangeFactor3D(1, 2, 4.0, A.noiseModel.Unit.Create(1)).measured() == 4.0
    assert A.BearingFactor3D(1, 2, u, A.noiseModel.Unit.Create(2)).measured() is u


def test_extract_of_a_small_bearing_range_graph():
    graph, initial = small_graph()
    p, v0, keys = A.extract(graph, initial)
    assert p.var_type.tolist() == [2, 2, 0, 0]                                   # Values order: landmarks, then poses
    assert (p.n_sam, p.n_proj, p.n_stereo, p.n_prior) == (5, 0, 0, 1)
    assert p.sam_kind.tolist() == [SAM_BEARING_RANGE, SAM_RANGE, SAM_BEARING, SAM_RANGE, SAM_BEARING_RANGE]
    assert p.sam_pose.tolist() == [2, 3, 3, 2, 3] and p.sam_point.tolist() == [0, 0, 1, 1, 1]
    # the Unit3's three doubles, then the range; what a kind does not use is 0
    assert p.sam_z.reshape(-1, 4).tolist() == [[0.0, 0.0, 1.0, 5.0], [0.0, 0.0, 0.0, 5.5], [0.6, 0.0, 0.8, 0.0], [0.0, 0.0, 0.0, 6.5], [1.0, 0.0, 0.0, 6.0]]
    assert p.noise_dim[p.sam_noise].tolist() == [3, 1, 2, 1, 3]
    assert p.sam_noise[0] == p.sam_noise[4] and p.sam_noise[1] != p.sam_noise[3]
    assert p.noise_robust[p.sam_noise].tolist() == [0, 0, 0, 3, 0] and p.noise_robust_param[p.sam_noise[3]] == 0.5
    assert p.calib.size == 0 and p.sensor.size == 0                              # no calibration, no sensor: none is read
    c = p.to_ctypes()
    assert c.n_sam == 5 and c.n_calib == 0 and bool(c.sam_kind) and bool(c.sam_z) and not bool(c.calib)


def test_extract_checks_the_noise_dimension_by_kind():
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    for f in (A.BearingRangeFactor3D(X(0), L(0), A.Unit3(0, 0, 1), 5.0, A.noiseModel.Isotropic.Sigma(2, 0.1)),
              A.RangeFactor3D(X(0), L(0), 5.0, A.noiseModel.Isotropic.Sigma(3, 0.1)),
              A.BearingFactor3D(X(0), L(0), A.Unit3(0, 0, 1), A.noiseModel.Isotropic.Sigma(1, 0.1))):
        graph, initial = small_graph()
        graph.add(f)
        with pytest.raises(ValueError, match="NoiseModel has wrong dimension"):
            A.extract(graph, initial)


def test_add_sam_takes_what_its_kind_measures():
    p = SS.problem_of(SS.fixture("sam3d_mixed"))
    n = p.n_sam
    p.add_sam(SAM_RANGE, int(p.sam_pose[0]), int(p.sam_point[0]), int(p.sam_noise[p.sam_kind == 1][0]), range_=3.0)
    assert p.n_sam == n + 1 and p.sam_z[-4:].tolist() == [0.0, 0.0, 0.0, 3.0]
    with pytest.raises(ValueError):
        p.add_sam(SAM_BEARING, 0, 1, 0, range_=3.0)
    with pytest.raises(ValueError):
        p.add_sam(SAM_BEARING_RANGE, 0, 1, 0, bearing=[0, 0, 1])
    with pytest.raises(ValueError):
        p.add_sam(7, 0, 1, 0, bearing=[0, 0, 1], range_=1.0)


def test_fixture_problems_are_what_extract_returns():
    """Every table but the bearings bit for bit; a bearing to two ulps (the generator stores what the reference's Unit3 constructor
    makes of the mirror's unit vector, which may round a component the other way)."""
    cases = (("sam3d_mixed", D.sam3d_mixed_graph()[:2]), ("sam3d_slam", D.landmark_slam3d_graph()))
    for name, (graph, initial) in cases:
        g = SS.fixture(name)
        p, v0, _ = A.extract(graph, initial)
        assert np.array_equal(v0, g["values0"])
        for k, want in g.items():
            if k == "p_sam_z":
                assert np.abs(p.sam_z - want).max() <= 2 * np.finfo(float).eps, name
                assert np.array_equal(p.sam_z.reshape(-1, 4)[:, 3], want.reshape(-1, 4)[:, 3])
            elif k.startswith("p_"):
                assert np.array_equal(getattr(p, k[2:]), want), (name, k)
    g = SS.fixture("sam3d_mixed")
    _, _, branch = D.sam3d_mixed_graph()
    assert {n: int(g["branch_" + n]) for n in branch} == branch
    s = SS.problem_of(SS.fixture("sam3d_slam"))
    assert s.calib.size == 0 and s.n_proj == 0 and s.n_stereo == 0 and s.n_sam == 3000 and int((s.var_type == 0).sum()) == 40 and int((s.var_type == 2).sum()) == 300


CHILD = r"""
import ctypes, json
import numpy as np
from gtsam_amd import lib as L
from tests import sam_support as SS
g = SS.fixture("sam3d_mixed")
out = {}

def info(p, shard=0, n_shards=1):
    def lockstep(ptr, n, stream):
        buf = np.frombuffer((ctypes.c_double * n).from_address(ptr), dtype=np.float64); buf *= n_shards
    d = L.DeviceGraph(p, shard=shard, n_shards=n_shards, allreduce=lockstep if n_shards > 1 else None)
    r = {"values": int(d.val_size), "tangent": int(d.dim_size), "reduced": int(d.reduced_dim), "hash": int(d.structure_hash())}
    d.close()
    return r

def error_of(**override):
    try:
        info(SS.problem_of(g, **override))
    except L.GtsamAmdError as e:
        return str(e)
    return "no error"

p = SS.problem_of(g)
out["counts"] = [p.n_vars, p.n_proj, p.n_stereo, p.n_sam, int((p.var_type == 2).sum())]
out["one"] = info(p)
out["two"] = [info(p, s, 2) for s in range(2)]
slam = SS.problem_of(SS.fixture("sam3d_slam"))
out["slam"] = info(slam); out["slam_counts"] = [int((slam.var_type == 0).sum()), int((slam.var_type == 2).sum()), int(slam.calib.size)]
none = dict(sam_kind=[], sam_pose=[], sam_point=[], sam_z=[], sam_noise=[])
old = SS.problem_of(g, **none)
c = old.to_ctypes()
out["old_fields"] = [int(c.n_sam), bool(c.sam_kind), bool(c.sam_z)]
out["old"] = info(old)
stereo = SS.S.problem_of(SS.S.fixture("stereo_mixed"))
out["stereo_mixed"] = info(stereo)
def with_first(name, value):
    a = np.array(g["p_" + name]); a[0] = value; return {name: a}
first = {k: int(np.flatnonzero(p.sam_kind == k)[0]) for k in (0, 1, 2)}
def with_at(name, i, value):
    a = np.array(g["p_" + name]); a[i] = value; return {name: a}
nz_of = {d: int(np.flatnonzero(p.noise_dim == d)[0]) for d in (1, 2, 3)}
pose0 = int(np.flatnonzero(p.var_type == 0)[0]); pt0 = int(np.flatnonzero(p.var_type == 2)[0])
out["errors"] = {
    "keys_swapped": error_of(sam_pose=np.array(g["p_sam_point"]), sam_point=np.array(g["p_sam_pose"])),
    "point_is_pose": error_of(**with_at("sam_point", first[1], pose0)),
    "pose_is_point": error_of(**with_at("sam_pose", first[2], pt0)),
    "key_out_of_range": error_of(**with_first("sam_pose", p.n_vars)),
    "noise_dim_br": error_of(**with_at("sam_noise", first[0], nz_of[2])),
    "noise_dim_range": error_of(**with_at("sam_noise", first[1], nz_of[3])),
    "noise_dim_bearing": error_of(**with_at("sam_noise", first[2], nz_of[1])),
    "noise_index": error_of(**with_first("sam_noise", p.noise_kind.size)),
    "kind_high": error_of(**with_first("sam_kind", 3)),
    "kind_negative": error_of(**with_first("sam_kind", -1)),
}
# beside pose-type smart factors (three-row records are refused there)
q = SS.problem_of(g, stereo_pose=[], stereo_point=[], stereo_z=[], stereo_noise=[], stereo_calib=[], stereo_sensor=[], calib_baseline=[])
n2 = q.add_noise(1, 2, [1.0])
poses = np.flatnonzero(q.var_type == 0)[:2]
q.add_smart(poses, [320.0, 240.0, 321.0, 239.0], n2, calib=0)
try:
    info(q); out["errors"]["smart_pose"] = "no error"
except L.GtsamAmdError as e:
    out["errors"]["smart_pose"] = str(e)
cp = SS.problem_of(g).to_ctypes()
cp.sam_z = ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
lib = L.load(); h = ctypes.c_void_p()
assert lib.gtg_create(ctypes.byref(h), 0) == 0
rc = lib.gtg_upload_problem(h, ctypes.byref(cp), 0, 1)
out["null_table"] = [int(rc), lib.gtg_last_error().decode()]
lib.gtg_destroy(h)
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def result():
    if not os.path.exists(os.path.join(ROOT, "gtsam_amd", "lib", "libgtsam_amd.so")):
        pytest.skip("libgtsam_amd.so not built")
    return HP.run_snippet(CHILD)


def test_upload_sizes_and_landmark_split(result):
    n_vars, n_proj, n_stereo, n_sam, n_points = result["counts"]
    n_poses = n_vars - n_points
    assert (n_poses, n_points, n_proj, n_stereo, n_sam) == (7, 43, 40, 90, 301)
    one = result["one"]
    assert one["values"] == 12 * n_poses + 3 * n_points and one["tangent"] == 6 * n_poses + 3 * n_points
    # every POINT3 is a landmark -- also those touched by bearing / range factors alone: the reduced system is the poses
    assert one["reduced"] == 6 * n_poses
    poses, points, calib = result["slam_counts"]
    assert (poses, points, calib) == (40, 300, 0) and result["slam"]["reduced"] == 6 * poses and result["slam"]["tangent"] == 6 * poses + 3 * points


def test_two_shards_share_the_layout(result):
    one, two = result["one"], result["two"]
    assert two[0]["hash"] == two[1]["hash"] == one["hash"] != 0
    assert [t["reduced"] for t in two] == [one["reduced"]] * 2 and [t["tangent"] for t in two] == [one["tangent"]] * 2


def test_a_problem_without_the_table_uploads_as_before(result):
    assert result["old_fields"] == [0, False, False]
    assert result["old"]["reduced"] == result["one"]["reduced"] and result["old"]["values"] == result["one"]["values"]
    assert result["stereo_mixed"]["reduced"] == 36 and result["stereo_mixed"]["hash"] != 0


def test_refusals_and_their_text(result):
    e = result["errors"]
    assert "keys must be (POSE3, POINT3)" in e["keys_swapped"]
    assert "RangeFactor keys must be (POSE3, POINT3)" in e["point_is_pose"], e["point_is_pose"]
    assert "BearingFactor keys must be (POSE3, POINT3)" in e["pose_is_point"], e["pose_is_point"]
    assert "factor refers to a key that is not in Values" in e["key_out_of_range"]
    assert "BearingRangeFactor: NoiseModel has wrong dimension" in e["noise_dim_br"], e["noise_dim_br"]
    assert "RangeFactor: NoiseModel has wrong dimension" in e["noise_dim_range"] and "Bearing" not in e["noise_dim_range"]
    assert "BearingFactor: NoiseModel has wrong dimension" in e["noise_dim_bearing"], e["noise_dim_bearing"]
    assert "NoiseModel has wrong dimension" in e["noise_index"]
    for k in ("kind_high", "kind_negative"):
        assert "unknown sam_kind" in e[k], (k, e[k])
    assert "pose-type smart factors together with bearing / range factors" in e["smart_pose"], e["smart_pose"]
    assert result["null_table"][0] == -1 and "bearing / range factor tables missing" in result["null_table"][1]      # GTG_ERR_USAGE
