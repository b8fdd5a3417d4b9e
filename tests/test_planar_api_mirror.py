"""The Python mirror of the wrapped API for planar landmark SLAM (gtsam_amd/api.py: Point2 values, BearingRange2D, BearingRangeFactor2D,
RangeFactor2D, BearingFactor2D): what extract() makes of a small graph and of the graphs behind the fixtures; and, in a child process
under tools/hipstub (a dry-run HIP runtime: host code only, no kernel runs), gtg_upload_problem with the sam2 table: sizes, the symbolic
analysis (reduced dimension 3 x poses: a landmark seen by planar factors alone is eliminated), every refusal with its message, and the
refusal of gtg_try_lambda_pcg at the call."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from gtsam_amd import api as A
from gtsam_amd import datasets as D
from gtsam_amd.problem import SAM_BEARING, SAM_BEARING_RANGE, SAM_RANGE, VAR_POINT2, VAR_POSE2
from tests import planar_support as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402


def test_bearing_range_2d_holds_both_and_the_factors_their_measurements():
    r = A.Rot2.fromAngle(0.5)
    br = A.BearingRange2D(r, 2.5)
    assert br.bearing() is r and br.range() == 2.5
    f = A.BearingRangeFactor2D(1, 2, r, 2.5, A.noiseModel.Unit.Create(2))
    assert f.measured().range() == 2.5 and f.measured().bearing() is r and f.keys_ == (1, 2)
    assert A.RangeFactor2D(1, 2, 4.0, A.noiseModel.Unit.Create(1)).measured() == 4.0
    assert A.BearingFactor2D(1, 2, r, A.noiseModel.Unit.Create(1)).measured() is r


def test_extract_of_the_planar_slam_example():
    graph, initial = D.planar_slam_example()
    p, v0, keys = A.extract(graph, initial)
    assert p.var_type.tolist() == [VAR_POINT2, VAR_POINT2, VAR_POSE2, VAR_POSE2, VAR_POSE2]      # Values order: landmarks, then poses
    # a Point2 is padded to the landmark slot: (x, y, 0)
    assert v0.tolist() == [1.8, 2.1, 0.0, 4.1, 1.8, 0.0, 0.5, 0.0, 0.2, 2.3, 0.1, -0.2, 4.1, 0.1, 0.1]
    assert p.val_offsets().tolist() == p.dim_offsets().tolist() == [0, 3, 6, 9, 12, 15]
    assert (p.n_sam2, p.n_sam, p.n_between, p.n_prior) == (3, 0, 2, 1)
    assert p.sam2_kind.tolist() == [SAM_BEARING_RANGE] * 3 and p.sam2_pose.tolist() == [2, 3, 4] and p.sam2_point.tolist() == [0, 0, 1]
    z = p.sam2_z.reshape(-1, 3)
    assert np.array_equal(z[:, 0], np.cos([np.pi / 4, np.pi / 2, np.pi / 2])) and np.array_equal(z[:, 1], np.sin([np.pi / 4, np.pi / 2, np.pi / 2]))
    assert z[:, 2].tolist() == [np.sqrt(8.0), 2.0, 2.0]
    assert p.noise_dim[p.sam2_noise].tolist() == [2, 2, 2] and len(set(p.sam2_noise.tolist())) == 1
    c = p.to_ctypes()
    assert c.planar.n_sam2 == 3 and bool(c.planar.sam2_kind) and bool(c.planar.sam2_z) and c.n_sam == 0 and not bool(c.sam_z)
    # the table is the last member of the C struct, behind gtg_problem's own fields (the partial pose priors last among them)
    from gtsam_amd.problem import gtg_planar_table, gtg_problem, gtg_problem_full
    assert type(c) is gtg_problem_full and gtg_problem_full.planar.offset == C.sizeof(gtg_problem) and C.sizeof(gtg_problem_full) == C.sizeof(gtg_problem) + C.sizeof(gtg_planar_table)
    assert [f[0] for f in gtg_planar_table._fields_] == ["n_sam2", "sam2_kind", "sam2_pose", "sam2_point", "sam2_z", "sam2_noise"]
    hdr = open(os.path.join(ROOT, "include", "gtsam_amd.h")).read()
    table = hdr[hdr.index("typedef struct gtg_planar_table {"):hdr.index("} gtg_planar_table;")]
    assert re.findall(r"(?:const\s+)?(?:int32_t|int64_t|double)\s*\*?\s*([a-z_0-9]+);", table) == [f[0] for f in gtg_planar_table._fields_]
    body = hdr[hdr.index("typedef struct gtg_problem {"):hdr.index("} gtg_problem;")]
    assert body.rstrip().splitlines()[-1].strip().startswith("gtg_planar_table planar;")


def test_extract_checks_the_noise_dimension_by_kind_and_refuses_a_prior_on_a_point2():
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    nm = A.noiseModel
    for f in (A.BearingRangeFactor2D(X(1), L(1), A.Rot2(0.1), 5.0, nm.Isotropic.Sigma(1, 0.1)),
              A.RangeFactor2D(X(1), L(1), 5.0, nm.Isotropic.Sigma(2, 0.1)),
              A.BearingFactor2D(X(1), L(1), A.Rot2(0.1), nm.Isotropic.Sigma(2, 0.1))):
        graph, initial = D.planar_slam_example()
        graph.add(f)
        with pytest.raises(ValueError, match="NoiseModel has wrong dimension"):
            A.extract(graph, initial)
    graph, initial = D.planar_slam_example()
    graph.add(A._Prior(L(1), A.Point2(1.0, 2.0), nm.Isotropic.Sigma(2, 0.1)))
    with pytest.raises(ValueError, match="PriorFactor on a Point2"):
        A.extract(graph, initial)


def test_add_sam2_takes_what_its_kind_measures():
    p = PL.problem_of(PL.fixture("planar_mixed"))
    n = p.n_sam2
    p.add_sam2(SAM_RANGE, int(p.sam2_pose[0]), int(p.sam2_point[0]), int(p.sam2_noise[p.sam2_kind == 1][0]), range_=3.0)
    assert p.n_sam2 == n + 1 and p.sam2_z[-3:].tolist() == [0.0, 0.0, 3.0]
    with pytest.raises(ValueError):
        p.add_sam2(SAM_BEARING, 0, 1, 0, range_=3.0)
    with pytest.raises(ValueError):
        p.add_sam2(SAM_BEARING_RANGE, 0, 1, 0, bearing=[1, 0])
    with pytest.raises(ValueError):
        p.add_sam2(7, 0, 1, 0, bearing=[1, 0], range_=1.0)


def test_fixture_problems_are_what_extract_returns():
    """Every table but the bearings bit for bit; a bearing to one ulp (the generator stores what the reference's Rot2::fromCosSin makes of
    the mirror's pair)."""
    for name, build in (("planar_mixed", D.planar_mixed_graph), ("planar_slam", D.planar_slam_graph)):
        g = PL.fixture(name)
        made = build(seed=int(g["seed"]))
        p, v0, _ = A.extract(made[0], made[1])
        assert np.array_equal(v0, g["values0"])
        for k, want in g.items():
            if k == "p_sam2_z":
                assert np.abs(p.sam2_z - want).max() <= np.finfo(float).eps, name
                assert np.array_equal(p.sam2_z.reshape(-1, 3)[:, 2], want.reshape(-1, 3)[:, 2])
            elif k.startswith("p_"):
                assert np.array_equal(getattr(p, k[2:]), want), (name, k)
        if len(made) > 2:
            assert {n: int(g["branch_" + n]) for n in made[2]} == made[2]
        ex, ex_v0, _ = A.extract(*D.planar_slam_example())
        assert np.array_equal(ex_v0, g["ex_values0"]) and np.array_equal(ex.sam2_pose, g["ex_p_sam2_pose"]) and np.array_equal(ex.sam2_z, g["ex_p_sam2_z"])


CHILD = r"""
import ctypes, json
import numpy as np
from gtsam_amd import lib as L
from gtsam_amd.problem import Problem
from tests import planar_support as PL
from tests import sam_support as SS
g = PL.fixture("planar_mixed")
out = {}

def info(p, shard=0, n_shards=1):
    def lockstep(ptr, n, stream):
        buf = np.frombuffer((ctypes.c_double * n).from_address(ptr), dtype=np.float64); buf *= n_shards
    d = L.DeviceGraph(p, shard=shard, n_shards=n_shards, allreduce=lockstep if n_shards > 1 else None)
    r = {"values": int(d.val_size), "tangent": int(d.dim_size), "reduced": int(d.reduced_dim), "hash": int(d.structure_hash()), "order": [int(v) for v in d.reduced_order()]}
    d.close()
    return r

def error_of(p=None, shards=1, **override):
    try:
        info(p if p is not None else PL.problem_of(g, **override), 0, shards)
    except L.GtsamAmdError as e:
        return str(e)
    return "no error"

p = PL.problem_of(g)
out["counts"] = [p.n_vars, int((p.var_type == 3).sum()), int((p.var_type == 4).sum()), p.n_sam2]
out["one"] = info(p)
slam = PL.problem_of(PL.fixture("planar_slam"))
out["slam"] = info(slam); out["slam_counts"] = [int((slam.var_type == 3).sum()), int((slam.var_type == 4).sum())]
ex, _ = PL.example_problem(g)
out["example"] = info(ex)
# a Pose2 graph without the table uploads as before
none = dict(sam2_kind=[], sam2_pose=[], sam2_point=[], sam2_z=[], sam2_noise=[])
old = PL.problem_of(g, var_type=np.array(g["p_var_type"])[np.array(g["p_var_type"]) == 3], pose_partial_var=np.array(g["p_pose_partial_var"]) - 33,
                    between_v1=np.array(g["p_between_v1"]) - 33, between_v2=np.array(g["p_between_v2"]) - 33, prior_var=np.array(g["p_prior_var"]) - 33, **none)
c = old.to_ctypes()
out["old_fields"] = [int(c.planar.n_sam2), bool(c.planar.sam2_kind), bool(c.planar.sam2_z)]
out["old"] = info(old)
def with_at(name, i, value):
    a = np.array(g["p_" + name]); a[i] = value; return {name: a}
first = {k: int(np.flatnonzero(p.sam2_kind == k)[0]) for k in (0, 1, 2)}
nz_of = {d: int(np.flatnonzero(p.noise_dim == d)[0]) for d in (1, 2, 3)}
pose0 = int(np.flatnonzero(p.var_type == 3)[0]); pt0 = int(np.flatnonzero(p.var_type == 4)[0])
def retyped(v, t):
    a = np.array(g["p_var_type"]); a[v] = t; return {"var_type": a}
unseen = [v for v in np.flatnonzero(p.var_type == 4)]
sam3 = SS.problem_of(SS.fixture("sam3d_mixed"))
mixed_vars = Problem(var_type=np.concatenate([sam3.var_type, [4]]), **{f: getattr(sam3, f) for f in (
    "noise_kind", "noise_dim", "noise_off", "noise_data", "noise_robust", "noise_robust_param", "sam_kind", "sam_pose", "sam_point", "sam_z", "sam_noise",
    "prior_var", "prior_off", "prior_data", "prior_noise", "between_v1", "between_v2", "between_z", "between_noise")})
with_smart = PL.problem_of(g); n2 = with_smart.add_noise(1, 2, [1.0]); with_smart.add_smart([pose0, pose0 + 1], [1.0, 2.0, 3.0, 4.0], n2)
with_sfm = PL.problem_of(g, sfm_cam=[pose0], sfm_point=[pt0], sfm_z=[0.0, 0.0], sfm_noise=[nz_of[2]])
with_sam3 = PL.problem_of(g, sam_kind=[1], sam_pose=[pose0], sam_point=[pt0], sam_z=[0.0, 0.0, 0.0, 1.0], sam_noise=[nz_of[1]])
with_prior = PL.problem_of(g); n3 = nz_of[3]; with_prior.add_prior(pt0, [1.0, 2.0, 0.0], n3)
out["errors"] = {
    "keys_swapped": error_of(sam2_pose=np.array(g["p_sam2_point"]), sam2_point=np.array(g["p_sam2_pose"])),
    "point_is_pose": error_of(**with_at("sam2_point", first[1], pose0)),
    "pose_is_point": error_of(**with_at("sam2_pose", first[2], pt0)),
    "key_out_of_range": error_of(**with_at("sam2_pose", 0, p.n_vars)),
    "noise_dim_br": error_of(**with_at("sam2_noise", first[0], nz_of[1])),
    "noise_dim_range": error_of(**with_at("sam2_noise", first[1], nz_of[2])),
    "noise_dim_bearing": error_of(**with_at("sam2_noise", first[2], nz_of[2])),
    "kind_high": error_of(**with_at("sam2_kind", 0, 3)),
    "kind_negative": error_of(**with_at("sam2_kind", 0, -1)),
    "pose3_variable": error_of(**retyped(pose0, 0)),
    "point3_variable": error_of(**retyped(pt0, 2)),
    "camera_variable": error_of(**retyped(pose0, 1)),
    "point2_in_a_3d_graph": error_of(mixed_vars),
    "smart_factor": error_of(with_smart),
    "sfm_factor": error_of(with_sfm),
    "sam3d_factor": error_of(with_sam3),
    "prior_on_point2": error_of(with_prior),
    "two_shards": error_of(p, shards=2),
    "unknown_variable_type": error_of(**retyped(pt0, 5)),
}
cp = PL.problem_of(g).to_ctypes()
cp.planar.sam2_z = ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
lib = L.load(); h = ctypes.c_void_p()
assert lib.gtg_create(ctypes.byref(h), 0) == 0
rc = lib.gtg_upload_problem(h, ctypes.byref(cp), 0, 1)
out["null_table"] = [int(rc), lib.gtg_last_error().decode()]
lib.gtg_destroy(h)
# gtg_try_lambda_pcg on a planar graph: refused at the call (the dry-run runtime runs no kernel: linearize returns, the refusal comes first)
d = L.DeviceGraph(p); d.set_values(np.ascontiguousarray(g["values0"])); d.linearize()
try:
    d.try_lambda_pcg(1e-3, False); out["pcg"] = "no error"
except L.GtsamAmdError as e:
    out["pcg"] = str(e)
d.close()
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def result():
    if not os.path.exists(os.path.join(ROOT, "gtsam_amd", "lib", "libgtsam_amd.so")):
        pytest.skip("libgtsam_amd.so not built")
    return HP.run_snippet(CHILD)


def test_upload_sizes_and_the_symbolic_analysis(result):
    n_vars, n_poses, n_points, n_sam2 = result["counts"]
    assert (n_vars, n_poses, n_points, n_sam2) == (45, 12, 33, 158)
    one = result["one"]
    # three storage doubles and three tangent entries per variable of either type; every POINT2 is a landmark: the reduced system is the poses
    assert one["values"] == 3 * n_vars and one["tangent"] == 3 * n_vars and one["reduced"] == 3 * n_poses and one["hash"] != 0
    p = PL.problem_of(PL.fixture("planar_mixed"))
    assert sorted(one["order"]) == sorted(int(v) for v in np.flatnonzero(p.var_type == VAR_POSE2))
    poses, points = result["slam_counts"]
    assert (poses, points) == (40, 120) and result["slam"]["reduced"] == 3 * poses and result["slam"]["tangent"] == 3 * (poses + points)
    assert result["example"]["reduced"] == 9 and result["example"]["values"] == 15


def test_a_pose2_graph_without_the_table_uploads_as_before(result):
    assert result["old_fields"] == [0, False, False]
    assert result["old"]["reduced"] == 36 and result["old"]["values"] == 36 and result["old"]["hash"] != 0


def test_refusals_and_their_text(result):
    e = result["errors"]
    assert "keys must be (POSE2, POINT2)" in e["keys_swapped"]
    assert "RangeFactor2D keys must be (POSE2, POINT2)" in e["point_is_pose"], e["point_is_pose"]
    assert "BearingFactor2D keys must be (POSE2, POINT2)" in e["pose_is_point"], e["pose_is_point"]
    assert "factor refers to a key that is not in Values" in e["key_out_of_range"]
    assert "BearingRangeFactor2D: NoiseModel has wrong dimension" in e["noise_dim_br"], e["noise_dim_br"]
    assert "RangeFactor2D: NoiseModel has wrong dimension" in e["noise_dim_range"] and "Bearing" not in e["noise_dim_range"]
    assert "BearingFactor2D: NoiseModel has wrong dimension" in e["noise_dim_bearing"], e["noise_dim_bearing"]
    for k in ("kind_high", "kind_negative"):
        assert "unknown sam2_kind" in e[k], (k, e[k])
    for k in ("pose3_variable", "point3_variable", "camera_variable", "point2_in_a_3d_graph", "smart_factor", "sfm_factor", "sam3d_factor"):
        assert "planar graph: POINT2 variables and planar bearing / range factors cannot share a graph with" in e[k], (k, e[k])
    assert "PriorFactor on a POINT2 variable is not supported" in e["prior_on_point2"], e["prior_on_point2"]
    assert "planar graph: n_shards > 1 is not supported" in e["two_shards"], e["two_shards"]
    assert "unknown variable type" in e["unknown_variable_type"]
    assert result["null_table"][0] == -1 and "planar bearing / range factor tables missing" in result["null_table"][1]      # GTG_ERR_USAGE
    assert "gtg_try_lambda_pcg: a planar graph" in result["pcg"], result["pcg"]
