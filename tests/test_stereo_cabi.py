"""gtg_upload_problem with GenericStereoFactor tables, on the CPU: the product library in a child process under tools/hipstub (a
dry-run HIP runtime: host code only, no kernel runs).  Upload of stereo_mixed on one and on two shards, the landmark / reduced
split, the sizes, the structure hash across shards, every usage error of the stereo tables, and an old-style problem."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402

CHILD = r"""
import ctypes, json
import numpy as np
from gtsam_amd import lib as L
from tests import stereo_support as S
g = S.fixture("stereo_mixed")
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
        info(S.problem_of(g, **override))
    except L.GtsamAmdError as e:
        return str(e)
    return "no error"

p = S.problem_of(g)
out["counts"] = [p.n_vars, p.n_proj, p.n_stereo, int((p.var_type == 2).sum())]
out["one"] = info(p)
out["two"] = [info(p, s, 2) for s in range(2)]
stereo_only = S.problem_of(g, proj_pose=[], proj_point=[], proj_z=[], proj_noise=[], proj_calib=[], proj_sensor=[])
out["stereo_only"] = info(stereo_only)
# an old-style problem: the new fields zero / NULL
old = S.problem_of(g, stereo_pose=[], stereo_point=[], stereo_z=[], stereo_noise=[], stereo_calib=[], stereo_sensor=[], calib_baseline=[])
c = old.to_ctypes()
out["old_fields"] = [int(c.n_stereo), bool(c.stereo_pose), bool(c.calib_baseline)]
out["old"] = info(old)
n2 = int(np.flatnonzero(p.noise_dim == 2)[0]); pose0 = int(np.flatnonzero(p.var_type == 0)[0]); pt0 = int(np.flatnonzero(p.var_type == 2)[0])
def with_first(name, value):
    a = np.array(g["p_" + name]); a[0] = value; return {name: a}
out["errors"] = {
    "keys_swapped": error_of(stereo_pose=np.array(g["p_stereo_point"]), stereo_point=np.array(g["p_stereo_pose"])),
    "point_is_pose": error_of(**with_first("stereo_point", pose0)),
    "pose_is_point": error_of(**with_first("stereo_pose", pt0)),
    "key_out_of_range": error_of(**with_first("stereo_pose", p.n_vars)),
    "noise_dim": error_of(**with_first("stereo_noise", n2)),
    "noise_index": error_of(**with_first("stereo_noise", p.noise_kind.size)),
    "calib_high": error_of(**with_first("stereo_calib", p.calib.size // 5)),
    "calib_negative": error_of(**with_first("stereo_calib", -1)),
    "sensor_high": error_of(**with_first("stereo_sensor", p.sensor.size // 12)),
}
# calib_baseline NULL with n_stereo > 0: through the struct (the Python wrapper refuses to build such a problem)
q = S.problem_of(g)
try:
    q.calib_baseline = np.zeros(0); q.to_ctypes(); out["wrapper_refuses_missing_baseline"] = False
except ValueError:
    out["wrapper_refuses_missing_baseline"] = True
q = S.problem_of(g)
cp = q.to_ctypes()
cp.calib_baseline = ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
lib = L.load(); h = ctypes.c_void_p()
assert lib.gtg_create(ctypes.byref(h), 0) == 0
rc = lib.gtg_upload_problem(h, ctypes.byref(cp), 0, 1)
out["null_baseline"] = [int(rc), lib.gtg_last_error().decode()]
cp = q.to_ctypes()
cp.stereo_z = ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
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
    n_vars, n_proj, n_stereo, n_points = result["counts"]
    n_poses = n_vars - n_points
    assert (n_poses, n_points, n_proj, n_stereo) == (6, 40, 41, 316)
    one = result["one"]
    assert one["values"] == 12 * n_poses + 3 * n_points and one["tangent"] == 6 * n_poses + 3 * n_points
    # every POINT3 is a landmark (touched by stereo / projection factors and a prior only): the reduced system is the poses
    assert one["reduced"] == 6 * n_poses
    # a stereo-only graph takes the same Schur path
    assert result["stereo_only"]["reduced"] == 6 * n_poses and result["stereo_only"]["tangent"] == one["tangent"]


def test_two_shards_share_the_layout(result):
    one, two = result["one"], result["two"]
    assert two[0]["hash"] == two[1]["hash"] == one["hash"] != 0
    assert [t["reduced"] for t in two] == [one["reduced"]] * 2 and [t["tangent"] for t in two] == [one["tangent"]] * 2


def test_old_style_problem_behaves_as_before(result):
    assert result["old_fields"] == [0, False, False]
    assert result["old"]["reduced"] == result["one"]["reduced"] and result["old"]["values"] == result["one"]["values"]


def test_usage_errors_and_their_text(result):
    e = result["errors"]
    for k in ("keys_swapped", "point_is_pose", "pose_is_point"):
        assert "GenericStereoFactor keys must be (POSE3, POINT3)" in e[k], (k, e[k])
    assert "factor refers to a key that is not in Values" in e["key_out_of_range"]
    for k in ("noise_dim", "noise_index"):
        assert "GenericStereoFactor: NoiseModel has wrong dimension" in e[k], (k, e[k])
    for k in ("calib_high", "calib_negative"):
        assert "bad calibration index" in e[k], (k, e[k])
    assert "bad body_P_sensor index" in e["sensor_high"]
    assert result["wrapper_refuses_missing_baseline"]
    assert result["null_baseline"][0] == -1 and "calib_baseline" in result["null_baseline"][1]      # GTG_ERR_USAGE
    assert result["null_table"][0] == -1 and "stereo factor tables missing" in result["null_table"][1]
