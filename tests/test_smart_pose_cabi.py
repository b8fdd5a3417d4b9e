"""gtg_upload_problem with pose-type smart factors (smart_calib / smart_sensor), on the CPU: the product library in a child process
under tools/hipstub (a dry-run HIP runtime: host code only, no kernel runs).  Upload of every fixture, the sizes without the hidden
landmarks, two shards, each refusal with its message, and an old-style problem (smart_calib == NULL)."""
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
from gtsam_amd import datasets as D
from gtsam_amd.problem import smart_bal_problem, VAR_POSE3, VAR_POINT3
from tests import smart_pose_support as S
out = {"fixtures": {}}

def info(p, shard=0, n_shards=1):
    def lockstep(ptr, n, stream):
        buf = np.frombuffer((ctypes.c_double * n).from_address(ptr), dtype=np.float64); buf *= n_shards
    d = L.DeviceGraph(p, shard=shard, n_shards=n_shards, allreduce=lockstep if n_shards > 1 else None)
    r = {"values": int(d.val_size), "tangent": int(d.dim_size), "reduced": int(d.reduced_dim), "hash": int(d.structure_hash())}
    d.close()
    return r

for name in S.FIXTURES:
    g, p, v0 = S.load(name)
    out["fixtures"][name] = {"info": info(p), "poses": int((p.var_type == VAR_POSE3).sum()), "points": int((p.var_type == VAR_POINT3).sum()),
                             "smart": p.n_smart, "v0": int(v0.size)}
g, p, v0 = S.load("smart_pose_mixed")
out["one"] = info(p)
out["two"] = [info(p, s, 2) for s in range(2)]

def error_of(q):
    try:
        info(q)
    except L.GtsamAmdError as e:
        return str(e)
    return "no error"

def mixed(**override):
    return S.problem_of(g, **override)

def with_first(name, value):
    a = np.array(g["p_" + name]); a[0] = value; return {name: a}

e = {}
# camera-type and pose-type factors in one graph
a = np.array(g["p_smart_calib"]); a[1] = -1
e["mixed_kinds"] = error_of(mixed(smart_calib=a))
# beside stereo factors
pt0 = int(np.flatnonzero(p.var_type == VAR_POINT3)[0]); n3 = None
q = mixed(stereo_pose=[0], stereo_point=[pt0], stereo_z=[1.0, 2.0, 3.0], stereo_calib=[0], stereo_sensor=[-1], calib_baseline=np.full(p.calib.size // 5, 0.2))
q.stereo_noise = np.array([q.add_noise(1, 3, [1.0])], np.int32)
e["with_stereo"] = error_of(q)
d = np.zeros(4 * (p.calib.size // 5)); d[0] = 0.01
e["distortion"] = error_of(mixed(calib_distortion=d))
prm = np.array(g["p_smart_params"]); prm[6] = 1.0
e["epi"] = error_of(mixed(smart_params=prm))
e["key_is_point"] = error_of(mixed(**with_first("smart_cam", pt0)))
e["key_out_of_range"] = error_of(mixed(**with_first("smart_cam", p.n_vars)))
e["calib_high"] = error_of(mixed(**with_first("smart_calib", p.calib.size // 5)))
e["sensor_high"] = error_of(mixed(**with_first("smart_sensor", p.sensor.size // 12)))
e["sensor_low"] = error_of(mixed(**with_first("smart_sensor", -2)))
out["errors"] = e
# an old-style problem: smart_calib NULL = camera-type factors, as before
cams, pts, oc, op, oz = D.synthetic_orbit_scene(n_cams=5, n_points=20, seed=1)
old, _ = smart_bal_problem(cams, oc, op, oz)
c = old.to_ctypes()
out["old_fields"] = [bool(c.smart_calib), bool(c.smart_sensor), int(c.n_smart)]
out["old"] = info(old); out["old_cams"] = int(old.n_vars)
# ... and pose keys handed to a camera-type table are refused as before
bad = mixed(smart_calib=[], smart_sensor=[])
out["pose_keys_without_calib"] = error_of(bad)
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def result():
    if not os.path.exists(os.path.join(ROOT, "gtsam_amd", "lib", "libgtsam_amd.so")):
        pytest.skip("libgtsam_amd.so not built")
    return HP.run_snippet(CHILD)


def test_upload_accepts_every_fixture_and_sizes_exclude_hidden_landmarks(result):
    for name, r in result["fixtures"].items():
        i = r["info"]
        assert r["smart"] > 0
        assert i["values"] == 12 * r["poses"] + 3 * r["points"] == r["v0"], name
        assert i["tangent"] == 6 * r["poses"] + 3 * r["points"], name
        # every POINT3, hidden or explicit, is a landmark: the reduced system is the poses
        assert i["reduced"] == 6 * r["poses"], name
    assert result["fixtures"]["smart_pose_mixed"]["points"] == 6 and result["fixtures"]["smart_pose_mixed"]["smart"] == 291


def test_two_shards_share_the_layout(result):
    one, two = result["one"], result["two"]
    assert two[0]["hash"] == two[1]["hash"] == one["hash"] != 0
    assert [t["reduced"] for t in two] == [one["reduced"]] * 2 and [t["tangent"] for t in two] == [one["tangent"]] * 2


def test_each_refusal_names_its_cause(result):
    e = result["errors"]
    assert "mixes camera-type" in e["mixed_kinds"] and "pose-type" in e["mixed_kinds"]
    assert "GenericStereoFactor" in e["with_stereo"] and "pose-type smart factors" in e["with_stereo"]
    assert "Cal3DS2 distortion" in e["distortion"]
    assert "enableEPI is not supported on a pose-type smart factor" in e["epi"]
    assert "must be POSE3 variables" in e["key_is_point"] and "must be POSE3 variables" in e["key_out_of_range"]
    assert "smart_calib index out of range" in e["calib_high"]
    assert "smart_sensor index out of range" in e["sensor_high"] and "smart_sensor index out of range" in e["sensor_low"]


def test_problem_without_smart_calib_behaves_as_before(result):
    assert result["old_fields"][:2] == [False, False] and result["old_fields"][2] > 0
    assert result["old"]["tangent"] == 9 * result["old_cams"] and result["old"]["values"] == 17 * result["old_cams"]
    assert "its keys must be SFM_CAMERA variables" in result["pose_keys_without_calib"]
