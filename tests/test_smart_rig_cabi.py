"""gtg_upload_problem with rig-type smart factors (smart_calib == GTG_SMART_RIG, smart_meas_calib / smart_meas_sensor), on the CPU: the
product library in a child process under tools/hipstub (a dry-run HIP runtime: host code only, no kernel runs).  Upload of both
fixtures, the repeated-key flag (one shard, two shards, graphs without a repeated key), and each refusal with its message."""
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
from gtsam_amd.problem import VAR_POSE3, VAR_POINT3, SMART_RIG
from tests import smart_rig_support as S
from tests import smart_pose_support as SP
out = {"fixtures": {}}

def info(p, shard=0, n_shards=1):
    def lockstep(ptr, n, stream):
        buf = np.frombuffer((ctypes.c_double * n).from_address(ptr), dtype=np.float64); buf *= n_shards
    d = L.DeviceGraph(p, shard=shard, n_shards=n_shards, allreduce=lockstep if n_shards > 1 else None)
    r = {"values": int(d.val_size), "tangent": int(d.dim_size), "reduced": int(d.reduced_dim), "hash": int(d.structure_hash()),
         "repeats": d.smart_repeated_keys()}
    d.close()
    return r

for name in S.FIXTURES:
    g, p, v0 = S.load(name)
    out["fixtures"][name] = {"info": info(p), "two": [info(p, s, 2) for s in range(2)], "poses": int((p.var_type == VAR_POSE3).sum()),
                             "points": int((p.var_type == VAR_POINT3).sum()), "smart": p.n_smart, "v0": int(v0.size),
                             "repeated_tracks": int(S.repeated(p).sum())}
g, p, v0 = S.load("smart_rig_mixed")
norep = S.one_camera_per_track(p)
out["norep"] = [info(norep)["repeats"]] + [info(norep, s, 2)["repeats"] for s in range(2)]
out["as_pose"] = info(S.as_pose_type(norep))["repeats"]
# a repeated key in a POSE-type factor is not this flag's business: such graphs launch what they launched before
gp, pp, _ = SP.load("smart_pose_mixed")
out["pose_fixture"] = info(pp)["repeats"]
# the only repeated key of the graph in the LAST track: whichever shard owns it, both report it
last = S.one_camera_per_track(p)
a = int(last.smart_ptr[-2])
assert last.smart_calib[-1] == SMART_RIG and int(last.smart_ptr[-1]) - a >= 2
cam = np.array(last.smart_cam); cam[a + 1] = cam[a]; last.smart_cam = cam
out["last_track"] = [info(last)["repeats"]] + [info(last, s, 2)["repeats"] for s in range(2)]

def error_of(q):
    try:
        info(q)
    except L.GtsamAmdError as e:
        return str(e)
    return "no error"

def mixed(**override):
    return S.problem_of(g, **override)

rig0 = int(np.flatnonzero(p.smart_calib == SMART_RIG)[0]); k0 = int(p.smart_ptr[rig0])
def at(name, index, value):
    a = np.array(g["p_" + name]); a[index] = value; return {name: a}

e = {}
prm = np.array(g["p_smart_params"]).reshape(-1, 8)
for tag, col, val in (("degeneracy", 4, 0.0), ("degeneracy2", 4, 2.0), ("linearization", 5, 2.0), ("epi", 6, 1.0)):
    q = prm.copy(); q[rig0, col] = val
    e[tag] = error_of(mixed(smart_params=q.reshape(-1)))
d = np.zeros(4 * (p.calib.size // 5)); d[4 * int(p.smart_meas_calib[k0])] = 0.01
e["distortion"] = error_of(mixed(calib_distortion=d))
e["sensor_on_rig"] = error_of(mixed(**at("smart_sensor", rig0, 0)))
e["tables_missing"] = error_of(mixed(smart_meas_calib=[], smart_meas_sensor=[]))
e["calib_high"] = error_of(mixed(**at("smart_meas_calib", k0, p.calib.size // 5)))
e["calib_low"] = error_of(mixed(**at("smart_meas_calib", k0, -1)))
e["sensor_high"] = error_of(mixed(**at("smart_meas_sensor", k0, p.sensor.size // 12)))
e["sensor_low"] = error_of(mixed(**at("smart_meas_sensor", k0, -2)))
e["smart_calib_low"] = error_of(mixed(**at("smart_calib", rig0, -3)))
pt0 = int(np.flatnonzero(p.var_type == VAR_POINT3)[0])
e["key_is_point"] = error_of(mixed(**at("smart_cam", k0, pt0)))
e["key_out_of_range"] = error_of(mixed(**at("smart_cam", k0, p.n_vars)))
e["camera_type_beside"] = error_of(mixed(**at("smart_calib", rig0 + 1 if p.smart_calib[rig0 + 1] == SMART_RIG else rig0, -1)))
q = mixed(stereo_pose=[0], stereo_point=[pt0], stereo_z=[1.0, 2.0, 3.0], stereo_calib=[0], stereo_sensor=[-1], calib_baseline=np.full(p.calib.size // 5, 0.2))
q.stereo_noise = np.array([q.add_noise(1, 3, [1.0])], np.int32)
e["with_stereo"] = error_of(q)
q = mixed()
q.add_sam(1, 0, pt0, q.add_noise(1, 1, [1.0]), range_=2.0)
e["with_sam"] = error_of(q)
out["errors"] = e
# untouched tables of other factors' measurements are not read: garbage at the measurements of the pose-type factors
pose0 = int(np.flatnonzero(p.smart_calib >= 0)[0])
junk = np.array(g["p_smart_meas_calib"]); junk[int(p.smart_ptr[pose0]):int(p.smart_ptr[pose0 + 1])] = 12345
out["junk_at_pose_type"] = error_of(mixed(smart_meas_calib=junk))
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def result():
    if not os.path.exists(os.path.join(ROOT, "gtsam_amd", "lib", "libgtsam_amd.so")):
        pytest.skip("libgtsam_amd.so not built")
    return HP.run_snippet(CHILD)


def test_upload_accepts_both_fixtures_and_sizes_exclude_hidden_landmarks(result):
    for name, r in result["fixtures"].items():
        i = r["info"]
        assert r["smart"] > 0 and r["repeated_tracks"] > 0
        assert i["values"] == 12 * r["poses"] + 3 * r["points"] == r["v0"], name
        assert i["tangent"] == 6 * r["poses"] + 3 * r["points"], name
        assert i["reduced"] == 6 * r["poses"], name
        assert r["two"][0]["hash"] == r["two"][1]["hash"] == i["hash"] != 0
    assert result["fixtures"]["smart_rig_pair"]["poses"] == 3 and result["fixtures"]["smart_rig_mixed"]["points"] == 5


def test_repeated_key_flag_is_the_whole_graphs_on_every_shard(result):
    for name, r in result["fixtures"].items():
        assert r["info"]["repeats"] == 1 and [t["repeats"] for t in r["two"]] == [1, 1], name
    assert result["norep"] == [0, 0, 0] and result["as_pose"] == 0 and result["pose_fixture"] == 0
    assert result["last_track"] == [1, 1, 1]


def test_each_refusal_names_its_cause(result):
    e = result["errors"]
    assert "ZERO_ON_DEGENERACY" in e["degeneracy"] and "rig-type" in e["degeneracy"] and "ZERO_ON_DEGENERACY" in e["degeneracy2"]
    assert "linearizationMode must be set to HESSIAN" in e["linearization"] and "rig-type" in e["linearization"]
    assert "enableEPI is not supported on a rig-type smart factor" in e["epi"]
    assert "Cal3DS2 distortion" in e["distortion"] and "rig-type" in e["distortion"]
    assert "smart_sensor must be -1 on a rig-type smart factor" in e["sensor_on_rig"]
    assert "needs the per-measurement tables smart_meas_calib and smart_meas_sensor" in e["tables_missing"]
    assert "smart_meas_calib index out of range" in e["calib_high"] and "smart_meas_calib index out of range" in e["calib_low"]
    assert "smart_meas_sensor index out of range" in e["sensor_high"] and "smart_meas_sensor index out of range" in e["sensor_low"]
    assert "smart_calib index out of range" in e["smart_calib_low"]
    assert "rig-type smart factor must be POSE3 variables" in e["key_is_point"] and "must be POSE3 variables" in e["key_out_of_range"]
    assert "mixes camera-type" in e["camera_type_beside"]
    assert "GenericStereoFactor" in e["with_stereo"] and "bearing / range" in e["with_sam"]


def test_tables_are_read_at_rig_measurements_only(result):
    assert result["junk_at_pose_type"] == "no error"
