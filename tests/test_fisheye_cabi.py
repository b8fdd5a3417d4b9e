"""gtg_set_calibration_models and what gtg_upload_problem does with its list, on the CPU: the product library in a child process under
tools/hipstub (a dry-run HIP runtime: host code only, no kernel runs).  The protocol of the setter (kept by the handle, consumed by one
upload -- also by one that fails --, NULL clears, wrong length); every refusal by its own message; an upload without the call, or
with every model zero, makes the host-to-device copies it made before in their order and reports the same structure hash, while a
fisheye row adds exactly one copy, the model table (the form of the projection range is not visible through the C ABI in any other way:
its records have the layout of a two-row graph)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402

CHILD = r"""
import ctypes as C, json
import numpy as np
from tools import host_profile as HP
from gtsam_amd import lib as L
from tests import fisheye_support as FS
from tests import planar_support as PL
from tests import smart_pose_support as SP
from tests import smart_rig_support as SR
stub = C.CDLL(HP.STUB)
stub.hipstub_h2d_record.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong)]
lib = L.load()
out = {}

def create():
    h = C.c_void_p()
    assert lib.gtg_create(C.byref(h), 0) == 0
    return h

def set_models(h, model):
    if model is None:
        return lib.gtg_set_calibration_models(h, None, 0)
    m = np.ascontiguousarray(model, np.int32)
    return lib.gtg_set_calibration_models(h, m.ctypes.data, m.size)

def upload(h, p):
    # -> (rc, message, host-to-device copies "bytes:hash" in order, structure hash)
    stub.hipstub_reset()
    cp = p.to_ctypes()
    rc = lib.gtg_upload_problem(h, C.byref(cp), 0, 1)
    n = C.c_longlong(); hh = C.c_ulonglong(); rec = []
    for i in range(stub.hipstub_h2d_count()):
        stub.hipstub_h2d_record(i, C.byref(n), C.byref(hh)); rec.append("%d:%d" % (n.value, hh.value))
    return int(rc), lib.gtg_last_error().decode() if rc < 0 else "", rec, int(lib.gtg_structure_hash(h)) if rc >= 0 else 0

def once(p, model):
    h = create()
    assert set_models(h, model) == 0
    r = upload(h, p)
    lib.gtg_destroy(h)
    return r

g = FS.fixture("fisheye_mixed")
p = FS.problem_of(g, calib_model=[])          # (the list goes through the setter by hand here)
model = [int(m) for m in g["p_calib_model"]]
out["n_calib"] = len(model)

# ---- the protocol
h = create()
assert set_models(h, model) == 0
out["first"] = upload(h, p)
out["second"] = upload(h, p)                  # the list was consumed: every row a pinhole again
assert set_models(h, model) == 0 and set_models(h, None) == 0
out["cleared"] = upload(h, p)
assert set_models(h, model[:3]) == 0
out["wrong_length"] = upload(h, p)
out["after_failure"] = upload(h, p)           # consumed by the upload that failed
lib.gtg_destroy(h)
out["never_set"] = once(p, None)
out["all_zero"] = once(p, [0] * len(model))
out["negative_n"] = int(lib.gtg_set_calibration_models(create(), np.zeros(1, np.int32).ctypes.data, -1))
out["null_handle"] = int(lib.gtg_set_calibration_models(None, None, 0))
# through the Python surface: DeviceGraph calls the setter for the fixture's own list, and not for an all-zero one
stub.hipstub_reset(); d = L.DeviceGraph(FS.problem_of(g)); out["device_graph"] = stub.hipstub_h2d_count(); d.close()
stub.hipstub_reset(); d = L.DeviceGraph(FS.problem_of(g, calib_model=[0] * len(model))); out["device_graph_zero"] = stub.hipstub_h2d_count(); d.close()

# ---- the refusals
e = {}
e["unknown_model"] = once(p, [1, 0, 2, 0])[1]
e["no_distortion"] = once(FS.problem_of(g, calib_model=[], calib_distortion=np.zeros(0)), model)[1]
gs = FS.fixture("stereo_mixed"); ps = FS.problem_of(gs)
n = ps.calib.size // 5
row = lambda k: [1 if i == k else 0 for i in range(n)]
named = int(ps.stereo_calib[0]); mono_only = [k for k in set(ps.proj_calib.tolist()) if k not in set(ps.stereo_calib.tolist())][0]
e["stereo_names"] = once(ps, row(named))[1]
e["beside_stereo"] = once(ps, row(mono_only))[1]
gm = FS.fixture("sam3d_mixed"); pm = FS.problem_of(gm)
nm = pm.calib.size // 5
dist = pm.calib_distortion if pm.calib_distortion.size else np.zeros(4 * nm)
pm = FS.problem_of(gm, calib_distortion=dist, stereo_pose=[], stereo_point=[], stereo_z=[], stereo_noise=[], stereo_calib=[], stereo_sensor=[], calib_baseline=[])
e["beside_sam"] = once(pm, [1 if i == int(pm.proj_calib[0]) else 0 for i in range(nm)])[1]
_, pp, _ = SP.load("smart_pose_mixed")
npc = pp.calib.size // 5
pp.calib_distortion = np.zeros(4 * npc)
e["smart_calib"] = once(pp, [1 if i == int(pp.smart_calib[0]) else 0 for i in range(npc)])[1]
_, pq, _ = SP.load("smart_pose_mixed")       # a fisheye row that no factor names, beside smart factors
pq.calib = np.concatenate([pq.calib, [300.0, 300.0, 0.0, 320.0, 240.0]]); pq.calib_distortion = np.zeros(4 * (npc + 1))
e["beside_smart"] = once(pq, [0] * npc + [1])[1]
_, pr, _ = SR.load("smart_rig_mixed")
nrc = pr.calib.size // 5
pr.calib_distortion = np.zeros(4 * nrc)
rig_meas = np.flatnonzero(pr.smart_meas_calib >= 0)
e["smart_meas_calib"] = once(pr, [1 if i == int(pr.smart_meas_calib[rig_meas[0]]) else 0 for i in range(nrc)])[1]
gl = PL.fixture("planar_mixed")
pl = PL.problem_of(gl, calib=[300.0, 300.0, 0.0, 320.0, 240.0], calib_distortion=np.zeros(4))
e["planar"] = once(pl, [1])[1]
out["planar_without"] = once(pl, None)[0]
out["errors"] = e
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def result():
    if not os.path.exists(os.path.join(ROOT, "gtsam_amd", "lib", "libgtsam_amd.so")):
        pytest.skip("libgtsam_amd.so not built")
    return HP.run_snippet(CHILD)


def test_the_list_is_consumed_by_one_upload(result):
    first, second, never = result["first"], result["second"], result["never_set"]
    assert first[0] == 0 and second[0] == 0 and never[0] == 0
    assert second[2] == never[2] and len(first[2]) == len(never[2]) + 1
    # the one more copy is the model table: an int32 per calib row, between copies that are otherwise the same in the same order
    extra = [i for i in range(len(first[2])) if first[2][:i] + first[2][i + 1:] == never[2]]
    assert len(extra) >= 1 and first[2][extra[0]].split(":")[0] == str(4 * result["n_calib"])
    assert first[3] == second[3] == never[3] != 0                 # the layout of the reduced system does not depend on the camera model


def test_null_clears_and_a_failed_upload_consumes(result):
    assert result["cleared"][0] == 0 and result["cleared"][2] == result["never_set"][2]
    rc, msg, _, _ = result["wrong_length"]
    assert rc < 0 and "n_calib differs" in msg and "gtg_set_calibration_models" in msg
    assert result["after_failure"][0] == 0 and result["after_failure"][2] == result["never_set"][2]
    assert result["negative_n"] < 0 and result["null_handle"] < 0


def test_without_the_call_or_with_all_zero_models_nothing_changes(result):
    never, zero = result["never_set"], result["all_zero"]
    assert zero[0] == 0 and zero[2] == never[2] and zero[3] == never[3] and len(never[2]) > 20
    assert result["device_graph"] == len(never[2]) + 1 and result["device_graph_zero"] == len(never[2])


def test_every_refusal_has_its_own_message(result):
    e = result["errors"]
    want = {"unknown_model": "unknown calibration model",
            "no_distortion": "needs calib_distortion",
            "stereo_names": "a GenericStereoFactor names a fisheye calibration row",
            "smart_calib": "through smart_calib",
            "smart_meas_calib": "through smart_meas_calib",
            "beside_stereo": "in a graph with stereo, 3-D bearing / range or smart factors",
            "beside_sam": "in a graph with stereo, 3-D bearing / range or smart factors",
            "beside_smart": "in a graph with stereo, 3-D bearing / range or smart factors",
            "planar": "in a planar graph"}
    assert set(e) == set(want)
    for k, text in want.items():
        assert text in e[k], (k, e[k])
    assert len({e[k] for k in ("unknown_model", "no_distortion", "stereo_names", "smart_calib", "smart_meas_calib", "beside_stereo", "planar")}) == 7
    assert result["planar_without"] == 0                          # the same planar problem uploads without the list
