"""gtg_upload_problem with TriangulationParameters::useLOST (smart_params[8 i + 7]), on the CPU: the product library in a child process
under tools/hipstub (a dry-run HIP runtime: host code only, no kernel runs).  Upload of every fixture; the LOST work space exists only
where LOST is in use and holds 8 doubles per smart measurement of the shard; a graph with LOST off uploads what it uploaded before
(turning LOST on changes one host-to-device copy, the parameter table, and adds none); a negative or non-finite slot is refused with its
own message; the getter's argument checks."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402

CHILD = r"""
import ctypes, json
import numpy as np
from tools import host_profile as HP
from gtsam_amd import lib as L
from tests import smart_lost_support as S
from tests import smart_pose_support as SP
stub = ctypes.CDLL(HP.STUB)
stub.hipstub_h2d_record.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ulonglong)]
out = {"fixtures": {}}

def open_graph(p, shard=0, n_shards=1):
    def lockstep(ptr, n, stream):
        buf = np.frombuffer((ctypes.c_double * n).from_address(ptr), dtype=np.float64); buf *= n_shards
    return L.DeviceGraph(p, shard=shard, n_shards=n_shards, allreduce=lockstep if n_shards > 1 else None)

def info(p, shard=0, n_shards=1):
    stub.hipstub_reset()
    d = open_graph(p, shard, n_shards)
    n = ctypes.c_longlong(); h = ctypes.c_ulonglong(); rec = []
    for i in range(stub.hipstub_h2d_count()):
        stub.hipstub_h2d_record(i, ctypes.byref(n), ctypes.byref(h)); rec.append("%d:%d" % (n.value, h.value))
    r = {"values": int(d.val_size), "workspace": d.smart_lost_workspace(), "records": rec}
    d.close()
    return r

def lost_off(g):
    prm = np.array(g["p_smart_params"]).reshape(-1, 8); prm[:, 7] = 0.0
    return S.problem_of(g, smart_params=prm.reshape(-1))

for name in S.FIXTURES:
    g, p, v0 = S.load(name)
    out["fixtures"][name] = {"on": info(p), "off": info(lost_off(g)), "two": [info(p, s, 2)["workspace"] for s in range(2)],
                             "two_off": [info(lost_off(g), s, 2)["workspace"] for s in range(2)],
                             "meas": int(p.smart_ptr[-1]), "v0": int(v0.size), "n_smart": int(p.n_smart)}
_, pp, _ = SP.load("smart_pose_mixed")
out["dlt_fixture_workspace"] = info(pp)["workspace"]

def error_of(q):
    try:
        info(q)
    except L.GtsamAmdError as e:
        return str(e)
    return "no error"

g, p, v0 = S.load("smart_lost_pose")
e = {}
for tag, val in (("negative", -1e-4), ("nan", float("nan")), ("inf", float("inf")), ("tiny", 1e-300)):
    prm = np.array(g["p_smart_params"]).reshape(-1, 8); prm[5, 7] = val
    e[tag] = error_of(S.problem_of(g, smart_params=prm.reshape(-1)))
out["errors"] = e
d = open_graph(p)
st, pts = np.zeros(p.n_smart, np.int32), np.zeros((p.n_smart, 3))
rc = L.load().gtg_get_smart_triangulation(d.h, st.ctypes.data, pts.ctypes.data, p.n_smart)
out["getter_before"] = int(rc)
try:
    d.smart_triangulation(); out["getter_message"] = "no error"
except L.GtsamAmdError as ex:
    out["getter_message"] = str(ex)
out["getter_wrong_n"] = int(L.load().gtg_get_smart_triangulation(d.h, st.ctypes.data, pts.ctypes.data, p.n_smart - 1))
d.close()
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def result():
    if not os.path.exists(os.path.join(ROOT, "gtsam_amd", "lib", "libgtsam_amd.so")):
        pytest.skip("libgtsam_amd.so not built")
    return HP.run_snippet(CHILD)


def test_work_space_only_where_lost_is_in_use(result):
    for name, r in result["fixtures"].items():
        assert r["on"]["workspace"] == 8 * r["meas"] > 0, name
        assert r["off"]["workspace"] == 0 and r["two_off"] == [0, 0], name
        assert sum(r["two"]) == 8 * r["meas"] and min(r["two"]) > 0, name          # per shard: its own measurements
        assert r["on"]["values"] == r["off"]["values"] == r["v0"]
    assert result["dlt_fixture_workspace"] == 0


def test_lost_changes_one_upload_and_adds_none(result):
    """The work space is allocated, not uploaded: with LOST on, the same host-to-device copies, and exactly one of them
    -- the 8-doubles-per-factor parameter table -- with other contents."""
    from collections import Counter
    for name, r in result["fixtures"].items():
        on, off = r["on"]["records"], r["off"]["records"]
        assert len(on) == len(off) > 20, name
        only_on, only_off = list((Counter(on) - Counter(off)).elements()), list((Counter(off) - Counter(on)).elements())
        assert len(only_on) == len(only_off) == 1, (name, only_on, only_off)       # (copies of independent tables may swap places)
        assert only_on[0].split(":")[0] == only_off[0].split(":")[0] == str(64 * r["n_smart"])


def test_a_bad_slot_is_refused_with_its_message(result):
    e = result["errors"]
    for tag in ("negative", "nan", "inf"):
        assert "useLOST sigma" in e[tag] and "smart_params[8 i + 7]" in e[tag], (tag, e[tag])
    assert e["tiny"] == "no error"


def test_getter_checks_its_arguments(result):
    assert result["getter_before"] != 0 and result["getter_wrong_n"] != 0
    assert "gtg_error or gtg_linearize first" in result["getter_message"]
