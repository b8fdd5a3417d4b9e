"""The C++ shim's extractor on a graph with SmartProjectionRigFactor<PinholePose<Cal3_S2>> against the Python mirror's, on the CPU: both
run under tools/hipstub, which hashes every host-to-device copy (tests/test_shim_extractor_cpu.py explains the method).  Equal records:
the library was handed identical tables -- the smart tables with smart_calib = GTG_SMART_RIG and the per-measurement calib / sensor
rows (one per rig camera, the extrinsics behind the other sensor rows), the pose-type factors' rows beside them, the calibration row
shared with the projection factors, the noise rows, the packed values -- and built the identical symbolic analysis, the repeated-key
lists included.  Graph: smart_rig_mixed.  (tests/cpp/test_shim_extractor_smart_rig.cpp also checks what the shim refuses.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402
from tests import smart_rig_support as S  # noqa: E402

EXE = os.path.join(ROOT, "tests", "_build", "test_shim_extractor_smart_rig")

_CHILD = r'''
import ctypes, json
import numpy as np
from tools import host_profile as HP
from gtsam_amd import lib as L
from tests import smart_rig_support as S
stub = ctypes.CDLL(HP.STUB)
stub.hipstub_h2d_record.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ulonglong)]
def records(p, v0):
    stub.hipstub_reset()
    g = L.DeviceGraph(p); g.set_values(np.ascontiguousarray(v0, np.float64))
    n = ctypes.c_longlong(); h = ctypes.c_ulonglong(); out = []
    for i in range(stub.hipstub_h2d_count()):
        stub.hipstub_h2d_record(i, ctypes.byref(n), ctypes.byref(h)); out.append("%d:%d" % (n.value, h.value))
    g.close(); return out
_, p, v0 = S.load("smart_rig_mixed")
print("RESULT " + json.dumps([records(p, v0)]))
'''


def test_cpp_and_python_extractors_hand_the_library_identical_smart_rig_tables(tmp_path):
    if not (os.path.exists(EXE) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so"))):
        pytest.skip("shim extractor test / oracle/_ref not built")
    stub = HP.build_stub()
    _, p, v0 = S.load("smart_rig_mixed")
    dump = str(tmp_path / "smart_rig_mixed.txt")
    S.write_problem_text(dump, p, v0)
    env = dict(os.environ); env["LD_PRELOAD"] = stub
    r = subprocess.run([EXE, dump], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    cpp = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
    # the same tables for any number of extraction threads (chunks of 7 factors: the cuts fall inside the smart run, so the rig's
    # cameras, the shared sensor row and the calibration rows are met again in every chunk)
    env_mt = dict(env); env_mt["GTG_HOST_THREADS"] = "5"; env_mt["GTG_EXTRACT_GRAIN"] = "7"
    r_mt = subprocess.run([EXE, dump], env=env_mt, capture_output=True, text=True, timeout=300)
    assert r_mt.returncode == 0 and "ALL PASSED" in r_mt.stdout, r_mt.stdout[-2000:] + r_mt.stderr[-2000:]
    assert [sorted(ln.split()[2:]) for ln in r_mt.stdout.splitlines() if ln.startswith("CASE ")] == [sorted(c) for c in cpp]
    py = HP.run_snippet(_CHILD)
    assert len(cpp) == len(py) == 1
    assert len(cpp[0]) > 30
    assert sorted(cpp[0]) == sorted(py[0])
