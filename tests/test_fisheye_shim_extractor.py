"""The C++ shim's extractor on graphs with GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> against the Python mirror's, on the CPU:
both run under tools/hipstub, which hashes every host-to-device copy (tests/test_shim_extractor_cpu.py explains the method).  Equal
records: the library was handed identical tables -- the projection table, the calibration table with the fisheye coefficients in its
distortion rows, the model of every calib row, the shared sensor and noise rows, the packed values -- and built the identical symbolic
analysis.  Graphs: fisheye_mixed (four calibrations of three classes) and the FisheyeExample graph (fisheye_support.extractor_cases)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402
from tests import fisheye_support as FS  # noqa: E402

EXE = os.path.join(ROOT, "tests", "_build", "test_shim_extractor_fisheye")

_CHILD = r'''
import ctypes, json
import numpy as np
from tools import host_profile as HP
from gtsam_amd import lib as L
from tests import fisheye_support as FS
stub = ctypes.CDLL(HP.STUB)
stub.hipstub_h2d_record.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ulonglong)]
def records(p, v0):
    stub.hipstub_reset()
    g = L.DeviceGraph(p); g.set_values(np.ascontiguousarray(v0, np.float64))
    n = ctypes.c_longlong(); h = ctypes.c_ulonglong(); out = []
    for i in range(stub.hipstub_h2d_count()):
        stub.hipstub_h2d_record(i, ctypes.byref(n), ctypes.byref(h)); out.append("%d:%d" % (n.value, h.value))
    g.close(); return out
print("RESULT " + json.dumps([records(p, v0) for p, v0 in FS.extractor_cases()]))
'''


def test_cpp_and_python_extractors_hand_the_library_identical_fisheye_tables(tmp_path):
    if not (os.path.exists(EXE) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so"))):
        pytest.skip("shim extractor test / oracle/_ref not built")
    stub = HP.build_stub()
    dumps = []
    for i, (p, v0) in enumerate(FS.extractor_cases()):
        dumps.append(str(tmp_path / f"case{i}.txt"))
        FS.write_problem_text(dumps[-1], p, v0)
    env = dict(os.environ); env["LD_PRELOAD"] = stub
    r = subprocess.run([EXE] + dumps, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    cpp = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
    # the same tables for any number of extraction threads (chunks of 7 factors: the cuts fall between factors of different calibrations)
    env_mt = dict(env); env_mt["GTG_HOST_THREADS"] = "5"; env_mt["GTG_EXTRACT_GRAIN"] = "7"
    r_mt = subprocess.run([EXE] + dumps, env=env_mt, capture_output=True, text=True, timeout=300)
    assert r_mt.returncode == 0 and "ALL PASSED" in r_mt.stdout, r_mt.stdout[-2000:] + r_mt.stderr[-2000:]
    assert [sorted(ln.split()[2:]) for ln in r_mt.stdout.splitlines() if ln.startswith("CASE ")] == [sorted(c) for c in cpp]
    py = HP.run_snippet(_CHILD)
    assert len(cpp) == len(py) == 2
    for a, b in zip(cpp, py):
        assert len(a) > 20
        assert sorted(a) == sorted(b)
