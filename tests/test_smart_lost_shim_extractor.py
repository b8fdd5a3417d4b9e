"""The C++ shim's extractor on graphs whose smart factors have TriangulationParameters::useLOST set, against the Python mirror's, on the
CPU: both run under tools/hipstub, which hashes every host-to-device copy (tests/test_shim_extractor_cpu.py explains the method).  Equal
records: the library was handed identical tables -- slot 7 of every smart_params row (the LOST sigma; 0.0 on the DLT factors of the mixed
graph; 0.4 from the triangulation noise model of the rig graph) among them -- for a camera-type, a pose-type and a rig-type graph.
tests/cpp/test_shim_extractor_smart_lost.cpp also checks that useLOST is accepted and what the shim still refuses beside it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402
from tests import smart_lost_support as S  # noqa: E402

EXE = os.path.join(ROOT, "tests", "_build", "test_shim_extractor_smart_lost")
GRAPHS = ("smart_lost_cam", "smart_lost_pose", "smart_lost_rig")

_CHILD = r'''
import ctypes, json
import numpy as np
from tools import host_profile as HP
from gtsam_amd import lib as L
from tests import smart_lost_support as S
stub = ctypes.CDLL(HP.STUB)
stub.hipstub_h2d_record.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ulonglong)]
def records(p, v0):
    stub.hipstub_reset()
    g = L.DeviceGraph(p); g.set_values(np.ascontiguousarray(v0, np.float64))
    n = ctypes.c_longlong(); h = ctypes.c_ulonglong(); out = []
    for i in range(stub.hipstub_h2d_count()):
        stub.hipstub_h2d_record(i, ctypes.byref(n), ctypes.byref(h)); out.append("%d:%d" % (n.value, h.value))
    g.close(); return out
print("RESULT " + json.dumps([records(*S.load(name)[1:]) for name in ("smart_lost_cam", "smart_lost_pose", "smart_lost_rig")]))
'''


def test_cpp_and_python_extractors_hand_the_library_identical_lost_tables(tmp_path):
    if not (os.path.exists(EXE) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so"))):
        pytest.skip("shim extractor test / oracle/_ref not built")
    stub = HP.build_stub()
    dumps = []
    for name in GRAPHS:
        _, p, v0 = S.load(name)
        dumps.append(str(tmp_path / (name + ".txt")))
        S.write_problem_text(dumps[-1], p, v0)
    env = dict(os.environ); env["LD_PRELOAD"] = stub
    r = subprocess.run([EXE] + dumps, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    cpp = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
    py = HP.run_snippet(_CHILD)
    assert len(cpp) == len(py) == len(GRAPHS)
    for a, b in zip(cpp, py):
        assert len(a) > 20
        assert sorted(a) == sorted(b)
