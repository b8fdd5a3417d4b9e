"""The C++ shim's extractor on graphs with BearingRangeFactor / RangeFactor / BearingFactor <Pose3, Point3> against the Python mirror's,
on the CPU: both run under tools/hipstub, which hashes every host-to-device copy (tests/test_shim_extractor_cpu.py explains the
method).  Equal records: the library was handed identical tables -- the sam table with its kinds and measurements, the shared noise
rows, the packed values -- and built the identical symbolic analysis.  Graphs: sam3d_mixed and sam3d_slam.

The fixtures hold the bearings as fixed points of Unit3's normalising constructor where there is one (tests/golden/make_golden_sam3d.py);
the few that alternate between two neighbouring doubles would reach the library one ulp off, so the dumps are written from a
Problem whose bearings went through the C++ test's own constructor once more: tests/_build/test_shim_extractor_sam prints, for
every case, the sam_z it extracted, and the Python side uploads exactly those."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402
from tests import sam_support as SS  # noqa: E402

EXE = os.path.join(ROOT, "tests", "_build", "test_shim_extractor_sam")

_CHILD = r'''
import ctypes, json, os
import numpy as np
from tools import host_profile as HP
from gtsam_amd import lib as L
from tests import sam_support as SS
stub = ctypes.CDLL(HP.STUB)
stub.hipstub_h2d_record.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ulonglong)]
held = json.load(open(os.environ["SAM_HELD_Z"]))
def records(p, v0, z):
    p.sam_z = np.array([float.fromhex(x) for x in z])
    stub.hipstub_reset()
    g = L.DeviceGraph(p); g.set_values(np.ascontiguousarray(v0, np.float64))
    n = ctypes.c_longlong(); h = ctypes.c_ulonglong(); out = []
    for i in range(stub.hipstub_h2d_count()):
        stub.hipstub_h2d_record(i, ctypes.byref(n), ctypes.byref(h)); out.append("%d:%d" % (n.value, h.value))
    g.close(); return out
print("RESULT " + json.dumps([records(p, v0, z) for (p, v0), z in zip(SS.extractor_cases(), held)]))
'''


def test_cpp_and_python_extractors_hand_the_library_identical_sam_tables(tmp_path):
    if not (os.path.exists(EXE) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so"))):
        pytest.skip("shim extractor test / oracle/_ref not built")
    stub = HP.build_stub()
    dumps = []
    for i, (p, v0) in enumerate(SS.extractor_cases()):
        dumps.append(str(tmp_path / f"case{i}.txt"))
        SS.write_problem_text(dumps[-1], p, v0)
    env = dict(os.environ); env["LD_PRELOAD"] = stub
    r = subprocess.run([EXE] + dumps, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    cpp = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
    # what the reference's factors hold for the measurements: the fixture's doubles, a bearing at most one ulp from them
    held = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("SAMZ ")]
    for (p, _), z in zip(SS.extractor_cases(), held):
        z = np.array([float.fromhex(x) for x in z])
        assert z.size == p.sam_z.size and np.abs(z - p.sam_z).max() <= np.finfo(float).eps
        assert np.array_equal(z.reshape(-1, 4)[:, 3], p.sam_z.reshape(-1, 4)[:, 3])
        assert np.mean(z == p.sam_z) >= 0.99
    # the same tables for any number of extraction threads (chunks of 7 factors: the cuts fall inside the sam run)
    env_mt = dict(env); env_mt["GTG_HOST_THREADS"] = "5"; env_mt["GTG_EXTRACT_GRAIN"] = "7"
    r_mt = subprocess.run([EXE] + dumps, env=env_mt, capture_output=True, text=True, timeout=300)
    assert r_mt.returncode == 0 and "ALL PASSED" in r_mt.stdout, r_mt.stdout[-2000:] + r_mt.stderr[-2000:]
    assert [sorted(ln.split()[2:]) for ln in r_mt.stdout.splitlines() if ln.startswith("CASE ")] == [sorted(c) for c in cpp]
    held_path = str(tmp_path / "held.json")
    with open(held_path, "w") as f:
        json.dump(held, f)
    py = HP.run_snippet(_CHILD, env_extra={"SAM_HELD_Z": held_path})
    assert len(cpp) == len(py) == 2
    for a, b in zip(cpp, py):
        assert len(a) > 30
        assert sorted(a) == sorted(b)
