"""The C++ shim's extractor on planar landmark SLAM graphs against the Python mirror's, on the CPU: both run under tools/hipstub, which
hashes every host-to-device copy (tests/test_shim_extractor_cpu.py explains the method).  Equal records: the library was handed
identical tables -- the sam2 table with its kinds and measurements, the shared noise rows, the packed values with every Point2 padded to
(x, y, 0), compared by the C++ test itself -- and built the identical symbolic analysis.  Graphs: planar_mixed and planar_slam.

The fixtures hold every measured bearing as the reference's Rot2::fromCosSin returned it; the dump's (c, s) go through it once more in
the C++ test.  tests/_build/test_shim_extractor_planar prints, for every case, the sam2_z it extracted, and the Python side uploads
exactly those (they are asserted to be the fixture's doubles to one ulp, nearly all bit for bit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402
from tests import planar_support as PL  # noqa: E402

EXE = os.path.join(ROOT, "tests", "_build", "test_shim_extractor_planar")

_CHILD = r'''
import ctypes, json, os
import numpy as np
from tools import host_profile as HP
from gtsam_amd import lib as L
from tests import planar_support as PL
stub = ctypes.CDLL(HP.STUB)
stub.hipstub_h2d_record.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ulonglong)]
held = json.load(open(os.environ["PLANAR_HELD_Z"]))
def records(name, z):
    g = PL.fixture(name); p = PL.problem_of(g)
    p.sam2_z = np.array([float.fromhex(x) for x in z])
    stub.hipstub_reset()
    d = L.DeviceGraph(p); d.set_values(np.ascontiguousarray(g["values0"], np.float64))
    n = ctypes.c_longlong(); h = ctypes.c_ulonglong(); out = []
    for i in range(stub.hipstub_h2d_count()):
        stub.hipstub_h2d_record(i, ctypes.byref(n), ctypes.byref(h)); out.append("%d:%d" % (n.value, h.value))
    d.close(); return out
print("RESULT " + json.dumps([records(name, z) for name, z in zip(PL.FIXTURES, held)]))
'''


def test_cpp_and_python_extractors_hand_the_library_identical_planar_tables(tmp_path):
    if not (os.path.exists(EXE) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so"))):
        pytest.skip("shim extractor test / oracle/_ref not built")
    stub = HP.build_stub()
    dumps = []
    for name in PL.FIXTURES:
        g = PL.fixture(name)
        dumps.append(str(tmp_path / f"{name}.txt"))
        PL.write_problem_text(dumps[-1], PL.problem_of(g), g["values0"])
    env = dict(os.environ); env["LD_PRELOAD"] = stub
    r = subprocess.run([EXE] + dumps, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    cpp = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
    held = [ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("SAM2Z ")]
    for name, z in zip(PL.FIXTURES, held):
        p = PL.problem_of(PL.fixture(name))
        z = np.array([float.fromhex(x) for x in z])
        assert z.size == p.sam2_z.size and np.abs(z - p.sam2_z).max() <= np.finfo(float).eps
        assert np.array_equal(z.reshape(-1, 3)[:, 2], p.sam2_z.reshape(-1, 3)[:, 2])
        assert np.mean(z == p.sam2_z) >= 0.99
    # the same tables for any number of extraction threads (chunks of 7 factors: the cuts fall inside the planar run)
    env_mt = dict(env); env_mt["GTG_HOST_THREADS"] = "5"; env_mt["GTG_EXTRACT_GRAIN"] = "7"
    r_mt = subprocess.run([EXE] + dumps, env=env_mt, capture_output=True, text=True, timeout=300)
    assert r_mt.returncode == 0 and "ALL PASSED" in r_mt.stdout, r_mt.stdout[-2000:] + r_mt.stderr[-2000:]
    assert [sorted(ln.split()[2:]) for ln in r_mt.stdout.splitlines() if ln.startswith("CASE ")] == [sorted(c) for c in cpp]
    held_path = str(tmp_path / "held.json")
    with open(held_path, "w") as f:
        json.dump(held, f)
    py = HP.run_snippet(_CHILD, env_extra={"PLANAR_HELD_Z": held_path})
    assert len(cpp) == len(py) == 2
    for name, a, b in zip(PL.FIXTURES, cpp, py):
        # every upload but the packed values: a Pose2 of the reference holds (cos, sin), and the theta() the shim packs is atan2 of them --
        # the dump's angle to an ulp, not bit for bit (the C++ test has compared the values themselves to 1e-12)
        # ... and the between measurements, Pose2 objects as well
        g = PL.fixture(name)
        angles = ("%d:" % (8 * g["values0"].size), "%d:" % (8 * g["p_between_z"].size))
        rest_a, rest_b = [x for x in a if not x.startswith(angles)], [x for x in b if not x.startswith(angles)]
        assert len(rest_a) > 20 and len(a) - len(rest_a) == len(b) - len(rest_b) == 2
        assert sorted(rest_a) == sorted(rest_b)
