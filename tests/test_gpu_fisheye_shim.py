"""GPU: graphs with GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> through the C++ drop-in (gtsam_amd::GpuLevenbergMarquardtOptimizer)
against the reference's own optimizer on the same NonlinearFactorGraph / Values, built with the reference's own factor classes --
tests/cpp/test_gpu_fisheye_gtsam.cpp, prebuilt in the build container (needs GTSAM headers) together with oracle/_ref: optimize() of
both with default parameters: identical iteration counts, the final error to 1e-9, values to 1e-5.  Graphs: the FisheyeExample graph
and fisheye_mixed (two Cal3Fisheye, a Cal3_S2 and a Cal3DS2 in one graph), handed over as text dumps."""
import os
import subprocess

import pytest

from tests import fisheye_support as FS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_shim_matches_reference_optimizer_on_fisheye_graphs(tmp_path):
    exe = os.path.join(ROOT, "tests", "_build", "test_gpu_fisheye_gtsam")
    if not os.path.exists(exe) or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so")):
        pytest.skip("prebuilt shim test / oracle/_ref did not travel")
    dumps = []
    for name in ("fisheye_example", "fisheye_mixed"):
        g = FS.fixture(name)
        dumps.append(str(tmp_path / (name + ".txt")))
        FS.write_problem_text(dumps[-1], FS.problem_of(g), g["values0"])
    r = subprocess.run([exe] + dumps, capture_output=True, text=True, timeout=600)
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")))
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout
