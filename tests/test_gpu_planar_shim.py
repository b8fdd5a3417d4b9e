"""GPU: planar landmark SLAM graphs (BearingRangeFactor / RangeFactor / BearingFactor <Pose2, Point2>) through the C++ drop-in
(gtsam_amd::GpuLevenbergMarquardtOptimizer) against the reference's own optimizer on the same NonlinearFactorGraph / Values, built
with the reference's own factor classes -- tests/cpp/test_gpu_planar_gtsam.cpp, prebuilt in the build container (needs GTSAM headers)
together with oracle/_ref: linearize() per factor (the landmark blocks two columns wide), solve() of the reference's damped system in
both damping modes through the virtuals (a landmark's entry a 2-vector), optimize(): identical iteration counts, the final error to
1e-9, values to 1e-5.  Graphs: planar_slam and planar_mixed, handed over as text dumps."""
import os
import subprocess

import pytest

from tests import planar_support as PL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_shim_matches_reference_optimizer_on_planar_graphs(tmp_path):
    exe = os.path.join(ROOT, "tests", "_build", "test_gpu_planar_gtsam")
    if not os.path.exists(exe) or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so")):
        pytest.skip("prebuilt shim test / oracle/_ref did not travel")
    dumps = []
    for name in ("planar_slam", "planar_mixed"):
        g = PL.fixture(name)
        dumps.append(str(tmp_path / (name + ".txt")))
        PL.write_problem_text(dumps[-1], PL.problem_of(g), g["values0"])
    r = subprocess.run([exe] + dumps, capture_output=True, text=True, timeout=600)
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")))
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout
