"""GPU: graphs with PoseTranslationPrior / PoseRotationPrior <Pose3 | Pose2> through the C++ drop-in
(gtsam_amd::GpuLevenbergMarquardtOptimizer) against the reference's own optimizer on the same NonlinearFactorGraph / Values, built
with the reference's own factor classes -- tests/cpp/test_gpu_lm_pose_partial.cpp, prebuilt in the build container (needs GTSAM
headers) together with oracle/_ref: linearize() per factor, the records of the shim's tables against those of the Python extractor's
tables for the same graph (recorded here, on the same device), the accept / reject sequence iterate() by iterate(), optimize() (the
same iteration counts, final error to 1e-9, values to 1e-5), and RangeFactor<Pose3, Pose3> still refused.  Graphs: the three fixtures
of tests/golden/make_golden_pose_partial.py, handed over as text dumps."""
import os
import subprocess

import pytest

from tests import pose_partial_support as PS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_shim_matches_reference_optimizer_on_partial_pose_prior_graphs(tmp_path):
    exe = os.path.join(ROOT, "tests", "_build", "test_gpu_lm_pose_partial")
    if not os.path.exists(exe) or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so")):
        pytest.skip("prebuilt shim test / oracle/_ref did not travel")
    from gtsam_amd import lib
    dumps = []
    for name in PS.FIXTURES:
        g = PS.fixture(name)
        p = PS.problem_of(g)
        dev = lib.DeviceGraph(p)
        dev.set_values(g["values0"])
        dev.linearize()
        jac6 = dev.jacobians(6)
        dev.close()
        assert PS.rel(jac6, g["jac6"]) <= 1e-12
        dumps.append(str(tmp_path / (name + ".txt")))
        PS.write_problem_text(dumps[-1], p, g["values0"], jac6=jac6)
    r = subprocess.run([exe] + dumps, capture_output=True, text=True, timeout=600)
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")))
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout
