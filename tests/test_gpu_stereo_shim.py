"""GPU: graphs with GenericStereoFactor<Pose3, Point3> through the C++ drop-in (gtsam_amd::GpuLevenbergMarquardtOptimizer) against the
reference's own optimizer on the same NonlinearFactorGraph / Values -- tests/cpp/test_gpu_stereo_gtsam.cpp, prebuilt in the build
container (needs GTSAM headers) together with oracle/_ref: linearize() per factor, solve() of the reference's damped system in
both damping modes, optimize() with the direct solver and with a tightly converged block-Jacobi PCG.  Graphs: stereo_mixed and
the data of examples/StereoVOExample_large.cpp, handed over as text dumps."""
import os
import subprocess

import pytest

from tests import stereo_support as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_shim_matches_reference_optimizer_on_stereo_graphs(tmp_path):
    exe = os.path.join(ROOT, "tests", "_build", "test_gpu_stereo_gtsam")
    if not os.path.exists(exe) or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so")):
        pytest.skip("prebuilt shim test / oracle/_ref did not travel")
    g = S.fixture("stereo_mixed")
    dumps = [str(tmp_path / "stereo_mixed.txt"), str(tmp_path / "stereo_vo_large.txt")]
    S.write_problem_text(dumps[0], S.problem_of(g), g["values0"])
    S.write_problem_text(dumps[1], *S.vo_problem())
    r = subprocess.run([exe] + dumps, capture_output=True, text=True, timeout=600)
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")))
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout
