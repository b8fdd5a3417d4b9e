"""GPU: graphs whose smart factors have TriangulationParameters::useLOST set through the C++ drop-in
(gtsam_amd::GpuLevenbergMarquardtOptimizer) against the reference's own optimizer on the same NonlinearFactorGraph / Values --
tests/cpp/test_gpu_smart_lost_gtsam.cpp, prebuilt in the build container (needs GTSAM headers) together with oracle/_ref: optimize() of
both, same iteration counts, values within 1e-5.  Graphs: one of each smart factor kind (smart_lost_cam, smart_lost_pose,
smart_lost_rig), handed over as text dumps."""
import os
import subprocess

import pytest

from tests import smart_lost_support as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_shim_matches_reference_optimizer_on_lost_graphs_of_each_kind(tmp_path):
    exe = os.path.join(ROOT, "tests", "_build", "test_gpu_smart_lost_gtsam")
    if not os.path.exists(exe) or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtsam_ref.so")):
        pytest.skip("prebuilt shim test / oracle/_ref did not travel")
    dumps = []
    for name in ("smart_lost_cam", "smart_lost_pose", "smart_lost_rig"):
        _, p, v0 = S.load(name)
        dumps.append(str(tmp_path / (name + ".txt")))
        S.write_problem_text(dumps[-1], p, v0)
    r = subprocess.run([exe] + dumps, capture_output=True, text=True, timeout=600)
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")))
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout
