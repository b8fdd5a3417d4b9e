// tests/cpp/test_gpu_fisheye_gtsam.cpp -- GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> through the drop-in, against the reference's
// optimizer on the same NonlinearFactorGraph / Values built with the reference's own factor classes: optimize() of both optimizers with
// default LevenbergMarquardtParams -- same iteration counts, final error to 1e-9 relative, values to 1e-5 (the numbers of
// tests/cpp/test_gpu_lm_pose_partial.cpp).  A consistent scene (the FisheyeExample graph) ends at an error that is zero to the rounding
// of its residuals in either optimizer: there the two final errors must both lie below 1e-12 of the initial error instead.
// Graphs: text dumps of tests/golden/fisheye_example.npz and fisheye_mixed.npz (argv; written by tests/test_gpu_fisheye_shim.py).
#include <GpuLevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>

#include <algorithm>
#include <cstdio>

#include "fisheye_graph_text.h"

using namespace gtsam;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static double valuesDiff(const Values& a, const Values& b) {
  double worst = 0;
  for (const auto& kv : a) worst = std::max(worst, kv.value.localCoordinates_(b.at(kv.key)).cwiseAbs().maxCoeff());
  return worst;
}

static void compare(const char* name, const fisheye_text::Graph& g, const LevenbergMarquardtParams& params) {
  const NonlinearFactorGraph& graph = g.graph; const Values& initial = g.initial;
  LevenbergMarquardtOptimizer cpu(graph, initial, params);
  const Values rc = cpu.optimize();
  gtsam_amd::GpuLevenbergMarquardtOptimizer gpu(graph, initial, params);
  const double e0 = gpu.error();
  const Values rg = gpu.optimize();
  std::printf("%-28s init %.9g | cpu: it %zu inner %d err %.15g lambda %.3g | gpu: it %zu inner %d err %.15g lambda %.3g | values %.3g\n", name, e0, cpu.iterations(),
              cpu.getInnerIterations(), cpu.error(), cpu.lambda(), gpu.iterations(), gpu.getInnerIterations(), gpu.error(), gpu.lambda(), valuesDiff(rc, rg));
  EXPECT(std::abs(e0 - graph.error(initial)) <= 1e-9 * std::abs(e0), "%s initial error %.15g vs %.15g", name, e0, graph.error(initial));
  EXPECT(cpu.iterations() == gpu.iterations(), "%s iterations %zu vs %zu", name, cpu.iterations(), gpu.iterations());
  EXPECT(cpu.getInnerIterations() == gpu.getInnerIterations(), "%s inner iterations %d vs %d", name, cpu.getInnerIterations(), gpu.getInnerIterations());
  const bool zero = cpu.error() <= 1e-12 * e0;   // (a consistent scene: zero to the rounding of the residuals)
  EXPECT(zero ? gpu.error() <= 1e-12 * e0 : std::abs(cpu.error() - gpu.error()) <= 1e-9 * std::abs(cpu.error()), "%s final error %.15g vs %.15g", name, cpu.error(), gpu.error());
  EXPECT(std::abs(graph.error(rg) - gpu.error()) <= 1e-9 * std::abs(gpu.error()) + 1e-12, "%s values()/error() out of sync", name);
  EXPECT(valuesDiff(rc, rg) <= 1e-5, "%s optimised values differ by %.3g", name, valuesDiff(rc, rg));
  EXPECT(rg.size() == initial.size(), "%s the result holds %zu values", name, rg.size());
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: test_gpu_fisheye_gtsam <graph dump> ...\n"); return 2; }
  for (int a = 1; a < argc; a++) {
    const fisheye_text::Graph g = fisheye_text::read(argv[a]);
    const std::string name = std::string(argv[a]).substr(std::string(argv[a]).find_last_of('/') + 1);
    std::printf("%s: %zu factors (%zu projection, %zu of them fisheye), %zu variables\n", name.c_str(), g.graph.size(), g.n_proj, g.n_fisheye, g.initial.size());
    EXPECT(g.n_fisheye > 0, "%s has no fisheye factor", name.c_str());
    const LevenbergMarquardtParams params;   // defaults: COLAMD ordering, multifrontal Cholesky
    compare((name + " direct").c_str(), g, params);
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
