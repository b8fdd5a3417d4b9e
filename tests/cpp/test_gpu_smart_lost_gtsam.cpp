// tests/cpp/test_gpu_smart_lost_gtsam.cpp -- smart factors with TriangulationParameters::useLOST through the drop-in, against the reference's
// optimizer on the same NonlinearFactorGraph / Values (the protocol of compare() in tests/cpp/test_gpu_smart_rig_gtsam.cpp): optimize() of
// both optimizers -- same iteration counts, errors to 1e-6 relative, values to 1e-5.  Graphs: text dumps of the smart_lost_* fixtures, one
// of each smart factor kind (argv; written by tests/test_gpu_smart_lost_shim.py).
#include <GpuLevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>

#include <algorithm>
#include <cstdio>

#include "smart_lost_graph_text.h"

using namespace gtsam;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static double valuesDiff(const Values& a, const Values& b) {
  double worst = 0;
  for (const auto& kv : a) worst = std::max(worst, kv.value.localCoordinates_(b.at(kv.key)).cwiseAbs().maxCoeff());
  return worst;
}

// (each optimizer gets a graph of its own from the dump: a smart factor caches its triangulation inside the factor object)
static void compare(const char* name, const char* path, const LevenbergMarquardtParams& params) {
  const smart_lost_text::Graph gc = smart_lost_text::read(path), gg = smart_lost_text::read(path), ge = smart_lost_text::read(path);
  LevenbergMarquardtOptimizer cpu(gc.graph, gc.initial, params);
  const Values rc = cpu.optimize();
  gtsam_amd::GpuLevenbergMarquardtOptimizer gpu(gg.graph, gg.initial, params);
  const double e0 = gpu.error();
  const Values rg = gpu.optimize();
  std::printf("%-34s init %.9g | cpu: it %zu inner %d err %.12g lambda %.3g | gpu: it %zu inner %d err %.12g lambda %.3g\n", name, e0, cpu.iterations(),
              cpu.getInnerIterations(), cpu.error(), cpu.lambda(), gpu.iterations(), gpu.getInnerIterations(), gpu.error(), gpu.lambda());
  const double e_ref = ge.graph.error(ge.initial);
  EXPECT(std::abs(e0 - e_ref) <= 1e-9 * std::abs(e0), "%s initial error %.15g vs %.15g", name, e0, e_ref);
  EXPECT(cpu.iterations() == gpu.iterations(), "%s iterations %zu vs %zu", name, cpu.iterations(), gpu.iterations());
  EXPECT(cpu.getInnerIterations() == gpu.getInnerIterations(), "%s inner iterations %d vs %d", name, cpu.getInnerIterations(), gpu.getInnerIterations());
  EXPECT(std::abs(cpu.error() - gpu.error()) <= 1e-6 * std::abs(cpu.error()) + 1e-12, "%s final error %.15g vs %.15g", name, cpu.error(), gpu.error());
  EXPECT(std::abs(ge.graph.error(rg) - gpu.error()) <= 1e-9 * std::abs(gpu.error()) + 1e-12, "%s values()/error() out of sync", name);
  EXPECT(valuesDiff(rc, rg) <= 1e-5, "%s optimised values differ by %.3g", name, valuesDiff(rc, rg));
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: test_gpu_smart_lost_gtsam <graph dump> ...\n"); return 2; }
  for (int a = 1; a < argc; a++) {
    const smart_lost_text::Graph g = smart_lost_text::read(argv[a]);
    const std::string name = std::string(argv[a]).substr(std::string(argv[a]).find_last_of('/') + 1);
    std::printf("%s: %zu factors (%zu smart: %zu camera-type, %zu rig-type; %zu with useLOST), %zu variables\n", name.c_str(), g.graph.size(), g.n_smart,
                g.n_camera, g.n_rig, g.n_lost, g.initial.size());
    EXPECT(g.n_lost > 0, "%s has no LOST factor", name.c_str());
    compare((name + " direct").c_str(), argv[a], LevenbergMarquardtParams());   // defaults: COLAMD ordering, multifrontal Cholesky
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
