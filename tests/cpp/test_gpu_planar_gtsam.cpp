// tests/cpp/test_gpu_planar_gtsam.cpp -- planar landmark SLAM (BearingRangeFactor / RangeFactor / BearingFactor <Pose2, Point2>) through the
// drop-in, against the reference's optimizer on the same NonlinearFactorGraph / Values built with the reference's own factor classes
// (the protocol of tests/cpp/test_gpu_sam_gtsam.cpp, restated for these graphs): gpu.linearize() against graph.linearize() per factor
// (<= 1e-9; a landmark block has TWO columns: the padding of the C ABI does not reach the caller); gpu.solve() of the reference's own
// damped system against cpu.solve(), both damping modes, to max(1e-7, 10 x the reference's own difference under a reversed ordering),
// every landmark's entry a 2-vector; optimize() of both optimizers: same iteration counts, final error to 1e-9 relative, values to 1e-5.
// Graphs: text dumps of tests/golden/planar_slam.npz and planar_mixed.npz (argv; written by tests/test_gpu_planar_shim.py).
#include <GpuLevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/internal/LevenbergMarquardtState.h>

#include <algorithm>
#include <cstdio>

#include "planar_graph_text.h"

using namespace gtsam;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static double valuesDiff(const Values& a, const Values& b) {
  double worst = 0;
  for (const auto& kv : a) worst = std::max(worst, kv.value.localCoordinates_(b.at(kv.key)).cwiseAbs().maxCoeff());
  return worst;
}

static void abTest(const char* name, const planar_text::Graph& g, const LevenbergMarquardtParams& params) {
  const NonlinearFactorGraph& graph = g.graph; const Values& initial = g.initial;
  gtsam_amd::GpuLevenbergMarquardtOptimizer gpu(graph, initial, params);
  LevenbergMarquardtOptimizer cpu(graph, initial, params);
  const GaussianFactorGraph::shared_ptr lc = graph.linearize(initial), lg = gpu.linearize();
  EXPECT(lc->size() == lg->size(), "%s linearize(): %zu vs %zu factors", name, lc->size(), lg->size());
  double worstJ = 0; size_t planarRows = 0;
  for (size_t i = 0; i < std::min(lc->size(), lg->size()); i++) {
    // (an ExpressionFactor sorts its keys: the reference's blocks are brought into the order of the factor's own keys, pose first)
    const auto jc = std::dynamic_pointer_cast<JacobianFactor>(lc->at(i)), jg = std::dynamic_pointer_cast<JacobianFactor>(lg->at(i));
    if (!jc || !jg || jc->size() != jg->size() || jc->rows() != jg->rows()) { EXPECT(false, "%s linearize(): factor %zu shape", name, i); continue; }
    double scale = 1.0, worst = 0.0;
    bool shape = true;
    for (Key k : jg->keys()) {
      const auto ic = jc->find(k);
      if (ic == jc->end()) { shape = false; break; }
      const Matrix a = jc->getA(ic), b = jg->getA(jg->find(k));
      if (a.cols() != b.cols()) { shape = false; break; }
      scale = std::max(scale, a.cwiseAbs().maxCoeff()); worst = std::max(worst, (a - b).cwiseAbs().maxCoeff());
    }
    if (!shape) { EXPECT(false, "%s linearize(): factor %zu keys / block widths", name, i); continue; }
    scale = std::max(scale, jc->getb().cwiseAbs().maxCoeff()); worst = std::max(worst, (jc->getb() - jg->getb()).cwiseAbs().maxCoeff());
    if (i < g.n_sam2 && (int)jg->rows() == (g.kind[i] == 0 ? 2 : 1) && jg->getA(jg->begin()).cols() == 3 && jg->getA(jg->begin() + 1).cols() == 2) planarRows++;
    worstJ = std::max(worstJ, worst / scale);
  }
  EXPECT(planarRows == g.n_sam2, "%s linearize(): %zu of %zu planar factors have their kind's rows x (3 + 2 + 1)", name, planarRows, g.n_sam2);
  EXPECT(worstJ <= 1e-9, "%s linearize(): Jacobians differ by %.3g", name, worstJ);
  double worstD = 0, self = 0, worstCost = 0;
  for (int diag = 0; diag < 2; diag++) {
    const double lambda = 1e-2;
    internal::LevenbergMarquardtState st(initial, graph.error(initial), lambda, 10.0);
    GaussianFactorGraph damped;
    if (diag) {
      VectorValues sq = lc->hessianDiagonal();
      for (auto& kv : sq) kv.second = kv.second.cwiseMax(params.minDiagonal).cwiseMin(params.maxDiagonal).cwiseSqrt();
      damped = st.buildDampedSystem(*lc, sq);
    } else {
      damped = st.buildDampedSystem(*lc);
    }
    LevenbergMarquardtParams pd = params; pd.diagonalDamping = diag;
    const VectorValues xc = cpu.solve(damped, pd), xg = gpu.solve(damped, pd);
    LevenbergMarquardtParams po = pd;
    Ordering other = pd.ordering ? *pd.ordering : Ordering::Colamd(damped);
    std::reverse(other.begin(), other.end());
    po.ordering = other;
    const VectorValues xo = cpu.solve(damped, po);
    double scale = 0; for (const auto& kv : xc) scale = std::max(scale, kv.second.cwiseAbs().maxCoeff());
    for (const auto& kv : xc) {
      if (xg.at(kv.first).size() != kv.second.size()) { EXPECT(false, "%s solve(): entry of key %zu has %d numbers, the reference's %d", name, (size_t)kv.first, (int)xg.at(kv.first).size(), (int)kv.second.size()); continue; }
      worstD = std::max(worstD, (kv.second - xg.at(kv.first)).cwiseAbs().maxCoeff() / std::max(scale, 1e-300));
      self = std::max(self, (kv.second - xo.at(kv.first)).cwiseAbs().maxCoeff() / std::max(scale, 1e-300));
    }
    worstCost = std::max(worstCost, std::abs(damped.error(xg) - damped.error(xc)) / std::max(std::abs(damped.error(xc)), 1e-300));
  }
  EXPECT(worstD <= std::max(1e-7, 10.0 * self), "%s solve(): delta differs by %.3g (the reference from itself under another ordering: %.3g)", name, worstD, self);
  EXPECT(worstCost <= 1e-8, "%s solve(): quadratic cost at the device's delta differs by %.3g", name, worstCost);
  std::printf("%-28s A/B: linearize() %.2g, solve() %.2g (reference vs itself %.2g, cost %.2g)\n", name, worstJ, worstD, self, worstCost);
}

static void compare(const char* name, const planar_text::Graph& g, const LevenbergMarquardtParams& params) {
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
  EXPECT(std::abs(cpu.error() - gpu.error()) <= 1e-9 * std::abs(cpu.error()), "%s final error %.15g vs %.15g", name, cpu.error(), gpu.error());
  EXPECT(std::abs(graph.error(rg) - gpu.error()) <= 1e-9 * std::abs(gpu.error()) + 1e-12, "%s values()/error() out of sync", name);
  EXPECT(valuesDiff(rc, rg) <= 1e-5, "%s optimised values differ by %.3g", name, valuesDiff(rc, rg));
  size_t points = 0;
  for (const auto& kv : rg) if (dynamic_cast<const GenericValue<Point2>*>(&kv.value)) points++;
  EXPECT(points > 0 && rg.size() == initial.size(), "%s the result holds %zu Point2 values", name, points);
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: test_gpu_planar_gtsam <graph dump> ...\n"); return 2; }
  for (int a = 1; a < argc; a++) {
    const planar_text::Graph g = planar_text::read(argv[a]);
    const std::string name = std::string(argv[a]).substr(std::string(argv[a]).find_last_of('/') + 1);
    std::printf("%s: %zu factors (%zu planar bearing / range), %zu variables\n", name.c_str(), g.graph.size(), g.n_sam2, g.initial.size());
    const LevenbergMarquardtParams params;   // defaults: COLAMD ordering, multifrontal Cholesky
    abTest(name.c_str(), g, params);
    compare((name + " direct").c_str(), g, params);
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
