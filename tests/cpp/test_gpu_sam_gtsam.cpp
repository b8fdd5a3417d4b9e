// tests/cpp/test_gpu_sam_gtsam.cpp -- BearingRangeFactor / RangeFactor / BearingFactor <Pose3, Point3> through the drop-in, against the
// reference's optimizer on the same NonlinearFactorGraph / Values built with the reference's own factor classes (the protocol of
// tests/cpp/test_gpu_stereo_gtsam.cpp, restated for these graphs): gpu.linearize() against graph.linearize() per factor (<= 1e-9); gpu.solve() of the reference's own damped system
// against cpu.solve(), both damping modes, to max(1e-7, 10 x the reference's own difference under a reversed ordering); optimize()
// of both optimizers: same iteration counts, errors to 1e-6 relative, values to 1e-5; the same with NonlinearOptimizerParams::Iterative
// and a tightly converged block-Jacobi PCG.  Graphs: text dumps of tests/golden/sam3d_slam.npz and sam3d_mixed.npz (argv; written by
// tests/test_gpu_sam_shim.py).
#include <GpuLevenbergMarquardtOptimizer.h>
#include <gtsam/linear/PCGSolver.h>
#include <gtsam/linear/Preconditioner.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/internal/LevenbergMarquardtState.h>

#include <algorithm>
#include <cstdio>

#include "sam_graph_text.h"

using namespace gtsam;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static double valuesDiff(const Values& a, const Values& b) {
  double worst = 0;
  for (const auto& kv : a) worst = std::max(worst, kv.value.localCoordinates_(b.at(kv.key)).cwiseAbs().maxCoeff());
  return worst;
}

static LevenbergMarquardtParams iterativeParams(LevenbergMarquardtParams params) {
  auto pcg = std::make_shared<PCGSolverParameters>(std::make_shared<BlockJacobiPreconditionerParameters>());
  pcg->maxIterations = 5000; pcg->epsilon_rel = 1e-13; pcg->epsilon_abs = 1e-26;
  params.linearSolverType = NonlinearOptimizerParams::Iterative;
  params.iterativeParams = pcg;
  return params;
}

static void abTest(const char* name, const sam_text::Graph& g, const LevenbergMarquardtParams& params) {
  const NonlinearFactorGraph& graph = g.graph; const Values& initial = g.initial;
  gtsam_amd::GpuLevenbergMarquardtOptimizer gpu(graph, initial, params);
  LevenbergMarquardtOptimizer cpu(graph, initial, params);
  const GaussianFactorGraph::shared_ptr lc = graph.linearize(initial), lg = gpu.linearize();
  EXPECT(lc->size() == lg->size(), "%s linearize(): %zu vs %zu factors", name, lc->size(), lg->size());
  double worstJ = 0; size_t threeRows = 0, samRows = 0;
  for (size_t i = 0; i < std::min(lc->size(), lg->size()); i++) {
    const Matrix a = lc->at(i)->augmentedJacobian(), b = lg->at(i)->augmentedJacobian();
    if (a.rows() != b.rows() || a.cols() != b.cols() || lc->at(i)->keys() != lg->at(i)->keys()) { EXPECT(false, "%s linearize(): factor %zu shape / keys", name, i); continue; }
    if (i >= g.n_proj && i < g.n_proj + g.n_stereo && a.rows() == 3 && a.cols() == 10) threeRows++;
    if (i >= g.n_proj + g.n_stereo && i < g.n_proj + g.n_stereo + g.n_sam) {   // a sam factor has its kind's 3, 1 or 2 rows
      const int kind = g.sam_kind[i - g.n_proj - g.n_stereo];
      if (a.rows() == (kind == 0 ? 3 : kind == 1 ? 1 : 2) && a.cols() == 10) samRows++;
    }
    worstJ = std::max(worstJ, (a - b).cwiseAbs().maxCoeff() / std::max(1.0, a.cwiseAbs().maxCoeff()));
  }
  EXPECT(threeRows == g.n_stereo, "%s linearize(): %zu of %zu stereo factors are 3 x (6 + 3 + 1)", name, threeRows, g.n_stereo);
  EXPECT(samRows == g.n_sam, "%s linearize(): %zu of %zu bearing / range factors have their kind's rows x (6 + 3 + 1)", name, samRows, g.n_sam);
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
      worstD = std::max(worstD, (kv.second - xg.at(kv.first)).cwiseAbs().maxCoeff() / std::max(scale, 1e-300));
      self = std::max(self, (kv.second - xo.at(kv.first)).cwiseAbs().maxCoeff() / std::max(scale, 1e-300));
    }
    worstCost = std::max(worstCost, std::abs(damped.error(xg) - damped.error(xc)) / std::max(std::abs(damped.error(xc)), 1e-300));
  }
  EXPECT(worstD <= std::max(1e-7, 10.0 * self), "%s solve(): delta differs by %.3g (the reference from itself under another ordering: %.3g)", name, worstD, self);
  EXPECT(worstCost <= 1e-8, "%s solve(): quadratic cost at the device's delta differs by %.3g", name, worstCost);
  std::printf("%-28s A/B: linearize() %.2g, solve() %.2g (reference vs itself %.2g, cost %.2g)\n", name, worstJ, worstD, self, worstCost);
}

static void compare(const char* name, const sam_text::Graph& g, const LevenbergMarquardtParams& params) {
  const NonlinearFactorGraph& graph = g.graph; const Values& initial = g.initial;
  LevenbergMarquardtOptimizer cpu(graph, initial, params);
  const Values rc = cpu.optimize();
  gtsam_amd::GpuLevenbergMarquardtOptimizer gpu(graph, initial, params);
  const double e0 = gpu.error();
  const Values rg = gpu.optimize();
  std::printf("%-28s init %.9g | cpu: it %zu inner %d err %.12g lambda %.3g | gpu: it %zu inner %d err %.12g lambda %.3g\n", name, e0, cpu.iterations(),
              cpu.getInnerIterations(), cpu.error(), cpu.lambda(), gpu.iterations(), gpu.getInnerIterations(), gpu.error(), gpu.lambda());
  EXPECT(std::abs(e0 - graph.error(initial)) <= 1e-9 * std::abs(e0), "%s initial error %.15g vs %.15g", name, e0, graph.error(initial));
  EXPECT(cpu.iterations() == gpu.iterations(), "%s iterations %zu vs %zu", name, cpu.iterations(), gpu.iterations());
  EXPECT(cpu.getInnerIterations() == gpu.getInnerIterations(), "%s inner iterations %d vs %d", name, cpu.getInnerIterations(), gpu.getInnerIterations());
  EXPECT(std::abs(cpu.error() - gpu.error()) <= 1e-6 * std::abs(cpu.error()) + 1e-12, "%s final error %.15g vs %.15g", name, cpu.error(), gpu.error());
  EXPECT(std::abs(graph.error(rg) - gpu.error()) <= 1e-9 * std::abs(gpu.error()) + 1e-12, "%s values()/error() out of sync", name);
  EXPECT(valuesDiff(rc, rg) <= 1e-5, "%s optimised values differ by %.3g", name, valuesDiff(rc, rg));
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: test_gpu_sam_gtsam <graph dump> ...\n"); return 2; }
  for (int a = 1; a < argc; a++) {
    const sam_text::Graph g = sam_text::read(argv[a]);
    const std::string name = std::string(argv[a]).substr(std::string(argv[a]).find_last_of('/') + 1);
    std::printf("%s: %zu factors (%zu bearing / range, %zu stereo, %zu projection), %zu variables\n", name.c_str(), g.graph.size(), g.n_sam, g.n_stereo, g.n_proj, g.initial.size());
    const LevenbergMarquardtParams params;   // defaults: COLAMD ordering, multifrontal Cholesky
    abTest(name.c_str(), g, params);
    compare((name + " direct").c_str(), g, params);
    compare((name + " Iterative PCG").c_str(), g, iterativeParams(params));
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
