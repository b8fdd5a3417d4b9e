// tests/cpp/test_gpu_lm_pose_partial.cpp -- PoseTranslationPrior / PoseRotationPrior <Pose3 | Pose2> through the drop-in, against the
// reference's optimizer on the same NonlinearFactorGraph / Values built with the reference's own factor classes:
//   - gpu.linearize() against graph.linearize() per Jacobian factor (<= 1e-9), a partial prior with its 3, 2 or 1 rows;
//   - the records the shim uploaded tables give for the partial priors EQUAL those the Python extractor's tables gave (`jac6` of the
//     dump, recorded on the same device by tests/test_gpu_pose_partial_shim.py): same library, same numbers in, same bits out;
//   - iterate() by iterate() of both optimizers in the loop of NonlinearOptimizer::defaultOptimize: the same inner iteration count
//     after every outer iteration (the accept / reject sequence);
//   - optimize() of both: the same iteration count and accept / reject total, the final error to 1e-9 relative, values to 1e-5;
//   - RangeFactor<Pose3, Pose3> is still refused with invalid_argument.
// Graphs: text dumps of tests/golden/pose_partial_graph3d.npz, pose_partial_vo.npz and pose_partial_graph2d.npz (argv).
#include <GpuLevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/sam/RangeFactor.h>

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "pose_partial_graph_text.h"

using namespace gtsam;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static double valuesDiff(const Values& a, const Values& b) {
  double worst = 0;
  for (const auto& kv : a) worst = std::max(worst, kv.value.localCoordinates_(b.at(kv.key)).cwiseAbs().maxCoeff());
  return worst;
}

static void records(const char* name, const pose_partial_text::Graph& g, const LevenbergMarquardtParams& params) {
  gtsam_amd::GpuLevenbergMarquardtOptimizer gpu(g.graph, g.initial, params);
  const GaussianFactorGraph::shared_ptr lc = g.graph.linearize(g.initial), lg = gpu.linearize();
  EXPECT(lc->size() == lg->size(), "%s linearize(): %zu vs %zu factors", name, lc->size(), lg->size());
  const size_t first = g.graph.size() - g.n_partial;
  double worstJ = 0, worstRec = 0; size_t shaped = 0, compared = 0;
  for (size_t i = g.n_smart; i < std::min(lc->size(), lg->size()); i++) {      // (a smart factor's linearisation is a Hessian factor the device never forms)
    if (!lg->at(i)) { EXPECT(false, "%s linearize(): factor %zu missing", name, i); continue; }
    const Matrix a = lc->at(i)->augmentedJacobian(), b = lg->at(i)->augmentedJacobian();
    if (a.rows() != b.rows() || a.cols() != b.cols() || lc->at(i)->keys() != lg->at(i)->keys()) { EXPECT(false, "%s linearize(): factor %zu shape / keys", name, i); continue; }
    worstJ = std::max(worstJ, (a - b).cwiseAbs().maxCoeff() / std::max(1.0, a.cwiseAbs().maxCoeff()));
    if (i < first) continue;
    const size_t k = i - first;
    const int R = g.rows[k], d = g.dim[k];
    if (b.rows() == R && b.cols() == d + 1) shaped++;
    if (g.jac6.empty()) continue;
    const double* rec = &g.jac6[90 * k];
    for (int r = 0; r < R; r++) {
      for (int c = 0; c < d; c++) worstRec = std::max(worstRec, std::abs(b(r, c) - rec[r * d + c]));
      worstRec = std::max(worstRec, std::abs(b(r, d) - rec[81 + r]));
    }
    compared++;
  }
  EXPECT(shaped == g.n_partial, "%s linearize(): %zu of %zu partial priors have their rows x (d + 1)", name, shaped, g.n_partial);
  EXPECT(worstJ <= 1e-9, "%s linearize(): Jacobians differ by %.3g", name, worstJ);
  EXPECT(compared == g.n_partial && worstRec == 0.0, "%s: the shim's records of %zu / %zu partial priors differ from the Python extractor's by %.3g", name, compared, g.n_partial, worstRec);
  std::printf("%-28s linearize() %.2g, records vs the Python extractor's %.2g (%zu factors)\n", name, worstJ, worstRec, compared);
}

// the loop of NonlinearOptimizer::defaultOptimize (nonlinear/NonlinearOptimizer.cpp:62-117) around iterate(): the inner iteration count after every outer iteration
template <class OPT> static std::vector<int> sequence(OPT& opt, const LevenbergMarquardtParams& params) {
  std::vector<int> inner;
  double currentError = opt.error(), newError = currentError;
  if (currentError <= params.errorTol) return inner;
  do {
    currentError = newError;
    opt.iterate();
    newError = opt.error();
    inner.push_back(opt.getInnerIterations());
  } while (opt.iterations() < (size_t)params.maxIterations &&
           !checkConvergence(params.relativeErrorTol, params.absoluteErrorTol, params.errorTol, currentError, newError, params.verbosity) && std::isfinite(currentError));
  return inner;
}

static void compare(const char* name, const pose_partial_text::Graph& g, const LevenbergMarquardtParams& params) {
  const NonlinearFactorGraph& graph = g.graph; const Values& initial = g.initial;
  {
    LevenbergMarquardtOptimizer cpu(graph, initial, params);
    gtsam_amd::GpuLevenbergMarquardtOptimizer gpu(graph, initial, params);
    const std::vector<int> sc = sequence(cpu, params), sg = sequence(gpu, params);
    EXPECT(sc == sg && !sc.empty(), "%s iterate(): accept / reject sequences differ (%zu vs %zu outer iterations)", name, sc.size(), sg.size());
    EXPECT(std::abs(cpu.error() - gpu.error()) <= 1e-9 * std::abs(cpu.error()), "%s iterate(): final error %.15g vs %.15g", name, cpu.error(), gpu.error());
  }
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
  EXPECT(std::abs(cpu.error() - gpu.error()) <= 1e-9 * std::abs(cpu.error()), "%s final error %.15g vs %.15g", name, cpu.error(), gpu.error());
  EXPECT(std::abs(graph.error(rg) - gpu.error()) <= 1e-9 * std::abs(gpu.error()) + 1e-12, "%s values()/error() out of sync", name);
  EXPECT(valuesDiff(rc, rg) <= 1e-5, "%s optimised values differ by %.3g", name, valuesDiff(rc, rg));
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: test_gpu_lm_pose_partial <graph dump> ...\n"); return 2; }
  for (int a = 1; a < argc; a++) {
    const pose_partial_text::Graph g = pose_partial_text::read(argv[a]);
    const std::string name = std::string(argv[a]).substr(std::string(argv[a]).find_last_of('/') + 1);
    std::printf("%s: %zu factors (%zu partial pose priors, %zu between, %zu smart, %zu projection), %zu variables\n", name.c_str(), g.graph.size(), g.n_partial,
                g.n_between, g.n_smart, g.n_proj, g.initial.size());
    const LevenbergMarquardtParams params;   // defaults: COLAMD ordering, multifrontal Cholesky
    records(name.c_str(), g, params);
    compare(name.c_str(), g, params);
  }
  {
    NonlinearFactorGraph graph; Values initial;
    initial.insert(0, Pose3()); initial.insert(1, Pose3(Rot3(), Point3(0, 0, 5)));
    graph.emplace_shared<RangeFactor<Pose3, Pose3>>(0, 1, 5.0, noiseModel::Unit::Create(1));
    graph.emplace_shared<PoseTranslationPrior<Pose3>>(Key(0), Point3(0, 0, 0), noiseModel::Unit::Create(3));
    bool ok = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(graph, initial); } catch (const std::invalid_argument&) { ok = true; } catch (...) {}
    EXPECT(ok, "RangeFactor<Pose3, Pose3> must raise invalid_argument");
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
