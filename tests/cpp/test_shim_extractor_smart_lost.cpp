// tests/cpp/test_shim_extractor_smart_lost.cpp -- the shim's extractor on graphs whose smart factors have useLOST set, on the CPU.
// Runs under tools/hipstub like tests/cpp/test_shim_extractor_smart_rig.cpp: the graph of a text dump (smart_lost_graph_text.h) goes
// through gtsam_amd::GpuLevenbergMarquardtOptimizer and the records of everything the library uploaded are printed;
// tests/test_smart_lost_shim_extractor.py compares them with the records of the Python mirror's extractor for the same graph (slot 7 of
// smart_params is part of them).  Also: useLOST is accepted on all three kinds, with and without a triangulation noise model, and the
// refusals beside it stay -- enableEPI together with a triangulation noise model, enableEPI on pose-type and rig-type factors; what
// sigmas() throws for a model without sigmas leaves the constructor.
#include <GpuLevenbergMarquardtOptimizer.h>

#include <cstdio>
#include <cstring>

#include "smart_lost_graph_text.h"

using namespace gtsam;

extern "C" {
int hipstub_h2d_count(void) __attribute__((weak));
void hipstub_h2d_record(int i, long long* n, unsigned long long* h) __attribute__((weak));
void hipstub_reset(void) __attribute__((weak));
}

typedef PinholeCamera<Cal3Bundler> SfmCamera;
typedef SmartProjectionRigFactor<PinholePose<Cal3_S2>> Rig;

// a two-view graph of the given kind (0 camera-type, 1 pose-type, 2 rig-type) with these parameters
static void build(int kind, const SmartProjectionParams& params, NonlinearFactorGraph* graph, Values* initial) {
  const Pose3 a, b(Rot3(), Point3(1, 0, 0));
  const auto unit = noiseModel::Unit::Create(2);
  const auto K = std::make_shared<Cal3_S2>(500, 500, 0, 320, 240);
  if (kind == 0) {
    initial->insert(0, SfmCamera(a, Cal3Bundler(500, 0, 0, 320, 240))); initial->insert(1, SfmCamera(b, Cal3Bundler(500, 0, 0, 320, 240)));
    auto f = std::make_shared<SmartProjectionFactor<SfmCamera>>(unit, params);
    f->add(Point2(320, 240), 0); f->add(Point2(220, 240), 1);
    graph->push_back(f);
    return;
  }
  initial->insert(0, a); initial->insert(1, b);
  if (kind == 1) {
    auto f = std::make_shared<SmartProjectionPoseFactor<Cal3_S2>>(unit, K, params);
    f->add(Point2(320, 240), 0); f->add(Point2(220, 240), 1);
    graph->push_back(f);
  } else {
    auto rig = std::make_shared<Rig::Cameras>();
    rig->emplace_back(Pose3(), K);
    auto f = std::make_shared<Rig>(unit, rig, params);
    f->add(Point2(320, 240), 0, 0); f->add(Point2(220, 240), 1, 0);
    graph->push_back(f);
  }
}
// 0 accepted, 1 invalid_argument naming `word`, 2 a thrown string literal naming `word` (noiseModel::Base::sigmas), -1 anything else
static int outcome(int kind, const SmartProjectionParams& params, const char* word) {
  NonlinearFactorGraph graph; Values initial;
  build(kind, params, &graph, &initial);
  try { gtsam_amd::GpuLevenbergMarquardtOptimizer lm(graph, initial); return 0; }
  catch (const std::invalid_argument& e) { return std::strstr(e.what(), word) ? 1 : -1; }
  catch (const char* e) { return std::strstr(e, word) ? 2 : -1; }
  catch (...) {}
  return -1;
}

int main(int argc, char** argv) {
  if (!hipstub_h2d_count) { std::printf("run under LD_PRELOAD=tools/hipstub/libhipstub.so\n"); return 2; }
  int failures = 0;
  for (int a = 1; a < argc; a++) {
    const smart_lost_text::Graph g = smart_lost_text::read(argv[a]);
    if (!g.n_lost) { failures++; std::printf("FAIL %s has no LOST factor\n", argv[a]); }
    hipstub_reset();
    gtsam_amd::GpuLevenbergMarquardtOptimizer lm(g.graph, g.initial);
    std::printf("CASE %d", a);
    for (int i = 0; i < hipstub_h2d_count(); i++) { long long n; unsigned long long h; hipstub_h2d_record(i, &n, &h); std::printf(" %lld:%llu", n, h); }
    std::printf("\n");
    if (lm.values().size() != g.initial.size() || !lm.values().equals(g.initial, 1e-12)) { failures++; std::printf("FAIL initial values\n"); }
  }
  for (int kind = 0; kind < 3; kind++) {
    SmartProjectionParams lost(HESSIAN, ZERO_ON_DEGENERACY);
    lost.triangulation.useLOST = true; lost.setRankTolerance(1e-9);
    if (outcome(kind, lost, "") != 0) { failures++; std::printf("FAIL useLOST must be accepted (kind %d)\n", kind); }
    lost.triangulation.noiseModel = noiseModel::Diagonal::Sigmas(Vector2(0.3, 0.5));
    if (outcome(kind, lost, "") != 0) { failures++; std::printf("FAIL useLOST with a triangulation noise model must be accepted (kind %d)\n", kind); }
    // sigmas() of a Robust model throws in the reference (noiseModel::Base::sigmas, NoiseModel.cpp:71-73, a string literal): it leaves the
    // constructor as it is
    lost.triangulation.noiseModel = noiseModel::Robust::Create(noiseModel::mEstimator::Huber::Create(1.0), noiseModel::Unit::Create(2));
    if (outcome(kind, lost, "sigmas") != 2) { failures++; std::printf("FAIL the exception of sigmas() must leave the constructor (kind %d)\n", kind); }
    SmartProjectionParams epi(HESSIAN, ZERO_ON_DEGENERACY); epi.setEnableEPI(true);
    if (kind > 0 && outcome(kind, epi, "enableEPI") != 1) { failures++; std::printf("FAIL enableEPI on a pose-type / rig-type smart factor must raise invalid_argument (kind %d)\n", kind); }
    epi.triangulation.noiseModel = noiseModel::Unit::Create(2);
    if (outcome(kind, epi, "enableEPI") != 1) { failures++; std::printf("FAIL enableEPI with a triangulation noise model must raise invalid_argument (kind %d)\n", kind); }
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
