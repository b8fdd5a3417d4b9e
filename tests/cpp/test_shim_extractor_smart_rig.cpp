// tests/cpp/test_shim_extractor_smart_rig.cpp -- the shim's extractor on graphs with SmartProjectionRigFactor<PinholePose<Cal3_S2>>, on the CPU.
// Runs under tools/hipstub like tests/cpp/test_shim_extractor_smart_pose.cpp: the graph of a text dump (smart_rig_graph_text.h) goes
// through gtsam_amd::GpuLevenbergMarquardtOptimizer and the records of everything the library uploaded are printed;
// tests/test_smart_rig_shim_extractor.py compares them with the records of the Python mirror's extractor for the same graph.
// Also: what the shim refuses of this factor (enableEPI; the other parameter sets are refused by the reference's own constructor).
#include <GpuLevenbergMarquardtOptimizer.h>

#include <cstdio>
#include <cstring>

#include "smart_rig_graph_text.h"

using namespace gtsam;

extern "C" {
int hipstub_h2d_count(void) __attribute__((weak));
void hipstub_h2d_record(int i, long long* n, unsigned long long* h) __attribute__((weak));
void hipstub_reset(void) __attribute__((weak));
}

static bool refused(const SmartProjectionParams& params, const char* word) {
  NonlinearFactorGraph graph; Values initial;
  initial.insert(0, Pose3()); initial.insert(1, Pose3(Rot3(), Point3(1, 0, 0)));
  typedef SmartProjectionRigFactor<PinholePose<Cal3_S2>> Rig;
  auto rig = std::make_shared<Rig::Cameras>();
  rig->emplace_back(Pose3(), std::make_shared<Cal3_S2>(500, 500, 0, 320, 240));
  auto f = std::make_shared<Rig>(noiseModel::Unit::Create(2), rig, params);
  f->add(Point2(320, 240), 0, 0); f->add(Point2(220, 240), 1, 0);
  graph.push_back(f);
  try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(graph, initial); }
  catch (const std::invalid_argument& e) { return std::strstr(e.what(), word) != nullptr; }
  catch (...) {}
  return false;
}

int main(int argc, char** argv) {
  if (!hipstub_h2d_count) { std::printf("run under LD_PRELOAD=tools/hipstub/libhipstub.so\n"); return 2; }
  int failures = 0;
  for (int a = 1; a < argc; a++) {
    const smart_rig_text::Graph g = smart_rig_text::read(argv[a]);
    hipstub_reset();
    gtsam_amd::GpuLevenbergMarquardtOptimizer lm(g.graph, g.initial);
    std::printf("CASE %d", a);
    for (int i = 0; i < hipstub_h2d_count(); i++) { long long n; unsigned long long h; hipstub_h2d_record(i, &n, &h); std::printf(" %lld:%llu", n, h); }
    std::printf("\n");
    if (lm.values().size() != g.initial.size() || !lm.values().equals(g.initial, 1e-12)) { failures++; std::printf("FAIL initial values\n"); }
  }
  {
    SmartProjectionParams epi(HESSIAN, ZERO_ON_DEGENERACY); epi.setEnableEPI(true);
    if (!refused(epi, "enableEPI")) { failures++; std::printf("FAIL enableEPI on a rig-type smart factor must raise invalid_argument\n"); }
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
