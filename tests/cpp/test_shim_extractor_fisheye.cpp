// tests/cpp/test_shim_extractor_fisheye.cpp -- the shim's extractor on graphs with GenericProjectionFactor<Pose3, Point3, Cal3Fisheye>, on
// the CPU.  Runs under tools/hipstub like tests/cpp/test_shim_extractor.cpp: the graph of a text dump (fisheye_graph_text.h) goes through
// gtsam_amd::GpuLevenbergMarquardtOptimizer and the records of everything the library uploaded are printed;
// tests/test_fisheye_shim_extractor.py compares them with the records of the Python mirror's extractor for the same graph.
// Also: throwCheirality = true is refused, as it is for the other projection factors.
#include <GpuLevenbergMarquardtOptimizer.h>

#include <cstdio>

#include "fisheye_graph_text.h"

using namespace gtsam;

extern "C" {
int hipstub_h2d_count(void) __attribute__((weak));
void hipstub_h2d_record(int i, long long* n, unsigned long long* h) __attribute__((weak));
void hipstub_reset(void) __attribute__((weak));
}

int main(int argc, char** argv) {
  if (!hipstub_h2d_count) { std::printf("run under LD_PRELOAD=tools/hipstub/libhipstub.so\n"); return 2; }
  int failures = 0;
  for (int a = 1; a < argc; a++) {
    const fisheye_text::Graph g = fisheye_text::read(argv[a]);
    hipstub_reset();
    gtsam_amd::GpuLevenbergMarquardtOptimizer lm(g.graph, g.initial);
    std::printf("CASE %d", a);
    for (int i = 0; i < hipstub_h2d_count(); i++) { long long n; unsigned long long h; hipstub_h2d_record(i, &n, &h); std::printf(" %lld:%llu", n, h); }
    std::printf("\n");
    if (lm.values().size() != g.initial.size() || !lm.values().equals(g.initial, 1e-12)) { failures++; std::printf("FAIL initial values\n"); }
  }
  {
    NonlinearFactorGraph graph; Values initial;
    initial.insert(0, Pose3()); initial.insert(1, Point3(0, 0, 5));
    auto K = std::make_shared<Cal3Fisheye>(300, 300, 0, 320, 240, -0.01, 0.02, -0.01, 0.002);
    graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3Fisheye>>(Point2(320, 240), noiseModel::Unit::Create(2), 0, 1, K, true, false);
    bool ok = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(graph, initial); } catch (const std::invalid_argument&) { ok = true; } catch (...) {}
    if (!ok) { failures++; std::printf("FAIL throwCheirality = true must raise invalid_argument\n"); }
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
