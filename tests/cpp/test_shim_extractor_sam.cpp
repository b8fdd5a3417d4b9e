// tests/cpp/test_shim_extractor_sam.cpp -- the shim's extractor on graphs with BearingRangeFactor / RangeFactor / BearingFactor
// <Pose3, Point3>, on the CPU.  Runs under tools/hipstub like tests/cpp/test_shim_extractor_stereo.cpp: the graph of a text dump
// (sam_graph_text.h) goes through gtsam_amd::GpuLevenbergMarquardtOptimizer and the records of everything the library uploaded are
// printed; tests/test_sam_shim_extractor.py compares them with the records of the Python mirror's extractor for the same graph.
// Also: a RangeFactor<Pose3, Pose3> (a pose-pose factor, out of scope) is refused as a factor type outside the GPU hot path.
#include <GpuLevenbergMarquardtOptimizer.h>

#include <cstdio>

#include "sam_graph_text.h"

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
    const sam_text::Graph g = sam_text::read(argv[a]);
    hipstub_reset();
    gtsam_amd::GpuLevenbergMarquardtOptimizer lm(g.graph, g.initial);
    std::printf("CASE %d", a);
    for (int i = 0; i < hipstub_h2d_count(); i++) { long long n; unsigned long long h; hipstub_h2d_record(i, &n, &h); std::printf(" %lld:%llu", n, h); }
    std::printf("\n");
    // the measurements as the reference's factors hold them (hexadecimal floats: exact), in the layout of sam_z
    std::printf("SAMZ %d", a);
    for (const auto& f : g.graph) {
      double z[4] = {0, 0, 0, 0};
      const Unit3* u = nullptr;
      if (auto br = dynamic_cast<const BearingRangeFactor<Pose3, Point3>*>(f.get())) { u = &br->measured().bearing(); z[3] = br->measured().range(); }
      else if (auto rf = dynamic_cast<const RangeFactor<Pose3, Point3>*>(f.get())) z[3] = rf->measured();
      else if (auto bf = dynamic_cast<const BearingFactor<Pose3, Point3>*>(f.get())) u = &bf->measured();
      else continue;
      if (u) { const Vector3 v = u->unitVector(); z[0] = v(0); z[1] = v(1); z[2] = v(2); }
      std::printf(" %a %a %a %a", z[0], z[1], z[2], z[3]);
    }
    std::printf("\n");
    if (lm.values().size() != g.initial.size() || !lm.values().equals(g.initial, 1e-12)) { failures++; std::printf("FAIL initial values\n"); }
  }
  {
    NonlinearFactorGraph graph; Values initial;
    initial.insert(0, Pose3()); initial.insert(1, Pose3(Rot3(), Point3(0, 0, 5)));
    graph.emplace_shared<RangeFactor<Pose3, Pose3>>(0, 1, 5.0, noiseModel::Unit::Create(1));
    graph.addPrior(Key(0), Pose3(), noiseModel::Unit::Create(6));
    bool ok = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(graph, initial); } catch (const std::invalid_argument&) { ok = true; } catch (...) {}
    if (!ok) { failures++; std::printf("FAIL RangeFactor<Pose3, Pose3> must raise invalid_argument\n"); }
    // (a bearing / range factor with a model of another dimension cannot be constructed in the reference at all -- ExpressionFactor
    // checks --: the library's own check of the noise dimension is exercised through the C ABI, tests/test_sam_api_mirror.py)
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
