// tests/cpp/test_shim_extractor_planar.cpp -- the shim's extractor on planar landmark SLAM graphs (BearingRangeFactor / RangeFactor /
// BearingFactor <Pose2, Point2>), on the CPU.  Runs under tools/hipstub like tests/cpp/test_shim_extractor_sam.cpp: the graph of a text
// dump (planar_graph_text.h) goes through gtsam_amd::GpuLevenbergMarquardtOptimizer and the records of everything the library uploaded
// are printed; tests/test_planar_shim_extractor.py compares them with the records of the Python mirror's extractor for the same graph.
// Also: RangeFactor<Pose2, Pose2> and RangeFactor<Pose3, Pose3> (pose-pose factors, out of scope) are refused as factor types outside
// the GPU hot path, and the values the optimizer hands back hold Point2 landmarks.
#include <GpuLevenbergMarquardtOptimizer.h>
#include <gtsam/geometry/Pose3.h>

#include <cstdio>

#include "planar_graph_text.h"

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
    const planar_text::Graph g = planar_text::read(argv[a]);
    hipstub_reset();
    gtsam_amd::GpuLevenbergMarquardtOptimizer lm(g.graph, g.initial);
    std::printf("CASE %d", a);
    for (int i = 0; i < hipstub_h2d_count(); i++) { long long n; unsigned long long h; hipstub_h2d_record(i, &n, &h); std::printf(" %lld:%llu", n, h); }
    std::printf("\n");
    // the measurements as the reference's factors hold them (hexadecimal floats: exact), in the layout of sam2_z
    std::printf("SAM2Z %d", a);
    for (const auto& f : g.graph) {
      double z[3] = {0, 0, 0};
      const Rot2* u = nullptr;
      if (auto br = dynamic_cast<const BearingRangeFactor<Pose2, Point2>*>(f.get())) { u = &br->measured().bearing(); z[2] = br->measured().range(); }
      else if (auto rf = dynamic_cast<const RangeFactor<Pose2, Point2>*>(f.get())) z[2] = rf->measured();
      else if (auto bf = dynamic_cast<const BearingFactor<Pose2, Point2>*>(f.get())) u = &bf->measured();
      else continue;
      if (u) { z[0] = u->c(); z[1] = u->s(); }
      std::printf(" %a %a %a", z[0], z[1], z[2]);
    }
    std::printf("\n");
    if (lm.values().size() != g.initial.size() || !lm.values().equals(g.initial, 1e-12)) { failures++; std::printf("FAIL initial values\n"); }
    size_t points = 0;
    for (const auto& kv : lm.values()) if (dynamic_cast<const GenericValue<Point2>*>(&kv.value)) points++;
    if (points == 0) { failures++; std::printf("FAIL no Point2 among the values\n"); }
  }
  {
    NonlinearFactorGraph graph; Values initial;
    initial.insert(0, Pose2()); initial.insert(1, Pose2(5.0, 0.0, 0.0));
    graph.emplace_shared<RangeFactor<Pose2, Pose2>>(0, 1, 5.0, noiseModel::Unit::Create(1));
    graph.addPrior(Key(0), Pose2(), noiseModel::Unit::Create(3));
    bool ok = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(graph, initial); } catch (const std::invalid_argument&) { ok = true; } catch (...) {}
    if (!ok) { failures++; std::printf("FAIL RangeFactor<Pose2, Pose2> must raise invalid_argument\n"); }
  }
  {
    NonlinearFactorGraph graph; Values initial;
    initial.insert(0, Pose3()); initial.insert(1, Pose3(Rot3(), Point3(0, 0, 5)));
    graph.emplace_shared<RangeFactor<Pose3, Pose3>>(0, 1, 5.0, noiseModel::Unit::Create(1));
    graph.addPrior(Key(0), Pose3(), noiseModel::Unit::Create(6));
    bool ok = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(graph, initial); } catch (const std::invalid_argument&) { ok = true; } catch (...) {}
    if (!ok) { failures++; std::printf("FAIL RangeFactor<Pose3, Pose3> must raise invalid_argument\n"); }
  }
  {   // a PriorFactor<Point2> is out of scope: refused, not silently dropped
    NonlinearFactorGraph graph; Values initial;
    initial.insert(0, Pose2()); initial.insert(1, Point2(1.0, 2.0));
    graph.emplace_shared<RangeFactor<Pose2, Point2>>(0, 1, 2.0, noiseModel::Unit::Create(1));
    graph.addPrior(Key(1), Point2(1.0, 2.0), noiseModel::Unit::Create(2));
    bool ok = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(graph, initial); } catch (const std::invalid_argument&) { ok = true; } catch (...) {}
    if (!ok) { failures++; std::printf("FAIL PriorFactor<Point2> must raise invalid_argument\n"); }
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
