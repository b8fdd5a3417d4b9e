// tests/cpp/test_shim_extractor.cpp -- the extractor of the GTSAM-side shim (NonlinearFactorGraph / Values -> the SoA tables
// of gtg_problem), on the CPU.  Runs under tools/hipstub (LD_PRELOAD; dry-run HIP runtime that hashes every host-to-device
// copy): graphs are built the way the reference's examples build them, from the reference's shipped files through the
// reference's own loaders, handed to gtsam_amd::GpuLevenbergMarquardtOptimizer, and the records of everything the library
// uploaded are printed.  tests/test_shim_extractor_cpu.py compares them with the records of the Python mirror's extractor
// for the same graphs: equal records = identical device tables (variable order, factor tables, shared noise rows, packed
// values, and the whole symbolic analysis behind them).  Also: content outside the path is rejected with the reference's
// exception types before anything reaches the device.
#include <GpuLevenbergMarquardtOptimizer.h>
#include <gtsam/geometry/Cal3Bundler.h>
#include <gtsam/geometry/Cal3DS2.h>
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/geometry/PinholeCamera.h>
#include <gtsam/geometry/Pose2.h>
#include <gtsam/inference/Symbol.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/sfm/SfmData.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/GeneralSFMFactor.h>
#include <gtsam/slam/ProjectionFactor.h>
#include <gtsam/slam/SmartProjectionFactor.h>
#include <gtsam/slam/dataset.h>

#include <cstdio>
#include <string>

using namespace gtsam;
using symbol_shorthand::C;
using symbol_shorthand::P;
typedef PinholeCamera<Cal3Bundler> SfmCamera;
typedef GeneralSFMFactor<SfmCamera, Point3> MyFactor;

extern "C" {
int hipstub_h2d_count(void) __attribute__((weak));
void hipstub_h2d_record(int i, long long* n, unsigned long long* h) __attribute__((weak));
void hipstub_reset(void) __attribute__((weak));
}

// all-reduce stand-ins for shards that are set up one after the other in this process (under the stub a "device" pointer is
// host memory): as if every shard contributed the same buffer -- true for the layout check of the upload -- or nothing
static int lockstepSum(void* ptr, int64_t n, void*, void* user) { double* p = static_cast<double*>(ptr); for (int64_t i = 0; i < n; i++) p[i] *= *static_cast<int*>(user); return 0; }
static int noSum(void*, int64_t, void*, void*) { return 0; }

// A graph from literals that enters every branch of the extractor the three file cases miss: GeneralSFMFactors beside smart factors
// (three parameter sets), projection factors with Cal3_S2 / Cal3DS2 calibrations (objects shared between factors) with and without
// body_P_sensor, BetweenFactor<Pose3>, priors on Pose3 / SfmCamera / Point3, and Robust(Huber) / full Gaussian / Diagonal / Unit /
// Isotropic models, two of them as pairs of distinct objects with equal values.  Every number is exactly representable (small
// integers, dyadic fractions, axis-permutation rotations), so tests/test_shim_extractor_cpu.py packs the same bits from the same
// literals.  30 factors: with GTG_HOST_THREADS=5 GTG_EXTRACT_GRAIN=3 the chunks are [0,6) [6,12) [12,18) [18,24) [24,30): the cuts at
// 6, 12 and 18 fall inside the runs of GeneralSFM, projection and between factors, the cut at 24 between the priors and a smart
// factor, and the last chunk holds one more factor of every table, so every table's offset is added at least once.  A noise model
// makes its first appearance in graph order, in table order and in chunk order at the same place (rows are handed out in
// first-occurrence order per table within a chunk, by the Python mirror in graph order).
static void mixedEveryBranch(NonlinearFactorGraph* graph, Values* initial) {
  using symbol_shorthand::L;
  using symbol_shorthand::X;
  typedef GenericProjectionFactor<Pose3, Point3, Cal3_S2> Proj;
  typedef GenericProjectionFactor<Pose3, Point3, Cal3DS2> ProjDS2;
  typedef SmartProjectionFactor<SfmCamera> Smart;
  const Rot3 Rz(0, -1, 0, 1, 0, 0, 0, 0, 1), Rx(1, 0, 0, 0, 0, -1, 0, 1, 0), Ry(0, 0, 1, 0, 1, 0, -1, 0, 0);
  const Pose3 X0(Rot3(), Point3(0, 0, 0)), X1(Rz, Point3(1, 2, -3)), X2(Rx, Point3(-0.5, 4, 0.25));
  const Pose3 T1(Rz, Point3(1, 0, 0.5)), T2(Ry, Point3(0, -2, 8)), T3(Rx, Point3(0.125, 3, -1));
  const Pose3 S1(Ry, Point3(0.5, 0, 0)), S2(Rz, Point3(0, 0.25, -0.125));
  const SfmCamera cam[4] = {SfmCamera(X1, Cal3Bundler(512, 0.25, -0.125, 0, 0)), SfmCamera(T2, Cal3Bundler(256, 0, 0.5, 2, -4)),
                            SfmCamera(T3, Cal3Bundler(640, -0.0625, 0, 0, 0)), SfmCamera(X2, Cal3Bundler(128, 0.5, 0.25, -1, 1))};
  for (int i = 0; i < 4; i++) initial->insert(C(i), cam[i]);
  initial->insert(P(0), Point3(1, -2, 3)); initial->insert(P(1), Point3(0.5, 0.25, 16)); initial->insert(P(2), Point3(-4, 7, 9));
  initial->insert(L(0), Point3(0.5, 0.25, -4)); initial->insert(L(1), Point3(2, 2, 32));
  initial->insert(X(0), X0); initial->insert(X(1), X1); initial->insert(X(2), X2);
  auto nA = noiseModel::Isotropic::Sigma(2, 0.5), nA2 = noiseModel::Isotropic::Sigma(2, 0.5);   // two objects, one row
  auto nH = noiseModel::Robust::Create(noiseModel::mEstimator::Huber::Create(1.5), noiseModel::Isotropic::Sigma(2, 0.25));
  auto nU = noiseModel::Unit::Create(2);
  Matrix6 R = 2.0 * Matrix6::Identity(); R(0, 1) = 0.5; R(0, 5) = -0.25; R(2, 3) = 1; R(4, 5) = 0.125;
  auto nG = noiseModel::Gaussian::SqrtInformation(R);
  const Vector6 sig = (Vector6() << 0.5, 0.5, 0.5, 0.25, 0.25, 0.125).finished();
  auto nD = noiseModel::Diagonal::Sigmas(sig), nD2 = noiseModel::Diagonal::Sigmas(sig);         // two objects, one row
  auto n9 = noiseModel::Isotropic::Sigma(9, 0.125), n3 = noiseModel::Isotropic::Sigma(3, 0.5), n3b = noiseModel::Isotropic::Sigma(3, 0.5);
  auto nS = noiseModel::Isotropic::Sigma(2, 2.0);
  auto K1 = std::make_shared<Cal3_S2>(500, 400, 0.5, 320, 240), K2 = std::make_shared<Cal3_S2>(250, 250, 0, 160, 120);
  auto D1 = std::make_shared<Cal3DS2>(300, 350, 0.25, 100, 50, 0.125, -0.0625, 0.03125, 0.015625);
  // chunk [0, 6)
  graph->emplace_shared<MyFactor>(Point2(1, 2), nA, C(0), P(0));
  graph->emplace_shared<MyFactor>(Point2(-3, 4), nA, C(1), P(0));
  graph->emplace_shared<MyFactor>(Point2(0.5, -1.5), nA, C(2), P(0));
  graph->emplace_shared<MyFactor>(Point2(8, -2), nA, C(0), P(1));
  graph->emplace_shared<MyFactor>(Point2(2.25, 1), nH, C(1), P(1));
  graph->emplace_shared<MyFactor>(Point2(-7, 3), nH, C(2), P(1));
  // chunk [6, 12)
  graph->emplace_shared<MyFactor>(Point2(4, 4), nA2, C(0), P(2));
  graph->emplace_shared<MyFactor>(Point2(-0.75, 6), nA2, C(2), P(2));
  SmartProjectionParams sp1(JACOBIAN_Q, HANDLE_INFINITY);
  sp1.setRankTolerance(4);
  auto s1 = std::make_shared<Smart>(nA2, sp1);
  s1->add(Point2(1, 1), C(0)); s1->add(Point2(2, -1), C(1)); s1->add(Point2(-3, 0.5), C(2));
  graph->push_back(s1);
  SmartProjectionParams sp2(JACOBIAN_SVD, ZERO_ON_DEGENERACY, false, false, 0.125);
  sp2.setRankTolerance(0.25); sp2.setLandmarkDistanceThreshold(64); sp2.setDynamicOutlierRejectionThreshold(8);
  auto s2 = std::make_shared<Smart>(nA, sp2);
  s2->add(Point2(5, 2), C(3)); s2->add(Point2(-1, -2), C(0));
  graph->push_back(s2);
  graph->emplace_shared<Proj>(Point2(10, 20), nA, X(0), L(0), K1);
  graph->emplace_shared<Proj>(Point2(-5, 7.5), nA, X(1), L(0), K1, S1);
  // chunk [12, 18)
  graph->emplace_shared<Proj>(Point2(3, -4), nU, X(2), L(0), K2, S2);
  graph->emplace_shared<ProjDS2>(Point2(6.5, 1), nU, X(0), L(1), D1);
  graph->emplace_shared<ProjDS2>(Point2(-2, -8), nA, X(1), L(1), D1, S1);
  graph->emplace_shared<BetweenFactor<Pose3>>(X(0), X(1), T1, nG);
  graph->emplace_shared<BetweenFactor<Pose3>>(X(1), X(2), T2, nD);
  graph->emplace_shared<BetweenFactor<Pose3>>(X(0), X(2), T3, nG);
  // chunk [18, 24)
  graph->emplace_shared<BetweenFactor<Pose3>>(X(2), X(1), T1, nD2);
  graph->emplace_shared<BetweenFactor<Pose3>>(X(1), X(0), T2, nG);
  graph->addPrior(X(0), X0, nD);
  graph->addPrior(C(0), cam[0], n9);
  graph->addPrior(P(0), Point3(1, -2, 3), n3);
  graph->addPrior(L(0), Point3(0.5, 0.25, -4), n3b);
  // chunk [24, 30)
  auto s3 = std::make_shared<Smart>(nS);
  s3->add(Point2(0, 1), C(1)); s3->add(Point2(1, 0), C(2));
  graph->push_back(s3);
  graph->addPrior(X(2), X2, nD2);
  graph->emplace_shared<BetweenFactor<Pose3>>(X(2), X(0), T3, nG);
  graph->emplace_shared<Proj>(Point2(1.5, 2.5), nU, X(2), L(1), K2, S2);
  graph->emplace_shared<MyFactor>(Point2(9, -9), nH, C(1), P(2));
  graph->emplace_shared<MyFactor>(Point2(-6, 0.5), nA, C(3), P(2));
}

static void report(const char* name) {
  std::printf("CASE %s", name);
  for (int i = 0; i < hipstub_h2d_count(); i++) { long long n; unsigned long long h; hipstub_h2d_record(i, &n, &h); std::printf(" %lld:%llu", n, h); }
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (!hipstub_h2d_count) { std::printf("run under LD_PRELOAD=tools/hipstub/libhipstub.so\n"); return 2; }
  const std::string data = argc > 1 ? argv[1] : "/root/reference/examples/Data/";
  int failures = 0;
  {  // examples/SFMExample_bal.cpp:43-76 on dubrovnik-3-7-pre
    SfmData mydata = SfmData::FromBalFile(data + "dubrovnik-3-7-pre.txt");
    NonlinearFactorGraph graph;
    auto noise = noiseModel::Isotropic::Sigma(2, 1.0);
    size_t j = 0;
    for (const SfmTrack& track : mydata.tracks) {
      for (const auto& m : track.measurements) graph.emplace_shared<MyFactor>(m.second, noise, C(m.first), P(j));
      j += 1;
    }
    graph.addPrior(C(0), mydata.cameras[0], noiseModel::Isotropic::Sigma(9, 0.1));
    graph.addPrior(P(0), mydata.tracks[0].p, noiseModel::Isotropic::Sigma(3, 0.1));
    Values initial;
    size_t i = 0; j = 0;
    for (const SfmCamera& camera : mydata.cameras) initial.insert(C(i++), camera);
    for (const SfmTrack& track : mydata.tracks) initial.insert(P(j++), track.p);
    hipstub_reset();
    gtsam_amd::GpuLevenbergMarquardtOptimizer lm(graph, initial);
    report("sfmexample_bal_dubrovnik_3_7");
    // (this program runs under tools/hipstub, where kernels do not run: the initial error, which the optimizer takes from the device
    // since round 3, is checked against graph.error(initial) by the GPU test tests/cpp/test_gpu_lm_gtsam.cpp; here: the state exists,
    // holds the caller's values, and the copy of the graph is complete)
    if (lm.values().size() != initial.size() || !lm.values().equals(initial, 1e-12)) { failures++; std::printf("FAIL initial values\n"); }
    // the same graph as shard s of 2 (ShardSpec): set-up incl. the layout verification through the callback
    int world = 2;
    for (int sh = 0; sh < world; sh++) {
      try { gtsam_amd::GpuLevenbergMarquardtOptimizer part(graph, initial, LevenbergMarquardtParams(), 0, gtsam_amd::ShardSpec{sh, world, &lockstepSum, &world}); }
      catch (const std::exception& e) { failures++; std::printf("FAIL sharded construction %d: %s\n", sh, e.what()); }
    }
    bool threw = false;   // an all-reduce that does not span the shards is detected at construction
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer part(graph, initial, LevenbergMarquardtParams(), 0, gtsam_amd::ShardSpec{0, world, &noSum, nullptr}); }
    catch (const std::runtime_error&) { threw = true; }
    if (!threw) { failures++; std::printf("FAIL a communicator that does not span n_shards must be rejected\n"); }
    threw = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer part(graph, initial, LevenbergMarquardtParams(), 0, gtsam_amd::ShardSpec{0, world, nullptr, nullptr}); }
    catch (const std::invalid_argument&) { threw = true; }
    if (!threw) { failures++; std::printf("FAIL n_shards > 1 without a callback must be rejected\n"); }
  }
  {  // examples/Pose2SLAMExample_g2o.cpp:46-67 protocol on w100.graph (load2D creates one noise model object per edge)
    auto gv = load2D(data + "w100.graph");
    NonlinearFactorGraph graph = *gv.first;
    graph.addPrior(0, Pose2(), noiseModel::Diagonal::Variances(Vector3(1e-6, 1e-6, 1e-8)));
    hipstub_reset();
    gtsam_amd::GpuLevenbergMarquardtOptimizer lm(graph, *gv.second);
    report("pose2slam_w100");
  }
  {  // Pose3SLAMExample_g2o.cpp protocol on pose3example.txt (EDGE_SE3:QUAT, full information matrices)
    auto gv = readG2o(data + "pose3example.txt", true);
    NonlinearFactorGraph graph = *gv.first;
    graph.addPrior(0, gv.second->at<Pose3>(0), noiseModel::Diagonal::Variances((Vector(6) << 1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4).finished()));
    hipstub_reset();
    gtsam_amd::GpuLevenbergMarquardtOptimizer lm(graph, *gv.second);
    report("pose3slam_pose3example");
  }
  {  // every remaining branch of the extractor, from literals (see mixedEveryBranch)
    NonlinearFactorGraph graph; Values initial;
    mixedEveryBranch(&graph, &initial);
    hipstub_reset();
    gtsam_amd::GpuLevenbergMarquardtOptimizer lm(graph, initial);
    report("mixed_every_branch");
    if (graph.size() != 30 || lm.values().size() != initial.size() || !lm.values().equals(initial, 1e-12)) { failures++; std::printf("FAIL mixed_every_branch: graph / initial values\n"); }
  }
  {  // rejected before anything is uploaded: the reference's exception types
    NonlinearFactorGraph graph; Values initial;
    initial.insert(0, Pose3()); initial.insert(1, Pose3());
    graph.emplace_shared<BetweenFactor<Pose3>>(0, 7, Pose3(), noiseModel::Unit::Create(6));       // key 7 is not in Values
    bool ok = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(graph, initial); } catch (const ValuesKeyDoesNotExist&) { ok = true; } catch (...) {}
    if (!ok) { failures++; std::printf("FAIL unknown key must raise ValuesKeyDoesNotExist\n"); }
    NonlinearFactorGraph g2; g2.emplace_shared<BetweenFactor<Pose3>>(0, 1, Pose3(), noiseModel::Constrained::All(6));
    ok = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(g2, initial); } catch (const std::invalid_argument&) { ok = true; } catch (...) {}
    if (!ok) { failures++; std::printf("FAIL constrained noise must raise invalid_argument\n"); }
    Values v3; v3.insert(0, Rot3()); 
    ok = false;
    try { gtsam_amd::GpuLevenbergMarquardtOptimizer bad(NonlinearFactorGraph(), v3); } catch (const std::invalid_argument&) { ok = true; } catch (...) {}
    if (!ok) { failures++; std::printf("FAIL unsupported value type must raise invalid_argument\n"); }
  }
  std::printf(failures ? "FAILED (%d)\n" : "ALL PASSED\n", failures);
  return failures ? 1 : 0;
}
