// tests/cpp/planar_graph_text.h -- a planar landmark SLAM graph (BearingRangeFactor / RangeFactor / BearingFactor <Pose2, Point2>,
// BetweenFactor<Pose2>, PriorFactor<Pose2>, the 2-D partial pose priors) from the text dump tests/planar_support.py writes of a
// gtg_problem and its packed values (lines "name count" followed by the numbers), in the pattern of sam_graph_text.h: POSE2 / POINT2
// variables with Key = variable id -- a POINT2 takes three doubles of the dump (x, y, 0) and becomes a Point2 --, factors in the order
// planar, between, prior, partial priors.  One noise-model object per row of the noise table, shared by the factors that name the row.
// A measured bearing goes through Rot2::fromCosSin, as the generator's did.
#pragma once
#include <gtsam/geometry/Pose2.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/Values.h>
#include <gtsam/sam/BearingFactor.h>
#include <gtsam/sam/BearingRangeFactor.h>
#include <gtsam/sam/RangeFactor.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/PoseRotationPrior.h>
#include <gtsam/slam/PoseTranslationPrior.h>

#include <fstream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace planar_text {
using namespace gtsam;

struct Graph { NonlinearFactorGraph graph; Values initial; size_t n_sam2 = 0; std::vector<int> kind; };

inline Graph read(const std::string& path) {
  std::ifstream is(path);
  if (!is) throw std::runtime_error("cannot open " + path);
  std::map<std::string, std::vector<double>> t;
  std::string name; size_t n;
  while (is >> name >> n) { auto& v = t[name]; v.resize(n); for (size_t i = 0; i < n; i++) is >> v[i]; }
  auto I = [&](const char* k, size_t i) { return (int)t.at(k).at(i); };
  auto has = [&](const char* k) { return t.count(k) && !t.at(k).empty(); };
  Graph out;
  const auto& vt = t.at("var_type"); const auto& values = t.at("values");
  for (size_t v = 0; v < vt.size(); v++) {
    const double* q = &values[3 * v];
    if ((int)vt[v] == 3) out.initial.insert(Key(v), Pose2(q[0], q[1], q[2]));
    else if ((int)vt[v] == 4) out.initial.insert(Key(v), Point2(q[0], q[1]));
    else throw std::runtime_error("POSE2 / POINT2 variables only");
  }
  std::vector<SharedNoiseModel> noise(t.at("noise_kind").size());
  for (size_t i = 0; i < noise.size(); i++) {
    const int kind = I("noise_kind", i), dim = I("noise_dim", i);
    const double* d = t.at("noise_data").data() + (size_t)t.at("noise_off")[i];
    SharedNoiseModel base;
    if (kind == 0) base = noiseModel::Unit::Create(dim);
    else if (kind == 1) base = noiseModel::Isotropic::Sigma(dim, d[0], false);
    else if (kind == 2) base = noiseModel::Diagonal::Sigmas(Eigen::Map<const Vector>(d, dim), false);
    else { Matrix R(dim, dim); for (int r = 0; r < dim; r++) for (int c = 0; c < dim; c++) R(r, c) = d[r * dim + c]; base = noiseModel::Gaussian::SqrtInformation(R, false); }
    const int rk = has("noise_robust") ? I("noise_robust", i) : 0;
    if (rk != 0 && rk != 2 && rk != 3) throw std::runtime_error("Huber, Cauchy or no m-estimator only");
    if (rk == 2) noise[i] = noiseModel::Robust::Create(noiseModel::mEstimator::Huber::Create(t.at("noise_robust_param")[i]), base);
    else if (rk == 3) noise[i] = noiseModel::Robust::Create(noiseModel::mEstimator::Cauchy::Create(t.at("noise_robust_param")[i]), base);
    else noise[i] = base;
  }
  out.n_sam2 = has("sam2_pose") ? t.at("sam2_pose").size() : 0;
  for (size_t i = 0; i < out.n_sam2; i++) {
    const double* z = &t.at("sam2_z")[3 * i];
    const Key x = Key(I("sam2_pose", i)), l = Key(I("sam2_point", i));
    const SharedNoiseModel& nz = noise[I("sam2_noise", i)];
    out.kind.push_back(I("sam2_kind", i));
    if (I("sam2_kind", i) == 0) out.graph.emplace_shared<BearingRangeFactor<Pose2, Point2>>(x, l, Rot2::fromCosSin(z[0], z[1]), z[2], nz);
    else if (I("sam2_kind", i) == 1) out.graph.emplace_shared<RangeFactor<Pose2, Point2>>(x, l, z[2], nz);
    else out.graph.emplace_shared<BearingFactor<Pose2, Point2>>(x, l, Rot2::fromCosSin(z[0], z[1]), nz);
  }
  for (size_t i = 0; has("between_v1") && i < t.at("between_v1").size(); i++) {
    const double* z = &t.at("between_z")[12 * i];
    out.graph.emplace_shared<BetweenFactor<Pose2>>(Key(I("between_v1", i)), Key(I("between_v2", i)), Pose2(z[0], z[1], z[2]), noise[I("between_noise", i)]);
  }
  for (size_t i = 0; has("prior_var") && i < t.at("prior_var").size(); i++) {
    const double* d = &t.at("prior_data")[(size_t)t.at("prior_off")[i]];
    out.graph.addPrior(Key(I("prior_var", i)), Pose2(d[0], d[1], d[2]), noise[I("prior_noise", i)]);
  }
  for (size_t i = 0; has("pose_partial_var") && i < t.at("pose_partial_var").size(); i++) {
    const double* z = &t.at("pose_partial_z")[9 * i];
    const Key v = Key(I("pose_partial_var", i));
    if (I("pose_partial_kind", i) == 0) out.graph.emplace_shared<PoseTranslationPrior<Pose2>>(v, Point2(z[0], z[1]), noise[I("pose_partial_noise", i)]);
    else out.graph.emplace_shared<PoseRotationPrior<Pose2>>(v, Rot2::fromCosSin(z[0], z[1]), noise[I("pose_partial_noise", i)]);
  }
  return out;
}
}  // namespace planar_text
