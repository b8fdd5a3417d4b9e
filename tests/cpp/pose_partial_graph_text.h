// tests/cpp/pose_partial_graph_text.h -- a factor graph with PoseTranslationPrior / PoseRotationPrior <Pose3 | Pose2> (gtsam/slam) from the
// text dump tests/pose_partial_support.py writes of a gtg_problem and its packed values (lines "name count" followed by the numbers), in
// the pattern of smart_pose_graph_text.h: POSE3 / POINT3 / POSE2 variables with Key = variable id, factors in the order smart
// (pose-type), projection, between, partial pose priors.  One noise-model object per row of the noise table and one calibration object
// per row of the calib table, shared by the factors that name the row -- what the shim's extractor de-duplicates by.  The dump may carry
// `jac6`: the partial priors' records as the device gave them for the Python extractor's tables of the same graph.
#pragma once
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/geometry/Pose2.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/Values.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/PoseRotationPrior.h>
#include <gtsam/slam/PoseTranslationPrior.h>
#include <gtsam/slam/ProjectionFactor.h>
#include <gtsam/slam/SmartProjectionPoseFactor.h>

#include <fstream>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

namespace pose_partial_text {
using namespace gtsam;

inline Pose3 pose(const double* p) {
  Matrix3 R;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R(i, j) = p[3 * i + j];
  return Pose3(Rot3(R), Point3(p[9], p[10], p[11]));
}

struct Graph {
  NonlinearFactorGraph graph; Values initial;
  size_t n_smart = 0, n_proj = 0, n_between = 0, n_partial = 0;
  std::vector<int> rows, dim;        // per partial prior: its rows and the tangent dimension of its pose
  std::vector<double> jac6;          // 90 per partial prior, or empty
};

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
  size_t at = 0;
  for (size_t v = 0; v < vt.size(); v++) {
    if ((int)vt[v] == 0) { out.initial.insert(Key(v), pose(&values[at])); at += 12; }
    else if ((int)vt[v] == 3) { out.initial.insert(Key(v), Pose2(values[at], values[at + 1], values[at + 2])); at += 3; }
    else { out.initial.insert(Key(v), Point3(values[at], values[at + 1], values[at + 2])); at += 3; }
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
  const size_t n_calib = has("calib") ? t.at("calib").size() / 5 : 0;
  std::vector<std::shared_ptr<Cal3_S2>> Ks(n_calib);
  for (size_t k = 0; k < n_calib; k++) { const double* c = &t.at("calib")[5 * k]; Ks[k] = std::make_shared<Cal3_S2>(c[0], c[1], c[2], c[3], c[4]); }
  auto sensorOf = [&](const char* tab, size_t i) { std::optional<Pose3> s; if (has(tab) && I(tab, i) >= 0) s = pose(&t.at("sensor")[12 * (size_t)I(tab, i)]); return s; };
  out.n_smart = has("smart_noise") ? t.at("smart_noise").size() : 0;
  for (size_t i = 0; i < out.n_smart; i++) {
    const double* sp = &t.at("smart_params")[8 * i];
    const LinearizationMode lm = sp[5] == 2.0 ? JACOBIAN_Q : (sp[5] == 3.0 ? JACOBIAN_SVD : HESSIAN);
    SmartProjectionParams params(lm, sp[4] == 1.0 ? ZERO_ON_DEGENERACY : (sp[4] == 2.0 ? HANDLE_INFINITY : IGNORE_DEGENERACY), false, false, sp[3]);
    params.setRankTolerance(sp[0]); params.setEnableEPI(sp[6] != 0.0);
    params.setLandmarkDistanceThreshold(sp[1]); params.setDynamicOutlierRejectionThreshold(sp[2]);
    auto f = std::make_shared<SmartProjectionPoseFactor<Cal3_S2>>(noise[I("smart_noise", i)], Ks.at((size_t)I("smart_calib", i)), sensorOf("smart_sensor", i), params);
    for (size_t k = (size_t)t.at("smart_ptr")[i]; k < (size_t)t.at("smart_ptr")[i + 1]; k++)
      f->add(Point2(t.at("smart_z")[2 * k], t.at("smart_z")[2 * k + 1]), Key(I("smart_cam", k)));
    out.graph.push_back(f);
  }
  out.n_proj = has("proj_pose") ? t.at("proj_pose").size() : 0;
  for (size_t i = 0; i < out.n_proj; i++)
    out.graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3_S2>>(Point2(t.at("proj_z")[2 * i], t.at("proj_z")[2 * i + 1]), noise[I("proj_noise", i)],
        Key(I("proj_pose", i)), Key(I("proj_point", i)), Ks.at((size_t)I("proj_calib", i)), sensorOf("proj_sensor", i));
  out.n_between = has("between_v1") ? t.at("between_v1").size() : 0;
  for (size_t i = 0; i < out.n_between; i++) {
    const double* z = &t.at("between_z")[12 * i];
    if ((int)vt[(size_t)I("between_v1", i)] == 3)
      out.graph.emplace_shared<BetweenFactor<Pose2>>(Key(I("between_v1", i)), Key(I("between_v2", i)), Pose2(z[0], z[1], z[2]), noise[I("between_noise", i)]);
    else
      out.graph.emplace_shared<BetweenFactor<Pose3>>(Key(I("between_v1", i)), Key(I("between_v2", i)), pose(z), noise[I("between_noise", i)]);
  }
  out.n_partial = has("pose_partial_var") ? t.at("pose_partial_var").size() : 0;
  for (size_t i = 0; i < out.n_partial; i++) {
    const int v = I("pose_partial_var", i), kind = I("pose_partial_kind", i);
    const double* z = &t.at("pose_partial_z")[9 * i];
    const SharedNoiseModel& m = noise[I("pose_partial_noise", i)];
    if ((int)vt[v] == 0) {
      Matrix3 R;
      for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R(r, c) = z[3 * r + c];
      if (kind == 0) out.graph.emplace_shared<PoseTranslationPrior<Pose3>>(Key(v), Point3(z[0], z[1], z[2]), m);
      else out.graph.emplace_shared<PoseRotationPrior<Pose3>>(Key(v), Rot3(R), m);
      out.rows.push_back(3); out.dim.push_back(6);
    } else {
      if (kind == 0) out.graph.emplace_shared<PoseTranslationPrior<Pose2>>(Key(v), Point2(z[0], z[1]), m);
      else out.graph.emplace_shared<PoseRotationPrior<Pose2>>(Key(v), Rot2::fromCosSin(z[0], z[1]), m);
      out.rows.push_back(kind == 0 ? 2 : 1); out.dim.push_back(3);
    }
  }
  if (has("jac6")) out.jac6 = t.at("jac6");
  return out;
}
}  // namespace pose_partial_text
