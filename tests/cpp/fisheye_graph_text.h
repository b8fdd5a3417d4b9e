// tests/cpp/fisheye_graph_text.h -- a factor graph with GenericProjectionFactors of three calibration classes (Cal3_S2, Cal3DS2,
// Cal3Fisheye) from the text dump tests/fisheye_support.py writes of a gtg_problem, the model of its calib rows (calib_model: 1 = a
// Cal3Fisheye) and its packed values (lines "name count" followed by the numbers): POSE3 / POINT3 variables with Key = variable id,
// factors in the order projection, between, prior.  One noise-model object per row of the noise table and one calibration object
// per row of the calib table, shared by the factors that name the row -- what the shim's extractor de-duplicates by.
#pragma once
#include <gtsam/geometry/Cal3DS2.h>
#include <gtsam/geometry/Cal3Fisheye.h>
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/Values.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/ProjectionFactor.h>

#include <fstream>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

namespace fisheye_text {
using namespace gtsam;

inline Pose3 pose(const double* p) {
  Matrix3 R;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R(i, j) = p[3 * i + j];
  return Pose3(Rot3(R), Point3(p[9], p[10], p[11]));
}

struct Graph { NonlinearFactorGraph graph; Values initial; size_t n_proj = 0, n_fisheye = 0; };

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
  std::vector<std::shared_ptr<Cal3_S2>> mono(n_calib); std::vector<std::shared_ptr<Cal3DS2>> ds2(n_calib); std::vector<std::shared_ptr<Cal3Fisheye>> fisheye(n_calib);
  auto sensorOf = [&](const char* tab, size_t i) { std::optional<Pose3> s; if (has(tab) && I(tab, i) >= 0) s = pose(&t.at("sensor")[12 * (size_t)I(tab, i)]); return s; };
  out.n_proj = has("proj_pose") ? t.at("proj_pose").size() : 0;
  for (size_t i = 0; i < out.n_proj; i++) {
    const size_t k = (size_t)I("proj_calib", i);
    const double* c = &t.at("calib")[5 * k];
    const double* d = has("calib_distortion") ? &t.at("calib_distortion")[4 * k] : nullptr;
    const Point2 z(t.at("proj_z")[2 * i], t.at("proj_z")[2 * i + 1]);
    if (has("calib_model") && I("calib_model", k) == 1) {
      if (!d) throw std::runtime_error("a fisheye row without calib_distortion");
      if (!fisheye[k]) fisheye[k] = std::make_shared<Cal3Fisheye>(c[0], c[1], c[2], c[3], c[4], d[0], d[1], d[2], d[3]);
      out.graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3Fisheye>>(z, noise[I("proj_noise", i)], Key(I("proj_pose", i)), Key(I("proj_point", i)), fisheye[k], sensorOf("proj_sensor", i));
      out.n_fisheye++;
    } else if (d && (d[0] != 0 || d[1] != 0 || d[2] != 0 || d[3] != 0)) {
      if (!ds2[k]) ds2[k] = std::make_shared<Cal3DS2>(c[0], c[1], c[2], c[3], c[4], d[0], d[1], d[2], d[3]);
      out.graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3DS2>>(z, noise[I("proj_noise", i)], Key(I("proj_pose", i)), Key(I("proj_point", i)), ds2[k], sensorOf("proj_sensor", i));
    } else {
      if (!mono[k]) mono[k] = std::make_shared<Cal3_S2>(c[0], c[1], c[2], c[3], c[4]);
      out.graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3_S2>>(z, noise[I("proj_noise", i)], Key(I("proj_pose", i)), Key(I("proj_point", i)), mono[k], sensorOf("proj_sensor", i));
    }
  }
  for (size_t i = 0; has("between_v1") && i < t.at("between_v1").size(); i++)
    out.graph.emplace_shared<BetweenFactor<Pose3>>(Key(I("between_v1", i)), Key(I("between_v2", i)), pose(&t.at("between_z")[12 * i]), noise[I("between_noise", i)]);
  for (size_t i = 0; has("prior_var") && i < t.at("prior_var").size(); i++) {
    const int v = I("prior_var", i);
    const double* d = &t.at("prior_data")[(size_t)t.at("prior_off")[i]];
    if ((int)vt[v] == 0) out.graph.addPrior(Key(v), pose(d), noise[I("prior_noise", i)]);
    else out.graph.addPrior(Key(v), Point3(d[0], d[1], d[2]), noise[I("prior_noise", i)]);
  }
  return out;
}
}  // namespace fisheye_text
