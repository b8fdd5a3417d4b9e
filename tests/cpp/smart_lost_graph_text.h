// tests/cpp/smart_lost_graph_text.h -- a factor graph whose smart factors may have TriangulationParameters::useLOST set, from the text dump
// tests/smart_lost_support.py writes of a gtg_problem and its packed values (lines "name count" followed by the numbers).  All three smart
// factor kinds: SmartProjectionFactor<PinholeCamera<Cal3Bundler>> on SFM_CAMERA variables (no smart_calib table, or -1),
// SmartProjectionPoseFactor<Cal3_S2> and SmartProjectionRigFactor<PinholePose<Cal3_S2>> on POSE3 variables.  Key = variable id; factors in
// the order smart, between, prior.  One noise-model object per row of the noise table and one calibration object per row of the calib
// table; the rig-type factors share ONE CameraSet (a camera per distinct (calib row, sensor row) pair, in first-appearance order).
// smart_params[8 i + 7] > 0: useLOST, with the triangulation noise model Isotropic::Sigma(2, that value) unless it is the 1e-4 the
// reference uses without a model.
#pragma once
#include <gtsam/geometry/Cal3Bundler.h>
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/geometry/PinholeCamera.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/Values.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/SmartProjectionFactor.h>
#include <gtsam/slam/SmartProjectionPoseFactor.h>
#include <gtsam/slam/SmartProjectionRigFactor.h>

#include <fstream>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

namespace smart_lost_text {
using namespace gtsam;

inline Pose3 pose(const double* p) {
  Matrix3 R;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R(i, j) = p[3 * i + j];
  return Pose3(Rot3(R), Point3(p[9], p[10], p[11]));
}

typedef PinholeCamera<Cal3Bundler> SfmCamera;
inline SfmCamera camera(const double* p) { return SfmCamera(pose(p), Cal3Bundler(p[12], p[13], p[14], p[15], p[16])); }

struct Graph { NonlinearFactorGraph graph; Values initial; size_t n_smart = 0, n_rig = 0, n_camera = 0, n_lost = 0; };

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
    else if ((int)vt[v] == 1) { out.initial.insert(Key(v), camera(&values[at])); at += 17; }
    else { out.initial.insert(Key(v), Point3(values[at], values[at + 1], values[at + 2])); at += 3; }
  }
  std::vector<SharedNoiseModel> noise(t.at("noise_kind").size());
  for (size_t i = 0; i < noise.size(); i++) {
    const int kind = I("noise_kind", i), dim = I("noise_dim", i);
    const double* d = t.at("noise_data").data() + (size_t)t.at("noise_off")[i];
    if (kind == 0) noise[i] = noiseModel::Unit::Create(dim);
    else if (kind == 1) noise[i] = noiseModel::Isotropic::Sigma(dim, d[0], false);
    else if (kind == 2) noise[i] = noiseModel::Diagonal::Sigmas(Eigen::Map<const Vector>(d, dim), false);
    else { Matrix R(dim, dim); for (int r = 0; r < dim; r++) for (int c = 0; c < dim; c++) R(r, c) = d[r * dim + c]; noise[i] = noiseModel::Gaussian::SqrtInformation(R, false); }
  }
  const size_t n_calib = has("calib") ? t.at("calib").size() / 5 : 0;
  std::vector<std::shared_ptr<Cal3_S2>> Ks(n_calib);
  for (size_t k = 0; k < n_calib; k++) { const double* c = &t.at("calib")[5 * k]; Ks[k] = std::make_shared<Cal3_S2>(c[0], c[1], c[2], c[3], c[4]); }
  auto sensorOf = [&](const char* tab, size_t i) { std::optional<Pose3> s; if (has(tab) && I(tab, i) >= 0) s = pose(&t.at("sensor")[12 * (size_t)I(tab, i)]); return s; };
  out.n_smart = has("smart_noise") ? t.at("smart_noise").size() : 0;
  typedef SmartProjectionRigFactor<PinholePose<Cal3_S2>> Rig;
  auto rig = std::make_shared<Rig::Cameras>();
  std::map<std::pair<int, int>, size_t> cam_id;
  auto calibOf = [&](size_t i) { return has("smart_calib") ? I("smart_calib", i) : -1; };
  for (size_t i = 0; i < out.n_smart; i++) {
    if (calibOf(i) != -2) continue;
    for (size_t k = (size_t)t.at("smart_ptr")[i]; k < (size_t)t.at("smart_ptr")[i + 1]; k++) {
      const std::pair<int, int> key(I("smart_meas_calib", k), I("smart_meas_sensor", k));
      if (cam_id.count(key)) continue;
      cam_id[key] = rig->size();
      rig->emplace_back(key.second >= 0 ? pose(&t.at("sensor")[12 * (size_t)key.second]) : Pose3(), Ks.at((size_t)key.first));
    }
  }
  for (size_t i = 0; i < out.n_smart; i++) {
    const double* sp = &t.at("smart_params")[8 * i];
    const LinearizationMode lm = sp[5] == 1.0 ? IMPLICIT_SCHUR : (sp[5] == 2.0 ? JACOBIAN_Q : (sp[5] == 3.0 ? JACOBIAN_SVD : HESSIAN));
    SmartProjectionParams params(lm, sp[4] == 1.0 ? ZERO_ON_DEGENERACY : (sp[4] == 2.0 ? HANDLE_INFINITY : IGNORE_DEGENERACY), false, false, sp[3]);
    params.setRankTolerance(sp[0]); params.setEnableEPI(sp[6] != 0.0);
    params.setLandmarkDistanceThreshold(sp[1]); params.setDynamicOutlierRejectionThreshold(sp[2]);
    if (sp[7] > 0.0) {
      params.triangulation.useLOST = true;
      if (sp[7] != 1e-4) params.triangulation.noiseModel = noiseModel::Isotropic::Sigma(2, sp[7], false);
      out.n_lost++;
    }
    if (calibOf(i) == -1) {
      auto f = std::make_shared<SmartProjectionFactor<SfmCamera>>(noise[I("smart_noise", i)], params);
      for (size_t k = (size_t)t.at("smart_ptr")[i]; k < (size_t)t.at("smart_ptr")[i + 1]; k++)
        f->add(Point2(t.at("smart_z")[2 * k], t.at("smart_z")[2 * k + 1]), Key(I("smart_cam", k)));
      out.graph.push_back(f);
      out.n_camera++;
      continue;
    }
    if (calibOf(i) == -2) {
      auto f = std::make_shared<Rig>(noise[I("smart_noise", i)], rig, params);
      for (size_t k = (size_t)t.at("smart_ptr")[i]; k < (size_t)t.at("smart_ptr")[i + 1]; k++)
        f->add(Point2(t.at("smart_z")[2 * k], t.at("smart_z")[2 * k + 1]), Key(I("smart_cam", k)), cam_id.at({I("smart_meas_calib", k), I("smart_meas_sensor", k)}));
      out.graph.push_back(f);
      out.n_rig++;
      continue;
    }
    auto f = std::make_shared<SmartProjectionPoseFactor<Cal3_S2>>(noise[I("smart_noise", i)], Ks.at((size_t)I("smart_calib", i)), sensorOf("smart_sensor", i), params);
    for (size_t k = (size_t)t.at("smart_ptr")[i]; k < (size_t)t.at("smart_ptr")[i + 1]; k++)
      f->add(Point2(t.at("smart_z")[2 * k], t.at("smart_z")[2 * k + 1]), Key(I("smart_cam", k)));
    out.graph.push_back(f);
  }
  for (size_t i = 0; has("between_v1") && i < t.at("between_v1").size(); i++)
    out.graph.emplace_shared<BetweenFactor<Pose3>>(Key(I("between_v1", i)), Key(I("between_v2", i)), pose(&t.at("between_z")[12 * i]), noise[I("between_noise", i)]);
  for (size_t i = 0; has("prior_var") && i < t.at("prior_var").size(); i++) {
    const int v = I("prior_var", i);
    const double* d = &t.at("prior_data")[(size_t)t.at("prior_off")[i]];
    if ((int)vt[v] == 0) out.graph.addPrior(Key(v), pose(d), noise[I("prior_noise", i)]);
    else if ((int)vt[v] == 1) out.graph.addPrior(Key(v), camera(d), noise[I("prior_noise", i)]);
    else out.graph.addPrior(Key(v), Point3(d[0], d[1], d[2]), noise[I("prior_noise", i)]);
  }
  return out;
}
}  // namespace smart_lost_text
