// tests/golden/make_golden_smart_lost.cpp -- reference answers for smart-factor graphs with TriangulationParameters::useLOST, computed by
// the real reference (oracle/_ref).  A small extern "C" library driven by tests/golden/make_golden_smart_lost.py through ctypes, after the
// pattern of make_golden_smart_rig.cpp: it builds the reference's NonlinearFactorGraph from a gtg_problem -- smart factors of all three
// kinds (SmartProjectionFactor<PinholeCamera<Cal3Bundler>> on SFM_CAMERA variables, SmartProjectionPoseFactor<Cal3_S2> and
// SmartProjectionRigFactor<PinholePose<Cal3_S2>> on POSE3 variables), between factors and priors -- and answers error / per-factor
// triangulation / Hessian diagonal / damped solves / retract / the LM trajectories.  smart_params[8 i + 7] > 0 sets useLOST on factor i,
// with a triangulation noise model Isotropic::Sigma(2, that value) unless it is the 1e-4 the reference uses without a model.
// slost_system rebuilds the LOST system of every such track outside the reference (the formula of geometry/triangulation.cpp:86-147
// written out here, on the reference's own cameras and calibrated measurements), checks that it reproduces triangulateLOST's point and
// reports the pivots of its column-pivoted QR and how far apart the column norms were at every pivot choice.
// Keys are the variable ids, so Values order = id order.  Factors are inserted in the order: smart, between, prior.  Every probe builds a
// FRESH graph: a smart factor caches its triangulation (SmartProjectionFactor.h:127-183), and no probe may see what another left behind.
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/geometry/Cal3Bundler.h>
#include <gtsam/geometry/PinholeCamera.h>
#include <gtsam/geometry/Pose3.h>
#include <gtsam/geometry/triangulation.h>
#include <gtsam/linear/GaussianFactorGraph.h>
#include <gtsam/linear/NoiseModel.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/internal/LevenbergMarquardtState.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/SmartProjectionFactor.h>
#include <gtsam/slam/SmartProjectionPoseFactor.h>
#include <gtsam/slam/SmartProjectionRigFactor.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <optional>
#include <vector>

#include "gtsam_amd.h"

using namespace gtsam;

namespace {
typedef SmartProjectionPoseFactor<Cal3_S2> SmartPose;
typedef SmartProjectionRigFactor<PinholePose<Cal3_S2>> SmartRig;
typedef PinholeCamera<Cal3Bundler> SfmCamera;
typedef SmartProjectionFactor<SfmCamera> SmartCam;

SfmCamera unpackCamera(const double* p);
void packCamera(const SfmCamera& c, double* p);

Pose3 unpackPose(const double* p) {
  Matrix3 R;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R(i, j) = p[3 * i + j];
  return Pose3(Rot3(R), Point3(p[9], p[10], p[11]));
}
void packPose(const Pose3& T, double* p) {
  const Matrix3 R = T.rotation().matrix();
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) p[3 * i + j] = R(i, j);
  p[9] = T.x(); p[10] = T.y(); p[11] = T.z();
}

SfmCamera unpackCamera(const double* p) { return SfmCamera(unpackPose(p), Cal3Bundler(p[12], p[13], p[14], p[15], p[16])); }
void packCamera(const SfmCamera& c, double* p) {
  packPose(c.pose(), p);
  p[12] = c.calibration().fx(); p[13] = c.calibration().k1(); p[14] = c.calibration().k2(); p[15] = c.calibration().px(); p[16] = c.calibration().py();
}

// a deep copy of the tables a graph is built from
struct Tables {
  std::vector<int> var_type, noise_kind, noise_dim;
  std::vector<int64_t> noise_off, smart_ptr, prior_off;
  std::vector<double> noise_data, calib, sensor, between_z, prior_data, smart_z, smart_params;
  std::vector<int> between_v1, between_v2, between_noise, prior_var, prior_noise,
      smart_cam, smart_noise, smart_calib, smart_sensor, smart_meas_calib, smart_meas_sensor;
};
template <class T, class S> void copyTo(std::vector<T>& v, const S* p, size_t n) { v.clear(); if (p) v.assign(p, p + n); }

struct Ref {
  Tables t;
  int n_vars = 0;
  std::vector<int64_t> val_off, dim_off;
  int64_t val_size = 0, dim_size = 0;
  int dimOf(int i) const { return t.var_type[i] == GTG_VAR_POSE3 ? 6 : (t.var_type[i] == GTG_VAR_SFM_CAMERA ? 9 : 3); }
  int sizeOf(int i) const { return t.var_type[i] == GTG_VAR_POSE3 ? 12 : (t.var_type[i] == GTG_VAR_SFM_CAMERA ? 17 : 3); }
  bool cameraType(size_t i) const { return t.smart_calib.empty() || t.smart_calib[i] == -1; }
  SharedNoiseModel noise(int idx) const {
    const int kind = t.noise_kind[idx], dim = t.noise_dim[idx];
    const double* d = t.noise_data.data() + t.noise_off[idx];
    if (kind == GTG_NOISE_UNIT) return noiseModel::Unit::Create(dim);
    if (kind == GTG_NOISE_ISOTROPIC) return noiseModel::Isotropic::Sigma(dim, d[0], false);
    if (kind == GTG_NOISE_DIAGONAL) return noiseModel::Diagonal::Sigmas(Eigen::Map<const Vector>(d, dim), false);
    Matrix R(dim, dim);
    for (int i = 0; i < dim; i++) for (int j = 0; j < dim; j++) R(i, j) = d[i * dim + j];
    return noiseModel::Gaussian::SqrtInformation(R, false);
  }
  std::optional<Pose3> sensorOf(int si) const {
    std::optional<Pose3> s;
    if (si >= 0) s = unpackPose(t.sensor.data() + 12 * si);
    return s;
  }
  NonlinearFactorGraph graph() const {
    NonlinearFactorGraph g;
    std::map<int, std::shared_ptr<Cal3_S2>> Ks;   // one shared calibration object per table entry, as user code has it
    auto K = [&](int ci) {
      auto& k = Ks[ci];
      if (!k) { const double* c = t.calib.data() + 5 * ci; k = std::make_shared<Cal3_S2>(c[0], c[1], c[2], c[3], c[4]); }
      return k;
    };
    // the rig: one camera per distinct (calib row, sensor row) of the rig-type measurements
    auto rig = std::make_shared<CameraSet<PinholePose<Cal3_S2>>>();
    std::map<std::pair<int, int>, size_t> cam_id;
    for (size_t i = 0; i < t.smart_noise.size(); i++) {
      if (cameraType(i) || t.smart_calib[i] != GTG_SMART_RIG) continue;
      for (int64_t k = t.smart_ptr[i]; k < t.smart_ptr[i + 1]; k++) {
        const std::pair<int, int> key(t.smart_meas_calib[k], t.smart_meas_sensor[k]);
        if (cam_id.count(key)) continue;
        cam_id[key] = rig->size();
        rig->emplace_back(key.second >= 0 ? unpackPose(t.sensor.data() + 12 * key.second) : Pose3(), K(key.first));
      }
    }
    for (size_t i = 0; i < t.smart_noise.size(); i++) {
      const double* sp = t.smart_params.data() + 8 * i;
      const LinearizationMode lm = sp[5] == 1.0 ? IMPLICIT_SCHUR : (sp[5] == 2.0 ? JACOBIAN_Q : (sp[5] == 3.0 ? JACOBIAN_SVD : HESSIAN));
      SmartProjectionParams params(lm, sp[4] == 1.0 ? ZERO_ON_DEGENERACY : (sp[4] == 2.0 ? HANDLE_INFINITY : IGNORE_DEGENERACY), false, false, sp[3]);
      params.setRankTolerance(sp[0]);
      params.setEnableEPI(sp[6] != 0.0);
      params.setLandmarkDistanceThreshold(sp[1]);
      params.setDynamicOutlierRejectionThreshold(sp[2]);
      if (sp[7] > 0.0) {
        params.triangulation.useLOST = true;
        if (sp[7] != 1e-4) params.triangulation.noiseModel = noiseModel::Isotropic::Sigma(2, sp[7], false);
      }
      if (cameraType(i)) {
        auto f = std::make_shared<SmartCam>(noise(t.smart_noise[i]), params);
        for (int64_t k = t.smart_ptr[i]; k < t.smart_ptr[i + 1]; k++) f->add(Point2(t.smart_z[2 * k], t.smart_z[2 * k + 1]), Key(t.smart_cam[k]));
        g.push_back(f);
        continue;
      }
      if (t.smart_calib[i] == GTG_SMART_RIG) {
        auto f = std::make_shared<SmartRig>(noise(t.smart_noise[i]), rig, params);
        for (int64_t k = t.smart_ptr[i]; k < t.smart_ptr[i + 1]; k++)
          f->add(Point2(t.smart_z[2 * k], t.smart_z[2 * k + 1]), Key(t.smart_cam[k]), cam_id.at({t.smart_meas_calib[k], t.smart_meas_sensor[k]}));
        g.push_back(f);
        continue;
      }
      auto f = std::make_shared<SmartPose>(noise(t.smart_noise[i]), K(t.smart_calib[i]), sensorOf(t.smart_sensor.empty() ? -1 : t.smart_sensor[i]), params);
      for (int64_t k = t.smart_ptr[i]; k < t.smart_ptr[i + 1]; k++) f->add(Point2(t.smart_z[2 * k], t.smart_z[2 * k + 1]), Key(t.smart_cam[k]));
      g.push_back(f);
    }
    for (size_t i = 0; i < t.between_v1.size(); i++)
      g.emplace_shared<BetweenFactor<Pose3>>(Key(t.between_v1[i]), Key(t.between_v2[i]), unpackPose(t.between_z.data() + 12 * i), noise(t.between_noise[i]));
    for (size_t i = 0; i < t.prior_var.size(); i++) {
      const int v = t.prior_var[i];
      const double* d = t.prior_data.data() + t.prior_off[i];
      if (t.var_type[v] == GTG_VAR_POSE3) g.addPrior(Key(v), unpackPose(d), noise(t.prior_noise[i]));
      else if (t.var_type[v] == GTG_VAR_SFM_CAMERA) g.addPrior(Key(v), unpackCamera(d), noise(t.prior_noise[i]));
      else g.addPrior(Key(v), Point3(d[0], d[1], d[2]), noise(t.prior_noise[i]));
    }
    return g;
  }
  Values unpack(const double* v) const {
    Values vals;
    for (int i = 0; i < n_vars; i++) {
      const double* p = v + val_off[i];
      if (t.var_type[i] == GTG_VAR_POSE3) vals.insert(Key(i), unpackPose(p));
      else if (t.var_type[i] == GTG_VAR_SFM_CAMERA) vals.insert(Key(i), unpackCamera(p));
      else vals.insert(Key(i), Point3(p[0], p[1], p[2]));
    }
    return vals;
  }
  void pack(const Values& vals, double* v) const {
    for (int i = 0; i < n_vars; i++) {
      double* p = v + val_off[i];
      if (t.var_type[i] == GTG_VAR_POSE3) packPose(vals.at<Pose3>(Key(i)), p);
      else if (t.var_type[i] == GTG_VAR_SFM_CAMERA) packCamera(vals.at<SfmCamera>(Key(i)), p);
      else { const Point3 q = vals.at<Point3>(Key(i)); p[0] = q.x(); p[1] = q.y(); p[2] = q.z(); }
    }
  }
  void packDelta(const VectorValues& vv, double* d) const {
    for (int i = 0; i < n_vars; i++) { const Vector& v = vv.at(Key(i)); for (int k = 0; k < dimOf(i); k++) d[dim_off[i] + k] = v(k); }
  }
  VectorValues unpackDelta(const double* d) const {
    VectorValues vv;
    for (int i = 0; i < n_vars; i++) vv.insert(Key(i), Eigen::Map<const Vector>(d + dim_off[i], dimOf(i)));
    return vv;
  }
  static Ordering ordering(const NonlinearFactorGraph& g, int reversed) {
    Ordering o = Ordering::Create(Ordering::COLAMD, g);
    if (reversed) std::reverse(o.begin(), o.end());
    return o;
  }
};
}  // namespace

extern "C" {

void* slost_create(const gtg_problem* p) {
  try {
    auto* g = new Ref;
    Tables& t = g->t;
    g->n_vars = p->n_vars;
    copyTo(t.var_type, p->var_type, p->n_vars);
    for (int i = 0; i < p->n_vars; i++) {
      if (p->var_type[i] != GTG_VAR_POSE3 && p->var_type[i] != GTG_VAR_POINT3 && p->var_type[i] != GTG_VAR_SFM_CAMERA) throw std::invalid_argument("POSE3 / POINT3 / SFM_CAMERA only");
      g->val_off.push_back(g->val_size); g->dim_off.push_back(g->dim_size);
      g->val_size += g->sizeOf(i); g->dim_size += g->dimOf(i);
    }
    if (p->n_sfm || p->n_proj || p->n_stereo || p->calib_distortion) throw std::invalid_argument("smart LOST fixtures: between / prior / smart tables only");
    copyTo(t.noise_kind, p->noise_kind, p->n_noise); copyTo(t.noise_dim, p->noise_dim, p->n_noise); copyTo(t.noise_off, p->noise_off, p->n_noise);
    size_t nd = 0;
    for (int i = 0; i < p->n_noise; i++) {
      const int k = p->noise_kind[i], d = p->noise_dim[i];
      if (p->noise_robust && p->noise_robust[i] != GTG_ROBUST_NONE) throw std::invalid_argument("no robust models in these fixtures");
      nd = std::max(nd, (size_t)p->noise_off[i] + (k == GTG_NOISE_UNIT ? 0 : k == GTG_NOISE_ISOTROPIC ? 1 : k == GTG_NOISE_DIAGONAL ? d : d * d));
    }
    copyTo(t.noise_data, p->noise_data, nd);
    copyTo(t.calib, p->calib, 5 * (size_t)p->n_calib); copyTo(t.sensor, p->sensor, 12 * (size_t)p->n_sensor);
    copyTo(t.between_v1, p->between_v1, p->n_between); copyTo(t.between_v2, p->between_v2, p->n_between);
    copyTo(t.between_noise, p->between_noise, p->n_between); copyTo(t.between_z, p->between_z, 12 * p->n_between);
    copyTo(t.prior_var, p->prior_var, p->n_prior); copyTo(t.prior_noise, p->prior_noise, p->n_prior); copyTo(t.prior_off, p->prior_off, p->n_prior);
    size_t np = 0;
    for (int64_t i = 0; i < p->n_prior; i++) np = std::max(np, (size_t)p->prior_off[i] + (size_t)g->sizeOf(p->prior_var[i]));
    copyTo(t.prior_data, p->prior_data, np);
    if (p->n_smart > 0) {
      copyTo(t.smart_ptr, p->smart_ptr, p->n_smart + 1);
      const size_t nm = (size_t)p->smart_ptr[p->n_smart];
      copyTo(t.smart_cam, p->smart_cam, nm); copyTo(t.smart_z, p->smart_z, 2 * nm); copyTo(t.smart_noise, p->smart_noise, p->n_smart);
      copyTo(t.smart_params, p->smart_params, 8 * p->n_smart); copyTo(t.smart_calib, p->smart_calib, p->n_smart);
      copyTo(t.smart_sensor, p->smart_sensor, p->n_smart);
      copyTo(t.smart_meas_calib, p->smart_meas_calib, nm); copyTo(t.smart_meas_sensor, p->smart_meas_sensor, nm);
      for (int64_t i = 0; i < p->n_smart; i++) {
        if (p->smart_calib && p->smart_calib[i] == GTG_SMART_RIG && (t.smart_meas_calib.empty() || t.smart_meas_sensor.empty()))
          throw std::invalid_argument("a rig-type smart factor without the per-measurement tables");
      }
    }
    (void)g->graph();
    return g;
  } catch (const std::exception& e) { std::fprintf(stderr, "slost_create: %s\n", e.what()); return nullptr; }
}
void slost_destroy(void* h) { delete static_cast<Ref*>(h); }
int64_t slost_values_size(void* h) { return static_cast<Ref*>(h)->val_size; }
int64_t slost_tangent_size(void* h) { return static_cast<Ref*>(h)->dim_size; }

// NonlinearFactorGraph::error; *threw = 1 where the reference throws (a CheiralityException, or Cal3Bundler::calibrate not converging) (a failed track's point at infinity behind
// one of its cameras under HANDLE_INFINITY: CalibratedCamera.cpp:146-149, not caught by the smart factor)
double slost_error(void* h, const double* values, int* threw) {
  auto* g = static_cast<Ref*>(h);
  if (threw) *threw = 0;
  try { return g->graph().error(g->unpack(values)); }
  catch (const std::exception&) { if (threw) *threw = 1; return NAN; }
}
// 1: NonlinearFactorGraph::linearize throws (a CheiralityException, or Cal3Bundler::calibrate not converging) at these values, 0: it does not
int slost_linearize_throws(void* h, const double* values) {
  auto* g = static_cast<Ref*>(h);
  try { (void)g->graph().linearize(g->unpack(values)); return 0; }
  catch (const std::exception&) { return 1; }
}

// per smart factor: TriangulationResult::status (VALID 0, DEGENERATE 1, BEHIND_CAMERA 2, OUTLIER 3, FAR_POINT 4) and the point (zeros
// without one) of SmartProjectionFactor::point(values) on a fresh factor
int slost_triangulate(void* h, const double* values, int32_t* status, double* points) {
  auto* g = static_cast<Ref*>(h);
  const NonlinearFactorGraph graph = g->graph();
  const Values vals = g->unpack(values);
  try {
  for (size_t i = 0; i < g->t.smart_noise.size(); i++) {
    TriangulationResult r;
    if (auto f = std::dynamic_pointer_cast<SmartPose>(graph[i])) r = f->point(vals);
    else if (auto f2 = std::dynamic_pointer_cast<SmartRig>(graph[i])) r = f2->point(vals);
    else if (auto f3 = std::dynamic_pointer_cast<SmartCam>(graph[i])) r = f3->point(vals);
    else return -1;
    status[i] = (int32_t)r.status;
    for (int k = 0; k < 3; k++) points[3 * i + k] = r ? (*r)(k) : 0.0;
  }
  } catch (const std::exception&) { return -9; }   // (Cal3Bundler::calibrate not converging)
  return 0;
}
}  // extern "C"

namespace {
// The LOST system of one track, outside the reference: rows q_i skew(z_i)[0:2, :] R_i^T with q_i = |wZ_i x wZ_j| / (sigma |d_ij x wZ_j|)
// and the partner search of triangulation.cpp:97-139, on the poses and calibrated measurements given.  false: no partner (the
// reference throws TriangulationUnderconstrainedException there).
bool lostSystem(const std::vector<Pose3>& poses, const Point3Vector& zc, double sigma, Matrix* A, Vector* b) {
  const size_t m = zc.size();
  *A = Matrix::Zero(2 * m, 3); *b = Vector::Zero(2 * m);
  for (size_t i = 0; i < m; i++) {
    const Vector3 wZi = poses[i].rotation().matrix() * zc[i];
    double num = 0, den = 0;
    bool found = false;
    for (size_t k = 1; k < m && !found; k++) {
      const size_t j = (i + k) % m;
      const Vector3 wZj = poses[j].rotation().matrix() * zc[j];
      const Vector3 d = poses[j].translation() - poses[i].translation();
      num = wZi.cross(wZj).norm(); den = d.cross(wZj).norm();
      found = k == 1 ? !(num == 0 || den == 0) : (num > 0 && den > 0);
    }
    if (!found) return false;
    const double q = num / (sigma * den);
    Matrix23 S;
    S << 0.0, -zc[i].z(), zc[i].y(), zc[i].z(), 0.0, -zc[i].x();
    const Matrix23 C = q * S * poses[i].rotation().matrix().transpose();
    A->block<2, 3>(2 * i, 0) = C;
    b->segment<2>(2 * i) = C * poses[i].translation();
  }
  return true;
}
template <class FACTOR>
bool lostInputs(const std::shared_ptr<FACTOR>& f, const Values& vals, std::vector<Pose3>* poses, Point3Vector* zc) {
  if (!f) return false;
  const typename FACTOR::Cameras cameras = f->cameras(vals);
  for (const auto& c : cameras) poses->push_back(c.pose());
  try { *zc = calibrateMeasurements<typename FACTOR::Cameras::value_type>(cameras, f->measured()); }
  catch (const std::exception&) { zc->clear(); }   // (Cal3Bundler::calibrate not converging: reported by slost_system as -9)
  return true;
}
}  // namespace

extern "C" {
// Per smart factor with useLOST and at least two measurements: kind[i] = 0 the reference's triangulateLOST returns a point, 1 it throws
// with the system built (rank), 2 it throws and the partner search above failed; -1 a DLT factor or a single measurement.  For kind 0 / 1:
// pivots[3 i ..] = |R_11|, |R_22|, |R_33| of Eigen::ColPivHouseholderQR of the rebuilt matrix; gaps[2 i ..] = at the first and the second
// pivot choice, (largest - second largest) / largest of the remaining column norms (recomputed on the reflected matrix); mismatch[i] =
// for kind 0, the relative distance between the rebuilt system's solution and triangulateLOST's point.  Returns -1 on a factor of an
// unknown type.
int slost_system(void* h, const double* values, int32_t* kind, double* pivots, double* gaps, double* mismatch) {
  auto* g = static_cast<Ref*>(h);
  const NonlinearFactorGraph graph = g->graph();
  const Values vals = g->unpack(values);
  for (size_t i = 0; i < g->t.smart_noise.size(); i++) {
    const double* sp = g->t.smart_params.data() + 8 * i;
    kind[i] = -1; mismatch[i] = 0.0;
    for (int k = 0; k < 3; k++) pivots[3 * i + k] = 0.0;
    gaps[2 * i] = gaps[2 * i + 1] = 0.0;
    if (!(sp[7] > 0.0) || g->t.smart_ptr[i + 1] - g->t.smart_ptr[i] < 2) continue;
    std::vector<Pose3> poses; Point3Vector zc;
    if (!lostInputs(std::dynamic_pointer_cast<SmartPose>(graph[i]), vals, &poses, &zc) &&
        !lostInputs(std::dynamic_pointer_cast<SmartRig>(graph[i]), vals, &poses, &zc) &&
        !lostInputs(std::dynamic_pointer_cast<SmartCam>(graph[i]), vals, &poses, &zc)) return -1;
    if (zc.size() != poses.size()) return -9;
    bool threw = false;
    Point3 ref(0, 0, 0);
    try { ref = triangulateLOST(poses, zc, noiseModel::Isotropic::Sigma(2, sp[7], false), sp[0]); }
    catch (const TriangulationUnderconstrainedException&) { threw = true; }
    Matrix A; Vector b;
    if (!lostSystem(poses, zc, sp[7], &A, &b)) { kind[i] = 2; if (!threw) return -2; continue; }
    Eigen::ColPivHouseholderQR<Matrix> qr = A.colPivHouseholderQr();
    qr.setThreshold(sp[0]);
    for (int k = 0; k < 3; k++) pivots[3 * i + k] = std::abs(qr.matrixR()(k, k));
    if ((qr.rank() < 3) != threw) return -3;
    kind[i] = threw ? 1 : 0;
    if (!threw) { const Vector3 x = qr.solve(b); mismatch[i] = (x - ref).cwiseAbs().maxCoeff() / ref.cwiseAbs().maxCoeff(); }
    // the pivot choices on the reflected matrix, norms recomputed
    Matrix M = A;
    for (int k = 0; k < 2; k++) {
      const int rows = (int)M.rows() - k;
      std::vector<std::pair<double, int>> nrm;
      for (int c = k; c < 3; c++) nrm.emplace_back(M.col(c).tail(rows).norm(), c);
      std::sort(nrm.begin(), nrm.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
      gaps[2 * i + k] = nrm[0].first > 0 ? (nrm[0].first - nrm[1].first) / nrm[0].first : 0.0;
      M.col(k).swap(M.col(nrm[0].second));
      Vector ess(rows - 1), work(3);
      double tau, beta;
      M.col(k).tail(rows).makeHouseholder(ess, tau, beta);
      M.bottomRightCorner(rows, 3 - k).applyHouseholderOnTheLeft(ess, tau, work.data());
    }
  }
  return 0;
}

// GaussianFactorGraph::hessianDiagonal, variable id order
int slost_hessian_diagonal(void* h, const double* values, double* hd) {
  auto* g = static_cast<Ref*>(h);
  try {
    auto lin = g->graph().linearize(g->unpack(values));
    g->packDelta(lin->hessianDiagonal(), hd);
  } catch (const std::exception&) { return -9; }
  return 0;
}

// One tryLambda body up to the linear errors (LevenbergMarquardtOptimizer.cpp:121-190): buildDampedSystem + optimize with a
// COLAMD ordering (reversed: the same ordering back to front).  Returns 1 on IndeterminantLinearSystemException, -9 where linearize
// throws (a CheiralityException, or Cal3Bundler::calibrate not converging).
int slost_solve(void* h, const double* values, double lambda, int diagonal_damping, double min_diag, double max_diag, int reversed,
                double* delta, double* lin_err) {
  auto* g = static_cast<Ref*>(h);
  const NonlinearFactorGraph graph = g->graph();
  const Values vals = g->unpack(values);
  GaussianFactorGraph::shared_ptr lin;
  try { lin = graph.linearize(vals); } catch (const std::exception&) { return -9; }
  internal::LevenbergMarquardtState state(vals, 0.0, lambda, 10.0);
  GaussianFactorGraph damped;
  if (diagonal_damping) {
    VectorValues sq = lin->hessianDiagonal();
    for (auto& [key, value] : sq) value = value.cwiseMax(min_diag).cwiseMin(max_diag).cwiseSqrt();
    damped = state.buildDampedSystem(*lin, sq);
  } else {
    damped = state.buildDampedSystem(*lin);
  }
  try {
    VectorValues d = damped.optimize(Ref::ordering(graph, reversed), EliminatePreferCholesky);
    g->packDelta(d, delta);
    lin_err[0] = lin->error(VectorValues::Zero(d)); lin_err[1] = lin->error(d);
  } catch (const IndeterminantLinearSystemException&) { return 1; }
  return 0;
}

int slost_retract(void* h, const double* values, const double* delta, double* out) {
  auto* g = static_cast<Ref*>(h);
  g->pack(g->unpack(values).retract(g->unpackDelta(delta)), out);
  return 0;
}

// The reference's LM with the Ceres (ceres = 1) or the legacy default LevenbergMarquardtParams and a COLAMD ordering (reversed: back to
// front), the loop of NonlinearOptimizer::defaultOptimize (nonlinear/NonlinearOptimizer.cpp:62-117) around iterate() so that every
// outer iteration is recorded.  trace rows: [inner iterations, error, lambda].  Returns the outer iteration count, -9 where the run
// throws (a CheiralityException, or Cal3Bundler::calibrate not converging).
int slost_lm(void* h, const double* values0, int ceres, int reversed, double* values_out, int max_trace, double* trace, int* n_trace) {
  auto* g = static_cast<Ref*>(h);
  const NonlinearFactorGraph graph = g->graph();
  LevenbergMarquardtParams params = ceres ? LevenbergMarquardtParams::CeresDefaults() : LevenbergMarquardtParams::LegacyDefaults();
  params.ordering = Ref::ordering(graph, reversed);
  try {
  LevenbergMarquardtOptimizer lm(graph, g->unpack(values0), params);
  int nt = 0;
  auto rec = [&]() {
    if (nt < max_trace) { trace[3 * nt] = lm.getInnerIterations(); trace[3 * nt + 1] = lm.error(); trace[3 * nt + 2] = lm.lambda(); nt++; }
  };
  rec();
  double currentError = lm.error();
  if (!(currentError <= params.errorTol) && lm.iterations() < (size_t)params.maxIterations) {
    double newError = currentError;
    do {
      currentError = newError;
      lm.iterate();
      newError = lm.error();
      rec();
    } while (lm.iterations() < (size_t)params.maxIterations &&
             !checkConvergence(params.relativeErrorTol, params.absoluteErrorTol, params.errorTol, currentError, newError, params.verbosity) &&
             std::isfinite(currentError));
  }
  *n_trace = nt;
  g->pack(lm.values(), values_out);
  return (int)lm.iterations();
  } catch (const std::exception&) { *n_trace = 0; return -9; }
}

}  // extern "C"
