// tests/golden/make_golden_smart_rig.cpp -- reference answers for graphs with SmartProjectionRigFactor<PinholePose<Cal3_S2>> (beside
// SmartProjectionPoseFactor<Cal3_S2>, projection, between and prior factors), computed by the real reference (oracle/_ref).  A small
// extern "C" library driven by tests/golden/make_golden_smart_rig.py through ctypes, after the pattern of make_golden_smart_pose.cpp: it
// builds the reference's NonlinearFactorGraph from a gtg_problem (smart_calib == GTG_SMART_RIG with the smart_meas_calib /
// smart_meas_sensor tables included) and answers error / per-factor triangulation / Hessian diagonal / damped solves / retract / the LM
// trajectories.  The graph's rig factors share ONE CameraSet: a camera per distinct (calib row, sensor row) pair, in first-appearance order.
// Variables are POSE3 and POINT3 only; keys are the variable ids, so Values order = id order.
// Factors are inserted in the order: smart, projection, between, prior.  Every probe builds a FRESH graph: a smart factor caches its
// triangulation (SmartProjectionFactor.h:127-183), and no probe may see what another left behind.
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/geometry/Pose3.h>
#include <gtsam/linear/GaussianFactorGraph.h>
#include <gtsam/linear/NoiseModel.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/internal/LevenbergMarquardtState.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/ProjectionFactor.h>
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

// a deep copy of the tables a graph is built from
struct Tables {
  std::vector<int> var_type, noise_kind, noise_dim;
  std::vector<int64_t> noise_off, smart_ptr, prior_off;
  std::vector<double> noise_data, proj_z, calib, sensor, between_z, prior_data, smart_z, smart_params;
  std::vector<int> proj_pose, proj_point, proj_noise, proj_calib, proj_sensor, between_v1, between_v2, between_noise, prior_var, prior_noise,
      smart_cam, smart_noise, smart_calib, smart_sensor, smart_meas_calib, smart_meas_sensor;
};
template <class T, class S> void copyTo(std::vector<T>& v, const S* p, size_t n) { v.clear(); if (p) v.assign(p, p + n); }

struct Ref {
  Tables t;
  int n_vars = 0;
  std::vector<int64_t> val_off, dim_off;
  int64_t val_size = 0, dim_size = 0;
  int dimOf(int i) const { return t.var_type[i] == GTG_VAR_POSE3 ? 6 : 3; }
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
      if (t.smart_calib[i] != GTG_SMART_RIG) continue;
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
    for (size_t i = 0; i < t.proj_pose.size(); i++)
      g.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3_S2>>(Point2(t.proj_z[2 * i], t.proj_z[2 * i + 1]), noise(t.proj_noise[i]),
          Key(t.proj_pose[i]), Key(t.proj_point[i]), K(t.proj_calib[i]), sensorOf(t.proj_sensor.empty() ? -1 : t.proj_sensor[i]));
    for (size_t i = 0; i < t.between_v1.size(); i++)
      g.emplace_shared<BetweenFactor<Pose3>>(Key(t.between_v1[i]), Key(t.between_v2[i]), unpackPose(t.between_z.data() + 12 * i), noise(t.between_noise[i]));
    for (size_t i = 0; i < t.prior_var.size(); i++) {
      const int v = t.prior_var[i];
      const double* d = t.prior_data.data() + t.prior_off[i];
      if (t.var_type[v] == GTG_VAR_POSE3) g.addPrior(Key(v), unpackPose(d), noise(t.prior_noise[i]));
      else g.addPrior(Key(v), Point3(d[0], d[1], d[2]), noise(t.prior_noise[i]));
    }
    return g;
  }
  Values unpack(const double* v) const {
    Values vals;
    for (int i = 0; i < n_vars; i++) {
      const double* p = v + val_off[i];
      if (t.var_type[i] == GTG_VAR_POSE3) vals.insert(Key(i), unpackPose(p)); else vals.insert(Key(i), Point3(p[0], p[1], p[2]));
    }
    return vals;
  }
  void pack(const Values& vals, double* v) const {
    for (int i = 0; i < n_vars; i++) {
      double* p = v + val_off[i];
      if (t.var_type[i] == GTG_VAR_POSE3) packPose(vals.at<Pose3>(Key(i)), p);
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

void* srref_create(const gtg_problem* p) {
  try {
    auto* g = new Ref;
    Tables& t = g->t;
    g->n_vars = p->n_vars;
    copyTo(t.var_type, p->var_type, p->n_vars);
    for (int i = 0; i < p->n_vars; i++) {
      if (p->var_type[i] != GTG_VAR_POSE3 && p->var_type[i] != GTG_VAR_POINT3) throw std::invalid_argument("POSE3 / POINT3 only");
      g->val_off.push_back(g->val_size); g->dim_off.push_back(g->dim_size);
      g->val_size += p->var_type[i] == GTG_VAR_POSE3 ? 12 : 3; g->dim_size += g->dimOf(i);
    }
    if (p->n_sfm || p->n_stereo || p->calib_distortion) throw std::invalid_argument("smart rig fixtures: projection / between / prior / smart tables only");
    copyTo(t.noise_kind, p->noise_kind, p->n_noise); copyTo(t.noise_dim, p->noise_dim, p->n_noise); copyTo(t.noise_off, p->noise_off, p->n_noise);
    size_t nd = 0;
    for (int i = 0; i < p->n_noise; i++) {
      const int k = p->noise_kind[i], d = p->noise_dim[i];
      if (p->noise_robust && p->noise_robust[i] != GTG_ROBUST_NONE) throw std::invalid_argument("no robust models in these fixtures");
      nd = std::max(nd, (size_t)p->noise_off[i] + (k == GTG_NOISE_UNIT ? 0 : k == GTG_NOISE_ISOTROPIC ? 1 : k == GTG_NOISE_DIAGONAL ? d : d * d));
    }
    copyTo(t.noise_data, p->noise_data, nd);
    copyTo(t.proj_pose, p->proj_pose, p->n_proj); copyTo(t.proj_point, p->proj_point, p->n_proj); copyTo(t.proj_noise, p->proj_noise, p->n_proj);
    copyTo(t.proj_calib, p->proj_calib, p->n_proj); copyTo(t.proj_sensor, p->proj_sensor, p->n_proj); copyTo(t.proj_z, p->proj_z, 2 * p->n_proj);
    copyTo(t.calib, p->calib, 5 * (size_t)p->n_calib); copyTo(t.sensor, p->sensor, 12 * (size_t)p->n_sensor);
    copyTo(t.between_v1, p->between_v1, p->n_between); copyTo(t.between_v2, p->between_v2, p->n_between);
    copyTo(t.between_noise, p->between_noise, p->n_between); copyTo(t.between_z, p->between_z, 12 * p->n_between);
    copyTo(t.prior_var, p->prior_var, p->n_prior); copyTo(t.prior_noise, p->prior_noise, p->n_prior); copyTo(t.prior_off, p->prior_off, p->n_prior);
    size_t np = 0;
    for (int64_t i = 0; i < p->n_prior; i++) np = std::max(np, (size_t)p->prior_off[i] + (p->var_type[p->prior_var[i]] == GTG_VAR_POSE3 ? 12 : 3));
    copyTo(t.prior_data, p->prior_data, np);
    if (p->n_smart > 0) {
      if (!p->smart_calib) throw std::invalid_argument("pose-type and rig-type smart factors only (smart_calib missing)");
      copyTo(t.smart_ptr, p->smart_ptr, p->n_smart + 1);
      const size_t nm = (size_t)p->smart_ptr[p->n_smart];
      copyTo(t.smart_cam, p->smart_cam, nm); copyTo(t.smart_z, p->smart_z, 2 * nm); copyTo(t.smart_noise, p->smart_noise, p->n_smart);
      copyTo(t.smart_params, p->smart_params, 8 * p->n_smart); copyTo(t.smart_calib, p->smart_calib, p->n_smart);
      copyTo(t.smart_sensor, p->smart_sensor, p->n_smart);
      copyTo(t.smart_meas_calib, p->smart_meas_calib, nm); copyTo(t.smart_meas_sensor, p->smart_meas_sensor, nm);
      for (int64_t i = 0; i < p->n_smart; i++) {
        if (p->smart_calib[i] == GTG_SMART_RIG ? t.smart_meas_calib.empty() || t.smart_meas_sensor.empty() : p->smart_calib[i] < 0)
          throw std::invalid_argument("pose-type and rig-type smart factors only");
      }
    }
    (void)g->graph();
    return g;
  } catch (const std::exception& e) { std::fprintf(stderr, "srref_create: %s\n", e.what()); return nullptr; }
}
void srref_destroy(void* h) { delete static_cast<Ref*>(h); }
int64_t srref_values_size(void* h) { return static_cast<Ref*>(h)->val_size; }
int64_t srref_tangent_size(void* h) { return static_cast<Ref*>(h)->dim_size; }

// NonlinearFactorGraph::error; *threw = 1 where the reference throws a CheiralityException (a failed track's point at infinity behind
// one of its cameras under HANDLE_INFINITY: CalibratedCamera.cpp:146-149, not caught by the smart factor)
double srref_error(void* h, const double* values, int* threw) {
  auto* g = static_cast<Ref*>(h);
  if (threw) *threw = 0;
  try { return g->graph().error(g->unpack(values)); }
  catch (const CheiralityException&) { if (threw) *threw = 1; return NAN; }
}
// 1: NonlinearFactorGraph::linearize throws a CheiralityException at these values, 0: it does not
int srref_linearize_throws(void* h, const double* values) {
  auto* g = static_cast<Ref*>(h);
  try { (void)g->graph().linearize(g->unpack(values)); return 0; }
  catch (const CheiralityException&) { return 1; }
}

// per smart factor: TriangulationResult::status (VALID 0, DEGENERATE 1, BEHIND_CAMERA 2, OUTLIER 3, FAR_POINT 4) and the point (zeros
// without one) of SmartProjectionFactor::point(values) on a fresh factor
int srref_triangulate(void* h, const double* values, int32_t* status, double* points) {
  auto* g = static_cast<Ref*>(h);
  const NonlinearFactorGraph graph = g->graph();
  const Values vals = g->unpack(values);
  for (size_t i = 0; i < g->t.smart_noise.size(); i++) {
    TriangulationResult r;
    if (auto f = std::dynamic_pointer_cast<SmartPose>(graph[i])) r = f->point(vals);
    else if (auto f2 = std::dynamic_pointer_cast<SmartRig>(graph[i])) r = f2->point(vals);
    else return -1;
    status[i] = (int32_t)r.status;
    for (int k = 0; k < 3; k++) points[3 * i + k] = r ? (*r)(k) : 0.0;
  }
  return 0;
}

// GaussianFactorGraph::hessianDiagonal, variable id order
int srref_hessian_diagonal(void* h, const double* values, double* hd) {
  auto* g = static_cast<Ref*>(h);
  try {
    auto lin = g->graph().linearize(g->unpack(values));
    g->packDelta(lin->hessianDiagonal(), hd);
  } catch (const CheiralityException&) { return -9; }
  return 0;
}

// What a diagonal that treats every sighting as a camera of its own lies above the reference's (which lives on the unique keys): per
// rig factor with a point, from the reference's own whitened blocks, diag((sum_a G_a) P (sum_a G_a)^T - sum_a G_a P G_a^T) with
// G_a = F_a^T E_a over the sightings a of one pose key; variable id order, zero elsewhere
int srref_cross_terms(void* h, const double* values, double* cross) {
  auto* g = static_cast<Ref*>(h);
  const NonlinearFactorGraph graph = g->graph();
  const Values vals = g->unpack(values);
  for (int64_t k = 0; k < g->dim_size; k++) cross[k] = 0.0;
  for (size_t i = 0; i < g->t.smart_noise.size(); i++) {
    auto f = std::dynamic_pointer_cast<SmartRig>(graph[i]);
    if (!f) continue;
    const SmartRig::Cameras cameras = f->cameras(vals);
    if (!f->triangulateSafe(cameras)) continue;
    SmartRig::FBlocks Fs; Matrix E; Vector b;
    f->computeJacobiansWithTriangulatedPoint(Fs, E, b, cameras);
    const SharedNoiseModel model = g->noise(g->t.smart_noise[i]);
    model->WhitenSystem(E, b);
    for (auto& F : Fs) F = model->Whiten(F);
    const Matrix3 P = SmartRig::Cameras::PointCov(E);
    std::map<Key, Matrix> sum;   // 6 x 3 per unique key
    const KeyVector& keys = f->nonUniqueKeys();
    for (size_t a = 0; a < keys.size(); a++) {
      const Matrix G = Fs[a].transpose() * E.block(2 * a, 0, 2, 3);
      if (!sum.count(keys[a])) sum[keys[a]] = Matrix::Zero(6, 3);
      sum[keys[a]] += G;
      const Matrix own = G * P * G.transpose();
      for (int r = 0; r < 6; r++) cross[g->dim_off[keys[a]] + r] -= own(r, r);
    }
    for (const auto& [key, G] : sum) {
      const Matrix all = G * P * G.transpose();
      for (int r = 0; r < 6; r++) cross[g->dim_off[key] + r] += all(r, r);
    }
  }
  return 0;
}

// One tryLambda body up to the linear errors (LevenbergMarquardtOptimizer.cpp:121-190): buildDampedSystem + optimize with a
// COLAMD ordering (reversed: the same ordering back to front).  Returns 1 on IndeterminantLinearSystemException, -9 where linearize
// throws a CheiralityException.
int srref_solve(void* h, const double* values, double lambda, int diagonal_damping, double min_diag, double max_diag, int reversed,
                double* delta, double* lin_err) {
  auto* g = static_cast<Ref*>(h);
  const NonlinearFactorGraph graph = g->graph();
  const Values vals = g->unpack(values);
  GaussianFactorGraph::shared_ptr lin;
  try { lin = graph.linearize(vals); } catch (const CheiralityException&) { return -9; }
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

int srref_retract(void* h, const double* values, const double* delta, double* out) {
  auto* g = static_cast<Ref*>(h);
  g->pack(g->unpack(values).retract(g->unpackDelta(delta)), out);
  return 0;
}

// The reference's LM with the Ceres (ceres = 1) or the legacy default LevenbergMarquardtParams and a COLAMD ordering (reversed: back to
// front), the loop of NonlinearOptimizer::defaultOptimize (nonlinear/NonlinearOptimizer.cpp:62-117) around iterate() so that every
// outer iteration is recorded.  trace rows: [inner iterations, error, lambda].  Returns the outer iteration count, -9 where the run
// throws a CheiralityException.
int srref_lm(void* h, const double* values0, int ceres, int reversed, double* values_out, int max_trace, double* trace, int* n_trace) {
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
  } catch (const CheiralityException&) { *n_trace = 0; return -9; }
}

}  // extern "C"
