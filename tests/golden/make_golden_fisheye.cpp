// tests/golden/make_golden_fisheye.cpp -- reference answers for graphs with GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> beside
// the Cal3_S2 / Cal3DS2 instantiations, BetweenFactor<Pose3> and PriorFactors, computed by the real reference (oracle/_ref).  A small
// extern "C" library driven by tests/golden/make_golden_fisheye.py through ctypes, in the pattern of make_golden_sam3d.cpp: it builds the
// reference's NonlinearFactorGraph from a gtg_problem and the camera model of every calib row (what gtg_set_calibration_models takes)
// and answers error / per-factor Jacobians / Hessian diagonal / gradient / damped solves / retract / the LM trajectory / a probe of the
// fisheye factors.  Keys are the variable ids, so Values order = id order.  Factors are inserted in the order: projection, between, prior.
#include <gtsam/geometry/Cal3DS2.h>
#include <gtsam/geometry/Cal3Fisheye.h>
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/geometry/Cal3_S2Stereo.h>
#include <gtsam/geometry/Pose3.h>
#include <gtsam/geometry/StereoPoint2.h>
#include <gtsam/linear/GaussianFactorGraph.h>
#include <gtsam/linear/JacobianFactor.h>
#include <gtsam/linear/NoiseModel.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/internal/LevenbergMarquardtState.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/ProjectionFactor.h>
#include <gtsam/sam/BearingFactor.h>
#include <gtsam/sam/BearingRangeFactor.h>
#include <gtsam/sam/RangeFactor.h>
#include <gtsam/slam/StereoFactor.h>

#include <algorithm>
#include <cmath>
#include <optional>
#include <vector>

#include "gtsam_amd.h"

using namespace gtsam;

namespace {
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
SharedNoiseModel makeNoise(const gtg_problem* p, int idx) {
  const int kind = p->noise_kind[idx], dim = p->noise_dim[idx];
  const double* d = p->noise_data + p->noise_off[idx];
  SharedNoiseModel base;
  if (kind == GTG_NOISE_UNIT) base = noiseModel::Unit::Create(dim);
  else if (kind == GTG_NOISE_ISOTROPIC) base = noiseModel::Isotropic::Sigma(dim, d[0], false);
  else if (kind == GTG_NOISE_DIAGONAL) base = noiseModel::Diagonal::Sigmas(Eigen::Map<const Vector>(d, dim), false);
  else {
    Matrix R(dim, dim);
    for (int i = 0; i < dim; i++) for (int j = 0; j < dim; j++) R(i, j) = d[i * dim + j];
    base = noiseModel::Gaussian::SqrtInformation(R, false);
  }
  const int rk = p->noise_robust ? p->noise_robust[idx] : GTG_ROBUST_NONE;
  if (rk == GTG_ROBUST_NONE) return base;
  if (rk == GTG_ROBUST_HUBER) return noiseModel::Robust::Create(noiseModel::mEstimator::Huber::Create(p->noise_robust_param[idx]), base);
  if (rk == GTG_ROBUST_CAUCHY) return noiseModel::Robust::Create(noiseModel::mEstimator::Cauchy::Create(p->noise_robust_param[idx]), base);
  throw std::invalid_argument("make_golden_fisheye: only Huber and Cauchy are used by these fixtures");
}

struct FisheyeRef {
  int n_vars = 0;
  std::vector<int> var_type;
  std::vector<int64_t> val_off, dim_off;
  int64_t val_size = 0, dim_size = 0;
  NonlinearFactorGraph graph;
  size_t beg[6], end[6];   // factor ranges by GTG_FAC_*
  const gtg_problem* p = nullptr;       // the caller's tables, alive until fref_destroy
  std::vector<int32_t> calib_model;     // GTG_CALIB_* per calib row
  int dimOf(int i) const { return var_type[i] == GTG_VAR_POSE3 ? 6 : 3; }
  Values unpack(const double* v) const {
    Values vals;
    for (int i = 0; i < n_vars; i++) {
      const double* p = v + val_off[i];
      if (var_type[i] == GTG_VAR_POSE3) vals.insert(Key(i), unpackPose(p)); else vals.insert(Key(i), Point3(p[0], p[1], p[2]));
    }
    return vals;
  }
  void pack(const Values& vals, double* v) const {
    for (int i = 0; i < n_vars; i++) {
      double* p = v + val_off[i];
      if (var_type[i] == GTG_VAR_POSE3) packPose(vals.at<Pose3>(Key(i)), p);
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
  Ordering ordering(int reversed) const {
    Ordering o = Ordering::Create(Ordering::COLAMD, graph);
    if (reversed) std::reverse(o.begin(), o.end());
    return o;
  }
};
}  // namespace

extern "C" {

void* fref_create(const gtg_problem* p, const int32_t* calib_model) {
  try {
    auto* g = new FisheyeRef;
    g->n_vars = p->n_vars; g->p = p;
    g->calib_model.assign((size_t)p->n_calib, GTG_CALIB_PINHOLE);
    if (calib_model) g->calib_model.assign(calib_model, calib_model + p->n_calib);
    if (p->n_sfm || p->n_stereo || p->n_sam || p->n_smart || p->n_pose_partial || p->planar.n_sam2) throw std::invalid_argument("fisheye fixtures: projection / between / prior tables only");
    g->var_type.assign(p->var_type, p->var_type + p->n_vars);
    for (int i = 0; i < p->n_vars; i++) {
      if (p->var_type[i] != GTG_VAR_POSE3 && p->var_type[i] != GTG_VAR_POINT3) throw std::invalid_argument("POSE3 / POINT3 only");
      g->val_off.push_back(g->val_size); g->dim_off.push_back(g->dim_size);
      g->val_size += p->var_type[i] == GTG_VAR_POSE3 ? 12 : 3; g->dim_size += g->dimOf(i);
    }
    std::vector<SharedNoiseModel> noise(p->n_noise);
    for (int i = 0; i < p->n_noise; i++) noise[i] = makeNoise(p, i);
    auto sensorOf = [&](const int32_t* tab, int64_t i) {
      std::optional<Pose3> s;
      if (tab && tab[i] >= 0) s = unpackPose(p->sensor + 12 * tab[i]);
      return s;
    };
    g->beg[0] = g->end[0] = 0;
    g->beg[1] = g->graph.size();
    for (int64_t i = 0; i < p->n_proj; i++) {
      const double* c = p->calib + 5 * p->proj_calib[i];
      const double* d = p->calib_distortion ? p->calib_distortion + 4 * p->proj_calib[i] : nullptr;
      const Point2 z(p->proj_z[2 * i], p->proj_z[2 * i + 1]);
      if (g->calib_model[p->proj_calib[i]] == GTG_CALIB_FISHEYE)
        g->graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3Fisheye>>(z, noise[p->proj_noise[i]], Key(p->proj_pose[i]), Key(p->proj_point[i]),
            std::make_shared<Cal3Fisheye>(c[0], c[1], c[2], c[3], c[4], d[0], d[1], d[2], d[3]), sensorOf(p->proj_sensor, i));
      else if (d && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0 || d[3] != 0.0))
        g->graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3DS2>>(z, noise[p->proj_noise[i]], Key(p->proj_pose[i]), Key(p->proj_point[i]),
            std::make_shared<Cal3DS2>(c[0], c[1], c[2], c[3], c[4], d[0], d[1], d[2], d[3]), sensorOf(p->proj_sensor, i));
      else
        g->graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3_S2>>(z, noise[p->proj_noise[i]], Key(p->proj_pose[i]), Key(p->proj_point[i]),
            std::make_shared<Cal3_S2>(c[0], c[1], c[2], c[3], c[4]), sensorOf(p->proj_sensor, i));
    }
    g->end[1] = g->beg[2] = g->graph.size();
    g->beg[4] = g->end[4] = g->beg[5] = g->end[5] = 0;
    for (int64_t i = 0; i < p->n_between; i++)
      g->graph.emplace_shared<BetweenFactor<Pose3>>(Key(p->between_v1[i]), Key(p->between_v2[i]), unpackPose(p->between_z + 12 * i), noise[p->between_noise[i]]);
    g->end[2] = g->beg[3] = g->graph.size();
    for (int64_t i = 0; i < p->n_prior; i++) {
      const int v = p->prior_var[i];
      const double* d = p->prior_data + p->prior_off[i];
      if (p->var_type[v] == GTG_VAR_POSE3) g->graph.addPrior(Key(v), unpackPose(d), noise[p->prior_noise[i]]);
      else g->graph.addPrior(Key(v), Point3(d[0], d[1], d[2]), noise[p->prior_noise[i]]);
    }
    g->end[3] = g->graph.size();
    return g;
  } catch (const std::exception& e) { std::fprintf(stderr, "fref_create: %s\n", e.what()); return nullptr; }
}
void fref_destroy(void* h) { delete static_cast<FisheyeRef*>(h); }
int64_t fref_values_size(void* h) { return static_cast<FisheyeRef*>(h)->val_size; }
int64_t fref_tangent_size(void* h) { return static_cast<FisheyeRef*>(h)->dim_size; }
double fref_error(void* h, const double* values) { auto* g = static_cast<FisheyeRef*>(h); return g->graph.error(g->unpack(values)); }

// the layout of gtg_get_jacobians: row-major [A1 | A2 | b] per factor of the type; PRIOR [d x d | b at 81] (90)
int fref_jacobians(void* h, const double* values, int type, double* out, int64_t n_out) {
  auto* g = static_cast<FisheyeRef*>(h);
  const Values vals = g->unpack(values);
  int64_t pos = 0;
  for (size_t i = g->beg[type]; i < g->end[type]; i++) {
    auto jf = std::dynamic_pointer_cast<JacobianFactor>(g->graph[i]->linearize(vals));
    if (!jf) return -1;
    const Vector b = jf->getb();
    if (type == GTG_FAC_PRIOR) {
      if (pos + 90 > n_out) return -2;
      std::fill(out + pos, out + pos + 90, 0.0);
      const Matrix A = jf->getA(jf->begin());
      const int d = (int)A.rows();
      for (int r = 0; r < d; r++) for (int c = 0; c < d; c++) out[pos + r * d + c] = A(r, c);
      for (int r = 0; r < d; r++) out[pos + 81 + r] = b(r);
      pos += 90;
      continue;
    }
    for (auto it = jf->begin(); it != jf->end(); ++it) {
      const Matrix A = jf->getA(it);
      if (pos + (int64_t)A.size() > n_out) return -2;
      for (int r = 0; r < A.rows(); r++) for (int c = 0; c < A.cols(); c++) out[pos++] = A(r, c);
    }
    if (pos + (int64_t)b.size() > n_out) return -2;
    for (int r = 0; r < b.size(); r++) out[pos++] = b(r);
  }
  return pos == n_out ? 0 : -3;
}

// Per projection factor at these values, for the rows of a Cal3Fisheye calibration (zeros elsewhere, and for a point behind its
// camera): the intrinsic point (x, y) of PinholeBase::project2 through the composed pose, r = |(x, y)|, t = atan2(r, 1) and the factor
// s = Scaling(r) (1 + k1 t^2 + k2 t^4 + k3 t^6 + k4 t^8) of Cal3Fisheye::uncalibrate.  probe: 5 doubles per factor.
int fref_probe(void* h, const double* values, double* probe) {
  auto* g = static_cast<FisheyeRef*>(h);
  const gtg_problem* p = g->p;
  const Values vals = g->unpack(values);
  for (int64_t i = 0; i < p->n_proj; i++) {
    double* o = probe + 5 * i;
    for (int k = 0; k < 5; k++) o[k] = 0.0;
    if (g->calib_model[p->proj_calib[i]] != GTG_CALIB_FISHEYE) continue;
    Pose3 T = vals.at<Pose3>(Key(p->proj_pose[i]));
    if (p->proj_sensor && p->proj_sensor[i] >= 0) T = T.compose(unpackPose(p->sensor + 12 * p->proj_sensor[i]));
    const Point3 l = vals.at<Point3>(Key(p->proj_point[i]));
    if (T.transformTo(l).z() <= 0) continue;
    const Point2 pn = PinholeBase(T).project2(l);
    const double* d = p->calib_distortion + 4 * p->proj_calib[i];
    const double r = std::sqrt(pn.x() * pn.x() + pn.y() * pn.y()), t = std::atan2(r, 1.0);
    const double t2 = t * t, t4 = t2 * t2, t6 = t2 * t4, t8 = t4 * t4;
    o[0] = pn.x(); o[1] = pn.y(); o[2] = r; o[3] = t;
    o[4] = Cal3Fisheye::Scaling(r) * (1 + d[0] * t2 + d[1] * t4 + d[2] * t6 + d[3] * t8);
  }
  return 0;
}

// GaussianFactorGraph::hessianDiagonal and the gradient J^T b (= -gradientAtZero), variable id order
int fref_hessian_diagonal_gradient(void* h, const double* values, double* hd, double* grad) {
  auto* g = static_cast<FisheyeRef*>(h);
  auto lin = g->graph.linearize(g->unpack(values));
  g->packDelta(lin->hessianDiagonal(), hd);
  g->packDelta(lin->gradientAtZero(), grad);
  for (int64_t i = 0; i < g->dim_size; i++) grad[i] = -grad[i];
  return 0;
}

// One tryLambda body up to the linear errors (LevenbergMarquardtOptimizer.cpp:121-190): buildDampedSystem + optimize with a
// COLAMD ordering (reversed: the same ordering back to front).  Returns 1 on IndeterminantLinearSystemException.
int fref_solve(void* h, const double* values, double lambda, int diagonal_damping, double min_diag, double max_diag, int reversed,
               double* delta, double* lin_err) {
  auto* g = static_cast<FisheyeRef*>(h);
  const Values vals = g->unpack(values);
  auto lin = g->graph.linearize(vals);
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
    VectorValues d = damped.optimize(g->ordering(reversed), EliminatePreferCholesky);
    g->packDelta(d, delta);
    lin_err[0] = lin->error(VectorValues::Zero(d)); lin_err[1] = lin->error(d);
  } catch (const IndeterminantLinearSystemException&) { return 1; }
  return 0;
}

int fref_retract(void* h, const double* values, const double* delta, double* out) {
  auto* g = static_cast<FisheyeRef*>(h);
  g->pack(g->unpack(values).retract(g->unpackDelta(delta)), out);
  return 0;
}

// The reference's LM with default LevenbergMarquardtParams and a COLAMD ordering (reversed: back to front), the loop of
// NonlinearOptimizer::defaultOptimize (nonlinear/NonlinearOptimizer.cpp:62-117) around iterate() so that every outer iteration is
// recorded.  trace rows: [inner iterations, error, lambda].  Returns the outer iteration count.
int fref_lm(void* h, const double* values0, int reversed, double* values_out, int max_trace, double* trace, int* n_trace) {
  auto* g = static_cast<FisheyeRef*>(h);
  LevenbergMarquardtParams params;
  params.ordering = g->ordering(reversed);
  LevenbergMarquardtOptimizer lm(g->graph, g->unpack(values0), params);
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
}

}  // extern "C"
