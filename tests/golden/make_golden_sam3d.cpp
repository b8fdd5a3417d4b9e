// tests/golden/make_golden_sam3d.cpp -- reference answers for graphs with BearingRangeFactor / RangeFactor / BearingFactor <Pose3, Point3>
// (gtsam/sam), computed by the real reference (oracle/_ref).  A small extern "C" library driven by tests/golden/make_golden_sam3d.py
// through ctypes, in the pattern of make_golden_stereo.cpp: it builds the reference's NonlinearFactorGraph from a gtg_problem (the sam
// table included) and answers error / per-factor Jacobians / Hessian diagonal / gradient / damped solves / retract / the LM trajectory.
// Variables are POSE3 and POINT3 only; keys are the variable ids, so Values order = id order.
// Factors are inserted in the order: projection, stereo, sam, between, prior.  A sam record is given in the layout of GTG_FAC_SAM: three
// rows, the rows its kind does not use zero.
#include <gtsam/geometry/Cal3DS2.h>
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
  throw std::invalid_argument("make_golden_sam3d: only Huber and Cauchy are used by these fixtures");
}

struct StereoRef {
  int n_vars = 0;
  std::vector<int> var_type;
  std::vector<int64_t> val_off, dim_off;
  int64_t val_size = 0, dim_size = 0;
  NonlinearFactorGraph graph;
  size_t beg[6], end[6];   // factor ranges by GTG_FAC_*
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

void* sref_create(const gtg_problem* p) {
  try {
    auto* g = new StereoRef;
    g->n_vars = p->n_vars;
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
      if (d && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0 || d[3] != 0.0))
        g->graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3DS2>>(z, noise[p->proj_noise[i]], Key(p->proj_pose[i]), Key(p->proj_point[i]),
            std::make_shared<Cal3DS2>(c[0], c[1], c[2], c[3], c[4], d[0], d[1], d[2], d[3]), sensorOf(p->proj_sensor, i));
      else
        g->graph.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3_S2>>(z, noise[p->proj_noise[i]], Key(p->proj_pose[i]), Key(p->proj_point[i]),
            std::make_shared<Cal3_S2>(c[0], c[1], c[2], c[3], c[4]), sensorOf(p->proj_sensor, i));
    }
    g->end[1] = g->beg[4] = g->graph.size();
    for (int64_t i = 0; i < p->n_stereo; i++) {
      const double* c = p->calib + 5 * p->stereo_calib[i];
      auto K = std::make_shared<Cal3_S2Stereo>(c[0], c[1], c[2], c[3], c[4], p->calib_baseline[p->stereo_calib[i]]);
      g->graph.emplace_shared<GenericStereoFactor<Pose3, Point3>>(StereoPoint2(p->stereo_z[3 * i], p->stereo_z[3 * i + 1], p->stereo_z[3 * i + 2]),
          noise[p->stereo_noise[i]], Key(p->stereo_pose[i]), Key(p->stereo_point[i]), K, sensorOf(p->stereo_sensor, i));
    }
    g->end[4] = g->beg[5] = g->graph.size();
    for (int64_t i = 0; i < p->n_sam; i++) {
      const double* z = p->sam_z + 4 * i;
      const Key x = Key(p->sam_pose[i]), l = Key(p->sam_point[i]);
      const SharedNoiseModel& nz = noise[p->sam_noise[i]];
      if (p->sam_kind[i] == GTG_SAM_BEARING_RANGE) g->graph.emplace_shared<BearingRangeFactor<Pose3, Point3>>(x, l, Unit3(z[0], z[1], z[2]), z[3], nz);
      else if (p->sam_kind[i] == GTG_SAM_RANGE) g->graph.emplace_shared<RangeFactor<Pose3, Point3>>(x, l, z[3], nz);
      else if (p->sam_kind[i] == GTG_SAM_BEARING) g->graph.emplace_shared<BearingFactor<Pose3, Point3>>(x, l, Unit3(z[0], z[1], z[2]), nz);
      else throw std::invalid_argument("unknown sam_kind");
    }
    g->end[5] = g->beg[2] = g->graph.size();
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
  } catch (const std::exception& e) { std::fprintf(stderr, "sref_create: %s\n", e.what()); return nullptr; }
}
void sref_destroy(void* h) { delete static_cast<StereoRef*>(h); }
// the three doubles the reference holds for Unit3(x, y, z) (geometry/Unit3.cpp:38)
void sref_unit3(const double* in, double* out) { const Vector3 v = Unit3(in[0], in[1], in[2]).unitVector(); out[0] = v(0); out[1] = v(1); out[2] = v(2); }
int64_t sref_values_size(void* h) { return static_cast<StereoRef*>(h)->val_size; }
int64_t sref_tangent_size(void* h) { return static_cast<StereoRef*>(h)->dim_size; }
double sref_error(void* h, const double* values) { auto* g = static_cast<StereoRef*>(h); return g->graph.error(g->unpack(values)); }

// the layout of gtg_get_jacobians: row-major [A1 | A2 | b] per factor of the type; PRIOR [d x d | b at 81] (90)
int sref_jacobians(void* h, const double* values, int type, double* out, int64_t n_out) {
  auto* g = static_cast<StereoRef*>(h);
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
    if (type == GTG_FAC_SAM) {   // [A1 3x6 | A2 3x3 | b 3], the factor's 3, 1 or 2 rows first
      if (pos + 30 > n_out) return -2;
      std::fill(out + pos, out + pos + 30, 0.0);
      // (an ExpressionFactor sorts its keys: the pose's block is the one with six columns, wherever it stands)
      auto it = jf->begin();
      const Matrix Aa = jf->getA(it), Ab = jf->getA(++it);
      const Matrix &A1 = Aa.cols() == 6 ? Aa : Ab, &A2 = Aa.cols() == 6 ? Ab : Aa;
      for (int r = 0; r < A1.rows(); r++) {
        for (int c = 0; c < 6; c++) out[pos + 6 * r + c] = A1(r, c);
        for (int c = 0; c < 3; c++) out[pos + 18 + 3 * r + c] = A2(r, c);
        out[pos + 27 + r] = b(r);
      }
      pos += 30;
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

// GaussianFactorGraph::hessianDiagonal and the gradient J^T b (= -gradientAtZero), variable id order
int sref_hessian_diagonal_gradient(void* h, const double* values, double* hd, double* grad) {
  auto* g = static_cast<StereoRef*>(h);
  auto lin = g->graph.linearize(g->unpack(values));
  g->packDelta(lin->hessianDiagonal(), hd);
  g->packDelta(lin->gradientAtZero(), grad);
  for (int64_t i = 0; i < g->dim_size; i++) grad[i] = -grad[i];
  return 0;
}

// One tryLambda body up to the linear errors (LevenbergMarquardtOptimizer.cpp:121-190): buildDampedSystem + optimize with a
// COLAMD ordering (reversed: the same ordering back to front).  Returns 1 on IndeterminantLinearSystemException.
int sref_solve(void* h, const double* values, double lambda, int diagonal_damping, double min_diag, double max_diag, int reversed,
               double* delta, double* lin_err) {
  auto* g = static_cast<StereoRef*>(h);
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

int sref_retract(void* h, const double* values, const double* delta, double* out) {
  auto* g = static_cast<StereoRef*>(h);
  g->pack(g->unpack(values).retract(g->unpackDelta(delta)), out);
  return 0;
}

// The reference's LM with default LevenbergMarquardtParams and a COLAMD ordering (reversed: back to front), the loop of
// NonlinearOptimizer::defaultOptimize (nonlinear/NonlinearOptimizer.cpp:62-117) around iterate() so that every outer iteration is
// recorded.  trace rows: [inner iterations, error, lambda].  Returns the outer iteration count.
int sref_lm(void* h, const double* values0, int reversed, double* values_out, int max_trace, double* trace, int* n_trace) {
  auto* g = static_cast<StereoRef*>(h);
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
