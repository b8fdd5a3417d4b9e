// tests/golden/make_golden_planar.cpp -- reference answers for planar landmark SLAM graphs: BearingRangeFactor / RangeFactor /
// BearingFactor <Pose2, Point2> (gtsam/sam) beside BetweenFactor<Pose2>, PriorFactor<Pose2> and the 2-D partial pose priors, computed by
// the real reference (oracle/_ref).  A small extern "C" library driven by tests/golden/make_golden_planar.py through ctypes, in the
// pattern of make_golden_sam3d.cpp and make_golden_pose_partial.cpp: it builds the reference's NonlinearFactorGraph from a gtg_problem
// (the sam2 table included) and answers error / per-factor Jacobians / Hessian diagonal / gradient / damped solves / retract / the LM
// trajectory.  Variables are POSE2 and POINT2; keys are the variable ids, so Values order = id order.  A POINT2 crosses this interface
// as the C ABI holds it: three storage doubles (x, y, 0) and three tangent entries (dx, dy, 0); the reference sees a Point2.
// Factors are inserted in the order: sam2, between, prior, partial pose priors.  A sam2 record is given in the layout of GTG_FAC_SAM2:
// [A1 3x3 | A2 3x3 | b 3], the factor's 2 or 1 rows first, A2's third column and the unused rows zero.
#include <gtsam/geometry/Pose2.h>
#include <gtsam/linear/GaussianFactorGraph.h>
#include <gtsam/linear/JacobianFactor.h>
#include <gtsam/linear/NoiseModel.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/internal/LevenbergMarquardtState.h>
#include <gtsam/sam/BearingFactor.h>
#include <gtsam/sam/BearingRangeFactor.h>
#include <gtsam/sam/RangeFactor.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/PoseRotationPrior.h>
#include <gtsam/slam/PoseTranslationPrior.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gtsam_amd.h"

using namespace gtsam;

namespace {
struct Ref {
  const gtg_problem* p = nullptr;   // the caller's tables, alive until plref_destroy
  std::vector<int64_t> off;         // 3 storage doubles and 3 tangent entries per variable of either type
  int64_t size = 0;
  NonlinearFactorGraph graph;
  size_t beg[8] = {0}, end[8] = {0};   // factor ranges by GTG_FAC_*
  bool point(int i) const { return p->var_type[i] == GTG_VAR_POINT2; }
  SharedNoiseModel noise(int idx) const {
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
    throw std::invalid_argument("make_golden_planar: only Huber and Cauchy are used by these fixtures");
  }
  void build() {
    std::vector<SharedNoiseModel> nz(p->n_noise);
    for (int i = 0; i < p->n_noise; i++) nz[i] = noise(i);
    beg[GTG_FAC_SAM2] = graph.size();
    for (int64_t i = 0; i < p->planar.n_sam2; i++) {
      const double* z = p->planar.sam2_z + 3 * i;
      const Key x = Key(p->planar.sam2_pose[i]), l = Key(p->planar.sam2_point[i]);
      const SharedNoiseModel& m = nz[p->planar.sam2_noise[i]];
      if (p->planar.sam2_kind[i] == GTG_SAM_BEARING_RANGE) graph.emplace_shared<BearingRangeFactor<Pose2, Point2>>(x, l, Rot2::fromCosSin(z[0], z[1]), z[2], m);
      else if (p->planar.sam2_kind[i] == GTG_SAM_RANGE) graph.emplace_shared<RangeFactor<Pose2, Point2>>(x, l, z[2], m);
      else if (p->planar.sam2_kind[i] == GTG_SAM_BEARING) graph.emplace_shared<BearingFactor<Pose2, Point2>>(x, l, Rot2::fromCosSin(z[0], z[1]), m);
      else throw std::invalid_argument("unknown sam2_kind");
    }
    end[GTG_FAC_SAM2] = beg[GTG_FAC_BETWEEN_POSE3] = graph.size();
    for (int64_t i = 0; i < p->n_between; i++) {
      const double* z = p->between_z + 12 * i;
      graph.emplace_shared<BetweenFactor<Pose2>>(Key(p->between_v1[i]), Key(p->between_v2[i]), Pose2(z[0], z[1], z[2]), nz[p->between_noise[i]]);
    }
    end[GTG_FAC_BETWEEN_POSE3] = beg[GTG_FAC_PRIOR] = graph.size();
    for (int64_t i = 0; i < p->n_prior; i++) {
      const int v = p->prior_var[i];
      const double* d = p->prior_data + p->prior_off[i];
      if (point(v)) throw std::invalid_argument("no PriorFactor on a POINT2 in these fixtures");
      graph.addPrior(Key(v), Pose2(d[0], d[1], d[2]), nz[p->prior_noise[i]]);
    }
    end[GTG_FAC_PRIOR] = beg[GTG_FAC_POSE_PARTIAL] = graph.size();
    for (int64_t i = 0; i < p->n_pose_partial; i++) {
      const int v = p->pose_partial_var[i];
      const double* z = p->pose_partial_z + 9 * i;
      const SharedNoiseModel& m = nz[p->pose_partial_noise[i]];
      if (p->pose_partial_kind[i] == GTG_POSE_PARTIAL_TRANSLATION) graph.emplace_shared<PoseTranslationPrior<Pose2>>(Key(v), Point2(z[0], z[1]), m);
      else graph.emplace_shared<PoseRotationPrior<Pose2>>(Key(v), Rot2::fromCosSin(z[0], z[1]), m);
    }
    end[GTG_FAC_POSE_PARTIAL] = graph.size();
  }
  Values unpack(const double* v) const {
    Values vals;
    for (int i = 0; i < p->n_vars; i++) {
      const double* q = v + off[i];
      if (point(i)) vals.insert(Key(i), Point2(q[0], q[1])); else vals.insert(Key(i), Pose2(q[0], q[1], q[2]));
    }
    return vals;
  }
  void pack(const Values& vals, double* v) const {
    for (int i = 0; i < p->n_vars; i++) {
      double* q = v + off[i];
      if (point(i)) { const Point2 w = vals.at<Point2>(Key(i)); q[0] = w.x(); q[1] = w.y(); q[2] = 0.0; }
      else { const Pose2 T = vals.at<Pose2>(Key(i)); q[0] = T.x(); q[1] = T.y(); q[2] = T.theta(); }
    }
  }
  void packDelta(const VectorValues& vv, double* d) const {
    for (int i = 0; i < p->n_vars; i++) {
      const Vector& v = vv.at(Key(i));
      for (int k = 0; k < 3; k++) d[off[i] + k] = k < v.size() ? v(k) : 0.0;
    }
  }
  VectorValues unpackDelta(const double* d) const {
    VectorValues vv;
    for (int i = 0; i < p->n_vars; i++) vv.insert(Key(i), Eigen::Map<const Vector>(d + off[i], point(i) ? 2 : 3));
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

void* plref_create(const gtg_problem* p) {
  try {
    auto* g = new Ref;
    g->p = p;
    for (int i = 0; i < p->n_vars; i++) {
      if (p->var_type[i] != GTG_VAR_POSE2 && p->var_type[i] != GTG_VAR_POINT2) throw std::invalid_argument("POSE2 / POINT2 only");
      g->off.push_back(g->size); g->size += 3;
    }
    if (p->n_sfm || p->n_proj || p->n_stereo || p->n_sam || p->n_smart) throw std::invalid_argument("planar fixtures: sam2 / between / prior / partial tables only");
    g->build();
    return g;
  } catch (const std::exception& e) { std::fprintf(stderr, "plref_create: %s\n", e.what()); return nullptr; }
}
void plref_destroy(void* h) { delete static_cast<Ref*>(h); }
double plref_error(void* h, const double* values) { auto* g = static_cast<Ref*>(h); return g->graph.error(g->unpack(values)); }
// the (c, s) the reference's Rot2 holds for an angle (Rot2::fromAngle, geometry/Rot2.h:58-59) ...
void plref_rot2(double theta, double* cs) { const Rot2 r = Rot2::fromAngle(theta); cs[0] = r.c(); cs[1] = r.s(); }
// ... and for a pair handed to fromCosSin
void plref_rot2_cs(double c, double s, double* cs) { const Rot2 r = Rot2::fromCosSin(c, s); cs[0] = r.c(); cs[1] = r.s(); }

// Per sam2 factor at these values: q = transformTo(landmark), its norm (the argument of relativeBearing's threshold 1e-5), the range
// |p - t| (norm2's threshold 1e-10), the predicted Rot2 (c, s) and the unwrapped angle difference theta_z - theta_h (the bearing residual
// is that angle wrapped).  probe: 7 doubles per factor = qx, qy, |q|, range, hc, hs, theta_z - theta_h.
int plref_probe(void* h, const double* values, double* probe) {
  auto* g = static_cast<Ref*>(h);
  const gtg_problem* p = g->p;
  const Values vals = g->unpack(values);
  for (int64_t i = 0; i < p->planar.n_sam2; i++) {
    const Pose2 T = vals.at<Pose2>(Key(p->planar.sam2_pose[i]));
    const Point2 l = vals.at<Point2>(Key(p->planar.sam2_point[i]));
    const Point2 q = T.transformTo(l);
    const Rot2 hb = T.bearing(l);
    double* o = probe + 7 * i;
    o[0] = q.x(); o[1] = q.y(); o[2] = std::sqrt(q.x() * q.x() + q.y() * q.y()); o[3] = T.range(l);
    o[4] = hb.c(); o[5] = hb.s();
    o[6] = p->planar.sam2_kind[i] == GTG_SAM_RANGE ? 0.0 : std::atan2(p->planar.sam2_z[3 * i + 1], p->planar.sam2_z[3 * i]) - hb.theta();
  }
  return 0;
}

// the layout of gtg_get_jacobians: row-major [A1 | A2 | b] per factor of the type; a Pose2 pair in the 78-double between record,
// PRIOR and POSE_PARTIAL [A d x d | b at 81] (90), SAM2 [A1 3x3 | A2 3x3 | b 3] (21)
int plref_jacobians(void* h, const double* values, int type, double* out, int64_t n_out) {
  auto* g = static_cast<Ref*>(h);
  const Values vals = g->unpack(values);
  int64_t pos = 0;
  for (size_t i = g->beg[type]; i < g->end[type]; i++) {
    auto jf = std::dynamic_pointer_cast<JacobianFactor>(g->graph[i]->linearize(vals));
    if (!jf) return -1;
    const Vector b = jf->getb();
    if (type == GTG_FAC_PRIOR || type == GTG_FAC_POSE_PARTIAL) {
      if (pos + 90 > n_out) return -2;
      std::fill(out + pos, out + pos + 90, 0.0);
      const Matrix A = jf->getA(jf->begin());
      const int d = (int)A.cols();
      for (int r = 0; r < A.rows(); r++) for (int c = 0; c < d; c++) out[pos + r * d + c] = A(r, c);
      for (int r = 0; r < A.rows(); r++) out[pos + 81 + r] = b(r);
      pos += 90;
    } else if (type == GTG_FAC_SAM2) {
      if (pos + 21 > n_out) return -2;
      std::fill(out + pos, out + pos + 21, 0.0);
      // (an ExpressionFactor sorts its keys: the pose's block is the one with three columns, wherever it stands)
      auto it = jf->begin();
      const Matrix Aa = jf->getA(it), Ab = jf->getA(++it);
      const Matrix &A1 = Aa.cols() == 3 ? Aa : Ab, &A2 = Aa.cols() == 3 ? Ab : Aa;
      for (int r = 0; r < A1.rows(); r++) {
        for (int c = 0; c < 3; c++) out[pos + 3 * r + c] = A1(r, c);
        for (int c = 0; c < 2; c++) out[pos + 9 + 3 * r + c] = A2(r, c);
        out[pos + 18 + r] = b(r);
      }
      pos += 21;
    } else if (type == GTG_FAC_BETWEEN_POSE3) {   // a Pose2 pair: the 3 x 3 blocks at the start of the 36-double places, b in the first 3 of 6
      if (pos + 78 > n_out) return -2;
      std::fill(out + pos, out + pos + 78, 0.0);
      auto it = jf->begin();
      const Matrix A1 = jf->getA(it), A2 = jf->getA(++it);
      for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { out[pos + 3 * r + c] = A1(r, c); out[pos + 36 + 3 * r + c] = A2(r, c); }
      for (int r = 0; r < 3; r++) out[pos + 72 + r] = b(r);
      pos += 78;
    } else return -4;
  }
  return pos == n_out ? 0 : -3;
}

// GaussianFactorGraph::hessianDiagonal and the gradient J^T b (= -gradientAtZero), variable id order
int plref_hessian_diagonal_gradient(void* h, const double* values, double* hd, double* grad) {
  auto* g = static_cast<Ref*>(h);
  auto lin = g->graph.linearize(g->unpack(values));
  g->packDelta(lin->hessianDiagonal(), hd);
  g->packDelta(lin->gradientAtZero(), grad);
  for (int64_t i = 0; i < g->size; i++) grad[i] = -grad[i] + 0.0;   // (+ 0.0: the padding stays +0)
  return 0;
}

// One tryLambda body up to the linear errors (LevenbergMarquardtOptimizer.cpp:121-190): buildDampedSystem + optimize with a
// COLAMD ordering (reversed: the same ordering back to front).  Returns 1 on IndeterminantLinearSystemException.
int plref_solve(void* h, const double* values, double lambda, int diagonal_damping, double min_diag, double max_diag, int reversed,
                double* delta, double* lin_err) {
  auto* g = static_cast<Ref*>(h);
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

int plref_retract(void* h, const double* values, const double* delta, double* out) {
  auto* g = static_cast<Ref*>(h);
  g->pack(g->unpack(values).retract(g->unpackDelta(delta)), out);
  return 0;
}

// The reference's LM with default LevenbergMarquardtParams and a COLAMD ordering (reversed: back to front), the loop of
// NonlinearOptimizer::defaultOptimize (nonlinear/NonlinearOptimizer.cpp:62-117) around iterate() so that every outer iteration is
// recorded.  trace rows: [inner iterations, error, lambda].  Returns the outer iteration count.
int plref_lm(void* h, const double* values0, int reversed, double* values_out, int max_trace, double* trace, int* n_trace) {
  auto* g = static_cast<Ref*>(h);
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
