// tests/golden/make_golden_pose_partial.cpp -- reference answers for graphs with PoseTranslationPrior<POSE> / PoseRotationPrior<POSE>,
// POSE = Pose3 | Pose2 (gtsam/slam), computed by the real reference (oracle/_ref).  A small extern "C" library driven by
// tests/golden/make_golden_pose_partial.py through ctypes, in the pattern of make_golden_sam3d.cpp and make_golden_smart_pose.cpp: it
// builds the reference's NonlinearFactorGraph from a gtg_problem (the pose_partial table included) and answers error / per-factor
// Jacobians / Hessian diagonal / gradient / damped solves / retract / the LM trajectory.
// Variables are POSE3, POINT3 and POSE2; keys are the variable ids, so Values order = id order.
// Factors are inserted in the order: smart (pose-type), projection, between, prior, partial pose priors.  Every probe builds a FRESH
// graph from the caller's tables (which the caller keeps alive): a smart factor caches its triangulation, and no probe may see what
// another left behind.  A partial prior's record is given in the layout of GTG_FAC_POSE_PARTIAL: the PRIOR record of the pose's tangent
// dimension d with the factor's rows first and the other entries zero.
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/geometry/Pose2.h>
#include <gtsam/geometry/Pose3.h>
#include <gtsam/linear/GaussianFactorGraph.h>
#include <gtsam/linear/JacobianFactor.h>
#include <gtsam/linear/NoiseModel.h>
#include <gtsam/nonlinear/LevenbergMarquardtOptimizer.h>
#include <gtsam/nonlinear/NonlinearFactorGraph.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/internal/LevenbergMarquardtState.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/PoseRotationPrior.h>
#include <gtsam/slam/PoseTranslationPrior.h>
#include <gtsam/slam/ProjectionFactor.h>
#include <gtsam/slam/SmartProjectionPoseFactor.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <optional>
#include <vector>

#include "gtsam_amd.h"

using namespace gtsam;

namespace {
typedef SmartProjectionPoseFactor<Cal3_S2> SmartPose;

Pose3 unpackPose(const double* p) {
  Matrix3 R;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R(i, j) = p[3 * i + j];
  return Pose3(Rot3(R), Point3(p[9], p[10], p[11]));
}
Rot3 unpackRot(const double* p) {
  Matrix3 R;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R(i, j) = p[3 * i + j];
  return Rot3(R);
}
void packPose(const Pose3& T, double* p) {
  const Matrix3 R = T.rotation().matrix();
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) p[3 * i + j] = R(i, j);
  p[9] = T.x(); p[10] = T.y(); p[11] = T.z();
}

struct Ref {
  const gtg_problem* p = nullptr;   // the caller's tables, alive until ppref_destroy
  std::vector<int64_t> val_off, dim_off;
  int64_t val_size = 0, dim_size = 0;
  int dimOf(int i) const { return p->var_type[i] == GTG_VAR_POSE3 ? 6 : 3; }
  int sizeOf(int i) const { return p->var_type[i] == GTG_VAR_POSE3 ? 12 : 3; }
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
    throw std::invalid_argument("make_golden_pose_partial: only Huber and Cauchy are used by these fixtures");
  }
  std::optional<Pose3> sensorOf(const int32_t* tab, int64_t i) const {
    std::optional<Pose3> s;
    if (tab && tab[i] >= 0) s = unpackPose(p->sensor + 12 * tab[i]);
    return s;
  }
  // the graph, and the factor ranges by GTG_FAC_* in beg / end
  NonlinearFactorGraph graph(size_t* beg = nullptr, size_t* end = nullptr) const {
    NonlinearFactorGraph g;
    size_t b[7] = {0}, e[7] = {0};
    std::vector<SharedNoiseModel> nz(p->n_noise);
    for (int i = 0; i < p->n_noise; i++) nz[i] = noise(i);
    std::map<int, std::shared_ptr<Cal3_S2>> Ks;   // one shared calibration object per table entry, as user code has it
    auto K = [&](int ci) {
      auto& k = Ks[ci];
      if (!k) { const double* c = p->calib + 5 * ci; k = std::make_shared<Cal3_S2>(c[0], c[1], c[2], c[3], c[4]); }
      return k;
    };
    for (int64_t i = 0; i < p->n_smart; i++) {
      const double* sp = p->smart_params + 8 * i;
      const LinearizationMode lm = sp[5] == 2.0 ? JACOBIAN_Q : (sp[5] == 3.0 ? JACOBIAN_SVD : HESSIAN);
      SmartProjectionParams params(lm, sp[4] == 1.0 ? ZERO_ON_DEGENERACY : (sp[4] == 2.0 ? HANDLE_INFINITY : IGNORE_DEGENERACY), false, false, sp[3]);
      params.setRankTolerance(sp[0]);
      params.setEnableEPI(sp[6] != 0.0);
      params.setLandmarkDistanceThreshold(sp[1]);
      params.setDynamicOutlierRejectionThreshold(sp[2]);
      auto f = std::make_shared<SmartPose>(nz[p->smart_noise[i]], K(p->smart_calib[i]), sensorOf(p->smart_sensor, i), params);
      for (int64_t k = p->smart_ptr[i]; k < p->smart_ptr[i + 1]; k++) f->add(Point2(p->smart_z[2 * k], p->smart_z[2 * k + 1]), Key(p->smart_cam[k]));
      g.push_back(f);
    }
    b[1] = g.size();
    for (int64_t i = 0; i < p->n_proj; i++)
      g.emplace_shared<GenericProjectionFactor<Pose3, Point3, Cal3_S2>>(Point2(p->proj_z[2 * i], p->proj_z[2 * i + 1]), nz[p->proj_noise[i]],
          Key(p->proj_pose[i]), Key(p->proj_point[i]), K(p->proj_calib[i]), sensorOf(p->proj_sensor, i));
    e[1] = b[2] = g.size();
    for (int64_t i = 0; i < p->n_between; i++) {
      const double* z = p->between_z + 12 * i;
      if (p->var_type[p->between_v1[i]] == GTG_VAR_POSE2)
        g.emplace_shared<BetweenFactor<Pose2>>(Key(p->between_v1[i]), Key(p->between_v2[i]), Pose2(z[0], z[1], z[2]), nz[p->between_noise[i]]);
      else
        g.emplace_shared<BetweenFactor<Pose3>>(Key(p->between_v1[i]), Key(p->between_v2[i]), unpackPose(z), nz[p->between_noise[i]]);
    }
    e[2] = b[3] = g.size();
    for (int64_t i = 0; i < p->n_prior; i++) {
      const int v = p->prior_var[i];
      const double* d = p->prior_data + p->prior_off[i];
      if (p->var_type[v] == GTG_VAR_POSE3) g.addPrior(Key(v), unpackPose(d), nz[p->prior_noise[i]]);
      else if (p->var_type[v] == GTG_VAR_POSE2) g.addPrior(Key(v), Pose2(d[0], d[1], d[2]), nz[p->prior_noise[i]]);
      else g.addPrior(Key(v), Point3(d[0], d[1], d[2]), nz[p->prior_noise[i]]);
    }
    e[3] = b[6] = g.size();
    for (int64_t i = 0; i < p->n_pose_partial; i++) {
      const int v = p->pose_partial_var[i], kind = p->pose_partial_kind[i];
      const double* z = p->pose_partial_z + 9 * i;
      const SharedNoiseModel& m = nz[p->pose_partial_noise[i]];
      if (p->var_type[v] == GTG_VAR_POSE3) {
        if (kind == GTG_POSE_PARTIAL_TRANSLATION) g.emplace_shared<PoseTranslationPrior<Pose3>>(Key(v), Point3(z[0], z[1], z[2]), m);
        else g.emplace_shared<PoseRotationPrior<Pose3>>(Key(v), unpackRot(z), m);
      } else {
        if (kind == GTG_POSE_PARTIAL_TRANSLATION) g.emplace_shared<PoseTranslationPrior<Pose2>>(Key(v), Point2(z[0], z[1]), m);
        else g.emplace_shared<PoseRotationPrior<Pose2>>(Key(v), Rot2::fromCosSin(z[0], z[1]), m);
      }
    }
    e[6] = g.size();
    if (beg) for (int k = 0; k < 7; k++) { beg[k] = b[k]; end[k] = e[k]; }
    return g;
  }
  Values unpack(const double* v) const {
    Values vals;
    for (int i = 0; i < p->n_vars; i++) {
      const double* q = v + val_off[i];
      if (p->var_type[i] == GTG_VAR_POSE3) vals.insert(Key(i), unpackPose(q));
      else if (p->var_type[i] == GTG_VAR_POSE2) vals.insert(Key(i), Pose2(q[0], q[1], q[2]));
      else vals.insert(Key(i), Point3(q[0], q[1], q[2]));
    }
    return vals;
  }
  void pack(const Values& vals, double* v) const {
    for (int i = 0; i < p->n_vars; i++) {
      double* q = v + val_off[i];
      if (p->var_type[i] == GTG_VAR_POSE3) packPose(vals.at<Pose3>(Key(i)), q);
      else if (p->var_type[i] == GTG_VAR_POSE2) { const Pose2 T = vals.at<Pose2>(Key(i)); q[0] = T.x(); q[1] = T.y(); q[2] = T.theta(); }
      else { const Point3 w = vals.at<Point3>(Key(i)); q[0] = w.x(); q[1] = w.y(); q[2] = w.z(); }
    }
  }
  void packDelta(const VectorValues& vv, double* d) const {
    for (int i = 0; i < p->n_vars; i++) { const Vector& v = vv.at(Key(i)); for (int k = 0; k < dimOf(i); k++) d[dim_off[i] + k] = v(k); }
  }
  VectorValues unpackDelta(const double* d) const {
    VectorValues vv;
    for (int i = 0; i < p->n_vars; i++) vv.insert(Key(i), Eigen::Map<const Vector>(d + dim_off[i], dimOf(i)));
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

void* ppref_create(const gtg_problem* p) {
  try {
    auto* g = new Ref;
    g->p = p;
    for (int i = 0; i < p->n_vars; i++) {
      const int t = p->var_type[i];
      if (t != GTG_VAR_POSE3 && t != GTG_VAR_POINT3 && t != GTG_VAR_POSE2) throw std::invalid_argument("POSE3 / POINT3 / POSE2 only");
      g->val_off.push_back(g->val_size); g->dim_off.push_back(g->dim_size);
      g->val_size += g->sizeOf(i); g->dim_size += g->dimOf(i);
    }
    if (p->n_sfm || p->n_stereo || p->n_sam || p->calib_distortion) throw std::invalid_argument("partial pose prior fixtures: smart / projection / between / prior / partial tables only");
    for (int64_t i = 0; i < p->n_smart; i++) if (!p->smart_calib || p->smart_calib[i] < 0) throw std::invalid_argument("pose-type smart factors only");
    (void)g->graph();
    return g;
  } catch (const std::exception& e) { std::fprintf(stderr, "ppref_create: %s\n", e.what()); return nullptr; }
}
void ppref_destroy(void* h) { delete static_cast<Ref*>(h); }
double ppref_error(void* h, const double* values) { auto* g = static_cast<Ref*>(h); return g->graph().error(g->unpack(values)); }
// the (c, s) the reference's Rot2 holds for an angle (Rot2::fromAngle, geometry/Rot2.h:58-59)
void ppref_rot2(double theta, double* cs) { const Rot2 r = Rot2::fromAngle(theta); cs[0] = r.c(); cs[1] = r.s(); }

// the layout of gtg_get_jacobians: row-major [A1 | A2 | b] per factor of the type; PRIOR and POSE_PARTIAL [A d x d | b at 81] (90), a
// partial prior's rows first
int ppref_jacobians(void* h, const double* values, int type, double* out, int64_t n_out) {
  auto* g = static_cast<Ref*>(h);
  size_t beg[7], end[7];
  const NonlinearFactorGraph graph = g->graph(beg, end);
  const Values vals = g->unpack(values);
  int64_t pos = 0;
  for (size_t i = beg[type]; i < end[type]; i++) {
    auto jf = std::dynamic_pointer_cast<JacobianFactor>(graph[i]->linearize(vals));
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
      continue;
    }
    for (auto it = jf->begin(); it != jf->end(); ++it) {
      const Matrix A = jf->getA(it);
      if (pos + (int64_t)A.size() > n_out) return -2;
      if (type == GTG_FAC_BETWEEN_POSE3 && A.cols() == 3) {   // a Pose2 pair: the 3 x 3 block at the start of the 36-double place
        if (pos + 36 > n_out) return -2;
        std::fill(out + pos, out + pos + 36, 0.0);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) out[pos + 3 * r + c] = A(r, c);
        pos += 36;
        continue;
      }
      for (int r = 0; r < A.rows(); r++) for (int c = 0; c < A.cols(); c++) out[pos++] = A(r, c);
    }
    if (type == GTG_FAC_BETWEEN_POSE3) {
      if (pos + 6 > n_out) return -2;
      std::fill(out + pos, out + pos + 6, 0.0);
      for (int r = 0; r < b.size(); r++) out[pos + r] = b(r);
      pos += 6;
      continue;
    }
    if (pos + (int64_t)b.size() > n_out) return -2;
    for (int r = 0; r < b.size(); r++) out[pos++] = b(r);
  }
  return pos == n_out ? 0 : -3;
}

// Per partial prior: the branch SO3::Logmap (geometry/SO3.cpp:247-323) takes for a PoseRotationPrior<Pose3> at these values, from the
// trace of the matrix the reference hands it (measured.between(R)): 0 Taylor, 1 acos, 2 near pi; -1 for every other form.  tr[i] that trace.
int ppref_rot_branch(void* h, const double* values, int32_t* branch, double* tr) {
  auto* g = static_cast<Ref*>(h);
  const gtg_problem* p = g->p;
  const Values vals = g->unpack(values);
  for (int64_t i = 0; i < p->n_pose_partial; i++) {
    branch[i] = -1; tr[i] = 0.0;
    const int v = p->pose_partial_var[i];
    if (p->var_type[v] != GTG_VAR_POSE3 || p->pose_partial_kind[i] != GTG_POSE_PARTIAL_ROTATION) continue;
    const Matrix3 M = unpackRot(p->pose_partial_z + 9 * i).between(vals.at<Pose3>(Key(v)).rotation()).matrix();
    tr[i] = M.trace();
    branch[i] = tr[i] + 1.0 < 1e-3 ? 2 : (tr[i] - 3.0 < -1e-6 ? 1 : 0);
  }
  return 0;
}

// GaussianFactorGraph::hessianDiagonal and the gradient J^T b (= -gradientAtZero), variable id order
int ppref_hessian_diagonal_gradient(void* h, const double* values, double* hd, double* grad) {
  auto* g = static_cast<Ref*>(h);
  auto lin = g->graph().linearize(g->unpack(values));
  g->packDelta(lin->hessianDiagonal(), hd);
  g->packDelta(lin->gradientAtZero(), grad);
  for (int64_t i = 0; i < g->dim_size; i++) grad[i] = -grad[i];
  return 0;
}

// One tryLambda body up to the linear errors (LevenbergMarquardtOptimizer.cpp:121-190): buildDampedSystem + optimize with a
// COLAMD ordering (reversed: the same ordering back to front).  Returns 1 on IndeterminantLinearSystemException.
int ppref_solve(void* h, const double* values, double lambda, int diagonal_damping, double min_diag, double max_diag, int reversed,
                double* delta, double* lin_err) {
  auto* g = static_cast<Ref*>(h);
  const NonlinearFactorGraph graph = g->graph();
  const Values vals = g->unpack(values);
  auto lin = graph.linearize(vals);
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

int ppref_retract(void* h, const double* values, const double* delta, double* out) {
  auto* g = static_cast<Ref*>(h);
  g->pack(g->unpack(values).retract(g->unpackDelta(delta)), out);
  return 0;
}

// The reference's LM with default LevenbergMarquardtParams and a COLAMD ordering (reversed: back to front), the loop of
// NonlinearOptimizer::defaultOptimize (nonlinear/NonlinearOptimizer.cpp:62-117) around iterate() so that every outer iteration is
// recorded.  trace rows: [inner iterations, error, lambda].  Returns the outer iteration count.
int ppref_lm(void* h, const double* values0, int reversed, double* values_out, int max_trace, double* trace, int* n_trace) {
  auto* g = static_cast<Ref*>(h);
  const NonlinearFactorGraph graph = g->graph();
  LevenbergMarquardtParams params;
  params.ordering = Ref::ordering(graph, reversed);
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
}

}  // extern "C"
