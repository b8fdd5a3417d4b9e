// GpuLevenbergMarquardtOptimizer.cpp -- extractor (NonlinearFactorGraph/Values -> SoA gtg_problem) and the
// host LM state machine around the C ABI.  See the header for the reference anchors.
#include "GpuLevenbergMarquardtOptimizer.h"

#include <gtsam/geometry/Cal3Bundler.h>
#include <gtsam/geometry/Cal3DS2.h>
#include <gtsam/geometry/Cal3Fisheye.h>
#include <gtsam/geometry/Cal3_S2.h>
#include <gtsam/geometry/PinholeCamera.h>
#include <gtsam/geometry/Pose2.h>
#include <gtsam/geometry/Pose3.h>
#include <gtsam/linear/JacobianFactor.h>
#include <gtsam/linear/NoiseModel.h>
#include <gtsam/linear/linearExceptions.h>
#include <gtsam/linear/PCGSolver.h>
#include <gtsam/linear/Preconditioner.h>
#include <gtsam/nonlinear/PriorFactor.h>
#include <gtsam/nonlinear/internal/LevenbergMarquardtState.h>
#include <gtsam/slam/BetweenFactor.h>
#include <gtsam/slam/GeneralSFMFactor.h>
#include <gtsam/slam/ProjectionFactor.h>
#include <gtsam/slam/SmartProjectionFactor.h>
#include <gtsam/slam/SmartProjectionPoseFactor.h>
#include <gtsam/slam/SmartProjectionRigFactor.h>
#include <gtsam/slam/StereoFactor.h>
#include <gtsam/sam/BearingFactor.h>
#include <gtsam/sam/BearingRangeFactor.h>
#include <gtsam/slam/PoseRotationPrior.h>
#include <gtsam/slam/PoseTranslationPrior.h>
#include <gtsam/sam/RangeFactor.h>

#include <gtsam/config.h>

// The compile-time options of the linked GTSAM change the mathematics of this path (gtsam/config.h.in:31-90).  The device code
// implements the DEFAULT-flag semantics; refuse to build the shim against a GTSAM configured otherwise.
#if defined(GTSAM_USE_QUATERNIONS)
#error "gtsam_amd: built for Rot3 as a rotation matrix (GTSAM_USE_QUATERNIONS off): Rot3 retract / Logmap differ with quaternions"
#endif
#if !defined(GTSAM_POSE3_EXPMAP) || !defined(GTSAM_ROT3_EXPMAP)
#error "gtsam_amd: the device retracts Pose3 / Rot3 with the full exponential map (GTSAM_POSE3_EXPMAP and GTSAM_ROT3_EXPMAP on)"
#endif
#if defined(GTSAM_SLOW_BUT_CORRECT_BETWEENFACTOR)
#error "gtsam_amd: BetweenFactor Jacobians are not multiplied by dLog on the device (GTSAM_SLOW_BUT_CORRECT_BETWEENFACTOR off)"
#endif
#if defined(GTSAM_SLOW_BUT_CORRECT_EXPMAP)
#error "gtsam_amd: Pose2 uses the first-order chart on the device (GTSAM_SLOW_BUT_CORRECT_EXPMAP off)"
#endif
#if !defined(GTSAM_THROW_CHEIRALITY_EXCEPTION)
#error "gtsam_amd: a point behind the camera zeroes the factor, as the reference does when it throws CheiralityException (flag on)"
#endif

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <map>
#include <set>
#include <new>
#include <stdexcept>
#include <thread>
#include <array>
#include <type_traits>
#include <typeinfo>

using namespace gtsam;

namespace gtsam_amd {

typedef PinholeCamera<Cal3Bundler> SfmCamera;
typedef GeneralSFMFactor<SfmCamera, Point3> SfmFactor;
typedef GenericProjectionFactor<Pose3, Point3, Cal3_S2> ProjFactor;
typedef GenericProjectionFactor<Pose3, Point3, Cal3DS2> ProjFactorDS2;
typedef GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> ProjFactorFisheye;
typedef GenericStereoFactor<Pose3, Point3> StereoFactor;
typedef BearingRangeFactor<Pose3, Point3> SamBearingRangeFactor;   // gtsam/sam: wrapped as BearingRangeFactor3D, RangeFactor3D, BearingFactor3D
typedef RangeFactor<Pose3, Point3> SamRangeFactor;
typedef BearingFactor<Pose3, Point3> SamBearingFactor;
typedef BearingRangeFactor<Pose2, Point2> Sam2BearingRangeFactor;   // planar: wrapped as BearingRangeFactor2D, RangeFactor2D, BearingFactor2D
typedef RangeFactor<Pose2, Point2> Sam2RangeFactor;
typedef BearingFactor<Pose2, Point2> Sam2BearingFactor;
// partial pose priors (gtsam/slam): wrapped as PoseTranslationPrior3D / 2D and PoseRotationPrior3D / 2D
typedef PoseTranslationPrior<Pose3> TranslationPrior3;
typedef PoseRotationPrior<Pose3> RotationPrior3;
typedef PoseTranslationPrior<Pose2> TranslationPrior2;
typedef PoseRotationPrior<Pose2> RotationPrior2;
typedef SmartProjectionFactor<SfmCamera> SmartFactor;   // the factor of timing/timeSFMBALsmart.cpp
// The smart factor keeps its noise model and its parameters protected and has no accessor for them; a class derived from it may
// name them, and the pointers to member it forms are ordinary pointers to members of the factor (a maintainer binding this into
// GTSAM would add two accessors instead).
struct SmartAccess : SmartFactor {
  static SharedIsotropic SmartFactorBase<SfmCamera>::* noise() { return &SmartAccess::noiseModel_; }
  static SmartProjectionParams SmartFactor::* params() { return &SmartAccess::params_; }
};
// SmartProjectionPoseFactor<Cal3_S2> (wrapped as SmartProjectionPose3Factor; examples/SFMExample_SmartFactor.cpp): K through
// calibration(); noise model, parameters and the optional body_P_sensor the same way
typedef PinholePose<Cal3_S2> PoseCamera;
typedef SmartProjectionPoseFactor<Cal3_S2> SmartPoseFactor;
struct SmartPoseAccess : SmartPoseFactor {
  static SharedIsotropic SmartFactorBase<PoseCamera>::* noise() { return &SmartPoseAccess::noiseModel_; }
  static SmartProjectionParams SmartProjectionFactor<PoseCamera>::* params() { return &SmartPoseAccess::params_; }
  static std::optional<Pose3> SmartFactorBase<PoseCamera>::* sensor() { return &SmartPoseAccess::body_P_sensor_; }
};
// SmartProjectionRigFactor<PinholePose<Cal3_S2>>: the same bases, so the same accessors read its noise model and parameters; the rig,
// the camera ids and the non-unique keys have accessors of their own (slam/SmartProjectionRigFactor.h:166-174)
typedef SmartProjectionRigFactor<PoseCamera> SmartRigFactor;
typedef internal::LevenbergMarquardtState State;

// The States THIS class publishes have a dynamic type of their own: that -- not an address, which the allocator hands out again -- is
// how a State somebody else installed is told from one of ours (the base class's decreaseLambda() makes plain LevenbergMarquardtStates).
struct GpuState : State {
  using State::State;
  // Both constructors of LevenbergMarquardtState deep-copy the Values they are given (the Values&& one passes its argument on as an
  // lvalue, LevenbergMarquardtState.h:61-63): 16 ms for the 158 000 variables of the L1723 shape, per State.  So a GpuState is built on
  // an EMPTY Values, and the caller's map is then MOVED into the member's storage: the empty member is destroyed and a new Values is
  // constructed in its place from an rvalue (Values(Values&&), Values.h:118: the map's nodes change hands, O(1)).  `values` is declared
  // const in NonlinearOptimizerState, so it cannot be assigned or swapped -- but ending the lifetime of a const member SUBOBJECT of a heap
  // object and creating a new object of the same type in its storage is storage reuse, not modification of a const object ([basic.life]:
  // the restriction on re-creating const objects covers complete objects of static / thread / automatic storage; since C++20 the new
  // member is "transparently replaceable" under its old name, and implementations treat earlier dialects alike -- it is what
  // std::vector<T>::emplace does for a T with a const member).  Rounds 3-5 swapped through a const_cast instead, which IS a
  // modification of a const object.
  static std::unique_ptr<GpuState> make(Values&& v, double error, double lambda, double factor, unsigned iterations, unsigned inner) {
    std::unique_ptr<GpuState> s(new GpuState(Values(), error, lambda, factor, iterations, inner));
    void* at = const_cast<void*>(static_cast<const void*>(&s->values));
    s->values.~Values();
    ::new (at) Values(std::move(v));     // (Values' move constructor moves a std::map: it does not throw)
    return s;
  }
};

namespace {
void check(int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + gtg_last_error()); }
// Key -> variable id: the keys are sorted, so a binary search over the contiguous array (a std::map of 158 000 keys cost 0.2 s of
// pointer chasing for the 1.35 M lookups of the L1723 shape)
int32_t idOf(const std::vector<Key>& keys, Key k) {
  auto it = std::lower_bound(keys.begin(), keys.end(), k);
  if (it == keys.end() || *it != k) throw ValuesKeyDoesNotExist("GpuLevenbergMarquardtOptimizer", k);
  return (int32_t)(it - keys.begin());
}
void packPose(const Pose3& T, double* p) {
  const Matrix3 R = T.rotation().matrix();
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) p[3 * i + j] = R(i, j);
  p[9] = T.x(); p[10] = T.y(); p[11] = T.z();
}
Pose3 unpackPose(const double* p) {
  Matrix3 R;
  R << p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8];
  return Pose3(Rot3(R), Point3(p[9], p[10], p[11]));
}
void packCamera(const SfmCamera& c, double* p) {
  packPose(c.pose(), p);
  p[12] = c.calibration().fx(); p[13] = c.calibration().k1(); p[14] = c.calibration().k2();
  p[15] = c.calibration().px(); p[16] = c.calibration().py();
}
// ---- variable types (GTG_VAR_*), each fact once: which Values are of one, its storage size and tangent dimension, to doubles and back
int32_t classify(const Value* v) {   // -1: a type outside the GPU path
  return dynamic_cast<const GenericValue<Point3>*>(v) ? GTG_VAR_POINT3 : dynamic_cast<const GenericValue<SfmCamera>*>(v) ? GTG_VAR_SFM_CAMERA :
         dynamic_cast<const GenericValue<Pose3>*>(v) ? GTG_VAR_POSE3 : dynamic_cast<const GenericValue<Pose2>*>(v) ? GTG_VAR_POSE2 :
         dynamic_cast<const GenericValue<Point2>*>(v) ? GTG_VAR_POINT2 : -1;
}
template <class T> struct VarTypeOf;
template <> struct VarTypeOf<Pose3> { static constexpr int32_t value = GTG_VAR_POSE3; };
template <> struct VarTypeOf<SfmCamera> { static constexpr int32_t value = GTG_VAR_SFM_CAMERA; };
template <> struct VarTypeOf<Point3> { static constexpr int32_t value = GTG_VAR_POINT3; };
template <> struct VarTypeOf<Pose2> { static constexpr int32_t value = GTG_VAR_POSE2; };
constexpr int storageSize(int32_t t) { return t == GTG_VAR_POSE3 ? 12 : t == GTG_VAR_SFM_CAMERA ? 17 : 3; }
constexpr int tangentDim(int32_t t) { return t == GTG_VAR_POSE3 ? 6 : t == GTG_VAR_SFM_CAMERA ? 9 : 3; }
// A Point2 is padded to the landmark slot at the C ABI: (x, y, 0) and (dx, dy, 0).  The padding never leaves this file: the caller's
// Values hold a Point2, a VectorValues entry of it two numbers, a Jacobian block on it two columns.
constexpr int userDim(int32_t t) { return t == GTG_VAR_POINT2 ? 2 : tangentDim(t); }
// an object of a variable's type (a value, a prior, a measurement) as storageSize() doubles; payload(): of a Value whose type the caller knows, no check
void packAs(const Point3& q, double* p) { p[0] = q.x(); p[1] = q.y(); p[2] = q.z(); }
void packAs(const Pose2& q, double* p) { p[0] = q.x(); p[1] = q.y(); p[2] = q.theta(); }
void packAs(const Pose3& q, double* p) { packPose(q, p); }
void packAs(const SfmCamera& q, double* p) { packCamera(q, p); }
template <class T> const T& payload(const Value& v) { return static_cast<const GenericValue<T>&>(v).value(); }
template <class T> T& payload(Value& v) { return static_cast<GenericValue<T>&>(v).value(); }
void pack(int32_t t, const Value& v, double* p) {
  if (t == GTG_VAR_POINT3) packAs(payload<Point3>(v), p);
  else if (t == GTG_VAR_SFM_CAMERA) packAs(payload<SfmCamera>(v), p);
  else if (t == GTG_VAR_POSE3) packAs(payload<Pose3>(v), p);
  else if (t == GTG_VAR_POINT2) { const Point2& q = payload<Point2>(v); p[0] = q.x(); p[1] = q.y(); p[2] = 0.0; }
  else packAs(payload<Pose2>(v), p);
}
void unpack(int32_t t, const double* p, Value& v) {
  if (t == GTG_VAR_POINT3) payload<Point3>(v) = Point3(p[0], p[1], p[2]);
  else if (t == GTG_VAR_SFM_CAMERA) payload<SfmCamera>(v) = SfmCamera(unpackPose(p), Cal3Bundler(p[12], p[13], p[14], p[15], p[16]));
  else if (t == GTG_VAR_POSE3) payload<Pose3>(v) = unpackPose(p);
  else if (t == GTG_VAR_POINT2) payload<Point2>(v) = Point2(p[0], p[1]);
  else payload<Pose2>(v) = Pose2(p[0], p[1], p[2]);
}
// ---- Jacobian records (gtg_get_jacobians): one whitened [A1 | A2 | b] per factor, row-major blocks at fixed offsets; the record's width follows
// the factor type, the block sizes the factor's first variable (Pose2: 3x3 blocks inside the record of the Pose3 factor)
constexpr int kFacTypes = 8;
const int64_t kRecordWidth[kFacTypes] = {26, 20, 78, 90, 30, 30, 90, 21};   // by GTG_FAC_*
struct RecordLayout {
  int rows, nblk, boff[2], bcols[2], rhs; int64_t width;
  int bpitch[2] = {0, 0};   // doubles from one row of a block to the next where that is not bcols (the padded landmark block of a planar record)
  int pitch(int k) const { return bpitch[k] ? bpitch[k] : bcols[k]; }
};
template <class F> RecordLayout recordLayout(int32_t fac, F&& firstVarType) {   // firstVarType(): GTG_VAR_* of the factor's first variable, asked only where the layout depends on it
  const int64_t w = kRecordWidth[fac];
  if (fac == GTG_FAC_GENERAL_SFM) return {2, 2, {0, 18}, {tangentDim(GTG_VAR_SFM_CAMERA), 3}, 24, w};
  if (fac == GTG_FAC_PROJECTION) return {2, 2, {0, 12}, {tangentDim(GTG_VAR_POSE3), 3}, 18, w};
  if (fac == GTG_FAC_STEREO) return {3, 2, {0, 18}, {tangentDim(GTG_VAR_POSE3), 3}, 27, w};
  if (fac == GTG_FAC_SAM) return {3, 2, {0, 18}, {tangentDim(GTG_VAR_POSE3), 3}, 27, w};   // (rows: the caller puts the kind's 3, 1 or 2 -- Impl::layoutOf)
  if (fac == GTG_FAC_SAM2) return {2, 2, {0, 9}, {tangentDim(GTG_VAR_POSE2), userDim(GTG_VAR_POINT2)}, 18, w, {0, 3}};   // (rows: the kind's 2 or 1)
  const int d = tangentDim(firstVarType());
  if (fac == GTG_FAC_BETWEEN_POSE3) return {d, 2, {0, 36}, {d, d}, 72, w};
  return {d, 1, {0, 0}, {d, 0}, 81, w};   // PRIOR, and POSE_PARTIAL (rows: the caller puts the factor's 3, 2 or 1 -- Impl::layoutOf)
}
typedef std::vector<std::pair<int32_t, int64_t>> FactorMap;   // factor of graph_ -> (GTG_FAC_*, index in that type's table); (-1, 0): null; (-2, i): smart factor i
// The device's current records, one buffer per GTG_FAC_* (null and smart factors have none: a smart factor's linearisation is a Hessian factor the device never forms)
struct Records {
  std::vector<double> rec[kFacTypes];
  const double* of(const std::pair<int32_t, int64_t>& tf) const { return rec[tf.first].data() + tf.second * kRecordWidth[tf.first]; }
};
Records fetchRecords(gtg_handle h, const FactorMap& fac_map) {
  Records out;
  int64_t count[kFacTypes] = {0};
  for (const auto& tf : fac_map) if (tf.first >= 0) count[tf.first]++;
  for (int t = 0; t < kFacTypes; t++) {
    if (!count[t]) continue;
    out.rec[t].resize((size_t)(count[t] * kRecordWidth[t]));
    check(gtg_get_jacobians(h, t, out.rec[t].data(), (int64_t)out.rec[t].size()), "gtg_get_jacobians");
  }
  return out;
}
// params.iterativeParams as the cg[4] of gtg_try_lambda_pcg (PCGSolverParameters only); `who` opens the text of the exception
std::shared_ptr<PCGSolverParameters> pcgParameters(const NonlinearOptimizerParams& params, const char* who, double cg[4]) {
  auto pcg = std::dynamic_pointer_cast<PCGSolverParameters>(params.iterativeParams);
  if (!pcg) throw std::runtime_error(std::string(who) + ": only PCGSolverParameters are handled by the GPU path");
  cg[0] = (double)pcg->maxIterations; cg[1] = (double)pcg->minIterations; cg[2] = pcg->epsilon_rel; cg[3] = pcg->epsilon_abs;
  return pcg;
}
// ---- host threads.  Range t of nthreads over [0, n) is [cut(t), cut(t + 1)).
size_t cut(size_t n, size_t nthreads, size_t t) { return n * t / nthreads; }
struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } };
struct JoinAll { std::vector<std::thread>& v; ~JoinAll() { for (auto& t : v) if (t.joinable()) t.join(); } };
// starts fn(t, begin, end) on a thread of its own for the ranges t = first .. nthreads - 1; the caller owns (and joins) `pool`
template <class F> void startRanges(std::vector<std::thread>& pool, size_t n, size_t nthreads, size_t first, F fn) {
  for (size_t t = first; t < nthreads; t++) pool.emplace_back(fn, t, cut(n, nthreads, t), cut(n, nthreads, t + 1));
}
// fn(t, begin, end) for every range: range 0 on the calling thread, the others on threads that are joined on every way out
template <class F> void parallelRanges(size_t n, size_t nthreads, F fn) {
  std::vector<std::thread> pool;
  JoinAll join{pool};
  startRanges(pool, n, nthreads, 1, fn);
  fn((size_t)0, cut(n, nthreads, 0), cut(n, nthreads, 1));
}
// GTG_HOST_THREADS, or the hardware's threads up to `cap` (every site has its own, measured)
size_t hostThreads(unsigned cap) {
  const char* env = std::getenv("GTG_HOST_THREADS");
  return (size_t)(env ? std::max(1, std::atoi(env)) : (int)std::min(std::max(1u, std::thread::hardware_concurrency()), cap));
}
// GTG_DEBUG_TIMING: host-side breakdown of the construction on stderr, one line per lap
struct Lap {
  const bool on = std::getenv("GTG_DEBUG_TIMING") != nullptr;
  std::chrono::high_resolution_clock::time_point prev = std::chrono::high_resolution_clock::now();
  void operator()(const char* what) {
    const auto now = std::chrono::high_resolution_clock::now();
    if (on) std::fprintf(stderr, "[gtsam_amd shim ] %-46s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - prev).count());
    prev = now;
  }
};
}  // namespace

struct GpuLevenbergMarquardtOptimizer::Impl {
  gtg_handle h = nullptr;
  std::vector<Key> keys;                 // variable id -> Key (Values order: sorted)
  std::vector<int32_t> var_type;
  std::vector<int64_t> val_off;
  std::vector<double> packed;            // host copy of the packed values
  Values scratch;                        // the deep copy of the caller's Values (made beside the extraction); swapped into the State at the end of init
  std::vector<Value*> slots;             // variable id -> the GenericValue object of that variable inside the State's Values (heap objects
                                         // owned by the map's nodes: they stay where they are when the map is swapped into the next State)
  const Values* published = nullptr;     // the Values object (inside the State THIS class published last) whose nodes `slots` point into:
                                         // checked before every write through `slots` (adoptStateIfForeign)
  FactorMap fac_map;                     // by factor of graph_
  std::vector<int64_t> dim_off;          // variable id -> offset in the tangent vector (delta)
  bool keep_linearization = false;       // iterate(): download the records right after gtg_linearize
  GaussianFactorGraph::shared_ptr linearization;
  bool host_values_stale = false;
  // device-side copies of the LM state while optimize() keeps Values on the GPU
  double error = 0, lambda = 0, factor = 0;
  size_t iterations = 0; int inner = 0;
  std::chrono::high_resolution_clock::time_point start = std::chrono::high_resolution_clock::now();   // logFile's seconds column
  ~Impl() { if (h) gtg_destroy(h); }
  void takeScalars(const State& s) { error = s.error; lambda = s.lambda; factor = s.currentFactor; iterations = s.iterations; inner = s.totalNumberInnerIterations; }
  std::vector<int32_t> sam_kind;         // GTG_SAM_* by row of the sam table: a bearing / range record has its kind's 3, 1 or 2 rows
  std::vector<int32_t> pp_kind;          // GTG_POSE_PARTIAL_* by row of the partial pose prior table: 3 rows on a Pose3, 2 or 1 on a Pose2
  std::vector<int32_t> sam2_kind;        // GTG_SAM_* by row of the planar sam table: 2 rows for a bearing-range record, else 1
  RecordLayout layoutOf(const std::pair<int32_t, int64_t>& tf, Key first) const {
    RecordLayout lay = recordLayout(tf.first, [&] { return var_type[idOf(keys, first)]; });
    if (tf.first == GTG_FAC_SAM) lay.rows = sam_kind[(size_t)tf.second] == GTG_SAM_BEARING_RANGE ? 3 : sam_kind[(size_t)tf.second] == GTG_SAM_RANGE ? 1 : 2;
    if (tf.first == GTG_FAC_SAM2) lay.rows = sam2_kind[(size_t)tf.second] == GTG_SAM_BEARING_RANGE ? 2 : 1;
    if (tf.first == GTG_FAC_POSE_PARTIAL) lay.rows = lay.bcols[0] == 6 ? 3 : pp_kind[(size_t)tf.second] == GTG_POSE_PARTIAL_TRANSLATION ? 2 : 1;
    return lay;
  }
};

namespace {
struct NoiseTable {
  std::vector<int32_t> kind, dim, rkind; std::vector<int64_t> off; std::vector<double> data, rparam;
  std::map<const noiseModel::Base*, int32_t> seen;        // by object: the usual case of one shared_ptr on many factors
  std::map<std::vector<double>, int32_t> seen_value;      // by value: loaders create one model object per factor (load2D / load3D)
  // noiseModel::Robust (NoiseModel.h:670-760) -> (GTG_ROBUST_*, parameter) beside the base model's row
  static void estimator(const noiseModel::Robust& rb, int32_t* rk, double* k) {
    namespace me = noiseModel::mEstimator;
    const auto& e = rb.robust();
    if (!e) throw std::invalid_argument("Robust noise model without an m-estimator");
    if (std::dynamic_pointer_cast<me::Null>(e)) { *rk = GTG_ROBUST_NONE; *k = 0.0; return; }
    if (e->reweightScheme() != me::Base::Block)
      throw std::invalid_argument("m-estimators with the Scalar re-weighting scheme are outside the GPU path");
    if (auto p = std::dynamic_pointer_cast<me::Fair>(e)) { *rk = GTG_ROBUST_FAIR; *k = p->modelParameter(); }
    else if (auto p = std::dynamic_pointer_cast<me::Huber>(e)) { *rk = GTG_ROBUST_HUBER; *k = p->modelParameter(); }
    else if (auto p = std::dynamic_pointer_cast<me::Cauchy>(e)) { *rk = GTG_ROBUST_CAUCHY; *k = p->modelParameter(); }
    else if (auto p = std::dynamic_pointer_cast<me::Tukey>(e)) { *rk = GTG_ROBUST_TUKEY; *k = p->modelParameter(); }
    else if (auto p = std::dynamic_pointer_cast<me::Welsch>(e)) { *rk = GTG_ROBUST_WELSCH; *k = p->modelParameter(); }
    else if (auto p = std::dynamic_pointer_cast<me::GemanMcClure>(e)) { *rk = GTG_ROBUST_GEMANMCCLURE; *k = p->modelParameter(); }
    else if (auto p = std::dynamic_pointer_cast<me::DCS>(e)) { *rk = GTG_ROBUST_DCS; *k = p->modelParameter(); }
    else if (auto p = std::dynamic_pointer_cast<me::L2WithDeadZone>(e)) { *rk = GTG_ROBUST_L2WITHDEADZONE; *k = p->modelParameter(); }
    // the asymmetric estimators differ from their symmetric namesakes for NEGATIVE distances only (LossFunctions.cpp:433-500); what a
    // Robust noise model hands them is a norm (NoiseModel.h:716-718, NoiseModel.cpp:697-730), so on this path they are Tukey / Cauchy
    else if (auto p = std::dynamic_pointer_cast<me::AsymmetricTukey>(e)) { *rk = GTG_ROBUST_TUKEY; *k = p->modelParameter(); }
    else if (auto p = std::dynamic_pointer_cast<me::AsymmetricCauchy>(e)) { *rk = GTG_ROBUST_CAUCHY; *k = p->modelParameter(); }
    else throw std::invalid_argument("m-estimator outside the GPU path (supported: Fair, Huber, Cauchy, Tukey, Welsch, GemanMcClure, DCS, L2WithDeadZone, "
                                     "AsymmetricTukey, AsymmetricCauchy; not: Custom)");
  }
  int32_t add(const SharedNoiseModel& outer, size_t expect_dim) {
    if (!outer) throw std::invalid_argument("factor without a noise model is not supported");
    auto it = seen.find(outer.get());
    if (it != seen.end()) return it->second;
    if (outer->dim() != expect_dim) throw std::invalid_argument("NoiseModelFactor: NoiseModel has wrong dimension");
    SharedNoiseModel nm = outer;
    int32_t rk = GTG_ROBUST_NONE; double rp = 0.0;
    if (auto rb = std::dynamic_pointer_cast<noiseModel::Robust>(outer)) { estimator(*rb, &rk, &rp); nm = rb->noise(); }
    if (nm->isConstrained() || std::dynamic_pointer_cast<noiseModel::Robust>(nm))
      throw std::invalid_argument("Constrained / nested Robust noise models are outside the GPU path");
    int32_t k; std::vector<double> params;
    if (nm->isUnit()) k = GTG_NOISE_UNIT;
    else if (auto iso = std::dynamic_pointer_cast<noiseModel::Isotropic>(nm)) { k = GTG_NOISE_ISOTROPIC; params.push_back(iso->sigma()); }
    else if (auto dg = std::dynamic_pointer_cast<noiseModel::Diagonal>(nm)) { k = GTG_NOISE_DIAGONAL; for (size_t i = 0; i < dg->dim(); i++) params.push_back(dg->sigma(i)); }
    else if (auto ga = std::dynamic_pointer_cast<noiseModel::Gaussian>(nm)) {
      k = GTG_NOISE_GAUSSIAN;
      const Matrix R = ga->R();
      for (int i = 0; i < R.rows(); i++) for (int j = 0; j < R.cols(); j++) params.push_back(R(i, j));
    } else throw std::invalid_argument("unsupported noise model type");
    // identical models share a row of the table (first-occurrence order), however many objects they are
    std::vector<double> key{(double)k, (double)nm->dim(), (double)rk, rp};
    key.insert(key.end(), params.begin(), params.end());
    auto byValue = seen_value.find(key);
    if (byValue != seen_value.end()) { seen[outer.get()] = byValue->second; return byValue->second; }
    const int32_t idx = (int32_t)kind.size();
    off.push_back((int64_t)data.size()); dim.push_back((int32_t)nm->dim());
    rkind.push_back(rk); rparam.push_back(rp);
    kind.push_back(k); data.insert(data.end(), params.begin(), params.end());
    seen_value[key] = idx;
    seen[outer.get()] = idx;
    return idx;
  }
};
}  // namespace

// Construction.  The reference's constructor (LevenbergMarquardtOptimizer.cpp:47-66, NonlinearOptimizer.cpp:41-43) copies the graph
// and the Values and evaluates graph.error(initialValues) on the host -- 0.11 s for the L1723 shape, one thread (NonlinearFactorGraph.cpp
// :170-179 is serial even with TBB).  Here the base classes are constructed on an EMPTY graph (so that neither that pass nor COLAMD
// runs: the ordering handed over is the caller's, or a trivial one -- the device path has its own elimination structure), then
// graph_ and state_ (both protected, NonlinearOptimizer.h:78-80) are set: the graph by shared_ptr copies, the state from the
// caller's Values and the error the DEVICE computed for them (k_error, <= 1e-9 of the reference's, tests/test_gpu_parity.py).
static LevenbergMarquardtParams withOrdering(const LevenbergMarquardtParams& params, const Values& initial, const Ordering* ordering) {
  LevenbergMarquardtParams p = params;
  if (ordering) p.ordering = *ordering;
  else if (!p.ordering) p.ordering = Ordering(initial.keys());
  return p;
}

GpuLevenbergMarquardtOptimizer::GpuLevenbergMarquardtOptimizer(const NonlinearFactorGraph& graph, const Values& initial,
                                                               const LevenbergMarquardtParams& params, int device,
                                                               const ShardSpec& shards)
    : LevenbergMarquardtOptimizer(NonlinearFactorGraph(), Values(), withOrdering(params, initial, nullptr)), impl_(new Impl) {
  init(graph, initial, device, shards);
}

GpuLevenbergMarquardtOptimizer::GpuLevenbergMarquardtOptimizer(const NonlinearFactorGraph& graph, const Values& initial,
                                                               const Ordering& ordering,
                                                               const LevenbergMarquardtParams& params, int device,
                                                               const ShardSpec& shards)
    : LevenbergMarquardtOptimizer(NonlinearFactorGraph(), Values(), withOrdering(params, initial, &ordering)), impl_(new Impl) {
  init(graph, initial, device, shards);
}

GpuLevenbergMarquardtOptimizer::~GpuLevenbergMarquardtOptimizer() = default;

namespace {
// What one host thread extracts from its range of the graph: the rows of every factor table in graph order, the noise models and
// calibrations as (run length, object) -- rows of the shared tables are handed out afterwards, sequentially, in first-occurrence
// order, so that the tables are those of a single-threaded pass whatever the thread count.
struct Extract {
  std::vector<int32_t> sfm_cam, sfm_pt, pj_pose, pj_pt, pj_sen, st_pose, st_pt, st_sen, sam_kind, sam_pose, sam_pt, bt_1, bt_2, pr_var, sm_cam, pp_kind, pp_var, s2_kind, s2_pose, s2_pt;
  std::vector<double> sfm_z, pj_z, st_z, sam_z, sensor, bt_z, pr_data, sm_z, sm_prm, pp_z, s2_z;
  std::vector<int64_t> pr_off, sm_ptr;
  FactorMap fac_map;                                                        // (type, index in THIS chunk's table of that type)
  typedef std::vector<std::pair<int64_t, SharedNoiseModel>> Runs;
  Runs sfm_nz, pj_nz, st_nz, sam_nz, bt_nz, pr_nz, sm_nz, pp_nz, s2_nz;
  std::vector<int32_t> bt_dim, pr_dim, sam_dim, pp_dim, s2_dim;             // expected noise dimension per between / prior / sam / partial prior / planar sam factor
  std::vector<std::pair<const void*, int>> pj_cal;                          // calibration object per projection factor, 1 = Cal3DS2, 3 = Cal3Fisheye
  std::vector<const Cal3_S2Stereo*> st_cal;                                 // calibration object per stereo factor
  std::vector<const Cal3_S2*> sm_cal;                                       // per smart factor: the shared K of a pose-type factor, null for a camera-type one
  std::vector<int32_t> sm_sen;                                              // per smart factor: row of `sensor` (this chunk's) or -1
  std::vector<const SmartRigFactor::Cameras*> sm_rig;                       // per smart factor: the rig of a rig-type factor, else null
  std::vector<int32_t> sm_cid;                                              // per smart measurement: camera id in that rig (0 for other factors)
  std::vector<uint8_t> sensor_shared;                                       // per row of `sensor`: 1 = a smart factor's body_P_sensor, shared by value (mergeTables)
  std::vector<std::pair<const void*, int>> cal_order;                       // the calibration objects the chunk's factors name, in the order they are first met (0 Cal3_S2, 1 Cal3DS2, 2 Cal3_S2Stereo, 3 Cal3Fisheye):
  std::set<const void*> cal_seen;                                           // the calib table gets its rows in GRAPH order, whichever factor type names an object first
  void calibration(const void* K, int kind) { if (cal_seen.insert(K).second) cal_order.emplace_back(K, kind); }
  std::exception_ptr err;                                                   // what the chunk's first offending factor threw
  static void run(Runs& r, const SharedNoiseModel& nm) { if (!r.empty() && r.back().second.get() == nm.get()) r.back().first++; else r.emplace_back(1, nm); }
  static double* grow(std::vector<double>& v, size_t n) { v.resize(v.size() + n); return v.data() + v.size() - n; }   // n more doubles, zero-filled
};
void addSfm(Extract& x, const SfmFactor& s, const std::vector<Key>& keys) {
  x.fac_map.emplace_back(GTG_FAC_GENERAL_SFM, (int64_t)x.sfm_cam.size());
  x.sfm_cam.push_back(idOf(keys, s.key1())); x.sfm_pt.push_back(idOf(keys, s.key2()));
  x.sfm_z.push_back(s.measured().x()); x.sfm_z.push_back(s.measured().y());
  Extract::run(x.sfm_nz, s.noiseModel());
}
// GenericProjectionFactor<Pose3, Point3, Cal3_S2>, or the same factor with a Cal3DS2 calibration (section 8(f) #3) or a Cal3Fisheye one
template <class CAL> constexpr int calibrationKind() { return std::is_same<CAL, Cal3DS2>::value ? 1 : std::is_same<CAL, Cal3Fisheye>::value ? 3 : 0; }
template <class CAL> void addProjection(Extract& x, const GenericProjectionFactor<Pose3, Point3, CAL>& p, const std::vector<Key>& keys) {
  x.fac_map.emplace_back(GTG_FAC_PROJECTION, (int64_t)x.pj_pose.size());
  if (p.throwCheirality()) throw std::invalid_argument("GenericProjectionFactor with throwCheirality is not supported");
  x.pj_pose.push_back(idOf(keys, p.key1())); x.pj_pt.push_back(idOf(keys, p.key2()));
  x.pj_z.push_back(p.measured().x()); x.pj_z.push_back(p.measured().y());
  Extract::run(x.pj_nz, p.noiseModel());
  x.pj_cal.emplace_back(p.calibration().get(), calibrationKind<CAL>());
  x.calibration(p.calibration().get(), calibrationKind<CAL>());
  if (p.body_P_sensor()) { x.pj_sen.push_back((int32_t)(x.sensor.size() / 12)); packPose(*p.body_P_sensor(), Extract::grow(x.sensor, 12)); x.sensor_shared.push_back(0); }
  else x.pj_sen.push_back(-1);
}
// GenericStereoFactor<Pose3, Point3> (slam/StereoFactor.h): measurement (uL, uR, v), shared Cal3_S2Stereo, optional body_P_sensor in the
// sensor table of the projection factors
void addStereo(Extract& x, const StereoFactor& p, const std::vector<Key>& keys) {
  x.fac_map.emplace_back(GTG_FAC_STEREO, (int64_t)x.st_pose.size());
  if (p.throwCheirality()) throw std::invalid_argument("GenericStereoFactor with throwCheirality is not supported");
  x.st_pose.push_back(idOf(keys, p.key1())); x.st_pt.push_back(idOf(keys, p.key2()));
  x.st_z.push_back(p.measured().uL()); x.st_z.push_back(p.measured().uR()); x.st_z.push_back(p.measured().v());
  Extract::run(x.st_nz, p.noiseModel());
  x.st_cal.push_back(p.calibration().get()); x.calibration(p.calibration().get(), 2);
  if (p.body_P_sensor()) { x.st_sen.push_back((int32_t)(x.sensor.size() / 12)); packPose(*p.body_P_sensor(), Extract::grow(x.sensor, 12)); x.sensor_shared.push_back(0); }
  else x.st_sen.push_back(-1);
}
// BearingRangeFactor / RangeFactor / BearingFactor <Pose3, Point3> (gtsam/sam): one row of the sam table; bearing: the measured Unit3 or
// null, range: the measured range or null.  No calibration, no sensor.
void addSam(Extract& x, int32_t kind, Key pose, Key point, const Unit3* bearing, const double* range, const SharedNoiseModel& nm, const std::vector<Key>& keys) {
  x.fac_map.emplace_back(GTG_FAC_SAM, (int64_t)x.sam_pose.size());
  x.sam_kind.push_back(kind); x.sam_pose.push_back(idOf(keys, pose)); x.sam_pt.push_back(idOf(keys, point));
  double* z = Extract::grow(x.sam_z, 4);
  if (bearing) { const Vector3 u = bearing->unitVector(); z[0] = u(0); z[1] = u(1); z[2] = u(2); }
  if (range) z[3] = *range;
  Extract::run(x.sam_nz, nm); x.sam_dim.push_back(kind == GTG_SAM_BEARING_RANGE ? 3 : kind == GTG_SAM_RANGE ? 1 : 2);
}
// BearingRangeFactor / RangeFactor / BearingFactor <Pose2, Point2> (gtsam/sam, planar): one row of the sam2 table; bearing: the measured
// Rot2 or null -- its (c, s) as the reference holds them --, range: the measured range or null
void addSam2(Extract& x, int32_t kind, Key pose, Key point, const Rot2* bearing, const double* range, const SharedNoiseModel& nm, const std::vector<Key>& keys) {
  x.fac_map.emplace_back(GTG_FAC_SAM2, (int64_t)x.s2_pose.size());
  x.s2_kind.push_back(kind); x.s2_pose.push_back(idOf(keys, pose)); x.s2_pt.push_back(idOf(keys, point));
  double* z = Extract::grow(x.s2_z, 3);
  if (bearing) { z[0] = bearing->c(); z[1] = bearing->s(); }
  if (range) z[2] = *range;
  Extract::run(x.s2_nz, nm); x.s2_dim.push_back(kind == GTG_SAM_BEARING_RANGE ? 2 : 1);
}
// the rows every smart factor has, whatever its camera type: parameters, noise model, keys and measurements
template <class FACTOR>
void addSmartRows(Extract& x, const FACTOR& sf, const KeyVector& fkeys, const SmartProjectionParams& sp, const SharedIsotropic& iso, const std::vector<Key>& keys, const char* what) {
  x.fac_map.emplace_back(-2, (int64_t)x.sm_prm.size() / 8);   // (no Jacobian record: its linearisation is a Hessian factor)
  const TriangulationParameters& tp = sp.triangulation;
  // HESSIAN, JACOBIAN_Q and JACOBIAN_SVD are the same normal equations (the device never forms the factor itself); an
  // IMPLICIT_SCHUR factor cannot be eliminated by the reference's direct solvers either.
  if (sp.linearizationMode == IMPLICIT_SCHUR) throw std::invalid_argument(std::string(what) + ": the IMPLICIT_SCHUR linearisation is not supported");
  // useLOST: the sigma triangulatePoint3 hands to triangulateLOST (geometry/triangulation.h:503) -- the mean of the triangulation noise
  // model's sigmas, 1e-4 without one; what sigmas() throws (a Robust model) leaves the constructor as it leaves the reference's optimizer
  const double lost_sigma = tp.useLOST ? (tp.noiseModel ? tp.noiseModel->sigmas().mean() : 1e-4) : 0.0;
  if (tp.enableEPI && tp.noiseModel) throw std::invalid_argument(std::string(what) + ": enableEPI with a noise model in the triangulation parameters is not supported");
  Extract::run(x.sm_nz, iso);
  const auto& zs = sf.measured();
  if (zs.size() != fkeys.size() || zs.empty()) throw std::invalid_argument(std::string(what) + ": measurements and keys do not match");
  for (size_t k = 0; k < zs.size(); k++) { x.sm_cam.push_back(idOf(keys, fkeys[k])); x.sm_z.push_back(zs[k].x()); x.sm_z.push_back(zs[k].y()); }
  x.sm_ptr.push_back((int64_t)x.sm_cam.size());
  x.sm_prm.insert(x.sm_prm.end(), {tp.rankTolerance, tp.landmarkDistanceThreshold, tp.dynamicOutlierRejectionThreshold, sp.retriangulationThreshold,
                                   sp.degeneracyMode == ZERO_ON_DEGENERACY ? 1.0 : (sp.degeneracyMode == HANDLE_INFINITY ? 2.0 : 0.0),
                                   sp.linearizationMode == JACOBIAN_Q ? 2.0 : (sp.linearizationMode == JACOBIAN_SVD ? 3.0 : 0.0), tp.enableEPI ? 1.0 : 0.0, lost_sigma});
}
// SmartProjectionFactor<SfmCamera>.  (throwCheirality / verboseCheirality are read by the pose-only smart factors, not by
// SmartProjectionFactor<CAMERA>.)
void addSmart(Extract& x, const SmartFactor& sf, const std::vector<Key>& keys) {
  addSmartRows(x, sf, sf.keys(), sf.*SmartAccess::params(), sf.*SmartAccess::noise(), keys, "SmartProjectionFactor");
  x.sm_cal.push_back(nullptr); x.sm_sen.push_back(-1); x.sm_rig.push_back(nullptr); x.sm_cid.resize(x.sm_cam.size(), 0);
}
// SmartProjectionPoseFactor<Cal3_S2>: the keys are Pose3 variables, one shared K (a row of the calib table) and an optional
// body_P_sensor (a row of the sensor table, shared by value among the smart factors)
void addSmartPose(Extract& x, const SmartPoseFactor& sf, const std::vector<Key>& keys) {
  if (!sf.calibration()) throw std::invalid_argument("SmartProjectionPoseFactor: no calibration");
  if ((sf.*SmartPoseAccess::params()).triangulation.enableEPI) throw std::invalid_argument("SmartProjectionPoseFactor: enableEPI is not supported");
  addSmartRows(x, sf, sf.keys(), sf.*SmartPoseAccess::params(), sf.*SmartPoseAccess::noise(), keys, "SmartProjectionPoseFactor");
  x.sm_cal.push_back(sf.calibration().get()); x.calibration(sf.calibration().get(), 0); x.sm_rig.push_back(nullptr); x.sm_cid.resize(x.sm_cam.size(), 0);
  const std::optional<Pose3>& bs = sf.*SmartPoseAccess::sensor();
  if (bs) { x.sm_sen.push_back((int32_t)(x.sensor.size() / 12)); packPose(*bs, Extract::grow(x.sensor, 12)); x.sensor_shared.push_back(1); }
  else x.sm_sen.push_back(-1);
}
// SmartProjectionRigFactor<PinholePose<Cal3_S2>>: the keys are the BODY poses, one per measurement and possibly repeated
// (nonUniqueKeys(); keys() holds the unique ones); every measurement names a camera of the rig, whose K and extrinsic become one calib
// and one sensor row per (rig object, camera id) in mergeTables.  (The constructor has refused every degeneracy / linearisation mode
// but ZERO_ON_DEGENERACY / HESSIAN.)
void addSmartRig(Extract& x, const SmartRigFactor& sf, const std::vector<Key>& keys) {
  if (!sf.cameraRig()) throw std::invalid_argument("SmartProjectionRigFactor: no camera rig");
  const SmartProjectionParams& sp = sf.*SmartPoseAccess::params();
  if (sp.triangulation.enableEPI) throw std::invalid_argument("SmartProjectionRigFactor: enableEPI is not supported");
  if (sf.cameraIds().size() != sf.nonUniqueKeys().size()) throw std::invalid_argument("SmartProjectionRigFactor: camera ids and keys do not match");
  for (size_t id : sf.cameraIds()) if (id >= sf.cameraRig()->size()) throw std::invalid_argument("SmartProjectionRigFactor: camera id outside the rig");
  addSmartRows(x, sf, sf.nonUniqueKeys(), sp, sf.*SmartPoseAccess::noise(), keys, "SmartProjectionRigFactor");
  x.sm_cal.push_back(nullptr); x.sm_sen.push_back(-1); x.sm_rig.push_back(sf.cameraRig().get());
  for (size_t id : sf.cameraIds()) { x.sm_cid.push_back((int32_t)id); x.calibration(&(*sf.cameraRig())[id].calibration(), 0); }
}
// BetweenFactor<Pose3>, and <Pose2> in the same table: the factor's type follows from its variables', (x, y, theta) in the first 3 of the 12 doubles
template <class T> void addBetween(Extract& x, const BetweenFactor<T>& b, const std::vector<Key>& keys) {
  x.fac_map.emplace_back(GTG_FAC_BETWEEN_POSE3, (int64_t)x.bt_1.size());
  x.bt_1.push_back(idOf(keys, b.key1())); x.bt_2.push_back(idOf(keys, b.key2()));
  packAs(b.measured(), Extract::grow(x.bt_z, 12));
  Extract::run(x.bt_nz, b.noiseModel()); x.bt_dim.push_back(tangentDim(VarTypeOf<T>::value));
}
template <class T> void addPrior(Extract& x, const PriorFactor<T>& q, const std::vector<Key>& keys) {
  x.fac_map.emplace_back(GTG_FAC_PRIOR, (int64_t)x.pr_var.size());
  x.pr_var.push_back(idOf(keys, q.key())); x.pr_off.push_back((int64_t)x.pr_data.size());
  packAs(q.prior(), Extract::grow(x.pr_data, storageSize(VarTypeOf<T>::value)));
  Extract::run(x.pr_nz, q.noiseModel()); x.pr_dim.push_back(tangentDim(VarTypeOf<T>::value));
}
// PoseTranslationPrior / PoseRotationPrior <Pose3 | Pose2>: one row of the partial pose prior table; z: the measurement's doubles (a
// Point3, a Rot3's matrix row-major, a Point2, the (c, s) of a Rot2), rows: what the noise model's dimension must be
void addPosePartial(Extract& x, int32_t kind, Key pose, const double* z, int nz, int rows, const SharedNoiseModel& nm, const std::vector<Key>& keys) {
  x.fac_map.emplace_back(GTG_FAC_POSE_PARTIAL, (int64_t)x.pp_var.size());
  x.pp_kind.push_back(kind); x.pp_var.push_back(idOf(keys, pose));
  std::copy(z, z + nz, Extract::grow(x.pp_z, 9));
  Extract::run(x.pp_nz, nm); x.pp_dim.push_back(rows);
}
void addFactor(Extract& x, const NonlinearFactor* f, const std::vector<Key>& keys) {
  if (auto s = dynamic_cast<const SfmFactor*>(f)) addSfm(x, *s, keys);
  else if (auto p = dynamic_cast<const ProjFactor*>(f)) addProjection(x, *p, keys);
  else if (auto pd = dynamic_cast<const ProjFactorDS2*>(f)) addProjection(x, *pd, keys);
  else if (auto pf = dynamic_cast<const ProjFactorFisheye*>(f)) addProjection(x, *pf, keys);
  else if (auto st = dynamic_cast<const StereoFactor*>(f)) addStereo(x, *st, keys);
  else if (auto br = dynamic_cast<const SamBearingRangeFactor*>(f)) { const Unit3 u = br->measured().bearing(); const double r = br->measured().range(); addSam(x, GTG_SAM_BEARING_RANGE, br->keys()[0], br->keys()[1], &u, &r, br->noiseModel(), keys); }
  else if (auto rf = dynamic_cast<const SamRangeFactor*>(f)) { const double r = rf->measured(); addSam(x, GTG_SAM_RANGE, rf->keys()[0], rf->keys()[1], nullptr, &r, rf->noiseModel(), keys); }
  else if (auto bf = dynamic_cast<const SamBearingFactor*>(f)) addSam(x, GTG_SAM_BEARING, bf->keys()[0], bf->keys()[1], &bf->measured(), nullptr, bf->noiseModel(), keys);
  else if (auto br2 = dynamic_cast<const Sam2BearingRangeFactor*>(f)) { const Rot2 u = br2->measured().bearing(); const double r = br2->measured().range(); addSam2(x, GTG_SAM_BEARING_RANGE, br2->keys()[0], br2->keys()[1], &u, &r, br2->noiseModel(), keys); }
  else if (auto rf2 = dynamic_cast<const Sam2RangeFactor*>(f)) { const double r = rf2->measured(); addSam2(x, GTG_SAM_RANGE, rf2->keys()[0], rf2->keys()[1], nullptr, &r, rf2->noiseModel(), keys); }
  else if (auto bf2 = dynamic_cast<const Sam2BearingFactor*>(f)) addSam2(x, GTG_SAM_BEARING, bf2->keys()[0], bf2->keys()[1], &bf2->measured(), nullptr, bf2->noiseModel(), keys);
  else if (auto sf = dynamic_cast<const SmartFactor*>(f)) addSmart(x, *sf, keys);
  else if (auto sp = dynamic_cast<const SmartPoseFactor*>(f)) addSmartPose(x, *sp, keys);
  else if (auto sr = dynamic_cast<const SmartRigFactor*>(f)) addSmartRig(x, *sr, keys);
  else if (auto bb = dynamic_cast<const BetweenFactor<Pose3>*>(f)) addBetween(x, *bb, keys);
  else if (auto b2 = dynamic_cast<const BetweenFactor<Pose2>*>(f)) addBetween(x, *b2, keys);
  else if (auto t3 = dynamic_cast<const TranslationPrior3*>(f)) { const Point3& t = t3->measured(); const double z[3] = {t.x(), t.y(), t.z()}; addPosePartial(x, GTG_POSE_PARTIAL_TRANSLATION, t3->key(), z, 3, 3, t3->noiseModel(), keys); }
  else if (auto r3 = dynamic_cast<const RotationPrior3*>(f)) { double z[12]; packPose(Pose3(r3->measured(), Point3(0, 0, 0)), z); addPosePartial(x, GTG_POSE_PARTIAL_ROTATION, r3->key(), z, 9, 3, r3->noiseModel(), keys); }
  else if (auto t2 = dynamic_cast<const TranslationPrior2*>(f)) { const double z[2] = {t2->measured().x(), t2->measured().y()}; addPosePartial(x, GTG_POSE_PARTIAL_TRANSLATION, t2->key(), z, 2, 2, t2->noiseModel(), keys); }
  else if (auto r2 = dynamic_cast<const RotationPrior2*>(f)) { const double z[2] = {r2->measured().c(), r2->measured().s()}; addPosePartial(x, GTG_POSE_PARTIAL_ROTATION, r2->key(), z, 2, 1, r2->noiseModel(), keys); }
  else if (auto q2 = dynamic_cast<const PriorFactor<Pose2>*>(f)) addPrior(x, *q2, keys);
  else if (auto pp = dynamic_cast<const PriorFactor<Pose3>*>(f)) addPrior(x, *pp, keys);
  else if (auto pc = dynamic_cast<const PriorFactor<SfmCamera>*>(f)) addPrior(x, *pc, keys);
  else if (auto p3 = dynamic_cast<const PriorFactor<Point3>*>(f)) addPrior(x, *p3, keys);
  else throw std::invalid_argument("GpuLevenbergMarquardtOptimizer: factor type outside the GPU hot path "   // (anything else is a hard error)
                                   "(supported: GeneralSFMFactor<SfmCamera,Point3>, GenericProjectionFactor<Pose3,Point3,Cal3_S2|Cal3DS2|Cal3Fisheye>, "
                                   "GenericStereoFactor<Pose3,Point3>, BearingRangeFactor|RangeFactor|BearingFactor<Pose3,Point3> and <Pose2,Point2>, SmartProjectionFactor<SfmCamera>, SmartProjectionPoseFactor<Cal3_S2>, SmartProjectionRigFactor<PinholePose<Cal3_S2>>, BetweenFactor<Pose3|Pose2>, PriorFactor<Pose3|Pose2|SfmCamera|Point3>, PoseTranslationPrior|PoseRotationPrior<Pose3|Pose2>)");
}
// The factors [b, e) of `graph` into x, each pointer also copied into `graphCopy`; the chunk stops at its first offending factor and keeps what that threw.
void extractChunk(Extract& x, const NonlinearFactorGraph& graph, NonlinearFactorGraph& graphCopy, const std::vector<Key>& keys, size_t b, size_t e) {
  x.fac_map.reserve(e - b);
  x.sm_ptr.push_back(0);
  // (a chunk is nearly always one kind of factor: room for that kind up front -- vectors that grow by doubling go through mmap / munmap
  // above 128 KB, and 16 threads doing that held up the thread that deep-copies the Values: it was the last thing the constructor
  // waited for, 7 ms with 32 extraction threads, 0.3 ms with 16 -- round 6, L1723 shape)
  if (b < e && graph.begin()[b]) {
    const NonlinearFactor* f0 = graph.begin()[b].get();
    if (dynamic_cast<const SfmFactor*>(f0)) { x.sfm_cam.reserve(e - b); x.sfm_pt.reserve(e - b); x.sfm_z.reserve(2 * (e - b)); }
    else if (dynamic_cast<const ProjFactor*>(f0) || dynamic_cast<const ProjFactorDS2*>(f0) || dynamic_cast<const ProjFactorFisheye*>(f0)) { x.pj_pose.reserve(e - b); x.pj_pt.reserve(e - b); x.pj_sen.reserve(e - b); x.pj_z.reserve(2 * (e - b)); x.pj_cal.reserve(e - b); }
    else if (dynamic_cast<const BetweenFactor<Pose3>*>(f0) || dynamic_cast<const BetweenFactor<Pose2>*>(f0)) { x.bt_1.reserve(e - b); x.bt_2.reserve(e - b); x.bt_z.reserve(12 * (e - b)); x.bt_dim.reserve(e - b); }
  }
  try {
    for (size_t i = b; i < e; i++) {
      const auto& f = (graphCopy.at(i) = graph.begin()[i]);   // (graph[i] returns a COPY of the pointer: two more atomic operations per factor)
      if (f) addFactor(x, f.get(), keys); else x.fac_map.emplace_back(-1, 0);
    }
  } catch (...) { x.err = std::current_exception(); }
}
// ---- the merged tables.  The GeneralSFM tables -- 30 MB on the L1723 shape -- are plain buffers, not value-initialised: threads fill them (mergeTables)
template <class T> struct Raw {
  std::unique_ptr<T[]> p; size_t n = 0;
  void alloc(size_t k) { p.reset(new T[k ? k : 1]); n = k; }
  T* data() const { return p.get(); } size_t size() const { return n; }
};
typedef Raw<int32_t> RawI; typedef Raw<double> RawD;
struct Place { int64_t o_sfm, o_pj, o_st, o_sam, o_bt, o_pr, o_sm, o_pp, o_s2; std::vector<std::pair<int64_t, int32_t>> sfm_rows; };   // per chunk: offsets of its tables, (count, noise row) of its GeneralSFM runs
struct HostProblem {
  NoiseTable nt;
  RawI sfm_cam, sfm_pt, sfm_nz;
  RawD sfm_z;
  std::vector<int32_t> pj_pose, pj_pt, pj_nz, pj_cal, pj_sen, st_pose, st_pt, st_nz, st_cal, st_sen, sam_kind, sam_pose, sam_pt, sam_nz, bt_1, bt_2, bt_nz, pr_var, pr_nz, sm_cam, sm_nz, sm_cal, sm_sen, sm_mcal, sm_msen, pp_kind, pp_var, pp_nz, s2_kind, s2_pose, s2_pt, s2_nz;
  std::vector<double> pj_z, st_z, sam_z, calib, sensor, rig_sensor, bt_z, pr_data, sm_z, sm_prm, pp_z, s2_z;   // (rig_sensor: the rigs' extrinsics, appended to `sensor` behind every chunk's rows)
  std::vector<int64_t> pr_off, sm_ptr{0};    // (smart factors: one track each)
  bool any_smart_pose = false;               // a SmartProjectionPoseFactor: the smart_calib / smart_sensor tables go to the library
  bool any_smart_rig = false;                // a SmartProjectionRigFactor: sm_mcal / sm_msen (per smart measurement) go to the library too
  std::map<std::pair<const void*, int32_t>, std::pair<int32_t, int32_t>> rig_rows;   // (rig object, camera id) -> (calib row, sensor row or -1)
  std::map<std::array<double, 12>, int32_t> shared_sensor;   // the body_P_sensor of smart factors -> row of the sensor table
  std::map<const void*, int32_t> calib_id;   // shared calibration objects (Cal3_S2 or Cal3DS2) -> row of the calibration table
  std::vector<double> calib_dist;            // k1 k2 p1 p2 per row (zero for a Cal3_S2), k1 k2 k3 k4 of a Cal3Fisheye
  std::vector<int32_t> calib_model;          // GTG_CALIB_* per row: what gtg_set_calibration_models takes when some row is a Cal3Fisheye
  bool any_fisheye = false;
  std::vector<double> calib_base;            // baseline per row (zero unless the row is a Cal3_S2Stereo)
  bool any_distortion = false;
  template <class CAL> void pinhole(const CAL* K) { calib.insert(calib.end(), {K->fx(), K->fy(), K->skew(), K->px(), K->py()}); }
  int32_t calibRow(const void* object, int kind) {   // kind: 0 Cal3_S2, 1 Cal3DS2, 3 Cal3Fisheye
    auto it = calib_id.find(object);
    if (it != calib_id.end()) return it->second;
    it = calib_id.emplace(object, (int32_t)(calib.size() / 5)).first;
    const Cal3DS2* D = kind == 1 ? static_cast<const Cal3DS2*>(object) : nullptr;
    const Cal3Fisheye* F = kind == 3 ? static_cast<const Cal3Fisheye*>(object) : nullptr;
    calib_model.push_back(F ? GTG_CALIB_FISHEYE : GTG_CALIB_PINHOLE);
    if (F) { pinhole(F); calib_dist.insert(calib_dist.end(), {F->k1(), F->k2(), F->k3(), F->k4()}); any_distortion = true; any_fisheye = true; }
    else if (D) { pinhole(D); calib_dist.insert(calib_dist.end(), {D->k1(), D->k2(), D->p1(), D->p2()}); any_distortion = true; }
    else { pinhole(static_cast<const Cal3_S2*>(object)); calib_dist.insert(calib_dist.end(), {0.0, 0.0, 0.0, 0.0}); }
    calib_base.push_back(0.0);
    return it->second;
  }
  // the rows of camera `id` of a rig: its K like any shared calibration object, its extrinsic as a row of rig_sensor -- none (-1) for
  // an identity pose, whose composition with the body pose returns the body pose's own numbers
  std::pair<int32_t, int32_t> rigRows(const SmartRigFactor::Cameras* rig, int32_t id) {
    auto it = rig_rows.find({rig, id});
    if (it != rig_rows.end()) return it->second;
    const PoseCamera& cam = (*rig)[(size_t)id];
    const int32_t ci = calibRow(&cam.calibration(), 0);
    int32_t si = -1;
    if (!cam.pose().equals(Pose3(), 0.0)) { si = (int32_t)(rig_sensor.size() / 12); rig_sensor.resize(rig_sensor.size() + 12); packPose(cam.pose(), rig_sensor.data() + rig_sensor.size() - 12); }
    return rig_rows.emplace(std::make_pair((const void*)rig, id), std::make_pair(ci, si)).first->second;
  }
  int32_t stereoCalibRow(const Cal3_S2Stereo* K) {
    auto it = calib_id.find(K);
    if (it != calib_id.end()) return it->second;
    it = calib_id.emplace(K, (int32_t)(calib.size() / 5)).first;
    pinhole(K); calib_dist.insert(calib_dist.end(), {0.0, 0.0, 0.0, 0.0}); calib_base.push_back(K->baseline()); calib_model.push_back(GTG_CALIB_PINHOLE);
    return it->second;
  }
  gtg_problem view(const std::vector<int32_t>& var_type) const {   // (pointers into this object and into var_type: both outlive the upload)
    gtg_problem pb{};
    pb.n_vars = (int32_t)var_type.size(); pb.var_type = var_type.data();
    pb.n_noise = (int32_t)nt.kind.size(); pb.noise_kind = nt.kind.data(); pb.noise_dim = nt.dim.data();
    pb.noise_off = nt.off.data(); pb.noise_data = nt.data.data();
    pb.noise_robust = nt.rkind.data(); pb.noise_robust_param = nt.rparam.data();
    pb.n_sfm = (int64_t)sfm_cam.size(); pb.sfm_cam = sfm_cam.data(); pb.sfm_point = sfm_pt.data(); pb.sfm_z = sfm_z.data(); pb.sfm_noise = sfm_nz.data();
    pb.n_proj = (int64_t)pj_pose.size(); pb.proj_pose = pj_pose.data(); pb.proj_point = pj_pt.data(); pb.proj_z = pj_z.data();
    pb.proj_noise = pj_nz.data(); pb.proj_calib = pj_cal.data(); pb.proj_sensor = pj_sen.data();
    pb.n_calib = (int32_t)(calib.size() / 5); pb.calib = calib.data(); pb.calib_distortion = any_distortion ? calib_dist.data() : nullptr;
    pb.n_sensor = (int32_t)(sensor.size() / 12); pb.sensor = sensor.data();
    pb.n_stereo = (int64_t)st_pose.size(); pb.stereo_pose = st_pose.data(); pb.stereo_point = st_pt.data(); pb.stereo_z = st_z.data();
    pb.stereo_noise = st_nz.data(); pb.stereo_calib = st_cal.data(); pb.stereo_sensor = st_sen.data();
    pb.calib_baseline = pb.n_stereo ? calib_base.data() : nullptr;
    pb.n_sam = (int64_t)sam_pose.size(); pb.sam_kind = sam_kind.data(); pb.sam_pose = sam_pose.data(); pb.sam_point = sam_pt.data();
    pb.sam_z = sam_z.data(); pb.sam_noise = sam_nz.data();
    pb.n_between = (int64_t)bt_1.size(); pb.between_v1 = bt_1.data(); pb.between_v2 = bt_2.data(); pb.between_z = bt_z.data(); pb.between_noise = bt_nz.data();
    pb.n_smart = (int64_t)sm_nz.size(); pb.smart_ptr = sm_ptr.data(); pb.smart_cam = sm_cam.data(); pb.smart_z = sm_z.data();
    pb.smart_noise = sm_nz.data(); pb.smart_params = sm_prm.data();
    pb.smart_calib = any_smart_pose ? sm_cal.data() : nullptr; pb.smart_sensor = any_smart_pose ? sm_sen.data() : nullptr;
    pb.smart_meas_calib = any_smart_rig ? sm_mcal.data() : nullptr; pb.smart_meas_sensor = any_smart_rig ? sm_msen.data() : nullptr;
    pb.n_prior = (int64_t)pr_var.size(); pb.prior_var = pr_var.data(); pb.prior_off = pr_off.data(); pb.prior_data = pr_data.data(); pb.prior_noise = pr_nz.data();
    pb.n_pose_partial = (int64_t)pp_var.size();
    if (pb.n_pose_partial) { pb.pose_partial_kind = pp_kind.data(); pb.pose_partial_var = pp_var.data(); pb.pose_partial_z = pp_z.data(); pb.pose_partial_noise = pp_nz.data(); }
    pb.planar.n_sam2 = (int64_t)s2_pose.size();
    if (pb.planar.n_sam2) { pb.planar.sam2_kind = s2_kind.data(); pb.planar.sam2_pose = s2_pose.data(); pb.planar.sam2_point = s2_pt.data(); pb.planar.sam2_z = s2_z.data(); pb.planar.sam2_noise = s2_nz.data(); }
    return pb;
  }
};
// Variables in Values order (sorted by Key, Values.h:74-79): `keys` and a pointer to every Value.  The walk over the map is pointer
// chasing (1.5 - 5 ms for the 158 000 variables of the L1723 shape, beside the two copier threads); it is cut into key ranges walked
// side by side: the range boundaries are lower_bound()s of keys interpolated inside every symbol's index range (Symbol keys: character
// in the top byte, Key.h / Symbol.h; plain integer keys are one such range), so the pieces are equal where the indices are dense and
// merely unequal where they are not.  Classification (a chain of dynamic_casts) runs on the extraction's threads, each thread its
// range; the values are packed on threads while the factor tables are merged.
void walkValues(const Values& initial, std::vector<Key>* keys, std::vector<const Value*>* vptr, Lap& lap) {
  const size_t nvars = initial.size();
  keys->reserve(nvars); vptr->reserve(nvars);
  const char* walk_env = std::getenv("GTG_VALUES_WALKERS");   // (tests: the split walk on small graphs)
  const size_t walkers = nvars < 2 ? 1 : walk_env ? (size_t)std::max(1, std::atoi(walk_env)) : nvars >= 32768 ? 4 : 1;
  std::vector<Values::deref_iterator> cuts;           // walker t takes [cuts[t], cuts[t + 1])
  cuts.push_back(initial.begin());
  if (walkers > 1) {
    struct Seg { Key first, last; };
    std::vector<Seg> segs;                            // the keys of one symbol character each
    for (auto it = initial.begin(); it != initial.end();) {
      const Key first = (*it).key, top = first >> 56;
      auto next = top == 0xFF ? initial.end() : initial.lower_bound((top + 1) << 56);
      auto last = next; --last.it_;
      segs.push_back(Seg{first, (*last).key});
      it = next;
    }
    long double total = 0;
    for (const Seg& g : segs) total += (long double)(g.last - g.first) + 1;
    size_t gi = 0; long double before = 0;
    for (size_t t = 1; t < walkers; t++) {
      const long double want = total * t / walkers;
      while (gi + 1 < segs.size() && before + (long double)(segs[gi].last - segs[gi].first) + 1 <= want) { before += (long double)(segs[gi].last - segs[gi].first) + 1; gi++; }
      const Key k = segs[gi].first + (Key)std::min<long double>(want - before, (long double)(segs[gi].last - segs[gi].first));
      cuts.push_back(initial.lower_bound(k));
    }
  }
  cuts.push_back(initial.end());
  lap("(variables: key ranges)");
  const size_t pieces = cuts.size() - 1;
  std::vector<std::vector<Key>> pk(pieces);
  std::vector<std::vector<const Value*>> pv(pieces);
  parallelRanges(pieces, pieces, [&](size_t t, size_t, size_t) {
    pk[t].reserve(nvars / pieces + 16); pv[t].reserve(nvars / pieces + 16);
    for (auto it = cuts[t]; it != cuts[t + 1]; ++it) { const auto kv = *it; pk[t].push_back(kv.key); pv[t].push_back(&kv.value); }
  });
  lap("(variables: walk)");
  for (size_t t = 0; t < pieces; t++) { keys->insert(keys->end(), pk[t].begin(), pk[t].end()); vptr->insert(vptr->end(), pv[t].begin(), pv[t].end()); }
  if (keys->size() != nvars) throw std::logic_error("GpuLevenbergMarquardtOptimizer: the walk over the Values lost variables");
}
// Host threads, a range each: every factor into the Extract of its chunk (and its pointer into graphCopy, sized by the caller), every variable's
// type into var_type.  Throws for a variable of an unsupported type, else what the first offending factor in graph order threw.
std::vector<Extract> extractFactors(const NonlinearFactorGraph& graph, NonlinearFactorGraph& graphCopy, const std::vector<const Value*>& vptr,
                                    const std::vector<Key>& keys, std::vector<int32_t>* var_type) {
  const size_t nfac = graph.size(), nvars = vptr.size();
  const size_t grain = std::getenv("GTG_EXTRACT_GRAIN") ? std::max(1, std::atoi(std::getenv("GTG_EXTRACT_GRAIN"))) : 4096;   // factors per thread at least (tests: 1)
  const size_t nthreads = std::max<size_t>(1, std::min<size_t>(hostThreads(16), nfac / grain + 1));
  var_type->assign(nvars, -1);
  std::vector<Extract> part(nthreads);
  parallelRanges(nfac, nthreads, [&](size_t ti, size_t b, size_t e) {
    for (size_t v = cut(nvars, nthreads, ti); v < cut(nvars, nthreads, ti + 1); v++) (*var_type)[v] = classify(vptr[v]);   // (-1: unsupported, reported below)
    extractChunk(part[ti], graph, graphCopy, keys, b, e);
  });
  for (size_t v = 0; v < nvars; v++)
    if ((*var_type)[v] < 0) throw std::invalid_argument("GpuLevenbergMarquardtOptimizer: unsupported value type for key " + DefaultKeyFormatter(keys[v]));
  for (const Extract& x : part) if (x.err) std::rethrow_exception(x.err);   // the first offending factor in graph order
  return part;
}
// offsets of the packed values / of the tangent vector
void layoutValues(const std::vector<int32_t>& var_type, std::vector<int64_t>* val_off, std::vector<int64_t>* dim_off) {
  const size_t nvars = var_type.size();
  val_off->assign(nvars + 1, 0); dim_off->assign(nvars + 1, 0);
  for (size_t v = 0; v < nvars; v++) { (*val_off)[v + 1] = (*val_off)[v] + storageSize(var_type[v]); (*dim_off)[v + 1] = (*dim_off)[v] + tangentDim(var_type[v]); }
}
// Merge in graph order: the chunks' tables concatenated, noise / calibration rows in first-occurrence order; fac_map: (type, index in the merged table)
HostProblem mergeTables(const std::vector<Extract>& part, size_t nfac, FactorMap* fac_map) {
  HostProblem hp;
  auto cat = [](auto& dst, const auto& src) { dst.insert(dst.end(), src.begin(), src.end()); };
  auto rows = [&hp](std::vector<int32_t>& dst, const Extract::Runs& runs, const std::vector<int32_t>* expect_dim) {
    size_t at = 0;
    for (const auto& r : runs) { dst.insert(dst.end(), (size_t)r.first, hp.nt.add(r.second, expect_dim ? (size_t)(*expect_dim)[at] : 2)); at += (size_t)r.first; }
  };
  auto rows3 = [&hp](std::vector<int32_t>& dst, const Extract::Runs& runs) { for (const auto& r : runs) dst.insert(dst.end(), (size_t)r.first, hp.nt.add(r.second, 3)); };
  size_t n_sfm = 0, n_pj = 0, n_bt = 0;
  for (const Extract& x : part) { n_sfm += x.sfm_cam.size(); n_pj += x.pj_pose.size(); n_bt += x.bt_1.size(); }
  hp.sfm_cam.alloc(n_sfm); hp.sfm_pt.alloc(n_sfm); hp.sfm_nz.alloc(n_sfm); hp.sfm_z.alloc(2 * n_sfm);
  hp.pj_pose.reserve(n_pj); hp.pj_pt.reserve(n_pj); hp.pj_nz.reserve(n_pj); hp.pj_cal.reserve(n_pj); hp.pj_sen.reserve(n_pj); hp.pj_z.reserve(2 * n_pj);
  hp.bt_1.reserve(n_bt); hp.bt_2.reserve(n_bt); hp.bt_nz.reserve(n_bt); hp.bt_z.reserve(12 * n_bt);
  fac_map->clear(); fac_map->resize(nfac);
  std::vector<Place> place(part.size());
  int64_t o_sfm_next = 0;
  for (size_t pi = 0; pi < part.size(); pi++) {
    const Extract& x = part[pi];
    const int64_t o_prd = (int64_t)hp.pr_data.size(), o_smc = (int64_t)hp.sm_cam.size();
    // the chunk's sensor rows into the table, in graph order: a projection / stereo factor's row as it is, a smart factor's shared
    // by value with the rows other smart factors brought (one body_P_sensor for a whole front end) -- the rows of a one-thread pass
    std::vector<int32_t> sen_row(x.sensor.size() / 12);
    for (size_t r = 0; r < sen_row.size(); r++) {
      const double* sp = x.sensor.data() + 12 * r;
      if (x.sensor_shared[r]) {
        std::array<double, 12> key; std::copy(sp, sp + 12, key.begin());
        auto it = hp.shared_sensor.find(key);
        if (it != hp.shared_sensor.end()) { sen_row[r] = it->second; continue; }
        hp.shared_sensor.emplace(key, (int32_t)(hp.sensor.size() / 12));
      }
      sen_row[r] = (int32_t)(hp.sensor.size() / 12);
      hp.sensor.insert(hp.sensor.end(), sp, sp + 12);
    }
    for (const auto& kc : x.cal_order) { if (kc.second == 2) hp.stereoCalibRow(static_cast<const Cal3_S2Stereo*>(kc.first)); else hp.calibRow(kc.first, kc.second); }
    place[pi].o_sfm = o_sfm_next; place[pi].o_pj = (int64_t)hp.pj_pose.size(); place[pi].o_st = (int64_t)hp.st_pose.size(); place[pi].o_sam = (int64_t)hp.sam_pose.size(); place[pi].o_bt = (int64_t)hp.bt_1.size();
    place[pi].o_pr = (int64_t)hp.pr_var.size(); place[pi].o_sm = (int64_t)hp.sm_nz.size(); place[pi].o_pp = (int64_t)hp.pp_var.size(); place[pi].o_s2 = (int64_t)hp.s2_pose.size();
    o_sfm_next += (int64_t)x.sfm_cam.size();
    for (const auto& r : x.sfm_nz) place[pi].sfm_rows.emplace_back(r.first, hp.nt.add(r.second, 2));
    cat(hp.pj_pose, x.pj_pose); cat(hp.pj_pt, x.pj_pt); cat(hp.pj_z, x.pj_z);
    rows(hp.pj_nz, x.pj_nz, nullptr);
    for (int32_t sidx : x.pj_sen) hp.pj_sen.push_back(sidx < 0 ? -1 : sen_row[(size_t)sidx]);
    for (const auto& kc : x.pj_cal) hp.pj_cal.push_back(hp.calibRow(kc.first, kc.second));
    cat(hp.st_pose, x.st_pose); cat(hp.st_pt, x.st_pt); cat(hp.st_z, x.st_z);
    rows3(hp.st_nz, x.st_nz);
    for (int32_t sidx : x.st_sen) hp.st_sen.push_back(sidx < 0 ? -1 : sen_row[(size_t)sidx]);
    for (const Cal3_S2Stereo* K : x.st_cal) hp.st_cal.push_back(hp.stereoCalibRow(K));
    cat(hp.sam_kind, x.sam_kind); cat(hp.sam_pose, x.sam_pose); cat(hp.sam_pt, x.sam_pt); cat(hp.sam_z, x.sam_z);
    rows(hp.sam_nz, x.sam_nz, &x.sam_dim);
    cat(hp.s2_kind, x.s2_kind); cat(hp.s2_pose, x.s2_pose); cat(hp.s2_pt, x.s2_pt); cat(hp.s2_z, x.s2_z);
    rows(hp.s2_nz, x.s2_nz, &x.s2_dim);
    cat(hp.bt_1, x.bt_1); cat(hp.bt_2, x.bt_2); cat(hp.bt_z, x.bt_z);
    rows(hp.bt_nz, x.bt_nz, &x.bt_dim);
    cat(hp.pr_var, x.pr_var); cat(hp.pr_data, x.pr_data);
    for (int64_t o : x.pr_off) hp.pr_off.push_back(o + o_prd);
    rows(hp.pr_nz, x.pr_nz, &x.pr_dim);
    cat(hp.pp_kind, x.pp_kind); cat(hp.pp_var, x.pp_var); cat(hp.pp_z, x.pp_z);
    rows(hp.pp_nz, x.pp_nz, &x.pp_dim);
    cat(hp.sm_cam, x.sm_cam); cat(hp.sm_z, x.sm_z); cat(hp.sm_prm, x.sm_prm);
    for (size_t k = 1; k < x.sm_ptr.size(); k++) hp.sm_ptr.push_back(x.sm_ptr[k] + o_smc);
    rows(hp.sm_nz, x.sm_nz, nullptr);
    for (size_t f = 0; f < x.sm_cal.size(); f++) {
      const Cal3_S2* K = x.sm_cal[f];
      const SmartRigFactor::Cameras* rig = x.sm_rig[f];
      hp.sm_cal.push_back(rig ? GTG_SMART_RIG : K ? hp.calibRow(K, 0) : -1);
      hp.any_smart_pose = hp.any_smart_pose || K || rig; hp.any_smart_rig = hp.any_smart_rig || rig;
      for (int64_t k = x.sm_ptr[f]; k < x.sm_ptr[f + 1]; k++) {      // the per-measurement rows: -1 at the measurements of other factors
        const std::pair<int32_t, int32_t> rows = rig ? hp.rigRows(rig, x.sm_cid[(size_t)k]) : std::make_pair(-1, -1);
        hp.sm_mcal.push_back(rows.first); hp.sm_msen.push_back(rows.second);
      }
    }
    for (int32_t sidx : x.sm_sen) hp.sm_sen.push_back(sidx < 0 ? -1 : sen_row[(size_t)sidx]);
  }
  // the rigs' extrinsics behind the sensor rows of the other factors, whatever the number of chunks
  for (int32_t& si : hp.sm_msen) if (si >= 0) si += (int32_t)(hp.sensor.size() / 12);
  cat(hp.sensor, hp.rig_sensor);
  // the big tables, by threads, one chunk each, now that the offsets and the noise rows are handed out in graph order
  parallelRanges(part.size(), part.size(), [&](size_t pi, size_t, size_t) {
    const Extract& x = part[pi];
    const Place& pl = place[pi];
    const size_t k = x.sfm_cam.size();
    if (k) {
      std::memcpy(hp.sfm_cam.data() + pl.o_sfm, x.sfm_cam.data(), 4 * k); std::memcpy(hp.sfm_pt.data() + pl.o_sfm, x.sfm_pt.data(), 4 * k);
      std::memcpy(hp.sfm_z.data() + 2 * pl.o_sfm, x.sfm_z.data(), 16 * k);
      int32_t* nz = hp.sfm_nz.data() + pl.o_sfm;
      for (const auto& r : pl.sfm_rows) { std::fill(nz, nz + r.first, r.second); nz += r.first; }
    }
    auto* fm_out = fac_map->data() + cut(nfac, part.size(), pi);     // (the chunk's factors: the range extractFactors gave it)
    for (const auto& fm : x.fac_map)
      *fm_out++ = {fm.first, fm.second + (fm.first == GTG_FAC_GENERAL_SFM ? pl.o_sfm : fm.first == GTG_FAC_PROJECTION ? pl.o_pj : fm.first == GTG_FAC_STEREO ? pl.o_st : fm.first == GTG_FAC_SAM ? pl.o_sam :
                                           fm.first == GTG_FAC_BETWEEN_POSE3 ? pl.o_bt : fm.first == GTG_FAC_PRIOR ? pl.o_pr : fm.first == GTG_FAC_POSE_PARTIAL ? pl.o_pp : fm.first == GTG_FAC_SAM2 ? pl.o_s2 : fm.first == -2 ? pl.o_sm : 0)};
  });
  return hp;
}
}  // namespace

void GpuLevenbergMarquardtOptimizer::init(const NonlinearFactorGraph& graph, const Values& initial, int device, const ShardSpec& shards) {
  Impl& m = *impl_;
  Lap lap;
  // Two copies the optimizer owes its base class run beside the extraction, which reads the CALLER's graph meanwhile:
  //  - graph_ (NonlinearOptimizer.h:78): one shared-pointer copy per factor -- 18 ms for the 0.68 M factors of the L1723 shape;
  //  - a deep copy of the caller's Values (one heap object per variable).  It stays in the Impl: values() needs a Values object
  //    inside a State, and BOTH constructors of LevenbergMarquardtState deep-copy what they are given (the Values&& one passes
  //    its argument on as an lvalue, LevenbergMarquardtState.h:61-63), so the cheapest way to a current State is to overwrite the
  //    payloads of this copy in place (syncValuesToHost) and let the constructor copy it.
  //  - `slots` (variable id -> the GenericValue object of the copy): one walk over the copy's map, made by the same thread.
  // Two threads: the two copies are as long as each other (18 + 16 ms on the L1723 shape) and as the whole of the library's set-up beside them.
  std::exception_ptr copyErr, copyErr2;
  // (graph_: the copy used to run on a thread of its own -- a second pass of cache misses over the 0.68 M factors beside the extraction's,
  // and with the deep copy of the Values the last thing the constructor waited for.  The extraction threads make it now, each factor
  // while it is in the thread's cache anyway.)
  std::thread copier([&] { try { graph_.resize(graph.size()); } catch (...) { copyErr = std::current_exception(); } });
  std::thread copier2([&] {
    try {
      m.scratch = initial;
      m.slots.clear(); m.slots.reserve(m.scratch.size());
      for (const auto& kv : m.scratch) m.slots.push_back(const_cast<Value*>(&kv.value));   // (the GenericValue objects are non-const heap objects owned by the map's nodes)
    } catch (...) { copyErr2 = std::current_exception(); }
  });
  Join joinCopier{copier}, joinCopier2{copier2};
  // The one-time work of the process -- HIP runtime start, code-object load, function objects of every kernel -- starts on a helper
  // thread now and runs under the host passes below (gtg_prewarm is idempotent: later constructions return at once).
  std::thread prewarmer([device] { gtg_prewarm(device); });
  Join joinPrewarmer{prewarmer};
  lap("(threads started)");
  std::vector<const Value*> vptr;
  walkValues(initial, &m.keys, &vptr, lap);
  const size_t nvars = m.keys.size();
  lap("variables: keys + value pointers");
  copier.join();   // (the extraction's threads fill the graph_ it sized)
  if (copyErr) std::rethrow_exception(copyErr);
  const std::vector<Extract> part = extractFactors(graph, graph_, vptr, m.keys, &m.var_type);
  lap("factors: extraction, variables: classification (host threads)");
  // the packing itself on threads beside the merge of the factor tables
  layoutValues(m.var_type, &m.val_off, &m.dim_off);
  m.packed.resize((size_t)m.val_off[nvars]);
  const size_t npack = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(part.size(), 8), nvars / 8192 + 1));
  std::vector<std::thread> packers;
  JoinAll joinPackers{packers};
  startRanges(packers, nvars, npack, 0, [&](size_t, size_t b, size_t e) {
    for (size_t v = b; v < e; v++) pack(m.var_type[v], *vptr[v], m.packed.data() + m.val_off[v]);
  });
  const HostProblem hp = mergeTables(part, graph.size(), &m.fac_map);
  lap("factors: merge, noise / calibration tables");
  const gtg_problem pb = hp.view(m.var_type);
  m.sam_kind = hp.sam_kind; m.pp_kind = hp.pp_kind; m.sam2_kind = hp.s2_kind;
  if (shards.n_shards < 1 || shards.shard < 0 || shards.shard >= shards.n_shards) throw std::invalid_argument("GpuLevenbergMarquardtOptimizer: bad ShardSpec");
  if (shards.n_shards > 1 && !shards.allreduce) throw std::invalid_argument("GpuLevenbergMarquardtOptimizer: n_shards > 1 needs an all-reduce callback");
  for (auto& t : packers) t.join();
  lap("variables: packed (threads, beside the merge)");
  // (the prewarm thread is NOT waited for here: gtg_create below blocks inside the runtime until it has started, and the upload's first
  // launches either find their kernels loaded or load them themselves, while the helper goes on to the per-try kernels)
  check(gtg_create(&m.h, device), "gtg_create");
  if (shards.allreduce) check(gtg_set_allreduce(m.h, shards.allreduce, shards.user), "gtg_set_allreduce");   // before the upload: it verifies the layout across the shards
  // (a Cal3Fisheye row: its model goes beside the problem, consumed by the upload that follows)
  if (hp.any_fisheye) check(gtg_set_calibration_models(m.h, hp.calib_model.data(), (int32_t)hp.calib_model.size()), "gtg_set_calibration_models");
  check(gtg_upload_problem(m.h, &pb, shards.shard, shards.n_shards), "gtg_upload_problem");
  check(gtg_set_values(m.h, m.packed.data(), (int64_t)m.packed.size()), "gtg_set_values");
  lap("library: create + upload + set_values");
  // State(initialValues, graph.error(initialValues), lambdaInitial, lambdaFactor) -- LevenbergMarquardtOptimizer.cpp:47-53 -- with
  // the error evaluated on the device
  double e0 = 0.0;
  check(gtg_error(m.h, &e0), "gtg_error");
  lap("device: initial error");
  copier2.join();
  lap("wait for the copies of the graph and the Values");
  if (copyErr2) std::rethrow_exception(copyErr2);
  // The State: the deep copy made beside the extraction moves into a GpuState (see GpuState::make: no second copy).  `slots` points
  // into the nodes of that Values' map -- heap objects that stay where they are when the map moves on into the next State -- and every
  // use checks first that state_ is still a State of this class holding that map (adoptStateIfForeign): a State published by anybody
  // else -- the inherited public tryLambda() does that -- is adopted, not written over.
  if (m.slots.size() != nvars) throw std::logic_error("GpuLevenbergMarquardtOptimizer: the copy of the Values lost variables");
  state_ = GpuState::make(std::move(m.scratch), e0, params_.lambdaInitial, params_.lambdaFactor, 0, 0);   // (`slots`, collected by the copier thread, points into the nodes that move here)
  m.published = &state_->values;
  m.takeScalars(*static_cast<const State*>(state_.get()));
  lap("state");
  prewarmer.join();
  lap("wait for the prewarm thread");
}

// state_ was replaced or changed by code outside this class since this class last published it.  LevenbergMarquardtOptimizer::tryLambda is
// public and non-virtual: it solves (through the overridden solve()), retracts and evaluates on the CPU, and then EITHER installs a new plain
// LevenbergMarquardtState with a deep copy of ITS new values (accepted step, LM.cpp:246-249) OR raises lambda IN PLACE on the State it
// found (rejected step, LM.cpp:262-268).  The device follows the host in both cases:
//  - a State that is not a GpuState, or a GpuState that does not hold the map `slots` points into: values re-packed and uploaded, `slots`
//    rebuilt on its nodes (identity = the dynamic type; an address can be handed out again by the allocator between two foreign States);
//  - in every case the scalars (error, lambda, factor, both counters) are taken from the State: an in-place increaseLambda() on our own
//    State changes nothing else.
void GpuLevenbergMarquardtOptimizer::adoptStateIfForeign() const {
  Impl& m = *impl_;
  const State* st = static_cast<const State*>(state_.get());
  const bool ours = dynamic_cast<const GpuState*>(state_.get()) != nullptr && m.published == &state_->values && state_->values.size() == m.slots.size();
  if (!ours) {
    const Values& v = state_->values;
    if (v.size() != m.keys.size()) throw std::logic_error("GpuLevenbergMarquardtOptimizer: the optimizer's State holds other variables than the graph was uploaded with");
    m.slots.clear(); m.slots.reserve(m.keys.size());
    size_t id = 0;
    for (const auto& kv : v) {
      if (kv.key != m.keys[id]) throw std::logic_error("GpuLevenbergMarquardtOptimizer: the optimizer's State holds other variables than the graph was uploaded with");
      if (classify(&kv.value) != m.var_type[id]) throw std::bad_cast();   // (what Value::cast<T>() throws: a variable that changed its type)
      pack(m.var_type[id], kv.value, m.packed.data() + m.val_off[id]);
      m.slots.push_back(const_cast<Value*>(&kv.value));
      id++;
    }
    check(gtg_set_values(m.h, m.packed.data(), (int64_t)m.packed.size()), "gtg_set_values");
    m.host_values_stale = false;
    m.published = &state_->values;
  }
  m.takeScalars(*st);
}

void GpuLevenbergMarquardtOptimizer::syncValuesToHost(bool force) {
  Impl& m = *impl_;
  if (!m.host_values_stale && !force) return;
  if (m.published != &state_->values)     // (the public entry points adopt a foreign State before they touch the device: cannot happen through them)
    throw std::logic_error("GpuLevenbergMarquardtOptimizer: the optimizer's State was replaced while the values were on the device");
  if (m.host_values_stale) {
    check(gtg_get_values(m.h, m.packed.data(), (int64_t)m.packed.size()), "gtg_get_values");
    // overwrite the payloads of the State's Values in place (m.slots: the GenericValue objects by variable id), host threads
    const size_t nv = m.slots.size();
    const size_t nthreads = std::max<size_t>(1, std::min<size_t>(hostThreads(32), nv / 8192 + 1));   // (8 until round 6: the 1.8 M payloads of the Venice shape took 12 % of its optimize())
    parallelRanges(nv, nthreads, [&](size_t, size_t b, size_t e) {
      for (size_t v = b; v < e; v++) unpack(m.var_type[v], m.packed.data() + m.val_off[v], *m.slots[v]);
    });
  }
  // the next State, with the device's error / lambda / counters
  std::unique_ptr<GpuState> fresh;
  if (dynamic_cast<const GpuState*>(state_.get())) {
    // ours: it takes the map of the current one over (O(1); the nodes -- and with them `slots` -- move on).  The object in the current
    // State's `values` storage is the one GpuState::make created there by placement new -- an object of type Values, not const Values --
    // so it may be moved from, through a pointer to that object (std::launder).
    Values* current = std::launder(static_cast<Values*>(const_cast<void*>(static_cast<const void*>(&state_->values))));
    fresh = GpuState::make(std::move(*current), m.error, m.lambda, m.factor, (unsigned)m.iterations, (unsigned)m.inner);
  } else {
    // a State the base class published and this class adopted: its `values` IS a const member -- deep copy (once; from here on the
    // States are ours again), `slots` follows the copy's nodes
    fresh = GpuState::make(Values(state_->values), m.error, m.lambda, m.factor, (unsigned)m.iterations, (unsigned)m.inner);
    m.slots.clear();
    for (const auto& kv : fresh->values) m.slots.push_back(const_cast<Value*>(&kv.value));
  }
  state_ = std::move(fresh);
  m.published = &state_->values;
  m.host_values_stale = false;
}

// LevenbergMarquardtOptimizer::tryLambda (LM.cpp:121-270) with solve / error / retract on the device.
bool GpuLevenbergMarquardtOptimizer::tryLambdaDevice() {
  Impl& m = *impl_;
  using std::cout; using std::endl;
  const bool verbose = params_.verbosityLM >= LevenbergMarquardtParams::TRYLAMBDA;
  const auto tryStart = std::chrono::high_resolution_clock::now();
  if (verbose) cout << "trying lambda = " << m.lambda << endl;
  if (params_.verbosityLM >= LevenbergMarquardtParams::DAMPED) cout << "building damped system with lambda " << m.lambda << endl;
  double out[4] = {0, 0, 0, 0};
  int rc;
  if (params_.isIterative()) {
    // NonlinearOptimizer::solve, Iterative branch (NonlinearOptimizer.cpp:154-172): PCGSolverParameters only, and the device solver is
    // block-Jacobi PCG on the implicit Schur complement (a Dummy preconditioner or a SubgraphSolver is outside the GPU path).
    if (!params_.iterativeParams) throw std::runtime_error("NonlinearOptimizer::solve: cg parameter has to be assigned ...");
    double cg[4];
    if (!std::dynamic_pointer_cast<BlockJacobiPreconditionerParameters>(pcgParameters(params_, "GpuLevenbergMarquardtOptimizer", cg)->preconditioner))
      throw std::runtime_error("GpuLevenbergMarquardtOptimizer: the GPU PCG solver is block-Jacobi preconditioned "
                               "(set PCGSolverParameters::preconditioner to BlockJacobiPreconditionerParameters)");
    int32_t cg_iterations = 0;
    rc = gtg_try_lambda_pcg(m.h, m.lambda, params_.diagonalDamping, params_.minDiagonal, params_.maxDiagonal, cg, out, &cg_iterations);
    check(rc, "gtg_try_lambda_pcg");
  } else {
    rc = gtg_try_lambda(m.h, m.lambda, params_.diagonalDamping, params_.minDiagonal, params_.maxDiagonal, out);
    check(rc, "gtg_try_lambda");
  }
  bool step_is_successful = false, stopSearchingLambda = false;
  double modelFidelity = 0.0, newError = std::numeric_limits<double>::infinity(), costChange = 0.0;
  const bool systemSolvedSuccessfully = rc != GTG_INDETERMINATE;   // else: IndeterminantLinearSystemException path, LM.cpp:158-160
  if (systemSolvedSuccessfully) {
    if (verbose) cout << "linear delta norm = " << out[3] << endl;
    const double oldLinearizedError = out[0], newlinearizedError = out[1];
    const double linearizedCostChange = oldLinearizedError - newlinearizedError;
    if (verbose) cout << "newlinearizedError = " << newlinearizedError << "  linearizedCostChange = " << linearizedCostChange << endl;
    if (linearizedCostChange >= 0) {
      newError = out[2];
      if (verbose) cout << "calculating error:" << endl << "old error (" << m.error << ") new (tentative) error (" << newError << ")" << endl;
      costChange = m.error - newError;
      if (linearizedCostChange > std::numeric_limits<double>::epsilon() * oldLinearizedError) {
        modelFidelity = costChange / linearizedCostChange;
        step_is_successful = modelFidelity > params_.minModelFidelity;
        if (verbose) cout << "modelFidelity: " << modelFidelity << endl;
      }
      const double minAbsoluteTolerance = params_.relativeErrorTol * m.error;
      if (std::abs(costChange) < minAbsoluteTolerance) {
        if (verbose)
          cout << "abs(costChange)=" << std::abs(costChange) << "  minAbsoluteTolerance=" << minAbsoluteTolerance
               << " (relativeErrorTol=" << params_.relativeErrorTol << ")" << endl;
        stopSearchingLambda = true;
      }
    }
  }
  if (params_.verbosityLM == LevenbergMarquardtParams::SUMMARY) {   // LM.cpp:223-242
    const double iterationTime = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - tryStart).count() / 1e6;
    if (m.iterations == 0) cout << "iter      cost      cost_change    lambda  success iter_time" << endl;
    cout << std::setw(4) << m.iterations << " " << std::setw(12) << newError << " " << std::setw(12) << std::setprecision(2)
         << costChange << " " << std::setw(10) << std::setprecision(2) << m.lambda << " " << std::setw(6)
         << systemSolvedSuccessfully << " " << std::setw(10) << std::setprecision(2) << iterationTime << endl;
  }
  if (step_is_successful) {   // decreaseLambda, LevenbergMarquardtState.h:81-94
    double newLambda = m.lambda, newFactor = m.factor;
    if (params_.useFixedLambdaFactor) newLambda /= m.factor;
    else { newLambda *= std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * modelFidelity - 1.0, 3)); newFactor = 2.0 * m.factor; }
    m.lambda = std::max(params_.lambdaLowerBound, newLambda); m.factor = newFactor;
    check(gtg_accept(m.h), "gtg_accept");
    m.error = newError; m.iterations += 1; m.inner += 1; m.host_values_stale = true;
    return true;
  } else if (!stopSearchingLambda) {   // increaseLambda, LevenbergMarquardtState.h:70-76
    if (verbose) cout << "increasing lambda" << endl;
    m.lambda *= m.factor; m.inner += 1;
    if (!params_.useFixedLambdaFactor) m.factor *= 2.0;
    if (m.lambda >= params_.lambdaUpperBound) {
      if (params_.verbosity >= NonlinearOptimizerParams::TERMINATION || params_.verbosityLM == LevenbergMarquardtParams::SUMMARY)
        cout << "Warning:  Levenberg-Marquardt giving up because cannot decrease error with maximum lambda" << endl;
      return true;
    }
    return false;
  }
  if (verbose) cout << "Levenberg-Marquardt: stopping as relative cost reduction is small" << endl;
  return true;
}

// writeLogFile, LM.cpp:101-118: inner iterations, seconds, error, lambda, outer iterations
void GpuLevenbergMarquardtOptimizer::writeLogFileDevice(double currentError) {
  const Impl& m = *impl_;
  if (params_.logFile.empty()) return;
  std::ofstream os(params_.logFile.c_str(), std::ios::app);
  const double timeSpent = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - m.start).count() / 1e6;
  os << m.inner << "," << timeSpent << "," << currentError << "," << m.lambda << "," << m.iterations << std::endl;
}

// LevenbergMarquardtOptimizer::iterate (LM.cpp:273-308) on the device state
void GpuLevenbergMarquardtOptimizer::iterateDevice() {
  Impl& m = *impl_;
  if (params_.verbosityLM >= LevenbergMarquardtParams::DAMPED) std::cout << "linearizing = " << std::endl;
  check(gtg_linearize(m.h), "gtg_linearize");
  if (m.keep_linearization) m.linearization = downloadLinearization();   // iterate()'s return value: the graph linearised here
  if (m.inner == 0) {   // write initial error
    writeLogFileDevice(m.error);
    if (params_.verbosityLM == LevenbergMarquardtParams::SUMMARY)
      std::cout << "Initial error: " << m.error << ", values: " << m.keys.size() << std::endl;
  }
  while (!tryLambdaDevice()) writeLogFileDevice(m.error);
}

GaussianFactorGraph::shared_ptr GpuLevenbergMarquardtOptimizer::iterate() {
  Impl& m = *impl_;
  adoptStateIfForeign();
  m.keep_linearization = true;   // what the reference returns: `linear`, the graph linearised at the values the iteration
  iterateDevice();               // started from (LevenbergMarquardtOptimizer.cpp:277,307)
  m.keep_linearization = false;
  syncValuesToHost(true);   // iterate() is a public entry point: values()/error()/lambda() must be current
  GaussianFactorGraph::shared_ptr out = m.linearization;
  m.linearization.reset();
  return out;
}

// The device's whitened records [A1 | A2 | b] (gtg_get_jacobians) as JacobianFactors without a noise model (the records are
// whitened and, for Robust models, re-weighted -- what NoiseModelFactor::linearize returns for unconstrained models,
// NonlinearFactor.cpp:150-182), one per factor of graph_, in its order.
GaussianFactorGraph::shared_ptr GpuLevenbergMarquardtOptimizer::downloadLinearization() const {
  const Impl& m = *impl_;
  const Records records = fetchRecords(m.h, m.fac_map);
  auto out = std::make_shared<GaussianFactorGraph>();
  out->reserve(graph_.size());
  typedef Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor> RowMat;
  for (size_t i = 0; i < graph_.size(); i++) {
    const auto tf = m.fac_map[i];
    if (tf.first < 0) { out->push_back(GaussianFactor::shared_ptr()); continue; }   // (null, or a smart factor: left empty here)
    const double* r = records.of(tf);
    const KeyVector& keys = graph_[i]->keys();
    const RecordLayout lay = m.layoutOf(tf, keys[0]);
    auto block = [&](int k) { return Matrix(Eigen::Map<const RowMat, 0, Eigen::OuterStride<>>(r + lay.boff[k], lay.rows, lay.bcols[k], Eigen::OuterStride<>(lay.pitch(k)))); };
    const Vector b = Eigen::Map<const Vector>(r + lay.rhs, lay.rows);
    if (lay.nblk == 2) out->emplace_shared<JacobianFactor>(keys[0], block(0), keys[1], block(1), b);
    else out->emplace_shared<JacobianFactor>(keys[0], block(0), b);
  }
  return out;
}

GaussianFactorGraph::shared_ptr GpuLevenbergMarquardtOptimizer::linearize() const {
  adoptStateIfForeign();
  const Impl& m = *impl_;
  if (m.host_values_stale) throw std::logic_error("GpuLevenbergMarquardtOptimizer::linearize: host values out of date");   // (cannot happen through the public entry points)
  check(gtg_linearize(m.h), "gtg_linearize");
  return downloadLinearization();
}

VectorValues GpuLevenbergMarquardtOptimizer::solve(const GaussianFactorGraph& gfg, const NonlinearOptimizerParams& params) const {
  const Impl& m = *impl_;
  // Is this buildDampedSystem's output for our graph (LevenbergMarquardtState.h:125-156)?  graph_.size() linear factors, then one
  // unary JacobianFactor per variable: A = I (or diag(sqrt hessian diagonal)), b = 0, Isotropic sigma = 1 / sqrt(lambda).
  const size_t nf = graph_.size(), nv = m.keys.size();
  double lambda = 0.0; bool diagonal = false, recognised = gfg.size() == nf + nv && nv > 0;
  for (size_t v = 0; recognised && v < nv; v++) {
    auto jf = std::dynamic_pointer_cast<JacobianFactor>(gfg[nf + v]);
    auto iso = jf ? std::dynamic_pointer_cast<noiseModel::Isotropic>(jf->get_model()) : nullptr;
    if (!jf || jf->size() != 1 || !iso || jf->getb().cwiseAbs().maxCoeff() != 0.0) { recognised = false; break; }
    const double l = 1.0 / (iso->sigma() * iso->sigma());
    if (v == 0) lambda = l; else if (std::abs(l - lambda) > 1e-12 * lambda) { recognised = false; break; }
    const Matrix A = jf->getA(jf->begin());
    if (!A.isDiagonal()) { recognised = false; break; }
    if ((A.diagonal().array() != 1.0).any()) diagonal = true;
  }
  if (!recognised) return LevenbergMarquardtOptimizer::solve(gfg, params);
  const auto* lm = dynamic_cast<const LevenbergMarquardtParams*>(&params);
  const double dmin = lm ? lm->minDiagonal : params_.minDiagonal, dmax = lm ? lm->maxDiagonal : params_.maxDiagonal;
  check(gtg_linearize(m.h), "gtg_linearize");   // the device's own linearisation at values(): what `gfg` should have been built from
  // ... which is VERIFIED, not assumed, for EVERY factor: gfg's [A | b] blocks are compared with the device's raw records of the same
  // factors (same keys, same numbers to 1e-9) on host threads, without constructing a single factor object.  A graph linearised at
  // other values, or with any factor edited by the caller, has the right SHAPE but not these numbers; it goes to the reference's CPU
  // solve like any other graph.  (Entries of smart factors -- Hessian factors the device never forms -- are skipped.)
  {
    const Records records = fetchRecords(m.h, m.fac_map);
    std::atomic<bool> same{true};
    const size_t nthreads = std::max<size_t>(1, std::min<size_t>({(size_t)std::min(std::max(1u, std::thread::hardware_concurrency()), 16u), nf / 16384 + 1}));
    parallelRanges(nf, nthreads, [&](size_t, size_t b0, size_t e0) {
      for (size_t i = b0; i < e0 && same.load(std::memory_order_relaxed); i++) {
        const auto tf = m.fac_map[i];
        if (tf.first < 0) continue;
        const auto* theirs = dynamic_cast<const JacobianFactor*>(gfg[i].get());
        if (!theirs || theirs->get_model() || theirs->keys() != graph_[i]->keys()) { same = false; return; }
        const double* r = records.of(tf);
        const RecordLayout lay = m.layoutOf(tf, theirs->keys()[0]);   // (what downloadLinearization wraps: row-major blocks, then b)
        if ((int)theirs->size() != lay.nblk || (int)theirs->rows() != lay.rows) { same = false; return; }
        double scale = 1.0, worst = 0.0;
        for (int k = 0; k < lay.nblk; k++) {
          const auto A = theirs->getA(theirs->begin() + k);
          if ((int)A.cols() != lay.bcols[k]) { same = false; return; }
          for (int a = 0; a < lay.rows; a++)
            for (int cc = 0; cc < lay.bcols[k]; cc++) { const double x = A(a, cc); scale = std::max(scale, std::abs(x)); worst = std::max(worst, std::abs(x - r[lay.boff[k] + a * lay.pitch(k) + cc])); }
        }
        const auto bb = theirs->getb();
        for (int a = 0; a < lay.rows; a++) { scale = std::max(scale, std::abs(bb(a))); worst = std::max(worst, std::abs(bb(a) - r[lay.rhs + a])); }
        if (!(worst <= 1e-9 * scale)) { same = false; return; }
      }
    });
    if (!same) return LevenbergMarquardtOptimizer::solve(gfg, params);
  }
  double out[4];
  int rc;
  if (params.isIterative()) {
    double cg[4]; int32_t its = 0;
    pcgParameters(params, "GpuLevenbergMarquardtOptimizer::solve", cg);
    rc = gtg_try_lambda_pcg(m.h, lambda, diagonal, dmin, dmax, cg, out, &its);
  } else {
    rc = gtg_try_lambda(m.h, lambda, diagonal, dmin, dmax, out);
  }
  check(rc, "gtg_try_lambda");
  if (rc == GTG_INDETERMINATE) throw IndeterminantLinearSystemException(m.keys.empty() ? Key(0) : m.keys[0]);
  std::vector<double> delta((size_t)m.dim_off.back());
  check(gtg_get_delta(m.h, delta.data(), (int64_t)delta.size()), "gtg_get_delta");
  VectorValues x;
  for (size_t v = 0; v < nv; v++)
    x.insert(m.keys[v], Vector(Eigen::Map<const Vector>(delta.data() + m.dim_off[v], userDim(m.var_type[v]))));
  return x;
}

const Values& GpuLevenbergMarquardtOptimizer::optimize() {
  Impl& m = *impl_;
  adoptStateIfForeign();
  const LevenbergMarquardtParams& p = params_;
  using std::cout; using std::endl;
  double currentError = m.error;
  if (currentError <= p.errorTol) {
    if (p.verbosity >= NonlinearOptimizerParams::ERROR) cout << "Exiting, as error = " << currentError << " < " << p.errorTol << endl;
    return values();
  }
  if (p.verbosity >= NonlinearOptimizerParams::VALUES) values().print("Initial values");
  if (p.verbosity >= NonlinearOptimizerParams::ERROR) cout << "Initial error: " << currentError << endl;
  if (m.iterations >= p.maxIterations) {
    if (p.verbosity >= NonlinearOptimizerParams::TERMINATION) cout << "iterations: " << m.iterations << " >? " << p.maxIterations << endl;
    return values();
  }
  double newError = currentError;
  const bool timing = std::getenv("GTG_DEBUG_TIMING") != nullptr;
  const auto tOpt = std::chrono::high_resolution_clock::now();
  do {   // NonlinearOptimizer::defaultOptimize, NonlinearOptimizer.cpp:86-105
    currentError = newError;
    const auto tIt = std::chrono::high_resolution_clock::now();
    iterateDevice();
    if (timing) std::fprintf(stderr, "[gtsam_amd shim ]   iteration %zu: %.2f ms\n", m.iterations, std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - tIt).count());
    newError = m.error;
    if (p.iterationHook) { syncValuesToHost(false); p.iterationHook(m.iterations, currentError, newError); }
    if (p.verbosity >= NonlinearOptimizerParams::VALUES) { syncValuesToHost(false); values().print("newValues"); }
    if (p.verbosity >= NonlinearOptimizerParams::ERROR) cout << "newError: " << newError << endl;
  } while (m.iterations < p.maxIterations &&
           !checkConvergence(p.relativeErrorTol, p.absoluteErrorTol, p.errorTol, currentError, newError, p.verbosity) &&
           std::isfinite(currentError));
  if (p.verbosity >= NonlinearOptimizerParams::TERMINATION) {
    cout << "iterations: " << m.iterations << " >? " << p.maxIterations << endl;
    if (m.iterations >= p.maxIterations) cout << "Terminating because reached maximum iterations" << endl;
  }
  const auto tSync = std::chrono::high_resolution_clock::now();
  syncValuesToHost(true);
  if (timing)
    std::fprintf(stderr, "[gtsam_amd shim ] optimize(): %zu iterations %.2f ms, values back into the State %.2f ms\n", m.iterations,
                 std::chrono::duration<double, std::milli>(tSync - tOpt).count(),
                 std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - tSync).count());
  return values();
}

void GpuLevenbergMarquardtOptimizer::enablePhaseTiming(bool on) { gtg_enable_timing(impl_->h, on ? 1 : 0); }

std::vector<double> GpuLevenbergMarquardtOptimizer::phaseMilliseconds() const {
  std::vector<double> ms(GTG_PH_COUNT, 0.0);
  std::vector<int64_t> calls(GTG_PH_COUNT, 0);
  gtg_get_phase_ms(impl_->h, ms.data(), calls.data(), GTG_PH_COUNT);
  return ms;
}

std::vector<long long> GpuLevenbergMarquardtOptimizer::phaseCalls() const {
  std::vector<double> ms(GTG_PH_COUNT, 0.0);
  std::vector<int64_t> calls(GTG_PH_COUNT, 0);
  gtg_get_phase_ms(impl_->h, ms.data(), calls.data(), GTG_PH_COUNT);
  return std::vector<long long>(calls.begin(), calls.end());
}

gtg_handle GpuLevenbergMarquardtOptimizer::handle() const { return impl_->h; }

}  // namespace gtsam_amd
