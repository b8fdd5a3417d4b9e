// upload.hip -- gtg_upload_problem behind its argument checks: the caller's tables become the handle's device tables, stage by stage
// (upload_problem at the bottom is the list).  Host code only; the symbolic analysis that follows the tables is analysis.hip.
#include <algorithm>
#include <cmath>
#include <exception>
#include <stdexcept>
#include <string>
#include <thread>

#include "analysis.h"
#include "factors.h"
#include "kernels.h"

// GTG_FUSED_SFM=0 at compile time builds the stored-record form of rounds 1-4 for every graph (the A/B of the fused linearisation,
// `make records`); the product library is built with 1
#ifndef GTG_FUSED_SFM
#define GTG_FUSED_SFM 1
#endif
namespace gt {
namespace {
static_assert(proj_rec(ProjForm::Planar) == kPlanarRec, "context.h states the record lengths of factors.h");
static_assert(kSamBearingRange == GTG_SAM_BEARING_RANGE && kSamRange == GTG_SAM_RANGE && kSamBearing == GTG_SAM_BEARING, "factors.h names the sam kinds of the C ABI");
static_assert(kPartialTranslation == GTG_POSE_PARTIAL_TRANSLATION && kPartialRotation == GTG_POSE_PARTIAL_ROTATION, "factors.h names the partial pose prior kinds of the C ABI");

// Smart factors become what the rest of the library already knows: a hidden POINT3 variable per factor behind the caller's
// variables and one observation per measurement behind the caller's -- a GeneralSFM observation for a camera-type factor
// (SmartProjectionFactor<PinholeCamera<Cal3Bundler>>), a projection observation for a pose-type factor (SmartProjectionPoseFactor<Cal3_S2>:
// smart_calib >= 0) or a rig-type factor (SmartProjectionRigFactor<PinholePose<Cal3_S2>>: smart_calib == GTG_SMART_RIG, calib and sensor
// per measurement); every table is built from problem().  Without smart factors that is the caller's struct and nothing is owned.
// Pure host code.
struct SmartView {
  std::vector<int32_t> var_type, sfm_cam, sfm_point, sfm_noise, proj_pose, proj_point, proj_noise, proj_calib, proj_sensor;
  std::vector<int32_t> of_obs;   // per observation of the range the measurements joined in problem(): its smart factor, -1 for the caller's own factors
  std::vector<double> sfm_z, proj_z;
  std::vector<uint8_t> is_rig;   // per smart factor: rig-type
  bool pose = false;             // the range is the projection range
  bool repeats = false;          // some rig-type factor names a pose key more than once (the whole table: the same on every shard)
  explicit SmartView(const gtg_problem& user);
  SmartView(const SmartView&) = delete;   // (p may point at q)
  const gtg_problem& problem() const { return *p; }
 private:
  gtg_problem q; const gtg_problem* p;
  void expand_cameras(const gtg_problem& user, int64_t n_smart);
  void expand_poses(const gtg_problem& user, int64_t n_smart);
  void expand_rig(const gtg_problem& user, int64_t i);
};

SmartView::SmartView(const gtg_problem& user) : q(user), p(&user) {
  const int64_t n_smart = user.n_smart > 0 ? user.n_smart : 0;
  if (!n_smart) return;
  if (!user.smart_ptr || !user.smart_cam || !user.smart_z || !user.smart_noise || !user.smart_params)
    throw std::invalid_argument("smart factor tables missing");
  const int64_t n_meas = user.smart_ptr[n_smart];
  int64_t n_pose = 0;
  if (user.smart_calib) for (int64_t i = 0; i < n_smart; i++) n_pose += user.smart_calib[i] != -1;   // (pose-type and rig-type)
  if (n_pose != 0 && n_pose != n_smart)
    throw std::invalid_argument("smart factors: a graph that mixes camera-type (smart_calib -1) and pose-type (smart_calib >= 0) smart factors is not supported");
  pose = n_pose > 0;
  if (pose && user.n_stereo > 0)
    throw std::invalid_argument("smart factors: pose-type smart factors together with GenericStereoFactors (three-row records) are not supported");
  if (pose && user.n_sam > 0)
    throw std::invalid_argument("smart factors: pose-type smart factors together with bearing / range factors (three-row records) are not supported");
  var_type.assign(user.var_type, user.var_type + user.n_vars); var_type.resize((size_t)user.n_vars + n_smart, GTG_VAR_POINT3);
  // the device addresses a factor's measurements as smart_obs0 + smart_ptr[i] while the expanded observations are appended one
  // after the other: the offsets must start at 0 and be strictly increasing
  if (user.smart_ptr[0] != 0) throw std::invalid_argument("smart factors: smart_ptr[0] must be 0");
  for (int64_t i = 0; i < n_smart; i++) {
    const int64_t k0 = user.smart_ptr[i], k1 = user.smart_ptr[i + 1];
    if (k1 <= k0 || k1 > n_meas) throw std::invalid_argument("smart factor without measurements / bad smart_ptr");
    const double* sp = user.smart_params + 8 * i;
    if (!(sp[4] == 0.0 || sp[4] == 1.0 || sp[4] == 2.0)) throw std::invalid_argument("smart factor: unknown degeneracy mode");
    if (!(sp[6] == 0.0 || sp[6] == 1.0)) throw std::invalid_argument("smart factor: enableEPI must be 0 or 1");
    // LinearizationMode (SmartFactorParams.h:31-33): HESSIAN, JACOBIAN_Q, JACOBIAN_SVD give the same normal equations (they differ in
    // what a failed track contributes and in the constant of the linear error); IMPLICIT_SCHUR factors cannot be eliminated by
    // the reference's direct solvers at all (RegularImplicitSchurFactor has no augmentedJacobian / augmentedInformation)
    if (!(sp[5] == 0.0 || sp[5] == 2.0 || sp[5] == 3.0)) throw std::invalid_argument("smart factor: linearization mode must be 0 HESSIAN, 2 JACOBIAN_Q or 3 JACOBIAN_SVD");
    // rankTolerance, landmarkDistanceThreshold, dynamicOutlierRejectionThreshold (negative = off, as in the reference),
    // retriangulationThreshold: numbers, not NaN / inf (a NaN threshold silently disables the test it guards)
    for (int e = 0; e < 4; e++) if (!std::isfinite(sp[e])) throw std::invalid_argument("smart factor: a threshold is not finite");
    // useLOST: 0 = DLT, > 0 = LOST with that measurement sigma (triangulation.h:503)
    if (!(std::isfinite(sp[7]) && sp[7] >= 0.0)) throw std::invalid_argument("smart factor: the useLOST sigma (smart_params[8 i + 7]) must be 0 (DLT) or a positive finite number");
    // the reference requires an isotropic model (SmartFactorBase.h:107-114: "SmartFactorBase: needs isotropic")
    const int32_t nz = user.smart_noise[i];
    if (nz < 0 || nz >= user.n_noise || user.noise_dim[nz] != 2 ||
        !(user.noise_kind[nz] == GTG_NOISE_UNIT || user.noise_kind[nz] == GTG_NOISE_ISOTROPIC))
      throw std::invalid_argument("smart factor: smart_noise must index a dim-2 Unit or Isotropic noise model");
  }
  if (pose) expand_poses(user, n_smart); else expand_cameras(user, n_smart);
  q.n_vars = (int32_t)var_type.size(); q.var_type = var_type.data();
  p = &q;
}

void SmartView::expand_cameras(const gtg_problem& user, int64_t n_smart) {
  sfm_cam.assign(user.sfm_cam, user.sfm_cam + user.n_sfm); sfm_point.assign(user.sfm_point, user.sfm_point + user.n_sfm);
  sfm_noise.assign(user.sfm_noise, user.sfm_noise + user.n_sfm); sfm_z.assign(user.sfm_z, user.sfm_z + 2 * user.n_sfm);
  of_obs.assign((size_t)user.n_sfm, -1);
  for (int64_t i = 0; i < n_smart; i++)
    for (int64_t k = user.smart_ptr[i]; k < user.smart_ptr[i + 1]; k++) {
      const int cam = user.smart_cam[k];
      if (cam < 0 || cam >= user.n_vars || user.var_type[cam] != GTG_VAR_SFM_CAMERA)
        throw std::invalid_argument("smart factor: its keys must be SFM_CAMERA variables");
      sfm_cam.push_back(cam); sfm_point.push_back((int32_t)(user.n_vars + i)); sfm_noise.push_back(user.smart_noise[i]);
      sfm_z.push_back(user.smart_z[2 * k]); sfm_z.push_back(user.smart_z[2 * k + 1]);
      of_obs.push_back((int32_t)i);
    }
  q.n_sfm = (int64_t)sfm_cam.size(); q.sfm_cam = sfm_cam.data(); q.sfm_point = sfm_point.data();
  q.sfm_noise = sfm_noise.data(); q.sfm_z = sfm_z.data();
}

// rig-type factor i: as a pose-type factor, with the calib / sensor entry of every measurement; what the reference's constructor and
// this library's scope rule out is refused, each with its own message
void SmartView::expand_rig(const gtg_problem& user, int64_t i) {
  const double* sp = user.smart_params + 8 * i;
  if (sp[4] != 1.0) throw std::invalid_argument("smart factor: a rig-type smart factor needs degeneracyMode 1 (SmartProjectionRigFactor: degeneracyMode must be set to ZERO_ON_DEGENERACY)");
  if (sp[5] != 0.0) throw std::invalid_argument("smart factor: a rig-type smart factor needs linearizationMode 0 (SmartProjectionRigFactor: linearizationMode must be set to HESSIAN)");
  if (sp[6] != 0.0) throw std::invalid_argument("smart factor: enableEPI is not supported on a rig-type smart factor (the refinement is written for Cal3Bundler cameras)");
  if (user.smart_sensor && user.smart_sensor[i] != -1)
    throw std::invalid_argument("smart factor: smart_sensor must be -1 on a rig-type smart factor (its extrinsics are per measurement: smart_meas_sensor)");
  if (!user.smart_meas_calib || !user.smart_meas_sensor)
    throw std::invalid_argument("smart factor: a GTG_SMART_RIG factor needs the per-measurement tables smart_meas_calib and smart_meas_sensor");
  std::vector<int32_t> keys;
  for (int64_t k = user.smart_ptr[i]; k < user.smart_ptr[i + 1]; k++) {
    const int v = user.smart_cam[k];
    const int32_t ci = user.smart_meas_calib[k], si = user.smart_meas_sensor[k];
    if (ci < 0 || ci >= user.n_calib || !user.calib) throw std::invalid_argument("smart factor: smart_meas_calib index out of range");
    if (si < -1 || si >= user.n_sensor || (si >= 0 && !user.sensor)) throw std::invalid_argument("smart factor: smart_meas_sensor index out of range");
    if (user.calib_distortion)
      for (int j = 0; j < 4; j++)
        if (user.calib_distortion[4 * (size_t)ci + j] != 0.0)
          throw std::invalid_argument("smart factor: a calibration with Cal3DS2 distortion is not supported by a rig-type smart factor (SmartProjectionRigFactor<PinholePose<Cal3_S2>> only)");
    if (v < 0 || v >= user.n_vars || user.var_type[v] != GTG_VAR_POSE3)
      throw std::invalid_argument("smart factor: the keys of a rig-type smart factor must be POSE3 variables");
    proj_pose.push_back(v); proj_point.push_back((int32_t)(user.n_vars + i)); proj_noise.push_back(user.smart_noise[i]);
    proj_calib.push_back(ci); proj_sensor.push_back(si);
    proj_z.push_back(user.smart_z[2 * k]); proj_z.push_back(user.smart_z[2 * k + 1]);
    of_obs.push_back((int32_t)i);
    keys.push_back(v);
  }
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) repeats = true;
}

// pose-type: one projection observation per measurement behind the caller's own GTG_FAC_PROJECTION observations, the way the stereo
// factors joined that range
void SmartView::expand_poses(const gtg_problem& user, int64_t n_smart) {
  if (user.n_proj > 0 && (!user.proj_pose || !user.proj_point || !user.proj_z || !user.proj_noise || !user.proj_calib))
    throw std::invalid_argument("projection factor tables missing");
  proj_pose.assign(user.proj_pose, user.proj_pose + user.n_proj); proj_point.assign(user.proj_point, user.proj_point + user.n_proj);
  proj_noise.assign(user.proj_noise, user.proj_noise + user.n_proj); proj_calib.assign(user.proj_calib, user.proj_calib + user.n_proj);
  if (user.proj_sensor) proj_sensor.assign(user.proj_sensor, user.proj_sensor + user.n_proj); else proj_sensor.assign((size_t)user.n_proj, -1);
  proj_z.assign(user.proj_z, user.proj_z + 2 * user.n_proj);
  of_obs.assign((size_t)user.n_proj, -1);
  is_rig.assign((size_t)n_smart, 0);
  for (int64_t i = 0; i < n_smart; i++) {
    const int32_t ci = user.smart_calib[i], si = user.smart_sensor ? user.smart_sensor[i] : -1;
    if (ci == GTG_SMART_RIG) { is_rig[(size_t)i] = 1; expand_rig(user, i); continue; }
    if (ci < 0 || ci >= user.n_calib || !user.calib) throw std::invalid_argument("smart factor: smart_calib index out of range");
    if (si < -1 || si >= user.n_sensor || (si >= 0 && !user.sensor)) throw std::invalid_argument("smart factor: smart_sensor index out of range");
    if (user.calib_distortion)
      for (int j = 0; j < 4; j++)
        if (user.calib_distortion[4 * (size_t)ci + j] != 0.0)
          throw std::invalid_argument("smart factor: a calibration with Cal3DS2 distortion is not supported by a pose-type smart factor (SmartProjectionPoseFactor<Cal3_S2> only)");
    if (user.smart_params[8 * i + 6] != 0.0)
      throw std::invalid_argument("smart factor: enableEPI is not supported on a pose-type smart factor (the refinement is written for Cal3Bundler cameras)");
    for (int64_t k = user.smart_ptr[i]; k < user.smart_ptr[i + 1]; k++) {
      const int v = user.smart_cam[k];
      if (v < 0 || v >= user.n_vars || user.var_type[v] != GTG_VAR_POSE3)
        throw std::invalid_argument("smart factor: the keys of a pose-type smart factor must be POSE3 variables");
      proj_pose.push_back(v); proj_point.push_back((int32_t)(user.n_vars + i)); proj_noise.push_back(user.smart_noise[i]);
      proj_calib.push_back(ci); proj_sensor.push_back(si);
      proj_z.push_back(user.smart_z[2 * k]); proj_z.push_back(user.smart_z[2 * k + 1]);
      of_obs.push_back((int32_t)i);
    }
  }
  q.n_proj = (int64_t)proj_pose.size(); q.proj_pose = proj_pose.data(); q.proj_point = proj_point.data(); q.proj_noise = proj_noise.data();
  q.proj_calib = proj_calib.data(); q.proj_sensor = proj_sensor.data(); q.proj_z = proj_z.data();
}

// per smart factor: parameters, an empty triangulation cache, cleared status words (smart_ptr and obs_smart follow the shard
// filter of the observation table: upload_smart_tracks); a handle without smart factors gives the buffers of an earlier problem back
void upload_smart_state(gtg_context& c, const gtg_problem& user) {
  const int64_t n_smart = c.n_smart;
  if (!n_smart) {
    c.smart_ptr.free(); c.smart_params.free(); c.obs_smart.free(); c.lm_smart.free(); c.smart_status.free(); c.smart_lin_status.free();
    c.smart_cache_state.free(); c.smart_cache_pose.free(); c.smart_cache_point.free();
    c.smart_lost = false; c.smart_lost_rows.free(); c.smart_last_status = nullptr;
    return;
  }
  const int64_t n_meas = user.smart_ptr[n_smart];
  std::vector<double> prm(user.smart_params, user.smart_params + 8 * n_smart);
  c.smart_lost = false; c.smart_last_status = nullptr;
  for (int64_t i = 0; i < n_smart; i++) c.smart_lost = c.smart_lost || prm[8 * (size_t)i + 7] > 0.0;
  up(c.smart_params, prm, c.stream);
  std::vector<int32_t> none((size_t)n_smart, -1);
  up(c.smart_cache_state, none, c.stream);
  c.smart_status.alloc((size_t)n_smart); c.smart_lin_status.alloc((size_t)n_smart); c.smart_cache_point.alloc(3 * (size_t)n_smart); c.smart_cache_pose.alloc(12 * (size_t)n_meas);
  check_hip(hipMemsetAsync(c.smart_status.p, 0, sizeof(int32_t) * n_smart, c.stream), "memset");
  check_hip(hipMemsetAsync(c.smart_lin_status.p, 0, sizeof(int32_t) * n_smart, c.stream), "memset");
}

// where every variable starts in the packed values / tangent vectors; values, trial point and step
void layout_variables(gtg_context& c, const gtg_problem& p) {
  c.n_vars = p.n_vars;
  c.h_var_type.assign(p.var_type, p.var_type + p.n_vars);
  c.h_val_off.assign(p.n_vars + 1, 0); c.h_dim_off.assign(p.n_vars + 1, 0);
  for (int v = 0; v < p.n_vars; v++) {
    const int t = p.var_type[v];
    if (t < 0 || t > GTG_VAR_POINT2) throw std::invalid_argument("unknown variable type");
    c.h_val_off[v + 1] = c.h_val_off[v] + storage_size(t);
    c.h_dim_off[v + 1] = c.h_dim_off[v] + tangent_dim(t);
  }
  c.val_size = c.h_val_off[p.n_vars]; c.dim_size = c.h_dim_off[p.n_vars];
  c.user_val_size = c.h_val_off[c.n_user_vars]; c.user_dim_size = c.h_dim_off[c.n_user_vars];
  // on the device a POINT2 is the POINT3 whose slot it is padded to (x, y, 0 / dx, dy, 0): retraction and everything else that reads
  // var_type there stay as they are; the host keeps the caller's types
  std::vector<int32_t> dev_type(c.h_var_type);
  for (int32_t& t : dev_type) if (t == GTG_VAR_POINT2) t = GTG_VAR_POINT3;
  up(c.var_type, dev_type, c.stream); up(c.val_off, c.h_val_off, c.stream); up(c.dim_off, c.h_dim_off, c.stream);
  c.values.alloc(std::max<int64_t>(c.val_size, 1)); c.trial.alloc(std::max<int64_t>(c.val_size, 1));
  c.delta.alloc(std::max<int64_t>(c.dim_size, 1));
  check_hip(hipMemsetAsync(c.delta.p, 0, sizeof(double) * c.delta.n, c.stream), "memset");
}

// A planar graph (a POINT2 variable or a planar bearing / range factor) is a graph of POSE2 and POINT2 variables with no other
// observation: its projection range is ProjForm::Planar (context.h).  Sharding is a follow-up.
bool check_planar(const gtg_problem& p, int n_shards) {
  bool planar = p.planar.n_sam2 > 0;
  for (int v = 0; v < p.n_vars && !planar; v++) planar = p.var_type[v] == GTG_VAR_POINT2;
  if (!planar) return false;
  bool other = p.n_sfm > 0 || p.n_proj > 0 || p.n_stereo > 0 || p.n_sam > 0 || p.n_smart > 0;
  for (int v = 0; v < p.n_vars && !other; v++) other = p.var_type[v] == GTG_VAR_POSE3 || p.var_type[v] == GTG_VAR_SFM_CAMERA || p.var_type[v] == GTG_VAR_POINT3;
  if (other)
    throw std::invalid_argument("planar graph: POINT2 variables and planar bearing / range factors cannot share a graph with POSE3, SFM_CAMERA or POINT3 "
                                "variables or with camera, stereo, 3-D bearing / range or smart factors");
  if (n_shards > 1) throw std::invalid_argument("planar graph: n_shards > 1 is not supported");
  return true;
}

// The list gtg_set_calibration_models left in the host index (upload_problem has taken it out), checked against the problem it is consumed by.  Returns the model of
// every calib row when some row is a Cal3Fisheye, and an empty list otherwise: a list of pinhole rows is no list.  A fisheye row is
// allowed only where the projection range would be ProjForm::Rows2 without it (context.h).
std::vector<int32_t> check_calibration_models(std::vector<int32_t> model, const gtg_problem& p, bool planar) {
  if (model.empty()) return model;
  if ((int64_t)model.size() != (int64_t)(p.n_calib > 0 ? p.n_calib : 0))
    throw std::invalid_argument("gtg_set_calibration_models: n_calib differs from the n_calib of the uploaded problem");
  bool fisheye = false;
  for (int32_t m : model) {
    if (m != GTG_CALIB_PINHOLE && m != GTG_CALIB_FISHEYE)
      throw std::invalid_argument("gtg_set_calibration_models: unknown calibration model (GTG_CALIB_PINHOLE or GTG_CALIB_FISHEYE)");
    fisheye = fisheye || m == GTG_CALIB_FISHEYE;
  }
  if (!fisheye) return {};
  if (planar) throw std::invalid_argument("Cal3Fisheye: a fisheye calibration row in a planar graph is not supported");
  if (!p.calib_distortion)
    throw std::invalid_argument("Cal3Fisheye: a fisheye calibration row needs calib_distortion (k1, k2, k3, k4), which is NULL");
  const auto is_fisheye = [&](int32_t ci) { return ci >= 0 && ci < p.n_calib && model[(size_t)ci] == GTG_CALIB_FISHEYE; };
  const int64_t n_stereo = p.n_stereo > 0 && p.stereo_calib ? p.n_stereo : 0, n_smart = p.n_smart > 0 ? p.n_smart : 0;
  for (int64_t i = 0; i < n_stereo; i++)
    if (is_fisheye(p.stereo_calib[i]))
      throw std::invalid_argument("Cal3Fisheye: a GenericStereoFactor names a fisheye calibration row (Cal3_S2Stereo only)");
  if (n_smart && p.smart_calib)
    for (int64_t i = 0; i < n_smart; i++)
      if (is_fisheye(p.smart_calib[i]))
        throw std::invalid_argument("Cal3Fisheye: a smart factor names a fisheye calibration row through smart_calib (Cal3_S2 only)");
  if (n_smart && p.smart_meas_calib && p.smart_ptr)
    for (int64_t k = 0; k < p.smart_ptr[n_smart]; k++)
      if (is_fisheye(p.smart_meas_calib[k]))
        throw std::invalid_argument("Cal3Fisheye: a smart factor names a fisheye calibration row through smart_meas_calib (Cal3_S2 only)");
  if (p.n_stereo > 0 || p.n_sam > 0 || n_smart)
    throw std::invalid_argument("Cal3Fisheye: a fisheye calibration row in a graph with stereo, 3-D bearing / range or smart factors is not supported "
                                "(two-row projection graphs only)");
  return model;
}

// noise table: derive the inverse sigmas like the reference constructors (NoiseModel.cpp:275-281, Isotropic ctor)
void upload_noise_table(gtg_context& c, const gtg_problem& p) {
  std::vector<int32_t> kind(p.noise_kind, p.noise_kind + p.n_noise);
  std::vector<int64_t> noff(p.n_noise);
  std::vector<double> data;
  for (int i = 0; i < p.n_noise; i++) {
    const int dim = p.noise_dim[i];
    const double* d = p.noise_data + p.noise_off[i];
    noff[i] = (int64_t)data.size();
    switch (kind[i]) {
      case GTG_NOISE_UNIT: data.push_back(0.0); break;
      case GTG_NOISE_ISOTROPIC: data.push_back(1.0 / d[0]); break;
      case GTG_NOISE_DIAGONAL: for (int k = 0; k < dim; k++) data.push_back(1.0 / d[k]); break;
      case GTG_NOISE_GAUSSIAN: for (int k = 0; k < dim * dim; k++) data.push_back(d[k]); break;
      default: throw std::invalid_argument("unsupported noise model kind (Robust/Constrained are out of scope)");
    }
  }
  std::vector<int32_t> rkind(p.n_noise, GTG_ROBUST_NONE);
  std::vector<double> rk(p.n_noise, 0.0);
  for (int i = 0; i < p.n_noise; i++) {
    if (p.noise_robust) rkind[i] = p.noise_robust[i];
    if (rkind[i] < GTG_ROBUST_NONE || rkind[i] > GTG_ROBUST_L2WITHDEADZONE) throw std::invalid_argument("unsupported m-estimator");
    if (rkind[i] != GTG_ROBUST_NONE) {
      rk[i] = p.noise_robust_param ? p.noise_robust_param[i] : 0.0;
      if (!(rk[i] > 0.0)) throw std::invalid_argument("m-estimator parameter must be > 0");   // LossFunctions.cpp ctor checks
    }
  }
  up(c.noise_kind, kind, c.stream); up(c.noise_off, noff, c.stream); up(c.noise_data, data, c.stream);
  up(c.noise_rkind, rkind, c.stream); up(c.noise_rk, rk, c.stream);
}

// what every factor family checks of its rows
void check_var(const gtg_problem& p, int v) { if (v < 0 || v >= p.n_vars) throw std::invalid_argument("factor refers to a key that is not in Values"); }
void check_noise(const gtg_problem& p, int idx, int dim, const char* what) {
  if (idx < 0 || idx >= p.n_noise || p.noise_dim[idx] != dim)
    throw std::invalid_argument(std::string(what) + ": NoiseModel has wrong dimension");  // NonlinearFactor.cpp:97-104
}

// shard filter: landmark factors follow their landmark (rank among POINT3 variables), others round-robin; a prior follows its
// variable if that is a landmark.  (One shard owns everything: the family stages ask only when n_shards > 1.)
struct ShardFilter {
  std::vector<int32_t> lm_rank;
  int shard, n_shards;
  ShardFilter(const gtg_problem& p, int shard_, int n_shards_) : lm_rank(p.n_vars, -1), shard(shard_), n_shards(n_shards_) {
    int k = 0; for (int v = 0; v < p.n_vars; v++) if (p.var_type[v] == GTG_VAR_POINT3) lm_rank[v] = k++;
  }
  bool owns_landmark(int v) const { return lm_rank[v] >= 0 && (lm_rank[v] % n_shards) == shard; }
  bool owns_round_robin(int64_t i) const { return (i % n_shards) == shard; }
  bool owns_prior(int v, int64_t i) const { return lm_rank[v] >= 0 ? owns_landmark(v) : owns_round_robin(i); }
};

// sharded layouts are derived from the keys of the WHOLE graph (HostIndex, analysis.h)
void keep_whole_graph_keys(HostIndex& hi, const gtg_problem& p, int n_shards) {
  hi.all_obs_red_var.clear(); hi.all_obs_point.clear(); hi.all_between_v1.clear(); hi.all_between_v2.clear();
  if (n_shards == 1) return;
  for (int64_t i = 0; i < p.n_sfm; i++) { check_var(p, p.sfm_cam[i]); check_var(p, p.sfm_point[i]); }
  for (int64_t i = 0; i < p.n_proj; i++) { check_var(p, p.proj_pose[i]); check_var(p, p.proj_point[i]); }
  const int64_t n_stereo = p.n_stereo > 0 && p.stereo_pose && p.stereo_point ? p.n_stereo : 0;   // (the tables are checked by upload_projection)
  for (int64_t i = 0; i < n_stereo; i++) { check_var(p, p.stereo_pose[i]); check_var(p, p.stereo_point[i]); }
  const int64_t n_sam = p.n_sam > 0 && p.sam_pose && p.sam_point ? p.n_sam : 0;
  for (int64_t i = 0; i < n_sam; i++) { check_var(p, p.sam_pose[i]); check_var(p, p.sam_point[i]); }
  for (int64_t i = 0; i < p.n_between; i++) { check_var(p, p.between_v1[i]); check_var(p, p.between_v2[i]); }
  hi.all_obs_red_var.assign(p.sfm_cam, p.sfm_cam + p.n_sfm); hi.all_obs_red_var.insert(hi.all_obs_red_var.end(), p.proj_pose, p.proj_pose + p.n_proj);
  hi.all_obs_red_var.insert(hi.all_obs_red_var.end(), p.stereo_pose, p.stereo_pose + n_stereo);
  hi.all_obs_red_var.insert(hi.all_obs_red_var.end(), p.sam_pose, p.sam_pose + n_sam);
  hi.all_obs_point.assign(p.sfm_point, p.sfm_point + p.n_sfm); hi.all_obs_point.insert(hi.all_obs_point.end(), p.proj_point, p.proj_point + p.n_proj);
  hi.all_obs_point.insert(hi.all_obs_point.end(), p.stereo_point, p.stereo_point + n_stereo);
  hi.all_obs_point.insert(hi.all_obs_point.end(), p.sam_point, p.sam_point + n_sam);
  hi.all_between_v1.assign(p.between_v1, p.between_v1 + p.n_between); hi.all_between_v2.assign(p.between_v2, p.between_v2 + p.n_between);
}

// The noise rows and the measurements of a whole GeneralSFM table (20 bytes per factor: 13.5 MB on the L1723 shape, 1.2 ms from pageable
// memory) are not read by the symbolic analysis: they go up from the caller's arrays on a helper thread and the handle's copy stream
// beside it.  finish() waits for them and rethrows what the thread met; the destructor only waits.
class SideUpload {
  std::thread t;
  std::exception_ptr err;
 public:
  ~SideUpload() { if (t.joinable()) t.join(); }
  void start(gtg_context& c, const int32_t* h_nz, const double* h_z, size_t n) {
    c.f.sfm_noise.alloc(n); c.f.sfm_z.alloc(2 * n);
    const int dev = c.device; hipStream_t cs = c.copy_stream;
    int32_t* d_nz = c.f.sfm_noise.p; double* d_z = c.f.sfm_z.p;
    t = std::thread([this, dev, cs, d_nz, d_z, h_nz, h_z, n] {
      try {
        check_hip(hipSetDevice(dev), "hipSetDevice");
        check_hip(hipMemcpyAsync(d_nz, h_nz, sizeof(int32_t) * n, hipMemcpyHostToDevice, cs), "H2D");
        check_hip(hipMemcpyAsync(d_z, h_z, sizeof(double) * 2 * n, hipMemcpyHostToDevice, cs), "H2D");
        check_hip(hipStreamSynchronize(cs), "sync");
      } catch (...) { err = std::current_exception(); }
    });
  }
  void finish() { if (t.joinable()) t.join(); if (err) std::rethrow_exception(err); }
};

// Sharded, a smart factor follows its hidden landmark like any landmark factor: this shard holds the measurements of the
// tracks it owns, in the order of the whole table.  The per-factor arrays keep the GLOBAL factor index (parameters, status,
// cache); a factor of another shard has no measurements here (smart_ptr[i + 1] == smart_ptr[i]) and is skipped.
// (n, point): the observation range the measurements joined -- GeneralSFM, or projection for pose-type factors.
std::vector<int32_t> upload_smart_tracks(gtg_context& c, int64_t n, const int32_t* point, const std::vector<int32_t>& of_obs, const ShardFilter& own) {
  std::vector<int64_t> rel((size_t)c.n_smart + 1, 0);
  std::vector<int32_t> of_local;
  int64_t obs0 = 0;
  for (int64_t i = 0; i < n; i++) {
    if (own.n_shards > 1 && !own.owns_landmark(point[i])) continue;
    const int32_t sf = of_obs[(size_t)i];
    of_local.push_back(sf);
    if (sf < 0) obs0++; else rel[(size_t)sf + 1]++;
  }
  for (int64_t i = 0; i < c.n_smart; i++) rel[(size_t)i + 1] += rel[(size_t)i];
  c.smart_obs0 = obs0;
  if (c.smart_lost) c.smart_lost_rows.alloc(8 * (size_t)std::max<int64_t>(rel.back(), 1)); else c.smart_lost_rows.free();   // (geom.h::triangulate_lost)
  up(c.smart_ptr, rel, c.stream);
  up(c.obs_smart, of_local, c.stream);
  return of_local;
}

// The sightings of every (pose, rig-type track) group with more than one member among this shard's observations (a track lives on one
// shard with all its measurements): sorted by (pose variable, track, observation), so that every sum over a group runs in range order.
// pose / of_local: this shard's part of the projection range.
void upload_smart_repeats(gtg_context& c, const std::vector<int32_t>& pose, const std::vector<int32_t>& of_local, const std::vector<uint8_t>& is_rig) {
  c.n_rep_vars = 0;
  c.rep_var.free(); c.rep_grp_ptr.free(); c.rep_obs_ptr.free(); c.rep_smart.free(); c.rep_obs.free();
  if (!c.smart_repeats) return;
  struct Sighting { int32_t var, track, obs; };
  std::vector<Sighting> s;
  for (size_t o = 0; o < of_local.size(); o++)
    if (of_local[o] >= 0 && is_rig[(size_t)of_local[o]]) s.push_back({pose[o], of_local[o], (int32_t)o});
  std::sort(s.begin(), s.end(), [](const Sighting& a, const Sighting& b) {
    return a.var != b.var ? a.var < b.var : a.track != b.track ? a.track < b.track : a.obs < b.obs; });
  std::vector<int32_t> var, grp_ptr{0}, obs_ptr{0}, track, obs;
  for (size_t a = 0; a < s.size();) {
    size_t b = a + 1;
    while (b < s.size() && s[b].var == s[a].var && s[b].track == s[a].track) b++;
    if (b - a > 1) {
      if (var.empty() || var.back() != s[a].var) { if (!var.empty()) grp_ptr.push_back((int32_t)track.size()); var.push_back(s[a].var); }
      track.push_back(s[a].track);
      for (size_t k = a; k < b; k++) obs.push_back(s[k].obs);
      obs_ptr.push_back((int32_t)obs.size());
    }
    a = b;
  }
  if (var.empty()) return;     // (the groups of the graph are on other shards)
  grp_ptr.push_back((int32_t)track.size());
  c.n_rep_vars = (int32_t)var.size();
  up(c.rep_var, var, c.stream); up(c.rep_grp_ptr, grp_ptr, c.stream); up(c.rep_obs_ptr, obs_ptr, c.stream);
  up(c.rep_smart, track, c.stream); up(c.rep_obs, obs, c.stream);
}

void upload_sfm(gtg_context& c, HostIndex& hi, const gtg_problem& p, const std::vector<int32_t>& of_obs, const ShardFilter& own, SideUpload& side) {
  auto& f = c.f;
  for (int64_t i = 0; i < p.n_sfm; i++) { check_var(p, p.sfm_cam[i]); check_var(p, p.sfm_point[i]); check_noise(p, p.sfm_noise[i], 2, "GeneralSFMFactor"); }
  std::vector<int32_t> cam, pt, nz; std::vector<double> z;
  const bool whole = own.n_shards == 1 && p.n_sfm > 0;
  if (whole) {   // the whole table: the keys are copied (kept by the host index: gtg_set_reduced_ordering analyses again), the rest goes up beside the analysis
    cam.assign(p.sfm_cam, p.sfm_cam + p.n_sfm); pt.assign(p.sfm_point, p.sfm_point + p.n_sfm);
  } else {       // this shard's rows (or none at all)
    for (int64_t i = 0; i < p.n_sfm; i++) {
      if (!own.owns_landmark(p.sfm_point[i])) continue;
      cam.push_back(p.sfm_cam[i]); pt.push_back(p.sfm_point[i]); nz.push_back(p.sfm_noise[i]);
      z.push_back(p.sfm_z[2 * i]); z.push_back(p.sfm_z[2 * i + 1]);
    }
  }
  if (c.n_smart && !c.smart_pose) upload_smart_tracks(c, p.n_sfm, p.sfm_point, of_obs, own);
  f.n_sfm = (int64_t)cam.size();
  up(f.sfm_cam, cam, c.stream); up(f.sfm_point, pt, c.stream);
  if (whole) side.start(c, p.sfm_noise, p.sfm_z, (size_t)p.n_sfm);
  else { up(f.sfm_noise, nz, c.stream); up(f.sfm_z, z, c.stream); }
  if (c.val_size >= (int64_t)1 << 31) throw std::invalid_argument("gtg_upload_problem: more than 2^31 packed value entries");
  f.sfm_cam_at.alloc(std::max<size_t>(cam.size(), 1)); f.sfm_point_at.alloc(std::max<size_t>(pt.size(), 1));
  launch_sfm_value_offsets(c);     // where each factor's camera / point start in the packed values (a gather through val_off, on the device)
  f.sfm_J.alloc(c.fused_sfm ? 1 : std::max<size_t>((size_t)kSfmRec * f.n_sfm, 1));
  hi.sfm_cam = std::move(cam); hi.sfm_point = std::move(pt);
}

// The projection range of a planar graph: its bearing / range factors <Pose2, Point2> alone, the POSE2 as the "camera".  The factors
// read no calib or sensor entry; their kinds and measurements (c, s of a Rot2 and a range) go into the buffers of the 3-D sam factors.
void upload_planar(gtg_context& c, HostIndex& hi, const gtg_problem& p) {
  auto& f = c.f;
  f.form = ProjForm::Planar;
  const int64_t n = p.planar.n_sam2 > 0 ? p.planar.n_sam2 : 0;
  if (n && (!p.planar.sam2_kind || !p.planar.sam2_pose || !p.planar.sam2_point || !p.planar.sam2_z || !p.planar.sam2_noise)) throw std::invalid_argument("planar bearing / range factor tables missing");
  std::vector<int32_t> pose, pt, nz, none, kind; std::vector<double> z;
  for (int64_t i = 0; i < n; i++) {
    const int k = p.planar.sam2_kind[i];
    if (k != GTG_SAM_BEARING_RANGE && k != GTG_SAM_RANGE && k != GTG_SAM_BEARING)
      throw std::invalid_argument("planar bearing / range factor: unknown sam2_kind (GTG_SAM_BEARING_RANGE, GTG_SAM_RANGE or GTG_SAM_BEARING)");
    const char* what = k == GTG_SAM_BEARING_RANGE ? "BearingRangeFactor2D" : k == GTG_SAM_RANGE ? "RangeFactor2D" : "BearingFactor2D";
    check_var(p, p.planar.sam2_pose[i]); check_var(p, p.planar.sam2_point[i]);
    if (p.var_type[p.planar.sam2_pose[i]] != GTG_VAR_POSE2 || p.var_type[p.planar.sam2_point[i]] != GTG_VAR_POINT2)
      throw std::invalid_argument(std::string(what) + " keys must be (POSE2, POINT2)");
    check_noise(p, p.planar.sam2_noise[i], sam2_rows(k), what);
    pose.push_back(p.planar.sam2_pose[i]); pt.push_back(p.planar.sam2_point[i]); nz.push_back(p.planar.sam2_noise[i]); none.push_back(-1);
    kind.push_back(k);
    for (int e = 0; e < 3; e++) z.push_back(p.planar.sam2_z[3 * i + e]);
  }
  f.n_mono = 0; f.n_cam = 0; f.n_proj = n;
  c.n_rep_vars = 0; c.rep_var.free(); c.rep_grp_ptr.free(); c.rep_obs_ptr.free(); c.rep_smart.free(); c.rep_obs.free();
  up(f.sam_kind, kind, c.stream); up(f.sam_z, z, c.stream);
  up(f.proj_pose, pose, c.stream); up(f.proj_point, pt, c.stream); up(f.proj_noise, nz, c.stream); up(f.proj_calib, none, c.stream);
  up(f.proj_sensor, none, c.stream);
  const std::vector<double> empty;
  up(f.proj_z, empty, c.stream); up(f.calib, empty, c.stream); up(f.sensor, empty, c.stream); f.calib_baseline.free(); f.calib_model.free();
  f.proj_J.alloc(std::max<size_t>((size_t)kPlanarRec * f.n_proj, 1));
  hi.proj_pose = pose; hi.proj_point = pt;
}

void upload_projection(gtg_context& c, HostIndex& hi, const gtg_problem& p, const std::vector<int32_t>& of_obs, const std::vector<uint8_t>& is_rig, const ShardFilter& own, bool planar,
                       const std::vector<int32_t>& calib_model) {
  auto& f = c.f;
  std::vector<int32_t> pose, pt, nz, cal, sen; std::vector<double> z;
  const int64_t n_stereo = p.n_stereo > 0 ? p.n_stereo : 0, n_sam = p.n_sam > 0 ? p.n_sam : 0;
  if (planar) { upload_planar(c, hi, p); return; }
  f.form = n_sam > 0 ? ProjForm::Rows3Sam : n_stereo > 0 ? ProjForm::Rows3 : c.smart_pose ? ProjForm::Rows2Smart : ProjForm::Rows2;   // from the WHOLE graph (context.h; SmartView has refused smart_pose beside the other two)
  static_assert(proj_rec(ProjForm::Rows2) == kProjRec && proj_rec(ProjForm::Rows3) == kStereoRec, "context.h states the record lengths of factors.h");
  if (!calib_model.empty()) {   // some calib row is a Cal3Fisheye (take_calibration_models has refused it beside everything but Rows2)
    if (f.form != ProjForm::Rows2) throw std::logic_error("Cal3Fisheye: the projection range is not two-row");
    f.form = ProjForm::Rows2Fisheye;
    static_assert(proj_rec(ProjForm::Rows2Fisheye) == kProjRec, "the fisheye form keeps the records of Rows2");
  }
  for (int64_t i = 0; i < p.n_proj; i++) {
    check_var(p, p.proj_pose[i]); check_var(p, p.proj_point[i]); check_noise(p, p.proj_noise[i], 2, "GenericProjectionFactor");
    if (p.proj_calib[i] < 0 || p.proj_calib[i] >= p.n_calib) throw std::invalid_argument("bad calibration index");
    const int si = p.proj_sensor ? p.proj_sensor[i] : -1;
    if (si >= p.n_sensor) throw std::invalid_argument("bad body_P_sensor index");
    if (own.n_shards > 1 && !own.owns_landmark(p.proj_point[i])) continue;
    pose.push_back(p.proj_pose[i]); pt.push_back(p.proj_point[i]); nz.push_back(p.proj_noise[i]);
    cal.push_back(p.proj_calib[i]); sen.push_back(si);
    z.push_back(p.proj_z[2 * i]); z.push_back(p.proj_z[2 * i + 1]);
    if (proj_rows(f.form) == 3) z.push_back(0.0);   // a three-row graph keeps three measurement entries per camera observation
  }
  f.n_mono = (int64_t)pose.size();
  if (c.smart_pose) upload_smart_repeats(c, pose, upload_smart_tracks(c, p.n_proj, p.proj_point, of_obs, own), is_rig);   // (their measurements are part of the range above)
  else upload_smart_repeats(c, pose, {}, is_rig);
  // the stereo factors join the observation range behind the monocular ones: the symbolic analysis, the incidence lists, the E slots,
  // the Schur terms, PCG and the shard filter see more projection observations and nothing else
  if (n_stereo) {
    if (!p.stereo_pose || !p.stereo_point || !p.stereo_z || !p.stereo_noise || !p.stereo_calib) throw std::invalid_argument("stereo factor tables missing");
    if (!p.calib_baseline) throw std::invalid_argument("GenericStereoFactor: calib_baseline is missing");
  }
  for (int64_t i = 0; i < n_stereo; i++) {
    check_var(p, p.stereo_pose[i]); check_var(p, p.stereo_point[i]); check_noise(p, p.stereo_noise[i], 3, "GenericStereoFactor");
    if (p.var_type[p.stereo_pose[i]] != GTG_VAR_POSE3 || p.var_type[p.stereo_point[i]] != GTG_VAR_POINT3)
      throw std::invalid_argument("GenericStereoFactor keys must be (POSE3, POINT3)");
    if (p.stereo_calib[i] < 0 || p.stereo_calib[i] >= p.n_calib) throw std::invalid_argument("bad calibration index");
    const int si = p.stereo_sensor ? p.stereo_sensor[i] : -1;
    if (si >= p.n_sensor) throw std::invalid_argument("bad body_P_sensor index");
    if (own.n_shards > 1 && !own.owns_landmark(p.stereo_point[i])) continue;
    pose.push_back(p.stereo_pose[i]); pt.push_back(p.stereo_point[i]); nz.push_back(p.stereo_noise[i]);
    cal.push_back(p.stereo_calib[i]); sen.push_back(si < 0 ? -1 : si);
    for (int k = 0; k < 3; k++) z.push_back(p.stereo_z[3 * i + k]);
  }
  f.n_cam = (int64_t)pose.size();
  // the bearing / range factors (gtsam/sam) join the range behind the stereo factors the same way; they have no calib or sensor entry
  // and their measurements (a Unit3 and a range) stay in an array of their own, so that proj_z is what it was
  if (n_sam && (!p.sam_kind || !p.sam_pose || !p.sam_point || !p.sam_z || !p.sam_noise)) throw std::invalid_argument("bearing / range factor tables missing");
  std::vector<int32_t> sam_kind; std::vector<double> sam_z;
  for (int64_t i = 0; i < n_sam; i++) {
    const int kind = p.sam_kind[i];
    if (kind != GTG_SAM_BEARING_RANGE && kind != GTG_SAM_RANGE && kind != GTG_SAM_BEARING)
      throw std::invalid_argument("bearing / range factor: unknown sam_kind (GTG_SAM_BEARING_RANGE, GTG_SAM_RANGE or GTG_SAM_BEARING)");
    const char* what = kind == GTG_SAM_BEARING_RANGE ? "BearingRangeFactor" : kind == GTG_SAM_RANGE ? "RangeFactor" : "BearingFactor";
    check_var(p, p.sam_pose[i]); check_var(p, p.sam_point[i]);
    if (p.var_type[p.sam_pose[i]] != GTG_VAR_POSE3 || p.var_type[p.sam_point[i]] != GTG_VAR_POINT3)
      throw std::invalid_argument(std::string(what) + " keys must be (POSE3, POINT3)");
    check_noise(p, p.sam_noise[i], sam_rows(kind), what);
    if (own.n_shards > 1 && !own.owns_landmark(p.sam_point[i])) continue;
    pose.push_back(p.sam_pose[i]); pt.push_back(p.sam_point[i]); nz.push_back(p.sam_noise[i]);
    cal.push_back(-1); sen.push_back(-1);
    sam_kind.push_back(kind);
    for (int k = 0; k < 4; k++) sam_z.push_back(p.sam_z[4 * i + k]);
  }
  f.n_proj = (int64_t)pose.size();
  if (n_sam) { up(f.sam_kind, sam_kind, c.stream); up(f.sam_z, sam_z, c.stream); } else { f.sam_kind.free(); f.sam_z.free(); }
  up(f.proj_pose, pose, c.stream); up(f.proj_point, pt, c.stream); up(f.proj_noise, nz, c.stream); up(f.proj_calib, cal, c.stream);
  up(f.proj_sensor, sen, c.stream); up(f.proj_z, z, c.stream);
  // device calibration table: 9 per entry, fx fy s u0 v0 k1 k2 p1 p2 (the distortion part zero for a Cal3_S2)
  std::vector<double> calib(kCalibStride * (size_t)p.n_calib, 0.0), sensor(p.sensor, p.sensor + 12 * (size_t)p.n_sensor);
  for (int32_t k = 0; k < p.n_calib; k++) {
    for (int j = 0; j < 5; j++) calib[kCalibStride * (size_t)k + j] = p.calib[5 * (size_t)k + j];
    if (p.calib_distortion) for (int j = 0; j < 4; j++) calib[kCalibStride * (size_t)k + 5 + j] = p.calib_distortion[4 * (size_t)k + j];
  }
  up(f.calib, calib, c.stream); up(f.sensor, sensor, c.stream);
  if (f.form == ProjForm::Rows2Fisheye) up(f.calib_model, calib_model, c.stream); else f.calib_model.free();   // (a fisheye row: fx fy s u0 v0 k1 k2 k3 k4)
  if (n_stereo) {   // the baselines beside the table, so that the table and the kernels of a graph without stereo factors stay as they are
    std::vector<double> bl(p.calib_baseline, p.calib_baseline + p.n_calib);
    up(f.calib_baseline, bl, c.stream);
  } else f.calib_baseline.free();
  f.proj_J.alloc(std::max<size_t>((size_t)proj_rec(f.form) * f.n_proj, 1));
  hi.proj_pose = pose; hi.proj_point = pt;
}

void upload_between(gtg_context& c, HostIndex& hi, const gtg_problem& p, const ShardFilter& own) {
  auto& f = c.f;
  std::vector<int32_t> v1, v2, nz; std::vector<double> z;
  for (int64_t i = 0; i < p.n_between; i++) {
    check_var(p, p.between_v1[i]); check_var(p, p.between_v2[i]);
    check_noise(p, p.between_noise[i], tangent_dim(p.var_type[p.between_v1[i]]), "BetweenFactor");
    if (own.n_shards > 1 && !own.owns_round_robin(i)) continue;
    v1.push_back(p.between_v1[i]); v2.push_back(p.between_v2[i]); nz.push_back(p.between_noise[i]);
    for (int k = 0; k < 12; k++) z.push_back(p.between_z[12 * i + k]);
  }
  f.n_between = (int64_t)v1.size();
  up(f.between_v1, v1, c.stream); up(f.between_v2, v2, c.stream); up(f.between_noise, nz, c.stream); up(f.between_z, z, c.stream);
  f.between_J.alloc(std::max<size_t>((size_t)kBetweenRec * f.n_between, 1));
  hi.between_v1 = v1; hi.between_v2 = v2;
}

void upload_priors(gtg_context& c, HostIndex& hi, const gtg_problem& p, const ShardFilter& own) {
  auto& f = c.f;
  std::vector<int32_t> var, nz; std::vector<int64_t> poff; std::vector<double> data;
  for (int64_t i = 0; i < p.n_prior; i++) {
    const int v = p.prior_var[i];
    check_var(p, v);
    if (p.var_type[v] == GTG_VAR_POINT2) throw std::invalid_argument("PriorFactor on a POINT2 variable is not supported");
    check_noise(p, p.prior_noise[i], tangent_dim(p.var_type[v]), "PriorFactor");
    if (own.n_shards > 1 && !own.owns_prior(v, i)) continue;
    var.push_back(v); nz.push_back(p.prior_noise[i]); poff.push_back((int64_t)data.size());
    const double* d = p.prior_data + p.prior_off[i];
    for (int k = 0; k < storage_size(p.var_type[v]); k++) data.push_back(d[k]);
  }
  f.n_user_prior = (int64_t)var.size();
  // the partial pose priors (PoseTranslationPrior / PoseRotationPrior) join the prior range behind the caller's priors, the way the
  // smart measurements join the projection range: the symbolic analysis, the assembly, the linear error, PCG and the shard filter see
  // more priors and nothing else.  Dealt round-robin like the other non-landmark factors.
  const int64_t n_partial = p.n_pose_partial > 0 ? p.n_pose_partial : 0;
  if (n_partial && (!p.pose_partial_kind || !p.pose_partial_var || !p.pose_partial_z || !p.pose_partial_noise))
    throw std::invalid_argument("partial pose prior tables missing");
  std::vector<int32_t> partial_kind; std::vector<double> partial_z;
  for (int64_t i = 0; i < n_partial; i++) {
    const int kind = p.pose_partial_kind[i], v = p.pose_partial_var[i];
    if (kind != GTG_POSE_PARTIAL_TRANSLATION && kind != GTG_POSE_PARTIAL_ROTATION)
      throw std::invalid_argument("partial pose prior: unknown pose_partial_kind (GTG_POSE_PARTIAL_TRANSLATION or GTG_POSE_PARTIAL_ROTATION)");
    const char* what = kind == GTG_POSE_PARTIAL_TRANSLATION ? "PoseTranslationPrior" : "PoseRotationPrior";
    if (v < 0 || v >= p.n_vars || (p.var_type[v] != GTG_VAR_POSE3 && p.var_type[v] != GTG_VAR_POSE2))
      throw std::invalid_argument(std::string(what) + ": its key must be a POSE3 or POSE2 variable in Values");
    check_noise(p, p.pose_partial_noise[i], pose_partial_rows(kind, p.var_type[v]), what);
    if (own.n_shards > 1 && !own.owns_round_robin(i)) continue;
    var.push_back(v); nz.push_back(p.pose_partial_noise[i]);
    partial_kind.push_back(kind);
    for (int k = 0; k < kPosePartialZ; k++) partial_z.push_back(p.pose_partial_z[kPosePartialZ * i + k]);
  }
  if (n_partial) { up(f.partial_kind, partial_kind, c.stream); up(f.partial_z, partial_z, c.stream); } else { f.partial_kind.free(); f.partial_z.free(); }
  f.n_prior = (int64_t)var.size();
  up(f.prior_var, var, c.stream); up(f.prior_noise, nz, c.stream); up(f.prior_off, poff, c.stream); up(f.prior_data, data, c.stream);
  f.prior_J.alloc(std::max<size_t>((size_t)kPriorRec * f.n_prior, 1));
  hi.prior_var = var;
}

// landmark index of every smart factor's hidden variable (known once analyze() has classified the variables)
void link_smart_landmarks(gtg_context& c) {
  if (!c.n_smart) return;
  std::vector<int32_t> lm_smart((size_t)std::max(c.n_lm, 1), -1);
  for (int64_t i = 0; i < c.n_smart; i++) {
    const int l = c.h_lm_index[c.n_user_vars + i];
    if (l < 0) throw std::runtime_error("smart factor: its hidden landmark was not classified as a landmark");
    lm_smart[(size_t)l] = (int32_t)i;
  }
  up(c.lm_smart, lm_smart, c.stream);
  check_hip(hipStreamSynchronize(c.stream), "sync");
}

}  // namespace

void upload_problem(gtg_context& c, const gtg_problem& user, int shard, int n_shards) {
  // a handle holds one whole problem or none: an upload that throws half-way leaves none, not the tables of two behind "uploaded"
  c.uploaded = false; c.linearized = false; c.have_trial = false;
  StageClock clk;
  c.shard = shard; c.n_shards = n_shards;
  c.n_smart = user.n_smart > 0 ? user.n_smart : 0; c.n_user_vars = user.n_vars;
  // GeneralSFM records recomputed where they are needed instead of stored (fused.h) -- not with smart factors, whose measurements'
  // records depend on the factor's triangulation status, and not beside stereo or bearing / range factors, whose three-row records
  // only the stored-record kernels read
  std::vector<int32_t> pending_models;
  pending_models.swap(host_index(&c).calib_model);   // consumed by this upload, whatever becomes of it
  const bool planar = check_planar(user, n_shards);   // (its own records and kernels: context.h ProjForm::Planar)
  c.fused_sfm = GTG_FUSED_SFM != 0 && c.n_smart == 0 && !(user.n_stereo > 0) && !(user.n_sam > 0) && !planar;
  const std::vector<int32_t> calib_model = check_calibration_models(std::move(pending_models), user, planar);   // (empty: every calib row a pinhole)
  const SmartView view(user);
  const gtg_problem& p = view.problem();
  c.smart_pose = view.pose; c.smart_repeats = view.repeats; c.smart_obs0 = view.pose ? user.n_proj : user.n_sfm;
  upload_smart_state(c, user);
  layout_variables(c, p);
  upload_noise_table(c, p);
  const ShardFilter own(p, shard, n_shards);
  HostIndex& hi = host_index(&c);
  keep_whole_graph_keys(hi, p, n_shards);
  SideUpload side;   // started by upload_sfm for a whole, non-empty table
  upload_sfm(c, hi, p, view.of_obs, own, side);
  upload_projection(c, hi, p, view.of_obs, view.is_rig, own, planar, calib_model);
  upload_between(c, hi, p, own);
  upload_priors(c, hi, p, own);
  clk.lap("factor tables (shard filter + upload)");
  analyze(c);
  side.finish();
  link_smart_landmarks(c);
}

}  // namespace gt
