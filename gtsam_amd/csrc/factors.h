// factors.h -- one-factor evaluators: whitened Jacobian blocks + rhs, and the factor's error.
//
// Each function is what ONE lane executes for ONE factor.  They restate, for the GPU,
//   GeneralSFMFactor::linearize / evaluateError      slam/GeneralSFMFactor.h:127-177
//   GenericProjectionFactor::evaluateError           slam/ProjectionFactor.h:138-166
//   GenericStereoFactor<Pose3,Point3>::evaluateError  slam/StereoFactor.h:126-154
//   BearingRange / Range / BearingFactor<Pose3,Point3>  sam/*.h through nonlinear/ExpressionFactor.h:104-153
//   BearingRange / Range / BearingFactor<Pose2,Point2>  the same, planar
//   BetweenFactor<Pose3>::evaluateError              slam/BetweenFactor.h:111-124
//   PriorFactor<T>::evaluateError                    nonlinear/PriorFactor.h:98-102
// followed by NoiseModelFactor::linearize's  b = -r, WhitenSystem(A, b)
// (nonlinear/NonlinearFactor.cpp:150-182) and NoiseModelFactor::error = 0.5*||whiten(r)||^2
// (NonlinearFactor.cpp:136-147).
#pragma once
#include "geom.h"

namespace gt {

// A noise-table entry as the factor evaluators see it: base model + optional m-estimator.
struct NoiseRef {
  int kind; const double* data;   // GTG_NOISE_*, device data (inverse sigmas / R)
  int rkind; double rk;           // GTG_ROBUST_* (0 = none) and its parameter
};

// m-estimators (linear/LossFunctions.cpp): weight(distance) and loss(distance), distance = ||whitened residual||
GT_HD double robust_weight(int rkind, double k, double d) {
  const double a = fabs(d);
  switch (rkind) {
    case 1: return 1.0 / (1.0 + a / k);                                    // Fair   :146-148
    case 2: return (a <= k) ? 1.0 : (k / a);                               // Huber  :179-182
    case 3: return (k * k) / (k * k + d * d);                              // Cauchy :217-219
    case 4: { if (a <= k) { const double t = 1.0 - d * d / (k * k); return t * t; } return 0.0; }   // Tukey :250-256
    case 5: return exp(-(d * d) / (k * k));                                // Welsch :289-292
    case 6: { const double c2 = k * k, c4 = c2 * c2, ce = c2 + d * d; return c4 / (ce * ce); }     // Geman-McClure :320-325
    case 7: { const double e2 = d * d; if (e2 > k) { const double w = 2.0 * k / (k + e2); return w * w; } return 1.0; }   // DCS :355-364
    case 8: return (a <= k) ? 0.0 : (-k + a) / a;                          // L2WithDeadZone :402-409 (distance = a norm: >= 0)
    default: return 1.0;
  }
}
GT_HD double robust_loss(int rkind, double k, double d) {
  const double a = fabs(d);
  switch (rkind) {
    case 1: { const double ne = a / k; return k * k * (ne - log1p(ne)); }                            // :150-155
    case 2: return (a <= k) ? d * d / 2 : k * (a - (k / 2));                                         // :184-191
    case 3: return k * k * log1p(d * d / (k * k)) * 0.5;                                             // :221-224
    case 4: { if (a <= k) { const double t = 1.0 - d * d / (k * k); return k * k * (1 - t * t * t) / 6.0; } return k * k / 6.0; }  // :258-267
    case 5: return k * k * 0.5 * -expm1(-(d * d) / (k * k));                                         // :294-297
    case 6: { const double c2 = k * k, e2 = d * d; return 0.5 * (c2 * e2) / (c2 + e2); }             // :327-331
    case 7: { const double e2 = d * d, e4 = e2 * e2, c2 = k * k; return (c2 * e2 + k * e4) / ((e2 + k) * (e2 + k)); }   // DCS :366-375
    case 8: return (a < k) ? 0.0 : 0.5 * (k - a) * (k - a);                                          // L2WithDeadZone :411-414
    default: return 0.5 * d * d;
  }
}
// NoiseModelFactor::error: noiseModel_->loss(squaredMahalanobisDistance(r)) (NonlinearFactor.cpp:136-147);
// plain models 0.5 d^2, Robust robust_->loss(sqrt(d^2)) (NoiseModel.h:716-718)
GT_HD double factor_loss(const NoiseRef& n, double sq) { return n.rkind ? robust_loss(n.rkind, n.rk, sqrt(sq)) : 0.5 * sq; }
// Robust::WhitenSystem = noise_->WhitenSystem then robust_->reweight (Block scheme): scale by sqrt(weight(||b||))
GT_HD double reweight_factor(const NoiseRef& n, const double* b, int m) {
  if (!n.rkind) return 1.0;
  double s = 0.0;
  for (int i = 0; i < m; i++) s += b[i] * b[i];
  return sqrt(robust_weight(n.rkind, n.rk, sqrt(s)));
}

// row lengths of the per-factor Jacobian records (doubles)
constexpr int kSfmRec = 2 * 9 + 2 * 3 + 2;   // [A1 2x9 | A2 2x3 | b 2]
constexpr int kProjRec = 2 * 6 + 2 * 3 + 2;  // [A1 2x6 | A2 2x3 | b 2]
constexpr int kStereoRec = 3 * 6 + 3 * 3 + 3;  // [A1 3x6 | A2 3x3 | b 3]: every projection observation of a three-row graph (stereo or bearing / range factors)
constexpr int kBetweenRec = 36 + 36 + 6;     // [A1 6x6 | A2 6x6 | b 6]
constexpr int kPriorRec = 81 + 9;            // [A dxd packed | pad ... | b d at 81]

// ---- GeneralSFMFactor<PinholeCamera<Cal3Bundler>,Point3> ---------------------------------------
// NOTE (reference behaviour, reproduced on purpose): GeneralSFMFactor::linearize whitens H1, H2 and b through
// noiseModel->Whiten(Matrix) separately (GeneralSFMFactor.h:162-168); for a Robust model that path re-weights with
// an EMPTY error vector, i.e. weight 1 -- the m-estimator changes this factor's error(), not its linear system.
// The record must be the SAME DOUBLES in every kernel that inlines this function (k_lin_sfm and, since the fused linearisation, k_cam_fused,
// k_lm_fused, k_obs_E, k_obs_v, the PCG kernels and the debug getter): H_cc, V and W = Jc^T Jp are then blocks of ONE J^T J, and
// gtg_get_jacobians returns what was summed.  Left to itself the compiler contracts multiply-adds differently per kernel -- one rounding
// of pi is hundreds of ulps of b = z - pi -- so contraction is off here and in what this calls (geom.h: sfm_project, project2,
// mat3_tvec, whiten_cols); tests/test_gpu_reduced_system.py holds the sums to the summation bound on that ground.
GT_HD void sfm_linearize(const double* cam, const double* pt, const double* z, const NoiseRef& n, double* J) {
  _Pragma("clang fp contract(off)")
  const int nkind = n.kind; const double* nd = n.data;
  double pi[2];
  if (!sfm_project(cam, pt, pi, J, J + 18)) {  // CheiralityException: H1,H2,b = 0 (:153-158)
    for (int i = 0; i < kSfmRec; i++) J[i] = 0.0;
    return;
  }
  J[24] = z[0] - pi[0];
  J[25] = z[1] - pi[1];
  whiten_cols<2>(nkind, nd, J, 9);
  whiten_cols<2>(nkind, nd, J + 18, 3);
  whiten_cols<2>(nkind, nd, J + 24, 1);
}
GT_HD double sfm_error(const double* cam, const double* pt, const double* z, const NoiseRef& n) {
  double pi[2];
  if (!sfm_project(cam, pt, pi, nullptr, nullptr)) return factor_loss(n, 0.0);  // evaluateError returns Z_2x1 (:131-137)
  double r[2] = {pi[0] - z[0], pi[1] - z[1]};
  whiten_cols<2>(n.kind, n.data, r, 1);
  return factor_loss(n, r[0] * r[0] + r[1] * r[1]);
}

// One measurement of a smart factor whose landmark is a point at infinity (SmartFactorBase::computeJacobians<Unit3>,
// slam/SmartFactorBase.h:316-324, whitened as :356-363): the same record, the landmark block 2 x 2 padded with a zero column.
// false where the reference throws a CheiralityException (not caught by the smart factor).
GT_HD bool sfm_linearize_at_infinity(const double* cam, const double* dir, const double* z, const NoiseRef& n, double* J) {
  double pi[2];
  if (!sfm_project_at_infinity(cam, dir, pi, J, J + 18)) {
    for (int i = 0; i < kSfmRec; i++) J[i] = 0.0;
    return false;
  }
  J[24] = z[0] - pi[0];
  J[25] = z[1] - pi[1];
  whiten_cols<2>(n.kind, n.data, J, 9);
  whiten_cols<2>(n.kind, n.data, J + 18, 3);
  whiten_cols<2>(n.kind, n.data, J + 24, 1);
  // A Robust model here: the factor's own linearize() whitens H1, H2 and b ONE AT A TIME through Robust::Whiten(Matrix), whose
  // WhitenSystem sees an empty b -- the m-estimator's weight is evaluated at distance 0 (slam/GeneralSFMFactor.h:162-168,
  // linear/NoiseModel.h:711-714).  That is exactly 1 for every estimator but L2WithDeadZone, whose weight(0) is 0: the reference
  // drops the factor from the linear system (and keeps it in the error); so does this.
  if (n.rkind) { const double w = sqrt(robust_weight(n.rkind, n.rk, 0.0)); if (w != 1.0) for (int i = 0; i < kSfmRec; i++) J[i] *= w; }
  return true;
}
// its share of SmartFactorBase::totalReprojectionError<Unit3> (SmartFactorBase.h:296-303): 0.5 |whitened (h - z)|^2
GT_HD bool sfm_error_at_infinity(const double* cam, const double* dir, const double* z, const NoiseRef& n, double* e) {
  double pi[2];
  *e = 0.0;
  if (!sfm_project_at_infinity(cam, dir, pi, nullptr, nullptr)) return false;
  double r[2] = {pi[0] - z[0], pi[1] - z[1]};
  whiten_cols<2>(n.kind, n.data, r, 1);
  *e = 0.5 * (r[0] * r[0] + r[1] * r[1]);
  return true;
}

// ---- GenericProjectionFactor<Pose3,Point3,Cal3_S2> ---------------------------------------------
GT_HD void proj_linearize(const double* pose, const double* K, const double* sensor, const double* pt,
                          const double* z, const NoiseRef& n, double* J) {
  const int nkind = n.kind; const double* nd = n.data;
  double pi[2];
  bool ok;
  if (sensor) {  // pose.compose(body_P_sensor, H0); H1 = H1 * H0, H0 = sensor^-1 AdjointMap (Lie.h:56-61)
    double T[12], Dp[12], Si[12], H0[36];
    pose_compose(pose, sensor, T);
    ok = s2_project(T, K, pt, pi, Dp, J + 12);
    if (ok) {
      pose_inverse(sensor, Si);
      pose_adjoint(Si, H0);
      for (int r = 0; r < 2; r++)
        for (int c = 0; c < 6; c++) {
          double acc = 0.0;
          for (int k = 0; k < 6; k++) acc += Dp[6 * r + k] * H0[6 * k + c];
          J[6 * r + c] = acc;
        }
    }
  } else {
    ok = s2_project(pose, K, pt, pi, J, J + 12);
  }
  if (!ok) {  // H = 0 and residual 2*fx (ProjectionFactor.h:157-165, throwCheirality_ = false)
    for (int i = 0; i < 18; i++) J[i] = 0.0;
    J[18] = -2.0 * K[0]; J[19] = -2.0 * K[0];
  } else {
    J[18] = -(pi[0] - z[0]); J[19] = -(pi[1] - z[1]);
  }
  whiten_cols<2>(nkind, nd, J, 6);
  whiten_cols<2>(nkind, nd, J + 12, 3);
  whiten_cols<2>(nkind, nd, J + 18, 1);
  if (n.rkind) { const double w = reweight_factor(n, J + 18, 2); for (int i = 0; i < kProjRec; i++) J[i] *= w; }
}
GT_HD double proj_error(const double* pose, const double* K, const double* sensor, const double* pt,
                        const double* z, const NoiseRef& n) {
  double pi[2], r[2];
  bool ok;
  if (sensor) {
    double T[12];
    pose_compose(pose, sensor, T);
    ok = s2_project(T, K, pt, pi, nullptr, nullptr);
  } else {
    ok = s2_project(pose, K, pt, pi, nullptr, nullptr);
  }
  if (ok) { r[0] = pi[0] - z[0]; r[1] = pi[1] - z[1]; }
  else { r[0] = 2.0 * K[0]; r[1] = 2.0 * K[0]; }
  whiten_cols<2>(n.kind, n.data, r, 1);
  return factor_loss(n, r[0] * r[0] + r[1] * r[1]);
}

// ---- GenericProjectionFactor<Pose3,Point3,Cal3Fisheye> -----------------------------------------
// The same factor (slam/ProjectionFactor.h:138-166) through PinholeCamera<Cal3Fisheye>: K = fx, fy, s, u0, v0, k1, k2, k3, k4.  The contract
// of proj_linearize / proj_error, written out beside them so that the two-row kernels of the pinhole models keep their instruction
// streams (factors.hip, above k_lin_proj): the record [A1 2x6 | A2 2x3 | b 2] of kProjRec doubles.
GT_HD void proj_linearize_fisheye(const double* pose, const double* K, const double* sensor, const double* pt,
                                  const double* z, const NoiseRef& n, double* J) {
  const int nkind = n.kind; const double* nd = n.data;
  double pi[2];
  bool ok;
  if (sensor) {  // pose.compose(body_P_sensor, H0); H1 = H1 * H0, H0 = sensor^-1 AdjointMap (Lie.h:56-61)
    double T[12], Dp[12], Si[12], H0[36];
    pose_compose(pose, sensor, T);
    ok = fisheye_project(T, K, pt, pi, Dp, J + 12);
    if (ok) {
      pose_inverse(sensor, Si);
      pose_adjoint(Si, H0);
      for (int r = 0; r < 2; r++)
        for (int c = 0; c < 6; c++) {
          double acc = 0.0;
          for (int k = 0; k < 6; k++) acc += Dp[6 * r + k] * H0[6 * k + c];
          J[6 * r + c] = acc;
        }
    }
  } else {
    ok = fisheye_project(pose, K, pt, pi, J, J + 12);
  }
  if (!ok) {  // H = 0 and residual 2*fx (ProjectionFactor.h:157-165, throwCheirality_ = false)
    for (int i = 0; i < 18; i++) J[i] = 0.0;
    J[18] = -2.0 * K[0]; J[19] = -2.0 * K[0];
  } else {
    J[18] = -(pi[0] - z[0]); J[19] = -(pi[1] - z[1]);
  }
  whiten_cols<2>(nkind, nd, J, 6);
  whiten_cols<2>(nkind, nd, J + 12, 3);
  whiten_cols<2>(nkind, nd, J + 18, 1);
  if (n.rkind) { const double w = reweight_factor(n, J + 18, 2); for (int i = 0; i < kProjRec; i++) J[i] *= w; }
}
GT_HD double proj_error_fisheye(const double* pose, const double* K, const double* sensor, const double* pt,
                                const double* z, const NoiseRef& n) {
  double pi[2], r[2];
  bool ok;
  if (sensor) {
    double T[12];
    pose_compose(pose, sensor, T);
    ok = fisheye_project(T, K, pt, pi, nullptr, nullptr);
  } else {
    ok = fisheye_project(pose, K, pt, pi, nullptr, nullptr);
  }
  if (ok) { r[0] = pi[0] - z[0]; r[1] = pi[1] - z[1]; }
  else { r[0] = 2.0 * K[0]; r[1] = 2.0 * K[0]; }
  whiten_cols<2>(n.kind, n.data, r, 1);
  return factor_loss(n, r[0] * r[0] + r[1] * r[1]);
}

// One measurement of a SmartProjectionPoseFactor<Cal3_S2> whose landmark is a point at infinity (SmartFactorBase::computeJacobians<Unit3>,
// slam/SmartFactorBase.h:203-239, whitened by the isotropic model): the projection record with F = Dpose (rotation part only) times
// the H of world_P_body.compose(body_P_sensor) when there is a sensor (:216-233), the landmark block 2 x 2 padded with a zero column.
// false where the reference throws a CheiralityException (not caught by the smart factor).
GT_HD bool proj_linearize_at_infinity(const double* pose, const double* K, const double* sensor, const double* dir,
                                      const double* z, const NoiseRef& n, double* J) {
  double pi[2];
  bool ok;
  if (sensor) {
    double T[12], Dp[12], Si[12], H0[36];
    pose_compose(pose, sensor, T);
    ok = s2_project_at_infinity(T, K, dir, pi, Dp, J + 12);
    if (ok) {
      pose_inverse(sensor, Si);
      pose_adjoint(Si, H0);
      for (int r = 0; r < 2; r++)
        for (int c = 0; c < 6; c++) {
          double acc = 0.0;
          for (int k = 0; k < 6; k++) acc += Dp[6 * r + k] * H0[6 * k + c];
          J[6 * r + c] = acc;
        }
    }
  } else {
    ok = s2_project_at_infinity(pose, K, dir, pi, J, J + 12);
  }
  if (!ok) {
    for (int i = 0; i < kProjRec; i++) J[i] = 0.0;
    return false;
  }
  J[18] = z[0] - pi[0];
  J[19] = z[1] - pi[1];
  whiten_cols<2>(n.kind, n.data, J, 6);
  whiten_cols<2>(n.kind, n.data, J + 12, 3);
  whiten_cols<2>(n.kind, n.data, J + 18, 1);
  return true;
}
// its share of SmartFactorBase::totalReprojectionError<Unit3> (SmartFactorBase.h:296-303): 0.5 |whitened (h - z)|^2
GT_HD bool proj_error_at_infinity(const double* pose, const double* K, const double* sensor, const double* dir,
                                  const double* z, const NoiseRef& n, double* e) {
  double pi[2];
  bool ok;
  *e = 0.0;
  if (sensor) {
    double T[12];
    pose_compose(pose, sensor, T);
    ok = s2_project_at_infinity(T, K, dir, pi, nullptr, nullptr);
  } else {
    ok = s2_project_at_infinity(pose, K, dir, pi, nullptr, nullptr);
  }
  if (!ok) return false;
  double r[2] = {pi[0] - z[0], pi[1] - z[1]};
  whiten_cols<2>(n.kind, n.data, r, 1);
  *e = 0.5 * (r[0] * r[0] + r[1] * r[1]);
  return true;
}

// ---- GenericStereoFactor<Pose3,Point3> ---------------------------------------------------------
// Three residual rows (uL, uR, v) where the monocular factor has two; K = the calib table entry (skew unused), bl = its baseline.
GT_HD void stereo_linearize(const double* pose, const double* K, double bl, const double* sensor, const double* pt,
                            const double* z, const NoiseRef& n, double* J) {
  const int nkind = n.kind; const double* nd = n.data;
  double pi[3];
  bool ok;
  if (sensor) {  // pose.compose(body_P_sensor, H0); H1 = H1 * H0 (StereoFactor.h:129-135)
    double T[12], Dp[18], Si[12], H0[36];
    pose_compose(pose, sensor, T);
    ok = stereo_project(T, K, bl, pt, pi, Dp, J + 18);
    if (ok) {
      pose_inverse(sensor, Si);
      pose_adjoint(Si, H0);
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 6; c++) {
          double acc = 0.0;
          for (int k = 0; k < 6; k++) acc += Dp[6 * r + k] * H0[6 * k + c];
          J[6 * r + c] = acc;
        }
    }
  } else {
    ok = stereo_project(pose, K, bl, pt, pi, J, J + 18);
  }
  if (!ok) {  // H = 0 and residual Vector3::Constant(2 fx) (StereoFactor.h:144-153, throwCheirality_ = false)
    for (int i = 0; i < 27; i++) J[i] = 0.0;
    J[27] = -2.0 * K[0]; J[28] = -2.0 * K[0]; J[29] = -2.0 * K[0];
  } else {
    J[27] = -(pi[0] - z[0]); J[28] = -(pi[1] - z[1]); J[29] = -(pi[2] - z[2]);
  }
  whiten_cols<3>(nkind, nd, J, 6);
  whiten_cols<3>(nkind, nd, J + 18, 3);
  whiten_cols<3>(nkind, nd, J + 27, 1);
  if (n.rkind) { const double w = reweight_factor(n, J + 27, 3); for (int i = 0; i < kStereoRec; i++) J[i] *= w; }
}
// the whitened residual h(x) - z of the factor (what its error is the loss of)
GT_HD void stereo_residual(const double* pose, const double* K, double bl, const double* sensor, const double* pt,
                           const double* z, const NoiseRef& n, double* r) {
  double pi[3];
  bool ok;
  if (sensor) {
    double T[12];
    pose_compose(pose, sensor, T);
    ok = stereo_project(T, K, bl, pt, pi, nullptr, nullptr);
  } else {
    ok = stereo_project(pose, K, bl, pt, pi, nullptr, nullptr);
  }
  if (ok) { r[0] = pi[0] - z[0]; r[1] = pi[1] - z[1]; r[2] = pi[2] - z[2]; }
  else { r[0] = 2.0 * K[0]; r[1] = 2.0 * K[0]; r[2] = 2.0 * K[0]; }
  whiten_cols<3>(n.kind, n.data, r, 1);
}
GT_HD double stereo_error(const double* pose, const double* K, double bl, const double* sensor, const double* pt,
                          const double* z, const NoiseRef& n) {
  double r[3];
  stereo_residual(pose, K, bl, sensor, pt, z, n, r);
  return factor_loss(n, r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
}
// A monocular factor of a graph that also has stereo factors: the same doubles as proj_linearize gives, in the three-row layout with
// a zero third row, so that one record size serves the whole observation range.
GT_HD void proj_linearize_rows3(const double* pose, const double* K, const double* sensor, const double* pt,
                                const double* z, const NoiseRef& n, double* J) {
  proj_linearize(pose, K, sensor, pt, z, n, J);   // [A1 2x6 | A2 2x3 | b 2] in the first 20 places
  const double a0 = J[12], a1 = J[13], a2 = J[14], a3 = J[15], a4 = J[16], a5 = J[17], b0 = J[18], b1 = J[19];
  for (int i = 12; i < 18; i++) J[i] = 0.0;
  J[18] = a0; J[19] = a1; J[20] = a2; J[21] = a3; J[22] = a4; J[23] = a5;
  J[24] = 0.0; J[25] = 0.0; J[26] = 0.0;
  J[27] = b0; J[28] = b1; J[29] = 0.0;
}

// ---- BearingRangeFactor / RangeFactor / BearingFactor <Pose3,Point3> (gtsam/sam) ---------------
// ExpressionFactorN (nonlinear/ExpressionFactor.h:104-153): h = Pose3::bearing / Pose3::range of the point (geometry/Pose3.cpp:399-439),
// b = Local(h, z) -- [h_bearing.localCoordinates(z_bearing) ; z_range - h_range] (BearingRange.h:138-144), in the basis of the PREDICTED
// direction -- the Jacobians those of h alone (the chart derivative of Local is not applied), then WhitenSystem on the whole system
// (:147-150): a Robust model re-weights by sqrt(weight(|whitened b|)).  z: the measured Unit3's three doubles, then the range.
// The record is the three-row one (kStereoRec): bearing rows 0-1 and range row 2; a range-only factor in row 0; unused rows exactly 0.
// Contraction is off as in sfm_linearize: q - x p and 1 - x^2 of the bearing (geom.h unit3_local) cancel, so the record must not depend
// on which kernel, or which compiler (the host compile of the CPU parity test), inlined this.
enum { kSamBearingRange = 0, kSamRange = 1, kSamBearing = 2 };   // = GTG_SAM_*
GT_HD int sam_rows(int kind) { return kind == kSamBearingRange ? 3 : kind == kSamRange ? 1 : 2; }
// the unwhitened compact system [A1 ROWS x 6 | A2 ROWS x 3 | b ROWS] (A1 = nullptr: b alone)
template <int KIND>
GT_HD void sam_system(const double* pose, const double* pt, const double* z, double* A1, double* A2, double* b) {
  _Pragma("clang fp contract(off)")
  const double dp[3] = {pt[0] - pose[9], pt[1] - pose[10], pt[2] - pose[11]};
  double q[3];
  mat3_tvec(pose, dp, q);   // Pose3::transformTo
  constexpr int r0 = KIND == kSamRange ? 0 : 2;   // the range's row
  if (KIND != kSamRange) {
    double h[3], b1[3], b2[3], D[6];
    unit3_from_point(q, h, b1, b2, A1 ? D : nullptr);
    if (A1) { local_chain_row(pose, q, D, A1, A2); local_chain_row(pose, q, D + 3, A1 + 6, A2 + 3); }
    unit3_local(h, b1, b2, z, b);
  }
  if (KIND != kSamBearing) {
    double D[3];
    const double r = norm3_with_derivative(q, D);
    if (A1) local_chain_row(pose, q, D, A1 + 6 * r0, A2 + 3 * r0);
    b[r0] = z[3] - r;
  }
}
template <int KIND>
GT_HD void sam_linearize_kind(const double* pose, const double* pt, const double* z, const NoiseRef& n, double* J) {
  _Pragma("clang fp contract(off)")
  constexpr int R = KIND == kSamBearingRange ? 3 : KIND == kSamRange ? 1 : 2;
  double A1[6 * R], A2[3 * R], b[R];
  sam_system<KIND>(pose, pt, z, A1, A2, b);
  whiten_cols<R>(n.kind, n.data, A1, 6);
  whiten_cols<R>(n.kind, n.data, A2, 3);
  whiten_cols<R>(n.kind, n.data, b, 1);
  if (n.rkind) {
    const double w = reweight_factor(n, b, R);
    for (int i = 0; i < 6 * R; i++) A1[i] *= w;
    for (int i = 0; i < 3 * R; i++) A2[i] *= w;
    for (int i = 0; i < R; i++) b[i] *= w;
  }
  for (int i = 0; i < kStereoRec; i++) J[i] = 0.0;
  for (int r = 0; r < R; r++) {
    for (int k = 0; k < 6; k++) J[6 * r + k] = A1[6 * r + k];
    for (int k = 0; k < 3; k++) J[18 + 3 * r + k] = A2[3 * r + k];
    J[27 + r] = b[r];
  }
}
GT_HD void sam_linearize(int kind, const double* pose, const double* pt, const double* z, const NoiseRef& n, double* J) {
  if (kind == kSamBearingRange) sam_linearize_kind<kSamBearingRange>(pose, pt, z, n, J);
  else if (kind == kSamRange) sam_linearize_kind<kSamRange>(pose, pt, z, n, J);
  else sam_linearize_kind<kSamBearing>(pose, pt, z, n, J);
}
// the whitened residual -Local(h, z) of the factor in its first sam_rows(kind) places (what its error is the loss of)
template <int KIND>
GT_HD double sam_residual_kind(const double* pose, const double* pt, const double* z, const NoiseRef& n, double* r) {
  constexpr int R = KIND == kSamBearingRange ? 3 : KIND == kSamRange ? 1 : 2;
  sam_system<KIND>(pose, pt, z, nullptr, nullptr, r);
  for (int i = 0; i < R; i++) r[i] = -r[i];
  whiten_cols<R>(n.kind, n.data, r, 1);
  double sq = 0.0;
  for (int i = 0; i < R; i++) sq += r[i] * r[i];
  return sq;
}
GT_HD double sam_residual(int kind, const double* pose, const double* pt, const double* z, const NoiseRef& n, double* r) {
  if (kind == kSamBearingRange) return sam_residual_kind<kSamBearingRange>(pose, pt, z, n, r);
  if (kind == kSamRange) return sam_residual_kind<kSamRange>(pose, pt, z, n, r);
  return sam_residual_kind<kSamBearing>(pose, pt, z, n, r);
}
GT_HD double sam_error(int kind, const double* pose, const double* pt, const double* z, const NoiseRef& n) {
  double r[3];
  return factor_loss(n, sam_residual(kind, pose, pt, z, n, r));
}

// ---- BearingRangeFactor / RangeFactor / BearingFactor <Pose2,Point2> (gtsam/sam, planar) -------
// The same ExpressionFactorN as above with h = Pose2::bearing / Pose2::range of the landmark:
//   transformTo (geometry/Pose2.cpp:207-214, Rot2::unrotate Rot2.cpp:110-116): q = R^T (p - t), Hpose = [-1 0 q.y; 0 -1 -q.x], Hpoint = R^T
//   bearing (Pose2.cpp:245-256) = Rot2::relativeBearing(q) (Rot2.cpp:119-130): H = [-y/d2, x/d2] and fromCosSin(x/n, y/n) when n > 1e-5,
//     otherwise the identity rotation with a ZERO Jacobian
//   range (Pose2.cpp:270-284) = norm2(p - t) (Point2.cpp:27-36), Jacobian (1, 1) at r <= 1e-10, Hpose = D [-c s 0; -s -c 0], Hpoint = D
//   b = Local(h, z) = [theta(h^-1 z) ; z_range - h_range] (BearingRange.h:138-144); the product goes through Rot2::operator* /
//     fromCosSin (re-normalised beyond 1e-10 only, Rot2.cpp:56-64), the angle is atan2's
// The Jacobians are those of h alone; the whole system is whitened, a Robust model re-weights by sqrt(weight(|whitened b|)).
// pose: (x, y, theta) as stored; pt: (x, y, 0), the POINT2 padded to the landmark slot; z: (c, s) of the measured Rot2 as the reference
// holds it, then the range.  Record [A1 3x3 | A2 3x3 | b 3] (kPlanarRec): bearing in row 0 and range in row 1 of a bearing-range factor,
// a bearing-only or range-only factor in row 0; A2's third column and every unused row are exactly 0.
// Contraction is off where p - t, the products of unrotate and h^-1 z are formed: one record, the same doubles in every kernel and in
// the host compile of the CPU parity test.
constexpr int kPlanarRec = 3 * 3 + 3 * 3 + 3;
GT_HD int sam2_rows(int kind) { return kind == kSamBearingRange ? 2 : 1; }
// the unwhitened compact system [A1 ROWS x 3 | A2 ROWS x 2 | b ROWS] (A1 = nullptr: b alone)
template <int KIND>
GT_HD void sam2_system(const double* pose, const double* pt, const double* z, double* A1, double* A2, double* b) {
  _Pragma("clang fp contract(off)")
  const double c = cos(pose[2]), s = sin(pose[2]);
  const double dx = pt[0] - pose[0], dy = pt[1] - pose[1];
  constexpr int r0 = KIND == kSamBearingRange ? 1 : 0;   // the range's row
  if (KIND != kSamRange) {
    const double qx = c * dx + s * dy, qy = -s * dx + c * dy;
    const double d2 = qx * qx + qy * qy, n = sqrt(d2);
    double hc = 1.0, hs = 0.0, H0 = 0.0, H1 = 0.0;
    if (fabs(n) > 1e-5) {
      H0 = -qy / d2; H1 = qx / d2;
      hc = qx / n; hs = qy / n;
      rot2_normalize(hc, hs);
    }
    if (A1) {
      A1[0] = H0 * -1.0 + H1 * 0.0; A1[1] = H0 * 0.0 + H1 * -1.0; A1[2] = H0 * qy + H1 * -qx;
      A2[0] = H0 * c + H1 * -s; A2[1] = H0 * s + H1 * c;
    }
    // h^-1 z: Rot2(hc, -hs) * Rot2(z0, z1)
    double bc = hc * z[0] - (-hs) * z[1], bs = (-hs) * z[0] + hc * z[1];
    rot2_normalize(bc, bs);
    b[0] = atan2(bs, bc);
  }
  if (KIND != kSamBearing) {
    const double r = sqrt(dx * dx + dy * dy);
    double D0 = 1.0, D1 = 1.0;
    if (fabs(r) > 1e-10) { D0 = dx / r; D1 = dy / r; }
    if (A1) {
      A1[3 * r0] = D0 * -c + D1 * -s; A1[3 * r0 + 1] = D0 * s + D1 * -c; A1[3 * r0 + 2] = D0 * 0.0 + D1 * 0.0;
      A2[2 * r0] = D0; A2[2 * r0 + 1] = D1;
    }
    b[r0] = z[2] - r;
  }
}
template <int KIND>
GT_HD void sam2_linearize_kind(const double* pose, const double* pt, const double* z, const NoiseRef& n, double* J) {
  _Pragma("clang fp contract(off)")
  constexpr int R = KIND == kSamBearingRange ? 2 : 1;
  double A1[3 * R], A2[2 * R], b[R];
  sam2_system<KIND>(pose, pt, z, A1, A2, b);
  whiten_cols<R>(n.kind, n.data, A1, 3);
  whiten_cols<R>(n.kind, n.data, A2, 2);
  whiten_cols<R>(n.kind, n.data, b, 1);
  if (n.rkind) {
    const double w = reweight_factor(n, b, R);
    for (int i = 0; i < 3 * R; i++) A1[i] *= w;
    for (int i = 0; i < 2 * R; i++) A2[i] *= w;
    for (int i = 0; i < R; i++) b[i] *= w;
  }
  for (int i = 0; i < kPlanarRec; i++) J[i] = 0.0;
  for (int r = 0; r < R; r++) {
    for (int k = 0; k < 3; k++) J[3 * r + k] = A1[3 * r + k];
    for (int k = 0; k < 2; k++) J[9 + 3 * r + k] = A2[2 * r + k];
    J[18 + r] = b[r];
  }
}
GT_HD void sam2_linearize(int kind, const double* pose, const double* pt, const double* z, const NoiseRef& n, double* J) {
  if (kind == kSamBearingRange) sam2_linearize_kind<kSamBearingRange>(pose, pt, z, n, J);
  else if (kind == kSamRange) sam2_linearize_kind<kSamRange>(pose, pt, z, n, J);
  else sam2_linearize_kind<kSamBearing>(pose, pt, z, n, J);
}
// the whitened residual -Local(h, z) of the factor in its first sam2_rows(kind) places (what its error is the loss of)
template <int KIND>
GT_HD double sam2_residual_kind(const double* pose, const double* pt, const double* z, const NoiseRef& n, double* r) {
  constexpr int R = KIND == kSamBearingRange ? 2 : 1;
  sam2_system<KIND>(pose, pt, z, nullptr, nullptr, r);
  for (int i = 0; i < R; i++) r[i] = -r[i];
  whiten_cols<R>(n.kind, n.data, r, 1);
  double sq = 0.0;
  for (int i = 0; i < R; i++) sq += r[i] * r[i];
  return sq;
}
GT_HD double sam2_residual(int kind, const double* pose, const double* pt, const double* z, const NoiseRef& n, double* r) {
  if (kind == kSamBearingRange) return sam2_residual_kind<kSamBearingRange>(pose, pt, z, n, r);
  if (kind == kSamRange) return sam2_residual_kind<kSamRange>(pose, pt, z, n, r);
  return sam2_residual_kind<kSamBearing>(pose, pt, z, n, r);
}
GT_HD double sam2_error(int kind, const double* pose, const double* pt, const double* z, const NoiseRef& n) {
  double r[2];
  return factor_loss(n, sam2_residual(kind, pose, pt, z, n, r));
}

// ---- BetweenFactor<Pose3> ---------------------------------------------------------------------
// h = T1^-1 T2 ; H1 = -Ad(h^-1), H2 = I (Lie.h:63-69) ; r = Logmap(z^-1 h), Jacobians NOT
// multiplied by dLog (GTSAM_SLOW_BUT_CORRECT_BETWEENFACTOR is OFF by default, BetweenFactor.h:115-123)
GT_HD void between_residual(const double* T1, const double* T2, const double* Z, double* h, double* r) {
  pose_between(T1, T2, h);
  pose_local(Z, h, r);
}
GT_HD void between_linearize(const double* T1, const double* T2, const double* Z, const NoiseRef& n, double* J) {
  const int nkind = n.kind; const double* nd = n.data;
  double h[12], hi[12], r[6];
  between_residual(T1, T2, Z, h, r);
  pose_inverse(h, hi);
  pose_adjoint(hi, J);
  for (int i = 0; i < 36; i++) J[i] = -J[i];
  for (int i = 0; i < 36; i++) J[36 + i] = 0.0;
  for (int i = 0; i < 6; i++) J[36 + 7 * i] = 1.0;
  for (int i = 0; i < 6; i++) J[72 + i] = -r[i];
  whiten_cols<6>(nkind, nd, J, 6);
  whiten_cols<6>(nkind, nd, J + 36, 6);
  whiten_cols<6>(nkind, nd, J + 72, 1);
  if (n.rkind) { const double w = reweight_factor(n, J + 72, 6); for (int i = 0; i < kBetweenRec; i++) J[i] *= w; }
}
GT_HD double between_error(const double* T1, const double* T2, const double* Z, const NoiseRef& n) {
  double h[12], r[6];
  between_residual(T1, T2, Z, h, r);
  whiten_cols<6>(n.kind, n.data, r, 1);
  double e = 0.0;
  for (int i = 0; i < 6; i++) e += r[i] * r[i];
  return factor_loss(n, e);
}

// ---- BetweenFactor<Pose2> ---------------------------------------------------------------------
// Same generic LieGroup::between (Lie.h:63-69): h = p1^-1 p2, H1 = -Ad(h^-1) (Pose2.cpp:126-135), H2 = I;
// r = Local(z, h) = (x, y, theta) of z^-1 h, Jacobians not multiplied by the chart derivative (default flags).
// Record = the BetweenFactor<Pose3> record with 3x3 blocks: A1 at [0..8], A2 at [36..44], b at [72..74].
GT_HD void between2_residual(const double* p1, const double* p2, const double* z, double* h, double* r) {
  pose2_between_cs(p1[0], p1[1], cos(p1[2]), sin(p1[2]), p2[0], p2[1], cos(p2[2]), sin(p2[2]), h);
  double g[4];
  pose2_between_cs(z[0], z[1], cos(z[2]), sin(z[2]), h[0], h[1], h[2], h[3], g);
  r[0] = g[0]; r[1] = g[1]; r[2] = atan2(g[3], g[2]);
}
GT_HD void between2_linearize(const double* p1, const double* p2, const double* z, const NoiseRef& n, double* J) {
  double h[4], r[3];
  between2_residual(p1, p2, z, h, r);
  for (int i = 0; i < kBetweenRec; i++) J[i] = 0.0;
  // h^-1 = (c, -s, unrotate(-t_h)); Ad(pose) = [c -s y; s c -x; 0 0 1]
  const double c = h[2], s = -h[3];
  const double x = h[2] * (-h[0]) + h[3] * (-h[1]), y = -h[3] * (-h[0]) + h[2] * (-h[1]);
  J[0] = -c; J[1] = s; J[2] = -y;
  J[3] = -s; J[4] = -c; J[5] = x;
  J[6] = 0.0; J[7] = 0.0; J[8] = -1.0;
  J[36] = 1.0; J[40] = 1.0; J[44] = 1.0;
  for (int i = 0; i < 3; i++) J[72 + i] = -r[i];
  whiten_cols<3>(n.kind, n.data, J, 3);
  whiten_cols<3>(n.kind, n.data, J + 36, 3);
  whiten_cols<3>(n.kind, n.data, J + 72, 1);
  if (n.rkind) { const double w = reweight_factor(n, J + 72, 3); for (int i = 0; i < kBetweenRec; i++) J[i] *= w; }
}
GT_HD double between2_error(const double* p1, const double* p2, const double* z, const NoiseRef& n) {
  double h[4], r[3];
  between2_residual(p1, p2, z, h, r);
  whiten_cols<3>(n.kind, n.data, r, 1);
  return factor_loss(n, r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
}

// ---- PriorFactor<T> ---------------------------------------------------------------------------
// r = -Local(x, prior), H = I (approximate on purpose, PriorFactor.h:99).  d = tangent dim.
template <int D>
GT_HD void prior_linearize_d(int vtype, const double* x, const double* z, const NoiseRef& n, double* J) {
  const int nkind = n.kind; const double* nd = n.data;
  double loc[9];
  value_local(vtype, x, z, loc);
  for (int i = 0; i < kPriorRec; i++) J[i] = 0.0;
  for (int i = 0; i < D; i++) J[i * D + i] = 1.0;
  for (int i = 0; i < D; i++) J[81 + i] = loc[i];  // b = -r = Local(x, prior)
  whiten_cols<D>(nkind, nd, J, D);
  whiten_cols<D>(nkind, nd, J + 81, 1);
  if (n.rkind) { const double w = reweight_factor(n, J + 81, D); for (int i = 0; i < kPriorRec; i++) J[i] *= w; }
}
GT_HD void prior_linearize(int vtype, const double* x, const double* z, const NoiseRef& n, double* J) {
  if (vtype == 0) prior_linearize_d<6>(vtype, x, z, n, J);
  else if (vtype == 1) prior_linearize_d<9>(vtype, x, z, n, J);
  else prior_linearize_d<3>(vtype, x, z, n, J);
}
GT_HD double prior_error(int vtype, const double* x, const double* z, const NoiseRef& n) {
  double r[9];
  value_local(vtype, x, z, r);
  const int d = vtype == 0 ? 6 : vtype == 1 ? 9 : 3;
  if (d == 6) whiten_cols<6>(n.kind, n.data, r, 1);
  else if (d == 9) whiten_cols<9>(n.kind, n.data, r, 1);
  else whiten_cols<3>(n.kind, n.data, r, 1);
  double e = 0.0;
  for (int i = 0; i < d; i++) e += r[i] * r[i];
  return factor_loss(n, e);
}

// ---- PoseTranslationPrior<POSE> / PoseRotationPrior<POSE>, POSE = Pose3 | Pose2 -----------------
// The absolute fix of part of a pose (slam/PoseTranslationPrior.h:65-77, slam/PoseRotationPrior.h:81-90).  The kind and the variable's
// type give the form:
//   translation, Pose3: r = t - z (traits<Point3>::Local(z, t)), H = [0 | R]
//   rotation,    Pose3: r = Z.localCoordinates(R) = SO3::Logmap(Z^T R) (GTSAM_ROT3_EXPMAP), H = [I | 0] -- the identity block the
//                       reference writes, NOT the derivative of Logmap
//   translation, Pose2: r = t - z, H = [[c -s], [s c] | 0]
//   rotation,    Pose2: r = theta of Rot2(c_z, -s_z) * Rot2(c, s) (Rot2::localCoordinates: between, then atan2; the product goes through
//                       Rot2::fromCosSin, which re-normalises only beyond 1e-10, Rot2.cpp:56-64), H = [0 0 1]
// then b = -r and WhitenSystem on the whole system.  z: 9 doubles per factor (the measured Point3 | Rot3 row-major | Point2 | c_z, s_z),
// the rest 0.  The record is the PRIOR record of the pose's tangent dimension D ([A D x D | b at 81]) with the factor's R rows first and
// every other entry exactly 0.  Contraction is off where t - z and the entries of Z^T R are formed: the Taylor branch of Logmap sees
// differences of entries that are equal up to rounding, and the record must not depend on which compiler inlined this.
enum { kPartialTranslation = 0, kPartialRotation = 1 };   // = GTG_POSE_PARTIAL_*
constexpr int kPosePartialZ = 9;                          // measurement doubles per factor
GT_HD int pose_partial_rows(int kind, int vtype) { return vtype == 0 ? 3 : kind == kPartialTranslation ? 2 : 1; }
// FORM: 0 translation / Pose3, 1 rotation / Pose3, 2 translation / Pose2, 3 rotation / Pose2
constexpr int pose_partial_form_rows(int form) { return form < 2 ? 3 : form == 2 ? 2 : 1; }
template <int FORM>
GT_HD void pose_partial_residual(const double* x, const double* z, double* r) {
  _Pragma("clang fp contract(off)")
  if (FORM == 0) {
    for (int k = 0; k < 3; k++) r[k] = x[9 + k] - z[k];
  } else if (FORM == 1) {
    double M[9];   // Z^T R (Rot3::between)
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) M[3 * i + j] = z[i] * x[j] + z[3 + i] * x[3 + j] + z[6 + i] * x[6 + j];
    so3_logmap(M, r);
  } else if (FORM == 2) {
    r[0] = x[0] - z[0]; r[1] = x[1] - z[1];
  } else {
    const double c = cos(x[2]), s = sin(x[2]), cz = z[0], sz = -z[1];   // Rot2::inverse of the measurement
    double cc = cz * c - sz * s, ss = sz * c + cz * s;                   // Rot2::operator* (Rot2.h:116-118)
    rot2_normalize(cc, ss);
    r[0] = atan2(ss, cc);
  }
}
template <int FORM>
GT_HD void pose_partial_linearize_form(const double* x, const double* z, const NoiseRef& n, double* J) {
  constexpr int R = pose_partial_form_rows(FORM), D = FORM < 2 ? 6 : 3;
  double r[R];
  pose_partial_residual<FORM>(x, z, r);
  for (int i = 0; i < kPriorRec; i++) J[i] = 0.0;
  if (FORM == 0) { for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) J[6 * i + 3 + k] = x[3 * i + k]; }
  else if (FORM == 1) { for (int i = 0; i < 3; i++) J[6 * i + i] = 1.0; }
  else if (FORM == 2) { const double c = cos(x[2]), s = sin(x[2]); J[0] = c; J[1] = -s; J[3] = s; J[4] = c; }
  else J[2] = 1.0;
  for (int i = 0; i < R; i++) J[81 + i] = -r[i];
  whiten_cols<R>(n.kind, n.data, J, D);
  whiten_cols<R>(n.kind, n.data, J + 81, 1);
  if (n.rkind) {
    const double w = reweight_factor(n, J + 81, R);
    for (int i = 0; i < R * D; i++) J[i] *= w;
    for (int i = 0; i < R; i++) J[81 + i] *= w;
  }
}
GT_HD void pose_partial_linearize(int kind, int vtype, const double* x, const double* z, const NoiseRef& n, double* J) {
  if (vtype == 0) { if (kind == kPartialTranslation) pose_partial_linearize_form<0>(x, z, n, J); else pose_partial_linearize_form<1>(x, z, n, J); }
  else { if (kind == kPartialTranslation) pose_partial_linearize_form<2>(x, z, n, J); else pose_partial_linearize_form<3>(x, z, n, J); }
}
template <int FORM>
GT_HD double pose_partial_error_form(const double* x, const double* z, const NoiseRef& n) {
  constexpr int R = pose_partial_form_rows(FORM);
  double r[R];
  pose_partial_residual<FORM>(x, z, r);
  whiten_cols<R>(n.kind, n.data, r, 1);
  double e = 0.0;
  for (int i = 0; i < R; i++) e += r[i] * r[i];
  return factor_loss(n, e);
}
GT_HD double pose_partial_error(int kind, int vtype, const double* x, const double* z, const NoiseRef& n) {
  if (vtype == 0) return kind == kPartialTranslation ? pose_partial_error_form<0>(x, z, n) : pose_partial_error_form<1>(x, z, n);
  return kind == kPartialTranslation ? pose_partial_error_form<2>(x, z, n) : pose_partial_error_form<3>(x, z, n);
}

// ---- a pose named several times in one smart track (SmartProjectionRigFactor) ------------------------------------
// The reference builds that factor's Hessian on the UNIQUE keys (CameraSet::SchurComplementAndRearrangeBlocks,
// slam/SmartProjectionRigFactor.h:312-322): the sightings o_0 .. o_{n-1} of one track made from one pose are one block row
// F = [F_0; ..; F_{n-1}], and with E_o = F_o^T E_o' L^-T (the E slots) its diagonal block loses (sum_o E_o)(sum_o E_o)^T, not
// sum_o E_o E_o^T.  This is entry (i, j) of the difference, sum_{a<b} (row_i(E_a) . row_j(E_b) + row_i(E_b) . row_j(E_a)): every
// sighting against the running sum of the sightings before it, in list order (no cancellation, one fixed order).
// E: the slots of the range `obs` indexes, `stride` doubles apart, 3 per row.
GT_HD double smart_repeat_cross(const double* E, int stride, const int32_t* obs, int n, int i, int j) {
  double si[3] = {0.0, 0.0, 0.0}, sj[3] = {0.0, 0.0, 0.0}, acc = 0.0;
  if (i < j) { const int t = i; i = j; j = t; }     // (j, i) is computed as (i, j): the same bits on both sides of the diagonal
  for (int a = 0; a < n; a++) {
    const double* e = E + (int64_t)stride * obs[a];
    const double* ei = e + 3 * i; const double* ej = e + 3 * j;
    acc += ei[0] * sj[0] + ei[1] * sj[1] + ei[2] * sj[2] + si[0] * ej[0] + si[1] * ej[1] + si[2] * ej[2];
    for (int k = 0; k < 3; k++) { si[k] += ei[k]; sj[k] += ej[k]; }
  }
  return acc;
}

}  // namespace gt
