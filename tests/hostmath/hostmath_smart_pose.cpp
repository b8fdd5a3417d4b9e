// tests/hostmath/hostmath_smart_pose.cpp -- TEST INFRASTRUCTURE ONLY.
// The pose forms of the smart factor's device code (SmartProjectionPoseFactor<Cal3_S2>) compiled for the HOST: the triangulation of
// geom.h with the PoseCams accessor, exactly as k_smart_triangulate<true> calls it, and the at-infinity evaluators of factors.h
// (tests/test_smart_pose_hostmath.py).  noise data is in the DEVICE's form: inverse sigma (csrc/upload.hip::upload_noise_table);
// calib9 is the device's calibration table (kCalibStride doubles per entry).
#include <stdint.h>
#include "../../gtsam_amd/csrc/factors.h"
extern "C" {
int hmsp_record_size(void) { return gt::kProjRec; }
int hmsp_calib_stride(void) { return gt::kCalibStride; }
// one track: measurement k looks through pose variable pose_var[k]
int hmsp_triangulate(int m, const int32_t* pose_var, const int32_t* calib_idx, const int32_t* sensor_idx, const double* calib9,
                     const double* sensor, const int64_t* val_off, const double* values, const double* z, double rank_tol, double dist_thr,
                     double outlier_thr, double* point) {
  const gt::PoseCams cs{pose_var, calib_idx, sensor_idx, calib9, sensor, val_off, values};
  return gt::smart_triangulate(m, cs, z, rank_tol, dist_thr, outlier_thr, point);
}
// the composed camera pose of measurement k and the undistorted pixel (the calibrate / uncalibrate round trip)
void hmsp_camera(int k, const int32_t* pose_var, const int32_t* calib_idx, const int32_t* sensor_idx, const double* calib9,
                 const double* sensor, const int64_t* val_off, const double* values, const double* z, double* T, double* zu) {
  const gt::PoseCams cs{pose_var, calib_idx, sensor_idx, calib9, sensor, val_off, values};
  cs.pose(k, T);
  cs.undistort(k, z, zu);
}
void hmsp_backproject_at_infinity(const double* T, const double* K, const double* z, double* dir) { gt::s2_backproject_at_infinity(T, K, z, dir); }
void hmsp_unit3_basis(const double* n, double* b1, double* b2) { gt::unit3_basis(n, b1, b2); }
// record [A1 2x6 | A2 2x3 | b 2], error and whitened residual h - z of one measurement of a track at infinity; 0 = CheiralityException
int hmsp_at_infinity(const double* pose, const double* K9, const double* sensor, const double* dir, const double* z, int nk, const double* nd,
                     double* J, double* err) {
  const gt::NoiseRef nr{nk, nd, 0, 0.0};
  const bool a = gt::proj_linearize_at_infinity(pose, K9, sensor, dir, z, nr, J);
  const bool b = gt::proj_error_at_infinity(pose, K9, sensor, dir, z, nr, err);
  return a && b ? 1 : 0;
}
void hmsp_pose_retract(const double* T, const double* xi, double* out) { gt::pose_retract(T, xi, out); }
}
