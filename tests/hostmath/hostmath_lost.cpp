// tests/hostmath/hostmath_lost.cpp -- TEST INFRASTRUCTURE ONLY.
// TriangulationParameters::useLOST as the device computes it, compiled for the HOST: geom.h::triangulate_lost and both overloads of
// smart_triangulate exactly as k_smart_triangulate<., true> calls them (tests/test_smart_lost_hostmath.py).  calib9 is the device's
// calibration table (kCalibStride doubles per entry); rows: 8 doubles of work space per measurement.
#include <stdint.h>
#include "../../gtsam_amd/csrc/factors.h"
extern "C" {
int hml_calib_stride(void) { return gt::kCalibStride; }
// the linear triangulation alone, pose-type cameras (measurement k looks through pose variable pose_var[k]): LOST (sigma > 0) or the DLT
int hml_linear_pose(int m, const int32_t* pose_var, const int32_t* calib_idx, const int32_t* sensor_idx, const double* calib9,
                    const double* sensor, const int64_t* val_off, const double* values, const double* z, double rank_tol, double sigma,
                    double* rows, double* point) {
  const gt::PoseCams cs{pose_var, calib_idx, sensor_idx, calib9, sensor, val_off, values};
  return sigma > 0.0 ? gt::triangulate_lost(m, cs, z, sigma, rank_tol, rows, point) : gt::triangulate_dlt(m, cs, z, rank_tol, point);
}
// one pose-type or rig-type track through the whole of triangulateSafe
int hml_triangulate_pose(int m, const int32_t* pose_var, const int32_t* calib_idx, const int32_t* sensor_idx, const double* calib9,
                         const double* sensor, const int64_t* val_off, const double* values, const double* z, double rank_tol,
                         double dist_thr, double outlier_thr, double sigma, double* rows, double* point) {
  const gt::PoseCams cs{pose_var, calib_idx, sensor_idx, calib9, sensor, val_off, values};
  return gt::smart_triangulate(m, cs, z, rank_tol, dist_thr, outlier_thr, point, sigma, rows);
}
// one camera-type track (PinholeCamera<Cal3Bundler> variables)
int hml_triangulate_camera(int m, const int32_t* cams, const int64_t* val_off, const double* values, const double* z, double rank_tol,
                           double dist_thr, double outlier_thr, int enable_epi, double sigma, double* rows, double* point) {
  return gt::smart_triangulate(m, cams, val_off, values, z, rank_tol, dist_thr, outlier_thr, point, enable_epi != 0, sigma, rows);
}
}
