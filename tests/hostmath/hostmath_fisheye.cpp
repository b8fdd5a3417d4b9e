// tests/hostmath/hostmath_fisheye.cpp -- TEST INFRASTRUCTURE ONLY.
// The Cal3Fisheye evaluators of gtsam_amd/csrc (geom.h: fisheye_uncalibrate, fisheye_project; factors.h: proj_linearize_fisheye /
// proj_error_fisheye, GT_HD) compiled for the HOST, one call per projection table, with the tables addressed as k_lin_proj_fisheye and
// k_error_proj_fisheye address them: a calib row of model 0 goes through proj_linearize / proj_error (tests/test_fisheye_hostmath.py).
// noise_data is in the DEVICE's form: inverse sigmas / R (csrc/upload.hip::upload_noise_table); calib holds 9 doubles per row.
#include <stdint.h>
#include "../../gtsam_amd/csrc/factors.h"
extern "C" {
int hmfe_record_size(void) { return gt::kProjRec; }
int hmfe_calib_stride(void) { return gt::kCalibStride; }
// J [n x 20] records, err [n] factor errors
void hmfe_factors(long n, const int32_t* pose, const int32_t* point, const double* z2, const int32_t* nz, const int32_t* calib_idx,
                  const int32_t* sensor_idx, const double* calib9, const int32_t* model, const double* sensor, const double* values,
                  const int64_t* val_off, const int32_t* nkind, const int64_t* noff, const double* ndata, const int32_t* rkind,
                  const double* rk, double* J, double* err) {
  for (long i = 0; i < n; i++) {
    const int ni = nz[i], ci = calib_idx[i], si = sensor_idx[i];
    const gt::NoiseRef nr{nkind[ni], ndata + noff[ni], rkind ? rkind[ni] : 0, rk ? rk[ni] : 0.0};
    const double* T = values + val_off[pose[i]];
    const double* l = values + val_off[point[i]];
    const double* K = calib9 + gt::kCalibStride * ci;
    const double* S = si >= 0 ? sensor + 12 * si : nullptr;
    if (model[ci] == 1) {
      if (J) gt::proj_linearize_fisheye(T, K, S, l, z2 + 2 * i, nr, J + gt::kProjRec * i);
      if (err) err[i] = gt::proj_error_fisheye(T, K, S, l, z2 + 2 * i, nr);
    } else {
      if (J) gt::proj_linearize(T, K, S, l, z2 + 2 * i, nr, J + gt::kProjRec * i);
      if (err) err[i] = gt::proj_error(T, K, S, l, z2 + 2 * i, nr);
    }
  }
}
// Cal3Fisheye::uncalibrate of an intrinsic point: pixel [2] and d(pixel)/d(intrinsic point) [2 x 2]
void hmfe_uncalibrate(const double* K9, const double* pn, double* pi, double* D) { gt::fisheye_uncalibrate(K9, pn, pi, D); }
double hmfe_scaling(double r) { return gt::fisheye_scaling(r); }
// PinholePose<Cal3Fisheye>::project of a world point: pixel [2], Dpose [2 x 6], Dpoint [2 x 3]; 0 behind the camera
int hmfe_project(const double* T, const double* K9, const double* pw, double* pi, double* Dpose, double* Dpoint) {
  return gt::fisheye_project(T, K9, pw, pi, Dpose, Dpoint) ? 1 : 0;
}
}
