// tests/hostmath/hostmath_stereo.cpp -- TEST INFRASTRUCTURE ONLY.
// The GenericStereoFactor evaluators of gtsam_amd/csrc/factors.h (stereo_linearize / stereo_error, GT_HD) compiled for the HOST, one
// call per factor table, with the tables addressed as the device kernels address them (tests/test_stereo_hostmath.py).
// noise_data is in the DEVICE's form: inverse sigmas / R (csrc/upload.hip::upload_noise_table).
#include <stdint.h>
#include "../../gtsam_amd/csrc/factors.h"
extern "C" {
int hms_record_size(void) { return gt::kStereoRec; }
// J [n x 30] records, err [n] factor errors, resid [n x 3] whitened residuals h(x) - z (before any m-estimator)
void hms_stereo(long n, const int32_t* pose, const int32_t* pt, const double* z, const int32_t* nz, const int32_t* calib_idx,
                const int32_t* sensor_idx, const double* calib5, const double* baseline, const double* sensor, const double* values,
                const int64_t* val_off, const int32_t* nkind, const int64_t* noff, const double* ndata, const int32_t* rkind,
                const double* rk, double* J, double* err, double* resid) {
  for (long i = 0; i < n; i++) {
    const int ni = nz[i], ci = calib_idx[i], si = sensor_idx ? sensor_idx[i] : -1;
    const gt::NoiseRef nr{nkind[ni], ndata + noff[ni], rkind ? rkind[ni] : 0, rk ? rk[ni] : 0.0};
    const double* T = values + val_off[pose[i]];
    const double* p = values + val_off[pt[i]];
    const double* S = si >= 0 ? sensor + 12 * si : nullptr;
    if (J) gt::stereo_linearize(T, calib5 + 5 * ci, baseline[ci], S, p, z + 3 * i, nr, J + gt::kStereoRec * i);
    if (err) err[i] = gt::stereo_error(T, calib5 + 5 * ci, baseline[ci], S, p, z + 3 * i, nr);
    if (resid) gt::stereo_residual(T, calib5 + 5 * ci, baseline[ci], S, p, z + 3 * i, nr, resid + 3 * i);
  }
}
// a monocular factor's record in the three-row layout of a graph with stereo factors
void hms_proj_rows3(const double* pose, const double* K9, const double* sensor, const double* pt, const double* z, int nk, const double* nd, double* J) {
  gt::proj_linearize_rows3(pose, K9, sensor, pt, z, gt::NoiseRef{nk, nd, 0, 0.0}, J);
}
}
