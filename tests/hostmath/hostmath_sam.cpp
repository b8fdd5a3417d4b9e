// tests/hostmath/hostmath_sam.cpp -- TEST INFRASTRUCTURE ONLY.
// The bearing / range evaluators of gtsam_amd/csrc/factors.h (sam_linearize / sam_error / sam_residual, GT_HD) compiled for the HOST, one
// call per factor table, with the tables addressed as the device kernels address them (tests/test_sam_hostmath.py).
// noise_data is in the DEVICE's form: inverse sigmas / R (csrc/upload.hip::upload_noise_table).
#include <stdint.h>
#include "../../gtsam_amd/csrc/factors.h"
extern "C" {
int hmsam_record_size(void) { return gt::kStereoRec; }
// J [n x 30] records, err [n] factor errors, resid [n x 3] whitened residuals -Local(h, z) (before any m-estimator; the places a kind
// does not use are left as they are)
void hmsam_factors(long n, const int32_t* kind, const int32_t* pose, const int32_t* pt, const double* z4, const int32_t* nz, const double* values,
                   const int64_t* val_off, const int32_t* nkind, const int64_t* noff, const double* ndata, const int32_t* rkind, const double* rk,
                   double* J, double* err, double* resid) {
  for (long i = 0; i < n; i++) {
    const int ni = nz[i];
    const gt::NoiseRef nr{nkind[ni], ndata + noff[ni], rkind ? rkind[ni] : 0, rk ? rk[ni] : 0.0};
    const double* T = values + val_off[pose[i]];
    const double* p = values + val_off[pt[i]];
    if (J) gt::sam_linearize(kind[i], T, p, z4 + 4 * i, nr, J + gt::kStereoRec * i);
    if (err) err[i] = gt::sam_error(kind[i], T, p, z4 + 4 * i, nr);
    if (resid) gt::sam_residual(kind[i], T, p, z4 + 4 * i, nr, resid + 3 * i);
  }
}
// one factor with Unit noise: the unwhitened record
void hmsam_unwhitened(int kind, const double* pose, const double* pt, const double* z4, double* J) {
  gt::sam_linearize(kind, pose, pt, z4, gt::NoiseRef{gt::kNoiseUnit, nullptr, 0, 0.0}, J);
}
// h(x): out = predicted direction (3), its basis b1 (3), b2 (3), predicted range (1)
void hmsam_predict(const double* pose, const double* pt, double* out) {
  const double dp[3] = {pt[0] - pose[9], pt[1] - pose[10], pt[2] - pose[11]};
  double q[3], D[3];
  gt::mat3_tvec(pose, dp, q);
  gt::unit3_from_point(q, out, out + 3, out + 6, nullptr);
  out[9] = gt::norm3_with_derivative(q, D);
}
}
