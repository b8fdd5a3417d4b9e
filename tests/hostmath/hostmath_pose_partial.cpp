// tests/hostmath/hostmath_pose_partial.cpp -- TEST INFRASTRUCTURE ONLY.
// The partial pose prior evaluators of gtsam_amd/csrc/factors.h (pose_partial_linearize / pose_partial_error, GT_HD) compiled for the
// HOST, one call per factor table, with the tables addressed as the device kernels address them (tests/test_pose_partial_hostmath.py).
// noise_data is in the DEVICE's form: inverse sigmas / R (csrc/upload.hip::upload_noise_table).
#include <stdint.h>
#include "../../gtsam_amd/csrc/factors.h"
extern "C" {
int hmpp_record_size(void) { return gt::kPriorRec; }
int hmpp_rows(int kind, int vtype) { return gt::pose_partial_rows(kind, vtype); }
// J [n x 90] records, err [n] factor errors
void hmpp_factors(long n, const int32_t* kind, const int32_t* var, const int32_t* var_type, const double* z9, const int32_t* nz,
                  const double* values, const int64_t* val_off, const int32_t* nkind, const int64_t* noff, const double* ndata,
                  const int32_t* rkind, const double* rk, double* J, double* err) {
  for (long i = 0; i < n; i++) {
    const int ni = nz[i], v = var[i];
    const gt::NoiseRef nr{nkind[ni], ndata + noff[ni], rkind ? rkind[ni] : 0, rk ? rk[ni] : 0.0};
    const double* x = values + val_off[v];
    if (J) gt::pose_partial_linearize(kind[i], var_type[v], x, z9 + 9 * i, nr, J + gt::kPriorRec * i);
    if (err) err[i] = gt::pose_partial_error(kind[i], var_type[v], x, z9 + 9 * i, nr);
  }
}
// one factor with Unit noise: the unwhitened record [H | -r]
void hmpp_unwhitened(int kind, int vtype, const double* x, const double* z9, double* J) {
  gt::pose_partial_linearize(kind, vtype, x, z9, gt::NoiseRef{gt::kNoiseUnit, nullptr, 0, 0.0}, J);
}
}
