// tests/hostmath/hostmath_planar.cpp -- TEST INFRASTRUCTURE ONLY.
// The planar bearing / range evaluators of gtsam_amd/csrc/factors.h (sam2_linearize / sam2_error, GT_HD) compiled for the HOST, one call
// per factor table, with the tables addressed as the device kernels address them (tests/test_planar_hostmath.py).
// noise_data is in the DEVICE's form: inverse sigmas / R (csrc/upload.hip::upload_noise_table).
#include <stdint.h>
#include "../../gtsam_amd/csrc/factors.h"
extern "C" {
int hmpl_record_size(void) { return gt::kPlanarRec; }
int hmpl_rows(int kind) { return gt::sam2_rows(kind); }
// J [n x 21] records, err [n] factor errors
void hmpl_factors(long n, const int32_t* kind, const int32_t* pose, const int32_t* point, const double* z3, const int32_t* nz,
                  const double* values, const int64_t* val_off, const int32_t* nkind, const int64_t* noff, const double* ndata,
                  const int32_t* rkind, const double* rk, double* J, double* err) {
  for (long i = 0; i < n; i++) {
    const int ni = nz[i];
    const gt::NoiseRef nr{nkind[ni], ndata + noff[ni], rkind ? rkind[ni] : 0, rk ? rk[ni] : 0.0};
    const double* x = values + val_off[pose[i]];
    const double* l = values + val_off[point[i]];
    if (J) gt::sam2_linearize(kind[i], x, l, z3 + 3 * i, nr, J + gt::kPlanarRec * i);
    if (err) err[i] = gt::sam2_error(kind[i], x, l, z3 + 3 * i, nr);
  }
}
// one factor with Unit noise: the unwhitened record [H_pose | H_point | Local(h, z)]
void hmpl_unwhitened(int kind, const double* x, const double* l, const double* z3, double* J) {
  gt::sam2_linearize(kind, x, l, z3, gt::NoiseRef{gt::kNoiseUnit, nullptr, 0, 0.0}, J);
}
}
