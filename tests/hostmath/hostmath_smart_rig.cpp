// tests/hostmath/hostmath_smart_rig.cpp -- TEST INFRASTRUCTURE ONLY.
// The arithmetic of k_smart_hdiag_repeats / k_pcg_setup_repeats (SmartProjectionRigFactor: a pose named several times in one track)
// compiled for the HOST: factors.h::smart_repeat_cross exactly as the two kernels call it (tests/test_smart_rig_hostmath.py).
#include <stdint.h>
#include "../../gtsam_amd/csrc/factors.h"
extern "C" {
// entry (i, j) of (sum_a E_a)(sum_a E_a)^T - sum_a E_a E_a^T over the n slots obs[0..n) of E (stride doubles apart, 3 per row)
double hmsr_repeat_cross(const double* E, int stride, const int32_t* obs, int n, int i, int j) {
  return gt::smart_repeat_cross(E, stride, obs, n, i, j);
}
}
