// geom.h -- per-factor geometry of the LM hot path, written for one GPU lane per factor.
//
// Device-side re-derivation of exactly the formulas the reference evaluates inside every factor
// (SURVEY.md section 8(a) rows G1, F1-F4, R1); file:line citations are into /root/reference/gtsam.
// Everything is IEEE double, no fast-math, fused multiply-adds left to the compiler's default
// contraction (-ffp-contract=fast-honor-pragmas on hipcc): results agree with the reference to a
// few ulp, not bitwise (tolerances in tests/).
//
// GT_HD lets the same header be compiled by plain g++ for the CPU-side unit parity test of these
// formulas (tests/hostmath/, test infrastructure only -- the product has no CPU path).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GT_HD inline
#endif

namespace gt {

constexpr double kEps = 2.220446049250313e-16;  // std::numeric_limits<double>::epsilon()
constexpr double kPi = 3.14159265358979323846;

// ---- tiny fixed-size helpers (row-major) ------------------------------------------------------
GT_HD void mat3_mul(const double* A, const double* B, double* C) {  // C = A*B
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
GT_HD void mat3_tmul(const double* A, const double* B, double* C) {  // C = A^T * B
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
GT_HD void mat3_vec(const double* A, const double* x, double* y) {
  for (int i = 0; i < 3; i++) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}
GT_HD void mat3_tvec(const double* A, const double* x, double* y) {  // y = A^T x
  _Pragma("clang fp contract(off)")   // bit-reproducible wherever it is inlined: see sfm_linearize (factors.h)
  for (int i = 0; i < 3; i++) y[i] = A[i] * x[0] + A[3 + i] * x[1] + A[6 + i] * x[2];
}
GT_HD void skew3(double x, double y, double z, double* W) {  // skewSymmetric (base/Matrix.h)
  W[0] = 0; W[1] = -z; W[2] = y; W[3] = z; W[4] = 0; W[5] = -x; W[6] = -y; W[7] = x; W[8] = 0;
}

// ---- SO(3) -----------------------------------------------------------------------------------
// SO3::Expmap through so3::ExpmapFunctor (geometry/SO3.cpp:50-88,200-208).
GT_HD void so3_expmap(const double* w, double* R) {
  const double theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double W[9];
  skew3(w[0], w[1], w[2], W);
  if (theta2 <= kEps) {  // nearZero: I + W
    for (int i = 0; i < 9; i++) R[i] = W[i];
    R[0] += 1.0; R[4] += 1.0; R[8] += 1.0;
    return;
  }
  const double theta = sqrt(theta2);
  const double sin_theta = sin(theta);
  const double s2 = sin(theta / 2.0);
  const double one_minus_cos = 2.0 * s2 * s2;
  double K[9], KK[9];
  for (int i = 0; i < 9; i++) K[i] = W[i] / theta;
  mat3_mul(K, K, KK);
  for (int i = 0; i < 9; i++) R[i] = sin_theta * K[i] + one_minus_cos * KK[i];
  R[0] += 1.0; R[4] += 1.0; R[8] += 1.0;
}

// SO3::Logmap (geometry/SO3.cpp:247-323): near-pi branch by largest diagonal, acos branch,
// Taylor branch near the identity -- thresholds 1e-3 and -1e-6 as in the reference.
GT_HD void so3_logmap(const double* R, double* omega) {
  const double R11 = R[0], R12 = R[1], R13 = R[2];
  const double R21 = R[3], R22 = R[4], R23 = R[5];
  const double R31 = R[6], R32 = R[7], R33 = R[8];
  const double tr = R11 + R22 + R33;
  if (tr + 1.0 < 1e-3) {
    // axis a = the largest diagonal entry (ties as in the reference: 3 over 2 over 1), (b, c) the next two cyclically;
    // along a: 2 + 2 R_aa, along b: R_ab + R_ba, along c: R_ac + R_ca, antisymmetric part R_cb - R_bc
    double along_a, along_b, along_c, anti;
    int a;
    if (R33 > R22 && R33 > R11) { a = 2; anti = R21 - R12; along_a = 2.0 + 2.0 * R33; along_b = R31 + R13; along_c = R23 + R32; }
    else if (R22 > R11) { a = 1; anti = R13 - R31; along_a = 2.0 + 2.0 * R22; along_b = R23 + R32; along_c = R12 + R21; }
    else { a = 0; anti = R32 - R23; along_a = 2.0 + 2.0 * R11; along_b = R12 + R21; along_c = R31 + R13; }
    const double inv_root = 1 / sqrt(along_a);
    const double len = sqrt(along_a * along_a + along_b * along_b + along_c * along_c + anti * anti);
    const double sign = anti < 0 ? -1.0 : 1.0;
    const double angle = kPi - (2 * sign * anti) / len;
    const double k = 0.5 * inv_root * angle;
    const double wa = sign * k * along_a, wb = sign * k * along_b, wc = sign * k * along_c;
    if (a == 2) { omega[0] = wb; omega[1] = wc; omega[2] = wa; }
    else if (a == 1) { omega[0] = wc; omega[1] = wa; omega[2] = wb; }
    else { omega[0] = wa; omega[1] = wb; omega[2] = wc; }
  } else {
    double magnitude;
    const double tr_3 = tr - 3.0;
    if (tr_3 < -1e-6) {
      const double theta = acos((tr - 1.0) / 2.0);
      magnitude = theta / (2.0 * sin(theta));
    } else {
      magnitude = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0;
    }
    omega[0] = magnitude * (R32 - R23); omega[1] = magnitude * (R13 - R31); omega[2] = magnitude * (R21 - R12);
  }
}

// ---- SE(3): a pose is 12 doubles, R row-major then t ---------------------------------------
// Pose3::operator* (geometry/Pose3.h:114-116)
GT_HD void pose_compose(const double* A, const double* B, double* C) {
  double R[9], t[3];
  mat3_mul(A, B, R);
  mat3_vec(A, B + 9, t);
  for (int i = 0; i < 9; i++) C[i] = R[i];
  for (int i = 0; i < 3; i++) C[9 + i] = A[9 + i] + t[i];
}
// Pose3::inverse (geometry/Pose3.cpp:49-52)
GT_HD void pose_inverse(const double* A, double* B) {
  double nt[3] = {-A[9], -A[10], -A[11]}, t[3];
  mat3_tvec(A, nt, t);
  double R[9];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * i + j] = A[3 * j + i];
  for (int i = 0; i < 9; i++) B[i] = R[i];
  for (int i = 0; i < 3; i++) B[9 + i] = t[i];
}
// inverse(A) * B without materialising the inverse: LieGroup::between (base/Lie.h:63-69)
GT_HD void pose_between(const double* A, const double* B, double* C) {
  double Ai[12];
  pose_inverse(A, Ai);
  pose_compose(Ai, B, C);
}
// Pose3::AdjointMap (geometry/Pose3.cpp:57-63): [R 0; [t]x R, R], 6x6 row-major
GT_HD void pose_adjoint(const double* T, double* Ad) {
  double S[9], A[9];
  skew3(T[9], T[10], T[11], S);
  mat3_mul(S, T, A);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      Ad[6 * i + j] = T[3 * i + j];
      Ad[6 * i + 3 + j] = 0.0;
      Ad[6 * (3 + i) + j] = A[3 * i + j];
      Ad[6 * (3 + i) + 3 + j] = T[3 * i + j];
    }
}
// Pose3::Expmap (geometry/Pose3.cpp:169-185), xi = [omega; v]
GT_HD void pose_expmap(const double* xi, double* T) {
  const double* w = xi; const double* v = xi + 3;
  so3_expmap(w, T);
  const double theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  if (theta2 > kEps) {
    const double wv = w[0] * v[0] + w[1] * v[1] + w[2] * v[2];
    const double c[3] = {w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0]};
    double Rc[3];
    mat3_vec(T, c, Rc);
    for (int i = 0; i < 3; i++) T[9 + i] = (c[i] - Rc[i] + w[i] * wv) / theta2;
  } else {
    T[9] = v[0]; T[10] = v[1]; T[11] = v[2];
  }
}
// Pose3::Logmap (geometry/Pose3.cpp:188-208)
GT_HD void pose_logmap(const double* T, double* xi) {
  double w[3];
  so3_logmap(T, w);
  const double* Tt = T + 9;
  const double t = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  xi[0] = w[0]; xi[1] = w[1]; xi[2] = w[2];
  if (t < 1e-10) {
    xi[3] = Tt[0]; xi[4] = Tt[1]; xi[5] = Tt[2];
  } else {
    double W[9], WT[3], WWT[3];
    skew3(w[0] / t, w[1] / t, w[2] / t, W);
    const double Tan = tan(0.5 * t);
    mat3_vec(W, Tt, WT);
    mat3_vec(W, WT, WWT);
    const double c = 1 - t / (2. * Tan);
    for (int i = 0; i < 3; i++) xi[3 + i] = Tt[i] - (0.5 * t) * WT[i] + c * WWT[i];
  }
}
// LieGroup::retract = compose(Expmap(xi)) (base/Lie.h:131-133; GTSAM_POSE3_EXPMAP default)
GT_HD void pose_retract(const double* T, const double* xi, double* out) {
  double E[12];
  pose_expmap(xi, E);
  pose_compose(T, E, out);
}
// LieGroup::localCoordinates = Logmap(between(g)) (base/Lie.h:136-138)
GT_HD void pose_local(const double* A, const double* B, double* xi) {
  double C[12];
  pose_between(A, B, C);
  pose_logmap(C, xi);
}

// ---- pinhole projection -----------------------------------------------------------------------
// PinholeBase::project2 (geometry/CalibratedCamera.cpp:116-135) with Pose3::transformTo
// (Pose3.cpp:371-388), Project (:88-94), Dpose (:27-34), Dpoint (:37-46).
// Returns false on a CheiralityException (q.z <= 0, GTSAM_THROW_CHEIRALITY_EXCEPTION default ON).
// Dpose 2x6, Dpoint 2x3 row-major; pass nullptr to skip derivatives.
GT_HD bool project2(const double* T, const double* pw, double* pn, double* Dpose, double* Dpoint) {
  _Pragma("clang fp contract(off)")   // bit-reproducible wherever it is inlined: see sfm_linearize (factors.h)
  const double dx[3] = {pw[0] - T[9], pw[1] - T[10], pw[2] - T[11]};
  double q[3];
  mat3_tvec(T, dx, q);
  if (q[2] <= 0) return false;
  const double d = 1.0 / q[2];
  const double u = q[0] * d, v = q[1] * d;
  pn[0] = u; pn[1] = v;
  if (Dpose) {
    const double uv = u * v, uu = u * u, vv = v * v;
    Dpose[0] = uv; Dpose[1] = -1 - uu; Dpose[2] = v; Dpose[3] = -d; Dpose[4] = 0; Dpose[5] = d * u;
    Dpose[6] = 1 + vv; Dpose[7] = -uv; Dpose[8] = -u; Dpose[9] = 0; Dpose[10] = -d; Dpose[11] = d * v;
  }
  if (Dpoint) {  // Rt(i,j) = R(j,i) = T[3*j+i]
    for (int j = 0; j < 3; j++) {
      Dpoint[j] = (T[3 * j + 0] - u * T[3 * j + 2]) * d;
      Dpoint[3 + j] = (T[3 * j + 1] - v * T[3 * j + 2]) * d;
    }
  }
  return true;
}

// PinholeCamera<Cal3Bundler>::project2 (geometry/PinholeCamera.h:230-248) = PinholeBaseK::_project
// (PinholePose.h:89-109) + Cal3Bundler::uncalibrate (Cal3Bundler.cpp:66-92).
// cam = pose(12), f, k1, k2, u0, v0.  Dcam 2x9 = [Dp*Dpose | Dcal], Dpoint 2x3 (row-major).
GT_HD bool sfm_project(const double* cam, const double* pw, double* pi, double* Dcam, double* Dpoint) {
  _Pragma("clang fp contract(off)")   // bit-reproducible wherever it is inlined: see sfm_linearize (factors.h)
  double pn[2], Dpose[12], Dpt[6];
  // (both derivative buffers or none: a conditionally selected pointer keeps the local arrays in scratch memory on the device)
  const bool want = Dcam || Dpoint;
  if (!(want ? project2(cam, pw, pn, Dpose, Dpt) : project2(cam, pw, pn, nullptr, nullptr))) return false;
  const double f = cam[12], k1 = cam[13], k2 = cam[14], u0 = cam[15], v0 = cam[16];
  const double x = pn[0], y = pn[1];
  const double r = x * x + y * y;
  const double g = 1. + (k1 + k2 * r) * r;
  const double u = g * x, v = g * y;
  pi[0] = u0 + f * u; pi[1] = v0 + f * v;
  if (Dcam || Dpoint) {
    const double a = 2. * (k1 + 2. * k2 * r);
    const double axx = a * x * x, axy = a * x * y, ayy = a * y * y;
    const double Dp[4] = {(g + axx) * f, axy * f, axy * f, (g + ayy) * f};
    if (Dcam) {
      const double rx = r * x, ry = r * y;
      _Pragma("unroll") for (int j = 0; j < 6; j++) {   // (unrolled: Dpose stays in registers instead of scratch memory)
        Dcam[j] = Dp[0] * Dpose[j] + Dp[1] * Dpose[6 + j];
        Dcam[9 + j] = Dp[2] * Dpose[j] + Dp[3] * Dpose[6 + j];
      }
      Dcam[6] = u; Dcam[7] = f * rx; Dcam[8] = f * r * rx;
      Dcam[15] = v; Dcam[16] = f * ry; Dcam[17] = f * r * ry;
    }
    if (Dpoint)
      _Pragma("unroll") for (int j = 0; j < 3; j++) {
        Dpoint[j] = Dp[0] * Dpt[j] + Dp[1] * Dpt[3 + j];
        Dpoint[3 + j] = Dp[2] * Dpt[j] + Dp[3] * Dpt[3 + j];
      }
  }
  return true;
}

// ---- triangulation of a smart factor's landmark (slam/SmartProjectionFactor.h:166-183 -> geometry/triangulation.h:697-752) ----
// Cal3Bundler::calibrate (geometry/Cal3Bundler.cpp:95-128): the intrinsic point of a pixel by the reference's fixed-point
// iteration (at most 10 rounds, stops when uncalibrate(pn) is within tol = 1e-5 pixels -- the same rounds, hence the same point).
// false where the reference throws "fails to converge".
GT_HD bool bundler_calibrate(double f, double k1, double k2, double u0, double v0, const double* pi, double* pn) {
  double px = (pi[0] - u0) / f, py = (pi[1] - v0) / f;
  const double ix = px, iy = py;
  int iteration = 0;
  do {
    const double rr = (px * px) + (py * py);
    const double g = (1 + k1 * rr + k2 * rr * rr);
    pn[0] = ix / g; pn[1] = iy / g;
    const double x = pn[0], y = pn[1], r = x * x + y * y, g2 = 1. + (k1 + k2 * r) * r;
    const double du = (u0 + f * (g2 * x)) - pi[0], dv = (v0 + f * (g2 * y)) - pi[1];
    if (sqrt(du * du + dv * dv) <= 1e-5) break;
    px = pn[0]; py = pn[1];
    iteration++;
  } while (iteration < 10);
  return iteration < 10;
}

// ---- a smart factor's landmark at infinity (slam/SmartProjectionFactor.h:356-371, :419-427) ------------------------------------------
// When the triangulation is not VALID the reference replaces the landmark by the direction of the FIRST measurement seen from the
// FIRST camera, a Unit3 (two degrees of freedom), and projects that into every camera: rotation-only factors.
// Unit3::basis (geometry/Unit3.cpp:73-135): b1 = normalize(n x axis), axis = the coordinate axis of the smallest |n_i| (ties: x, then
// y), b2 = n x b1.
GT_HD void unit3_basis(const double* n, double* b1, double* b2) {
  _Pragma("clang fp contract(off)")   // the bearing factors (sam_linearize, factors.h) project differences of nearly equal vectors on it
  const double mx = fabs(n[0]), my = fabs(n[1]), mz = fabs(n[2]);
  double a[3] = {0.0, 0.0, 0.0};
  if (mx <= my && mx <= mz) a[0] = 1.0; else if (my <= mx && my <= mz) a[1] = 1.0; else a[2] = 1.0;
  const double c[3] = {n[1] * a[2] - n[2] * a[1], n[2] * a[0] - n[0] * a[2], n[0] * a[1] - n[1] * a[0]};
  const double l = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  b1[0] = c[0] / l; b1[1] = c[1] / l; b1[2] = c[2] / l;
  b2[0] = n[1] * b1[2] - n[2] * b1[1]; b2[1] = n[2] * b1[0] - n[0] * b1[2]; b2[2] = n[0] * b1[1] - n[1] * b1[0];
}
// PinholeBaseK::backprojectPointAtInfinity (geometry/PinholePose.h:164-168): Rot3::rotate(Unit3(calibrate(z), 1)); both Unit3
// constructors normalise (Unit3.cpp:36-38, Rot3.cpp:109-116).  false where Cal3Bundler::calibrate throws.
GT_HD bool sfm_backproject_at_infinity(const double* cam, const double* z, double* dir) {
  double pn[2];
  if (!bundler_calibrate(cam[12], cam[13], cam[14], cam[15], cam[16], z, pn)) return false;
  const double l = sqrt(pn[0] * pn[0] + pn[1] * pn[1] + 1.0);
  const double pc[3] = {pn[0] / l, pn[1] / l, 1.0 / l};
  double w[3];
  mat3_vec(cam, pc, w);
  const double lw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  dir[0] = w[0] / lw; dir[1] = w[1] / lw; dir[2] = w[2] / lw;
  return true;
}
// PinholeCamera<Cal3Bundler>::project2(Unit3) (geometry/PinholeCamera.h:251-254 -> PinholePose.h:89-109 ->
// CalibratedCamera.cpp:138-165): q = Unit3(R^T d) (Rot3.cpp:119-126), pn = (q_x, q_y) / q_z, then Cal3Bundler::uncalibrate.
//   Dpose = Duv B_q B_q^T [q]x on the rotation, ZERO on the translation;   Dpoint (2x2) = Duv B_q B_q^T R^T B_d
// with Duv = [1/q_z 0 -u/q_z; 0 1/q_z -v/q_z] and B the tangent bases.  Duv q = 0 and B_q B_q^T = I - q q^T, so the basis of q drops
// out: Dpose = Duv [q]x, Dpoint = Duv R^T B_d.  Dcam 2x9 = [Dp Dpose | Dcal]; Ddir 2x3 = [Dp Dpoint | 0]: the landmark keeps its
// 3-wide slot in the elimination, the third coordinate is not coupled to anything.
// false on a CheiralityException (q_z <= 0, CalibratedCamera.cpp:146-149) -- which the smart factor does NOT catch.
GT_HD bool sfm_project_at_infinity(const double* cam, const double* dir, double* pi, double* Dcam, double* Ddir) {
  double q[3];
  mat3_tvec(cam, dir, q);
  const double lq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  q[0] /= lq; q[1] /= lq; q[2] /= lq;
  if (q[2] <= 0) return false;
  const double d = 1.0 / q[2];
  const double x = q[0] * d, y = q[1] * d;
  const double f = cam[12], k1 = cam[13], k2 = cam[14], u0 = cam[15], v0 = cam[16];
  const double r = x * x + y * y;
  const double g = 1. + (k1 + k2 * r) * r;
  const double u = g * x, v = g * y;
  pi[0] = u0 + f * u; pi[1] = v0 + f * v;
  if (Dcam || Ddir) {
    const double a = 2. * (k1 + 2. * k2 * r);
    const double axx = a * x * x, axy = a * x * y, ayy = a * y * y;
    const double Dp[4] = {(g + axx) * f, axy * f, axy * f, (g + ayy) * f};
    const double Duv[6] = {d, 0.0, -x * d, 0.0, d, -y * d};
    if (Dcam) {
      double S[9];
      skew3(q[0], q[1], q[2], S);
      for (int j = 0; j < 3; j++) {
        const double r0 = Duv[0] * S[j] + Duv[1] * S[3 + j] + Duv[2] * S[6 + j];
        const double r1 = Duv[3] * S[j] + Duv[4] * S[3 + j] + Duv[5] * S[6 + j];
        Dcam[j] = Dp[0] * r0 + Dp[1] * r1; Dcam[9 + j] = Dp[2] * r0 + Dp[3] * r1;
        Dcam[3 + j] = 0.0; Dcam[12 + j] = 0.0;
      }
      const double rx = r * x, ry = r * y;
      Dcam[6] = u; Dcam[7] = f * rx; Dcam[8] = f * r * rx;
      Dcam[15] = v; Dcam[16] = f * ry; Dcam[17] = f * r * ry;
    }
    if (Ddir) {
      double B[2][3];
      unit3_basis(dir, B[0], B[1]);
      for (int j = 0; j < 2; j++) {
        double t[3];
        mat3_tvec(cam, B[j], t);                                       // R^T b_j
        const double r0 = Duv[0] * t[0] + Duv[2] * t[2], r1 = Duv[4] * t[1] + Duv[5] * t[2];
        Ddir[j] = Dp[0] * r0 + Dp[1] * r1; Ddir[3 + j] = Dp[2] * r0 + Dp[3] * r1;
      }
      Ddir[2] = 0.0; Ddir[5] = 0.0;
    }
  }
  return true;
}

// eigen-decomposition of a symmetric 4x4 matrix by cyclic Jacobi rotations: A -> diagonal, V = eigenvectors (columns)
GT_HD void jacobi_eig4(double (&A)[4][4], double (&V)[4][4]) {
  _Pragma("unroll") for (int i = 0; i < 4; i++) _Pragma("unroll") for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; sweep++) {
    double off = 0.0, dia = 0.0;
    _Pragma("unroll") for (int p = 0; p < 4; p++) { dia += A[p][p] * A[p][p]; _Pragma("unroll") for (int q = p + 1; q < 4; q++) off += A[p][q] * A[p][q]; }
    if (off <= 1e-40 * dia || off == 0.0) break;
    _Pragma("unroll") for (int p = 0; p < 3; p++)
      _Pragma("unroll") for (int q = p + 1; q < 4; q++) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        _Pragma("unroll") for (int k = 0; k < 4; k++) {      // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - sn * akq; A[k][q] = sn * akp + c * akq;
        }
        _Pragma("unroll") for (int k = 0; k < 4; k++) {      // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - sn * aqk; A[q][k] = sn * apk + c * aqk;
        }
        _Pragma("unroll") for (int k = 0; k < 4; k++) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - sn * vkq; V[k][q] = sn * vkp + c * vkq;
        }
      }
  }
}

enum { kTriValid = 0, kTriDegenerate = 1, kTriBehindCamera = 2, kTriOutlier = 3, kTriFarPoint = 4, kTriNoConvergence = 5,
       kTriCheiralityThrown = 6,   // enableEPI: the refinement linearised at a point behind a camera -- the reference throws (see triangulate_refine)
       kTriAtInfinity = 16 };   // flag on a failed status: this use of the factor replaces the landmark by a point at infinity

// ---- TriangulationParameters::enableEPI: gtsam::triangulateNonlinear (geometry/triangulation.h:211-221) ------------------------------
// The DLT point refined by the reference's own LevenbergMarquardtOptimizer on one TriangulationFactor per camera
// (slam/TriangulationFactor.h:121-136: h(x) - z through the camera's full projection, unit noise) with the parameters of
// triangulation.cpp:177-195 -- lambdaInitial 1, lambdaFactor 10 (fixed), at most 100 iterations, absoluteErrorTol 1.0, the rest
// defaults (relativeErrorTol 1e-5, lambdaUpperBound 1e5, minModelFidelity 1e-3, identity damping).  The state machine is that of
// LM.cpp:121-308 / NonlinearOptimizer.cpp:62-117 on one 3-dimensional variable; it stops after a step or two (absoluteErrorTol 1.0),
// so the RESULT depends on every accept / reject decision and is reproduced decision by decision.
//   tri_cost: sum over the cameras of |h - z|^2; with `H`: also A^T A (upper triangle: 00 01 02 11 12 22), A^T b with b = z - h.
//   A point behind a camera evaluates to the constant error (2 fx, 2 fx) (PinholeCamera.h:323-325) -- but LINEARISING there is a
//   CheiralityException nothing catches (TriangulationFactor::linearize projects without evaluateError's try / catch, :148-170):
//   returns false.
GT_HD bool tri_cost(int m, const int32_t* cams, const int64_t* val_off, const double* values, const double* z, const double* pt,
                    double* H, double* g, double* sumsq) {
  double f = 0.0;
  if (H) { for (int i = 0; i < 6; i++) H[i] = 0.0; g[0] = g[1] = g[2] = 0.0; }
  for (int k = 0; k < m; k++) {
    const double* c = values + val_off[cams[k]];
    double cam[17], pi[2], Dp[6];
    for (int j = 0; j < 17; j++) cam[j] = c[j];
    const bool front = H ? sfm_project(cam, pt, pi, nullptr, Dp) : sfm_project(cam, pt, pi, nullptr, nullptr);
    if (!front) {
      if (H) return false;
      f += 2.0 * (2.0 * cam[12]) * (2.0 * cam[12]);
      continue;
    }
    const double b0 = z[2 * k] - pi[0], b1 = z[2 * k + 1] - pi[1];
    f += b0 * b0 + b1 * b1;
    if (H) {
      H[0] += Dp[0] * Dp[0] + Dp[3] * Dp[3]; H[1] += Dp[0] * Dp[1] + Dp[3] * Dp[4]; H[2] += Dp[0] * Dp[2] + Dp[3] * Dp[5];
      H[3] += Dp[1] * Dp[1] + Dp[4] * Dp[4]; H[4] += Dp[1] * Dp[2] + Dp[4] * Dp[5]; H[5] += Dp[2] * Dp[2] + Dp[5] * Dp[5];
      g[0] += Dp[0] * b0 + Dp[3] * b1; g[1] += Dp[1] * b0 + Dp[4] * b1; g[2] += Dp[2] * b0 + Dp[5] * b1;
    }
  }
  *sumsq = f;
  return true;
}
// false: the reference throws (see above); the point is refined in place otherwise.
GT_HD bool triangulate_refine(int m, const int32_t* cams, const int64_t* val_off, const double* values, const double* z, double* pt) {
  double H[6], g[3], bb, f;
  tri_cost(m, cams, val_off, values, z, pt, nullptr, nullptr, &f);
  double err = 0.5 * f, lam = 1.0;
  int iterations = 0;
  if (err <= 0.0) return true;                                      // errorTol = 0 (NonlinearOptimizer.cpp:68-74)
  double new_error = err;
  for (;;) {
    const double current_error = new_error;
    if (!tri_cost(m, cams, val_off, values, z, pt, H, g, &bb)) return false;
    for (;;) {                                                      // tryLambda until a step is accepted or the search is given up
      // the one clique of the damped system: Eigen LLT of H + lambda I (choleskyPartial, base/cholesky.cpp:107-158) and its rank test
      // on the exponents of the last two pivots
      const double a00 = H[0] + lam, a11 = H[3] + lam, a22 = H[5] + lam;
      bool ok = a00 > 0.0;
      const double r00 = sqrt(a00), r01 = H[1] / r00, r02 = H[2] / r00;
      const double x11 = a11 - r01 * r01;
      ok = ok && x11 > 0.0;
      const double r11 = sqrt(x11), r12 = (H[4] - r01 * r02) / r11;
      const double x22 = a22 - r02 * r02 - r12 * r12;
      ok = ok && x22 > 0.0;
      const double r22 = sqrt(x22);
      if (ok) { int e2, e1; (void)frexp(r11, &e2); (void)frexp(r22, &e1); ok = e2 - e1 < 12; }
      bool step_ok = false, stop = false;
      double trial[3] = {0.0, 0.0, 0.0}, trial_err = 0.0;
      if (ok) {
        const double y0 = g[0] / r00, y1 = (g[1] - r01 * y0) / r11, y2 = (g[2] - r02 * y0 - r12 * y1) / r22;   // R^T y = g
        const double d2 = y2 / r22, d1 = (y1 - r12 * d2) / r11, d0 = (y0 - r01 * d1 - r02 * d2) / r00;      // R delta = y
        // linear.error(0) = 0.5 |b|^2; linear.error(delta) = 0.5 |A delta - b|^2 = 0.5 (|b|^2 - 2 g.delta + delta^T H delta), undamped
        const double Hd0 = H[0] * d0 + H[1] * d1 + H[2] * d2, Hd1 = H[1] * d0 + H[3] * d1 + H[4] * d2, Hd2 = H[2] * d0 + H[4] * d1 + H[5] * d2;
        const double old_lin = 0.5 * bb, new_lin = 0.5 * (bb - 2.0 * (g[0] * d0 + g[1] * d1 + g[2] * d2) + (d0 * Hd0 + d1 * Hd1 + d2 * Hd2));
        const double lin_change = old_lin - new_lin;
        if (lin_change >= 0) {
          trial[0] = pt[0] + d0; trial[1] = pt[1] + d1; trial[2] = pt[2] + d2;
          double ft;
          tri_cost(m, cams, val_off, values, z, trial, nullptr, nullptr, &ft);
          trial_err = 0.5 * ft;
          const double cost_change = err - trial_err;
          if (lin_change > kEps * old_lin) step_ok = cost_change / lin_change > 1e-3;
          if (fabs(cost_change) < 1e-5 * err) stop = true;
        }
      }
      if (step_ok) {
        lam = lam / 10.0;                                           // decreaseLambda, fixed factor; lambdaLowerBound 0
        pt[0] = trial[0]; pt[1] = trial[1]; pt[2] = trial[2]; err = trial_err;
        iterations++;
        break;
      } else if (!stop) {
        lam *= 10.0;                                                // increaseLambda
        if (lam >= 1e5) break;
      } else {
        break;
      }
    }
    new_error = err;
    // checkConvergence(relativeErrorTol 1e-5, absoluteErrorTol 1.0, errorTol 0) (NonlinearOptimizer.cpp:182-231)
    const double absolute_decrease = current_error - new_error, relative_decrease = absolute_decrease / current_error;
    const bool converged = new_error <= 0.0 || relative_decrease <= 1e-5 || absolute_decrease <= 1.0;
    if (!(iterations < 100 && !converged && current_error - current_error == 0.0)) break;     // (x - x == 0: finite)
  }
  return true;
}

// gtsam::triangulateSafe for PinholeCamera<Cal3Bundler> cameras (triangulation.h:697-752; useLOST = false):
//   undistort every measurement (calibrate with the camera's Cal3Bundler, uncalibrate with its pinhole part, :261-268),
//   DLT on the projection matrices K [R | t]^-1 (triangulation.cpp:27-57: rows x P_3 - P_1, y P_3 - P_2; the right singular vector
//   of the smallest singular value, rank = singular values above rank_tol -- here from the eigen-decomposition of A^T A),
//   rank < 3 -> DEGENERATE, a camera with the point not in front -> BEHIND_CAMERA (:536-541), then per camera the distance
//   threshold (FAR_POINT) and the largest reprojection error against the outlier threshold (OUTLIER).
// One code for both smart factors: the camera model comes in through an accessor.  z = 2 per measurement.
// The cameras of one track as the triangulation sees them -- pose, pinhole K, "undistort this pixel" (DLT), "calibrate this pixel"
// (LOST), "project":
//   BundlerCams  PinholeCamera<Cal3Bundler> variables (17 doubles: pose, f, k1, k2, u0, v0), SmartProjectionFactor<PinholeCamera<Cal3Bundler>>;
//   PoseCams     (behind s2_project) PinholePose<Cal3_S2>(pose * body_P_sensor, K), SmartProjectionPoseFactor<Cal3_S2>.
struct BundlerCams {
  const int32_t* cams; const int64_t* val_off; const double* values;
  static constexpr bool kSkew = false;                            // K = [f 0 u0; 0 f v0; 0 0 1]
  GT_HD const double* cam(int k) const { return values + val_off[cams[k]]; }
  GT_HD void pose(int k, double* T) const { const double* c = cam(k); for (int i = 0; i < 12; i++) T[i] = c[i]; }
  GT_HD void pinhole(int k, double* K) const { const double* c = cam(k); K[0] = c[12]; K[1] = c[12]; K[2] = 0.0; K[3] = c[15]; K[4] = c[16]; }
  // calibrate with the camera's Cal3Bundler, uncalibrate with Cal3_S2(f, f, 0, u0, v0); false: calibrate did not converge
  GT_HD bool undistort(int k, const double* z, double* zu) const {
    const double* c = cam(k);
    const double f = c[12], u0 = c[15], v0 = c[16];
    double pn[2];
    if (!bundler_calibrate(f, c[13], c[14], u0, v0, z, pn)) return false;
    zu[0] = f * pn[0] + u0; zu[1] = f * pn[1] + v0;
    return true;
  }
  // Cal3Bundler::calibrate alone: the intrinsic point of a pixel (calibrateMeasurements, triangulation.h:380-393); false: no convergence
  GT_HD bool calibrate(int k, const double* z, double* pn) const {
    const double* c = cam(k);
    return bundler_calibrate(c[12], c[13], c[14], c[15], c[16], z, pn);
  }
  GT_HD bool project(int k, const double* pw, double* pi) const {
    const double* c = cam(k);
    double cc[17];
    for (int j = 0; j < 17; j++) cc[j] = c[j];
    return sfm_project(cc, pw, pi, nullptr, nullptr);
  }
};

template <class Cams>
GT_HD int triangulate_dlt(int m, const Cams& cs, const double* z, double rank_tol, double* point) {
  point[0] = point[1] = point[2] = 0.0;
  if (m < 2) return kTriDegenerate;
  double M[4][4], V[4][4];
  _Pragma("unroll") for (int i = 0; i < 4; i++) _Pragma("unroll") for (int j = 0; j < 4; j++) M[i][j] = 0.0;
  for (int k = 0; k < m; k++) {
    double c[12], K[5], zu[2];
    cs.pose(k, c); cs.pinhole(k, K);
    if (!cs.undistort(k, z + 2 * k, zu)) return kTriNoConvergence;
    // [R | t]^-1 = [R^T | -R^T t]; P = K [R^T | -R^T t], K = [fx s u0; 0 fy v0; 0 0 1]
    double W[3][4];
    _Pragma("unroll") for (int i = 0; i < 3; i++) {
      W[i][0] = c[0 + i]; W[i][1] = c[3 + i]; W[i][2] = c[6 + i];   // R^T(i, j) = R(j, i)
      W[i][3] = -(c[0 + i] * c[9] + c[3 + i] * c[10] + c[6 + i] * c[11]);
    }
    double r0[4], r1[4];
    _Pragma("unroll") for (int j = 0; j < 4; j++) {
      const double P0 = Cams::kSkew ? K[0] * W[0][j] + K[2] * W[1][j] + K[3] * W[2][j] : K[0] * W[0][j] + K[3] * W[2][j];
      const double P1 = K[1] * W[1][j] + K[4] * W[2][j], P2 = W[2][j];
      r0[j] = zu[0] * P2 - P0; r1[j] = zu[1] * P2 - P1;
    }
    _Pragma("unroll") for (int i = 0; i < 4; i++) _Pragma("unroll") for (int j = 0; j < 4; j++) M[i][j] += r0[i] * r0[j] + r1[i] * r1[j];
  }
  jacobi_eig4(M, V);
  int rank = 0, smallest = 0;
  _Pragma("unroll") for (int j = 0; j < 4; j++) {
    const double sv = sqrt(M[j][j] > 0.0 ? M[j][j] : 0.0);
    if (sv > rank_tol) rank++;
    if (M[j][j] < M[smallest][smallest]) smallest = j;
  }
  if (rank < 3) return kTriDegenerate;
  double v[4] = {0, 0, 0, 0};
  _Pragma("unroll") for (int j = 0; j < 4; j++) if (j == smallest) { v[0] = V[0][j]; v[1] = V[1][j]; v[2] = V[2][j]; v[3] = V[3][j]; }
  point[0] = v[0] / v[3]; point[1] = v[1] / v[3]; point[2] = v[2] / v[3];
  return kTriValid;
}
// ... and the checks behind the linear triangulation (and behind the enableEPI refinement, where there is one)
template <class Cams>
GT_HD int smart_triangulate_checks(int m, const Cams& cs, const double* z, double dist_thr, double outlier_thr, const double* point) {
  for (int k = 0; k < m; k++) {       // triangulatePoint3's cheirality check: every camera first
    double c[12];
    cs.pose(k, c);
    const double dx[3] = {point[0] - c[9], point[1] - c[10], point[2] - c[11]};
    double q[3];
    mat3_tvec(c, dx, q);
    if (!(q[2] > 0)) return kTriBehindCamera;
  }
  double max_err = 0.0;
  for (int k = 0; k < m; k++) {
    if (dist_thr > 0) {
      double c[12];
      cs.pose(k, c);
      const double dx = point[0] - c[9], dy = point[1] - c[10], dz = point[2] - c[11];
      if (sqrt(dx * dx + dy * dy + dz * dz) > dist_thr) return kTriFarPoint;
    }
    if (outlier_thr > 0) {
      double pi[2];
      if (cs.project(k, point, pi)) {
        const double eu = pi[0] - z[2 * k], ev = pi[1] - z[2 * k + 1], e = sqrt(eu * eu + ev * ev);
        max_err = e > max_err ? e : max_err;
      }
    }
  }
  if (outlier_thr > 0 && max_err > outlier_thr) return kTriOutlier;
  return kTriValid;
}
// ---- TriangulationParameters::useLOST: gtsam::triangulateLOST (geometry/triangulation.cpp:86-147) behind triangulatePoint3
// (triangulation.h:500-518) -- Linear Optimal Sine Triangulation.  Per camera i the calibrated measurement z_i = (calibrate(pixel), 1),
// its world direction wZ_i = R_i z_i and a partner j = (i + 1) % m give the weight
//   q_i = |wZ_i x wZ_j| / (sigma |(t_j - t_i) x wZ_j|);
// where a numerator or denominator is exactly 0 (coinciding directions, coinciding centres) the partners (i + k) % m, k = 2 .. m - 1, are
// searched for the first with both > 0, and a track without one is a TriangulationUnderconstrainedException: DEGENERATE.  The two rows
// of camera i are q_i skew(z_i)[0:2, :] R_i^T, the right side those rows times t_i.  The 2m x 3 system is solved as the reference
// solves it: Eigen::ColPivHouseholderQR (Householder reflections, at every step the remaining column of largest norm first) with
// setThreshold(rank_tol), whose rank() counts the pivots |R_kk| > rank_tol * max_k |R_kk| -- a RELATIVE test (the DLT path compares
// singular values with rank_tol itself).  Reproduced on purpose: with the default rankTolerance = 1.0 no pivot exceeds the largest one,
// the rank is 0 and EVERY LOST track is DEGENERATE.  Not through the normal equations: a tolerance of 1e-9 on R is 1e-18 on A^T A, below
// what a double resolves.  The column norms are recomputed at every step where Eigen downdates them (ColPivHouseholderQR.h); the two
// differ in which of two (nearly) equal columns goes first, never in the rank of a matrix whose pivots are away from the threshold.
// `rows`: 8 doubles of work space per measurement (2 rows of [A | b]); there is no per-track array whose size depends on m.
// Contraction is off: the zero tests above are exact in the reference (its cross products of identical vectors cancel to 0.0; a
// contracted multiply-add would leave the rounding error of one product).
template <class Cams>
GT_HD int triangulate_lost(int m, const Cams& cs, const double* z, double sigma, double rank_tol, double* rows, double* point) {
  _Pragma("clang fp contract(off)")
  point[0] = point[1] = point[2] = 0.0;
  if (m < 2) return kTriDegenerate;
  // 1. calibrate every measurement first, as the reference does (a pixel that does not calibrate throws before anything else):
  //    slot k holds wZ_k in [0..2] and the intrinsic point in [4..5] until its rows are written
  for (int k = 0; k < m; k++) {
    double T[12], pn[2];
    cs.pose(k, T);
    if (!cs.calibrate(k, z + 2 * k, pn)) return kTriNoConvergence;
    double* s = rows + 8 * k;
    for (int r = 0; r < 3; r++) s[r] = T[3 * r] * pn[0] + T[3 * r + 1] * pn[1] + T[3 * r + 2] * 1.0;
    s[4] = pn[0]; s[5] = pn[1];
  }
  // 2. the weights q_i, kept in [6]
  for (int i = 0; i < m; i++) {
    double Ti[12];
    cs.pose(i, Ti);
    const double* wi = rows + 8 * i;
    double num = 0.0, den = 0.0;
    bool found = false;
    for (int k = 1; k < m && !found; k++) {
      const int j = (i + k) % m;
      double Tj[12];
      cs.pose(j, Tj);
      const double* wj = rows + 8 * j;
      const double d[3] = {Tj[9] - Ti[9], Tj[10] - Ti[10], Tj[11] - Ti[11]};
      const double a0 = wi[1] * wj[2] - wi[2] * wj[1], a1 = wi[2] * wj[0] - wi[0] * wj[2], a2 = wi[0] * wj[1] - wi[1] * wj[0];
      const double b0 = d[1] * wj[2] - d[2] * wj[1], b1 = d[2] * wj[0] - d[0] * wj[2], b2 = d[0] * wj[1] - d[1] * wj[0];
      num = sqrt(a0 * a0 + a1 * a1 + a2 * a2); den = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
      // the first partner is taken unless one of the two is exactly 0 (a NaN goes through, as in the reference); the others need both > 0
      found = k == 1 ? !(num == 0 || den == 0) : (num > 0 && den > 0);
    }
    if (!found) return kTriDegenerate;
    rows[8 * i + 6] = num / (sigma * den);
  }
  // 3. the rows [q S R^T | q S R^T t], S = skew(z)[0:2, :] = [0 -1 zy; 1 0 -zx]
  for (int i = 0; i < m; i++) {
    double T[12];
    cs.pose(i, T);
    double* s = rows + 8 * i;
    const double zx = s[4], zy = s[5], q = s[6];
    double r0[3], r1[3];
    _Pragma("unroll") for (int c = 0; c < 3; c++) {   // R^T(r, c) = T[3 c + r]
      r0[c] = -q * T[3 * c + 1] + (q * zy) * T[3 * c + 2];
      r1[c] = q * T[3 * c] + (q * -zx) * T[3 * c + 2];
    }
    s[0] = r0[0]; s[1] = r0[1]; s[2] = r0[2]; s[3] = r0[0] * T[9] + r0[1] * T[10] + r0[2] * T[11];
    s[4] = r1[0]; s[5] = r1[1]; s[6] = r1[2]; s[7] = r1[0] * T[9] + r1[1] * T[10] + r1[2] * T[11];
  }
  // 4. ColPivHouseholderQR in place on the n x 4 array [A | b]: row r is rows + 4 r
  const int n = 2 * m;
  int p0 = 0, p1 = 1, p2 = 2;                       // the column of the point that stands in position 0, 1, 2
  double max_pivot = 0.0, threshold_helper = 0.0, diag[3] = {0.0, 0.0, 0.0};
  int nonzero_pivots = 3;
  _Pragma("unroll") for (int k = 0; k < 3; k++) {
    double head[3] = {0.0, 0.0, 0.0}, tail[3] = {0.0, 0.0, 0.0};
    for (int r = k; r < n; r++)
      _Pragma("unroll") for (int c = k; c < 3; c++) { const double v = rows[4 * r + c]; if (r == k) head[c] = v * v; else tail[c] += v * v; }
    int piv = k;
    double biggest = head[k] + tail[k];
    _Pragma("unroll") for (int c = k + 1; c < 3; c++) if (head[c] + tail[c] > biggest) { biggest = head[c] + tail[c]; piv = c; }
    if (k == 0) { const double e = sqrt(biggest) * kEps / n; threshold_helper = e * e; }
    if (nonzero_pivots == 3 && biggest < threshold_helper * (n - k)) nonzero_pivots = k;
    if (piv != k) {
      for (int r = 0; r < n; r++) { const double v = rows[4 * r + k]; rows[4 * r + k] = rows[4 * r + piv]; rows[4 * r + piv] = v; }
      if (k == 0) { const int t = p0; if (piv == 1) { p0 = p1; p1 = t; } else { p0 = p2; p2 = t; } }
      else { const int t = p1; p1 = p2; p2 = t; }
    }
    // makeHouseholderInPlace on rows k .. n-1 of column k (Householder.h): the essential part stays below the diagonal
    const double c0 = rows[4 * k + k];
    double tail_sq = 0.0;
    for (int r = k + 1; r < n; r++) tail_sq += rows[4 * r + k] * rows[4 * r + k];
    double tau = 0.0, beta = c0;
    if (tail_sq <= 2.2250738585072014e-308) {
      for (int r = k + 1; r < n; r++) rows[4 * r + k] = 0.0;
    } else {
      beta = sqrt(c0 * c0 + tail_sq);
      if (c0 >= 0) beta = -beta;
      const double dn = c0 - beta;
      for (int r = k + 1; r < n; r++) rows[4 * r + k] /= dn;
      tau = (beta - c0) / beta;
    }
    rows[4 * k + k] = beta;
    diag[k] = fabs(beta);
    if (diag[k] > max_pivot) max_pivot = diag[k];
    // applyHouseholderOnTheLeft to the remaining columns and to b
    double tmp[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = k + 1; r < n; r++) {
      const double e = rows[4 * r + k];
      _Pragma("unroll") for (int c = k + 1; c < 4; c++) tmp[c] += e * rows[4 * r + c];
    }
    _Pragma("unroll") for (int c = k + 1; c < 4; c++) { tmp[c] += rows[4 * k + c]; rows[4 * k + c] -= tau * tmp[c]; }
    for (int r = k + 1; r < n; r++) {
      const double te = tau * rows[4 * r + k];
      _Pragma("unroll") for (int c = k + 1; c < 4; c++) rows[4 * r + c] -= te * tmp[c];
    }
  }
  int rank = 0;
  _Pragma("unroll") for (int k = 0; k < 3; k++) if (k < nonzero_pivots && diag[k] > rank_tol * max_pivot) rank++;
  if (rank < 3) return kTriDegenerate;
  // R x = Q^T b, then the permutation back
  const double x2 = rows[4 * 2 + 3] / rows[4 * 2 + 2];
  const double x1 = (rows[4 * 1 + 3] - rows[4 * 1 + 2] * x2) / rows[4 * 1 + 1];
  const double x0 = (rows[3] - rows[1] * x1 - rows[2] * x2) / rows[0];
  _Pragma("unroll") for (int e = 0; e < 3; e++) point[e] = p0 == e ? x0 : (p1 == e ? x1 : x2);
  return kTriValid;
}
// lost_sigma > 0: LOST with that sigma (lost_rows: its work space), else the DLT
template <class Cams>
GT_HD int smart_triangulate(int m, const Cams& cs, const double* z, double rank_tol, double dist_thr, double outlier_thr, double* point,
                            double lost_sigma = 0.0, double* lost_rows = nullptr) {
  const int st = lost_sigma > 0.0 ? triangulate_lost(m, cs, z, lost_sigma, rank_tol, lost_rows, point) : triangulate_dlt(m, cs, z, rank_tol, point);
  return st != kTriValid ? st : smart_triangulate_checks(m, cs, z, dist_thr, outlier_thr, point);
}
// PinholeCamera<Cal3Bundler> cameras: cams[k] -> values + val_off[cams[k]]; enable_epi: the linear point refined (triangulate_refine)
GT_HD int smart_triangulate(int m, const int32_t* cams, const int64_t* val_off, const double* values, const double* z,
                            double rank_tol, double dist_thr, double outlier_thr, double* point, bool enable_epi = false,
                            double lost_sigma = 0.0, double* lost_rows = nullptr) {
  const BundlerCams cs{cams, val_off, values};
  const int st = lost_sigma > 0.0 ? triangulate_lost(m, cs, z, lost_sigma, rank_tol, lost_rows, point) : triangulate_dlt(m, cs, z, rank_tol, point);
  if (st != kTriValid) return st;
  if (enable_epi && !triangulate_refine(m, cams, val_off, values, z, point)) return kTriCheiralityThrown;   // (triangulation.h:531-534)
  return smart_triangulate_checks(m, cs, z, dist_thr, outlier_thr, point);
}

// PinholeCamera<Cal3_S2>(pose, K).project (PinholePose.h:89-109) + Cal3_S2::uncalibrate (geometry/Cal3_S2.cpp:44-50), or, when the
// table entry carries distortion coefficients, + Cal3DS2_Base::uncalibrate (geometry/Cal3DS2_Base.cpp:93-132, derivative with
// respect to the intrinsic point D2dintrinsic :71-91).  K = fx, fy, s, u0, v0, k1, k2, p1, p2 (kCalibStride).  Dpose 2x6, Dpoint 2x3.
constexpr int kCalibStride = 9;
GT_HD bool s2_project(const double* T, const double* K, const double* pw, double* pi, double* Dpose,
                      double* Dpoint) {
  double pn[2], Dps[12], Dpt[6];
  const bool want = Dpose || Dpoint;
  if (!(want ? project2(T, pw, pn, Dps, Dpt) : project2(T, pw, pn, nullptr, nullptr))) return false;
  const double fx = K[0], fy = K[1], s = K[2], u0 = K[3], v0 = K[4];
  const double k1 = K[5], k2 = K[6], p1 = K[7], p2 = K[8];
  // d(pixel)/d(intrinsic point): DK for a Cal3_S2, DK * DR with distortion
  double d00 = fx, d01 = s, d10 = 0.0, d11 = fy;
  if (k1 == 0.0 && k2 == 0.0 && p1 == 0.0 && p2 == 0.0) {
    pi[0] = fx * pn[0] + s * pn[1] + u0;
    pi[1] = fy * pn[1] + v0;
  } else {
    const double x = pn[0], y = pn[1], xy = x * y, xx = x * x, yy = y * y;
    const double rr = xx + yy, r4 = rr * rr;
    const double g = 1. + k1 * rr + k2 * r4;
    const double dx = 2. * p1 * xy + p2 * (rr + 2. * xx);
    const double dy = 2. * p2 * xy + p1 * (rr + 2. * yy);
    const double pnx = g * x + dx, pny = g * y + dy;
    pi[0] = fx * pnx + s * pny + u0;
    pi[1] = fy * pny + v0;
    if (want) {
      const double drdx = 2. * x, drdy = 2. * y;
      const double dgdx = k1 * drdx + k2 * 2. * rr * drdx, dgdy = k1 * drdy + k2 * 2. * rr * drdy;
      const double dDxdx = 2. * p1 * y + p2 * (drdx + 4. * x), dDxdy = 2. * p1 * x + p2 * drdy;
      const double dDydx = 2. * p2 * y + p1 * drdx, dDydy = 2. * p2 * x + p1 * (drdy + 4. * y);
      const double r00 = g + x * dgdx + dDxdx, r01 = x * dgdy + dDxdy, r10 = y * dgdx + dDydx, r11 = g + y * dgdy + dDydy;
      d00 = fx * r00 + s * r10; d01 = fx * r01 + s * r11;
      d10 = 0.0 * r00 + fy * r10; d11 = 0.0 * r01 + fy * r11;
    }
  }
  if (Dpose)
    _Pragma("unroll") for (int j = 0; j < 6; j++) {
      Dpose[j] = d00 * Dps[j] + d01 * Dps[6 + j];
      Dpose[6 + j] = d10 * Dps[j] + d11 * Dps[6 + j];
    }
  if (Dpoint)
    _Pragma("unroll") for (int j = 0; j < 3; j++) {
      Dpoint[j] = d00 * Dpt[j] + d01 * Dpt[3 + j];
      Dpoint[3 + j] = d10 * Dpt[j] + d11 * Dpt[3 + j];
    }
  return true;
}

// ---- Cal3Fisheye: the equidistant (OpenCV fisheye / Kannala-Brandt) model ---------------------------------------------------------
// Cal3Fisheye::Scaling (geometry/Cal3Fisheye.cpp:35-44): atan(r) / r, by its Taylor series 1 - r^2/3 + r^4/5 for |r| <= 1e-8.
GT_HD double fisheye_scaling(double r) {
  if (r > 1e-8 || r < -1e-8) return atan(r) / r;
  const double r2 = r * r, r4 = r2 * r2;
  return 1.0 - r2 / 3 + r4 / 5;
}
// Cal3Fisheye::uncalibrate (geometry/Cal3Fisheye.cpp:47-108).  K = fx, fy, s, u0, v0, k1, k2, k3, k4 (kCalibStride); pn the intrinsic
// point.  D (or nullptr): d(pixel)/d(intrinsic point) 2x2 row-major -- DK alone when r^2 == 0 exactly (:79-80), else DK * DR (:82-103).
GT_HD void fisheye_uncalibrate(const double* K, const double* pn, double* pi, double* D) {
  const double fx = K[0], fy = K[1], sk = K[2], u0 = K[3], v0 = K[4];
  const double k1 = K[5], k2 = K[6], k3 = K[7], k4 = K[8];
  const double xi = pn[0], yi = pn[1], zi = 1;
  const double r2 = xi * xi + yi * yi, r = sqrt(r2);
  const double t = atan2(r, zi);
  const double t2 = t * t, t4 = t2 * t2, t6 = t2 * t4, t8 = t4 * t4;
  const double scaling = fisheye_scaling(r);
  const double s = scaling * (1 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8);   // K.dot(T) (:53-57), summed left to right as Eigen's 5-vector dot does
  const double xd = s * xi, yd = s * yi;
  pi[0] = fx * xd + sk * yd + u0;
  pi[1] = fy * yd + v0;
  if (!D) return;
  if (r2 == 0) {
    D[0] = fx; D[1] = sk; D[2] = 0.0; D[3] = fy;
    return;
  }
  const double dtd_dt = 1 + 3 * k1 * t2 + 5 * k2 * t4 + 7 * k3 * t6 + 9 * k4 * t8;
  const double R2 = r2 + zi * zi;
  const double dt_dr = zi / R2;
  const double rinv = 1 / r;
  const double dr_dxi = xi * rinv, dr_dyi = yi * rinv;
  const double dtd_dr = dtd_dt * dt_dr;
  const double c2 = dr_dxi * dr_dxi, s2 = dr_dyi * dr_dyi, cs = dr_dxi * dr_dyi;
  const double dxd_dxi = dtd_dr * c2 + s * (1 - c2);
  const double dxd_dyi = (dtd_dr - s) * cs;
  const double dyd_dxi = dxd_dyi;
  const double dyd_dyi = dtd_dr * s2 + s * (1 - s2);
  D[0] = fx * dxd_dxi + sk * dyd_dxi; D[1] = fx * dxd_dyi + sk * dyd_dyi;   // DK * DR, DK = [fx s; 0 fy] (the zero entry's products included, as Eigen forms them)
  D[2] = 0.0 * dxd_dxi + fy * dyd_dxi; D[3] = 0.0 * dxd_dyi + fy * dyd_dyi;
}
// PinholePose<Cal3Fisheye>(pose, K).project (PinholePose.h:89-109): project2 as it is, then the above, chained into Dpose 2x6 and
// Dpoint 2x3 (both or none).  false on a CheiralityException.
GT_HD bool fisheye_project(const double* T, const double* K, const double* pw, double* pi, double* Dpose, double* Dpoint) {
  double pn[2], Dps[12], Dpt[6], D[4];
  const bool want = Dpose || Dpoint;
  if (!(want ? project2(T, pw, pn, Dps, Dpt) : project2(T, pw, pn, nullptr, nullptr))) return false;
  if (!want) { fisheye_uncalibrate(K, pn, pi, nullptr); return true; }
  fisheye_uncalibrate(K, pn, pi, D);
  if (Dpose)
    _Pragma("unroll") for (int j = 0; j < 6; j++) {
      Dpose[j] = D[0] * Dps[j] + D[1] * Dps[6 + j];
      Dpose[6 + j] = D[2] * Dps[j] + D[3] * Dps[6 + j];
    }
  if (Dpoint)
    _Pragma("unroll") for (int j = 0; j < 3; j++) {
      Dpoint[j] = D[0] * Dpt[j] + D[1] * Dpt[3 + j];
      Dpoint[3 + j] = D[2] * Dpt[j] + D[3] * Dpt[3 + j];
    }
  return true;
}

// ---- SmartProjectionPoseFactor<Cal3_S2>: cameras PinholePose<Cal3_S2>(pose * body_P_sensor, K) (slam/SmartProjectionPoseFactor.h:138-147) ----
// Cal3_S2::calibrate (geometry/Cal3_S2.cpp:53-69) and ::uncalibrate (:44-50); K = fx, fy, s, u0, v0
GT_HD void s2_calibrate(const double* K, const double* pi, double* pn) {
  const double delta_u = pi[0] - K[3], delta_v = pi[1] - K[4];
  const double inv_fx = 1 / K[0], inv_fy = 1 / K[1];
  const double inv_fy_delta_v = inv_fy * delta_v;
  pn[0] = inv_fx * (delta_u - K[2] * inv_fy_delta_v); pn[1] = inv_fy_delta_v;
}
GT_HD void s2_uncalibrate(const double* K, const double* pn, double* pi) {
  pi[0] = K[0] * pn[0] + K[2] * pn[1] + K[3];
  pi[1] = K[1] * pn[1] + K[4];
}
// The cameras of one pose-type track: measurement k looks through pose variable pose_var[k], calibration calib_idx[k], sensor
// sensor_idx[k] (or -1).  "The camera's pose" is the composed world_P_sensor everywhere (cache, DLT, cheirality, distance).
// CameraSet<PinholePose<Cal3_S2>> does not hit the "do nothing" specialisations of undistortMeasurements (triangulation.h:297-302,
// :332-338 are for PinholeCamera<Cal3_S2>): every pixel goes through calibrate and uncalibrate of the same K (:315-330 -> :260-268),
// which is not the identity in floating point.  There is no "did not converge" for a Cal3_S2.
struct PoseCams {
  const int32_t *pose_var, *calib_idx, *sensor_idx; const double *calib, *sensor; const int64_t* val_off; const double* values;
  static constexpr bool kSkew = true;
  GT_HD void pose(int k, double* T) const {
    const double* p = values + val_off[pose_var[k]];
    const int si = sensor_idx[k];
    if (si >= 0) pose_compose(p, sensor + 12 * si, T);
    else for (int i = 0; i < 12; i++) T[i] = p[i];
  }
  GT_HD void pinhole(int k, double* K) const { const double* c = calib + kCalibStride * calib_idx[k]; for (int i = 0; i < 5; i++) K[i] = c[i]; }
  GT_HD bool undistort(int k, const double* z, double* zu) const {
    double K[5], pn[2];
    pinhole(k, K);
    s2_calibrate(K, z, pn);
    s2_uncalibrate(K, pn, zu);
    return true;
  }
  // Cal3_S2::calibrate alone (calibrateMeasurements, triangulation.h:380-393): no round trip through uncalibrate
  GT_HD bool calibrate(int k, const double* z, double* pn) const {
    double K[5];
    pinhole(k, K);
    s2_calibrate(K, z, pn);
    return true;
  }
  GT_HD bool project(int k, const double* pw, double* pi) const {
    double T[12], K[kCalibStride];
    pose(k, T);
    const double* c = calib + kCalibStride * calib_idx[k];
    for (int i = 0; i < kCalibStride; i++) K[i] = c[i];
    return s2_project(T, K, pw, pi, nullptr, nullptr);
  }
};
// PinholeBaseK::backprojectPointAtInfinity (PinholePose.h:164-168) with Cal3_S2::calibrate: T = the composed camera pose
GT_HD void s2_backproject_at_infinity(const double* T, const double* K, const double* z, double* dir) {
  double pn[2];
  s2_calibrate(K, z, pn);
  const double l = sqrt(pn[0] * pn[0] + pn[1] * pn[1] + 1.0);
  const double pc[3] = {pn[0] / l, pn[1] / l, 1.0 / l};
  double w[3];
  mat3_vec(T, pc, w);
  const double lw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  dir[0] = w[0] / lw; dir[1] = w[1] / lw; dir[2] = w[2] / lw;
}
// PinholePose<Cal3_S2>::project2(Unit3) (CalibratedCamera.cpp:138-165, then Cal3_S2::uncalibrate): as sfm_project_at_infinity with
// Dcal = [fx s; 0 fy].  Dpose 2x6 = [Dcal Duv [q]x | 0] (zero on the translation), Ddir 2x3 = [Dcal Duv R^T B_d | 0].
// false on a CheiralityException (q_z <= 0).
GT_HD bool s2_project_at_infinity(const double* T, const double* K, const double* dir, double* pi, double* Dpose, double* Ddir) {
  double q[3];
  mat3_tvec(T, dir, q);
  const double lq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  q[0] /= lq; q[1] /= lq; q[2] /= lq;
  if (q[2] <= 0) return false;
  const double d = 1.0 / q[2];
  const double pn[2] = {q[0] * d, q[1] * d};
  s2_uncalibrate(K, pn, pi);
  if (Dpose || Ddir) {
    const double fx = K[0], fy = K[1], s = K[2];
    const double Duv[6] = {d, 0.0, -pn[0] * d, 0.0, d, -pn[1] * d};
    if (Dpose) {
      double S[9];
      skew3(q[0], q[1], q[2], S);
      for (int j = 0; j < 3; j++) {
        const double r0 = Duv[0] * S[j] + Duv[1] * S[3 + j] + Duv[2] * S[6 + j];
        const double r1 = Duv[3] * S[j] + Duv[4] * S[3 + j] + Duv[5] * S[6 + j];
        Dpose[j] = fx * r0 + s * r1; Dpose[6 + j] = fy * r1;
        Dpose[3 + j] = 0.0; Dpose[9 + j] = 0.0;
      }
    }
    if (Ddir) {
      double B[2][3];
      unit3_basis(dir, B[0], B[1]);
      for (int j = 0; j < 2; j++) {
        double t[3];
        mat3_tvec(T, B[j], t);                                         // R^T b_j
        const double r0 = Duv[0] * t[0] + Duv[2] * t[2], r1 = Duv[4] * t[1] + Duv[5] * t[2];
        Ddir[j] = fx * r0 + s * r1; Ddir[3 + j] = fy * r1;
      }
      Ddir[2] = 0.0; Ddir[5] = 0.0;
    }
  }
  return true;
}

// StereoCamera::project2 (geometry/StereoCamera.cpp:37-79) with a Cal3_S2Stereo: K = fx, fy, s, u0, v0 as in the calib table and the
// baseline b.  The skew is stored and NOT used, as in the reference.  pi = (uL, uR, v); Dpose 3x6, Dpoint 3x3 row-major.
// Returns false on a StereoCheiralityException (q.z <= 0).
GT_HD bool stereo_project(const double* T, const double* K, double b, const double* pw, double* pi, double* Dpose,
                          double* Dpoint) {
  _Pragma("clang fp contract(off)")   // the host compile of the CPU parity test and the device then round alike
  const double dp[3] = {pw[0] - T[9], pw[1] - T[10], pw[2] - T[11]};
  double q[3];
  mat3_tvec(T, dp, q);
  if (q[2] <= 0) return false;
  const double fx = K[0], fy = K[1];
  const double d = 1.0 / q[2];
  const double x = q[0], y = q[1];
  const double dfx = d * fx, dfy = d * fy;
  const double uL = dfx * x, uR = dfx * (x - b), v = dfy * y;
  if (Dpose) {
    const double v1 = v / fy, v2 = fx * v1, dx = d * x;
    Dpose[0] = uL * v1; Dpose[1] = -fx - dx * uL; Dpose[2] = v2; Dpose[3] = -dfx; Dpose[4] = 0.0; Dpose[5] = d * uL;
    Dpose[6] = uR * v1; Dpose[7] = -fx - dx * uR; Dpose[8] = v2; Dpose[9] = -dfx; Dpose[10] = 0.0; Dpose[11] = d * uR;
    Dpose[12] = fy + v * v1; Dpose[13] = -dx * v; Dpose[14] = -x * dfy; Dpose[15] = 0.0; Dpose[16] = -dfy; Dpose[17] = d * v;
  }
  if (Dpoint) {  // R(j, c) = T[3 j + c]
    for (int j = 0; j < 3; j++) {
      Dpoint[j] = d * (fx * T[3 * j + 0] - T[3 * j + 2] * uL);
      Dpoint[3 + j] = d * (fx * T[3 * j + 0] - T[3 * j + 2] * uR);
      Dpoint[6 + j] = d * (fy * T[3 * j + 1] - T[3 * j + 2] * v);
    }
  }
  pi[0] = K[3] + uL; pi[1] = K[3] + uR; pi[2] = K[4] + v;
  return true;
}

// ---- bearing and range of a Point3 seen from a Pose3 (gtsam/sam factors) ------------------------
// Contraction is off in all of them: q - x p and 1 - x^2 below cancel, and a multiply-add contracted in one kernel and not in
// another (or not in the host compile of the CPU parity test) moves what is left by many ulps.
// One row of a chain rule through Pose3::transformTo (geometry/Pose3.cpp:371-388): a (1x3, the derivative of a scalar by the local
// point q) times D_local_pose = [[q]x | -I] and times D_local_point = R^T.
GT_HD void local_chain_row(const double* T, const double* q, const double* a, double* Hpose, double* Hpoint) {
  _Pragma("clang fp contract(off)")
  Hpose[0] = a[1] * q[2] - a[2] * q[1]; Hpose[1] = a[2] * q[0] - a[0] * q[2]; Hpose[2] = a[0] * q[1] - a[1] * q[0];
  Hpose[3] = -a[0]; Hpose[4] = -a[1]; Hpose[5] = -a[2];
  for (int j = 0; j < 3; j++) Hpoint[j] = a[0] * T[3 * j] + a[1] * T[3 * j + 1] + a[2] * T[3 * j + 2];
}
// Pose3::range's norm3 (geometry/Point3.cpp:41-50): r and its derivative by q, which falls back to (1, 1, 1) when r <= 1e-10
GT_HD double norm3_with_derivative(const double* q, double* D) {
  _Pragma("clang fp contract(off)")
  const double r = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  if (fabs(r) > 1e-10) { D[0] = q[0] / r; D[1] = q[1] / r; D[2] = q[2] / r; }
  else { D[0] = 1.0; D[1] = 1.0; D[2] = 1.0; }
  return r;
}
// Unit3::FromPoint3 (geometry/Unit3.cpp:44-52): h = normalize(q), its basis, and D 2x3 = basis^T * normalize's derivative
// (Point3.cpp:52-62); D may be null
GT_HD void unit3_from_point(const double* q, double* h, double* b1, double* b2, double* D) {
  _Pragma("clang fp contract(off)")
  const double x2 = q[0] * q[0], y2 = q[1] * q[1], z2 = q[2] * q[2];
  const double nrm = sqrt(x2 + y2 + z2);
  h[0] = q[0] / nrm; h[1] = q[1] / nrm; h[2] = q[2] / nrm;
  unit3_basis(h, b1, b2);
  if (!D) return;
  const double xy = q[0] * q[1], xz = q[0] * q[2], yz = q[1] * q[2];
  const double den = pow(x2 + y2 + z2, 1.5);
  const double N[9] = {(y2 + z2) / den, -xy / den, -xz / den, -xy / den, (x2 + z2) / den, -yz / den, -xz / den, -yz / den, (x2 + y2) / den};
  for (int j = 0; j < 3; j++) {
    D[j] = b1[0] * N[j] + b1[1] * N[3 + j] + b1[2] * N[6 + j];
    D[3 + j] = b2[0] * N[j] + b2[1] * N[3 + j] + b2[2] * N[6 + j];
  }
}
// Unit3::localCoordinates (geometry/Unit3.cpp:285-303): the tangent vector at p (basis b1, b2 of p) that points to q.  Three branches:
// the general one, the first-order form at x = 1, and the constant (pi, 0) at x = -1.
GT_HD void unit3_local(const double* p, const double* b1, const double* b2, const double* q, double* v) {
  _Pragma("clang fp contract(off)")
  const double x = p[0] * q[0] + p[1] * q[1] + p[2] * q[2];
  const double x2 = x * x;
  const double z = 1 - x2;
  double y;
  if (z < 2.220446049250313e-16) {   // std::numeric_limits<double>::epsilon()
    if (x > 0) y = 1.0 - (x - 1.0) / 3.0;
    else { v[0] = 3.14159265358979323846; v[1] = 0.0; return; }
  } else {
    y = acos(x) / sqrt(z);
  }
  const double d[3] = {q[0] - x * p[0], q[1] - x * p[1], q[2] - x * p[2]};
  v[0] = (b1[0] * y) * d[0] + (b1[1] * y) * d[1] + (b1[2] * y) * d[2];
  v[1] = (b2[0] * y) * d[0] + (b2[1] * y) * d[1] + (b2[2] * y) * d[2];
}

// ---- noise models (linear/NoiseModel.cpp) ------------------------------------------------------
enum { kNoiseUnit = 0, kNoiseIsotropic = 1, kNoiseDiagonal = 2, kNoiseGaussian = 3 };
// Device noise table entry data: ISOTROPIC {invsigma}; DIAGONAL invsigmas[dim]; GAUSSIAN R row-major.
// whiten a column vector / the columns of a row-major m x n matrix in place:
//   Unit no-op; Isotropic v*invsigma (:641-663); Diagonal v.*invsigmas (:311-325); Gaussian R*v (:163-181)
template <int M>
GT_HD void whiten_cols(int kind, const double* nd, double* A, int ncols) {
  _Pragma("clang fp contract(off)")   // bit-reproducible wherever it is inlined: see sfm_linearize (factors.h)
  if (kind == kNoiseUnit) return;
  if (kind == kNoiseIsotropic) {
    const double s = nd[0];
    for (int i = 0; i < M * ncols; i++) A[i] *= s;
  } else if (kind == kNoiseDiagonal) {
    for (int r = 0; r < M; r++) for (int c = 0; c < ncols; c++) A[r * ncols + c] *= nd[r];
  } else {
    for (int c = 0; c < ncols; c++) {
      double col[M];
      for (int r = 0; r < M; r++) col[r] = A[r * ncols + c];
      for (int r = 0; r < M; r++) {
        double acc = 0.0;
        for (int k = 0; k < M; k++) acc += nd[r * M + k] * col[k];
        A[r * ncols + c] = acc;
      }
    }
  }
}

// ---- Pose2 (geometry/Pose2.{h,cpp}, Rot2.{h,cpp}) --------------------------------------------------------------
// Stored as (x, y, theta); the reference keeps (c, s) instead of theta and multiplies rotations as complex numbers
// (Rot2.h:116-118: fromCosSin(c1 c2 - s1 s2, s1 c2 + c1 s2), re-normalised only when |c^2+s^2-1| > 1e-10,
// Rot2.cpp:56-64); theta() = atan2(s, c) (Rot2.h:186-188).  h = a^-1 b with
//   a^-1 = (R_a^T, R_a^T (-t_a))                       Pose2.cpp:201-203
//   p q  = (R_p R_q, t_p + R_p t_q)                    Pose2.h:131-133
// returned as (x, y, c, s).
GT_HD void rot2_normalize(double& c, double& s) {
  double scale = c * c + s * s;
  if (fabs(scale - 1.0) > 1e-10) { scale = 1.0 / sqrt(scale); c *= scale; s *= scale; }
}
GT_HD void pose2_between_cs(double xa, double ya, double ca, double sa, double xb, double yb, double cb, double sb,
                            double* h) {
  // inverse of a: rotation (ca, -sa), translation unrotate(-t_a)
  const double ix = ca * (-xa) + sa * (-ya), iy = -sa * (-xa) + ca * (-ya);
  double c = ca * cb - (-sa) * sb, s = (-sa) * cb + ca * sb;
  rot2_normalize(c, s);
  h[0] = ix + (ca * xb + sa * yb);        // t_inv + R_inv t_b   (Rot2::rotate with (c, s) = (ca, -sa), Rot2.cpp:100-106)
  h[1] = iy + (-sa * xb + ca * yb);
  h[2] = c; h[3] = s;
}
// Local(a, b) = ChartAtOrigin::Local(between(a, b)) = (x, y, theta) of a^-1 b  (Lie.h:136-138, Pose2.cpp:111-121,
// GTSAM_SLOW_BUT_CORRECT_EXPMAP off)
GT_HD void pose2_local(const double* a, const double* b, double* d) {
  double h[4];
  pose2_between_cs(a[0], a[1], cos(a[2]), sin(a[2]), b[0], b[1], cos(b[2]), sin(b[2]), h);
  d[0] = h[0]; d[1] = h[1]; d[2] = atan2(h[3], h[2]);
}
// Retract(a, v) = a * Pose2(v0, v1, v2)  (Lie.h:131-133, Pose2.cpp:99-109)
GT_HD void pose2_retract(const double* a, const double* v, double* y) {
  const double ca = cos(a[2]), sa = sin(a[2]), cv = cos(v[2]), sv = sin(v[2]);
  double c = ca * cv - sa * sv, s = sa * cv + ca * sv;
  rot2_normalize(c, s);
  y[0] = a[0] + (ca * v[0] + -sa * v[1]);
  y[1] = a[1] + (sa * v[0] + ca * v[1]);
  y[2] = atan2(s, c);
}

// traits<T>::Local(x, z) for the supported value types (PriorFactor.h:98-102):
// Pose3 Logmap(between); PinholeCamera [pose local; calib diff] (PinholeCamera.h:208-213,
// Cal3Bundler.h:150-152); Point3 z - x; Pose2 above.   vtype: 0 POSE3, 1 SFM_CAMERA, 2 POINT3, 3 POSE2.
GT_HD void value_local(int vtype, const double* x, const double* z, double* d) {
  if (vtype == 2) { d[0] = z[0] - x[0]; d[1] = z[1] - x[1]; d[2] = z[2] - x[2]; return; }
  if (vtype == 3) { pose2_local(x, z, d); return; }
  pose_local(x, z, d);
  if (vtype == 1) { d[6] = z[12] - x[12]; d[7] = z[13] - x[13]; d[8] = z[14] - x[14]; }
}
// traits<T>::Retract(x, d): Pose3 (Lie.h:131-133), PinholeCamera::retract (PinholeCamera.h:199-205)
// with Cal3Bundler::retract (Cal3Bundler.h:145-147), Point3 x + d, Pose2 above.
GT_HD void value_retract(int vtype, const double* x, const double* d, double* y) {
  if (vtype == 2) { y[0] = x[0] + d[0]; y[1] = x[1] + d[1]; y[2] = x[2] + d[2]; return; }
  if (vtype == 3) { pose2_retract(x, d, y); return; }
  pose_retract(x, d, y);
  if (vtype == 1) { y[12] = x[12] + d[6]; y[13] = x[13] + d[7]; y[14] = x[14] + d[8]; y[15] = x[15]; y[16] = x[16]; }
}

}  // namespace gt
