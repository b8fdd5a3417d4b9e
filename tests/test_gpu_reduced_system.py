"""The layer between the per-factor records and the step, on graphs with DESIGNED incidence (tests/structured.py), against a
long-double reference built from the device's own whitened records: k_cam_fused / k_cam_combine, k_lm_fused, k_red_diag, k_hoff,
k_point_factor, k_obs_E, k_build_diag, k_scatter_hoff, k_schur_pairs / k_schur_pairs_heavy, the tile Cholesky, the substitutions and
k_backsub_lm -- at the term counts, list lengths and dimensions where their chunking changes path.

Per design: set_values -> linearize -> try_lambda(1e-4, diagonal) and one identity-damped try, and for each
  (a) rc == 0;
  (b) hessian_diagonal() / gradient() against the long-double sums of the same records, entrywise within (k + 2) 2^-53 sum|terms| (k the
      entry's sum length: one rounding per product and per addition, in any association order -- derived, not tuned);
  (c) with L = tril(reduced_matrix()): rho(L L^T, S_ref, a) <= 8 max(rho64, 4), rho64 being the same pipeline in float64 numpy measured in
      the same test (the factor 8: another association order and the chain's reciprocal-plus-Newton pivot), and <= n_red + k_max + 16
      whatever rho64 is (componentwise backward error of a Cholesky factorisation plus the summation bound, through
      (|L||L^T|)_ij <= sqrt(S_ii S_jj) <= sqrt(a_i a_j)).  rho = max_ij |M - S_ref|_ij / sqrt(a_i a_j) / 2^-53 over the lower triangle, a the
      damped PRE-Schur diagonal;
  (d) delta() against the long-double solve of (S_ref, g_ref) plus back-substitution, 1e-7 in max-norm;
  (e) BAL designs: try_lambda_pcg at epsilon_rel = 1e-13, epsilon_abs = 1e-26 gives the same delta within 1e-5 (k_pcg_* over the same lists).
The two 4 608-dimensional chains (511 / 512 cameras: splits = 3 / 1 in k_cam_fused) leave (c) and (e) out -- a dense long-double S of that
size is too slow for a test -- and take the step from a float64 reference that tests/test_reduced_system_reference.py checks against the
oracle.  Every design is proved well-posed for the reference alone in that file.

Measured on the MI355X (rho of (c) per design, diagonal / identity try; rho64 of the same run beside it):
  design                 n_red    cap   rho / rho64 (diagonal)   rho / rho64 (identity)   (b): hdiag, gradient / bound
  A_pairs_mod0             270    831      29.30 / 29.63            57.63 / 64.48            0.311, 0.351
  A_pairs_mod1             261    822      73.67 / 34.38            55.99 / 35.11            0.282, 0.315
  A_pairs_mod2             270    831     109.19 / 86.83           142.47 / 123.29           0.345, 0.306
  A_pairs_mod3             270    831      35.72 / 44.31            88.37 / 107.60           0.318, 0.345
  B_heavy_513_577_639       27   6123       4.19 / 35.83             3.08 / 27.94            0.314, 0.351
  B_twin_500                27   5043       4.44 / 40.60             5.29 / 25.94            0.332, 0.390
  B_light_341               27   3453      18.01 / 26.88            23.03 / 22.50            0.308, 0.345
  C_cams16_splits16        144   5285      38.72 / 31.07            22.00 / 21.81            0.370, 0.374
  C_cams100_splits11       900   6041     405.18 / 321.39          210.93 / 266.23           0.330, 0.352
  D_lm63                   630    691      22.42 / 25.05            28.89 / 26.67            0.206, 0.234
  D_lm64                   630    701      22.44 / 6.87             34.19 / 11.44            0.272, 0.139
  D_lm65                   630    691      23.58 / 6.98             30.00 / 11.15            0.220, 0.233
  D_lm255                  630    816      30.95 / 8.71             29.33 / 8.04             0.265, 0.246
  D_lm256                  630    816      28.82 / 8.66             23.94 / 12.12            0.281, 0.220
  D_lm257                  630    831      25.72 / 10.46            28.43 / 10.21            0.252, 0.252
  E_bal14                  126    347       6.50 / 6.73              7.72 / 8.42             0.289, 0.351
  E_bal15                  135    336       8.49 / 7.24              8.76 / 7.37             0.325, 0.254
  E_bal29                  261    442      40.35 / 26.31            13.34 / 16.97            0.310, 0.276
  E_proj43                 258    844      20.88 / 18.04            20.88 / 15.44            0.104, 0.061
  E_proj64                 384    950      18.03 / 20.13            19.40 / 15.65            0.072, 0.049
  F_pose21                 126    172       4.90 / 2.59              6.05 / 2.80             0.121, 0.092
  F_pose22                 132    178       6.72 / 3.46              5.83 / 3.08             0.127, 0.113
  F_pose43                 258    304       5.80 / 3.24              6.09 / 5.59             0.106, 0.118
  F_pose64                 384    430       8.01 / 5.45              6.78 / 5.38             0.131, 0.097
  C_cams511_splits3          -      -          - / -                    - / -                0.361, 0.387
  C_cams512_splits1          -      -          - / -                    - / -                0.407, 0.328

(b) rests on the records being the same doubles in every kernel.  The first run of these tests showed that they were not: the fused
kernels (csrc/fused.h) recompute each GeneralSFM record where they need it, jacobians() in yet another kernel, and the compiler contracted
multiply-adds differently in each.  b = z - pi(x) cancels hundreds of pixels down to about one, so one rounding of pi is hundreds of ulps
of b: the Hessian diagonal missed the bound by up to 7.4 and the gradient by up to 1283 on the GeneralSFM designs (0.39 at most with the
stored-record build, 0.14 on the projection and pose-graph designs, whose records are stored).  FMA contraction is now off inside
sfm_linearize and what it calls (factors.h, geom.h); the figures above are from the build with that change.
"""
import numpy as np
import pytest

from tests import structured as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gtsam_amd import lib
    lib.load()
    return lib


def _sum_ratio(name, what, got, ref, k, abs_terms):
    """worst |got - ref| / ((k + 2) 2^-53 sum|terms|) over the entries, printed before anything is asserted"""
    bound = (k + 2) * T.U * np.asarray(abs_terms, np.longdouble)
    ratio = np.abs(np.asarray(got, np.longdouble) - ref) / np.where(bound > 0, bound, T.U)
    print(f"{name}: {what} worst |error| / bound = {float(ratio.max()):.3f} at entry {int(np.argmax(ratio))}")
    return float(ratio.max())


def _linearized(gpu, name):
    from oracle import gtsam_oracle as O
    (p, v0), _ = T.design(name)
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    dev.linearize()
    rec = T.device_records(dev)
    for ft in range(4):                                        # the ground the reference stands on: the records themselves
        if rec[ft].size:
            assert T.rel(rec[ft], O.jacobians_flat(p, v0, ft)) <= 1e-12, (name, ft)
    return p, dev, rec


@pytest.mark.parametrize("name", list(T.DESIGNS))
def test_assembly_sums_against_long_double_reference(gpu, name):
    """(b)"""
    p, dev, rec = _linearized(gpu, name)
    sums = T.reference_reduced_system(p, rec, None, 0.0, False, dense=False)
    hd, g = dev.hessian_diagonal(), dev.gradient()
    dev.close()
    rh = _sum_ratio(name, "hessian_diagonal", hd, sums.hdiag_ref, sums.hd_k, sums.hdiag_ref)      # (its terms are squares)
    rg = _sum_ratio(name, "gradient", g, sums.grad_ref, sums.grad_k, sums.grad_abs)
    assert rh <= 1.0 and rg <= 1.0, (name, rh, rg)


@pytest.mark.parametrize("name", list(T.DESIGNS))
def test_reduced_system_against_long_double_reference(gpu, name):
    """(a), (c), (d), (e)"""
    p, dev, rec = _linearized(gpu, name)
    kind = T.DESIGNS[name][2]
    order = dev.reduced_order()
    for lam, diag in T.modes(name):
        mode = f"{name} lambda {lam:g} {'diagonal' if diag else 'identity'}"
        rc, _ = dev.try_lambda(lam, diag)
        assert rc == 0, mode                                                                                        # (a)
        delta = dev.delta()
        ref = T.reference_reduced_system(p, rec, order, lam, diag, dtype=np.float64 if kind == "big" else np.longdouble)
        if kind != "big":
            L = np.tril(dev.reduced_matrix()).astype(np.longdouble)
            assert L.shape == ref.S_ref.shape
            r = T.rho(L @ L.T, ref.S_ref, ref.a)
            r64 = T.rho64(p, rec, order, lam, diag, ref)
            cap = ref.S_ref.shape[0] + ref.k_max + 16
            print(f"{mode}: rho {r:.2f}  rho64 {r64:.2f}  bound {8 * max(r64, 4):.1f}  cap {cap}  n_red {ref.S_ref.shape[0]}")
            assert r <= 8 * max(r64, 4) and r <= cap, (mode, r, r64, cap)                                           # (c)
        d_ref = T.solve_reference(ref)
        print(f"{mode}: delta rel {T.rel(delta, d_ref):.2e}")
        assert T.rel(delta, d_ref) <= 1e-7, (mode, T.rel(delta, d_ref))                                             # (d)
        if kind != "big" and p.n_sfm:
            rc, _, its = dev.try_lambda_pcg(lam, diag, max_iterations=3000, epsilon_rel=1e-13, epsilon_abs=1e-26)
            print(f"{mode}: pcg {its} iterations, delta rel {T.rel(dev.delta(), d_ref):.2e}")
            assert rc == 0 and T.rel(dev.delta(), d_ref) <= 1e-5, (mode, its, T.rel(dev.delta(), d_ref))            # (e)
    dev.close()
