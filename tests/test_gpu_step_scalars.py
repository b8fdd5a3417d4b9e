"""The scalars Levenberg-Marquardt accepts or rejects a step on, and the trial values, at the boundaries of their kernels:
k_error<1|2>, k_error_rows3, k_linear_error, k_sumsq, k_final_sum and k_retract (csrc/factors.hip) on the designs of
tests/step_designs.py, every one of which tests/test_step_designs_reference.py proves fit for its purpose on the host.

EXACT designs (per-factor errors are dyadic rationals: every partial sum is exact in double, in any order):
  (a) error() == the exact sum;
  (b) after linearize() and try_lambda(1, identity damping): out[0] == the exact 0.5 sum |b|^2 (the same number);
  (c) out[1] against the long-double 0.5 sum (A delta - b)^2 from jacobians() and delta(), within the allowance of
      step_designs.linear_costs (per row (m + 1) u (|b| + sum |A||delta|), per square 2 |v| e + e^2 + u v^2, over the sum (k + 2) u sum);
  (d) out[3] against the long-double |delta()|, within ((n + 2) / 2 + 1) u relative (n squares rounded and summed, one square root);
  (e) out[2] == error() of a second handle that was given trial_values(): the same kernel on the same doubles.
  A failing == in (a), (b) or (e) means a factor dropped or counted twice or a partial read from the wrong place.  The designs that only
  cross a cap of the error kernels stop after (a).
REALISTIC designs: error() against the long-double 0.5 sum |b|^2 of the device's own records, within the summation bound plus twice
  the forward error of one evaluation of b = z - pi (step_designs.sfm_residual_allowance: the error kernel and the record kernel each
  evaluate it once, under their own contraction of multiply-adds; z - pi cancels hundreds of pixels down to about one).
CHART designs: the census of branches recomputed from the device's own step and records (every branch still populated);
  trial_values() against the long-double retraction of values() by delta(), entrywise within the running-error allowance, the copied
  camera entries and the Point3 / calibration sums exactly; the b rows of jacobians(2) and jacobians(3) against the long-double Logmap
  within its allowance; error() against 0.5 sum |b|^2 of the records within twice the allowance of b per row plus the summation bound.

Measured on the MI355X (|error| / allowance; every == of (a), (b), (e) and of the copied / once-summed entries held on all designs):
  exact designs                         (c) worst ratio, design              (d) worst ratio, design
  ladders and mixes (49 designs)          0.021     sfm_1                      0.182    stereo_1
  partials_127/128/129_128                1.1e-06   partials_128_128           3.7e-05  partials_128_128
  cap-crossing with the linear part (25)  1.7e-06   prior_262145               0.033    between_262143
  realistic designs                     error() against the records
  E_bal14 / E_bal29 / D_lm65              9.0e-06 / 9.1e-05 / 3.2e-04
  chart designs        trial_values()   b of jacobians(3)   b of jacobians(2)   error() against the records
  mixed_1                 0.206            0.106                 -                 1.7e-02
  mixed_255               0.658            0.977               0.225               6.6e-04
  mixed_256               0.647            0.873               0.276               6.4e-04
  mixed_257               0.605            0.977               0.190               4.2e-04
  dims_255                0.482            0.686                 -                 2.8e-04
  dims_513                0.447            0.953                 -                 3.8e-04
  dims_1023               0.585            0.977                 -                 6.5e-04
  pose2_1                 0.489            0.102                 -                 8.6e-03
  pose2_85                0.824            0.150                 -                 1.1e-03
  pose2_257               0.822            0.191                 -                 1.3e-04
(0.977 is a Point3 / calibration difference: one subtraction, whose rounding may reach the whole of its one-rounding allowance.  The
sums sit far below their bounds because (k + 2) u sum|terms| is a worst case over every order of k additions.)

The tests themselves were checked once against deliberately wrong builds of factors.hip (not kept):
  - the second group of partials written at g1 + 1: every design that runs k_error<2> fails (a); only the two GeneralSFM-only graphs pass;
  - the second grid pass of the prior loops dropped: (a) fails on the six designs with more than 262 144 priors and on no other;
  - the second pass of k_error<2>'s prior loop reading prior i - stride again: (a) fails on the same six (the prior errors have the
    prime period 1021, so no grid stride maps a prior onto an equal one);
  - the second pass of the other four loops of k_linear_error dropped (the fused GeneralSFM chunk loop, the stored-record one, the
    projection loop with 2 and with 3 rows, the between loop): (b) fails on sfm_524289, sfm_524289_stereo_1, proj_524289,
    stereo_524226_mono_63 and between_524289 and on no other;
  - gmax of launch_error lowered by one: nothing fails, as it should -- a grid-stride loop is right for any grid, and the partials
    are summed over whatever g1 + g2 + g3 is.
"""
import numpy as np
import pytest

from gtsam_amd.problem import VAR_POINT3, VAR_SFM_CAMERA
from tests import step_designs as SD

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from gtsam_amd import lib
    lib.load()
    return lib


def _ratio(what, got, ref, allow):
    """worst |got - ref| / allowance, printed before anything is asserted; an entry with a zero allowance must be equal"""
    got = np.asarray(got, LD).reshape(-1); ref = np.asarray(ref, LD).reshape(-1); allow = np.asarray(allow, LD).reshape(-1)
    err = np.abs(got - ref)
    r = np.where(allow > 0, err / np.where(allow > 0, allow, 1), np.where(err == 0, 0.0, np.inf))
    print(f"{what}: worst |error| / allowance = {float(r.max()):.3g} at entry {int(np.argmax(r))} of {r.size}")
    return float(r.max())


def _records(dev, p):
    return {ft: dev.jacobians(ft) for ft, n in ((0, p.n_sfm), (1, p.n_proj), (2, p.n_between), (3, p.n_prior), (4, p.n_stereo)) if n}


@pytest.mark.parametrize("name", list(SD.EXACT))
def test_exact_designs(gpu, name):
    d = SD.exact(name)
    p = d.p
    dev = gpu.DeviceGraph(p)
    dev.set_values(d.values)
    e = dev.error()
    print(f"{name}: grids {SD.error_grids(**d.counts)} / {SD.linear_grid(**d.counts)}  error {e!r}  exact {d.exact!r}")
    assert e == d.exact, (name, e, d.exact, (e - d.exact) / SD.UNIT)                                             # (a)
    if not d.linear:
        dev.close()
        return
    dev.linearize()
    rc, out = dev.try_lambda(1.0, False)
    assert rc == 0, name
    print(f"{name}: out {out!r}")
    assert out[0] == d.exact, (name, out[0], d.exact, (out[0] - d.exact) / SD.UNIT)                             # (b)
    delta, trial = dev.delta(), dev.trial_values()
    e0, e1, allow = SD.linear_costs(p, _records(dev, p), delta)
    dev.close()
    assert float(e0) == d.exact, name                                     # (the records hold the designed residuals)
    rc_ = _ratio(f"{name}: (c) linear error of the step", out[1], e1, allow)
    norm = np.sqrt((delta.astype(LD) ** 2).sum())
    rd = _ratio(f"{name}: (d) |delta|", out[3], norm, ((delta.size + 2) / 2 + 1) * SD.U * norm)
    assert np.isfinite(out[2]) and out[0] - out[1] >= 0, name
    dev2 = gpu.DeviceGraph(p)
    dev2.set_values(trial)
    e2 = dev2.error()
    dev2.close()
    print(f"{name}: (e) trial error {out[2]!r}  error() at trial_values() {e2!r}")
    assert rc_ <= 1.0 and rd <= 1.0, (name, rc_, rd)                                                            # (c), (d)
    assert out[2] == e2, (name, out[2], e2)                                                                     # (e)


@pytest.mark.parametrize("name", SD.REALISTIC)
def test_error_against_the_records_on_realistic_graphs(gpu, name):
    from tests import structured as T
    (p, v0), _ = T.design(name)
    dev = gpu.DeviceGraph(p)
    dev.set_values(v0)
    e = dev.error()
    dev.linearize()
    rec = _records(dev, p)
    dev.close()
    b_allow = [2 * SD.sfm_residual_allowance(p, v0)]
    if p.n_prior:                      # Point3 priors, isotropic noise: a difference and a product, evaluated once by either kernel
        assert (p.var_type[p.prior_var] == VAR_POINT3).all()
        b_allow.append(4 * SD.U * np.abs(rec[3][:, 81:84]).astype(LD))
    ref, allow = SD.error_from_records(p, rec, b_allow)
    r = _ratio(f"{name}: error() against its records", e, ref, allow)
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("name", list(SD.CHART))
def test_chart_designs(gpu, name):
    d = SD.chart(name)
    p = d.p
    dev = gpu.DeviceGraph(p)
    dev.set_values(d.values)
    e = dev.error()
    dev.linearize()
    rc, out = dev.try_lambda(d.lam, False)
    assert rc == 0, name
    values, delta, trial = dev.values(), dev.delta(), dev.trial_values()
    rec = _records(dev, p)
    dev.close()
    assert np.array_equal(values, d.values)
    print(f"{name}: error {e!r}  out {out!r}  max |delta - xi| {np.abs(delta - d.xi).max():.2e}")
    # ---- the branches the device's own step and residuals take
    bb = rec[2][:, 72:78] if p.n_between else None
    c = SD.census(p, values, delta, rec[3][:, 81:90], bb)
    print(f"{name}: census {c}")
    if name in SD.CHART_FULL_CENSUS:
        assert all(c[b] >= 1 for b in SD.BRANCHES), (name, c)
    if name in ("pose2_85", "pose2_257"):
        assert all(c[b] >= 1 for b in SD.BRANCHES_POSE2), (name, c)
    # ---- the retraction
    y, ay, _ = SD.retract_reference(p, values, delta)
    rr = _ratio(f"{name}: trial_values() against the long-double retraction", trial, y, ay)
    voff, doff = p.val_offsets(), p.dim_offsets()
    for v, t in enumerate(p.var_type):                                        # what is copied or summed once must be exactly equal
        x = values[voff[v]:voff[v + 1]]; dl = delta[doff[v]:doff[v + 1]]; tv = trial[voff[v]:voff[v + 1]]
        if t == VAR_POINT3:
            assert np.array_equal(tv, x + dl), (name, v)
        elif t == VAR_SFM_CAMERA:
            assert np.array_equal(tv[12:15], x[12:15] + dl[6:9]) and tv[15] == x[15] and tv[16] == x[16], (name, v)
    # ---- the right-hand sides of the records against the long-double Logmap
    b, ab, _, _ = SD.prior_b_reference(p, values)
    rb = _ratio(f"{name}: b of jacobians(3) against the long-double Local", rec[3][:, 81:90], b, ab)
    b_allow = []
    re_ = 0.0
    if p.n_between:
        b2, ab2, _, _ = SD.between_b_reference(p, values)
        re_ = _ratio(f"{name}: b of jacobians(2) against the long-double Logmap", bb, b2, ab2)
        b_allow.append(2 * ab2)
    dims = np.array([3 if t in (2, 3) else 6 if t == 0 else 9 for t in p.var_type[p.prior_var]])
    b_allow += [2 * ab[dims == dd][:, :dd] for dd in np.unique(dims)]       # (the grouping of step_designs.record_rows)
    ref, allow = SD.error_from_records(p, rec, b_allow)
    rs = _ratio(f"{name}: error() against its records", e, ref, allow)
    assert rr <= 1.0 and rb <= 1.0 and re_ <= 1.0 and rs <= 1.0, (name, rr, rb, re_, rs)
