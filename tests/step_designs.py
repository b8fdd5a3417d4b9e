"""Designs and references for the scalars of one Levenberg-Marquardt step and for the retraction (tests only, numpy on the host).

error(), the error of the trial point, the two linear costs, |delta| and the trial values come from k_error<1|2|6>, k_error_rows3,
k_linear_error, k_sumsq, k_final_sum and k_retract (csrc/factors.hip).  Three families of graphs are built here:

EXACT designs (exact_design, EXACT): every factor's error is a dyadic rational by construction -- identity rotations, focal length
1, depths that are powers of two, translations, points and measurements in sixteenths, unit noise or diagonal noise with power-of-two
sigmas -- so every partial sum of the errors, in any association order and with or without fused multiply-adds, is exact in double
and the device must return the exact total bit for bit.  The builder knows each factor's error without evaluating a factor formula
(it chooses the residual and derives the measurement from it); tests/test_step_designs_reference.py proves, with the oracle and with
the host compile of factors.h, that the formulas indeed give those errors.  The counts walk the lane, wave, block and grid-cap
boundaries of the kernels; error_grids / linear_grid restate the launch arithmetic.

CHART designs (chart_design, CHART): unit-noise priors z = x (+) xi on interleaved Pose3 / SfmCamera / Point3 variables (Pose2 in a
graph of its own) whose xi walks every branch of so3_expmap, so3_logmap, pose_expmap, pose_logmap and the atan2 wrap of Pose2, plus
a few BetweenFactor<Pose3> edges in the same regimes.  One identity-damped try at a tiny lambda gives delta ~ xi on the prior-only
variables, so k_retract meets the same branches.

REALISTIC designs (REALISTIC): random-incidence graphs of tests/structured.py, for error() against the device's own records.

The long-double references restate geom.h branch for branch, NOT better-conditioned formulas: just above the near-zero threshold the
translation of pose_expmap cancels to a relative u / theta ~ 1e-8, and the near-pi Logmap is ill-conditioned; both are the
reference's behaviour.  Each reference value carries its RUNNING-ERROR ALLOWANCE (class E below; Higham, Accuracy and Stability of
Numerical Algorithms, section 3.3): every arithmetic operation of geom.h appears exactly once in the restatement and adds ONE
rounding, 2^-53 |result|, to the error bound it propagates from its operands (sums and differences: the operands' bounds added;
products: |a| e_b + |b| e_a + e_a e_b; quotients and square roots: carried through the division); every device transcendental (sin,
cos, tan, acos, atan2) adds FOUR roundings (two ulps) on top of its argument's bound times the derivative; multiplications by 0.5,
2 and -1 and copies are exact and add nothing; where one double enters an expression twice (theta / (2 sin theta),
t / (2 tan(t / 2))) its bound is carried through the derivative of the whole expression (E.composite).  The count of roundings on a
path is therefore made by the operations themselves, from the code, and nothing in it is tuned to a result.  A fused multiply-add on
the device rounds once where the bound counts twice.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from gtsam_amd.problem import (NOISE_DIAGONAL, NOISE_UNIT, STORAGE, TANGENT, VAR_POINT3, VAR_POSE2, VAR_POSE3, VAR_SFM_CAMERA, Problem)

U = 2.0 ** -53
LD = np.longdouble
EPS = 2.220446049250313e-16          # kEps of geom.h
UNIT = 2.0 ** -12                    # every per-factor error of an exact design is a multiple of this

# ------------------------------------------------------------------------------------------------------------------------
# launch arithmetic.  THIS RESTATEMENT MUST FOLLOW csrc/factors.hip (grid_for, launch_error, launch_linear_error, launch_retract):
# when a cap, the block size or the order of the partial groups changes there, change it here.
# ------------------------------------------------------------------------------------------------------------------------
K_BLOCK, K_MAX_BLOCKS = 256, 2048
CAP_ERROR, CAP_ERROR_STEREO, CAP_LINEAR = K_MAX_BLOCKS // 2, K_MAX_BLOCKS // 4, K_MAX_BLOCKS


def grid_for(n):
    return int(min(max((n + K_BLOCK - 1) // K_BLOCK, 1), K_MAX_BLOCKS))


def error_grids(n_sfm=0, n_proj=0, n_stereo=0, n_between=0, n_prior=0):
    """(g1, g2, g3) of launch_error: k_error<1>, k_error<2>, k_error_rows3; their partials lie at 0, g1 and g1 + g2."""
    stereo = n_stereo > 0
    total_proj = n_proj + n_stereo                       # the device's projection range: monocular first, then stereo
    nrest = max(0 if stereo else n_proj, n_between, n_prior)
    gmax = CAP_ERROR_STEREO if stereo else CAP_ERROR
    g1 = min(grid_for(n_sfm), gmax) if n_sfm else 0
    g2 = min(grid_for(nrest), gmax) if (nrest or not g1) else 0
    g3 = min(grid_for(total_proj), gmax) if stereo and total_proj else 0
    return g1, g2, g3


def linear_grid(n_sfm=0, n_proj=0, n_stereo=0, n_between=0, n_prior=0):
    return grid_for(max(n_sfm, n_proj + n_stereo, n_between, n_prior))


# ------------------------------------------------------------------------------------------------------------------------
# exact designs
# ------------------------------------------------------------------------------------------------------------------------
DEPTHS = np.array([1.0, 2.0, 4.0, -1.0, 1.0, -2.0, 2.0])      # powers of two; every fourth or so behind the camera


def _points(n):
    j = np.arange(n)
    return np.stack([((j * 7) % 65 - 32) / 16.0, ((j * 11) % 33 - 16) / 16.0, DEPTHS[j % DEPTHS.size]], 1)


def _pose_t(k):
    return np.stack([-(k % 8) / 2.0, (k % 8) / 4.0, np.zeros(k.shape)], 1)


def _residuals(i, dim):
    """designed whitened-free residuals of factor i: multiples of 1/16, |.| < 8"""
    cols = [((i * (37 + 6 * c)) % 255 - 127) / 16.0 for c in range(dim)]
    return np.stack(cols, 1)


def exact_design(n_sfm=0, n_proj=0, n_stereo=0, n_between=0, n_prior=0):
    """-> namespace p (Problem), values, errors {range name: per-factor error, float64 and exact}, exact (the exact total, a float that
    is an integer number of UNITs), units (that integer, a Python int), anchored (every variable has a unit prior: the linear system is
    well posed and linearize() / try_lambda() are part of the test), counts.
    Variables: min(8, n_sfm) cameras, up to 8 poses, the observed points, then up to 7 Point3 that only carry priors.  The first
    priors go one to each variable in order (Pose3 / camera priors: identity rotation, so Logmap takes its Taylor and t < 1e-10
    branches and the residual is the translation / calibration difference), the rest to the prior-only points."""
    nc = min(8, n_sfm)
    n_obs = max(n_proj, n_stereo)
    npose = 8 if n_between else min(8, n_obs)
    npt = max(-(-n_sfm // nc) if nc else 0, -(-n_obs // npose) if n_obs else 0)
    n_base = nc + npose + npt
    if n_base == 0:
        npose = n_base = 1                                   # a graph of priors only still has one reduced variable
    anchored = n_prior >= n_base
    extra = n_prior - n_base if anchored else 0
    n_extra_vars = min(7, extra)
    vt = np.concatenate([np.full(nc, VAR_SFM_CAMERA), np.full(npose, VAR_POSE3), np.full(npt + n_extra_vars, VAR_POINT3)]).astype(np.int32)
    p = Problem(var_type=vt)
    eye = np.eye(3).reshape(-1)
    kc = np.arange(nc)
    cams = np.zeros((nc, 17)); cams[:, :9] = eye
    cams[:, 9] = kc / 4.0; cams[:, 10] = -kc / 8.0; cams[:, 12] = 1.0; cams[:, 15] = kc / 2.0; cams[:, 16] = -kc / 4.0
    poses = np.zeros((npose, 12)); poses[:, :9] = eye; poses[:, 9:] = _pose_t(np.arange(npose))
    pts = _points(npt)
    xpts = np.stack([np.arange(n_extra_vars) / 4.0, -np.arange(n_extra_vars) / 2.0, np.ones(n_extra_vars)], 1)
    values = np.concatenate([cams.reshape(-1), poses.reshape(-1), pts.reshape(-1), xpts.reshape(-1)])
    pt0 = nc + npose
    errors = {}
    u2 = p.add_noise(NOISE_UNIT, 2); d2 = p.add_noise(NOISE_DIAGONAL, 2, [2.0, 0.5])
    u3 = p.add_noise(NOISE_UNIT, 3); d3 = p.add_noise(NOISE_DIAGONAL, 3, [2.0, 0.5, 1.0])
    u6 = p.add_noise(NOISE_UNIT, 6); d6 = p.add_noise(NOISE_DIAGONAL, 6, [1.0, 2.0, 4.0, 0.5, 2.0, 1.0])
    u9 = p.add_noise(NOISE_UNIT, 9)
    isig = {u2: np.ones(2), d2: np.array([0.5, 2.0]), u3: np.ones(3), d3: np.array([0.5, 2.0, 1.0]), u6: np.ones(6),
            d6: np.array([1.0, 0.5, 0.25, 2.0, 0.5, 1.0]), u9: np.ones(9)}

    def whitened_error(r, nz):
        w = np.stack([isig[int(k)] for k in np.unique(nz)])[np.searchsorted(np.unique(nz), nz)]
        return 0.5 * ((r * w) ** 2).sum(1)

    if n_sfm:
        i = np.arange(n_sfm); c = i % nc; j = i // nc
        q = pts[j] - cams[c, 9:12]
        front = q[:, 2] > 0
        pi = cams[c, 15:17] + q[:, :2] / np.where(front, q[:, 2], 1.0)[:, None]          # f = 1, k1 = k2 = 0: exact in sixteenths of 1/4
        r = _residuals(i, 2)
        nz = np.where(i % 3 == 1, d2, u2).astype(np.int32)
        p.sfm_cam = c.astype(np.int32); p.sfm_point = (pt0 + j).astype(np.int32); p.sfm_noise = nz
        p.sfm_z = (np.where(front[:, None], pi, 0.0) - r).reshape(-1)                    # r = pi - z
        errors["sfm"] = np.where(front, whitened_error(r, nz), 0.0)                      # behind: exactly 0 (GeneralSFMFactor.h:131-137)
    if n_proj or n_stereo:
        p.calib = np.array([1.0, 1.0, 0.0, 0.0, 0.0])
    for name, n, dim in (("proj", n_proj, 2), ("stereo", n_stereo, 3)):
        if not n:
            continue
        i = np.arange(n); k = i % npose; j = i // npose
        q = pts[j] - poses[k, 9:12]
        front = q[:, 2] > 0
        d = 1.0 / np.where(front, q[:, 2], 1.0)
        bl = 0.5
        pi = np.stack([q[:, 0] * d, q[:, 1] * d], 1) if dim == 2 else np.stack([q[:, 0] * d, (q[:, 0] - bl) * d, q[:, 1] * d], 1)
        r = _residuals(i + 5, dim)
        nz = np.where(i % 4 == 2, d2 if dim == 2 else d3, u2 if dim == 2 else u3).astype(np.int32)
        z = np.where(front[:, None], pi, 0.0) - r
        r_eff = np.where(front[:, None], r, 2.0)                                         # behind: the constant residual 2 fx
        errors[name] = whitened_error(r_eff, nz)
        setattr(p, name + "_pose", (nc + k).astype(np.int32)); setattr(p, name + "_point", (pt0 + j).astype(np.int32))
        setattr(p, name + "_z", z.reshape(-1)); setattr(p, name + "_noise", nz)
        setattr(p, name + "_calib", np.zeros(n, np.int32)); setattr(p, name + "_sensor", np.full(n, -1, np.int32))
        if dim == 3:
            p.calib_baseline = np.array([bl])
    if n_between:
        i = np.arange(n_between); a = i % 8; b = (a + 1 + (i // 8) % 7) % 8
        r = np.zeros((n_between, 6)); r[:, 3:] = _residuals(i + 11, 3)
        Z = np.zeros((n_between, 12)); Z[:, :9] = eye; Z[:, 9:] = poses[b, 9:] - poses[a, 9:] - r[:, 3:]      # r = h_t - Z_t
        nz = np.where(i % 5 == 3, d6, u6).astype(np.int32)
        p.between_v1 = (nc + a).astype(np.int32); p.between_v2 = (nc + b).astype(np.int32); p.between_z = Z.reshape(-1); p.between_noise = nz
        errors["between"] = whitened_error(r, nz)
    if n_prior:
        n_first = min(n_prior, n_base)
        var = np.concatenate([np.arange(n_first), n_base + np.arange(extra) % max(n_extra_vars, 1)]).astype(np.int32)
        t = vt[var]
        stor = np.array([STORAGE[int(x)] for x in range(4)])[t]
        off = np.concatenate([[0], np.cumsum(stor)])
        voff = p.val_offsets()
        data = np.zeros(int(off[-1])); e = np.zeros(n_prior); nzs = np.zeros(n_prior, np.int32)
        i = np.arange(n_prior)
        # (+ 5: prior 0 must not have a zero error; period 1021, a prime: every grid stride under test is a multiple of 1024, and a
        # second pass that read factor i - stride again, or partials exchanged 4 k blocks apart, must change the sum)
        m = (i * 37 + 5) % 1021
        r3 = np.stack([m / 8.0, (m % 5) / 4.0, -(m % 3) / 2.0], 1)                       # z - x of the translation / the point
        for ty, dim, slot in ((VAR_POSE3, 6, 9), (VAR_SFM_CAMERA, 9, 9), (VAR_POINT3, 3, 0)):
            sel = np.flatnonzero(t == ty)
            if not sel.size:
                continue
            st = STORAGE[ty]
            x = values[voff[var[sel]][:, None] + np.arange(st)[None, :]]
            z = x.copy(); z[:, slot:slot + 3] += r3[sel]
            r = np.zeros((sel.size, dim)); r[:, dim - 3 if ty == VAR_POSE3 else (3 if ty == VAR_SFM_CAMERA else 0):][:, :3] = r3[sel]
            if ty == VAR_SFM_CAMERA:
                dc = np.stack([(m[sel] % 7) / 4.0, (m[sel] % 2) / 8.0, -(m[sel] % 3) / 16.0], 1)
                z[:, 12:15] += dc; r[:, 6:9] = dc
            nz = np.full(sel.size, {VAR_POSE3: u6, VAR_SFM_CAMERA: u9, VAR_POINT3: u3}[ty], np.int32)
            if ty == VAR_POINT3:
                nz = np.where(sel % 2 == 1, d3, u3).astype(np.int32)
            if ty == VAR_POSE3:
                nz = np.where(sel % 2 == 1, d6, u6).astype(np.int32)
            data[off[sel][:, None] + np.arange(st)[None, :]] = z
            e[sel] = whitened_error(r, nz); nzs[sel] = nz
        p.prior_var = var; p.prior_off = off[:-1].astype(np.int64); p.prior_data = data; p.prior_noise = nzs
        errors["prior"] = e
    units = 0
    for e in errors.values():
        k = e / UNIT
        assert np.array_equal(k, np.floor(k)) and k.max(initial=0) < 2.0 ** 53
        units += int(k.astype(np.int64).sum())
    assert units < 2 ** 53
    counts = dict(n_sfm=n_sfm, n_proj=n_proj, n_stereo=n_stereo, n_between=n_between, n_prior=n_prior)
    return SimpleNamespace(p=p, values=values, errors=errors, units=units, exact=float(units) * UNIT, anchored=anchored, counts=counts)


LADDER = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)


def _anchors(n, more=0):
    """the variables of a design whose largest observation range has n factors (+ `more` others): a unit prior on each"""
    return min(8, n) + -(-n // min(8, n)) + more


def _caps(cap):
    return (cap * K_BLOCK - 1, cap * K_BLOCK, cap * K_BLOCK + 1)


# name -> (counts, run the linear part).  The linear part (checks (b)-(e)) needs every variable anchored; the cap-crossing designs of
# the error kernels leave it out where only error() is under test.
EXACT = {}
for _n in LADDER:
    EXACT[f"sfm_{_n}"] = (dict(n_sfm=_n, n_prior=min(8, _n) + -(-_n // min(8, _n))), True)
    EXACT[f"proj_{_n}"] = (dict(n_proj=_n, n_prior=min(8, _n) + -(-_n // min(8, _n))), True)
    EXACT[f"stereo_{_n}"] = (dict(n_stereo=_n, n_prior=min(8, _n) + -(-_n // min(8, _n))), True)
    EXACT[f"between_{_n}"] = (dict(n_between=_n, n_prior=8), True)
    EXACT[f"prior_{_n}"] = (dict(n_prior=_n), True)
for _n in _caps(CAP_ERROR):
    EXACT[f"sfm_{_n}_prior_1"] = (dict(n_sfm=_n, n_prior=1), False)                 # k_error<1> wraps its grid beside one prior in k_error<2>
    EXACT[f"prior_{_n}"] = (dict(n_prior=_n), True)
EXACT[f"between_{CAP_ERROR * K_BLOCK + 1}_proj_63_prior_8"] = (dict(n_between=CAP_ERROR * K_BLOCK + 1, n_proj=63, n_prior=8 + 8), False)
for _n, _mono in zip(_caps(CAP_ERROR_STEREO), (0, 64, 63)):                         # counts of the whole projection range, stereo graph
    EXACT[f"stereo_{_n - _mono}_mono_{_mono}"] = (dict(n_stereo=_n - _mono, n_proj=_mono, n_prior=3), False)
EXACT["stereo_200_mono_65"] = (dict(n_stereo=200, n_proj=65, n_prior=8 + 25), True)
EXACT["stereo_300_mono_256"] = (dict(n_stereo=300, n_proj=256, n_prior=8 + 38), True)          # the block boundary inside the range
EXACT["stereo_70_mono_512_sfm_40"] = (dict(n_stereo=70, n_proj=512, n_sfm=40, n_prior=8 + 8 + 64), True)
for _n in _caps(CAP_LINEAR):
    EXACT[f"prior_{_n}"] = (dict(n_prior=_n), True)                                 # k_linear_error wraps its grid, k_error<2> wraps twice
for _n, _mono in zip(_caps(CAP_LINEAR), (0, 64, 63)):                                # every other loop of k_linear_error wraps too, linear part on:
    EXACT[f"sfm_{_n}"] = (dict(n_sfm=_n, n_prior=_anchors(_n)), True)                # the fused GeneralSFM loop (its own chunk stride),
    EXACT[f"proj_{_n}"] = (dict(n_proj=_n, n_prior=_anchors(_n)), True)              # the projection loop with 2 rows
    EXACT[f"stereo_{_n - _mono}_mono_{_mono}"] = (dict(n_stereo=_n - _mono, n_proj=_mono, n_prior=_anchors(_n - _mono)), True)   # and with 3,
    EXACT[f"between_{_n}"] = (dict(n_between=_n, n_prior=8), True)
EXACT["sfm_524289_stereo_1"] = (dict(n_sfm=CAP_LINEAR * K_BLOCK + 1, n_stereo=1, n_prior=_anchors(CAP_LINEAR * K_BLOCK + 1, 1)), True)   # the stored-record GeneralSFM loop
for _n in _caps(CAP_ERROR):                                                         # the projection and between loops of k_error<2> at its cap
    EXACT[f"proj_{_n}"] = (dict(n_proj=_n, n_prior=_anchors(_n)), True)
for _n in _caps(CAP_ERROR)[:2]:
    EXACT[f"between_{_n}"] = (dict(n_between=_n, n_prior=8), True)
EXACT["prior_524289_sfm_1_proj_5_between_63"] = (dict(n_prior=CAP_LINEAR * K_BLOCK + 1, n_sfm=1, n_proj=5, n_between=63), True)
EXACT["between_1100_sfm_7_proj_33_prior_300"] = (dict(n_between=1100, n_sfm=7, n_proj=33, n_prior=300), True)
# the partials: g1 + g2 = 255, 256, 257 (1 is prior_1) and g1 = g2 = 1024, the end of the slot
EXACT["partials_127_128"] = (dict(n_sfm=127 * K_BLOCK - 3, n_prior=128 * K_BLOCK - 5), True)
EXACT["partials_128_128"] = (dict(n_sfm=128 * K_BLOCK - 3, n_prior=128 * K_BLOCK), True)
EXACT["partials_129_128"] = (dict(n_sfm=128 * K_BLOCK + 1, n_prior=127 * K_BLOCK + 1), True)
EXACT["partials_1024_1024"] = (dict(n_sfm=CAP_ERROR * K_BLOCK - 100, n_prior=CAP_ERROR * K_BLOCK + 1), False)


@functools.lru_cache(maxsize=4)
def exact(name):
    """The design, built once and kept for the tests that follow one another on it (the largest hold half a gigabyte of tables)."""
    d = exact_design(**EXACT[name][0])
    d.linear = EXACT[name][1]
    assert not d.linear or d.anchored, name
    return d


# ------------------------------------------------------------------------------------------------------------------------
# running-error arithmetic in long double
# ------------------------------------------------------------------------------------------------------------------------
class E:
    """A long-double value v and a bound e of |device double result - v| when the same operations are carried out in IEEE double
    on inputs that agree with this one's within its operands' bounds (module docstring)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = LD(v); self.e = LD(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def _r(v, e, k=1):
        return E(v, e + k * U * abs(v))

    def __add__(a, b): b = E.of(b); return E._r(a.v + b.v, a.e + b.e)
    __radd__ = __add__
    def __sub__(a, b): b = E.of(b); return E._r(a.v - b.v, a.e + b.e)
    def __rsub__(a, b): return E.of(b) - a
    def __mul__(a, b): b = E.of(b); return E._r(a.v * b.v, abs(a.v) * b.e + abs(b.v) * a.e + a.e * b.e)
    __rmul__ = __mul__
    def __neg__(a): return E(-a.v, a.e)

    def __truediv__(a, b):
        b = E.of(b); q = a.v / b.v
        assert abs(b.v) > 2 * b.e, "division by a quantity that is not known to be non-zero"
        return E._r(q, (a.e + abs(q) * b.e) / (abs(b.v) - b.e))

    def __rtruediv__(a, b): return E.of(b) / a
    def scale(a, s): return E(a.v * LD(s), a.e * abs(LD(s)))          # s a power of two: exact

    def sqrt(a):
        lo = a.v - a.e                                                # (lo <= 0: all that is known is 0 <= result <= sqrt(v + e))
        return E._r(np.sqrt(a.v), a.e / (2 * np.sqrt(lo)) if lo > 0 else np.sqrt(a.v + a.e))

    def sin(a): return E._r(np.sin(a.v), a.e * min(LD(1), abs(np.cos(a.v)) + a.e), 4)
    def cos(a): return E._r(np.cos(a.v), a.e * min(LD(1), abs(np.sin(a.v)) + a.e), 4)

    def tan(a):
        t = np.tan(a.v)
        return E._r(t, a.e * (1 + (abs(t) + 2 * a.e * (1 + t * t)) ** 2), 4)

    def composite(a, f, df, rounds):
        """f(a) where the device's expression uses the SAME double a more than once (t / (2 tan(t / 2)), theta / (2 sin theta)): the
        bound of a goes through the derivative df of the whole expression -- the occurrences move together -- and not through each
        occurrence as if it were independent; `rounds` roundings of the expression's own operations on top."""
        slope = max(abs(df(x)) for x in (a.v - a.e, a.v, a.v + a.e))
        return E._r(f(a.v), slope * a.e, rounds)

    def acos(a):
        x = min(abs(a.v) + a.e, LD(1))
        assert x < 1
        return E._r(np.arccos(a.v), a.e / np.sqrt(1 - x * x), 4)


def atan2(s, c):
    s, c = E.of(s), E.of(c)
    r2 = s.v * s.v + c.v * c.v
    rad = np.sqrt(r2) - np.sqrt(s.e * s.e + c.e * c.e)
    assert rad > 0
    return E._r(np.arctan2(s.v, c.v), (abs(c.v) * s.e + abs(s.v) * c.e) / (rad * rad), 4)


def lift(a):
    return [E(x) for x in np.asarray(a, np.float64).reshape(-1)]


def vals(xs):
    return np.array([x.v for x in xs], LD)


def errs(xs):
    return np.array([x.e for x in xs], LD)


# ---- geom.h, operation for operation ------------------------------------------------------------------------------------
def mat3_mul(A, B):
    return [A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def mat3_vec(A, x):
    return [A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2] for i in range(3)]


def mat3_tvec(A, x):
    return [A[i] * x[0] + A[3 + i] * x[1] + A[6 + i] * x[2] for i in range(3)]


def skew3(x, y, z):
    o = E(0.0)
    return [o, -z, y, z, o, -x, -y, x, o]


def so3_expmap(w):
    """-> (R[9], branch): 'near_zero' (theta^2 <= eps: I + W) or 'general'"""
    theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    W = skew3(*w)
    one = E(1.0)
    if theta2.v <= EPS:
        R = list(W); R[0] = W[0] + one; R[4] = W[4] + one; R[8] = W[8] + one
        return R, "near_zero"
    theta = theta2.sqrt()
    sin_theta = theta.sin()
    s2 = theta.scale(0.5).sin()
    omc = (s2 * s2).scale(2.0)
    K = [x / theta for x in W]
    KK = mat3_mul(K, K)
    R = [sin_theta * K[i] + omc * KK[i] for i in range(9)]
    R[0] = R[0] + one; R[4] = R[4] + one; R[8] = R[8] + one
    return R, "general"


def so3_logmap(R):
    """-> (omega[3], branch): 'pi_a0' | 'pi_a1' | 'pi_a2' (near pi, a = the largest diagonal entry) | 'acos' | 'taylor'"""
    R11, R12, R13, R21, R22, R23, R31, R32, R33 = R
    tr = R11 + R22 + R33
    if (tr + 1.0).v < 1e-3:
        if R33.v > R22.v and R33.v > R11.v:
            a = 2; anti = R21 - R12; along_a = (R33.scale(2.0)) + 2.0; along_b = R31 + R13; along_c = R23 + R32
        elif R22.v > R11.v:
            a = 1; anti = R13 - R31; along_a = (R22.scale(2.0)) + 2.0; along_b = R23 + R32; along_c = R12 + R21
        else:
            a = 0; anti = R32 - R23; along_a = (R11.scale(2.0)) + 2.0; along_b = R12 + R21; along_c = R31 + R13
        inv_root = 1.0 / along_a.sqrt()
        length = (along_a * along_a + along_b * along_b + along_c * along_c + anti * anti).sqrt()
        sign = -1.0 if anti.v < 0 else 1.0
        angle = np.pi - (anti.scale(2 * sign)) / length          # (kPi is the double nearest pi: np.pi)
        k = (inv_root.scale(0.5)) * angle
        wa, wb, wc = (k.scale(sign)) * along_a, (k.scale(sign)) * along_b, (k.scale(sign)) * along_c
        return ([wb, wc, wa] if a == 2 else [wc, wa, wb] if a == 1 else [wa, wb, wc]), f"pi_a{a}"
    tr_3 = tr - 3.0
    if tr_3.v < -1e-6:
        theta = ((tr - 1.0).scale(0.5)).acos()
        magnitude = theta.composite(lambda x: x / (2 * np.sin(x)), lambda x: (np.sin(x) - x * np.cos(x)) / (2 * np.sin(x) ** 2), 5)   # sin: 4, the division: 1
        branch = "acos"
    else:
        magnitude = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0
        branch = "taylor"
    return [magnitude * (R32 - R23), magnitude * (R13 - R31), magnitude * (R21 - R12)], branch


def pose_compose(A, B):
    R = mat3_mul(A, B)
    t = mat3_vec(A, B[9:12])
    return R + [A[9 + i] + t[i] for i in range(3)]


def pose_inverse(A):
    t = mat3_tvec(A, [-A[9], -A[10], -A[11]])
    return [A[3 * j + i] for i in range(3) for j in range(3)] + t


def pose_between(A, B):
    return pose_compose(pose_inverse(A), B)


def pose_expmap(xi):
    w, v = xi[:3], xi[3:6]
    R, branch = so3_expmap(w)
    theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if theta2.v > EPS:
        wv = w[0] * v[0] + w[1] * v[1] + w[2] * v[2]
        c = [w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0]]
        Rc = mat3_vec(R, c)
        t = [(c[i] - Rc[i] + w[i] * wv) / theta2 for i in range(3)]
    else:
        t = list(v)
    return R + t, branch


def pose_logmap(T):
    """-> (xi[6], so3 branch, 'small_t' (t < 1e-10: the translation as it is) | 'general_t')"""
    w, branch = so3_logmap(T[:9])
    Tt = T[9:12]
    t = (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]).sqrt()
    if t.v < 1e-10:
        return w + list(Tt), branch, "small_t"
    W = skew3(w[0] / t, w[1] / t, w[2] / t)
    WT = mat3_vec(W, Tt)
    WWT = mat3_vec(W, WT)
    c = 1.0 - t.composite(lambda x: x / (2 * np.tan(x / 2)), lambda x: (np.sin(x) - x) / (4 * np.sin(x / 2) ** 2), 5)       # tan: 4, the division: 1
    return w + [Tt[i] - t.scale(0.5) * WT[i] + c * WWT[i] for i in range(3)], branch, "general_t"


def pose_retract(T, xi):
    Ex, branch = pose_expmap(xi)
    return pose_compose(T, Ex), branch


def pose_local(A, B):
    return pose_logmap(pose_between(A, B))


def _rot2_normalize(c, s):
    scale = c * c + s * s
    if abs((scale - 1.0).v) > 1e-10:
        k = 1.0 / scale.sqrt()
        return c * k, s * k
    return c, s


def pose2_between_cs(xa, ya, ca, sa, xb, yb, cb, sb):
    ix = ca * (-xa) + sa * (-ya); iy = (-sa) * (-xa) + ca * (-ya)
    c, s = _rot2_normalize(ca * cb - (-sa) * sb, (-sa) * cb + ca * sb)
    return [ix + (ca * xb + sa * yb), iy + ((-sa) * xb + ca * yb), c, s]


def pose2_local(a, b):
    h = pose2_between_cs(a[0], a[1], a[2].cos(), a[2].sin(), b[0], b[1], b[2].cos(), b[2].sin())
    return [h[0], h[1], atan2(h[3], h[2])]


def pose2_retract(a, v):
    ca, sa, cv, sv = a[2].cos(), a[2].sin(), v[2].cos(), v[2].sin()
    c, s = _rot2_normalize(ca * cv - sa * sv, sa * cv + ca * sv)
    return [a[0] + (ca * v[0] + (-sa) * v[1]), a[1] + (sa * v[0] + ca * v[1]), atan2(s, c)]


def value_retract(vtype, x, d):
    """-> (y as a list of E, expmap branch or None).  Point3 sums, the camera's calibration sums and its copied entries are single
    double operations or none at all: their E holds the float64 result with a zero bound -- exact equality is demanded of them."""
    if vtype == VAR_POINT3:
        return [E(np.float64(x[i].v) + np.float64(d[i].v)) for i in range(3)], None
    if vtype == VAR_POSE2:
        return pose2_retract(x, d), None
    y, branch = pose_retract(x[:12], d[:6])
    if vtype == VAR_SFM_CAMERA:
        y = y + [E(np.float64(x[12 + i].v) + np.float64(d[6 + i].v)) for i in range(3)] + [x[15], x[16]]
    return y, branch


def value_local(vtype, x, z):
    """-> (d as a list of E, so3 branch or None, translation branch or None)"""
    if vtype == VAR_POINT3:
        return [z[i] - x[i] for i in range(3)], None, None
    if vtype == VAR_POSE2:
        return pose2_local(x, z), None, None
    d, b1, b2 = pose_local(x[:12], z[:12])
    if vtype == VAR_SFM_CAMERA:
        d = d + [z[12 + i] - x[12 + i] for i in range(3)]
    return d, b1, b2


def retract_reference(p, values, delta):
    """Values::retract of `values` by `delta` (both float64, taken as exact) -> (y, allowance) as long-double arrays, and the
    expmap branch per variable (None for Point3 / Pose2)."""
    voff, doff = p.val_offsets(), p.dim_offsets()
    y = np.zeros(values.size, LD); a = np.zeros(values.size, LD); branches = []
    for v, t in enumerate(p.var_type):
        out, br = value_retract(int(t), lift(values[voff[v]:voff[v + 1]]), lift(delta[doff[v]:doff[v + 1]]))
        y[voff[v]:voff[v + 1]] = vals(out); a[voff[v]:voff[v + 1]] = errs(out); branches.append(br)
    return y, a, branches


def prior_b_reference(p, values):
    """b = Local(x, prior) of every (unit-noise) prior -> (b [n, 9], allowance [n, 9], so3 branch, translation branch per prior)"""
    voff = p.val_offsets()
    b = np.zeros((p.n_prior, 9), LD); a = np.zeros((p.n_prior, 9), LD); b1, b2 = [], []
    for k in range(p.n_prior):
        v = int(p.prior_var[k]); t = int(p.var_type[v]); st = STORAGE[t]
        d, s1, s2 = value_local(t, lift(values[voff[v]:voff[v] + st]), lift(p.prior_data[p.prior_off[k]:p.prior_off[k] + st]))
        b[k, :len(d)] = vals(d); a[k, :len(d)] = errs(d); b1.append(s1); b2.append(s2)
    return b, a, b1, b2


def between_b_reference(p, values):
    """b = -Logmap(Z^-1 (T1^-1 T2)) of every (unit-noise) BetweenFactor<Pose3> -> (b [n, 6], allowance, so3 branch, translation branch)"""
    voff = p.val_offsets()
    n = p.n_between
    b = np.zeros((n, 6), LD); a = np.zeros((n, 6), LD); b1, b2 = [], []
    Z = p.between_z.reshape(-1, 12)
    for k in range(n):
        T1 = lift(values[voff[p.between_v1[k]]:][:12]); T2 = lift(values[voff[p.between_v2[k]]:][:12])
        r, s1, s2 = pose_local(lift(Z[k]), pose_between(T1, T2))
        b[k] = -vals(r); a[k] = errs(r); b1.append(s1); b2.append(s2)
    return b, a, b1, b2


# ------------------------------------------------------------------------------------------------------------------------
# chart designs
# ------------------------------------------------------------------------------------------------------------------------
ANGLES = (0.0, 1e-9, 1.4e-8, 1.6e-8, 1e-5, 1e-3, 1.0, 3.0, np.pi - 2e-2, np.pi - 5e-4, np.pi - 1e-5)    # 1.4e-8, 1.6e-8: either side of theta^2 = eps
AXES = np.array([[0.9, 0.3, -0.316], [-0.25, 0.92, 0.3], [0.31, -0.2, 0.93], [0.6, -0.64, 0.48]])     # each diagonal entry the largest in turn, and a generic axis
AXES = AXES / np.linalg.norm(AXES, axis=1)[:, None]
BRANCHES = ("expmap:near_zero", "expmap:general", "logmap:pi_a0", "logmap:pi_a1", "logmap:pi_a2", "logmap:acos", "logmap:taylor",
            "logmap:small_t", "logmap:general_t")
BRANCHES_POSE2 = ("pose2:wrap_up", "pose2:wrap_down", "pose2:no_wrap")
N_EDGES = 11


def _xi(i):
    w = ANGLES[i % len(ANGLES)] * AXES[(i // len(ANGLES)) % len(AXES)]
    v = np.roll(np.array([1e-3, 1.0, 50.0]) * np.array([1, -1, 1])[(np.arange(3) + i) % 3], i % 3)      # translations of mixed scale
    return np.concatenate([w, v])


def chart_design(types, edges=0):
    """Unit-noise priors z = x (+) xi on variables of the given types, xi walking ANGLES x AXES on the rotational ones; the last
    2 `edges` variables (Pose3) also carry `edges` BetweenFactor<Pose3> factors whose residual rotation walks ANGLES.  -> namespace p, values, xi (the designed steps, tangent layout), lam."""
    from oracle import gtsam_oracle as O
    types = np.asarray(types, np.int32)
    n = types.size
    rng = np.random.default_rng(1000 + n)
    p = Problem(var_type=types)
    voff, doff = p.val_offsets(), p.dim_offsets()
    values = np.zeros(int(voff[-1])); xi = np.zeros(int(doff[-1]))
    rot = 0
    for v, t in enumerate(types):
        x = values[voff[v]:voff[v + 1]]; d = xi[doff[v]:doff[v + 1]]
        if t == VAR_POINT3:
            x[:] = rng.normal(0, 3, 3); d[:] = rng.normal(0, 1, 3) * [1e-3, 1.0, 50.0]
        elif t == VAR_POSE2:
            th = (-3.1, 3.1, 0.4, -2.0, 3.0, -3.0)[v % 6]
            x[:] = [rng.normal(0, 5), rng.normal(0, 5), th]
            d[:] = [rng.normal(0, 1), rng.normal(0, 1e-3), (-0.3, 0.3, 0.5, -0.7, 2.9, -2.9)[v % 6]]      # theta + v past -pi, past +pi, inside
        else:
            R, tt = O.pose3_expmap(rng.normal(0, 1, (1, 6)) * [1.2, 1.2, 1.2, 4, 4, 4])
            x[:12] = O.pose_pack(R, tt)[0]
            d[:6] = _xi(rot); rot += 1
            if t == VAR_SFM_CAMERA:
                x[12:] = [rng.uniform(400, 900), rng.normal(0, 1e-2), rng.normal(0, 1e-3), 3.25, -7.5]
                d[6:] = [0.5, 1e-3, -1e-4]
    z = O.retract(p, values, xi)
    nz = {int(t): p.add_noise(NOISE_UNIT, TANGENT[int(t)]) for t in np.unique(types)}
    p.prior_var = np.arange(n, dtype=np.int32); p.prior_off = voff[:-1].astype(np.int64); p.prior_data = z
    p.prior_noise = np.array([nz[int(t)] for t in types], np.int32)
    if edges:
        assert (types[n - 2 * edges:] == VAR_POSE3).all()
        v1 = n - 2 * edges + 2 * np.arange(edges); v2 = v1 + 1
        T1 = values[voff[v1][:, None] + np.arange(12)]; T2 = values[voff[v2][:, None] + np.arange(12)]
        h = O.pose_pack(*O.pose_compose(*O.pose_inverse(*O.pose_unpack(T1)), *O.pose_unpack(T2)))
        Z = O.pose_retract(h, np.stack([_xi(e + (e % 4) * len(ANGLES)) for e in range(edges)]))    # Z^-1 h = Expmap(xi)^-1: the same angle
        p.between_v1 = v1.astype(np.int32); p.between_v2 = v2.astype(np.int32); p.between_z = Z.reshape(-1)
        p.between_noise = np.full(edges, nz[VAR_POSE3], np.int32)
    return SimpleNamespace(p=p, values=values, xi=xi, lam=1e-9, edges=edges)


def _interleaved(n, tail_poses=0):
    t = np.array([VAR_POSE3, VAR_SFM_CAMERA, VAR_POINT3])[np.arange(n) % 3]
    if tail_poses:
        t[n - tail_poses:] = VAR_POSE3
    return t


def _dims(total):
    """interleaved types whose tangent dimensions sum to `total` (a multiple of 3)"""
    t = []
    while total >= 18:
        t += [VAR_POSE3, VAR_SFM_CAMERA, VAR_POINT3]; total -= 18
    t += {0: [], 3: [VAR_POINT3], 6: [VAR_POSE3], 9: [VAR_SFM_CAMERA], 12: [VAR_SFM_CAMERA, VAR_POINT3], 15: [VAR_POSE3, VAR_SFM_CAMERA]}[total]
    return np.array(t)


# Variable counts at the lane / block boundaries of k_retract; user_dim_size = 255, 513, 1023 (256 k +- 1 is a multiple of 3 only there)
# for k_sumsq; Pose2 in graphs of its own (BetweenFactor decides its type by its variables, and the oracle keeps the two apart).
CHART = {
    "mixed_1": lambda: chart_design([VAR_POSE3]),
    **{f"mixed_{n}": functools.partial(lambda n: chart_design(_interleaved(n, 2 * N_EDGES), N_EDGES), n) for n in (255, 256, 257)},
    **{f"dims_{d}": functools.partial(lambda d: chart_design(_dims(d)), d) for d in (255, 513, 1023)},
    **{f"pose2_{n}": functools.partial(lambda n: chart_design(np.full(n, VAR_POSE2)), n) for n in (1, 85, 257)},
}
CHART_FULL_CENSUS = ("mixed_255", "mixed_256", "mixed_257")          # every branch of BRANCHES in ONE graph; pose2_85 / pose2_257: BRANCHES_POSE2


@functools.lru_cache(maxsize=None)
def chart(name):
    return CHART[name]()


def census_rotation(w):
    """branch of so3_expmap / pose_expmap for a rotation step w (float64, as the device sees it)"""
    w = np.asarray(w, np.float64)
    return "expmap:near_zero" if w[0] * w[0] + w[1] * w[1] + w[2] * w[2] <= EPS else "expmap:general"


def census_logmap(R, w):
    """branches of so3_logmap / pose_logmap for the rotation R (9 float64) whose Logmap came out as w: the conditions of geom.h"""
    R = np.asarray(R, np.float64)
    tr = R[0] + R[4] + R[8]
    if tr + 1.0 < 1e-3:
        a = 2 if (R[8] > R[4] and R[8] > R[0]) else 1 if R[4] > R[0] else 0
        so3 = f"logmap:pi_a{a}"
    else:
        so3 = "logmap:acos" if tr - 3.0 < -1e-6 else "logmap:taylor"
    t = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    return so3, ("logmap:small_t" if t < 1e-10 else "logmap:general_t")


def census(p, values, delta, b_prior, b_between=None):
    """How many variables / factors fall in each branch: the retraction of `values` by `delta` (expmap, Pose2 wrap) and the
    residuals of the priors and edges (logmap), from float64 inputs -- the designed step on the host, the device's own on the GPU."""
    from oracle import gtsam_oracle as O
    voff, doff = p.val_offsets(), p.dim_offsets()
    count = {b: 0 for b in BRANCHES + BRANCHES_POSE2}
    for v, t in enumerate(p.var_type):
        d = delta[doff[v]:doff[v + 1]]; x = values[voff[v]:voff[v + 1]]
        if t in (VAR_POSE3, VAR_SFM_CAMERA):
            count[census_rotation(d[:3])] += 1
        elif t == VAR_POSE2:
            s = x[2] + d[2]
            count["pose2:wrap_up" if s > np.pi else "pose2:wrap_down" if s < -np.pi else "pose2:no_wrap"] += 1
    for k in range(p.n_prior):
        v = int(p.prior_var[k]); t = int(p.var_type[v])
        if t in (VAR_POSE3, VAR_SFM_CAMERA):
            x = values[voff[v]:][:12]; z = p.prior_data[p.prior_off[k]:][:12]
            R, _ = O.pose_compose(*O.pose_inverse(*O.pose_unpack(x)), *O.pose_unpack(z))
            for b in census_logmap(R.reshape(-1), b_prior[k, :3]):
                count[b] += 1
    for k in range(p.n_between if b_between is not None else 0):
        T1 = values[voff[p.between_v1[k]]:][:12]; T2 = values[voff[p.between_v2[k]]:][:12]
        h = O.pose_compose(*O.pose_inverse(*O.pose_unpack(T1)), *O.pose_unpack(T2))
        R, _ = O.pose_compose(*O.pose_inverse(*O.pose_unpack(p.between_z.reshape(-1, 12)[k])), *h)
        for b in census_logmap(R.reshape(-1), b_between[k, :3]):
            count[b] += 1
    return count


# ------------------------------------------------------------------------------------------------------------------------
# the linear cost and the error from whitened records, in long double
# ------------------------------------------------------------------------------------------------------------------------
def record_rows(p, rec, delta=None):
    """The rows of the linear system from the device's records rec[ftype] (layout of gtg_get_jacobians; 4 = stereo): yields
    (A [n, rows, m], b [n, rows], d [n, m] or None) per group of factors, A the row's coefficients on its m tangent entries and d
    the step on those entries."""
    doff = p.dim_offsets()
    g = (lambda ids, w: delta[doff[ids][:, None] + np.arange(w)[None, :]]) if delta is not None else (lambda ids, w: None)
    cat = (lambda a, b: np.concatenate([a, b], 1)) if delta is not None else (lambda a, b: None)
    if p.n_sfm:
        J = rec[0]; n = J.shape[0]
        yield np.concatenate([J[:, :18].reshape(n, 2, 9), J[:, 18:24].reshape(n, 2, 3)], 2), J[:, 24:26], cat(g(p.sfm_cam, 9), g(p.sfm_point, 3))
    if p.n_proj:
        J = rec[1]; n = J.shape[0]
        yield np.concatenate([J[:, :12].reshape(n, 2, 6), J[:, 12:18].reshape(n, 2, 3)], 2), J[:, 18:20], cat(g(p.proj_pose, 6), g(p.proj_point, 3))
    if p.n_stereo:
        J = rec[4]; n = J.shape[0]
        yield np.concatenate([J[:, :18].reshape(n, 3, 6), J[:, 18:27].reshape(n, 3, 3)], 2), J[:, 27:30], cat(g(p.stereo_pose, 6), g(p.stereo_point, 3))
    if p.n_between:
        J = rec[2]; n = J.shape[0]
        dd = 3 if p.var_type[p.between_v1[0]] == VAR_POSE2 else 6
        yield (np.concatenate([J[:, :dd * dd].reshape(n, dd, dd), J[:, 36:36 + dd * dd].reshape(n, dd, dd)], 2), J[:, 72:72 + dd],
               cat(g(p.between_v1, dd), g(p.between_v2, dd)))
    if p.n_prior:
        J = rec[3]
        dims = np.array([TANGENT[int(t)] for t in range(4)])[p.var_type[p.prior_var]]
        for dd in np.unique(dims):
            sel = np.flatnonzero(dims == dd)
            yield J[sel, :dd * dd].reshape(sel.size, dd, dd), J[sel, 81:81 + dd], g(p.prior_var[sel], dd)


def linear_costs(p, rec, delta):
    """(0.5 sum b^2, 0.5 sum (A delta - b)^2, allowance of the second) in long double from the records and the step.
    Per row v = sum_j A_j d_j - b with m products: e_v = (m + 1) u (|b| + sum |A||d|); per square 2 |v| e_v + e_v^2 + u v^2; over the
    k squares (k + 2) u sum v^2; the factor 0.5 is exact."""
    e0 = LD(0); e1 = LD(0); allow = LD(0); k = 0
    for A, b, d in record_rows(p, rec, delta):
        A = A.astype(LD); b = b.astype(LD); d = d.astype(LD)
        v = np.einsum("nrm,nm->nr", A, d) - b
        ev = (A.shape[2] + 1) * U * (np.abs(b) + np.einsum("nrm,nm->nr", np.abs(A), np.abs(d)))
        e0 += (b * b).sum(); e1 += (v * v).sum()
        allow += (2 * np.abs(v) * ev + ev * ev + U * v * v).sum()
        k += v.size
    allow += (k + 2) * U * e1
    return 0.5 * e0, 0.5 * e1, 0.5 * allow


def error_from_records(p, rec, b_allow=None):
    """(0.5 sum b^2 over every row of the records, its allowance as the reference of error()).  error() recomputes each residual in
    another kernel: with e_b the bound of |b of the error kernel - b of the record| per row (b_allow, same grouping as record_rows;
    None: the residuals are the same doubles), a square differs by at most 2 |b| e_b + e_b^2, it is rounded once (u b^2), and the k
    squares are summed in some order: (k + 2) u sum b^2."""
    e = LD(0); allow = LD(0); k = 0
    for i, (A, b, _) in enumerate(record_rows(p, rec)):
        b = b.astype(LD)
        eb = b_allow[i] if b_allow is not None else 0.0
        e += (b * b).sum(); allow += (2 * np.abs(b) * eb + eb * eb + U * b * b).sum(); k += b.size
    allow += (k + 2) * U * e
    return 0.5 * e, 0.5 * allow


def sfm_residual_allowance(p, values):
    """Bound of the forward error of one evaluation of b = z - pi(camera, point) of every GeneralSFMFactor, from sfm_project (geom.h)
    operation by operation with magnitudes: q = R^T (p - t) is 1 + 3 roundings deep on terms of size |R|^T |p - t| =: L (4 u L per
    entry, plus u |p - t| carried through R); x = q_x / q_z: (e_qx + |x| e_qz) / q_z + 2 u |x| (reciprocal and product); r = x^2 + y^2
    and g = 1 + (k1 + k2 r) r change x by at most 8 u |g x| plus g e_x (|k1 r|, |k2 r^2| << 1 on these scenes: asserted);
    pi = u0 + f (g x): two more roundings on |u0| + |f g x|; b = z - pi: one on |z| + |pi|.  -> [n, 2]; the error kernel and the
    record kernel each stay within it, so their difference is within twice this."""
    voff = p.val_offsets()
    cam = values[voff[p.sfm_cam][:, None] + np.arange(17)].astype(LD); pt = values[voff[p.sfm_point][:, None] + np.arange(3)].astype(LD)
    R = cam[:, :9].reshape(-1, 3, 3); dx = pt - cam[:, 9:12]
    q = np.einsum("nji,nj->ni", R, dx)
    L = np.einsum("nji,nj->ni", np.abs(R), np.abs(dx))
    eq = 5 * U * L
    assert (q[:, 2] > 0).all()
    xy = q[:, :2] / q[:, 2:3]
    exy = (eq[:, :2] + np.abs(xy) * eq[:, 2:3]) / (q[:, 2:3] - eq[:, 2:3]) + 2 * U * np.abs(xy)
    r = (xy * xy).sum(1)
    f, k1, k2, u0v0 = cam[:, 12], cam[:, 13], cam[:, 14], cam[:, 15:17]
    assert (np.abs(k1 * r) + np.abs(k2 * r * r) < 0.5).all()
    g = 1 + (k1 + k2 * r) * r
    # d(g x) <= |g| e_x + |x| dg, dg <= (|k1| + 2 |k2| r) dr + roundings, dr <= 2 |x| e_x + 2 |y| e_y + roundings
    dr = 2 * (np.abs(xy) * exy).sum(1) + 3 * U * r
    dg = (np.abs(k1) + 2 * np.abs(k2) * r) * dr + 4 * U * (np.abs(k1 * r) + np.abs(k2 * r * r) + 1)
    egx = np.abs(g)[:, None] * exy + np.abs(xy) * dg[:, None] + U * np.abs(g[:, None] * xy)
    pi = u0v0 + f[:, None] * g[:, None] * xy
    epi = np.abs(f)[:, None] * egx + 2 * U * (np.abs(u0v0) + np.abs(f[:, None] * g[:, None] * xy))
    z = p.sfm_z.reshape(-1, 2).astype(LD)
    return epi + U * (np.abs(z) + np.abs(pi))


REALISTIC = ("E_bal14", "E_bal29", "D_lm65")          # designs of tests/structured.py: GeneralSFM factors (D_lm65: and two point priors)
