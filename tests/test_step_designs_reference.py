"""The designs and long-double references of tests/step_designs.py, on the host alone: everything tests/test_gpu_step_scalars.py
relies on is proved here without a GPU.

  exactness      every per-factor error of every exact design is the dyadic rational the builder states -- a multiple of 2^-12 --
                 according to the oracle AND to the host compile of csrc/factors.h (tests/hostmath; the stereo factors, which the
                 oracle does not restate, by the host compile alone), and the total stays below 2^53 units: every partial sum in any
                 order is exact in double.  Every row of the GeneralSFM, projection, stereo and between ranges is checked; a prior
                 range of more than 40 000 factors (one Python call per prior on either side) on its first and last 1000 and every
                 97th prior: a prior's error depends on its own row only, all rows come from one vectorised expression, and a row
                 that were not exact would fail the == of the GPU test.  The totals are exact integer sums.  What a wrong grid
                 would drop, or read a second time one stride later, changes the total.
  grid           the launch arithmetic restated in step_designs (it must follow csrc/factors.hip) puts the designs at the partial
                 counts, caps and range mixes the issue names.
  census         every branch of the chart code is populated by the designed steps.
  references     the long-double restatement agrees with the oracle within the tolerances tests/test_hostmath.py states for the same
                 functions (retract 1e-14, Logmap 1e-9 absolute, records 1e-11), and the host compile of geom.h -- the device's source
                 in IEEE double -- stays within the running-error allowance (ratio <= 1, printed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gtsam_amd.problem import VAR_POINT3, VAR_POSE3, VAR_SFM_CAMERA, Problem
from oracle import gtsam_oracle as O
from tests import step_designs as SD
from tests import stereo_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_library(name):
    so = os.path.join(ROOT, "tests", "_build", f"lib{name}.so")
    src = os.path.join(ROOT, "tests", "hostmath", f"{name}.cpp")
    deps = [src] + [os.path.join(ROOT, "gtsam_amd", "csrc", h) for h in ("geom.h", "factors.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hm():
    lib = _host_library("hostmath")
    lib.hm_prior_error.restype = C.c_double
    return lib


@pytest.fixture(scope="module")
def hms():
    lib = _host_library("hostmath_stereo")
    lib.hms_stereo.argtypes = [C.c_long] + [C.c_void_p] * 19
    return lib


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def _sample(n):
    """the rows of a prior range that the per-factor Python loops (the oracle's and the host compile's one call per prior) visit"""
    if n <= 40000:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(1000), np.arange(n - 1000, n), np.arange(0, n, 97)]))


RANGES = {"sfm": (("sfm_cam", 1), ("sfm_point", 1), ("sfm_z", 2), ("sfm_noise", 1)),
          "proj": (("proj_pose", 1), ("proj_point", 1), ("proj_z", 2), ("proj_noise", 1), ("proj_calib", 1), ("proj_sensor", 1)),
          "stereo": (("stereo_pose", 1), ("stereo_point", 1), ("stereo_z", 3), ("stereo_noise", 1), ("stereo_calib", 1), ("stereo_sensor", 1)),
          "between": (("between_v1", 1), ("between_v2", 1), ("between_z", 12), ("between_noise", 1)),
          "prior": (("prior_var", 1), ("prior_off", 1), ("prior_noise", 1))}


def _sampled(d):
    """(Problem with the sampled rows of every range, {range: rows})"""
    p = d.p
    q = Problem(var_type=p.var_type, noise_kind=p.noise_kind, noise_dim=p.noise_dim, noise_off=p.noise_off, noise_data=p.noise_data,
                noise_robust=p.noise_robust, noise_robust_param=p.noise_robust_param, calib=p.calib, calib_baseline=p.calib_baseline,
                prior_data=p.prior_data)
    rows = {}
    for name, fields in RANGES.items():
        n = getattr(p, fields[0][0]).size
        rows[name] = _sample(n) if name == "prior" else np.arange(n)      # every row of the vectorised ranges
        for f, w in fields:
            setattr(q, f, getattr(p, f).reshape(n, w)[rows[name]].reshape(-1))
    return q, rows


def _is_exact(e, want):
    k = np.asarray(e) / SD.UNIT
    return np.array_equal(e, want) and np.array_equal(k, np.floor(k))


@pytest.mark.parametrize("name", list(SD.EXACT))
def test_exact_designs_are_exact(hm, hms, name):
    d = SD.exact(name)
    p, v = d.p, d.values
    assert d.units < 2 ** 53 and d.exact / SD.UNIT == d.units                 # the total, an exact integer sum of the stated errors
    assert sum(e.size for e in d.errors.values()) == p.n_sfm + p.n_proj + p.n_stereo + p.n_between + p.n_prior
    q, rows = _sampled(d)
    # ---- the oracle (no stereo factors there: their rows are left out of its problem)
    qo = Problem(**{k: getattr(q, k) for k in q.__dataclass_fields__ if not k.startswith("stereo") and k != "calib_baseline"})
    lin = O._linearize_whitened(qo, v)
    for ft, rng in ((0, "sfm"), (1, "proj"), (2, "between"), (3, "prior")):
        if rng in d.errors:
            b = lin[ft][2]
            assert _is_exact(0.5 * (b * b).sum(1), d.errors[rng][rows[rng]]), (name, rng, "oracle")
    # ---- the host compile of factors.h
    voff = q.val_offsets(); nd = S.device_noise_data(q)
    gather = lambda ids, w: np.ascontiguousarray(v[voff[ids][:, None] + np.arange(w)[None, :]])

    def by_noise(nz, fn):
        e = np.zeros(nz.size)
        for ni in np.unique(nz):
            sel = np.flatnonzero(nz == ni)
            e[sel] = fn(sel, int(q.noise_kind[ni]), np.ascontiguousarray(nd[int(q.noise_off[ni]):][:9]) if q.noise_kind[ni] else np.zeros(1))
        return e

    if q.n_sfm:
        z = q.sfm_z.reshape(-1, 2)

        def f(sel, nk, ndk):
            e = np.zeros(sel.size)
            hm.hm_sfm_error(C.c_long(sel.size), P(gather(q.sfm_cam[sel], 17)), P(gather(q.sfm_point[sel], 3)), P(np.ascontiguousarray(z[sel])), C.c_int(nk), P(ndk), P(e))
            return e
        assert _is_exact(by_noise(q.sfm_noise, f), d.errors["sfm"][rows["sfm"]]), (name, "sfm", "host compile")
    if q.n_proj:
        z = q.proj_z.reshape(-1, 2); K9 = np.zeros(9); K9[:5] = q.calib[:5]

        def f(sel, nk, ndk):
            e = np.zeros(sel.size)
            hm.hm_proj_error(C.c_long(sel.size), P(gather(q.proj_pose[sel], 12)), P(K9), None, P(gather(q.proj_point[sel], 3)), P(np.ascontiguousarray(z[sel])), C.c_int(nk), P(ndk), P(e))
            return e
        assert _is_exact(by_noise(q.proj_noise, f), d.errors["proj"][rows["proj"]]), (name, "proj", "host compile")
    if q.n_between:
        Z = q.between_z.reshape(-1, 12)

        def f(sel, nk, ndk):
            e = np.zeros(sel.size)
            hm.hm_between_error(C.c_long(sel.size), P(gather(q.between_v1[sel], 12)), P(gather(q.between_v2[sel], 12)), P(np.ascontiguousarray(Z[sel])), C.c_int(nk), P(ndk), P(e))
            return e
        assert _is_exact(by_noise(q.between_noise, f), d.errors["between"][rows["between"]]), (name, "between", "host compile")
    if q.n_prior:
        e = np.zeros(q.n_prior)
        for k in range(q.n_prior):
            var = int(q.prior_var[k]); t = int(q.var_type[var]); ni = int(q.prior_noise[k])
            x = np.ascontiguousarray(v[voff[var]:voff[var + 1]]); z = np.ascontiguousarray(q.prior_data[q.prior_off[k]:][:x.size])
            ndk = np.ascontiguousarray(nd[int(q.noise_off[ni]):][:9]) if q.noise_kind[ni] else np.zeros(1)
            e[k] = hm.hm_prior_error(C.c_int(t), P(x), P(z), C.c_int(int(q.noise_kind[ni])), P(ndk))
        assert _is_exact(e, d.errors["prior"][rows["prior"]]), (name, "prior", "host compile")
    if q.n_stereo:
        n = q.n_stereo
        e = np.zeros(n)
        hms.hms_stereo(n, q.stereo_pose.ctypes.data, q.stereo_point.ctypes.data, q.stereo_z.ctypes.data, q.stereo_noise.ctypes.data,
                       q.stereo_calib.ctypes.data, q.stereo_sensor.ctypes.data, q.calib.ctypes.data, q.calib_baseline.ctypes.data,
                       np.zeros(12).ctypes.data, np.ascontiguousarray(v).ctypes.data, voff.ctypes.data, q.noise_kind.ctypes.data,
                       q.noise_off.ctypes.data, nd.ctypes.data, None, None, None, e.ctypes.data, None)
        assert _is_exact(e, d.errors["stereo"][rows["stereo"]]), (name, "stereo", "host compile")
    # ---- what a wrong grid or offset would lose is not zero: every range, the factors of its second grid pass (error kernels and
    # k_linear_error) and, beside a range that wraps, the whole small range carry a positive error
    g1, g2, g3 = SD.error_grids(**d.counts)
    gl = SD.linear_grid(**d.counts)
    whole = np.concatenate([d.errors["proj"], d.errors["stereo"]]) if p.n_stereo and p.n_proj else None
    for rng, e in d.errors.items():
        g = g1 if rng == "sfm" else g3 if (rng in ("proj", "stereo") and p.n_stereo) else g2
        e = whole if (whole is not None and rng in ("proj", "stereo")) else e            # (a stereo graph: one range, monocular first)
        assert e.sum() > 0 and e[0] > 0, (name, rng)
        for stride in (g * SD.K_BLOCK, gl * SD.K_BLOCK):
            assert e.size <= stride or e[stride:].sum() > 0, (name, rng, stride)
            # ... nor is it what the first pass saw one stride earlier: a pass that read factor i - stride again would change the sum
            assert e.size <= stride or e[stride:].sum() != e[:e.size - stride].sum(), (name, rng, stride)
        for stride in (SD.CAP_ERROR_STEREO * SD.K_BLOCK, SD.CAP_ERROR * SD.K_BLOCK, SD.CAP_LINEAR * SD.K_BLOCK):
            if e.size > stride + 2000:                          # no period that divides a grid stride: partials exchanged 4 k blocks apart differ
                assert not np.array_equal(e[stride:stride + 2000], e[:2000]), (name, rng, stride)
    if p.n_sfm + p.n_proj + p.n_between + p.n_prior <= 40000 and not p.n_stereo:
        assert O.error(p, v) == d.exact, name                                  # and the oracle's own sum, whatever its order


def test_designs_cover_the_grid_boundaries():
    """The restatement of grid_for / launch_error / launch_linear_error in step_designs must follow csrc/factors.hip."""
    assert (SD.K_BLOCK, SD.K_MAX_BLOCKS, SD.CAP_ERROR, SD.CAP_ERROR_STEREO, SD.CAP_LINEAR) == (256, 2048, 1024, 512, 2048)
    counts = {name: c for name, (c, _) in SD.EXACT.items()}
    grids = {name: SD.error_grids(**c) for name, c in counts.items()}
    for name, (g1, g2, g3) in grids.items():
        assert g1 + g2 + g3 <= SD.K_MAX_BLOCKS, name                           # k_final_sum's slot
    # per range: the ladder, and the cap of the kernel the range runs in (+-1 factor)
    for rng in ("n_sfm", "n_proj", "n_stereo", "n_between", "n_prior"):
        assert set(SD.LADDER) <= {c.get(rng, 0) for c in counts.values()}, rng
    # the cap of the error kernel each range runs in: k_error<1> (sfm), k_error<2> (projection without stereo factors, between, prior) ...
    mono_graphs = [c for c in counts.values() if not c.get("n_stereo")]
    for rng in ("n_sfm", "n_proj", "n_between", "n_prior"):
        assert set(SD._caps(SD.CAP_ERROR)) <= {c.get(rng, 0) for c in mono_graphs}, rng
    # ... k_error_rows3 (the whole projection range of a three-row graph) ...
    stereo_total = {c.get("n_proj", 0) + c["n_stereo"] for c in counts.values() if c.get("n_stereo")}
    assert set(SD._caps(SD.CAP_ERROR_STEREO)) <= stereo_total
    # ... and the cap of k_linear_error in EVERY one of its loops, with the linear part of the test on: the fused GeneralSFM loop (no
    # stereo factors in the graph), the stored-record one (a stereo graph), projection records of 2 and of 3 rows, between, prior
    linear = [c for n, c in counts.items() if SD.EXACT[n][1]]
    for rng in ("n_sfm", "n_proj", "n_between", "n_prior"):
        assert set(SD._caps(SD.CAP_LINEAR)) <= {c.get(rng, 0) for c in linear if not c.get("n_stereo")}, rng
    assert set(SD._caps(SD.CAP_LINEAR)) <= {c.get("n_proj", 0) + c["n_stereo"] for c in linear if c.get("n_stereo")}
    assert any(c.get("n_sfm", 0) > SD.CAP_LINEAR * SD.K_BLOCK and c.get("n_stereo") for c in linear)
    monos = {c.get("n_proj", 0) for c in counts.values() if c.get("n_stereo")}
    assert {0, 63, 64, 65} <= monos and any(m and m % SD.K_BLOCK == 0 for m in monos)
    # the linear part runs on the designs that cross the cap of k_linear_error
    assert all(SD.EXACT[f"prior_{n}"][1] for n in SD._caps(SD.CAP_LINEAR))
    # one range of 1 to 63 factors beside a range that wraps its grid: in k_error<2> (one grid, three loops) and in k_linear_error (four)
    def small_beside_wrap(c, cap, ranges):
        ns = [c.get(r, 0) for r in ranges]
        return any(0 < n <= 63 for n in ns) and max(ns) > cap * SD.K_BLOCK
    assert any(small_beside_wrap(c, SD.CAP_ERROR, ("n_proj", "n_between", "n_prior")) and not c.get("n_stereo") for c in counts.values())
    assert any(small_beside_wrap(c, SD.CAP_LINEAR, ("n_sfm", "n_proj", "n_between", "n_prior")) and SD.EXACT[n][1] for n, c in counts.items())
    # the partials: g1 + g2 at 1, 255, 256, 257 and g1 = g2 = 1024 (g1 + g2 = kMaxBlocks), with both kernels present from 255 on
    sums = {g1 + g2: (g1, g2) for g1, g2, g3 in grids.values() if (g1 and g2) or g1 + g2 == 1}
    assert {1, 255, 256, 257, SD.K_MAX_BLOCKS} <= set(sums), sorted(sums)
    assert (SD.CAP_ERROR, SD.CAP_ERROR) in set(sums.values())
    # all three groups of partials in one graph, the third behind g1 + g2
    assert any(g1 and g2 and g3 for g1, g2, g3 in grids.values())
    for name in SD.EXACT:                                                      # and the builder builds what the name says
        if SD.EXACT[name][0].get("n_prior", 0) <= 40000:
            d = SD.exact(name); c = counts[name]
            assert (d.p.n_sfm, d.p.n_proj, d.p.n_stereo, d.p.n_between, d.p.n_prior) == tuple(c.get(k, 0) for k in ("n_sfm", "n_proj", "n_stereo", "n_between", "n_prior"))
            assert d.anchored or not SD.EXACT[name][1]


def _design_census(d):
    p = d.p
    bp = O.jacobians_flat(p, d.values, 3)[:, 81:90]
    bb = O.jacobians_flat(p, d.values, 2)[:, 72:78] if p.n_between else None
    return SD.census(p, d.values, d.xi, bp, bb)


def test_branch_census_of_the_chart_designs():
    total = {}
    for name in SD.CHART:
        c = _design_census(SD.chart(name))
        print(name, c)
        for k, n in c.items():
            total[k] = total.get(k, 0) + n
        if name in SD.CHART_FULL_CENSUS:
            assert all(c[b] >= 1 for b in SD.BRANCHES), (name, c)
            assert SD.chart(name).edges == SD.N_EDGES
        if name in ("pose2_85", "pose2_257"):
            assert all(c[b] >= 1 for b in SD.BRANCHES_POSE2), (name, c)
    assert all(total[b] >= 1 for b in SD.BRANCHES + SD.BRANCHES_POSE2), total
    # the variable counts and step sizes the kernels change path at
    assert {SD.chart(f"mixed_{n}").p.n_vars for n in (1, 255, 256, 257)} == {1, 255, 256, 257}
    assert {int(SD.chart(f"dims_{n}").p.dim_offsets()[-1]) for n in (255, 513, 1023)} == {255, 513, 1023}
    for n in (255, 256, 257):                                                  # the value types interleaved: lanes of one wave diverge
        t = SD.chart(f"mixed_{n}").p.var_type
        assert set(t[:64]) == {VAR_POSE3, VAR_SFM_CAMERA, VAR_POINT3}
    # the edges' residual rotations meet every so3_logmap branch by themselves
    d = SD.chart("mixed_256")
    _, _, b1, b2 = SD.between_b_reference(d.p, d.values)
    assert {"pi_a0", "pi_a1", "pi_a2", "acos", "taylor"} <= set(b1) and {"small_t", "general_t"} <= set(b2)


def _ratio(what, got, ref, allow):
    allow = np.asarray(allow, np.longdouble)
    r = np.abs(np.asarray(got, np.longdouble) - ref) / np.where(allow > 0, allow, SD.U * 2.0 ** -1000)
    r = np.where((allow == 0) & (np.asarray(got, np.longdouble) == ref), 0, r)
    print(f"{what}: worst |error| / allowance = {float(r.max()):.3f} at entry {int(np.argmax(r))}")
    return float(r.max())


@pytest.mark.parametrize("name", list(SD.CHART))
def test_long_double_references_against_oracle_and_host_compile(hm, name):
    d = SD.chart(name)
    p, v, xi = d.p, d.values, d.xi
    voff, doff = p.val_offsets(), p.dim_offsets()
    # ---- retraction
    y, ay, _ = SD.retract_reference(p, v, xi)
    yo = O.retract(p, v, xi)
    # (1e-14 of the largest entry, as tests/test_hostmath.py has it.  Just above theta^2 = eps the translation of pose_expmap cancels to
    # a relative u / theta ~ 1e-8 in ANY double evaluation, the oracle's included: on the entries whose allowance exceeds the stated
    # tolerance -- and on those alone -- the oracle's own rounding, bounded like the device's by the allowance, is granted on top,
    # twice for its other order of operations.)
    tol = 1e-14 * np.abs(yo).max()
    loose = ay > tol
    miss = np.abs(y - yo) - np.where(loose, 2 * ay, 0)
    print(f"{name}: retract against the oracle: worst |error| {float(np.abs(y - yo)[~loose].max(initial=0)):.2e} of {tol:.2e} allowed; "
          f"{int(loose.sum())} of {loose.size} entries cancel beyond that and are held to 1e-14 + 2 allowances (worst allowance {float(ay.max()):.2e})")
    assert float(miss.max()) <= tol
    yh = np.zeros_like(v)
    for i, t in enumerate(p.var_type):
        out = np.zeros(int(voff[i + 1] - voff[i]))
        hm.hm_retract(C.c_int(int(t)), C.c_long(1), P(np.ascontiguousarray(v[voff[i]:voff[i + 1]])), P(np.ascontiguousarray(xi[doff[i]:doff[i + 1]])), P(out))
        yh[voff[i]:voff[i + 1]] = out
    assert _ratio(f"{name}: retract, host compile", yh, y, ay) <= 1.0
    # ---- Logmap of the priors' and edges' residual rotations, and the b rows of the records
    b, ab, b1, _ = SD.prior_b_reference(p, v)
    Jo = O.jacobians_flat(p, v, 3)
    assert S.rel(b.astype(np.float64), Jo[:, 81:90]) <= 1e-11
    bh = np.zeros((p.n_prior, 9))
    for k in range(p.n_prior):
        var = int(p.prior_var[k]); t = int(p.var_type[var])
        x = np.ascontiguousarray(v[voff[var]:voff[var + 1]]); z = np.ascontiguousarray(p.prior_data[p.prior_off[k]:][:x.size])
        out = np.zeros(9); hm.hm_local(C.c_int(t), C.c_long(1), P(x), P(z), P(out)); bh[k] = out
        if t in (VAR_POSE3, VAR_SFM_CAMERA):
            Rx, tx = O.pose_unpack(x[:12]); Rz, tz = O.pose_unpack(z[:12])
            R, _ = O.pose_compose(*O.pose_inverse(Rx, tx), Rz, tz)
            w, _ = SD.so3_logmap(SD.lift(R))
            assert np.abs(SD.vals(w).astype(np.float64) - O.so3_logmap(R)[0]).max() <= 1e-9
    assert _ratio(f"{name}: Local of the priors, host compile", bh, b, ab) <= 1.0
    if p.n_between:
        bb, abb, _, _ = SD.between_b_reference(p, v)
        assert S.rel(bb.astype(np.float64), O.jacobians_flat(p, v, 2)[:, 72:78]) <= 1e-11
        n = p.n_between
        J = np.zeros((n, 78))
        T1 = np.ascontiguousarray(v[voff[p.between_v1][:, None] + np.arange(12)]); T2 = np.ascontiguousarray(v[voff[p.between_v2][:, None] + np.arange(12)])
        hm.hm_between_linearize(C.c_long(n), P(T1), P(T2), P(np.ascontiguousarray(p.between_z)), C.c_int(0), P(np.zeros(1)), P(J))
        assert _ratio(f"{name}: b of the edges, host compile", J[:, 72:78], bb, abb) <= 1.0


def test_realistic_designs_have_plain_models_and_points_in_front():
    from tests import structured as T
    for name in SD.REALISTIC:
        (p, v0), _ = T.design(name)
        assert not np.any(p.noise_robust) and p.n_sfm and not (p.n_proj or p.n_between)
        a = SD.sfm_residual_allowance(p, v0)                                     # (asserts every point in front of its camera)
        assert a.shape == (p.n_sfm, 2) and float(a.max()) < 1e-9                 # pixels: the residuals are of order one
