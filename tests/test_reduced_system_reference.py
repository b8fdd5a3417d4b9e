"""Host-only: keeps tests/structured.py honest and proves that every design tests/test_gpu_reduced_system.py runs on the device is
well-posed FOR THE REFERENCE ALONE -- with records from the host oracle instead of the device.

Per design x (lambda, damping mode): oracle.solve_damped returns status 0, the long-double Cholesky of S_ref succeeds, the long-double
step equals solve_damped's within the project's 1e-7 in max-norm, and the designed counts are what the Problem contains.  A design for
which the reference did not factorise was replaced, not skipped: no case is left out on the device.  The two 4 608-dimensional chains
("big") have no dense long-double S: their float64 reference of the step is checked here against oracle.solve_damped on the 100-camera
design, and on themselves only for a successful float64 factorisation.

rho64 (printed per design, run with -s): the same pipeline in float64 numpy from the same records -- float64 Schur complement,
np.linalg.cholesky, L L^T -- against S_ref in the scale of structured.rho.  It is the yardstick the device test's bound is made of."""
import numpy as np
import pytest

from tests import structured as T

FULL = [n for n, d in T.DESIGNS.items() if d[2] == "full"]
BIG = [n for n, d in T.DESIGNS.items() if d[2] == "big"]


@pytest.fixture(scope="module")
def records():
    cache = {}

    def get(name):
        if name not in cache:
            (p, v0), _ = T.design(name)
            cache[name] = T.oracle_records(p, v0)
        return cache[name]
    return get


def _n_pairs_mod(name):
    return T.design(name)[1].n_pairs % 4


def test_designed_counts_are_what_the_problems_contain():
    for name in T.DESIGNS:
        (p, v0), counts = T.design(name)
        if counts is None:
            continue
        pair_terms, cam_len, track_len = T.recount(p)
        assert pair_terms == counts.pair_terms, name
        assert np.array_equal(cam_len, counts.cam_len) and np.array_equal(track_len, counts.track_len), name
        assert counts.n_pairs == len(pair_terms) and counts.n_pair_terms == sum(pair_terms.values()), name
        oc, op = p.sfm_cam, p.sfm_point                      # sorted by point, then camera
        assert np.all((np.diff(op) > 0) | ((np.diff(op) == 0) & (np.diff(oc) > 0))), name


def test_designs_hit_the_chunk_boundaries_they_are_named_for():
    # A: the chain blocks walk the ladder whatever the tracks add; the four variants cover the workgroup's early return
    for m in range(4):
        c = T.design(f"A_pairs_mod{m}")[1]
        assert c.n_pairs % 4 == m
        assert all(c.pair_terms[k] == n for k, n in c.want.items())
        assert set(T.PAIR_LADDER) <= set(c.want.values())
        assert {3, 5} <= set(c.track_len.tolist())
    # B: k_schur_pairs_heavy is chosen when n_pair_terms > 512 n_pairs; the device's block list holds the diagonal blocks too (6 blocks,
    # 3 terms per two-camera landmark), so 3 x 500 landmarks are heavy as well and the light twin of the shape has 3 x 341
    c = T.design("B_heavy_513_577_639")[1]
    assert [c.pair_terms[k] for k in ((0, 1), (0, 2), (1, 2))] == [513, 577, 639] and c.n_pairs == 6
    assert c.n_pair_terms == 3 * 1729 > 512 * c.n_pairs
    c = T.design("B_twin_500")[1]
    assert c.n_pair_terms == 4500 > 512 * c.n_pairs
    c = T.design("B_light_341")[1]
    assert c.n_pair_terms == 3069 <= 512 * c.n_pairs
    # C: the list lengths of the ladder; splits as launch_assemble computes it
    for name, n_cams, splits in (("C_cams16_splits16", 16, 16), ("C_cams100_splits11", 100, 11), ("C_cams511_splits3", 511, 3),
                                 ("C_cams512_splits1", 512, 1)):
        c = T.design(name)[1]
        assert c.cam_len.size == n_cams and (1 if n_cams >= 512 else min(16, (1024 + n_cams - 1) // n_cams)) == splits
        if n_cams <= 100:
            assert c.cam_len[:8].tolist() == [1025, 3, 63, 64, 65, 255, 256, 257]
        else:
            assert c.cam_len.min() < 3 <= c.cam_len.max()      # lists shorter than splits = 3: empty ranges
    # D: one track longer than a chunk, mixed lengths, observations of one landmark on both sides of a 64-observation chunk boundary of
    # its wavefront's stretch (k_lm_fused: 64 landmarks per wavefront), point priors on the first and the last landmark
    for n_lm in (63, 64, 65, 255, 256, 257):
        (p, v0), c = T.design(f"D_lm{n_lm}")
        assert c.track_len.size == n_lm and c.track_len.max() == 70 and np.unique(c.track_len).size >= 5
        ptr = np.concatenate([[0], np.cumsum(c.track_len)])
        straddle = 0
        for g0 in range(0, n_lm, 64):
            rel0 = ptr[g0:min(g0 + 64, n_lm)] - ptr[g0]; rel1 = ptr[g0 + 1:min(g0 + 64, n_lm) + 1] - 1 - ptr[g0]
            straddle += int((rel0 // 64 != rel1 // 64).sum())
        assert straddle >= 3
        assert sorted(p.prior_var.tolist()) == [70, 70 + n_lm - 1]
    # E / F: the dimension of the reduced system against the 128-tile
    dims = {"E_bal14": 126, "E_bal15": 135, "E_bal29": 261, "E_proj43": 258, "E_proj64": 384, "F_pose21": 126, "F_pose22": 132,
            "F_pose43": 258, "F_pose64": 384}
    for name, n_red in dims.items():
        p = T.design(name)[0][0]
        assert sum(T.TANGENT[int(t)] for t in p.var_type if t != T.VAR_POINT3) == n_red
    for n in (21, 22, 43, 64):
        p = T.design(f"F_pose{n}")[0][0]
        assert ((p.between_v1 == 0) & (p.between_v2 == 1)).sum() >= 3 and ((p.between_v1 == 3) & (p.between_v2 == 2)).sum() == 1


@pytest.mark.parametrize("name", FULL)
def test_reference_is_well_posed_and_agrees_with_the_oracle(name, records):
    from oracle import gtsam_oracle as O
    (p, v0), _ = T.design(name)
    rec = records(name)
    for lam, diag in T.modes(name):
        st, delta, H, g, _ = O.solve_damped(p, v0, lam, diag)
        assert st == 0, (name, lam, diag)
        ref = T.reference_reduced_system(p, rec, None, lam, diag)
        assert T.rel(ref.hdiag_ref, np.diag(H)) <= 1e-13 and T.rel(ref.grad_ref, g) <= 1e-12
        d = T.solve_reference(ref)                                  # (cholesky_longdouble raises if S_ref does not factorise)
        assert T.rel(d, delta) <= 1e-7, (name, lam, diag, T.rel(d, delta))
        r64 = T.rho64(p, rec, None, lam, diag, ref)
        print(f"rho64 {name:24s} lambda {lam:g} {'diagonal' if diag else 'identity'}: {r64:8.2f}   n_red {ref.S_ref.shape[0]}"
              f" k_max {ref.k_max}  min S_ii/a_i {float((np.diagonal(ref.S_ref) / ref.a).min()):.2e}")
        assert r64 <= ref.S_ref.shape[0] + ref.k_max + 16           # the hard cap of the device test holds for plain float64


def test_float64_step_reference_of_the_big_chains(records):
    """The float64 reference of the step that the 511- and 512-camera designs use, against oracle.solve_damped where that is affordable
    (the 100-camera design), and its factorisation on the chains themselves."""
    from oracle import gtsam_oracle as O
    name = "C_cams100_splits11"
    (p, v0), _ = T.design(name)
    for lam, diag in T.modes(name):
        st, delta, *_ = O.solve_damped(p, v0, lam, diag)
        ref = T.reference_reduced_system(p, records(name), None, lam, diag, dtype=np.float64)
        assert st == 0 and T.rel(T.solve_reference(ref), delta) <= 1e-7
    for name in BIG:
        (p, v0), _ = T.design(name)
        for lam, diag in T.modes(name):
            ref = T.reference_reduced_system(p, records(name), None, lam, diag, dtype=np.float64)
            np.linalg.cholesky(ref.S_ref)
            assert np.all(np.isfinite(T.solve_reference(ref)))


def test_cholesky_longdouble_and_rho():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(40, 40)); S = (A @ A.T + 40 * np.eye(40)).astype(np.longdouble)
    L = T.cholesky_longdouble(S)
    assert np.array_equal(L, np.tril(L))
    assert float(np.abs(L @ L.T - S).max()) <= 40 * 2.0 ** -63 * float(np.abs(S).max())
    assert np.abs(L.astype(float) - np.linalg.cholesky(S.astype(float))).max() <= 1e-13
    with pytest.raises(np.linalg.LinAlgError):
        T.cholesky_longdouble(np.array([[1.0, 2.0], [2.0, 1.0]], np.longdouble))
    a = np.diagonal(S)
    assert T.rho(S, S, a) == 0.0
    M = S.copy(); M[7, 3] += np.sqrt(a[7] * a[3]) * 2.0 ** -50
    assert abs(T.rho(M, S, a) - 8.0) < 1e-3
    M = S.copy(); M[3, 7] += 1.0                                    # the strict upper triangle is not looked at
    assert T.rho(M, S, a) == 0.0
