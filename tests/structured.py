"""Graphs with DESIGNED incidence and a long-double reference of the damped reduced system (tests only, numpy on the host).

The BAL graphs of the rest of the suite have random incidence: whether a Schur block has 16 or 17 terms, a camera 64 or 65 observations,
a landmark's observations straddle a 64-observation chunk is luck.  Here the counts are chosen (ring_scene + designed_bal), and everything
behind the per-factor records -- J^T J, J^T b, the damping, the elimination of the points, the Schur complement S, its factor and the
step -- is restated in np.longdouble from the SAME whitened records the device holds (reference_reduced_system), so that what is
compared is the association order of sums, not two linearisations.

DESIGNS (bottom of the file) names every graph that tests/test_reduced_system_reference.py proves well-posed on the host and
tests/test_gpu_reduced_system.py runs on the device.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from gtsam_amd import datasets as D
from gtsam_amd.problem import (FAC_BETWEEN_POSE3, FAC_GENERAL_SFM, FAC_PRIOR, FAC_PROJECTION, NOISE_ISOTROPIC, TANGENT, VAR_POINT3,
                               bal_problem)

U = 2.0 ** -53          # unit roundoff of float64
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------------
# scenes with full visibility and graphs with chosen counts
# ------------------------------------------------------------------------------------------------------------------------
def ring_scene(n_cams, n_points, seed):
    """Cameras on a ring of radius 30 looking at a compact cloud around the origin (every point within 5 of it on every axis): every
    (camera, point) pair is a valid observation in front of the camera.  Returns the true scene, the initial values (the truth
    perturbed as datasets.synthetic_bal perturbs it) and the seed of the pixel noise; measurements are made by designed_bal."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0, 2 * np.pi, n_cams, endpoint=False) + rng.normal(0, 0.02, n_cams)
    centers = np.stack([30 * np.cos(a), 30 * np.sin(a), rng.normal(0, 2.0, n_cams)], 1)
    fwd = rng.normal(0, 0.5, (n_cams, 3)) - centers
    fwd /= np.linalg.norm(fwd, axis=1)[:, None]
    right = np.cross(np.tile(np.array([0, 0, -1.0]), (n_cams, 1)), fwd)
    right /= np.linalg.norm(right, axis=1)[:, None]
    Rwc = np.stack([right, np.cross(fwd, right), fwd], 2)
    cams = np.zeros((n_cams, 17))
    cams[:, :9] = Rwc.reshape(-1, 9); cams[:, 9:12] = centers
    cams[:, 12] = rng.uniform(400, 900, n_cams); cams[:, 13] = rng.normal(0, 1e-2, n_cams); cams[:, 14] = rng.normal(0, 1e-4, n_cams)
    pts = np.clip(rng.normal(0, 2.0, (n_points, 3)), -5.0, 5.0)
    cams0 = cams.copy()
    cams0[:, :9] = (Rwc @ D._rodrigues(rng.normal(0, 2e-3, (n_cams, 3)))).reshape(-1, 9)
    cams0[:, 9:12] += rng.normal(0, 2e-2, (n_cams, 3))
    cams0[:, 12] += rng.normal(0, 1.0, n_cams)
    pts0 = pts + rng.normal(0, 5e-2, pts.shape)
    return SimpleNamespace(cams=cams, pts=pts, cams0=cams0, pts0=pts0, seed=seed, pixel_noise=0.5)


def designed_bal(scene, pair_counts, tracks=(), shuffle_seed=None):
    """BAL graph on `scene` with chosen incidence: for every (a, b) -> n of pair_counts, n landmarks seen by exactly cameras a and b
    (n terms of Schur block (a, b)); then one landmark per tuple of `tracks` (its cameras).  shuffle_seed: the landmarks in a seeded
    random order instead (track lengths mixed along the landmark list).  Observations sorted by point, then camera (FromBalFile).
    Returns ((Problem, values0), counts): counts.pair_terms[(a, b)], a <= b (the diagonal blocks included: that is what the device's
    block list holds), counts.cam_len[camera], counts.track_len[landmark], counts.n_pairs, counts.n_pair_terms."""
    from oracle import gtsam_oracle as O
    lms = []
    for (a, b), n in pair_counts.items():
        assert a != b and n >= 0
        lms += [(min(a, b), max(a, b))] * n
    lms += [tuple(sorted(t)) for t in tracks]
    if shuffle_seed is not None:
        lms = [lms[i] for i in np.random.default_rng(shuffle_seed).permutation(len(lms))]
    n_cams, n_lm = scene.cams.shape[0], len(lms)
    assert n_lm <= scene.pts.shape[0], "the scene has too few points for this design"
    obs_cam = np.array([c for t in lms for c in t], np.int32)
    obs_pt = np.repeat(np.arange(n_lm), [len(t) for t in lms]).astype(np.int32)
    pi, _, _, behind = O.sfm_project(scene.cams[obs_cam], scene.pts[obs_pt])
    assert not behind.any()
    noise = np.random.default_rng([scene.seed, 1]).normal(0, scene.pixel_noise, (n_cams, scene.pts.shape[0], 2))
    z = pi + noise[obs_cam, obs_pt]
    pair_terms = {}
    for t in lms:
        for i, a in enumerate(t):
            for b in t[i:]:
                pair_terms[(a, b)] = pair_terms.get((a, b), 0) + 1
    track_len = np.array([len(t) for t in lms], np.int64)
    counts = SimpleNamespace(pair_terms=pair_terms, cam_len=np.bincount(obs_cam, minlength=n_cams), track_len=track_len,
                             n_pairs=len(pair_terms), n_pair_terms=int((track_len * (track_len + 1) // 2).sum()))
    assert counts.cam_len.min() > 0, "a camera without observations"
    return bal_problem(scene.cams0, scene.pts0[:n_lm], obs_cam, obs_pt, z), counts


def recount(p):
    """The same counts read back from a BAL Problem (independent of designed_bal's bookkeeping): (pair_terms, cam_len, track_len)."""
    n_cams = int((p.var_type != VAR_POINT3).sum())
    B = np.zeros((p.n_vars - n_cams, n_cams), np.int64)
    np.add.at(B, (p.sfm_point - n_cams, p.sfm_cam), 1)
    assert B.max() == 1
    G = B.T @ B
    return {(a, b): int(G[a, b]) for a in range(n_cams) for b in range(a, n_cams) if G[a, b]}, B.sum(0), B.sum(1)


# ------------------------------------------------------------------------------------------------------------------------
# the reduced system in long double, from whitened records
# ------------------------------------------------------------------------------------------------------------------------
def oracle_records(p, values):
    """The four record tables from the host oracle, in the layout of DeviceGraph.jacobians (include/gtsam_amd.h)."""
    from oracle import gtsam_oracle as O
    return {ft: O.jacobians_flat(p, values, ft) for ft in range(4)}


def device_records(dev):
    return {ft: dev.jacobians(ft) for ft in range(4)}


def _chol3_inv(A):
    """L^-1 (lower) of the Cholesky factors A = L L^T of a stack of 3x3 matrices, closed form in their dtype.  The elimination goes
    through E = W L^-T (as choleskyPartial does): the error of E E^T is then relative to |E||E|^T, whatever the condition of A."""
    l00 = np.sqrt(A[:, 0, 0]); l10 = A[:, 1, 0] / l00; l20 = A[:, 2, 0] / l00
    l11 = np.sqrt(A[:, 1, 1] - l10 * l10); l21 = (A[:, 2, 1] - l20 * l10) / l11
    l22 = np.sqrt(A[:, 2, 2] - l20 * l20 - l21 * l21)
    if not np.all(np.isfinite(l22) & (l22 > 0)):
        raise np.linalg.LinAlgError("a damped point block is not positive definite")
    Li = np.zeros_like(A)
    Li[:, 0, 0] = 1 / l00; Li[:, 1, 1] = 1 / l11; Li[:, 2, 2] = 1 / l22
    Li[:, 1, 0] = -l10 * Li[:, 0, 0] * Li[:, 1, 1]
    Li[:, 2, 1] = -l21 * Li[:, 1, 1] * Li[:, 2, 2]
    Li[:, 2, 0] = -(l20 * Li[:, 0, 0] + l21 * Li[:, 1, 0]) * Li[:, 2, 2]
    return Li


def reference_reduced_system(p, records, order, lam, diagonal_damping, dmin=1e-6, dmax=1e32, dtype=LD, dense=True):
    """The damped reduced system of one LM try, accumulated in `dtype` (np.longdouble) from whitened per-factor records
    (records[ftype] = [n, row] in the layout of gtg_get_jacobians): full J^T J and J^T b, damping as oracle.solve_damped
    (lambda * clip(diag, dmin, dmax) or lambda), every POINT3 eliminated with a closed-form 3x3 Cholesky inverse, the reduced variables permuted into
    `order` (variable id per position: DeviceGraph.reduced_order(); None = id order).
    -> namespace: S_ref, g_ref (dense=True), a (damped pre-Schur diagonal of the reduced variables, in S's order), hdiag_ref, grad_ref
    (variable-id order) with their sum lengths hd_k / grad_k and sums of |terms| grad_abs (hdiag's terms are squares: it is its own),
    k_max (the longest sum behind any entry of S), and what solve_reference needs."""
    vt = np.asarray(p.var_type)
    is_lm = vt == VAR_POINT3
    red_vars = np.flatnonzero(~is_lm); lm_vars = np.flatnonzero(is_lm)
    nr, nl = red_vars.size, lm_vars.size
    red_index = -np.ones(p.n_vars, np.int64); red_index[red_vars] = np.arange(nr)
    lm_index = -np.ones(p.n_vars, np.int64); lm_index[lm_vars] = np.arange(nl)
    rdim = np.array([TANGENT[int(t)] for t in vt[red_vars]], np.int64)
    lam = dtype(lam)
    ar9 = np.arange(9)

    Hd = np.zeros((nr, 9, 9), dtype); g = np.zeros((nr, 9), dtype); gabs = np.zeros((nr, 9), dtype); krows = np.zeros(nr, np.int64)
    V = np.zeros((nl, 3, 3), dtype); gp = np.zeros((nl, 3), dtype); gpabs = np.zeros((nl, 3), dtype); klm = np.zeros(nl, np.int64)
    off_blocks = []                                           # (r1, r2, blocks[n, 9, 9]) of the between factors
    obs_c, obs_l, obs_W = [], [], []

    def add_red(r, A, b):                                     # A [n, rows, 9 (zero padded)], b [n, rows]
        np.add.at(Hd, r, np.einsum("nki,nkj->nij", A, A))
        np.add.at(g, r, np.einsum("nki,nk->ni", A, b))
        np.add.at(gabs, r, np.einsum("nki,nk->ni", np.abs(A), np.abs(b)))
        np.add.at(krows, r, A.shape[1])

    def add_lm(l, A, b):
        np.add.at(V, l, np.einsum("nki,nkj->nij", A, A))
        np.add.at(gp, l, np.einsum("nki,nk->ni", A, b))
        np.add.at(gpabs, l, np.einsum("nki,nk->ni", np.abs(A), np.abs(b)))
        np.add.at(klm, l, A.shape[1])

    for ft, cam, pt, dc in ((FAC_GENERAL_SFM, p.sfm_cam, p.sfm_point, 9), (FAC_PROJECTION, p.proj_pose, p.proj_point, 6)):
        J = records.get(ft)
        if J is None or not len(cam):
            continue
        J = np.asarray(J).astype(dtype)
        n = J.shape[0]
        assert n == len(cam)
        Jc = np.zeros((n, 2, 9), dtype); Jc[:, :, :dc] = J[:, :2 * dc].reshape(n, 2, dc)
        Jp = J[:, 2 * dc:2 * dc + 6].reshape(n, 2, 3); b = J[:, 2 * dc + 6:2 * dc + 8]
        r = red_index[cam]; l = lm_index[pt]
        assert (r >= 0).all() and (l >= 0).all()
        add_red(r, Jc, b); add_lm(l, Jp, b)
        obs_c.append(r); obs_l.append(l); obs_W.append(np.einsum("nki,nkj->nij", Jc, Jp))
    if p.n_between:
        J = np.asarray(records[FAC_BETWEEN_POSE3]).astype(dtype)
        n = J.shape[0]
        A1 = np.zeros((n, 6, 9), dtype); A2 = np.zeros((n, 6, 9), dtype)
        A1[:, :, :6] = J[:, :36].reshape(n, 6, 6); A2[:, :, :6] = J[:, 36:72].reshape(n, 6, 6); b = J[:, 72:78]
        r1 = red_index[p.between_v1]; r2 = red_index[p.between_v2]
        assert (rdim[r1] == 6).all() and (rdim[r2] == 6).all()
        add_red(r1, A1, b); add_red(r2, A2, b)
        off_blocks.append((r1, r2, np.einsum("nki,nkj->nij", A1, A2)))
    if p.n_prior:
        J = np.asarray(records[FAC_PRIOR]).astype(dtype)
        for k in range(p.n_prior):
            v = int(p.prior_var[k]); d = TANGENT[int(vt[v])]
            A = np.zeros((1, d, 9), dtype); A[0, :, :d] = J[k, :d * d].reshape(d, d); b = J[k, 81:81 + d][None]
            if is_lm[v]:
                add_lm(np.array([lm_index[v]]), A[:, :, :3], b)
            else:
                add_red(np.array([red_index[v]]), A, b)

    # per-variable quantities in variable-id order
    doff = p.dim_offsets(); ndim = int(doff[-1])
    hdiag = np.zeros(ndim, dtype); grad = np.zeros(ndim, dtype); grad_abs = np.zeros(ndim, dtype); kk = np.zeros(ndim, np.int64)
    for r, v in enumerate(red_vars):
        s = slice(doff[v], doff[v + 1]); d = rdim[r]
        hdiag[s] = np.diagonal(Hd[r])[:d]; grad[s] = g[r, :d]; grad_abs[s] = gabs[r, :d]; kk[s] = krows[r]
    if nl:
        idx = doff[lm_vars][:, None] + np.arange(3)[None, :]
        hdiag[idx] = np.diagonal(V, axis1=1, axis2=2); grad[idx] = gp; grad_abs[idx] = gpabs; kk[idx] = klm[:, None]

    def damp(h):
        return lam * np.minimum(np.maximum(h, dtype(dmin)), dtype(dmax)) if diagonal_damping else lam * np.ones_like(h)

    out = SimpleNamespace(hdiag_ref=hdiag, grad_ref=grad, grad_abs=grad_abs, hd_k=kk, grad_k=kk, dtype=dtype, p=p,
                          red_vars=red_vars, lm_vars=lm_vars, rdim=rdim)
    if not dense:
        return out

    hd_red = np.diagonal(Hd, axis1=1, axis2=2)                                     # [nr, 9]
    a_pad = hd_red + damp(hd_red)
    Vd = V.copy()
    if nl:
        dv = np.diagonal(V, axis1=1, axis2=2)
        Vd[:, ar9[:3], ar9[:3]] = dv + damp(dv)
    Linv = _chol3_inv(Vd) if nl else Vd
    ylm = np.einsum("nij,nj->ni", Linv, gp)

    S = np.zeros((nr * 9, nr * 9), dtype); gred = g.copy()
    blk_i = (red_index[red_vars] * 9)[:, None, None] + ar9[None, :, None]
    S[blk_i, np.swapaxes(blk_i, 1, 2)] = Hd
    di = np.arange(nr * 9)
    S[di, di] = a_pad.reshape(-1)
    for r1, r2, blocks in off_blocks:
        rows = (r1 * 9)[:, None, None] + ar9[None, :, None]; cols = (r2 * 9)[:, None, None] + ar9[None, None, :]
        np.add.at(S, (rows, cols), blocks)
        np.add.at(S, (np.swapaxes(cols, 1, 2), np.swapaxes(rows, 1, 2)), np.swapaxes(blocks, 1, 2))
    nobs = np.zeros(nr, np.int64)
    if obs_c:
        c = np.concatenate(obs_c); l = np.concatenate(obs_l); W = np.concatenate(obs_W)
        np.add.at(nobs, c, 1)
        by_lm = np.argsort(l, kind="stable")
        cnt = np.bincount(l, minlength=nl); start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        for t in np.unique(cnt[cnt > 0]):
            ls = np.flatnonzero(cnt == t)
            oi = by_lm[start[ls][:, None] + np.arange(t)[None, :]]                 # [n, t] observations of these landmarks
            E = np.einsum("ntak,nmk->ntam", W[oi], Linv[ls])                       # E = W L^-T
            for i in range(t):
                rows = (c[oi[:, i]] * 9)[:, None, None] + ar9[None, :, None]
                np.subtract.at(gred, c[oi[:, i]], np.einsum("nak,nk->na", E[:, i], ylm[ls]))
                for j in range(t):
                    cols = (c[oi[:, j]] * 9)[:, None, None] + ar9[None, None, :]
                    np.subtract.at(S, (rows, cols), np.einsum("nak,nbk->nab", E[:, i], E[:, j]))
        out.obs_c, out.obs_l, out.obs_W = c, l, W
    order = red_vars if order is None else np.asarray(order)
    assert sorted(order.tolist()) == red_vars.tolist(), "order is not a permutation of the reduced variables"
    keep = np.concatenate([red_index[v] * 9 + np.arange(rdim[red_index[v]]) for v in order])
    out.S_ref = S[np.ix_(keep, keep)]; out.g_ref = gred.reshape(-1)[keep]; out.a = a_pad.reshape(-1)[keep]
    out.keep = keep; out.Linv = Linv; out.gp = gp
    out.k_max = int((krows + 3 * nobs).max())
    return out


def cholesky_longdouble(S):
    """Lower Cholesky factor of S by columns, in S's dtype with numpy vector operations (np.linalg has no long-double path).
    Raises np.linalg.LinAlgError on a non-positive pivot."""
    S = np.asarray(S); n = S.shape[0]
    L = np.zeros_like(S)
    for j in range(n):
        col = S[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j:, j] = col / np.sqrt(col[0])
    return L


def solve_reference(ref):
    """delta (float64, variable-id order) of the system in `ref`: Cholesky + two substitutions in ref's dtype (long double: the
    column Cholesky above; float64: LAPACK), then the points by back-substitution."""
    dt = ref.dtype
    n = ref.S_ref.shape[0]
    if dt == np.float64:
        x = np.linalg.solve(ref.S_ref, ref.g_ref)
    else:
        L = cholesky_longdouble(ref.S_ref)
        y = np.zeros(n, dt)
        for i in range(n):
            y[i] = (ref.g_ref[i] - L[i, :i] @ y[:i]) / L[i, i]
        x = np.zeros(n, dt)
        for i in range(n - 1, -1, -1):
            x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    p = ref.p
    doff = p.dim_offsets()
    delta = np.zeros(int(doff[-1]), dt)
    xpad = np.zeros(ref.red_vars.size * 9, dt); xpad[ref.keep] = x
    xpad = xpad.reshape(-1, 9)
    for r, v in enumerate(ref.red_vars):
        delta[doff[v]:doff[v + 1]] = xpad[r, :ref.rdim[r]]
    if ref.lm_vars.size:
        rhs = ref.gp.copy()
        np.subtract.at(rhs, ref.obs_l, np.einsum("nak,na->nk", ref.obs_W, xpad[ref.obs_c]))
        dl = np.einsum("nji,nj->ni", ref.Linv, np.einsum("nij,nj->ni", ref.Linv, rhs))
        delta[doff[ref.lm_vars][:, None] + np.arange(3)[None, :]] = dl
    return delta.astype(np.float64)


def rho(M, S_ref, a):
    """max over the lower triangle of |M - S_ref|_ij / sqrt(a_i a_j), in units of 2^-53.  The scale is the damped PRE-Schur diagonal:
    the Schur complement cancels (S_ii / a_i goes down to 1e-3 and below), and the rounding of a subtraction is relative to what is
    subtracted."""
    E = np.abs(np.asarray(M, LD) - np.asarray(S_ref, LD)) / np.sqrt(np.outer(a, a).astype(LD))
    return float(np.tril(E).max() / U)


def rho64(p, records, order, lam, diagonal_damping, ref):
    """The same pipeline in float64 numpy from the same records (float64 sums and Schur complement, np.linalg.cholesky, L L^T) against
    the long-double S_ref: what plain double arithmetic in another association order gives on this design."""
    r64 = reference_reduced_system(p, records, order, lam, diagonal_damping, dtype=np.float64)
    L = np.linalg.cholesky(r64.S_ref).astype(LD)
    return rho(L @ L.T, ref.S_ref, ref.a)


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------------------------------
# the designs: the smallest graphs at which each kernel of the layer can still go wrong
# ------------------------------------------------------------------------------------------------------------------------
PAIR_LADDER = (1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49)     # k_schur_pairs: 16 terms per round, two per load


def _pair_ladder(n_cams, skips):
    """A: a chain of pairs (i, i + 1) whose TOTAL term counts walk PAIR_LADDER (cycled), tracks of 3 and 5 consecutive cameras on the
    well-filled part of the chain (a block's terms then come from landmarks of different track lengths), `skips` extra one-term blocks
    (i, i + 2).  n_cams and skips set the number of blocks modulo 4: the workgroup of 4 blocks and its early return."""
    want = {(i, i + 1): PAIR_LADDER[i % len(PAIR_LADDER)] for i in range(n_cams - 1)}
    tracks = [(3, 4, 5), (4, 5, 6), (7, 8, 9), (9, 10, 11), (5, 6, 7, 8, 9), (7, 8, 9, 10, 11), (16, 17, 18), (20, 21, 22, 23, 24)]
    tracks = [t for t in tracks if max(t) < n_cams]
    pc = dict(want)
    for t in tracks:
        for a, b in zip(t[:-1], t[1:]):
            pc[(a, b)] -= 1
    assert min(pc.values()) >= 0
    for s in range(skips):
        pc[(n_cams - 3 - 3 * s, n_cams - 1 - 3 * s)] = 1
    for i in range(n_cams - 15):                              # 12 more landmarks per camera with one far away: a one-term block does not
        pc[(i, i + 15)] = 12                                  # leave its cameras with 2 equations for 9 unknowns
    for i in range(n_cams - 15, 15):
        pc[(i, i + 14)] = 12
    n_lm = sum(pc.values()) + len(tracks)
    pv, counts = designed_bal(ring_scene(n_cams, n_lm, seed=11), pc, tracks)
    counts.want = want
    return pv, counts


def _heavy(terms):
    """B: 3 cameras, the three off-diagonal blocks with `terms` two-camera landmarks each."""
    pc = dict(zip(((0, 1), (0, 2), (1, 2)), terms))
    return designed_bal(ring_scene(3, sum(terms), seed=12), pc)


CAM_LADDER = (3, 63, 64, 65, 255, 256, 257)      # k_cam_fused: 64 entries per wavefront, 4 wavefronts; 3 < splits: empty ranges


def _cam_ladder(n_cams):
    """C: camera 0 has 1025 observations and shares a block with cameras 1..7, whose whole lists (CAM_LADDER) those blocks are; the
    remaining 62 go to camera 8, and cameras 8.. form a chain with 4 landmarks per block and one 3-camera track per 10 cameras."""
    pc = {(0, 1 + i): n for i, n in enumerate(CAM_LADDER)}
    pc[(0, 8)] = 1025 - sum(CAM_LADDER)
    for i in range(8, n_cams - 1):
        pc[(i, i + 1)] = 4
    tracks = [(i, i + 1, i + 2) for i in range(8, n_cams - 2, 10)]
    n_lm = sum(pc.values()) + len(tracks)
    return designed_bal(ring_scene(n_cams, n_lm, seed=13), pc, tracks)


def _cam_chain(n_cams):
    """C, 511 / 512 cameras (splits = 3 / 1): a chain whose blocks carry 1, 2, 3, 2, ... landmarks: lists of 1 to 5 entries."""
    pc = {(i, i + 1): (1, 2, 3, 2)[i % 4] for i in range(n_cams - 1)}
    return designed_bal(ring_scene(n_cams, sum(pc.values()), seed=14), pc)


def _lm_ladder(n_lm):
    """D: 70 cameras, n_lm landmarks of mixed track lengths in a seeded order, one of them seen by all 70 cameras (a track longer than
    a 64-observation chunk), point priors on the first and the last landmark."""
    n_cams = 70
    rng = np.random.default_rng(1000 + n_lm)
    tracks = [tuple(range(n_cams))]
    for i in range(0, n_cams, 2):                             # every camera in 2 or 3 tracks with its neighbours: no camera is bare
        tracks.append(tuple((i + k) % n_cams for k in range(5)))
    while len(tracks) < n_lm:
        k = int(rng.choice([2, 2, 3, 4, 5, 7, 11, 19]))
        tracks.append(tuple(rng.choice(n_cams, k, replace=False).tolist()))
    tracks = tracks[:n_lm]
    scene = ring_scene(n_cams, n_lm, seed=15)
    (p, v0), counts = designed_bal(scene, {}, tracks, shuffle_seed=7 * n_lm)
    n3 = p.add_noise(NOISE_ISOTROPIC, 3, [0.1])
    p.add_prior(n_cams, scene.pts[0], n3); p.add_prior(n_cams + n_lm - 1, scene.pts[n_lm - 1], n3)
    return (p, v0), counts


def _tile_bal(n_cams):
    """E: n_red = 9 n_cams around the 128-tile boundaries; every camera shares blocks with its two successors, some longer tracks."""
    pc = {}
    for i in range(n_cams):
        pc[(i, (i + 1) % n_cams)] = 7; pc[(i, (i + 2) % n_cams)] = 3
    pc = {(min(a, b), max(a, b)): n for (a, b), n in pc.items()}
    rng = np.random.default_rng(n_cams)
    tracks = [tuple(rng.choice(n_cams, int(k), replace=False).tolist()) for k in rng.integers(3, 7, 40)]
    n_lm = sum(pc.values()) + len(tracks)
    return designed_bal(ring_scene(n_cams, n_lm, seed=16), pc, tracks, shuffle_seed=n_cams)


def _tile_projection(n_poses):
    return D.random_projection_graph(n_poses, 200, seed=n_poses, behind=False), None


def _pose_graph(n):
    """F: datasets.random_pose_graph plus two more BetweenFactors on the already-connected pair (0, 1) -- an off-diagonal list of
    length 3 -- and edge (2, 3) entered as (3, 2) with the inverse measurement: the re-orientation after the ordering."""
    p, v0 = D.random_pose_graph(n, n // 3, seed=n)
    z = p.between_z.reshape(-1, 12).copy()
    e = int(np.flatnonzero((p.between_v1 == 2) & (p.between_v2 == 3))[0])
    R = z[e, :9].reshape(3, 3); t = z[e, 9:]
    z[e] = np.concatenate([R.T.reshape(-1), -R.T @ t])
    v1 = p.between_v1.copy(); v2 = p.between_v2.copy()
    v1[e], v2[e] = 3, 2
    e0 = int(np.flatnonzero((p.between_v1 == 0) & (p.between_v2 == 1))[0])
    extra = np.random.default_rng(n).normal(0, 0.01, (2, 3))
    z2 = np.repeat(z[e0][None], 2, 0); z2[:, 9:] += extra
    p.between_v1 = np.concatenate([v1, [0, 0]]).astype(np.int32); p.between_v2 = np.concatenate([v2, [1, 1]]).astype(np.int32)
    p.between_z = np.concatenate([z, z2]).reshape(-1)
    p.between_noise = np.concatenate([p.between_noise, p.between_noise[[e0, (e0 + 1) % len(v1)]]]).astype(np.int32)
    return (p, v0), None


# name -> (builder, identity-damping lambda, what the design is checked for).  "full": checks (a)-(e) (no PCG for graphs without
# GeneralSFM factors); "big": no dense long-double S (4 608^2), float64 reference of the step, checks (a), (b), (d).
DESIGNS = {
    "A_pairs_mod0": (lambda: _pair_ladder(30, 2), 1e-2, "full"),
    "A_pairs_mod1": (lambda: _pair_ladder(29, 1), 1e-2, "full"),
    "A_pairs_mod2": (lambda: _pair_ladder(30, 0), 1e-2, "full"),
    "A_pairs_mod3": (lambda: _pair_ladder(30, 1), 1e-2, "full"),
    "B_heavy_513_577_639": (lambda: _heavy((513, 577, 639)), 1e-2, "full"),
    "B_twin_500": (lambda: _heavy((500, 500, 500)), 1e-2, "full"),
    "B_light_341": (lambda: _heavy((341, 341, 341)), 1e-2, "full"),
    "C_cams16_splits16": (lambda: _cam_ladder(16), 1e-2, "full"),
    "C_cams100_splits11": (lambda: _cam_ladder(100), 1e-2, "full"),
    "C_cams511_splits3": (lambda: _cam_chain(511), 1e-2, "big"),
    "C_cams512_splits1": (lambda: _cam_chain(512), 1e-2, "big"),
    **{f"D_lm{n}": (functools.partial(_lm_ladder, n), 1e-2, "full") for n in (63, 64, 65, 255, 256, 257)},
    **{f"E_bal{n}": (functools.partial(_tile_bal, n), 1e-2, "full") for n in (14, 15, 29)},
    **{f"E_proj{n}": (functools.partial(_tile_projection, n), 1e-2, "full") for n in (43, 64)},
    **{f"F_pose{n}": (functools.partial(_pose_graph, n), 1e-2, "full") for n in (21, 22, 43, 64)},
}


@functools.lru_cache(maxsize=None)
def design(name):
    """-> ((Problem, values0), counts or None), built once per process."""
    return DESIGNS[name][0]()


def modes(name):
    """The (lambda, diagonal damping) pairs of a design: the project's usual first try and one identity-damped try."""
    return [(1e-4, True), (DESIGNS[name][1], False)]
