"""Synthetic stand-ins for the datasets the reference's configs name but this image does not ship
(no network): BAL Ladybug-1723 / Venice-1778 / Dubrovnik-16 shapes and small seeded graphs for tests.

The BAL generator follows SURVEY.md section 8(d): cameras on a closed multi-loop street path so that
distant cameras share points (non-banded reduced camera system), long-tailed track lengths
(2 + Exp(mean) capped, >= 1 % of points seen by > 50 cameras to emulate loop closures),
f ~ U(400, 900), small radial distortion, 0.5 px pixel noise, perturbed initial values.
Everything is seeded and generated with numpy on the host; nothing here is on the hot path.
"""
from __future__ import annotations

import numpy as np

from .problem import (NOISE_DIAGONAL, NOISE_GAUSSIAN, NOISE_ISOTROPIC, NOISE_UNIT, Problem, bal_problem,
                      pose_graph_problem)


def _rodrigues(w):
    """exp map for host-side data generation only (not the device formula)."""
    w = np.asarray(w, np.float64).reshape(-1, 3)
    th = np.linalg.norm(w, axis=1)
    k = w / np.where(th > 1e-12, th, 1.0)[:, None]
    K = np.zeros((w.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    s, c = np.sin(th)[:, None, None], np.cos(th)[:, None, None]
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K)


def synthetic_bal(n_cams, n_points, mean_track=4.34, seed=42, long_frac=0.012, pixel_noise=0.5,
                  n_loops=3):
    """Returns (cams17 initial, pts3 initial, obs_cam, obs_pt, obs_z) with observations sorted by point
    then camera, the order SfmData::FromBalFile produces (sfm/SfmData.cpp:189-246)."""
    rng = np.random.default_rng(seed)
    # camera path: n_loops laps around a rounded block, slightly different radii -> revisits
    s = np.linspace(0, n_loops * 2 * np.pi, n_cams, endpoint=False)
    radius = 60.0 + 4.0 * np.sin(3 * s) + 1.5 * (s / (2 * np.pi))
    centers = np.stack([radius * np.cos(s), radius * np.sin(s), 1.5 + 0.2 * np.sin(5 * s)], 1)
    heading = s + np.pi / 2 + rng.normal(0, 0.05, n_cams)        # drive direction
    # Ladybug is omnidirectional: each "camera" looks sideways-ish with a random yaw offset
    yaw = heading + rng.uniform(-np.pi, np.pi, n_cams)
    # camera frame: z forward (optical axis), x right, y down
    fwd = np.stack([np.cos(yaw), np.sin(yaw), np.zeros(n_cams)], 1)
    down = np.tile(np.array([0, 0, -1.0]), (n_cams, 1))
    right = np.cross(down, fwd)
    Rwc = np.stack([right, down, fwd], 2)                         # columns = camera axes in world
    tilt = _rodrigues(rng.normal(0, 0.03, (n_cams, 3)))
    Rwc = Rwc @ tilt
    f = rng.uniform(400, 900, n_cams)
    k1 = rng.normal(0, 1e-2, n_cams)
    k2 = rng.normal(0, 1e-4, n_cams)

    # points: scattered in an annulus around the path (building facades both sides)
    ang = rng.uniform(0, 2 * np.pi, n_points)
    rad = 60.0 + rng.choice([-1, 1], n_points) * rng.uniform(6, 25, n_points)
    pts = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(0, 12, n_points)], 1)

    # track lengths: 2 + Exp, long tail
    k = 2 + np.floor(rng.exponential(mean_track - 1.72 - 50 * long_frac, n_points)).astype(np.int64)
    long_idx = rng.choice(n_points, max(1, int(long_frac * n_points)), replace=False)
    k[long_idx] = rng.integers(50, 120, long_idx.size)
    k = np.minimum(k, n_cams)

    # candidate cameras for a point: those whose centre is close in angle (any lap) and that see it
    cam_ang = np.mod(s, 2 * np.pi)
    order = np.argsort(cam_ang)
    sorted_ang = cam_ang[order]
    obs_cam, obs_pt = [], []
    for j in range(n_points):
        width = 0.07 + 0.004 * k[j] + 3.0 * (2 * np.pi * n_loops / n_cams)
        lo = np.searchsorted(sorted_ang, ang[j] - width)
        hi = np.searchsorted(sorted_ang, ang[j] + width)
        cand = order[lo:hi]
        if ang[j] - width < 0:
            cand = np.concatenate([cand, order[np.searchsorted(sorted_ang, ang[j] - width + 2 * np.pi):]])
        if ang[j] + width > 2 * np.pi:
            cand = np.concatenate([cand, order[:np.searchsorted(sorted_ang, ang[j] + width - 2 * np.pi)]])
        if cand.size == 0:
            cand = order[[lo % n_cams]]
        # keep those with the point in front and within a generous field of view
        d = pts[j] - centers[cand]
        zc = np.einsum("ni,ni->n", d, Rwc[cand][:, :, 2])
        xc = np.einsum("ni,ni->n", d, Rwc[cand][:, :, 0])
        ok = (zc > 1.0) & (np.abs(xc) < 1.2 * zc)
        good = cand[ok]
        if good.size < 2:
            # force visibility: re-aim nothing, just take nearest cameras in front
            good = cand[zc > 0.5]
        if good.size < 2:
            continue
        take = rng.choice(good, min(k[j], good.size), replace=False)
        take.sort()
        obs_cam.append(take); obs_pt.append(np.full(take.size, j))
    obs_cam = np.concatenate(obs_cam); obs_pt_raw = np.concatenate(obs_pt)
    # drop unobserved points, renumber
    used = np.unique(obs_pt_raw)
    remap = -np.ones(n_points, np.int64); remap[used] = np.arange(used.size)
    obs_pt = remap[obs_pt_raw]; pts = pts[used]
    # drop cameras that ended up without observations (tiny configs), renumber
    usedc = np.unique(obs_cam)
    if usedc.size != n_cams:
        remapc = -np.ones(n_cams, np.int64); remapc[usedc] = np.arange(usedc.size)
        obs_cam = remapc[obs_cam]
        centers, Rwc, f, k1, k2 = centers[usedc], Rwc[usedc], f[usedc], k1[usedc], k2[usedc]
        n_cams = usedc.size

    # ground-truth projection (host-side generation only)
    Rcw = np.swapaxes(Rwc, 1, 2)
    q = np.einsum("nij,nj->ni", Rcw[obs_cam], pts[obs_pt] - centers[obs_cam])
    x, y = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    r2 = x * x + y * y
    g = 1 + (k1[obs_cam] + k2[obs_cam] * r2) * r2
    z = np.stack([f[obs_cam] * g * x, f[obs_cam] * g * y], 1) + rng.normal(0, pixel_noise, (obs_cam.size, 2))

    # initial values = truth perturbed
    dR = _rodrigues(rng.normal(0, 2e-3, (n_cams, 3)))
    cams = np.zeros((n_cams, 17))
    cams[:, :9] = (Rwc @ dR).reshape(-1, 9)
    cams[:, 9:12] = centers + rng.normal(0, 2e-2, (n_cams, 3))
    cams[:, 12] = f + rng.normal(0, 1.0, n_cams); cams[:, 13] = k1; cams[:, 14] = k2
    pts0 = pts + rng.normal(0, 5e-2, pts.shape)
    return cams, pts0, obs_cam.astype(np.int32), obs_pt.astype(np.int32), z


def synthetic_bal_streets(n_cams, n_points, mean_track=4.34, seed=42, grid=5, block=45.0, pixel_noise=0.5, long_frac=0.012):
    """A second BAL shape for the sensitivity of the ordering / tile design to the co-visibility structure (hard
    part 8): the cameras drive a RANDOM WALK through a grid x grid street network (no U-turns), so streets are revisited at random
    times and in both directions -- long-range loop closures all over the reduced camera system instead of the cyclic band of
    synthetic_bal's laps around one block.  Landmarks sit on the facades (6-25 m off a street's centre line); a landmark is seen
    by cameras within 35 m that have it in front and in their field of view, 2 + Exp(mean) of them (long tail as in
    synthetic_bal).  Same camera model, noise, perturbation and return convention as synthetic_bal."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    # ---- the drive: node to node on the grid, one camera every `step` metres
    n_edges_needed = 4 * grid * grid
    step = n_edges_needed * block / n_cams
    node = np.array([rng.integers(0, grid + 1), rng.integers(0, grid + 1)])
    prev_dir = None
    centers, headings = [], []
    carry = 0.0
    dirs = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]])
    while len(centers) < n_cams:
        ok = [d for d in dirs if 0 <= node[0] + d[0] <= grid and 0 <= node[1] + d[1] <= grid and (prev_dir is None or not np.array_equal(d, -prev_dir))]
        d = ok[rng.integers(0, len(ok))]
        a, b = node * block, (node + d) * block
        t = carry
        while t < block and len(centers) < n_cams:
            c = a + (b - a) * (t / block)
            centers.append([c[0] + rng.normal(0, 0.3), c[1] + rng.normal(0, 0.3), 1.5 + 0.2 * rng.normal()])
            headings.append(np.arctan2(d[1], d[0]))
            t += step
        carry = t - block
        node = node + d; prev_dir = d
    centers = np.array(centers); heading = np.array(headings) + rng.normal(0, 0.05, n_cams)
    yaw = heading + rng.uniform(-np.pi, np.pi, n_cams)                   # omnidirectional rig: a random viewing direction per camera
    fwd = np.stack([np.cos(yaw), np.sin(yaw), np.zeros(n_cams)], 1)
    down = np.tile(np.array([0, 0, -1.0]), (n_cams, 1))
    right = np.cross(down, fwd)
    Rwc = np.stack([right, down, fwd], 2) @ _rodrigues(rng.normal(0, 0.03, (n_cams, 3)))
    f = rng.uniform(400, 900, n_cams); k1 = rng.normal(0, 1e-2, n_cams); k2 = rng.normal(0, 1e-4, n_cams)
    # ---- landmarks on the facades of the streets that were driven
    anchor = centers[rng.integers(0, n_cams, n_points)]
    side = rng.uniform(0, 2 * np.pi, n_points)
    off = rng.uniform(6, 25, n_points)
    pts = np.stack([anchor[:, 0] + off * np.cos(side), anchor[:, 1] + off * np.sin(side), rng.uniform(0, 12, n_points)], 1)
    k = 2 + np.floor(rng.exponential(mean_track - 1.72 - 50 * long_frac, n_points)).astype(np.int64)
    long_idx = rng.choice(n_points, max(1, int(long_frac * n_points)), replace=False)
    k[long_idx] = rng.integers(50, 120, long_idx.size)
    tree = cKDTree(centers[:, :2])
    cand_all = tree.query_ball_point(pts[:, :2], r=35.0)
    obs_cam, obs_pt = [], []
    for j in range(n_points):
        cand = np.asarray(cand_all[j], np.int64)
        if cand.size < 2:
            continue
        d = pts[j] - centers[cand]
        zc = np.einsum("ni,ni->n", d, Rwc[cand][:, :, 2]); xc = np.einsum("ni,ni->n", d, Rwc[cand][:, :, 0])
        good = cand[(zc > 1.0) & (np.abs(xc) < 1.2 * zc)]
        if good.size < 2:
            continue
        take = rng.choice(good, min(k[j], good.size), replace=False); take.sort()
        obs_cam.append(take); obs_pt.append(np.full(take.size, j))
    obs_cam = np.concatenate(obs_cam); obs_pt_raw = np.concatenate(obs_pt)
    used = np.unique(obs_pt_raw)
    remap = -np.ones(n_points, np.int64); remap[used] = np.arange(used.size)
    obs_pt = remap[obs_pt_raw]; pts = pts[used]
    usedc = np.unique(obs_cam)
    if usedc.size != n_cams:
        remapc = -np.ones(n_cams, np.int64); remapc[usedc] = np.arange(usedc.size)
        obs_cam = remapc[obs_cam]
        centers, Rwc, f, k1, k2 = centers[usedc], Rwc[usedc], f[usedc], k1[usedc], k2[usedc]
        n_cams = usedc.size
    Rcw = np.swapaxes(Rwc, 1, 2)
    q = np.einsum("nij,nj->ni", Rcw[obs_cam], pts[obs_pt] - centers[obs_cam])
    x, y = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    r2 = x * x + y * y
    g = 1 + (k1[obs_cam] + k2[obs_cam] * r2) * r2
    z = np.stack([f[obs_cam] * g * x, f[obs_cam] * g * y], 1) + rng.normal(0, pixel_noise, (obs_cam.size, 2))
    dR = _rodrigues(rng.normal(0, 2e-3, (n_cams, 3)))
    cams = np.zeros((n_cams, 17))
    cams[:, :9] = (Rwc @ dR).reshape(-1, 9)
    cams[:, 9:12] = centers + rng.normal(0, 2e-2, (n_cams, 3))
    cams[:, 12] = f + rng.normal(0, 1.0, n_cams); cams[:, 13] = k1; cams[:, 14] = k2
    pts0 = pts + rng.normal(0, 5e-2, pts.shape)
    return cams, pts0, obs_cam.astype(np.int32), obs_pt.astype(np.int32), z


def streets_1723(seed=42):
    """The L1723 size (1 723 cameras, ~156 000 points, ~4.3 observations per point) on the street-network drive."""
    return synthetic_bal_streets(1723, 156502, mean_track=4.34, seed=seed)


def ladybug_1723(seed=42):
    """BAL Ladybug problem-1723-156502 shape (1723 cameras, 156 502 points, ~678 718 obs)."""
    return synthetic_bal(1723, 156502, mean_track=4.34, seed=seed)


def venice_1778(seed=42):
    return synthetic_bal(1778, 993923, mean_track=5.03, seed=seed)


def synthetic_bal_convergent(n_cams, n_points, mean_track, seed=42, pixel_noise=0.5):
    """A few cameras on a ring looking at one scene (the geometry of the small Dubrovnik problems): every camera sees
    every point, a point is observed by 2 + Exp cameras.  Same return convention as synthetic_bal."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0, 2 * np.pi, n_cams, endpoint=False) + rng.normal(0, 0.05, n_cams)
    centers = np.stack([30 * np.cos(a), 30 * np.sin(a), rng.normal(0, 2.0, n_cams)], 1)
    target = rng.normal(0, 1.0, (n_cams, 3))
    fwd = target - centers; fwd /= np.linalg.norm(fwd, axis=1)[:, None]
    down = np.tile(np.array([0, 0, -1.0]), (n_cams, 1))
    right = np.cross(down, fwd); right /= np.linalg.norm(right, axis=1)[:, None]
    down = np.cross(fwd, right)
    Rwc = np.stack([right, down, fwd], 2)
    f = rng.uniform(400, 900, n_cams); k1 = rng.normal(0, 1e-2, n_cams); k2 = rng.normal(0, 1e-4, n_cams)
    pts = rng.normal(0, 4.0, (n_points, 3))
    k = np.minimum(2 + np.floor(rng.exponential(mean_track - 2.0, n_points)).astype(np.int64), n_cams)
    obs_cam = np.concatenate([np.sort(rng.choice(n_cams, kk, replace=False)) for kk in k])
    obs_pt = np.repeat(np.arange(n_points), k)
    Rcw = np.swapaxes(Rwc, 1, 2)
    q = np.einsum("nij,nj->ni", Rcw[obs_cam], pts[obs_pt] - centers[obs_cam])
    x, y = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    r2 = x * x + y * y
    g = 1 + (k1[obs_cam] + k2[obs_cam] * r2) * r2
    z = np.stack([f[obs_cam] * g * x, f[obs_cam] * g * y], 1) + rng.normal(0, pixel_noise, (obs_cam.size, 2))
    dR = _rodrigues(rng.normal(0, 2e-3, (n_cams, 3)))
    cams = np.zeros((n_cams, 17))
    cams[:, :9] = (Rwc @ dR).reshape(-1, 9)
    cams[:, 9:12] = centers + rng.normal(0, 2e-2, (n_cams, 3))
    cams[:, 12] = f + rng.normal(0, 1.0, n_cams); cams[:, 13] = k1; cams[:, 14] = k2
    return cams, pts + rng.normal(0, 5e-2, pts.shape), obs_cam.astype(np.int32), obs_pt.astype(np.int32), z


def dubrovnik_16(seed=42):
    """BAL Dubrovnik problem-16-22106 shape (16 cameras, 22 106 points, ~83 718 observations)."""
    return synthetic_bal_convergent(16, 22106, mean_track=4.29, seed=seed)


def random_pose_graph(n, n_closures, seed=0, noise="mixed", rot_scale=1.0, init_noise=0.2):
    """Small seeded Pose3 graph: chain + loop closures, prior on pose 0.  Returns (Problem, values0)."""
    rng = np.random.default_rng(seed)
    xi = rng.normal(size=(n, 6)); xi[:, :3] *= rot_scale
    R = _rodrigues(xi[:, :3]); t = xi[:, 3:] * 2.0
    poses = np.concatenate([R.reshape(n, 9), t], 1)
    edges = [(i, i + 1) for i in range(n - 1)]
    while len(edges) < n - 1 + n_closures:
        a, b = rng.integers(0, n, 2)
        if a != b:
            edges.append((int(a), int(b)))
    v1 = np.array([e[0] for e in edges]); v2 = np.array([e[1] for e in edges])
    Ra, ta, Rb, tb = R[v1], t[v1], R[v2], t[v2]
    hR = np.swapaxes(Ra, 1, 2) @ Rb
    ht = np.einsum("nji,nj->ni", Ra, tb - ta)
    nR = _rodrigues(rng.normal(0, 0.03, (len(edges), 3))); nt = rng.normal(0, 0.05, (len(edges), 3))
    zR = hR @ nR; zt = ht + np.einsum("nij,nj->ni", hR, nt)
    z = np.concatenate([zR.reshape(-1, 9), zt], 1)
    nk = np.zeros(len(edges), np.int32); nd = np.zeros((len(edges), 36))
    for k in range(len(edges)):
        mode = {"mixed": k % 3, "diagonal": 0, "gaussian": 1, "isotropic": 2}[noise]
        if mode == 0:
            nk[k] = NOISE_DIAGONAL; nd[k, :6] = [0.1, 0.1, 0.1, 0.3, 0.3, 0.2]
        elif mode == 1:
            A = rng.normal(size=(6, 6)); info = A @ A.T + 6 * np.eye(6)
            nk[k] = NOISE_GAUSSIAN; nd[k] = np.linalg.cholesky(info).T.reshape(-1)
        else:
            nk[k] = NOISE_ISOTROPIC; nd[k, 0] = 0.2
    p = pose_graph_problem(n, v1, v2, z, nk, nd)
    npri = p.add_noise(NOISE_DIAGONAL, 6, np.sqrt([1e-6] * 3 + [1e-4] * 3))  # Pose3SLAMExample_g2o.cpp:41-43
    p.add_prior(0, poses[0], npri)
    dR = _rodrigues(rng.normal(0, init_noise, (n, 3)))
    v0 = np.concatenate([(R @ dR).reshape(n, 9), t + rng.normal(0, init_noise, (n, 3))], 1)
    v0[0] = poses[0]
    return p, v0.reshape(-1)


def random_projection_graph(n_poses=6, n_points=40, seed=0, with_sensor=True, behind=True, distortion=None):
    """Small GenericProjectionFactor<Pose3,Point3,Cal3_S2> graph (+ priors).  Returns (Problem, values0).
    distortion: optional (2, 4) array k1, k2, p1, p2 for the two calibrations -- a non-zero row makes that calibration a Cal3DS2
    (GenericProjectionFactor<Pose3,Point3,Cal3DS2>); the measurements are generated through the same distortion."""
    from .problem import VAR_POINT3, VAR_POSE3
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 1.0, n_poses)
    centers = np.stack([4 * np.sin(ang), 0.3 * rng.normal(size=n_poses), -6 + 0.5 * np.cos(ang)], 1)
    R = _rodrigues(np.stack([0.05 * rng.normal(size=n_poses), -0.4 * ang + 0.2, 0.03 * rng.normal(size=n_poses)], 1))
    pts = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(2, 8, n_points)], 1)
    if behind:
        pts[-2:, 2] = -9.0  # behind every camera: cheirality branch
    K = np.array([[520.0, 515.0, 0.3, 320.0, 240.0], [400.0, 400.0, 0.0, 300.0, 200.0]])
    sensor = np.concatenate([_rodrigues(np.array([[0.02, -0.03, 0.01]])).reshape(-1), [0.1, -0.05, 0.2]])
    vt = np.concatenate([np.full(n_poses, VAR_POSE3, np.int32), np.full(n_points, VAR_POINT3, np.int32)])
    p = Problem(var_type=vt)
    n_iso = p.add_noise(NOISE_ISOTROPIC, 2, [1.5]); n_unit = p.add_noise(NOISE_UNIT, 2)
    pose_i, pt_i, zs, nz, ci, si = [], [], [], [], [], []
    for i in range(n_poses):
        for j in range(n_points):
            if rng.uniform() < 0.5:
                continue
            use_s = with_sensor and (i % 2 == 1)
            Rw, tw = R[i], centers[i]
            if use_s:
                Rs = sensor[:9].reshape(3, 3); ts = sensor[9:]
                Rw, tw = Rw @ Rs, tw + R[i] @ ts
            q = Rw.T @ (pts[j] - tw)
            k = K[i % 2]
            if q[2] > 0:
                u, v = q[0] / q[2], q[1] / q[2]
                if distortion is not None:
                    k1, k2, p1, p2 = np.asarray(distortion, float)[i % 2]
                    rr = u * u + v * v; gg = 1 + k1 * rr + k2 * rr * rr
                    u, v = gg * u + 2 * p1 * u * v + p2 * (rr + 2 * u * u), gg * v + 2 * p2 * u * v + p1 * (rr + 2 * v * v)
                z = np.array([k[0] * u + k[2] * v + k[3], k[1] * v + k[4]]) + rng.normal(0, 1.0, 2)
            else:
                z = rng.normal(0, 50, 2)
            pose_i.append(i); pt_i.append(n_poses + j); zs.append(z); nz.append(n_iso if j % 2 else n_unit)
            ci.append(i % 2); si.append(0 if use_s else -1)
    p.proj_pose = np.array(pose_i, np.int32); p.proj_point = np.array(pt_i, np.int32)
    p.proj_z = np.array(zs).reshape(-1); p.proj_noise = np.array(nz, np.int32)
    p.proj_calib = np.array(ci, np.int32); p.proj_sensor = np.array(si, np.int32)
    p.calib = K.reshape(-1); p.sensor = sensor
    if distortion is not None:
        p.calib_distortion = np.ascontiguousarray(np.asarray(distortion, np.float64).reshape(-1))
    poses = np.concatenate([R.reshape(n_poses, 9), centers], 1)
    n6 = p.add_noise(NOISE_DIAGONAL, 6, [0.01] * 3 + [0.05] * 3); n3 = p.add_noise(NOISE_ISOTROPIC, 3, [0.1])
    p.add_prior(0, poses[0], n6); p.add_prior(1, poses[1], n6); p.add_prior(n_poses, pts[0], n3)
    dR = _rodrigues(rng.normal(0, 0.01, (n_poses, 3)))
    v0 = np.concatenate([np.concatenate([(R @ dR).reshape(n_poses, 9), centers + rng.normal(0, 0.05, centers.shape)], 1).reshape(-1),
                         (pts + rng.normal(0, 0.05, pts.shape)).reshape(-1)])
    return p, v0


def synthetic_orbit_scene(n_cams=10, n_points=120, seed=0, see=0.7, pixel_noise=0.5, init_noise=(0.01, 0.05), arc=0.9, far_points=0,
                          far_distance=(1500.0, 4000.0), spread=1.0):
    """A small structure-from-motion scene with a sane field of view (cameras on an arc around a point cloud, every measurement
    within ~0.5 of the optical axis in intrinsic coordinates, so that Cal3Bundler::calibrate converges): the input of the smart
    factor tests.  `arc`: half the opening of the arc in radians (below ~0.55 every camera sees every other camera's viewing
    directions in front of it: what a smart factor's point at infinity needs).  `far_points`: that many of the points lie
    `far_distance` away behind the cloud (parallax of a few pixels: a landmark-distance threshold rejects them and the point at
    infinity is a good model of them).  `spread` widens the cloud across the optical axes (the distortion coefficients are
    barely observable from measurements near the image centre).  Returns the BAL-style tuple (cams17 -- perturbed --, pts3, obs_cam, obs_pt, obs_z) with the packing of
    bal_problem (pose R row-major + t, f, k1, k2, u0, v0); every camera sees at least two points, every point is seen twice."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(-arc, arc, n_cams)
    centers = np.stack([8 * np.sin(ang), 0.3 * rng.normal(size=n_cams), -8 * np.cos(ang)], 1)
    R = _rodrigues(np.stack([0.02 * rng.normal(size=n_cams), -ang, 0.02 * rng.normal(size=n_cams)], 1))   # looks at the origin (+z)
    pts = np.stack([rng.uniform(-2, 2, n_points) * spread, rng.uniform(-1.5, 1.5, n_points) * spread, rng.uniform(-2, 2, n_points)], 1)
    if far_points:                                     # (own generator: the stream of the near scene does not depend on this option)
        r2 = np.random.default_rng(seed + 1000)
        dist = r2.uniform(far_distance[0], far_distance[1], far_points)
        pts[-far_points:] = np.stack([dist * r2.uniform(-0.15, 0.15, far_points), dist * r2.uniform(-0.12, 0.12, far_points), dist], 1)
    f = rng.uniform(450, 800, n_cams); k1 = rng.normal(0, 2e-2, n_cams); k2 = rng.normal(0, 2e-3, n_cams)
    oc, op, oz = [], [], []
    seen = rng.uniform(size=(n_cams, n_points)) < see
    seen[:2, :] = True
    for j in range(n_points):
        for i in range(n_cams):
            if not seen[i, j]:
                continue
            q = R[i].T @ (pts[j] - centers[i])
            u, v = q[0] / q[2], q[1] / q[2]
            rr = u * u + v * v
            g = 1 + (k1[i] + k2[i] * rr) * rr
            oc.append(i); op.append(j); oz.append([f[i] * g * u + pixel_noise * rng.normal(), f[i] * g * v + pixel_noise * rng.normal()])
    dR = _rodrigues(rng.normal(0, init_noise[0], (n_cams, 3)))
    cams = np.zeros((n_cams, 17))
    cams[:, :9] = (R @ dR).reshape(n_cams, 9); cams[:, 9:12] = centers + rng.normal(0, init_noise[1], centers.shape)
    cams[:, 12] = f + rng.normal(0, 1.0, n_cams); cams[:, 13] = k1; cams[:, 14] = k2
    return cams, pts + rng.normal(0, 0.05, pts.shape), np.array(oc, np.int32), np.array(op, np.int32), np.array(oz)


def stereo_mixed_graph(n_poses=6, n_points=40, seed=7):
    """A small stereo visual-odometry graph that enters every branch of GenericStereoFactor<Pose3, Point3> on the device, built
    through the API mirror (gtsam_amd.api) the way user code would: poses on an arc looking at a point cloud; a stereo factor for
    every (pose, landmark) pair with one Cal3_S2Stereo, a second rig -- another Cal3_S2Stereo, with a NON-ZERO skew (which
    StereoCamera::project2 ignores), mounted through body_P_sensor -- on a third of the pairs; dim-3 Unit / Isotropic / Diagonal /
    Gaussian noise and Robust(Huber) on some; monocular GenericProjectionFactors (Cal3_S2, one Cal3DS2) on a subset of the same
    landmarks; the last landmark lies BEHIND pose 0 (cheirality branch) and in front of the last two poses, its other observers; a prior on one landmark and on two poses, BetweenFactor<Pose3>
    along the arc.  Graph order: projection, stereo, between, prior.  Returns (graph, initial values, index of the behind-camera stereo factor)."""
    from . import api as A
    rng = np.random.default_rng(seed)
    ang = np.linspace(-0.5, 0.5, n_poses)
    centers = np.stack([8 * np.sin(ang), 0.3 * rng.normal(size=n_poses), -8 * np.cos(ang)], 1)
    R = _rodrigues(np.stack([0.02 * rng.normal(size=n_poses), -ang, 0.02 * rng.normal(size=n_poses)], 1))   # looks at the origin (+z)
    pts = np.stack([rng.uniform(-2, 2, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(-2, 2, n_points)], 1)
    pts[-1] = centers[0] - 0.5 * R[0][:, 2] + np.array([0.2, -0.1, 0.0])       # 0.5 behind pose 0 along its optical axis
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    K1 = A.Cal3_S2Stereo(720.0, 715.0, 0.0, 600.0, 170.0, 0.54)
    K2 = A.Cal3_S2Stereo(500.0, 510.0, 0.7, 320.0, 240.0, 0.25)                 # skew 0.7: stored, not used by the projection
    Km = A.Cal3_S2(520.0, 515.0, 0.3, 320.0, 240.0)
    Kd = A.Cal3DS2(400.0, 400.0, 0.0, 300.0, 200.0, 0.05, -0.01, 0.001, -0.002)
    sR = _rodrigues(np.array([[0.02, -0.03, 0.01]]))[0]; st = np.array([0.1, -0.05, 0.2])
    sensor = A.Pose3(A.Rot3(sR), st)
    Rg = np.array([[1.1, 0.2, -0.1], [0.0, 0.9, 0.3], [0.0, 0.0, 1.3]])
    nm = A.noiseModel
    models3 = [nm.Unit.Create(3), nm.Isotropic.Sigma(3, 1.5), nm.Diagonal.Sigmas([1.0, 1.2, 0.8]), nm.Gaussian.SqrtInformation(Rg),
               nm.Robust.Create(nm.mEstimator.Huber.Create(1.345), nm.Isotropic.Sigma(3, 1.2))]
    m2 = [nm.Isotropic.Sigma(2, 1.5), nm.Unit.Create(2)]

    def stereo_z(K, Rw, tw, pt):
        q = Rw.T @ (pt - tw)
        if q[2] <= 0:
            return rng.normal(300.0, 50.0, 3)
        fx, fy, _, u0, v0, b = K.v
        return np.array([u0 + fx * q[0] / q[2], u0 + fx * (q[0] - b) / q[2], v0 + fy * q[1] / q[2]]) + rng.normal(0, 0.7, 3)

    graph, initial = A.NonlinearFactorGraph(), A.Values()
    for i in range(min(4, n_poses)):                      # monocular factors on the first ten landmarks
        for j in range(10):
            q = R[i].T @ (pts[j] - centers[i])
            u, v = q[0] / q[2], q[1] / q[2]
            z = np.array([Km.v[0] * u + Km.v[2] * v + Km.v[3], Km.v[1] * v + Km.v[4]]) + rng.normal(0, 1.0, 2)
            graph.add(A.GenericProjectionFactorCal3_S2(z, m2[j % 2], X(i), L(j), Km))
    q = R[4].T @ (pts[3] - centers[4]); u, v = q[0] / q[2], q[1] / q[2]
    rr = u * u + v * v; gg = 1 + 0.05 * rr - 0.01 * rr * rr
    ud, vd = gg * u + 2 * 0.001 * u * v - 0.002 * (rr + 2 * u * u), gg * v + 2 * -0.002 * u * v + 0.001 * (rr + 2 * v * v)
    graph.add(A.GenericProjectionFactorCal3DS2(np.array([400.0 * ud + 300.0, 400.0 * vd + 200.0]) + rng.normal(0, 1.0, 2), m2[0], X(4), L(3), Kd))
    behind, k = -1, 0
    for i in range(n_poses):
        for j in range(n_points):
            if j == n_points - 1 and 0 < i < n_poses - 2:
                continue                                  # (the last landmark: seen from behind by pose 0, from the front by the last two poses only)
            if i == 0 and j == n_points - 1:
                behind = k
            graph.add(A.GenericStereoFactor3D(stereo_z(K1, R[i], centers[i], pts[j]), models3[k % 5], X(i), L(j), K1)); k += 1
            if (i * n_points + j) % 3 == 0:               # the second rig, through body_P_sensor
                Rw, tw = R[i] @ sR, centers[i] + R[i] @ st
                graph.add(A.GenericStereoFactor3D(stereo_z(K2, Rw, tw, pts[j]), models3[k % 5], X(i), L(j), K2, sensor)); k += 1
    n6 = nm.Diagonal.Sigmas([0.01] * 3 + [0.05] * 3); n6b = nm.Diagonal.Sigmas([0.02, 0.02, 0.03, 0.1, 0.1, 0.15])
    for i in range(n_poses - 1):
        Rz = R[i].T @ R[i + 1]; tz = R[i].T @ (centers[i + 1] - centers[i])
        graph.add(A.BetweenFactorPose3(X(i), X(i + 1), A.Pose3(A.Rot3(Rz @ _rodrigues(rng.normal(0, 0.005, (1, 3)))[0]), tz + rng.normal(0, 0.02, 3)), n6b))
    graph.addPriorPose3(X(0), A.Pose3(A.Rot3(R[0]), centers[0]), n6)
    graph.addPriorPose3(X(1), A.Pose3(A.Rot3(R[1]), centers[1]), n6)
    graph.addPriorPoint3(L(0), pts[0], nm.Isotropic.Sigma(3, 0.1))
    dR = _rodrigues(rng.normal(0, 0.01, (n_poses, 3)))
    for i in range(n_poses):
        initial.insert(X(i), A.Pose3(A.Rot3(R[i] @ dR[i]), centers[i] + rng.normal(0, 0.05, 3)))
    for j in range(n_points):
        initial.insert(L(j), pts[j] + rng.normal(0, 0.05, 3))
    return graph, initial, behind


def stereo_vo_graph(calibration_path, poses_path, factors_path):
    """The graph of examples/StereoVOExample_large.cpp (:45-107) from its three data files, through the API mirror: one shared
    Cal3_S2Stereo, Isotropic::Sigma(3, 1) (= Unit) on every GenericStereoFactor, camera poses from the 4 x 4 matrices of the pose
    file, a landmark initialised from the first factor that names it (camPose.transformFrom of the triangulated camera-frame point).
    Constrained noise is outside the device path: the example's NonlinearEquality<Pose3> on pose 1 is a
    PriorFactor<Pose3> with Isotropic::Sigma(6, 1e-6) here.  Returns (graph, initial values)."""
    from . import api as A
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    K = A.Cal3_S2Stereo(*np.loadtxt(calibration_path).reshape(-1)[:6])
    model = A.noiseModel.Isotropic.Sigma(3, 1.0)
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    poses = {}
    for row in np.loadtxt(poses_path).reshape(-1, 17):
        m = row[1:].reshape(4, 4)
        poses[int(row[0])] = A.Pose3(A.Rot3(m[:3, :3]), m[:3, 3])
        initial.insert(X(int(row[0])), poses[int(row[0])])
    for x, l, uL, uR, v, px, py, pz in np.loadtxt(factors_path).reshape(-1, 8):
        x, l = int(x), int(l)
        graph.add(A.GenericStereoFactor3D(A.StereoPoint2(uL, uR, v), model, X(x), L(l), K))
        if not initial.exists(L(l)):
            initial.insert(L(l), poses[x].R @ np.array([px, py, pz]) + poses[x].t)
    graph.addPriorPose3(X(1), poses[1], A.noiseModel.Isotropic.Sigma(6, 1e-6))
    return graph, initial


def smart_pose_graph(n_poses=8, n_tracks=8, seed=0, arc=np.pi, radius=25.0, box=(8.0, 8.0, 8.0), K=(50.0, 50.0, 0.0, 50.0, 50.0), sigma=1.0,
                     pixel_noise=0.05, see=1.0, params=None, sensor=None, single_tracks=0, far_tracks=0, far_distance=(1500.0, 4000.0),
                     outlier_tracks=0, outlier_shift=150.0, explicit_landmarks=0, between_chain=False, priors=(0, 1),
                     init_delta=None, init_noise=(0.01, 0.05)):
    """A visual-odometry scene whose landmarks live inside SmartProjectionPose3Factors (SmartProjectionPoseFactor<Cal3_S2>), built through
    the API mirror the way user code would: `n_poses` cameras on an arc of half opening `arc` (pi: a full circle) of radius `radius`
    looking inward at `n_tracks` points in a box, one shared Cal3_S2 `K`, Isotropic::Sigma(2, sigma), pixel noise; every track is seen by
    a camera with probability `see` (at least by two).  `sensor` (an api.Pose3): every smart factor has this body_P_sensor and the
    variables are the BODY poses (camera = body * sensor).  Bad tracks, in this order behind the good ones: `single_tracks` with one
    measurement (DEGENERATE), `far_tracks` points `far_distance` away along the arc's axis (FAR_POINT under a landmarkDistanceThreshold),
    `outlier_tracks` with one measurement moved by `outlier_shift` pixels (OUTLIER under a dynamicOutlierRejectionThreshold).
    `explicit_landmarks`: that many further points are Point3 variables with GenericProjectionFactors (same K and sensor);
    `between_chain`: BetweenFactor<Pose3> along the arc; `priors`: the poses with a Diagonal prior.  Initial poses: the truth composed
    with the fixed Pose3 `init_delta` (an api.Pose3), or perturbed by `init_noise` (rotation, translation).
    Graph order: smart factors, projection factors, between factors, priors.  Returns (graph, initial values, info) with
    info["kind"][t] = 0 good, 1 single, 2 far, 3 outlier for every smart factor."""
    from . import api as A
    rng = np.random.default_rng(seed)
    full = arc >= np.pi
    ang = np.linspace(-arc, arc, n_poses, endpoint=not full)
    centers = np.stack([radius * np.sin(ang), 0.02 * radius * rng.normal(size=n_poses), -radius * np.cos(ang)], 1)
    Rc = _rodrigues(np.stack([0.02 * rng.normal(size=n_poses), -ang, 0.02 * rng.normal(size=n_poses)], 1))   # looks at the origin (+z)
    n_all = n_tracks + explicit_landmarks
    pts = np.stack([rng.uniform(-b, b, n_all) for b in box], 1)
    kind = np.zeros(n_tracks, np.int64)
    n_bad = single_tracks + far_tracks + outlier_tracks
    if n_bad > n_tracks:
        raise ValueError("more bad tracks than tracks")
    kind[n_tracks - n_bad:n_tracks - n_bad + single_tracks] = 1
    kind[n_tracks - far_tracks - outlier_tracks:n_tracks - outlier_tracks] = 2
    kind[n_tracks - outlier_tracks:] = 3
    if far_tracks:
        dist = rng.uniform(far_distance[0], far_distance[1], far_tracks)
        pts[np.flatnonzero(kind == 2)] = np.stack([dist * rng.uniform(-0.15, 0.15, far_tracks), dist * rng.uniform(-0.12, 0.12, far_tracks), dist], 1)
    Kc = A.Cal3_S2(*K)
    fx, fy, s, u0, v0 = Kc.v
    model = A.noiseModel.Isotropic.Sigma(2, sigma)
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L

    def pixel(i, pt):
        q = Rc[i].T @ (pt - centers[i])
        u, v = q[0] / q[2], q[1] / q[2]
        return np.array([fx * u + s * v + u0, fy * v + v0]) + pixel_noise * rng.normal(size=2)

    # the variables are body poses: camera = body * sensor
    if sensor is not None:
        Rs, ts = sensor.R, sensor.t
        Rb = Rc @ Rs.T
        tb = centers - np.einsum("nij,j->ni", Rb, ts)
    else:
        Rb, tb = Rc, centers
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    seen = rng.uniform(size=(n_all, n_poses)) < see
    for t in range(n_tracks):
        views = np.flatnonzero(seen[t])
        if views.size < 2:
            views = np.sort(rng.choice(n_poses, 2, replace=False))
        if kind[t] == 1:
            views = views[:1]
        f = A.SmartProjectionPose3Factor(model, Kc, sensor, params)
        for n, i in enumerate(views):
            z = pixel(i, pts[t])
            if kind[t] == 3 and n == views.size - 1:
                z = z + outlier_shift * np.array([0.8, -0.6])
            f.add(z, X(int(i)))
        graph.add(f)
    for j in range(explicit_landmarks):
        views = np.flatnonzero(seen[n_tracks + j])
        if views.size < 2:
            views = np.arange(2)
        for i in views:
            graph.add(A.GenericProjectionFactorCal3_S2(pixel(i, pts[n_tracks + j]), model, X(int(i)), L(j), Kc, sensor))
    nm = A.noiseModel
    if between_chain:
        n6b = nm.Diagonal.Sigmas([0.02, 0.02, 0.03, 0.1, 0.1, 0.15])
        for i in range(n_poses - 1):
            Rz = Rb[i].T @ Rb[i + 1]; tz = Rb[i].T @ (tb[i + 1] - tb[i])
            graph.add(A.BetweenFactorPose3(X(i), X(i + 1), A.Pose3(A.Rot3(Rz @ _rodrigues(rng.normal(0, 0.005, (1, 3)))[0]), tz + rng.normal(0, 0.02, 3)), n6b))
    n6 = nm.Diagonal.Sigmas([0.1] * 3 + [0.3] * 3)
    for i in priors:
        graph.addPriorPose3(X(i), A.Pose3(A.Rot3(Rb[i]), tb[i]), n6)
    if init_delta is not None:
        Ri = Rb @ init_delta.R
        ti = tb + np.einsum("nij,j->ni", Rb, init_delta.t)
    else:
        Ri = Rb @ _rodrigues(rng.normal(0, init_noise[0], (n_poses, 3)))
        ti = tb + rng.normal(0, init_noise[1], tb.shape)
    for i in range(n_poses):
        initial.insert(X(i), A.Pose3(A.Rot3(Ri[i]), ti[i]))
    for j in range(explicit_landmarks):
        initial.insert(L(j), pts[n_tracks + j] + rng.normal(0, 0.05, 3))
    return graph, initial, {"kind": kind, "points": pts[:n_tracks]}


# The pose-type smart scenes the fixtures of tests/golden/make_golden_smart_pose.py are recorded on (name -> keyword arguments of
# smart_pose_graph + the SmartProjectionParams fields).  A seed is part of the fixture: the generator checks on the CPU that the
# reference's LM takes the same accept / reject sequence under the reversed ordering and moves to the next seed otherwise.
SMART_POSE_SCENES = {
    # the protocol of examples/SFMExample_SmartFactor.cpp on a scene of this project's own
    "smart_pose_example": dict(scene=dict(n_poses=8, n_tracks=8, K=(50.0, 50.0, 0.0, 50.0, 50.0), sigma=1.0, pixel_noise=0.05,
                                          init_delta=((-0.1, 0.2, 0.25), (0.05, -0.10, 0.20))), params=dict()),
    "smart_pose_mixed": dict(scene=dict(n_poses=12, n_tracks=291, arc=0.5, radius=8.0, box=(2.0, 1.5, 2.0), K=(520.0, 515.0, 0.3, 320.0, 240.0),
                                        sigma=1.5, pixel_noise=0.7, see=0.6, single_tracks=9, far_tracks=11, outlier_tracks=7, explicit_landmarks=6,
                                        between_chain=True, priors=(0,), sensor=((0.02, -0.03, 0.01), (0.1, -0.05, 0.2)),
                                        init_noise=(0.004, 0.02)),
                             params=dict(degeneracyMode=1, landmarkDistanceThreshold=100.0, dynamicOutlierRejectionThreshold=40.0)),
    "smart_pose_far_ignore": dict(scene=dict(n_poses=8, n_tracks=70, arc=0.45, radius=8.0, box=(2.0, 1.5, 2.0), K=(600.0, 600.0, 0.0, 320.0, 240.0),
                                             sigma=1.0, pixel_noise=0.5, see=0.7, single_tracks=3, far_tracks=8),
                                  params=dict(degeneracyMode=0, linearizationMode=0, landmarkDistanceThreshold=100.0)),
    "smart_pose_far_infinity": dict(scene=dict(n_poses=8, n_tracks=70, arc=0.45, radius=8.0, box=(2.0, 1.5, 2.0), K=(600.0, 600.0, 0.0, 320.0, 240.0),
                                               sigma=1.0, pixel_noise=0.5, see=0.7, single_tracks=3, far_tracks=8),
                                    params=dict(degeneracyMode=2, linearizationMode=0, landmarkDistanceThreshold=100.0)),
    "smart_pose_far_jacobian_q": dict(scene=dict(n_poses=8, n_tracks=70, arc=0.45, radius=8.0, box=(2.0, 1.5, 2.0), K=(600.0, 600.0, 0.0, 320.0, 240.0),
                                                 sigma=1.0, pixel_noise=0.5, see=0.7, single_tracks=3, far_tracks=8),
                                      params=dict(degeneracyMode=0, linearizationMode=2, landmarkDistanceThreshold=100.0)),
}


# The far scenes on a WIDE arc with a landmarkDistanceThreshold that fails the near tracks too: the direction of such a track's first
# measurement, seen from the first camera, lies behind the cameras at the other end of the arc, where the reference throws a
# CheiralityException (tests/test_gpu_smart_pose.py)
SMART_POSE_WIDE_ARC = dict(scene=dict(arc=0.9), params=dict(landmarkDistanceThreshold=8.0))


def smart_pose_scene(name, seed=0, scene=None, params=None):
    """(graph, initial values, info) of one of SMART_POSE_SCENES; `scene` / `params`: keyword arguments of smart_pose_graph /
    SmartProjectionParams fields to replace."""
    from . import api as A
    spec = SMART_POSE_SCENES[name]
    prm = A.SmartProjectionParams()
    for k, v in {**spec["params"], **(params or {})}.items():
        setattr(prm, k, v)
    scene = {**spec["scene"], **(scene or {})}
    for key in ("sensor", "init_delta"):
        if scene.get(key) is not None:
            w, t = scene[key]
            scene[key] = A.Pose3(A.Rot3(_rodrigues(np.array([w]))[0]), np.array(t))
    return smart_pose_graph(seed=seed, params=prm, **scene)


def smart_rig_graph(rig, n_poses, tracks, seed=0, arc=0.4, radius=8.0, box=(2.0, 1.5, 2.0), sigma=1.0, pixel_noise=0.3, params=None,
                    far_distance=(1500.0, 4000.0), outlier_shift=150.0, explicit_landmarks=0, see=0.6, between_chain=False, priors=(0,),
                    init_noise=(0.004, 0.02)):
    """A multi-camera visual-odometry scene whose landmarks live inside SmartProjectionRigFactors (SmartProjectionRigFactor<
    PinholePose<Cal3_S2>>), built through the API mirror the way user code would.  `rig`: ((fx, fy, s, u0, v0), extrinsic) per camera,
    extrinsic = None (identity) or (rotation vector, translation) of body_P_sensor.  `n_poses` BODY poses on an arc of half opening `arc`
    and radius `radius` look inward at points in `box`.  `tracks`: one entry per smart factor, in graph order --
      ("views", [(pose, camera id), ...])  a rig factor with exactly these sightings (a pose may occur several times);
      ("random",)     a rig factor: every (pose, camera) sees the point with probability `see` (at least two sightings);
      ("single",)     a rig factor with one sighting (DEGENERATE);
      ("far",)        "random" on a point `far_distance` away (FAR_POINT under a landmarkDistanceThreshold);
      ("outlier",)    "random" with the last measurement moved by `outlier_shift` pixels (OUTLIER under a
                      dynamicOutlierRejectionThreshold);
      ("pose",)       a SmartProjectionPose3Factor through camera 0 of the rig (its K, its extrinsic as body_P_sensor), seen from every
                      pose with probability `see` (at least two).
    `explicit_landmarks`: that many further points are Point3 variables with GenericProjectionFactors through camera 0;
    `between_chain`: BetweenFactor<Pose3> along the arc; `priors`: the poses with a Diagonal prior.
    Graph order: smart factors, projection factors, between factors, priors.  Returns (graph, initial values, info) with
    info["kind"][t] the track's kind and info["points"] the true points."""
    from . import api as A
    rng = np.random.default_rng(seed)
    ang = np.linspace(-arc, arc, n_poses)
    tb = np.stack([radius * np.sin(ang), 0.02 * radius * rng.normal(size=n_poses), -radius * np.cos(ang)], 1)
    Rb = _rodrigues(np.stack([0.02 * rng.normal(size=n_poses), -ang, 0.02 * rng.normal(size=n_poses)], 1))   # +z looks at the origin
    cams = A.CameraSetPinholePoseCal3_S2()
    ext = []
    for K, e in rig:
        pose = A.Pose3() if e is None else A.Pose3(A.Rot3(_rodrigues(np.array([e[0]]))[0]), np.array(e[1], np.float64))
        cams.push_back(A.PinholePoseCal3_S2(pose, A.Cal3_S2(*K)))
        ext.append(pose)
    n_tracks = len(tracks)
    pts = np.stack([rng.uniform(-b, b, n_tracks + explicit_landmarks) for b in box], 1)
    model = A.noiseModel.Isotropic.Sigma(2, sigma)
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    params = params or A.SmartProjectionParams(degeneracyMode=1)     # (what the rig factor's constructor accepts)

    def pixel(i, c, pt):
        R = Rb[i] @ ext[c].R; t = tb[i] + Rb[i] @ ext[c].t
        q = R.T @ (pt - t)
        fx, fy, s, u0, v0 = cams[c].calibration().v
        u, v = q[0] / q[2], q[1] / q[2]
        return np.array([fx * u + s * v + u0, fy * v + v0]) + pixel_noise * rng.normal(size=2)

    def random_views(n_cams_used):
        seen = np.argwhere(rng.uniform(size=(n_poses, n_cams_used)) < see)
        if seen.shape[0] < 2:
            seen = np.array([[0, 0], [n_poses - 1, 0]])
        return [(int(i), int(c)) for i, c in seen]

    graph, initial = A.NonlinearFactorGraph(), A.Values()
    for t, spec in enumerate(tracks):
        kind = spec[0]
        if kind == "far":
            d = rng.uniform(*far_distance)
            pts[t] = [d * rng.uniform(-0.15, 0.15), d * rng.uniform(-0.12, 0.12), d]
        if kind == "pose":
            f = A.SmartProjectionPose3Factor(model, cams[0].calibration(), None if rig[0][1] is None else ext[0], params)
            for i, _ in random_views(1):
                f.add(pixel(i, 0, pts[t]), X(i))
            graph.add(f)
            continue
        views = list(spec[1]) if kind == "views" else random_views(len(rig))
        if kind == "single":
            views = views[:1]
        f = A.SmartProjectionRigFactorPinholePoseCal3_S2(model, cams, params)
        for n, (i, c) in enumerate(views):
            z = pixel(i, c, pts[t])
            if kind == "outlier" and n == len(views) - 1:
                z = z + outlier_shift * np.array([0.8, -0.6])
            f.add(z, X(i), c)
        graph.add(f)
    for j in range(explicit_landmarks):
        views = np.flatnonzero(rng.uniform(size=n_poses) < see)
        if views.size < 2:
            views = np.arange(2)
        for i in views:
            graph.add(A.GenericProjectionFactorCal3_S2(pixel(int(i), 0, pts[n_tracks + j]), model, X(int(i)), L(j), cams[0].calibration(),
                                                       None if rig[0][1] is None else ext[0]))
    nm = A.noiseModel
    if between_chain:
        n6b = nm.Diagonal.Sigmas([0.02, 0.02, 0.03, 0.1, 0.1, 0.15])
        for i in range(n_poses - 1):
            Rz = Rb[i].T @ Rb[i + 1]; tz = Rb[i].T @ (tb[i + 1] - tb[i])
            graph.add(A.BetweenFactorPose3(X(i), X(i + 1), A.Pose3(A.Rot3(Rz @ _rodrigues(rng.normal(0, 0.005, (1, 3)))[0]), tz + rng.normal(0, 0.02, 3)), n6b))
    n6 = nm.Diagonal.Sigmas([0.1] * 3 + [0.3] * 3)
    for i in priors:
        graph.addPriorPose3(X(i), A.Pose3(A.Rot3(Rb[i]), tb[i]), n6)
    Ri = Rb @ _rodrigues(rng.normal(0, init_noise[0], (n_poses, 3)))
    ti = tb + rng.normal(0, init_noise[1], tb.shape)
    for i in range(n_poses):
        initial.insert(X(i), A.Pose3(A.Rot3(Ri[i]), ti[i]))
    for j in range(explicit_landmarks):
        initial.insert(L(j), pts[n_tracks + j] + rng.normal(0, 0.05, 3))
    return graph, initial, {"kind": [s[0] for s in tracks], "points": pts[:n_tracks]}


def _rig_pair_tracks():
    both = lambda i: [(i, 0), (i, 1)]
    # both cameras from all three poses (three of them, so that the third pose is held by more than one landmark); both cameras from
    # ONE pose only (one unique key: the rig's baseline triangulates it); no repetition; DEGENERATE; FAR_POINT
    return ([("views", both(0) + both(1) + both(2))] * 3 + [("views", both(1))] + [("views", [(0, 0), (1, 1), (2, 0)]), ("views", [(0, 1), (1, 0), (2, 1)])]
            + [("single",), ("far",)])


def _rig_mixed_tracks():
    t = []
    for k in range(151):
        t.append(("pose",) if k % 9 == 4 else ("random",))
    for k, kind in ((7, "single"), (38, "single"), (77, "far"), (90, "far"), (101, "far"), (120, "outlier"), (133, "outlier")):
        t[k] = (kind,)
    return t


# The rig-type smart scenes the fixtures of tests/golden/make_golden_smart_rig.py are recorded on (a seed is part of the fixture, as for
# SMART_POSE_SCENES).  smart_rig_pair: two cameras with different K (one with skew), camera 0 without an extrinsic, camera 1 rotated and
# offset; smart_rig_mixed: three cameras, pose-type smart factors and explicit landmarks beside the rig factors.
SMART_RIG_SCENES = {
    "smart_rig_pair": dict(scene=dict(rig=(((520.0, 515.0, 0.4, 320.0, 240.0), None),
                                           ((480.0, 490.0, 0.0, 300.0, 250.0), ((0.03, -0.06, 0.02), (0.6, -0.04, 0.05)))),
                                      n_poses=3, tracks=_rig_pair_tracks(), arc=0.25, sigma=1.0, pixel_noise=0.3, priors=(0, 1),
                                      init_noise=(0.004, 0.02)),
                           params=dict(degeneracyMode=1, landmarkDistanceThreshold=100.0)),
    "smart_rig_mixed": dict(scene=dict(rig=(((520.0, 515.0, 0.3, 320.0, 240.0), ((0.02, -0.03, 0.01), (0.1, -0.05, 0.2))),
                                            ((500.0, 505.0, 0.0, 310.0, 245.0), ((0.01, 0.08, -0.02), (0.45, 0.0, 0.15))),
                                            ((540.0, 530.0, -0.2, 330.0, 235.0), ((-0.02, -0.09, 0.01), (-0.4, 0.03, 0.18)))),
                                       n_poses=20, tracks=_rig_mixed_tracks(), arc=0.5, sigma=1.5, pixel_noise=0.7, see=0.65,
                                       explicit_landmarks=5, between_chain=True, priors=(0,), init_noise=(0.004, 0.02)),
                            params=dict(degeneracyMode=1, landmarkDistanceThreshold=100.0, dynamicOutlierRejectionThreshold=40.0)),
}


def smart_rig_scene(name, seed=0, scene=None, params=None):
    """(graph, initial values, info) of one of SMART_RIG_SCENES; `scene` / `params`: keyword arguments of smart_rig_graph /
    SmartProjectionParams fields to replace."""
    from . import api as A
    spec = SMART_RIG_SCENES[name]
    prm = A.SmartProjectionParams()
    for k, v in {**spec["params"], **(params or {})}.items():
        setattr(prm, k, v)
    return smart_rig_graph(seed=seed, params=prm, **{**spec["scene"], **(scene or {})})


def smart_lost_graph(kind, tracks, n_poses=10, seed=0, arc=0.5, radius=8.0, box=(2.0, 1.5, 2.0), sigma=1.0, pixel_noise=0.3, params=None,
                     dlt_params=None, K=(520.0, 515.0, 0.3, 320.0, 240.0), bundler=(560.0, -0.04, 0.006, 320.0, 240.0), sensor=None, rig=(),
                     see=0.6, far_distance=(150.0, 400.0), thin_distance=(2.0e6, 4.0e6), outlier_shift=150.0, priors=(0, 1),
                     between_chain=False, init_noise=(0.004, 0.02)):
    """A visual-odometry scene for TriangulationParameters::useLOST, built through the API mirror.  `kind`: "camera"
    (SmartProjectionFactor<PinholeCamera<Cal3Bundler>>: the variables are cameras with the calibration `bundler` = f, k1, k2, u0, v0),
    "pose" (SmartProjectionPose3Factor with `K` and the body_P_sensor `sensor`) or "rig" (SmartProjectionRigFactor over `rig`, as
    smart_rig_graph takes it).  `n_poses` bodies on an arc of half opening `arc` and radius `radius` look inward at points in `box`.
    `tracks`: one (kind, lost) per smart factor in graph order; lost False gives the factor `dlt_params` in place of `params` --
      "random"    every (pose, camera) sees the point with probability `see` (at least two sightings);
      "single"    one sighting (DEGENERATE);
      "far"       "random" on a point `far_distance` away (FAR_POINT under a landmarkDistanceThreshold);
      "thin"      "random" on a point `thin_distance` away, seen from the INITIAL poses without pixel noise: at the initial values its rays
                  are parallel to a few parts in 1e6 (DEGENERATE by LOST's rank test; with pixel noise, or from the true poses, the
                  rays of any far point differ by the angle of that noise, about 1e-3);
      "outlier"   "random" with the last measurement moved by `outlier_shift` pixels;
      "coincide"  two sightings, the second a copy of the first: same pose, camera and pixel (LOST finds no partner: DEGENERATE);
      "dup_first" three sightings, the second a copy of the first (LOST searches a partner for both and finds the third).
    Only a rig factor takes the same key twice (SmartFactorBase::add refuses it), so for the other two kinds the copy is seen from a TWIN
    of pose 0: one more variable, X(n_poses), with the same true and the same initial value and a prior of its own.
    Graph order: between factors, priors, smart factors (the order in which the C++ shim's extractor meets the noise models of a graph
    without projection factors, so that both extractors number them alike).  Returns (graph, initial values, info)."""
    from . import api as A
    rng = np.random.default_rng(seed)
    ang = np.linspace(-arc, arc, n_poses)
    tb = np.stack([radius * np.sin(ang), 0.02 * radius * rng.normal(size=n_poses), -radius * np.cos(ang)], 1)
    Rb = _rodrigues(np.stack([0.02 * rng.normal(size=n_poses), -ang, 0.02 * rng.normal(size=n_poses)], 1))   # +z looks at the origin
    as_pose = lambda e: A.Pose3() if e is None else A.Pose3(A.Rot3(_rodrigues(np.array([e[0]]))[0]), np.array(e[1], np.float64))
    if kind == "rig":
        cams = A.CameraSetPinholePoseCal3_S2()
        for Kc, e in rig:
            cams.push_back(A.PinholePoseCal3_S2(as_pose(e), A.Cal3_S2(*Kc)))
        ext = [c.pose() for c in cams]
        cals = [c.calibration().v for c in cams]
    else:
        ext = [as_pose(sensor if kind == "pose" else None)]
        cals = [np.array(K, np.float64)]
        Kc = A.Cal3_S2(*K)
    model = A.noiseModel.Isotropic.Sigma(2, sigma)
    X = A.symbol_shorthand.X
    pts = np.stack([rng.uniform(-b, b, len(tracks)) for b in box], 1)
    Ri = Rb @ _rodrigues(rng.normal(0, init_noise[0], (n_poses, 3)))
    ti = tb + rng.normal(0, init_noise[1], tb.shape)

    noise_of = []          # the noise of the pixels of the track in hand, in the order they were drawn

    def pixel(i, c, pt, initial=False):
        Rw, tw = (Ri, ti) if initial else (Rb, tb)
        R = Rw[i] @ ext[c].R; t = tw[i] + Rw[i] @ ext[c].t
        q = R.T @ (pt - t)
        u, v = q[0] / q[2], q[1] / q[2]
        if kind == "camera":
            f, k1, k2, u0, v0 = bundler
            g = 1.0 + (k1 + k2 * (u * u + v * v)) * (u * u + v * v)
            z = np.array([f * g * u + u0, f * g * v + v0])
        else:
            fx, fy, s, u0, v0 = cals[c]
            z = np.array([fx * u + s * v + u0, fy * v + v0])
        noise_of.append(pixel_noise * rng.normal(size=2))
        return z + noise_of[-1]

    def random_views():
        seen = np.argwhere(rng.uniform(size=(n_poses, len(ext))) < see)
        if seen.shape[0] < 2:
            seen = np.array([[0, 0], [n_poses - 1, 0]])
        return [(int(i), int(c)) for i, c in seen]

    graph, initial, smart = A.NonlinearFactorGraph(), A.Values(), []
    for t, (what, lost) in enumerate(tracks):
        noise_of = []
        if what in ("far", "thin"):
            d = rng.uniform(*(far_distance if what == "far" else thin_distance))
            pts[t] = [d * rng.uniform(-0.15, 0.15), d * rng.uniform(-0.12, 0.12), d]
        views = random_views()
        if what == "single":
            views = views[:1]
        if what in ("coincide", "dup_first"):
            views = [views[0] if kind == "rig" else (0, 0), views[-1] if views[-1][0] != 0 else (n_poses - 1, 0)]
        zs = [pixel(i, c, pts[t], what == "thin") for i, c in views]
        if what == "thin":
            zs = [z - e for z, e in zip(zs, noise_of)]
        if what == "outlier":
            zs[-1] = zs[-1] + outlier_shift * np.array([0.8, -0.6])
        copy = views[0] if kind == "rig" else (n_poses, 0)
        if what == "coincide":
            views, zs = [views[0], copy], [zs[0], zs[0]]
        if what == "dup_first":
            views, zs = [views[0], copy, views[1]], [zs[0], zs[0], zs[1]]
        prm = params if lost else dlt_params
        if kind == "camera":
            f = A.SmartProjectionFactorPinholeCameraCal3Bundler(model, prm)
        elif kind == "pose":
            f = A.SmartProjectionPose3Factor(model, Kc, ext[0] if sensor is not None else None, prm)
        else:
            f = A.SmartProjectionRigFactorPinholePoseCal3_S2(model, cams, prm)
        for z, (i, c) in zip(zs, views):
            f.add(z, X(i), c) if kind == "rig" else f.add(z, X(i))
        smart.append(f)
    nm = A.noiseModel
    if between_chain and kind != "camera":
        n6b = nm.Diagonal.Sigmas([0.02, 0.02, 0.03, 0.1, 0.1, 0.15])
        for i in range(n_poses - 1):
            Rz = Rb[i].T @ Rb[i + 1]; tz = Rb[i].T @ (tb[i + 1] - tb[i])
            graph.add(A.BetweenFactorPose3(X(i), X(i + 1), A.Pose3(A.Rot3(Rz @ _rodrigues(rng.normal(0, 0.005, (1, 3)))[0]), tz + rng.normal(0, 0.02, 3)), n6b))
    if kind != "rig":                                    # the twin of pose 0
        Rb, tb, Ri, ti = (np.concatenate([a, a[:1]]) for a in (Rb, tb, Ri, ti))
        priors = tuple(priors) + (n_poses,)
        n_poses += 1
    if kind == "camera":
        n9 = nm.Diagonal.Sigmas([0.1] * 3 + [0.3] * 3 + [5.0, 0.002, 0.002])
        for i in priors:
            graph.addPriorPinholeCameraCal3Bundler(X(i), A.PinholeCameraCal3Bundler(A.Pose3(A.Rot3(Rb[i]), tb[i]), A.Cal3Bundler(*bundler)), n9)
        for i in range(n_poses):
            initial.insert(X(i), A.PinholeCameraCal3Bundler(A.Pose3(A.Rot3(Ri[i]), ti[i]), A.Cal3Bundler(*bundler)))
    else:
        n6 = nm.Diagonal.Sigmas([0.1] * 3 + [0.3] * 3)
        for i in priors:
            graph.addPriorPose3(X(i), A.Pose3(A.Rot3(Rb[i]), tb[i]), n6)
        for i in range(n_poses):
            initial.insert(X(i), A.Pose3(A.Rot3(Ri[i]), ti[i]))
    for f in smart:
        graph.add(f)
    return graph, initial, {"kind": [w for w, _ in tracks], "lost": np.array([l for _, l in tracks]), "points": pts}


def _lost_tracks(n, mixed=False):
    """n tracks with every special kind of smart_lost_graph among them; mixed: every third random track is a DLT factor"""
    t = [("random", True)] * n
    for k, what in ((3, "coincide"), (5, "dup_first"), (8, "single"), (11, "far"), (14, "thin"), (17, "outlier"), (20, "far"), (23, "thin"),
                    (26, "dup_first"), (29, "outlier")):
        t[k] = (what, True)
    if mixed:
        t = [(w, not (w == "random" and k % 3 == 1)) for k, (w, _) in enumerate(t)]
    return t


# The LOST scenes the fixtures of tests/golden/make_golden_smart_lost.py are recorded on (a seed is part of the fixture, as for
# SMART_POSE_SCENES).  rankTolerance 1e-4: LOST's rank test is relative to the largest pivot, so the "thin" tracks (rays parallel to a
# few parts in 1e6) fail it and the near and the merely far ones pass.  The camera scene has a prior on every camera: few tracks leave
# the distortion coefficients of a camera weakly determined, and a step that moves them far makes Cal3Bundler::calibrate diverge.  `variants`: further fixtures <name>_<variant> on the same scene with
# these SmartProjectionParams fields replaced.
_LOST_PARAMS = dict(degeneracyMode=1, rankTolerance=1e-4, landmarkDistanceThreshold=100.0, dynamicOutlierRejectionThreshold=40.0, useLOST=True)
SMART_LOST_SCENES = {
    "smart_lost_cam": dict(scene=dict(kind="camera", tracks=_lost_tracks(37), n_poses=7, sigma=1.0, pixel_noise=0.3, see=0.55, priors=tuple(range(7))),
                           params=_LOST_PARAMS, variants={"epi": dict(enableEPI=True)}),
    "smart_lost_pose": dict(scene=dict(kind="pose", tracks=_lost_tracks(83, mixed=True), n_poses=9, sigma=1.5, pixel_noise=0.5, see=0.6,
                                       sensor=((0.02, -0.03, 0.01), (0.1, -0.05, 0.2)), between_chain=True, priors=(0,)),
                            params=_LOST_PARAMS, variants={}),
    "smart_lost_rig": dict(scene=dict(kind="rig", tracks=_lost_tracks(45), n_poses=6, sigma=1.0, pixel_noise=0.4, see=0.5,
                                      rig=(((520.0, 515.0, 0.3, 320.0, 240.0), ((0.02, -0.03, 0.01), (0.1, -0.05, 0.2))),
                                           ((500.0, 505.0, 0.0, 310.0, 245.0), ((0.01, 0.08, -0.02), (0.45, 0.0, 0.15)))),
                                      between_chain=True, priors=(0,)),
                           # a triangulation noise model: LOST's sigma is the mean of its sigmas, 0.4
                           params={**_LOST_PARAMS, "triangulationNoiseModel": (0.3, 0.5)}, variants={}),
}


def smart_lost_scene(name, seed=0, variant=None, scene=None, params=None):
    """(graph, initial values, info) of one of SMART_LOST_SCENES (or of its variant); LOST factors get the scene's parameters, DLT
    factors of a mixed scene the same with useLOST off.  `scene` / `params`: keyword arguments / parameter fields to replace."""
    from . import api as A
    spec = SMART_LOST_SCENES[name]
    fields = {**spec["params"], **(spec["variants"][variant] if variant else {}), **(params or {})}
    prm, dlt = A.SmartProjectionParams(), A.SmartProjectionParams()
    for k, v in fields.items():
        if k == "triangulationNoiseModel":
            v = A.noiseModel.Diagonal.Sigmas(v)
        setattr(prm, k, v)
        setattr(dlt, k, v)
    dlt.useLOST = False
    return smart_lost_graph(seed=seed, params=prm, dlt_params=dlt, **{**spec["scene"], **(scene or {})})


def _noisy_bearing(rng, q, sigma):
    """The direction of the local point q with a tangent-plane error of `sigma` radians, as a Unit3."""
    from . import api as A
    d = q / np.linalg.norm(q)
    return A.Unit3(d + sigma * rng.normal(size=3))


def _add_sam(graph, rng, kind, pose_key, point_key, q, model, bearing_sigma, range_sigma):
    """One bearing / range factor of `kind` (0 bearing-range, 1 range, 2 bearing) with a noisy measurement of the local point q."""
    from . import api as A
    r = float(np.linalg.norm(q)) + range_sigma * rng.normal()
    if kind == 0:
        graph.add(A.BearingRangeFactor3D(pose_key, point_key, _noisy_bearing(rng, q, bearing_sigma), r, model))
    elif kind == 1:
        graph.add(A.RangeFactor3D(pose_key, point_key, r, model))
    else:
        graph.add(A.BearingFactor3D(pose_key, point_key, _noisy_bearing(rng, q, bearing_sigma), model))


def sam3d_mixed_graph(n_poses=6, n_points=40, seed=3, bearing_sigma=0.004, range_sigma=0.02):
    """A small graph that enters every branch of BearingRangeFactor / RangeFactor / BearingFactor <Pose3, Point3> on the device, built
    through the API mirror: the arc of stereo_mixed_graph with monocular (Cal3_S2) and stereo factors on some landmarks and a
    bearing / range factor of every kind on all of them; dim-3 / dim-1 / dim-2 Unit, Isotropic, Diagonal and full Gaussian noise, one
    Robust(Huber) and one Robust(Cauchy); BetweenFactor<Pose3> along the arc and priors.  One more pose, X(n_poses), starts with the
    identity rotation and a translation of binary fractions, so that the direction it predicts for three more landmarks is exact in
    floating point: L(n_points) straight along +x with the measured bearing bit-equal to the predicted one (1 - x^2 < eps, x > 0),
    L(n_points + 1) along +y with the measured bearing exactly opposite (the (pi, 0) branch; a wide noise model: it is an outlier),
    L(n_points + 2) at (1, 1, 4): two equal smallest components (axis tie).  Graph order: projection, stereo, sam, between, prior.
    Returns (graph, initial values, {branch name: index among the sam factors})."""
    from . import api as A
    rng = np.random.default_rng(seed)
    ang = np.linspace(-0.5, 0.5, n_poses)
    centers = np.stack([8 * np.sin(ang), 0.3 * rng.normal(size=n_poses), -8 * np.cos(ang)], 1)
    R = _rodrigues(np.stack([0.02 * rng.normal(size=n_poses), -ang, 0.02 * rng.normal(size=n_poses)], 1))
    pts = np.stack([rng.uniform(-2, 2, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(-2, 2, n_points)], 1)
    t_id = np.array([0.5, -0.25, -9.0])                       # the identity-rotation pose
    special0 = t_id + np.array([[2.0, 0.0, 0.0], [0.0, 3.0, 0.0], [1.0, 1.0, 4.0]])     # initial values of the three branch landmarks
    special = special0 + rng.normal(0, 0.01, (3, 3))          # where they are
    R = np.concatenate([R, np.eye(3)[None]]); centers = np.concatenate([centers, t_id[None]])
    pts = np.concatenate([pts, special])
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    nm = A.noiseModel
    K1 = A.Cal3_S2Stereo(720.0, 715.0, 0.0, 600.0, 170.0, 0.54)
    Km = A.Cal3_S2(520.0, 515.0, 0.3, 320.0, 240.0)
    R3 = np.array([[90.0, 12.0, -6.0], [0.0, 110.0, 9.0], [0.0, 0.0, 30.0]]); R2 = np.array([[120.0, 15.0], [0.0, 95.0]])
    models = {0: [nm.Unit.Create(3), nm.Isotropic.Sigma(3, 0.02), nm.Diagonal.Sigmas([0.008, 0.01, 0.04]), nm.Gaussian.SqrtInformation(R3),
                  nm.Robust.Create(nm.mEstimator.Huber.Create(1.345), nm.Diagonal.Sigmas([0.006, 0.006, 0.03]))],
              1: [nm.Unit.Create(1), nm.Isotropic.Sigma(1, 0.03), nm.Diagonal.Sigmas([0.05], False), nm.Gaussian.SqrtInformation([[25.0]], False),
                  nm.Robust.Create(nm.mEstimator.Cauchy.Create(0.8), nm.Isotropic.Sigma(1, 0.03))],
              2: [nm.Unit.Create(2), nm.Isotropic.Sigma(2, 0.006), nm.Diagonal.Sigmas([0.005, 0.009]), nm.Gaussian.SqrtInformation(R2)]}
    m2, m3 = nm.Isotropic.Sigma(2, 1.5), nm.Isotropic.Sigma(3, 1.2)
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    for i in range(4):                                        # monocular factors on the first ten landmarks
        for j in range(10):
            q = R[i].T @ (pts[j] - centers[i]); u, v = q[0] / q[2], q[1] / q[2]
            z = np.array([Km.v[0] * u + Km.v[2] * v + Km.v[3], Km.v[1] * v + Km.v[4]]) + rng.normal(0, 1.0, 2)
            graph.add(A.GenericProjectionFactorCal3_S2(z, m2, X(i), L(j), Km))
    for i in range(n_poses):                                  # stereo factors on landmarks 5..19
        for j in range(5, 20):
            q = R[i].T @ (pts[j] - centers[i]); fx, fy, _, u0, v0, b = K1.v
            z = np.array([u0 + fx * q[0] / q[2], u0 + fx * (q[0] - b) / q[2], v0 + fy * q[1] / q[2]]) + rng.normal(0, 0.7, 3)
            graph.add(A.GenericStereoFactor3D(z, m3, X(i), L(j), K1))
    k, count = 0, {0: 0, 1: 0, 2: 0}
    for i in range(n_poses + 1):                              # a bearing / range factor of every kind, interleaved
        for j in range(n_points + 3):
            if i == n_poses and j >= n_points:
                continue                                      # (the identity pose's view of the branch landmarks: below)
            kind = k % 3
            _add_sam(graph, rng, kind, X(i), L(j), R[i].T @ (pts[j] - centers[i]), models[kind][count[kind] % len(models[kind])], bearing_sigma, range_sigma)
            count[kind] += 1; k += 1
    branch = {"same": k, "opposite": k + 1, "tie": k + 2}
    graph.add(A.BearingRangeFactor3D(X(n_poses), L(n_points), A.Unit3(1.0, 0.0, 0.0), 2.0 + range_sigma * rng.normal(), models[0][2]))
    graph.add(A.BearingFactor3D(X(n_poses), L(n_points + 1), A.Unit3(0.0, -1.0, 0.0), nm.Isotropic.Sigma(2, 40.0)))
    graph.add(A.BearingRangeFactor3D(X(n_poses), L(n_points + 2), _noisy_bearing(rng, special[2] - t_id, bearing_sigma),
                                     float(np.linalg.norm(special[2] - t_id)) + range_sigma * rng.normal(), models[0][3]))
    n6 = nm.Diagonal.Sigmas([0.01] * 3 + [0.05] * 3); n6b = nm.Diagonal.Sigmas([0.02, 0.02, 0.03, 0.1, 0.1, 0.15])
    for i in range(n_poses):
        Rz = R[i].T @ R[i + 1]; tz = R[i].T @ (centers[i + 1] - centers[i])
        graph.add(A.BetweenFactorPose3(X(i), X(i + 1), A.Pose3(A.Rot3(Rz @ _rodrigues(rng.normal(0, 0.005, (1, 3)))[0]), tz + rng.normal(0, 0.02, 3)), n6b))
    graph.addPriorPose3(X(0), A.Pose3(A.Rot3(R[0]), centers[0]), n6)
    graph.addPriorPose3(X(n_poses), A.Pose3(A.Rot3(np.eye(3)), t_id), n6)
    graph.addPriorPoint3(L(0), pts[0], nm.Isotropic.Sigma(3, 0.1))
    dR = _rodrigues(rng.normal(0, 0.01, (n_poses, 3)))
    for i in range(n_poses):
        initial.insert(X(i), A.Pose3(A.Rot3(R[i] @ dR[i]), centers[i] + rng.normal(0, 0.05, 3)))
    initial.insert(X(n_poses), A.Pose3(A.Rot3(np.eye(3)), t_id))
    for j in range(n_points):
        initial.insert(L(j), pts[j] + rng.normal(0, 0.05, 3))
    for j in range(3):
        initial.insert(L(n_points + j), special0[j])
    return graph, initial, branch


def landmark_slam3d_graph(n_poses=40, n_points=300, seed=11, views=10, bearing_sigma=0.005, range_sigma=0.03):
    """3-D landmark SLAM without a camera: a robot on a rising circle with odometry (BetweenFactorPose3) and a prior on its first
    pose; every landmark is seen from its `views` nearest poses by a BearingRangeFactor3D, a RangeFactor3D or a BearingFactor3D in
    turn (the first view of every landmark is a bearing-range one).  No calibration, no pixel: the graph of a lidar / sonar / UWB front
    end.  Fixed seed.  Returns (graph, initial values)."""
    from . import api as A
    rng = np.random.default_rng(seed)
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    nm = A.noiseModel
    th = np.linspace(0.0, 1.75 * np.pi, n_poses)
    centers = np.stack([12 * np.cos(th), 12 * np.sin(th), 0.05 * np.arange(n_poses)], 1)
    R = _rodrigues(np.stack([0.03 * rng.normal(size=n_poses), 0.03 * rng.normal(size=n_poses), th + np.pi / 2], 1))
    rad = rng.uniform(6.0, 18.0, n_points); phi = rng.uniform(0.0, 1.75 * np.pi, n_points)
    pts = np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(-2.0, 4.0, n_points)], 1)
    models = {0: nm.Diagonal.Sigmas([bearing_sigma, bearing_sigma, range_sigma]), 1: nm.Isotropic.Sigma(1, range_sigma),
              2: nm.Isotropic.Sigma(2, bearing_sigma)}
    odo = nm.Diagonal.Sigmas([0.01, 0.01, 0.01, 0.05, 0.05, 0.05])
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    for j in range(n_points):
        near = np.argsort(np.linalg.norm(centers - pts[j], axis=1))[:views]
        for k, i in enumerate(sorted(int(i) for i in near)):
            _add_sam(graph, rng, k % 3, X(i), L(j), R[i].T @ (pts[j] - centers[i]), models[k % 3], bearing_sigma, range_sigma)
    for i in range(n_poses - 1):
        Rz = R[i].T @ R[i + 1]; tz = R[i].T @ (centers[i + 1] - centers[i])
        graph.add(A.BetweenFactorPose3(X(i), X(i + 1), A.Pose3(A.Rot3(Rz @ _rodrigues(rng.normal(0, 0.01, (1, 3)))[0]), tz + rng.normal(0, 0.05, 3)), odo))
    graph.addPriorPose3(X(0), A.Pose3(A.Rot3(R[0]), centers[0]), nm.Diagonal.Sigmas([0.01] * 3 + [0.02] * 3))
    dR = _rodrigues(rng.normal(0, 0.02, (n_poses, 3)))
    for i in range(n_poses):
        initial.insert(X(i), A.Pose3(A.Rot3(R[i] @ dR[i]), centers[i] + rng.normal(0, 0.1, 3)))
    for j in range(n_points):
        initial.insert(L(j), pts[j] + rng.normal(0, 0.2, 3))
    return graph, initial


# ---- partial pose priors: PoseTranslationPrior / PoseRotationPrior <Pose3 | Pose2> -----------------------------------------------
# The scenes the fixtures of tests/golden/make_golden_pose_partial.py are recorded on.  No graph has a full PriorFactor: the gauge is
# fixed by position and attitude fixes alone.
def _partial_noise(A, rng, k, dim, scale):
    """The k-th partial prior's noise model: Unit, Isotropic, Diagonal, Gaussian in turn (`scale`: the size of a sigma)."""
    nm = A.noiseModel
    mode = k % 4
    if mode == 0:
        return nm.Unit.Create(dim)
    if mode == 1:
        return nm.Isotropic.Sigma(dim, scale, False)
    if mode == 2:
        return nm.Diagonal.Sigmas(scale * (1.0 + 0.5 * np.arange(dim)), False)
    R = np.triu(rng.normal(0, 0.2 / scale, (dim, dim))) + np.diag(rng.uniform(0.8, 1.6, dim) / scale)   # an upper-triangular sqrt information
    return nm.Gaussian.SqrtInformation(R, False)


def pose_partial_graph3d(n_poses=97, n_closures=23, seed=0):
    """A Pose3 pose graph anchored by partial priors alone: an odometry chain with drift (the initial values are the dead-reckoned
    odometry), `n_closures` loop closures, and 131 partial priors -- 95 PoseTranslationPrior3D (every pose but each eighth; a second
    one on every tenth pose) and 36 PoseRotationPrior3D (every third pose and poses 1, 50, 70) -- with Unit, Isotropic, Diagonal and
    Gaussian models in turn; a Huber model on the translation prior of pose 12 and a Cauchy model on that of pose 33, whose measurement
    is a gross outlier (30 m off).  Pose 0 carries two translation priors and a rotation prior.  The rotation prior of pose 1 measures
    the initial rotation of that pose bit for bit (the Taylor branch of SO3::Logmap), that of pose 50 is pi - 5e-5 away from it with a
    loose sigma (the near-pi branch); the others take the acos branch.
    Graph order: between factors, translation priors, rotation priors.  Returns (graph, initial values, info) with info["rot_taylor"],
    info["rot_near_pi"], info["outlier"], info["huber"] the indices of those factors among the partial priors."""
    from . import api as A
    rng = np.random.default_rng(seed)
    nm = A.noiseModel
    X = A.symbol_shorthand.X
    # truth: a slowly turning, climbing path
    step_w = np.stack([0.01 * rng.normal(size=n_poses), 0.01 * rng.normal(size=n_poses), 0.11 + 0.02 * rng.normal(size=n_poses)], 1)
    step_t = np.stack([1.0 + 0.05 * rng.normal(size=n_poses), 0.05 * rng.normal(size=n_poses), 0.03 + 0.01 * rng.normal(size=n_poses)], 1)
    dR = _rodrigues(step_w)
    R, t = [np.eye(3)], [np.zeros(3)]
    for i in range(1, n_poses):
        R.append(R[-1] @ dR[i]); t.append(t[-1] + R[-2] @ step_t[i])
    R, t = np.array(R), np.array(t)
    edges = [(i, i + 1) for i in range(n_poses - 1)]
    while len(edges) < n_poses - 1 + n_closures:
        a, b = sorted(int(x) for x in rng.integers(0, n_poses, 2))
        if b - a > 5 and (a, b) not in edges:
            edges.append((a, b))
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    n_odo = nm.Diagonal.Sigmas([0.01, 0.01, 0.015, 0.05, 0.05, 0.08], False)
    n_loop = nm.Isotropic.Sigma(6, 0.1, False)
    zs = []
    for k, (a, b) in enumerate(edges):
        zR = R[a].T @ R[b] @ _rodrigues(rng.normal(0, 0.01, (1, 3)))[0]
        zt = R[a].T @ (t[b] - t[a]) + rng.normal(0, 0.05, 3)
        zs.append((zR, zt))
        graph.add(A.BetweenFactorPose3(X(a), X(b), A.Pose3(A.Rot3(zR), zt), n_odo if k < n_poses - 1 else n_loop))
    # the initial values: the odometry composed from pose 0 (drift), pose 0 itself a little off the truth
    Ri, ti = [R[0] @ _rodrigues(np.array([[0.02, -0.01, 0.03]]))[0]], [t[0] + np.array([0.3, -0.2, 0.1])]
    for i in range(n_poses - 1):
        zR, zt = zs[i]
        ti.append(ti[-1] + Ri[-1] @ zt); Ri.append(Ri[-1] @ zR)
    for i in range(n_poses):
        initial.insert(X(i), A.Pose3(A.Rot3(Ri[i]), ti[i]))
    info, k = {}, 0
    trans = [i for i in range(n_poses) if i % 8 != 7] + list(range(0, n_poses, 10))
    for i in trans:
        z = t[i] + rng.normal(0, 0.3, 3)
        model = _partial_noise(A, rng, k, 3, 0.5)
        if k == 12:
            model = nm.Robust.Create(nm.mEstimator.Huber.Create(1.345), nm.Isotropic.Sigma(3, 0.4, False)); info["huber"] = k
        if k == 33:
            model = nm.Robust.Create(nm.mEstimator.Cauchy.Create(1.0), nm.Diagonal.Sigmas([0.4, 0.5, 0.6], False))
            z = z + np.array([30.0, -4.0, 2.0]); info["outlier"] = k
        graph.add(A.PoseTranslationPrior3D(X(i), A.Point3(*z), model) if k % 2 else A.PoseTranslationPrior3D(X(i), A.Pose3(A.Rot3(), z), model))
        k += 1
    for i in sorted(list(range(0, n_poses, 3)) + [1, 50, 70]):
        zR = R[i] @ _rodrigues(rng.normal(0, 0.02, (1, 3)))[0]
        model = _partial_noise(A, rng, k, 3, 0.05)
        if i == 1:
            zR = Ri[i].copy(); info["rot_taylor"] = k
        if i == 50:
            axis = np.array([0.6, -0.48, 0.64])
            zR = Ri[i] @ _rodrigues((np.pi - 5e-5) * axis[None])[0]
            model = nm.Isotropic.Sigma(3, 10.0, False); info["rot_near_pi"] = k
        graph.add(A.PoseRotationPrior3D(X(i), A.Rot3(zR), model) if k % 2 else A.PoseRotationPrior3D(X(i), A.Pose3(A.Rot3(zR), np.zeros(3)), model))
        k += 1
    return graph, initial, info


def pose_partial_vo_graph(seed=0, n_poses=16):
    """A smart-VO graph anchored by partial priors alone: smart_pose_graph's scene (SmartProjectionPose3Factor tracks, six explicit
    Point3 landmarks with GenericProjectionFactors, a BetweenFactor chain, NO full prior) with a PoseTranslationPrior3D on every fifth
    pose and one PoseRotationPrior3D on the first.  Graph order: smart, projection, between factors, then the partial priors.
    Returns (graph, initial values, info of smart_pose_graph)."""
    from . import api as A
    prm = A.SmartProjectionParams()
    prm.degeneracyMode = 1
    graph, initial, info = smart_pose_graph(n_poses=n_poses, n_tracks=67, seed=seed, arc=0.5, radius=8.0, box=(2.0, 1.5, 2.0),
                                            K=(520.0, 515.0, 0.3, 320.0, 240.0), sigma=1.5, pixel_noise=0.7, see=0.6, explicit_landmarks=6,
                                            between_chain=True, priors=(), init_noise=(0.004, 0.02), params=prm)
    rng = np.random.default_rng(seed + 1000)
    nm = A.noiseModel
    X = A.symbol_shorthand.X
    # (the scene returns the perturbed initial poses: the fixes are taken around them, a few centimetres and a degree off)
    for k, i in enumerate(range(0, n_poses, 5)):
        T = initial.at(X(i))
        graph.add(A.PoseTranslationPrior3D(X(i), A.Point3(*(T.translation() + rng.normal(0, 0.03, 3))), _partial_noise(A, rng, k + 1, 3, 0.05)))
    T = initial.at(X(0))
    graph.add(A.PoseRotationPrior3D(X(0), A.Rot3(T.rotation().matrix() @ _rodrigues(rng.normal(0, 0.01, (1, 3)))[0]), nm.Diagonal.Sigmas([0.02, 0.03, 0.02], False)))
    return graph, initial, info


def pose_partial_graph2d(n_poses=83, n_closures=9, seed=0):
    """A Pose2 pose graph anchored by partial priors alone: a chain once round a loop with `n_closures` loop closures, 31
    PoseTranslationPrior2D (every third pose and poses 1, 2, 4) and 15 PoseRotationPrior2D (every sixth pose and the wrap pose).  The
    wrap pose (info["wrap_pose"]; its factor info["wrap"] among the partial priors) starts at theta = -3.1 and its rotation prior
    measures 3.1: the residual is 2 pi - 6.2 = 0.083, not -6.2.  Returns (graph, initial values, info)."""
    from . import api as A
    rng = np.random.default_rng(seed)
    nm = A.noiseModel
    X = A.symbol_shorthand.X
    th = 2.0 + 2 * np.pi * np.arange(n_poses) / n_poses + 0.02 * rng.normal(size=n_poses)
    th = np.arctan2(np.sin(th), np.cos(th))
    xy = np.cumsum(np.stack([np.cos(th), np.sin(th)], 1) * 0.8, 0)

    def between(a, b):
        c, s = np.cos(th[a]), np.sin(th[a])
        d = xy[b] - xy[a]
        dth = th[b] - th[a]
        return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], np.arctan2(np.sin(dth), np.cos(dth))])

    edges = [(i, i + 1) for i in range(n_poses - 1)] + [(n_poses - 1, 0)]
    while len(edges) < n_poses + n_closures:
        a, b = sorted(int(x) for x in rng.integers(0, n_poses, 2))
        if b - a > 4 and (a, b) not in edges:
            edges.append((a, b))
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    n_odo = nm.Diagonal.Sigmas([0.05, 0.05, 0.02], False)
    for a, b in edges:
        z = between(a, b) + rng.normal(0, [0.03, 0.03, 0.01])
        graph.add(A.BetweenFactorPose2(X(a), X(b), A.Pose2(*z), n_odo))
    wrap_pose = int(np.argmin(np.abs(np.abs(th) - np.pi)))
    v0 = np.concatenate([xy + rng.normal(0, 0.15, xy.shape), (th + rng.normal(0, 0.05, n_poses))[:, None]], 1)
    v0[:, 2] = np.arctan2(np.sin(v0[:, 2]), np.cos(v0[:, 2]))
    v0[wrap_pose, 2] = -3.1
    for i in range(n_poses):
        initial.insert(X(i), A.Pose2(*v0[i]))
    info, k = {"wrap_pose": wrap_pose}, 0
    for i in sorted(set(range(0, n_poses, 3)) | {1, 2, 4}):
        z = xy[i] + rng.normal(0, 0.1, 2)
        model = _partial_noise(A, rng, k, 2, 0.2)
        graph.add(A.PoseTranslationPrior2D(X(i), A.Point2(*z), model) if k % 2 else A.PoseTranslationPrior2D(X(i), A.Pose2(z[0], z[1], 0.3), model))
        k += 1
    for i in sorted(set(range(0, n_poses, 6)) | {wrap_pose}):
        ang = th[i] + rng.normal(0, 0.02)
        model = nm.Unit.Create(1) if k % 3 == 0 else nm.Isotropic.Sigma(1, 0.05, False)
        if i == wrap_pose:
            ang = 3.1; info["wrap"] = k
        form = k % 3
        pose_z = ang if form == 0 else A.Rot2.fromAngle(ang) if form == 1 else A.Pose2(0.0, 0.0, ang)
        graph.add(A.PoseRotationPrior2D(X(i), pose_z, model))
        k += 1
    return graph, initial, info


# ---- planar landmark SLAM: BearingRangeFactor / RangeFactor / BearingFactor <Pose2, Point2> ----------------------------------------
def _pose2_between(a, b):
    """(x, y, theta) of a^-1 b for two (x, y, theta) rows."""
    c, s = np.cos(a[2]), np.sin(a[2])
    d = b[:2] - a[:2]
    dth = b[2] - a[2]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], np.arctan2(np.sin(dth), np.cos(dth))])


def _add_sam2(graph, rng, kind, pose_key, point_key, q, model, bearing_sigma, range_sigma):
    """One planar bearing / range factor of `kind` (0 bearing-range, 1 range, 2 bearing) with a noisy measurement of the local point q."""
    from . import api as A
    b = A.Rot2.fromAngle(float(np.arctan2(q[1], q[0])) + bearing_sigma * rng.normal())
    r = float(np.hypot(q[0], q[1])) + range_sigma * rng.normal()
    if kind == 0:
        graph.add(A.BearingRangeFactor2D(pose_key, point_key, b, r, model))
    elif kind == 1:
        graph.add(A.RangeFactor2D(pose_key, point_key, r, model))
    else:
        graph.add(A.BearingFactor2D(pose_key, point_key, b, model))


def planar_mixed_graph(n_poses=11, n_points=30, seed=5, views=8, bearing_sigma=0.01, range_sigma=0.03):
    """A small planar graph that enters every branch of BearingRangeFactor / RangeFactor / BearingFactor <Pose2, Point2> on the device,
    built through the API mirror: a robot on an arc sees its `views` nearest landmarks by a factor of every kind in turn; dim-2 and dim-1
    Unit, Isotropic, Diagonal and full Gaussian noise, one Robust(Huber) and one Robust(Cauchy); a BetweenFactorPose2 chain, one
    PriorFactorPose2 and two 2-D partial priors.  One more pose, X(n_poses), starts with theta = 0 and a translation of binary fractions,
    so that what it predicts for three more landmarks is exact in floating point:
      L(n_points)      at t + (3, 4): the predicted Rot2 is (3/5, 4/5) and the measured one holds the same two doubles ("same");
      L(n_points + 1)  starts ON the pose: a BearingFactor2D (relativeBearing below 1e-5: a zero Jacobian, "bearing_zero") and a
                       RangeFactor2D (norm2 at 0: the Jacobian (1, 1), "range_zero") see it there; the landmark itself lies elsewhere and two
                       other poses see it;
      L(n_points + 2)  behind the pose, a little to the left (predicted bearing just below pi) with a measured bearing just above -pi:
                       the residual crosses the cut ("wrap").
    Graph order: planar factors, between, prior, partial priors.  Returns (graph, initial values, {branch name: index among the planar
    factors})."""
    from . import api as A
    rng = np.random.default_rng(seed)
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    nm = A.noiseModel
    ang = np.linspace(0.3, 2.4, n_poses)
    poses = np.stack([7 * np.cos(ang), 7 * np.sin(ang), ang + np.pi / 2 + 0.05 * rng.normal(size=n_poses)], 1)
    t_id = np.array([0.5, -0.25])
    poses = np.concatenate([poses, [[t_id[0], t_id[1], 0.0]]])
    rad = rng.uniform(3.0, 11.0, n_points); phi = rng.uniform(0.0, 2.7, n_points)
    pts = np.stack([rad * np.cos(phi), rad * np.sin(phi)], 1)
    special = t_id + np.array([[3.0, 4.0], [1.5, 1.0], [-3.0, 0.015625]])       # where the three branch landmarks are
    special0 = np.array([special[0], t_id, special[2]])                         # ... and where they start
    pts = np.concatenate([pts, special])
    R2 = np.array([[80.0, 9.0], [0.0, 30.0]])
    models = {0: [nm.Unit.Create(2), nm.Isotropic.Sigma(2, 0.05), nm.Diagonal.Sigmas([bearing_sigma, range_sigma]), nm.Gaussian.SqrtInformation(R2),
                  nm.Robust.Create(nm.mEstimator.Huber.Create(1.345), nm.Diagonal.Sigmas([0.012, 0.04]))],
              1: [nm.Unit.Create(1), nm.Isotropic.Sigma(1, range_sigma), nm.Diagonal.Sigmas([0.05], False), nm.Gaussian.SqrtInformation([[25.0]], False),
                  nm.Robust.Create(nm.mEstimator.Cauchy.Create(0.8), nm.Isotropic.Sigma(1, 0.04))],
              2: [nm.Unit.Create(1), nm.Isotropic.Sigma(1, bearing_sigma), nm.Diagonal.Sigmas([0.02], False), nm.Gaussian.SqrtInformation([[70.0]], False)]}

    def local(i, j):
        c, s = np.cos(poses[i, 2]), np.sin(poses[i, 2])
        d = pts[j] - poses[i, :2]
        return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])

    graph, initial = A.NonlinearFactorGraph(), A.Values()
    k, count = 0, {0: 0, 1: 0, 2: 0}
    for i in range(n_poses):
        near = np.argsort(np.linalg.norm(pts[:n_points] - poses[i, :2], axis=1))[:views]
        for j in sorted(int(j) for j in near):
            kind = k % 3
            _add_sam2(graph, rng, kind, X(i), L(j), local(i, j), models[kind][count[kind] % len(models[kind])], bearing_sigma, range_sigma)
            count[kind] += 1; k += 1
    for j in range(n_points):                                  # every landmark is seen at least twice with a bearing and a range
        for i in (j % n_poses, (j + 5) % n_poses):
            _add_sam2(graph, rng, 0, X(i), L(j), local(i, j), models[0][2], bearing_sigma, range_sigma); k += 1
    for j in range(3):                                         # the branch landmarks from two poses of the arc
        for i in (1, n_poses - 2):
            _add_sam2(graph, rng, 0, X(i), L(n_points + j), local(i, n_points + j), models[0][2], bearing_sigma, range_sigma); k += 1
    branch = {"same": k, "bearing_zero": k + 1, "range_zero": k + 2, "wrap": k + 3}
    graph.add(A.BearingRangeFactor2D(X(n_poses), L(n_points), A.Rot2.fromCosSin(3.0 / 5.0, 4.0 / 5.0), 5.0 + range_sigma * rng.normal(), models[0][2]))
    q1 = special[1] - t_id
    graph.add(A.BearingFactor2D(X(n_poses), L(n_points + 1), A.Rot2.fromAngle(float(np.arctan2(q1[1], q1[0])) + bearing_sigma * rng.normal()), nm.Isotropic.Sigma(1, 0.2)))
    graph.add(A.RangeFactor2D(X(n_poses), L(n_points + 1), float(np.hypot(q1[0], q1[1])) + range_sigma * rng.normal(), nm.Isotropic.Sigma(1, 0.5)))
    graph.add(A.BearingFactor2D(X(n_poses), L(n_points + 2), A.Rot2.fromAngle(-(np.pi - 0.015)), nm.Isotropic.Sigma(1, 0.05)))
    n_odo = nm.Diagonal.Sigmas([0.05, 0.05, 0.02]); n_odo_g = nm.Gaussian.SqrtInformation(np.array([[20.0, 2.0, -1.0], [0.0, 18.0, 3.0], [0.0, 0.0, 45.0]]))
    for i in range(n_poses):
        z = _pose2_between(poses[i], poses[i + 1]) + rng.normal(0, [0.03, 0.03, 0.01])
        graph.add(A.BetweenFactorPose2(X(i), X(i + 1), A.Pose2(*z), n_odo_g if i % 3 == 1 else n_odo))
    graph.addPriorPose2(X(0), A.Pose2(*poses[0]), nm.Diagonal.Sigmas([0.02, 0.02, 0.01]))
    graph.add(A.PoseTranslationPrior2D(X(n_poses), A.Point2(*t_id), nm.Isotropic.Sigma(2, 0.02)))
    graph.add(A.PoseRotationPrior2D(X(n_poses), A.Rot2.fromAngle(0.0), nm.Isotropic.Sigma(1, 0.01)))
    for i in range(n_poses):
        initial.insert(X(i), A.Pose2(*(poses[i] + rng.normal(0, [0.08, 0.08, 0.02]))))
    initial.insert(X(n_poses), A.Pose2(t_id[0], t_id[1], 0.0))
    for j in range(n_points):
        initial.insert(L(j), A.Point2(*(pts[j] + rng.normal(0, 0.1, 2))))
    for j in range(3):
        initial.insert(L(n_points + j), A.Point2(*special0[j]))
    return graph, initial, branch


def planar_slam_graph(n_poses=40, n_points=120, seed=11, views=9, bearing_sigma=0.01, range_sigma=0.05):
    """Planar landmark SLAM: a robot once round a circle with odometry (BetweenFactorPose2) and a prior on its first pose; every
    landmark is seen from its `views` nearest poses by a BearingRangeFactor2D, a RangeFactor2D or a BearingFactor2D in turn (the first
    view of every landmark is a bearing-range one).  The graph of a 2-D lidar front end.  Returns (graph, initial values)."""
    from . import api as A
    rng = np.random.default_rng(seed)
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    nm = A.noiseModel
    th = np.linspace(0.0, 1.8 * np.pi, n_poses)
    poses = np.stack([12 * np.cos(th), 12 * np.sin(th), th + np.pi / 2 + 0.03 * rng.normal(size=n_poses)], 1)
    poses[:, 2] = np.arctan2(np.sin(poses[:, 2]), np.cos(poses[:, 2]))
    rad = rng.uniform(5.0, 19.0, n_points); phi = rng.uniform(0.0, 1.8 * np.pi, n_points)
    pts = np.stack([rad * np.cos(phi), rad * np.sin(phi)], 1)
    models = {0: nm.Diagonal.Sigmas([bearing_sigma, range_sigma]), 1: nm.Isotropic.Sigma(1, range_sigma), 2: nm.Isotropic.Sigma(1, bearing_sigma)}
    odo = nm.Diagonal.Sigmas([0.05, 0.05, 0.01])
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    for j in range(n_points):
        near = np.argsort(np.linalg.norm(poses[:, :2] - pts[j], axis=1))[:views]
        for k, i in enumerate(sorted(int(i) for i in near)):
            c, s = np.cos(poses[i, 2]), np.sin(poses[i, 2])
            d = pts[j] - poses[i, :2]
            _add_sam2(graph, rng, k % 3, X(i), L(j), np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]]), models[k % 3], bearing_sigma, range_sigma)
    for i in range(n_poses - 1):
        graph.add(A.BetweenFactorPose2(X(i), X(i + 1), A.Pose2(*(_pose2_between(poses[i], poses[i + 1]) + rng.normal(0, [0.04, 0.04, 0.01]))), odo))
    graph.addPriorPose2(X(0), A.Pose2(*poses[0]), nm.Diagonal.Sigmas([0.02, 0.02, 0.01]))
    for i in range(n_poses):
        v = poses[i] + rng.normal(0, [0.1, 0.1, 0.03])
        initial.insert(X(i), A.Pose2(v[0], v[1], float(np.arctan2(np.sin(v[2]), np.cos(v[2])))))
    for j in range(n_points):
        initial.insert(L(j), A.Point2(*(pts[j] + rng.normal(0, 0.2, 2))))
    return graph, initial


def planar_slam_example():
    """The graph of the reference's examples/PlanarSLAMExample.cpp: three poses with a prior and two odometry factors, two landmarks
    seen by three BearingRangeFactor2D.  Returns (graph, initial values)."""
    from . import api as A
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    nm = A.noiseModel
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    graph.addPriorPose2(X(1), A.Pose2(0.0, 0.0, 0.0), nm.Diagonal.Sigmas([0.3, 0.3, 0.1]))
    odo = nm.Diagonal.Sigmas([0.2, 0.2, 0.1])
    graph.add(A.BetweenFactorPose2(X(1), X(2), A.Pose2(2.0, 0.0, 0.0), odo))
    graph.add(A.BetweenFactorPose2(X(2), X(3), A.Pose2(2.0, 0.0, 0.0), odo))
    meas = nm.Diagonal.Sigmas([0.1, 0.2])
    graph.add(A.BearingRangeFactor2D(X(1), L(1), A.Rot2.fromAngle(np.pi * 45 / 180), np.sqrt(4.0 + 4.0), meas))
    graph.add(A.BearingRangeFactor2D(X(2), L(1), A.Rot2.fromAngle(np.pi * 90 / 180), 2.0, meas))
    graph.add(A.BearingRangeFactor2D(X(3), L(2), A.Rot2.fromAngle(np.pi * 90 / 180), 2.0, meas))
    initial.insert(X(1), A.Pose2(0.5, 0.0, 0.2)); initial.insert(X(2), A.Pose2(2.3, 0.1, -0.2)); initial.insert(X(3), A.Pose2(4.1, 0.1, 0.1))
    initial.insert(L(1), A.Point2(1.8, 2.1)); initial.insert(L(2), A.Point2(4.1, 1.8))
    return graph, initial


def _project_pixel(K, Rw, tw, pt):
    """The pixel of a world point through the calibration object K (Cal3_S2, Cal3DS2 or Cal3Fisheye of the API mirror) of a camera at
    (Rw, tw), or None behind the camera; for building scenes."""
    q = Rw.T @ (pt - tw)
    if q[2] <= 0:
        return None
    u, v = q[0] / q[2], q[1] / q[2]
    if hasattr(K, "uncalibrate"):
        return K.uncalibrate((u, v))
    fx, fy, s, u0, v0 = K.v[:5]
    if K.v.size == 9:       # Cal3DS2: radial and tangential distortion of the intrinsic point
        k1, k2, p1, p2 = K.v[5:]
        rr = u * u + v * v; g = 1 + k1 * rr + k2 * rr * rr
        u, v = g * u + 2 * p1 * u * v + p2 * (rr + 2 * u * u), g * v + 2 * p2 * u * v + p1 * (rr + 2 * v * v)
    return np.array([fx * u + s * v + u0, fy * v + v0])


def fisheye_example_graph():
    """The graph of the reference's examples/FisheyeExample.cpp: the eight corners of the cube of examples/SFMdata.h seen from its eight
    poses on a circle of radius 30, every (pose, corner) pair a GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> with the exact
    projection as its measurement and the example's calibration literal; a prior on the first pose and on the first corner; the
    example's perturbed initial values.  Graph order as in the example: the two priors, then the projection factors pose by pose.
    Returns (graph, initial values)."""
    from . import api as A
    from .io import _ypr
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    nm = A.noiseModel
    K = A.Cal3Fisheye(278.66, 278.48, 0.0, 319.75, 241.96, -0.013721808247486035, 0.020727425669427896, -0.012786476702685545,
                      0.0025242267320687625)
    points = np.array([[10.0, 10.0, 10.0], [-10.0, 10.0, 10.0], [-10.0, -10.0, 10.0], [10.0, -10.0, 10.0],
                       [10.0, 10.0, -10.0], [-10.0, 10.0, -10.0], [-10.0, -10.0, -10.0], [10.0, -10.0, -10.0]])
    Rd, td = _ypr(0.0, -np.pi / 4, 0.0), np.array([np.sin(np.pi / 4) * 30, 0.0, 30 * (1 - np.sin(np.pi / 4))])
    poses = [(_ypr(np.pi / 2, 0.0, -np.pi / 2), np.array([30.0, 0.0, 0.0]))]
    for _ in range(7):
        Rp, tp = poses[-1]
        poses.append((Rp @ Rd, tp + Rp @ td))
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    graph.addPriorPose3(X(0), A.Pose3(A.Rot3(poses[0][0]), poses[0][1]), nm.Diagonal.Sigmas([0.1] * 3 + [0.3] * 3))
    graph.addPriorPoint3(L(0), points[0], nm.Isotropic.Sigma(3, 0.1))
    noise = nm.Isotropic.Sigma(2, 1.0)
    for j, pt in enumerate(points):
        initial.insert(L(j), pt + np.array([-0.25, 0.20, 0.15]))
    Rk, tk = _rodrigues(np.array([[-0.1, 0.2, 0.25]]))[0], np.array([0.05, -0.10, 0.20])
    for i, (Rp, tp) in enumerate(poses):
        for j, pt in enumerate(points):
            graph.add(A.GenericProjectionFactorCal3Fisheye(_project_pixel(K, Rp, tp, pt), noise, X(i), L(j), K))
        initial.insert(X(i), A.Pose3(A.Rot3(Rp @ Rk), tp + Rp @ tk))
    return graph, initial


def fisheye_mixed_graph(n_poses=11, n_points=36, seed=0):
    """A small rig graph that enters every branch of GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> on the device, built through the
    API mirror the way user code would: poses on an arc looking at a point cloud, every (pose, landmark) pair a projection factor whose
    calibration cycles through two Cal3Fisheye (the second with a NON-ZERO skew), a Cal3_S2 and a Cal3DS2; every third factor is
    mounted through one of two body_P_sensor; dim-2 Unit / Isotropic / Diagonal / Gaussian noise, Robust(Huber) and Robust(Cauchy);
    BetweenFactor<Pose3> along the arc, a prior on the first pose and on one landmark.  The middle pose starts with the identity
    rotation, and three factors are in a branch of their own AT THE INITIAL VALUES:
      on_axis  a landmark exactly on the optical axis of the middle pose (r^2 == 0), through the skewed fisheye calibration, Unit noise;
      taylor   a landmark with 0 < r = 1e-9 from the same pose (the Taylor branch of Cal3Fisheye::Scaling);
      behind   the last landmark, 0.5 behind pose 0 (cheirality), which only the last two poses see from the front, Isotropic(1.5).
    Graph order: projection, between, prior.  Returns (graph, initial values, {branch name: index among the projection factors})."""
    from . import api as A
    rng = np.random.default_rng(seed)
    mid = n_poses // 2
    ang = np.linspace(-0.5, 0.5, n_poses)
    centers = np.stack([8 * np.sin(ang), 0.25 + 0.1 * rng.normal(size=n_poses), -8 * np.cos(ang)], 1)
    R = _rodrigues(np.stack([0.02 * rng.normal(size=n_poses), -ang, 0.02 * rng.normal(size=n_poses)], 1))   # looks at the origin (+z)
    pts = np.stack([rng.uniform(-2, 2, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(-2, 2, n_points)], 1)
    t_mid = np.array([0.0, 0.25, -8.0])                                        # where the middle pose starts, with the identity rotation
    pts[0] = t_mid + np.array([0.0, 0.0, 8.0]) + rng.normal(0, 0.03, 3)       # starts on its optical axis
    pts[1] = t_mid + np.array([0.0, 0.0, 7.0]) + rng.normal(0, 0.03, 3)       # starts 1e-9 off it
    pts[-1] = centers[0] - 0.5 * R[0][:, 2] + np.array([0.2, -0.1, 0.0])       # 0.5 behind pose 0 along its optical axis
    X, L = A.symbol_shorthand.X, A.symbol_shorthand.L
    Kf = A.Cal3Fisheye(278.66, 278.48, 0.0, 319.75, 241.96, -0.013721808247486035, 0.020727425669427896, -0.012786476702685545,
                       0.0025242267320687625)
    Ks = A.Cal3Fisheye(300.0, 295.0, 0.8, 320.0, 240.0, -0.02, 0.01, -0.005, 0.001)      # skew 0.8: DK's off-diagonal entry
    Km = A.Cal3_S2(520.0, 515.0, 0.3, 320.0, 240.0)
    Kd = A.Cal3DS2(400.0, 400.0, 0.0, 300.0, 200.0, 0.05, -0.01, 0.001, -0.002)
    cals = [Kf, Km, Ks, Kd]
    sensors = []
    for w, t in (([0.02, -0.03, 0.01], [0.1, -0.05, 0.2]), ([-0.01, 0.04, 0.02], [-0.08, 0.03, 0.1])):
        sensors.append((_rodrigues(np.array([w]))[0], np.array(t)))
    Rg = np.array([[1.1, 0.2], [0.0, 0.9]])
    nm = A.noiseModel
    models = [nm.Unit.Create(2), nm.Isotropic.Sigma(2, 1.5), nm.Diagonal.Sigmas([1.0, 1.3]), nm.Gaussian.SqrtInformation(Rg),
              nm.Robust.Create(nm.mEstimator.Huber.Create(1.345), nm.Isotropic.Sigma(2, 1.2)),
              nm.Robust.Create(nm.mEstimator.Cauchy.Create(2.0), nm.Diagonal.Sigmas([1.1, 0.9]))]
    graph, initial = A.NonlinearFactorGraph(), A.Values()
    branch, k = {}, 0
    for i in range(n_poses):
        for j in range(n_points):
            if j == n_points - 1 and 0 < i < n_poses - 2:
                continue                                  # (the last landmark: seen from behind by pose 0, from the front by the last two poses only)
            K, sen, model = cals[k % 4], sensors[(k // 3) % 2] if k % 3 == 0 else None, models[(k + k // 4) % 6]      # (every noise kind under every calibration)
            if i == mid and j == 0:
                branch["on_axis"] = k; K, sen, model = Ks, None, models[0]      # (Unit: the record is the factor's own Jacobian)
            elif i == mid and j == 1:
                branch["taylor"] = k; K, sen = Kf, None
            elif i == 0 and j == n_points - 1:
                branch["behind"] = k; K, sen, model = Kf, None, models[1]       # (Isotropic 1.5: the residual is 2 fx / 1.5 in both rows)
            Rw, tw = (R[i], centers[i]) if sen is None else (R[i] @ sen[0], centers[i] + R[i] @ sen[1])
            z = _project_pixel(K, Rw, tw, pts[j])
            z = rng.normal(300.0, 50.0, 2) if z is None else z + rng.normal(0, 0.7, 2)
            graph.add(type_of_projection(A, K)(z, model, X(i), L(j), K, None if sen is None else A.Pose3(A.Rot3(sen[0]), sen[1])))
            k += 1
    n6 = nm.Diagonal.Sigmas([0.01] * 3 + [0.05] * 3); n6b = nm.Diagonal.Sigmas([0.02, 0.02, 0.03, 0.1, 0.1, 0.15])
    for i in range(n_poses - 1):
        Rz = R[i].T @ R[i + 1]; tz = R[i].T @ (centers[i + 1] - centers[i])
        graph.add(A.BetweenFactorPose3(X(i), X(i + 1), A.Pose3(A.Rot3(Rz @ _rodrigues(rng.normal(0, 0.005, (1, 3)))[0]), tz + rng.normal(0, 0.02, 3)), n6b))
    graph.addPriorPose3(X(0), A.Pose3(A.Rot3(R[0]), centers[0]), n6)
    graph.addPriorPoint3(L(2), pts[2], nm.Isotropic.Sigma(3, 0.1))
    dR = _rodrigues(rng.normal(0, 0.01, (n_poses, 3)))
    for i in range(n_poses):
        if i == mid:
            initial.insert(X(i), A.Pose3(A.Rot3(np.eye(3)), t_mid))
        else:
            initial.insert(X(i), A.Pose3(A.Rot3(R[i] @ dR[i]), centers[i] + rng.normal(0, 0.05, 3)))
    for j in range(n_points):
        initial.insert(L(j), pts[j] + rng.normal(0, 0.05, 3))
    initial.update(L(0), t_mid + np.array([0.0, 0.0, 8.0]))
    initial.update(L(1), t_mid + np.array([7e-9, 0.0, 7.0]))
    return graph, initial, branch


def type_of_projection(A, K):
    """The GenericProjectionFactor instantiation of the API mirror for a calibration object."""
    return {A.Cal3_S2: A.GenericProjectionFactorCal3_S2, A.Cal3DS2: A.GenericProjectionFactorCal3DS2,
            A.Cal3Fisheye: A.GenericProjectionFactorCal3Fisheye}[type(K)]
