"""SmartProjectionRigFactor on the CPU: the arithmetic that completes the diagonal blocks of a pose named several times in one track
(factors.h::smart_repeat_cross, what k_smart_hdiag_repeats and k_pcg_setup_repeats run per lane) compiled for the host
(tests/hostmath/hostmath_smart_rig.cpp) against dense numpy algebra on the UNIQUE keys: H = F^T F - F^T E P E^T F with the block
column of a sighting placed at its key (CameraSet::SchurComplementAndRearrangeBlocks, slam/SmartProjectionRigFactor.h:312-322).

Tolerance: 1e-12 of the block's largest entry -- both sides are sums of a few dozen products of numbers of order 1 in double
precision (eps 1.1e-16), in different orders; nothing is cancelled beyond the subtraction of the two O(1) terms themselves."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 32        # doubles per E slot (context.h::kEStride)


@pytest.fixture(scope="module")
def hm():
    so = os.path.join(ROOT, "tests", "_build", "libhostmath_smart_rig.so")
    src = os.path.join(ROOT, "tests", "hostmath", "hostmath_smart_rig.cpp")
    deps = [src, os.path.join(ROOT, "gtsam_amd", "csrc", "factors.h"), os.path.join(ROOT, "gtsam_amd", "csrc", "geom.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.hmsr_repeat_cross.restype = C.c_double
    lib.hmsr_repeat_cross.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    return lib


def track(rng, keys):
    """whitened F_a (2 x 6) and E_a (2 x 3) of a track with the pose keys `keys` (one per sighting), its E slots
    F_a^T E_a L^-T (6 x 3 in a slot of STRIDE doubles, rows >= 6 zero) with L L^T = E^T E, and P = (E^T E)^-1"""
    m = len(keys)
    F = rng.normal(size=(m, 2, 6)); E = rng.normal(size=(m, 2, 3))
    EtE = np.einsum("aki,akj->ij", E, E)
    Linv = np.linalg.inv(np.linalg.cholesky(EtE))
    slots = np.zeros((m, STRIDE))
    for a in range(m):
        slots[a, :18] = (F[a].T @ E[a] @ Linv.T).reshape(-1)
    return F, E, np.linalg.inv(EtE), slots


def dense_blocks(F, E, P, keys):
    """diagonal blocks of F^T F - F^T E P E^T F on the unique keys (first-appearance order), by key"""
    uniq = list(dict.fromkeys(keys))
    m = len(keys)
    Fu = np.zeros((2 * m, 6 * len(uniq)))
    for a, k in enumerate(keys):
        Fu[2 * a:2 * a + 2, 6 * uniq.index(k):6 * uniq.index(k) + 6] = F[a]
    Es = E.reshape(2 * m, 3)
    H = Fu.T @ Fu - Fu.T @ Es @ P @ Es.T @ Fu
    return {k: H[6 * u:6 * u + 6, 6 * u:6 * u + 6] for u, k in enumerate(uniq)}


# the keys of a track, one per sighting: two cameras from every pose; one pose only; three cameras, one pose seen by all three and
# out of order; no repetition at all
CASES = ([0, 0, 1, 1, 2, 2], [5, 5], [3, 1, 3, 2, 1, 3, 4], [0, 1, 2])


@pytest.mark.parametrize("keys", CASES)
def test_cross_terms_complete_the_per_observation_blocks_to_the_unique_key_blocks(hm, keys):
    rng = np.random.default_rng(len(keys))
    F, E, P, slots = track(rng, keys)
    want = dense_blocks(F, E, P, keys)
    # the slots of the track somewhere inside a longer, shuffled range, as the projection range holds them
    n_range = 3 * len(keys) + 5
    place = rng.permutation(n_range)[:len(keys)]
    rng_E = rng.normal(size=(n_range, STRIDE))
    rng_E[place] = slots
    rng_E = np.ascontiguousarray(rng_E)
    for k in dict.fromkeys(keys):
        mine = [a for a, kk in enumerate(keys) if kk == k]
        obs = np.ascontiguousarray(np.sort(place[mine]), np.int32)          # range order, as upload_smart_repeats lists a group
        per_obs = sum(F[a].T @ F[a] - slots[a, :18].reshape(6, 3) @ slots[a, :18].reshape(6, 3).T for a in mine)
        cross = np.array([[hm.hmsr_repeat_cross(rng_E.ctypes.data, STRIDE, obs.ctypes.data, obs.size, i, j) for j in range(6)] for i in range(6)])
        assert np.array_equal(cross, cross.T)
        got = per_obs - cross
        assert np.abs(got - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), (keys, k)
        if len(mine) == 1:
            assert not cross.any()       # a single sighting has no cross terms: exactly zero
        else:                            # ... and several have: the per-observation block alone is not the unique-key block
            assert np.abs(per_obs - want[k]).max() > 1e-6 * np.abs(want[k]).max()


def test_diagonal_entries_are_what_the_hessian_diagonal_kernel_subtracts(hm):
    """k_smart_hdiag_repeats uses the entries (i, i): 2 sum_{a<b} row_i(E_a) . row_i(E_b) = |row_i(sum E)|^2 - sum |row_i(E)|^2"""
    rng = np.random.default_rng(7)
    slots = np.ascontiguousarray(rng.normal(size=(4, STRIDE)))
    obs = np.arange(4, dtype=np.int32)
    e = slots[:, :18].reshape(4, 6, 3)
    for i in range(6):
        want = (e[:, i].sum(0) ** 2).sum() - (e[:, i] ** 2).sum()
        got = hm.hmsr_repeat_cross(slots.ctypes.data, STRIDE, obs.ctypes.data, 4, i, i)
        assert abs(got - want) <= 1e-12 * (e[:, i] ** 2).sum()
