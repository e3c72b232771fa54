"""CPU checks of the covariance layer: the numpy recursion against explicit transition products on oracle step blocks and
against itself in extended precision, the packed layout, the wrapper's Sigma0 forms, argument validation that needs no
device, and the ctypes table."""
import ctypes as C

import numpy as np
import pytest

from tests import tracking_cov_ref as CR
from tests import tracking_ref as TR

CASES = [(2, 1, 1), (2, 3, 2), (3, 2, 1), (6, 3, 1), (6, 7, 2), (12, 8, 2), (12, 11, 1)]


def _problem(N, k_trans, init_mode, seed):
    from quadruped_landing_amd import problem_gen as PG

    b = PG.make_batch(1, N, min(max(k_trans, 2), N - 1) if N > 2 else 2, init_mode, seed=seed)
    rng = np.random.default_rng(seed)
    A, B = TR.oracle_blocks(N, k_trans, init_mode, b.Z[0])
    K = 0.05 * rng.normal(size=(N - 1, 4, 15))
    return A, B, K, CR.random_psd(rng), rng.uniform(0.0, 1e-2, size=15), b


@pytest.mark.parametrize("N,k_trans,init_mode", CASES)
@pytest.mark.parametrize("with_gains", [False, True])
def test_recursion_equals_the_explicit_transition_products(N, k_trans, init_mode, with_gains):
    """Both sides are float64 products of at most N-1 <= 11 blocks: they differ by rounding only, and the project's bar for
    such sweeps (1e-10 per knot, relative Frobenius) holds with orders of magnitude to spare."""
    A, B, K, S0, W, _ = _problem(N, k_trans, init_mode, seed=7 * N + k_trans)
    K = K if with_gains else None
    for Wd in (None, W):
        got = CR.propagate(A, B, K, S0, Wd)
        ref = CR.explicit(A, B, K, S0, Wd)
        assert np.array_equal(got, np.swapaxes(got, -1, -2))
        assert np.array_equal(got[0], CR.unpack(CR.pack(S0)))
        e = CR.knot_rel(got, ref)
        assert e <= 1e-10, e
    if 0 <= k_trans - 2 < N - 1:  # the jump knot keeps the clock and adds W behind it like every other knot
        S = CR.propagate(A, B, None, np.diag(np.arange(1.0, 16.0)), W)
        kj = k_trans - 2
        assert S[kj + 1, 14, 14] == S[kj, 14, 14] + W[14]
        assert S[kj + 1, 4, 4] == W[4] and S[kj + 1, 6, 6] == W[6]


def test_the_recursion_own_rounding_on_the_notebook_problem(golden_dir):
    """float64 against longdouble on the notebook problem at data_6.csv, gains from the numpy Riccati: how far the
    yardstick itself is from exact, to be set against the GPU tests' 1e-10 (where longdouble is no wider than float64 the
    comparison is trivially exact)."""
    import os

    from quadruped_landing_amd import problem_gen as PG, trajectory_io as TIO

    nb = PG.notebook_problem()
    Z = np.asarray(TIO.load_trajectory(os.path.join(golden_dir, "data_6.csv"), nb.N)).reshape(-1)[: 20 * nb.N - 5]
    A, B = TR.oracle_blocks(nb.N, int(nb.k_trans[0]), int(nb.init_mode[0]), Z)  # the default model is the notebook's
    Q = np.array([10.0] * 14 + [0.0])
    R = np.array([1e-3, 1e-2, 1e-3, 1e-2])
    K, _ = TR.riccati(A, B, Q, R, Q)
    S0 = np.diag(np.full(15, 1e-3))
    ld = np.longdouble
    for name, gains in (("closed loop", K), ("open loop", None)):
        lo = CR.propagate(A, B, gains, S0)
        hi = CR.propagate(A.astype(ld), B.astype(ld), None if gains is None else gains.astype(ld), S0.astype(ld))
        e = CR.knot_rel(lo, hi)
        print(f"float64 vs longdouble recursion, {name}: {e:.2e}")
        assert e <= 1e-12, (name, e)


def test_packed_layout_round_trips():
    from quadruped_landing_amd import nlp

    rng = np.random.default_rng(0)
    M = rng.normal(size=(3, 2, 15, 15))
    M = M + np.swapaxes(M, -1, -2)
    packed = np.zeros((3, 2, 120))
    for i in range(15):
        for j in range(i + 1):
            packed[..., i * (i + 1) // 2 + j] = M[..., i, j]
    np.testing.assert_array_equal(CR.pack(M), packed)
    np.testing.assert_array_equal(CR.unpack(packed), M)
    np.testing.assert_array_equal(nlp.unpack_covariance(packed), M)
    np.testing.assert_array_equal(nlp.pack_covariance(M), packed)
    np.testing.assert_array_equal(nlp.pack_covariance(nlp.unpack_covariance(packed)), packed)


def test_marginals_of_a_known_covariance():
    lb = 0.4
    S = np.zeros((2, 15, 15))
    S[:] = np.diag(np.arange(1.0, 16.0))
    S[:, 1, 2] = S[:, 2, 1] = 0.5
    K = np.zeros((1, 4, 15))
    K[0, 1, 3] = 2.0
    th = np.array([0.0, 0.3])
    mg = CR.marginals(S, K, th, lb)
    c0, c1 = lb / 2, -lb / 2 * np.cos(0.3)  # theta == 0 takes the + branch
    np.testing.assert_allclose(mg[:, 0], [2 + 2 * c0 * 0.5 + c0 * c0 * 3, 2 + 2 * c1 * 0.5 + c1 * c1 * 3], rtol=1e-15)
    assert np.array_equal(mg[0, 1:5], [0.0, 16.0, 0.0, 0.0]) and not mg[1, 1:5].any()
    assert np.array_equal(mg[:, 5], [5.0, 5.0]) and np.array_equal(mg[:, 6], [7.0, 7.0]) and np.array_equal(mg[:, 7], [120.0] * 2)
    assert not CR.marginals(S, None, th, lb)[:, 1:5].any()


def test_wrapper_sigma0_forms_give_the_same_packed_array():
    from quadruped_landing_amd import nlp

    B = 3
    v = np.arange(1.0, 16.0)
    ref = CR.pack(np.diag(v))[None]
    for form in (v, np.diag(v), ref[0], ref):
        got, nb = nlp.tracking_sigma0(form, B)
        assert nb == 1 and got.dtype == np.float64 and got.flags.c_contiguous and np.array_equal(got, ref)
    rng = np.random.default_rng(1)
    M = CR.random_psd(rng, shape=(B,))
    got, nb = nlp.tracking_sigma0(M, B)
    assert nb == B and np.array_equal(got, CR.pack(M))
    got2, nb2 = nlp.tracking_sigma0(CR.pack(M), B)
    assert nb2 == B and np.array_equal(got2, got)
    for bad in (np.ones(14), np.ones((2, 15, 15)), np.ones((2, 120)), np.ones((15, 14))):
        with pytest.raises(ValueError):
            nlp.tracking_sigma0(bad, B)
    assert nlp.tracking_noise(None) is None
    assert np.array_equal(nlp.tracking_noise(2.0), np.full(15, 2.0))


def test_entry_points_reject_bad_arguments_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    z = np.zeros(100)
    s0 = np.zeros(120)
    out = np.zeros(240)
    w = np.zeros(15)
    bad = _lib.QLN_ERR_INVALID_ARGUMENT
    for fn in (L.qln_tracking_covariance, L.qln_tracking_covariance_host):
        # everything else in order: the null handle is what is refused
        assert fn(None, z.ctypes.data, None, s0.ctypes.data, 1, w.ctypes.data, out.ctypes.data, None) == bad
        assert b"null handle" in L.qln_last_error()
        assert fn(None, z.ctypes.data, None, s0.ctypes.data, 1, None, None, out.ctypes.data) == bad
        assert b"null handle" in L.qln_last_error()
        # both outputs NULL
        assert fn(None, z.ctypes.data, None, s0.ctypes.data, 1, w.ctypes.data, None, None) == bad
        assert b"both NULL" in L.qln_last_error()
        # negative, NaN and infinite process noise
        for i, v in ((3, -1e-9), (0, np.nan), (14, np.inf)):
            wb = w.copy()
            wb[i] = v
            assert fn(None, z.ctypes.data, None, s0.ctypes.data, 1, wb.ctypes.data, out.ctypes.data, None) == bad
            assert b"Wdiag" in L.qln_last_error() and f"entry {i}".encode() in L.qln_last_error()
        # a batch count that no B can match
        for nb in (0, -1):
            assert fn(None, z.ctypes.data, None, s0.ctypes.data, nb, w.ctypes.data, out.ctypes.data, None) == bad
            assert b"sigma0_batch" in L.qln_last_error()


def test_ctypes_table():
    from quadruped_landing_amd import _lib

    for name in ("qln_tracking_covariance", "qln_tracking_covariance_host"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == 8 and args[4] is C.c_int32
        assert getattr(_lib.lib(), name).argtypes == args
    assert _lib.TRACK_MARG_STRIDE == 8
