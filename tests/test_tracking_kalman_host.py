"""CPU checks of the Kalman / LQG layer (qln_tracking_kalman): the numpy yardstick against itself in extended precision,
against the 30 x 30 joint recursion that does not assume orthogonality, and against the Riccati sweep it is the dual of; the
exact no-measurement case; the wrapper's measurement_model; argument validation that needs no device; the ctypes table."""
import ctypes as C

import numpy as np
import pytest

from tests import rollout_ref as RR
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR
from tests import tracking_kalman_ref as KR
from tests import tracking_ref as TR
from tests.estimation_cases import measurement

CASES = [(40, 14, 1, 8), (61, 21, 2, 8), (40, 14, 1, 3), (12, 5, 2, 1), (2, 2, 1, 8)]  # (N, k_trans, init_mode, ny)


def _problem(N, k_trans, init_mode, ny):
    seed = 11 * N + k_trans + ny
    Zref, K, _, _ = TC.problem(N, k_trans, init_mode, seed)
    F = RR.complex_step_blocks(N, k_trans, init_mode, Zref)
    rng = np.random.default_rng(seed + 100)
    H, V = measurement(rng, ny)
    return F[:, :, :15], F[:, :, 15:19], K, H, V, CR.random_psd(rng), rng.uniform(0.0, 1e-2, size=15)


@pytest.mark.parametrize("N,k_trans,init_mode,ny", CASES)
def test_float64_against_longdouble(N, k_trans, init_mode, ny):
    """The yardstick's own rounding, to be set against the GPU tests' 1e-10 (where longdouble is no wider than float64 the
    comparison is trivially exact)."""
    A, B, K, H, V, S0, W = _problem(N, k_trans, init_mode, ny)
    ld = np.longdouble
    lo = KR.recursion(A, B, K, H, V, S0, W)
    hi = KR.recursion(A.astype(ld), B.astype(ld), K.astype(ld), H.astype(ld), V.astype(ld), S0.astype(ld), W.astype(ld))
    for name in ("L", "Pp", "X", "M"):
        e = CR.knot_rel(lo[name], hi[name])
        print(f"float64 vs longdouble, N={N} ny={ny}, {name}: {e:.2e}")
        assert e <= 1e-12, (name, e)
        if name != "L":
            assert np.array_equal(lo[name], np.swapaxes(lo[name], -1, -2))
    # the filter alone returns the same gains and error covariances
    f = KR.recursion(A, B, None, H, V, S0, W)
    assert np.array_equal(f["L"], lo["L"]) and np.array_equal(f["Pp"], lo["Pp"]) and "X" not in f


@pytest.mark.parametrize("N,k_trans,init_mode,ny", CASES)
def test_x_equals_the_joint_recursion(N, k_trans, init_mode, ny):
    """X_k = M_k + P^+_k rests on the orthogonality of estimate and error; the joint covariance of (x, xhat^-) does not."""
    A, B, K, H, V, S0, W = _problem(N, k_trans, init_mode, ny)
    r = KR.recursion(A, B, K, H, V, S0, W)
    Xj = KR.joint(A, B, K, H, V, S0, r["L"], W)
    e = CR.knot_rel(r["X"], Xj)
    print(f"X against the joint recursion, N={N} ny={ny}: {e:.2e}")
    assert e <= 1e-12, e


@pytest.mark.parametrize("N,k_trans,init_mode", [(40, 14, 1), (12, 5, 2)])
def test_duality_with_the_riccati_sweep(N, k_trans, init_mode):
    """The filter's priors are the cost-to-go of the dual problem: tracking_ref.riccati on A_{N-2-k}', H', Q = W, R = V,
    Qf = diag Sigma0 returns P^-_k in reverse order (its P_k = Q + A'PA - ... with the measurement update inside)."""
    ny = 4
    A, B, K, H, V, _, W = _problem(N, k_trans, init_mode, ny)
    s0 = np.random.default_rng(N).uniform(0.5, 2.0, size=15)
    r = KR.recursion(A, B, None, H, V, np.diag(s0), W)
    Ad = np.swapaxes(A[::-1], -1, -2)
    Bd = np.broadcast_to(H.T, (N - 1, 15, ny))
    # riccati's recursion P_k = Q + A'(P - P B (R + B'PB)^-1 B'P) A from P_{N-1} = Qf: with A -> A', B -> H' that is
    # P^-_{k+1} = W + A (P^- - P^- H' S^-1 H P^-) A'
    _, Pd = TR.riccati(Ad, Bd, W, V, s0)
    e = CR.knot_rel(r["Pm"], Pd[::-1])
    print(f"priors against the dual Riccati sweep, N={N}: {e:.2e}")
    assert e <= 1e-12, e


def test_without_measurements_the_filter_is_the_open_loop_covariance():
    """H = 0, V = 1: no gain, no estimate, and P^+ is tracking_cov_ref.propagate(K=None), all exactly."""
    N, k_trans, init_mode = 40, 14, 1
    A, B, K, _, _, S0, W = _problem(N, k_trans, init_mode, 8)
    r = KR.recursion(A, B, K, np.zeros((8, 15)), np.ones(8), S0, W)
    assert not r["L"].any() and not r["M"].any()
    ref = CR.propagate(A, B, None, S0, W)
    assert np.array_equal(r["Pp"], ref) and np.array_equal(r["X"], ref) and np.array_equal(r["Pm"], ref)


def test_ldl_solve_against_numpy():
    rng = np.random.default_rng(3)
    for n in (1, 3, 8):
        G = rng.normal(size=(5, n, n))
        q = G @ np.swapaxes(G, -1, -2) + n * np.eye(n)
        rhs = rng.normal(size=(5, n, 4))
        np.testing.assert_allclose(KR.ldl_solve(q, rhs), np.linalg.solve(q, rhs), rtol=1e-12, atol=1e-14)


def test_measurement_model_checks_shapes_and_values():
    from quadruped_landing_amd import nlp

    rng = np.random.default_rng(0)
    H, V = nlp.measurement_model(rng.normal(size=(3, 15)), [1.0, 2.0, 0.5])
    assert H.shape == (3, 15) and V.shape == (3,) and H.flags.c_contiguous and H.dtype == np.float64
    H, V = nlp.measurement_model(np.ones(15), 2.0)
    assert H.shape == (1, 15) and np.array_equal(V, [2.0])
    H, V = nlp.measurement_model(np.ones((8, 15)), 0.1)
    assert np.array_equal(V, np.full(8, 0.1))
    bad_h = np.ones((2, 15))
    bad_h[1, 3] = np.inf
    for h, v in ((np.ones((9, 15)), 1.0), (np.ones((0, 15)), 1.0), (np.ones((2, 14)), 1.0), (np.ones((2, 15)), [1.0]),
                 (np.ones((2, 15)), [1.0, 0.0]), (np.ones((2, 15)), [1.0, -1.0]), (np.ones((2, 15)), [np.nan, 1.0]),
                 (np.ones((2, 15)), [np.inf, 1.0]), (bad_h, 1.0), (np.ones((2, 15)), np.ones((2, 2)))):
        with pytest.raises(ValueError):
            nlp.measurement_model(h, v)
    assert nlp.tracking_l_shape(3, 5, 2) == (3, 5, 15, 2)


def _calls(L):
    """(name, call(h, K, H, ny, V, s0, nb, W, Lg, Pe, S, mg)) for the four entry points, the guarded ones with an event"""
    z, ev = np.zeros(100), np.zeros(8)

    def plain(fn):
        return lambda K, H, ny, V, s0, nb, W, Lg, Pe, S, mg: fn(None, z.ctypes.data, K, H, ny, V, s0, nb, W, Lg, Pe, S, mg)

    def guarded(fn):
        return lambda K, H, ny, V, s0, nb, W, Lg, Pe, S, mg, event=ev.ctypes.data, var=None: fn(
            None, z.ctypes.data, K, None, event, H, ny, V, s0, nb, W, Lg, Pe, S, mg, var)

    return [("plain", plain(L.qln_tracking_kalman)), ("plain", plain(L.qln_tracking_kalman_host)),
            ("guarded", guarded(L.qln_tracking_kalman_guarded)), ("guarded", guarded(L.qln_tracking_kalman_guarded_host))]


def test_entry_points_reject_bad_arguments_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    bad = _lib.QLN_ERR_INVALID_ARGUMENT
    Hm, V, s0, w, k = np.zeros((8, 15)), np.ones(8), np.zeros(120), np.zeros(15), np.zeros(60)
    out = np.zeros(1000)
    p = lambda a: a.ctypes.data  # noqa: E731
    for kind, call in _calls(L):
        # everything in order: the null handle is what is refused
        assert call(p(k), p(Hm), 8, p(V), p(s0), 1, p(w), p(out), None, None, None) == bad
        assert b"null handle" in L.qln_last_error()
        assert call(None, p(Hm), 1, p(V), p(s0), 1, None, None, p(out), None, None) == bad
        assert b"null handle" in L.qln_last_error()
        for ny in (0, 9, -1):
            assert call(p(k), p(Hm), ny, p(V), p(s0), 1, p(w), p(out), None, None, None) == bad
            assert b"ny must be" in L.qln_last_error()
        assert call(p(k), p(Hm), 8, p(V), p(s0), 1, p(w), None, None, None, None) == bad
        assert b"nothing to compute" in L.qln_last_error()
        # Sigma and marg need the gains
        assert call(None, p(Hm), 8, p(V), p(s0), 1, p(w), p(out), None, p(out[500:]), None) == bad
        assert b"need K" in L.qln_last_error()
        assert call(None, p(Hm), 8, p(V), p(s0), 1, p(w), p(out), None, None, p(out[500:])) == bad
        assert b"need K" in L.qln_last_error()
        assert call(p(k), None, 8, p(V), p(s0), 1, p(w), p(out), None, None, None) == bad
        assert b"null H" in L.qln_last_error()
        for i, v in ((2, 0.0), (0, -1.0), (7, np.nan), (5, np.inf)):
            vb = V.copy()
            vb[i] = v
            assert call(p(k), p(Hm), 8, p(vb), p(s0), 1, p(w), p(out), None, None, None) == bad
            assert b"Vdiag" in L.qln_last_error() and f"entry {i}".encode() in L.qln_last_error()
        vb = V.copy()
        vb[5] = np.nan  # behind ny: not read
        assert call(p(k), p(Hm), 5, p(vb), p(s0), 1, p(w), p(out), None, None, None) == bad
        assert b"null handle" in L.qln_last_error()
        for i, v in ((3, -1e-9), (0, np.nan), (14, np.inf)):
            wb = w.copy()
            wb[i] = v
            assert call(p(k), p(Hm), 8, p(V), p(s0), 1, p(wb), p(out), None, None, None) == bad
            assert b"Wdiag" in L.qln_last_error() and f"entry {i}".encode() in L.qln_last_error()
        for nb in (0, -1):
            assert call(p(k), p(Hm), 8, p(V), p(s0), nb, p(w), p(out), None, None, None) == bad
            assert b"sigma0_batch" in L.qln_last_error()
        if kind == "guarded":
            assert call(p(k), p(Hm), 8, p(V), p(s0), 1, p(w), p(out), None, None, None, event=None) == bad
            assert b"null event" in L.qln_last_error()
            assert call(None, p(Hm), 8, p(V), p(s0), 1, p(w), p(out), None, None, None, var=p(out[500:])) == bad
            assert b"need K" in L.qln_last_error()


def test_ctypes_table():
    from quadruped_landing_amd import _lib

    for name, n in (("qln_tracking_kalman", 13), ("qln_tracking_kalman_host", 13), ("qln_tracking_kalman_guarded", 16),
                    ("qln_tracking_kalman_guarded_host", 16)):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n
        assert [i for i, a in enumerate(args) if a is C.c_int32] == ([4, 7] if n == 13 else [6, 9])
        assert getattr(_lib.lib(), name).argtypes == args
    assert _lib.TRACK_NY_MAX == 8
