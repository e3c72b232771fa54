"""The yardstick of qln_landing_smoother held on the CPU (tests/landing_smoother_ref.py): the header's Bryson-Frazier recursion
against the classical Rauch-Tung-Striebel recursion and against the dense MAP solve of the whole linear-Gaussian problem, in
float64 and in longdouble; with a singular prior, where the classical recursion cannot run; and against 4 096 samples of the
linear model.  No device."""
import functools

import numpy as np
import pytest

from tests import landing_smoother_ref as SM
from tests import tracking_cov_ref as CR
from tests import tracking_kalman_ref as KR
from tests.estimation_cases import vec_rel

NX = 15
BAND = 5 * np.sqrt(2 / 4095)  # the family's band on a sample variance of 4 096 draws: five standard deviations, 0.1105


def linear_problem(seed, N, ny, dt=np.float64, singular=False, V=None):
    """A random linear-Gaussian problem with Sigma0 > 0 and W > 0: blocks near the identity, a measurement matrix, noise levels,
    a prior mean and one drawn record of measurements.  singular: the last slot is a noiseless clock -- row 14 of every A is
    e_14', Sigma0's row and column 14 and W[14] are zero."""
    rng = np.random.default_rng(seed)
    A = np.eye(NX) + 0.4 * rng.normal(size=(N - 1, NX, NX)) / np.sqrt(NX)
    H = rng.normal(size=(ny, NX)) / np.sqrt(NX)
    Vd = rng.uniform(0.5, 2.0, size=ny) if V is None else np.full(ny, V)
    S0 = CR.random_psd(rng) + 0.1 * np.eye(NX)
    W = rng.uniform(0.01, 0.1, size=NX)
    m0 = rng.normal(size=NX)
    if singular:
        A[:, 14, :] = 0.0
        A[:, 14, 14] = 1.0
        S0[14, :] = S0[:, 14] = 0.0
        W[14] = 0.0
    w, U = np.linalg.eigh(S0)
    x = m0 + U @ (np.sqrt(np.maximum(w, 0.0)) * rng.normal(size=NX))
    if singular:
        x[14] = m0[14]
    y = np.zeros((N, ny))
    for k in range(N):
        y[k] = H @ x + np.sqrt(Vd) * rng.normal(size=ny)
        if k < N - 1:
            x = A[k] @ x + np.sqrt(W) * rng.normal(size=NX)
    return tuple(a.astype(dt) for a in (A, H, Vd, S0, W, m0, y))


def smooth(A, H, V, S0, W, m0, y):
    """The filter (tracking_kalman_ref.recursion and its means), then the three smoothers' inputs."""
    f = KR.recursion(A, np.zeros(A.shape[:-1] + (4,), dtype=A.dtype), None, H, V, S0, W)
    Xhat, innov = SM.filter_means(A, f["L"], H, m0, y)
    return f, Xhat, innov


@functools.lru_cache(maxsize=None)
def _pair(seed, N, ny):
    """(Xs, Ps) of bryson_frazier and of rts, in float64 and in longdouble, on one problem"""
    out = {}
    for dt in (np.float64, np.longdouble):
        p = linear_problem(seed, N, ny, dt)
        f, Xhat, innov = smooth(*p)
        out[dt] = (p, SM.bryson_frazier(p[0], f["L"], f["Pp"], p[1], p[2], Xhat, innov),
                   SM.rts(p[0], f["L"], f["Pm"], f["Pp"], Xhat, innov))
    return out


# ---- 1. the header's recursion against the classical one, and against the dense solve -------------------------------------
@pytest.mark.parametrize("seed,N,ny", [(1, 9, 3), (2, 9, 8), (3, 17, 1), (4, 2, 8), (5, 33, 3)])
@pytest.mark.parametrize("dt", [np.float64, np.longdouble])
def test_bryson_frazier_is_the_classical_rts_recursion(seed, N, ny, dt):
    """Two recursions that share no algebra beyond the filter: one inverts P^-_{k+1}, the other inverts nothing."""
    _, (xb, pb), (xr, pr) = _pair(seed, N, ny)[dt]
    ex, ep = vec_rel(xb, xr), CR.knot_rel(pb, pr)
    lo, hi = _pair(seed, N, ny)[np.float64][1], _pair(seed, N, ny)[np.longdouble][1]
    print(f"smoother yardstick seed={seed} N={N} ny={ny} {np.dtype(dt).name}: Bryson-Frazier to RTS Xs {ex:.2e}, Ps {ep:.2e}; "
          f"float64 to longdouble Xs {vec_rel(lo[0], hi[0]):.2e}, Ps {CR.knot_rel(lo[1], hi[1]):.2e}")
    bar = 1e-11 if dt is np.float64 else 1e-14  # both are backward-stable sweeps of at most 33 well-conditioned knots
    assert ex <= bar and ep <= bar
    assert xb.dtype == dt and pb.dtype == dt


@pytest.mark.parametrize("seed,N,ny", [(11, 2, 3), (12, 3, 8), (13, 4, 1)])
@pytest.mark.parametrize("dt", [np.float64, np.longdouble])
def test_bryson_frazier_is_the_dense_map_solve(seed, N, ny, dt):
    """The smoothed means and covariances are the solution and the inverse's diagonal blocks of one 15 N x 15 N system."""
    p = linear_problem(seed, N, ny, dt)
    f, Xhat, innov = smooth(*p)
    xb, pb = SM.bryson_frazier(p[0], f["L"], f["Pp"], p[1], p[2], Xhat, innov)
    xs, ps = SM.stacked(*p)
    ex, ep = vec_rel(xb, xs), CR.knot_rel(pb, ps)
    print(f"smoother yardstick seed={seed} N={N} ny={ny} {np.dtype(dt).name}: Bryson-Frazier to the dense solve Xs {ex:.2e}, Ps {ep:.2e}")
    bar = 1e-10 if dt is np.float64 else 1e-13  # the dense system's condition number (1e3 .. 1e4 here) is in this one
    assert ex <= bar and ep <= bar


# ---- 2. a singular prior: a noiseless clock slot ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed,N,ny", [(21, 4, 3), (22, 3, 8)])
def test_a_noiseless_clock_slot_is_smoothed_where_the_classical_recursion_cannot_run(seed, N, ny):
    """Sigma0[14][14] = W[14] = 0: P^-_{k+1} is singular at every knot.  The dense solve runs with the slot eliminated -- it
    is the known constant m0[14], which moves into the other slots' offsets and the measurements."""
    A, H, V, S0, W, m0, y = p = linear_problem(seed, N, ny, singular=True)
    f, Xhat, innov = smooth(*p)
    assert not f["Pm"][:, 14, :].any()
    with np.errstate(all="ignore"):
        xr, pr = SM.rts(A, f["L"], f["Pm"], f["Pp"], Xhat, innov)
    assert not np.isfinite(pr[:-1]).all()  # the classical recursion divides by zero
    xb, pb = SM.bryson_frazier(A, f["L"], f["Pp"], H, V, Xhat, innov)
    c = A[:, :14, 14] * m0[14]
    xs, ps = SM.stacked(A[:, :14, :14], H[:, :14], V, S0[:14, :14], W[:14], m0[:14], y - H[:, 14] * m0[14], c)
    ex, ep = vec_rel(xb[:, :14], xs), CR.knot_rel(pb[:, :14, :14], ps)
    print(f"smoother yardstick singular seed={seed} N={N} ny={ny}: Bryson-Frazier to the reduced dense solve Xs {ex:.2e}, Ps {ep:.2e}")
    assert ex <= 1e-10 and ep <= 1e-10
    assert np.allclose(xb[:, 14], m0[14], rtol=0, atol=1e-14) and not pb[:, 14, :].any() and not pb[:, :, 14].any()


# ---- 3. sampled consistency --------------------------------------------------------------------------------------------------
def test_smoothed_errors_of_4096_samples_have_the_covariance_the_recursion_returns():
    """x - Xs over 4 096 draws of the linear model at N = 9: its sample variance along 32 directions per knot against d' Ps d,
    within five standard deviations of a sample variance, and smaller than the filter's at every knot but the last."""
    N, ny, S = 9, 3, 4096
    A, H, V, S0, W, m0, _ = linear_problem(31, N, ny)
    rng = np.random.default_rng(32)
    x = m0 + rng.normal(size=(S, NX)) @ np.linalg.cholesky(S0).T
    X, y = np.zeros((S, N, NX)), np.zeros((S, N, ny))
    for k in range(N):
        X[:, k] = x
        y[:, k] = x @ H.T + np.sqrt(V) * rng.normal(size=(S, ny))
        if k < N - 1:
            x = x @ A[k].T + np.sqrt(W) * rng.normal(size=(S, NX))
    f = KR.recursion(A, np.zeros((N - 1, NX, 4)), None, H, V, S0, W)
    Xhat, innov = SM.filter_means(A, f["L"], H, m0, y)
    Xs, Ps = SM.bryson_frazier(A, f["L"], f["Pp"], H, V, Xhat, innov)
    assert Xs.shape == (S, N, NX) and Ps.shape == (N, NX, NX)
    D = rng.normal(size=(N, 32, NX))
    err = np.einsum("skj,kdj->skd", X - Xs, D)
    ratio = (err ** 2).mean(axis=0) / np.einsum("kdi,kij,kdj->kd", D, Ps, D)
    print(f"smoother yardstick samples: variance ratio in [{ratio.min():.4f}, {ratio.max():.4f}], band {BAND:.4f}")
    assert np.abs(ratio - 1).max() <= BAND
    rs, rf = np.sqrt(((X - Xs) ** 2).mean(axis=(0, 2))), np.sqrt(((X - Xhat) ** 2).mean(axis=(0, 2)))
    assert (rs[:-1] < rf[:-1]).all() and rs[-1] == rf[-1]


# ---- 4. small V: the conditioning of H' V^-1 H C -----------------------------------------------------------------------------
def test_the_float64_yardstick_at_one_millimetre_measurement_noise():
    """V = 1e-6, the examples' 1 mm grade: H' V^-1 H (I - L H) is the difference of two terms 1 / V times its size.  The
    float64 recursion's distance to longdouble is measured and held to the cancellation's size, eps / V."""
    out = {}
    for dt in (np.float64, np.longdouble):
        p = linear_problem(41, 9, 8, dt, V=1e-6)
        f, Xhat, innov = smooth(*p)
        out[dt] = SM.bryson_frazier(p[0], f["L"], f["Pp"], p[1], p[2], Xhat, innov)
    ex, ep = vec_rel(out[np.float64][0], out[np.longdouble][0]), CR.knot_rel(out[np.float64][1], out[np.longdouble][1])
    print(f"smoother yardstick V=1e-6: float64 to longdouble Xs {ex:.2e}, Ps {ep:.2e}")
    assert max(ex, ep) <= 100 * np.finfo(np.float64).eps / 1e-6
