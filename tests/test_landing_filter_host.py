"""The yardstick of qln_landing_filter held on the CPU (tests/landing_filter_ref.py): its replay of the flight yardstick's record
returns that flight's Xhat and innov; its log-likelihood is the dense Gaussian log-density of the stacked measurements of the
linear model, also with a noiseless clock slot; and over 4 096 draws of the linear model the mean of the normalised innovation
squared is ny at every knot.  No device."""
import functools

import numpy as np
import pytest

from tests import landing_filter_ref as FR
from tests import rollout_estimated_cases as EC
from tests import rollout_estimated_ref as ER
from tests import rollout_guarded_cases as GC
from tests import rollout_ref as RR
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR
from tests import tracking_kalman_ref as KR

NX = 15
LD = np.longdouble


# ---- 1. the replay of a flight --------------------------------------------------------------------------------------------
def _flight_inputs(N, guarded):
    B = 12
    if guarded:
        batch, Zref, K, x0, th = GC.case(N, 1, B, True, True)
        kt, im = None, 1
    else:
        kt, im = (3, 2) if N == 5 else (6, 1)
        batch = TC.batch(B, N, kt, im, seed=N + kt)
        rng = np.random.default_rng(N)
        Zref = np.ascontiguousarray(batch.Z, dtype=np.float64)
        x0 = Zref[:, :15] + 1e-2 * rng.normal(size=(B, 15))
        K = 0.05 * rng.normal(size=(B, N - 1, 4, 15))
        th = RR.draw_models(B, N, TC.SECOND)
    d = EC.draws(N + 1, B, N, 3)
    return B, kt, im, Zref, K, x0, th, d


@functools.lru_cache(maxsize=None)
def _replayed(N, guarded, dt):
    """(the flight yardstick's record, the filter yardstick's replay of it) in one dtype"""
    B, kt, im, Zref, K, x0, th, d = _flight_inputs(N, guarded)
    xhat0 = Zref[:, :15] + d["dxhat0"]
    fl = ER.rollout(N, im, Zref, K, d["Lgain"], d["H"], x0, th, TC.SECOND, d["vnoise"], d["wnoise"], xhat0, kt, guarded, dtype=dt)
    cast = lambda a: np.asarray(a).astype(dt)  # noqa: E731
    Y = FR.measurements(fl["Zout"], cast(Zref), cast(d["H"]), cast(d["vnoise"]))
    assert Y.dtype == dt
    rp = FR.replay(N, im, Zref, fl["Zout"], d["Lgain"], d["H"], Y, TC.SECOND, np.full(3, 1e-6), xhat0, kt, guarded, dtype=dt)
    return fl, rp


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N", [5, 17])
def test_the_replay_of_the_flight_yardsticks_record_is_that_flights_estimate(N, guarded):
    """Y recomputed from the flight's Zout and vnoise, the controls read from Zout.  The bar is 100 x the float64 replay's own
    distance to its longdouble run (RR.rel), measured here and written down in DESIGN.md 4.26."""
    fl, rp = _replayed(N, guarded, np.float64)
    flh, rph = _replayed(N, guarded, LD)
    keep = slice(None)
    if guarded:
        keep = np.minimum(fl["margin_hat"], fl["margin"]) >= GC.MARGIN
        assert keep.mean() >= 1 - GC.LEFT_OUT and (fl["events_hat"][:, 0] >= 0).any()
        assert np.allclose(rp["margin_hat"], fl["margin_hat"], rtol=1e-9, atol=0)  # the same estimator, the same guard
    own = max(RR.rel(rp[n][keep], rph[n][keep].astype(np.float64)) for n in ("Xhat", "innov"))
    dist = {n: RR.rel(rp[n][keep], fl[n][keep]) for n in ("Xhat", "innov") + (("events_hat",) if guarded else ())}
    print(f"filter yardstick replay N={N} guarded={guarded}: to the flight's record " + ", ".join(f"{n} {e:.2e}" for n, e in dist.items()) +
          f"; float64 to longdouble {own:.2e}, bar {100 * own:.2e}")
    assert own > 0 and all(e <= 100 * own for e in dist.values())
    assert rp["Xhat"].dtype == np.float64 and rph["Xhat"].dtype == LD and rph["loglik"].dtype == LD
    assert np.isfinite(rp["score"][keep][..., 0]).all()


# ---- 2. the log-likelihood against the dense Gaussian density ------------------------------------------------------------
def linear_problem(seed, N, ny, V, singular=False, S=None, prior=1.0):
    """A random linear-Gaussian problem: blocks near the identity, H, V, Sigma0 > 0 and W > 0 (both scaled by prior), a prior
    mean and drawn records of measurements (one, or S).  singular: slot 14 is a noiseless clock -- row 14 of every A is e_14',
    Sigma0's row and column 14 and W[14] are zero."""
    rng = np.random.default_rng(seed)
    A = np.eye(NX) + 0.4 * rng.normal(size=(N - 1, NX, NX)) / np.sqrt(NX)
    H = rng.normal(size=(ny, NX)) / np.sqrt(NX)
    Vd = np.full(ny, V) * rng.uniform(0.5, 2.0, size=ny)
    S0 = prior * (CR.random_psd(rng) + 0.1 * np.eye(NX))
    W = prior * rng.uniform(0.01, 0.1, size=NX)
    m0 = rng.normal(size=NX)
    if singular:
        A[:, 14, :] = 0.0
        A[:, 14, 14] = 1.0
        S0[14, :] = S0[:, 14] = 0.0
        W[14] = 0.0
    w, U = np.linalg.eigh(S0)
    lead = () if S is None else (S,)
    x = m0 + (np.sqrt(np.maximum(w, 0.0)) * rng.normal(size=lead + (NX,))) @ U.T
    y = np.zeros(lead + (N, ny))
    for k in range(N):
        y[..., k, :] = x @ H.T + np.sqrt(Vd) * rng.normal(size=lead + (ny,))
        if k < N - 1:
            x = x @ A[k].T + np.sqrt(W) * rng.normal(size=lead + (NX,))
    return A, H, Vd, S0, W, m0, y


def dense_logpdf(A, H, V, S0, W, m0, y):
    """The log-density of the stacked N ny measurements of one record under the joint Gaussian of the linear model, in the
    arrays' dtype: the mean H Phi_k m0, the covariance H Cov(x_j, x_k) H' + [j == k] diag(V) assembled from the blocks, and a
    Cholesky factorisation written out (numpy's does not take longdouble)."""
    dt = A.dtype.type
    N, ny = y.shape
    P = [S0]
    mean = [m0]
    for k in range(N - 1):
        P.append(A[k] @ P[k] @ A[k].T + np.diag(W))
        mean.append(A[k] @ mean[k])
    C = np.zeros((N * ny, N * ny), dtype=A.dtype)
    for j in range(N):
        X = P[j]                                   # Cov(x_j, x_k) = P_j (A_{k-1} .. A_j)' for k >= j
        for k in range(j, N):
            if k > j:
                X = X @ A[k - 1].T
            blk = H @ X @ H.T
            C[j * ny:(j + 1) * ny, k * ny:(k + 1) * ny] = blk
            C[k * ny:(k + 1) * ny, j * ny:(j + 1) * ny] = blk.T
        C[j * ny:(j + 1) * ny, j * ny:(j + 1) * ny] += np.diag(V)
    r = (y - np.stack(mean) @ H.T).reshape(-1)
    n = N * ny
    Lc = np.zeros_like(C)
    for i in range(n):
        for j in range(i + 1):
            s = C[i, j] - Lc[i, :j] @ Lc[j, :j]
            Lc[i, j] = np.sqrt(s) if i == j else s / Lc[j, j]
    z = np.zeros(n, dtype=A.dtype)
    for i in range(n):
        z[i] = (r[i] - Lc[i, :i] @ z[:i]) / Lc[i, i]
    return dt(-0.5) * (z @ z + dt(2) * np.log(np.diagonal(Lc)).sum() + dt(n) * np.log(dt(8) * np.arctan(dt(1))))


@pytest.mark.parametrize("singular", [False, True])
@pytest.mark.parametrize("seed,N,ny,V", [(1, 4, 8, 1e-6), (2, 4, 3, 1e-6), (3, 3, 1, 1e-6), (4, 2, 8, 1e-4), (5, 4, 8, 1.0), (6, 4, 1, 1e-2),
                                         (7, 3, 3, 1.0)])
def test_the_log_likelihood_is_the_dense_gaussian_log_density(seed, N, ny, V, singular):
    """loglik from the gains alone -- S^-1 = V^-1 (I - H L), no P^-, no Sigma0, no W -- against the density of the stacked
    measurement vector, which is assembled from Sigma0, W and the blocks and shares nothing with it but the problem.  The
    dense density runs in longdouble; the float64 yardstick is held to it within 1e-10 of max(1, |ref|), and with Sigma0[14][14]
    = W[14] = 0, the examples' clock slot.
    I - H L = V S^-1 is formed by a subtraction from one, which loses |H P^- H'| / V digits: the prior and the process noise are
    scaled to at most 100 V (the family's experiments have |H P^- H'| <= V: Sigma0 ~ 1e-8 against V from 1e-8 to 1e-4), so the
    loss is eps 1e2 ~ 2e-14 an entry.  With a prior of order one against V = 1e-6 the float64 yardstick is 1e-10 .. 1e-9 from the
    density, its longdouble run 1e-13: the identity's conditioning, not the recursion's."""
    A, H, Vd, S0, W, m0, y = linear_problem(seed, N, ny, V, singular, prior=min(1.0, 100 * V))
    L = KR.recursion(A, np.zeros((N - 1, NX, 4)), None, H, Vd, S0, W)["L"]
    _, _, sc, ll = FR.linear(A, L, H, Vd, m0, y)
    ref = dense_logpdf(*(a.astype(LD) for a in (A, H, Vd, S0, W, m0, y)))
    hi = KR.recursion(*(a.astype(LD) for a in (A, np.zeros((N - 1, NX, 4)))), None, *(a.astype(LD) for a in (H, Vd, S0, W)))["L"]
    _, _, _, llh = FR.linear(*(a.astype(LD) for a in (A, hi, H, Vd, m0, y)))
    e64, eld = float(abs(ll - ref) / max(1, abs(ref))), float(abs(llh - ref) / max(1, abs(ref)))
    print(f"filter yardstick loglik seed={seed} N={N} ny={ny} V={V:.0e} singular={singular}: loglik {float(ll):.6f}, to the dense density "
          f"float64 {e64:.2e}, longdouble {eld:.2e}")
    assert e64 <= 1e-10 and eld <= 1e-13
    assert sc.shape == (N, 2) and np.isfinite(sc).all()


# ---- 3. the mean of the score ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,V", [(8, 1e-6), (3, 1e-2), (1, 1.0)])
def test_the_normalised_innovation_squared_of_4096_draws_has_mean_ny_at_every_knot(ny, V):
    """nis_k ~ chi^2(ny) under the model the filter was designed for: the mean over S draws has relative standard deviation
    sqrt(2 / (ny S)), inside the family's band of five sqrt(2 / (S - 1)) for every ny."""
    N, S = 9, EC.MC_S
    A, H, Vd, S0, W, m0, y = linear_problem(31 + ny, N, ny, V, S=S)
    L = KR.recursion(A, np.zeros((N - 1, NX, 4)), None, H, Vd, S0, W)["L"]
    _, _, sc, ll = FR.linear(A, L, H, Vd, m0, y)
    assert sc.shape == (S, N, 2) and ll.shape == (S,)
    mean = sc[..., 0].mean(axis=0)
    print(f"filter yardstick samples ny={ny} V={V:.0e}: mean nis / ny per knot " + " ".join(f"{m / ny:.4f}" for m in mean) +
          f"; band {EC.band():.4f}")
    assert np.abs(mean / ny - 1).max() <= EC.band()
    assert np.array_equal(sc[..., 1], np.broadcast_to(sc[:1, :, 1], (S, N)))  # log det S_k does not depend on the record
