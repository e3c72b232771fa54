"""numpy yardstick of qln_kalman_design_jvp / _guarded_jvp (include/qln_evaluator.h): the forward sweep through the design of the
Kalman filter -- how the gains, the error covariances and log det S_k of tracking_kalman_ref.recursion move along a direction
(Sigma0_dot, W_dot, V_dot), at the gains that recursion returned.  Not a test module.  The header's recursion, batched, in the
dtype of the blocks it is given (float64, or longdouble to measure its own rounding).

design_quotient() is what holds it: central differences of tracking_kalman_ref.recursion itself, with the sum of the log
pivots of S_k as the differentiated log det.  composite() restates HybridNLP.landing_loglik_jvp."""
import numpy as np

from tests import tracking_cov_ref as CR
from tests import tracking_kalman_ref as KR

NX = CR.NX
_t = KR._t


def sinv(L, H, V):
    """diag(1/V) (I - H L), the full matrix as the header states it (symmetric for optimal gains, up to rounding)"""
    ny = H.shape[0]
    return (np.eye(ny, dtype=L.dtype) - H @ L) / V[:, None]


def sweep(A, H, V, Lgain, Sigma0_dot=None, W_dot=None, V_dot=None):
    """A (..., N-1, 15, 15) the open-loop blocks, H (ny, 15), V (ny,), Lgain (..., N, 15, ny); the direction: Sigma0_dot
    (..., 15, 15) or (15, 15), W_dot (15,), V_dot (ny,), None for zero.  Returns dict(Ld (..., N, 15, ny), Pd (..., N, 15, 15) =
    the tangent of P^+, Pdm = that of P^-, logdet (..., N))."""
    A = np.asarray(A)
    dt = A.dtype
    H, V, L = (np.asarray(a, dtype=dt) for a in (H, V, Lgain))
    lead, n1 = A.shape[:-3], A.shape[-3]
    N, ny = n1 + 1, H.shape[0]
    Wd = np.zeros((NX, NX), dtype=dt) if W_dot is None else np.diag(np.asarray(W_dot, dtype=dt))
    Vd = np.zeros(ny, dtype=dt) if V_dot is None else np.asarray(V_dot, dtype=dt)
    S0d = np.zeros((NX, NX), dtype=dt) if Sigma0_dot is None else np.asarray(Sigma0_dot, dtype=dt)
    Pd = np.broadcast_to(KR.sym(S0d), lead + (NX, NX))
    out = dict(Ld=np.zeros(lead + (N, NX, ny), dtype=dt), Pd=np.zeros(lead + (N, NX, NX), dtype=dt),
               Pdm=np.zeros(lead + (N, NX, NX), dtype=dt), logdet=np.zeros(lead + (N,), dtype=dt))
    I = np.eye(NX, dtype=dt)
    for k in range(N):
        Lk = L[..., k, :, :]
        Gd = H @ Pd
        Sd = Gd @ H.T + np.diag(Vd)
        Sd = np.tril(Sd) + _t(np.tril(Sd, -1))
        Si = sinv(Lk, H, V)
        out["Ld"][..., k, :, :] = (Pd @ H.T - Lk @ Sd) @ Si
        out["logdet"][..., k] = (Si * Sd).sum(axis=(-1, -2))
        IL = I - Lk @ H
        Pp = KR.sym(IL @ Pd @ _t(IL) + (Lk * Vd) @ _t(Lk))
        out["Pdm"][..., k, :, :], out["Pd"][..., k, :, :] = Pd, Pp
        if k < n1:
            a = A[..., k, :, :]
            Pd = KR.sym(a @ Pp @ _t(a) + Wd)
    return out


def log_pivots(S):
    """sum of the logs of the pivots of S (..., n, n) = log det S, by L D L' without pivoting, any real dtype"""
    n = S.shape[-1]
    Lf = np.zeros_like(S)
    d = np.zeros(S.shape[:-1], dtype=S.dtype)
    for c in range(n):
        d[..., c] = S[..., c, c] - sum(Lf[..., c, m] * Lf[..., c, m] * d[..., m] for m in range(c))
        for r in range(c + 1, n):
            Lf[..., r, c] = (S[..., r, c] - sum(Lf[..., r, m] * Lf[..., c, m] * d[..., m] for m in range(c))) / d[..., c]
    return np.log(d).sum(axis=-1)


def design(A, H, V, Sigma0, W, dtype):
    """tracking_kalman_ref.recursion's filter alone in dtype: dict(L, Pp, logdet) with logdet (..., N) the log pivots of S_k"""
    dt = np.dtype(dtype).type
    A, H, V, Sigma0, W = (np.asarray(a).astype(dt) for a in (A, H, V, Sigma0, W))
    r = KR.recursion(A, np.zeros(A.shape[:-1] + (4,), dtype=dt), None, H, V, Sigma0, W)
    S = H @ r["Pm"] @ H.T + np.diag(V)
    return dict(L=r["L"], Pp=r["Pp"], logdet=log_pivots(S))


def design_quotient(A, H, V, Sigma0, W, Sigma0_dot, W_dot, V_dot, t, dtype=np.longdouble):
    """Central differences of design() along the direction at step t, in dtype: dict(Ld, Pd, logdet)"""
    dt = np.dtype(dtype).type
    z = lambda a, like: np.zeros(np.shape(like), dtype=dt) if a is None else np.asarray(a).astype(dt)  # noqa: E731
    S0d, Wd, Vd = z(Sigma0_dot, Sigma0), z(W_dot, W), z(V_dot, V)
    at = lambda s: design(A, H, np.asarray(V).astype(dt) + dt(s) * Vd, np.asarray(Sigma0).astype(dt) + dt(s) * S0d,  # noqa: E731
                          np.asarray(W).astype(dt) + dt(s) * Wd, dt)
    p, m = at(t), at(-t)
    return {o: (p[i] - m[i]) / (2 * dt(t)) for o, i in (("Ld", "L"), ("Pd", "Pp"), ("logdet", "logdet"))}


def errors(got, ref):
    """(Ld, Pd in knot_rel, logdet in entry_rel) of two dicts of sweep()'s"""
    return (CR.knot_rel(got["Ld"], ref["Ld"]), CR.knot_rel(got["Pd"], ref["Pd"]), CR.entry_rel(got["logdet"], ref["logdet"]))


def directions(seed, ny, lead=()):
    """A random direction: a symmetric indefinite Sigma0_dot (lead + (15, 15)), signed W_dot (15,) and V_dot (ny,)"""
    rng = np.random.default_rng(seed)
    G = rng.normal(size=lead + (NX, NX)) / np.sqrt(NX)
    return G + _t(G), rng.normal(size=NX) * 1e-2, rng.normal(size=ny)


def composite(innov, innov_dot, Lgain, Lgain_dot, H, V, V_dot, logdet_dot):
    """HybridNLP.landing_loglik_jvp's third step in numpy: (loglik_dot (B,), nis_dot (B, N)) from the filter's innovations and
    their tangent under Lgain_dot, with the full matrix diag(1/V) (I - H L) as the filter's nis has it."""
    dt = innov.dtype
    H, V, L, Ld = (np.asarray(a, dtype=dt) for a in (H, V, Lgain, Lgain_dot))
    ny = H.shape[0]
    Vd = np.zeros(ny, dtype=dt) if V_dot is None else np.asarray(V_dot, dtype=dt)
    G = np.eye(ny, dtype=dt) - H @ L
    Si = G / V[:, None]
    Sid = -(Vd / (V * V))[:, None] * G - (H @ Ld) / V[:, None]
    q = lambda x, M, y: np.einsum("bkr,bkrs,bks->bk", x, M, y)  # noqa: E731
    nis_dot = q(innov, Si, innov_dot) + q(innov_dot, Si, innov) + q(innov, Sid, innov)
    return dt.type(-0.5) * (nis_dot + logdet_dot).sum(axis=1), nis_dot
