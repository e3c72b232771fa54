"""numpy yardstick of qln_noise_design_vjp / _guarded_vjp (include/qln_evaluator.h): the reverse sweep through the design of the
Kalman filter, the transpose of tracking_kalman_sweep_ref.sweep's linear map between the arrays as stored -- cotangents (Lgain_bar
(..., N, 15, ny), Pest_bar (..., N, 120) packed, logdet_bar (..., N)) in, (Sigma0_bar (..., 120) packed, Wdiag_bar (..., 15),
Vdiag_bar (..., ny)) per problem out.  Not a test module.  The header's recursion, batched, in the dtype of the blocks it is given
(float64, or longdouble to measure its own rounding).

dense_forward() is what holds it: the matrix of the forward yardstick's map, column by column.  loglik_grad() restates
HybridNLP.landing_loglik_grad."""
import numpy as np

from tests import tracking_cov_ref as CR
from tests import tracking_kalman_ref as KR
from tests import tracking_kalman_sweep_ref as KS

NX, NNZ = CR.NX, CR.NNZ
_t = KR._t
OUT = ("Sigma0", "W", "V")


def half(X):
    """(X + X') / 2"""
    return (X + _t(X)) / X.dtype.type(2)


def sym_cotangent(Pb):
    """(..., 120) packed -> (..., 15, 15): the full symmetric cotangent, a packed off-diagonal entry at half on each side"""
    F = CR.unpack(Pb)
    d = np.arange(NX)
    F = F / F.dtype.type(2)
    F[..., d, d] = F[..., d, d] * F.dtype.type(2)
    return F


def pack_cotangent(Lam):
    """(..., 15, 15) -> (..., 120): Lambda(i, j) + Lambda(j, i) off the diagonal, Lambda(i, i) on it"""
    r, c = np.tril_indices(NX)
    return np.where(r == c, Lam[..., r, c], Lam[..., r, c] + Lam[..., c, r])


def sweep(A, H, V, Lgain, Lgain_bar=None, Pest_bar=None, logdet_bar=None):
    """A (..., N-1, 15, 15) the open-loop blocks, H (ny, 15), V (ny,), Lgain (..., N, 15, ny); the cotangents, None for zero.
    Returns dict(Sigma0 (..., 120), W (..., 15), V (..., ny))."""
    A = np.asarray(A)
    dt = A.dtype
    H, V, L = (np.asarray(a, dtype=dt) for a in (H, V, Lgain))
    lead, n1 = A.shape[:-3], A.shape[-3]
    N, ny = n1 + 1, H.shape[0]
    Lb = np.zeros(lead + (N, NX, ny), dtype=dt) if Lgain_bar is None else np.asarray(Lgain_bar, dtype=dt)
    Pb = np.zeros(lead + (N, NNZ), dtype=dt) if Pest_bar is None else np.asarray(Pest_bar, dtype=dt)
    lb = np.zeros(lead + (N,), dtype=dt) if logdet_bar is None else np.asarray(logdet_bar, dtype=dt)
    Wb, Vb = np.zeros(lead + (NX,), dtype=dt), np.zeros(lead + (ny,), dtype=dt)
    Lam = np.zeros(lead + (NX, NX), dtype=dt)
    I = np.eye(NX, dtype=dt)
    diag = lambda X: np.diagonal(X, axis1=-2, axis2=-1)  # noqa: E731
    for k in range(N - 1, -1, -1):
        Lk = L[..., k, :, :]
        Pi = sym_cotangent(Pb[..., k, :])
        if k < n1:
            a = A[..., k, :, :]
            Wb = Wb + diag(Lam)
            Pi = _t(a) @ Lam @ a + Pi
        Vb = Vb + diag(_t(Lk) @ Pi @ Lk)
        Si = KS.sinv(Lk, H, V)
        Tb = Lb[..., k, :, :] @ _t(Si)
        Sb = -_t(Lk) @ Tb + lb[..., k, None, None] * Si
        Vb = Vb + diag(Sb)
        C = I - Lk @ H
        Lam = _t(C) @ Pi @ C + H.T @ half(Sb) @ H + half(Tb @ H)
    return dict(Sigma0=pack_cotangent(Lam), W=Wb, V=Vb)


def dense_forward(A, H, V, Lgain):
    """One problem's forward map as a matrix: A (N-1, 15, 15), Lgain (N, 15, ny).  Rows: Lgain_dot (N 15 ny), Pest_dot (N 120),
    logdet_dot (N), flattened in that order; columns: Sigma0_dot (120), W_dot (15), V_dot (ny).  Column by column through
    tracking_kalman_sweep_ref.sweep, in A's dtype."""
    dt = A.dtype
    ny = H.shape[0]
    cols = []
    for p in range(NNZ + NX + ny):
        e = np.zeros(NNZ + NX + ny, dtype=dt)
        e[p] = 1
        s = KS.sweep(A, H, V, Lgain, CR.unpack(e[:NNZ]), e[NNZ:NNZ + NX], e[NNZ + NX:])
        cols.append(np.concatenate([s["Ld"].reshape(-1), CR.pack(s["Pd"]).reshape(-1), s["logdet"].reshape(-1)]))
    return np.stack(cols, axis=1)


def cotangents(seed, N, ny, lead=()):
    """Signed cotangents, every entry drawn independently: (Lgain_bar, Pest_bar, logdet_bar)"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=lead + (N, NX, ny)), rng.normal(size=lead + (N, NNZ)), rng.normal(size=lead + (N,))


def inner(cot, fwd, rev, dirs):
    """(<cotangents, forward outputs>, <reverse outputs, direction>) per problem; fwd: tracking_kalman_sweep_ref.sweep's dict,
    dirs: (Sigma0_dot (..., 15, 15), W_dot (15,), V_dot (ny,))"""
    Lb, Pb, lb = cot
    S0d, Wd, Vd = dirs
    lhs = (Lb * fwd["Ld"]).sum(axis=(-1, -2, -3)) + (Pb * CR.pack(fwd["Pd"])).sum(axis=(-1, -2)) + (lb * fwd["logdet"]).sum(axis=-1)
    rhs = (rev["Sigma0"] * CR.pack(S0d)).sum(axis=-1) + (rev["W"] * Wd).sum(axis=-1) + (rev["V"] * Vd).sum(axis=-1)
    return lhs, rhs


def out_rel(got, ref, floor=1e-13):
    """The worst entry's distance relative to max(the output's largest entry, over the batch) -- and that scale times floor, which
    the callers use as the least distance a ratio is taken with"""
    got, ref = np.asarray(got).astype(np.longdouble), np.asarray(ref).astype(np.longdouble)
    scale = float(np.max(np.abs(ref)))
    return float(np.max(np.abs(got - ref))) / max(scale, 1e-300), floor


def loglik_grad(A, F, Lgain, H, V, innov, filter_vjp):
    """HybridNLP.landing_loglik_grad in numpy: the gradient of each record's log-likelihood with respect to (Sigma0, W, V) through
    the gains' design.  A: the design's blocks; F: the filter's (landing_filter_sweep_ref.blocks); filter_vjp(innov_bar) ->
    Lgain_bar (B, N, 15, ny): landing_filter_sweep_ref.sweep_vjp at fixed gains, no score cotangent.  Returns sweep()'s dict."""
    dt = innov.dtype
    H, V, L = (np.asarray(a, dtype=dt) for a in (H, V, Lgain))
    ny = H.shape[0]
    half_ = dt.type(0.5)
    G = np.eye(ny, dtype=dt) - H @ L                     # (B, N, ny, ny): I - H L
    Si = G / V[:, None]
    innov_bar = -half_ * np.einsum("bkrs,bks->bkr", Si + _t(Si), innov)
    Lb = filter_vjp(innov_bar)
    Lb = Lb + half_ * np.einsum("ri,bkr,bks->bkis", H, innov / V, innov)
    out = sweep(A, H, V, L, Lb, None, np.full(innov.shape[:2], -half_, dtype=dt))
    out["V"] = out["V"] + half_ * (innov * np.einsum("bkrs,bks->bkr", G, innov)).sum(axis=1) / (V * V)
    return out
