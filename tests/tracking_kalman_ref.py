"""numpy yardstick of qln_tracking_kalman / qln_tracking_kalman_guarded (include/qln_evaluator.h): the Kalman filter along a
trajectory's step blocks and the covariance of the loop that feeds back its estimate.  Not a test module.  dtype-generic, as
tracking_cov_ref: the arrays keep the dtype they come in with (float64, or longdouble to measure the recursion's own
rounding); np.linalg has no longdouble, so the ny x ny system is solved by a hand-written L D L' in every dtype.

recursion() is the statement of the header.  joint() is the check on it: the 30 x 30 covariance of (x, xhat^-) propagated
with the filter's gains, which does not use that estimate and error are orthogonal."""
import numpy as np

from tests import tracking_cov_ref as CR
from tests import tracking_guarded_ref as TG

NX, NU = CR.NX, CR.NU


def _t(M):
    return np.swapaxes(M, -1, -2)


def sym(M):
    """formed on the lower triangle: exactly symmetric"""
    return CR.unpack(CR.pack(M))


def ldl_solve(q, rhs):
    """q (..., n, n) symmetric positive definite, rhs (..., n, m): q^-1 rhs by L D L' without pivoting, any real dtype."""
    n = q.shape[-1]
    L = np.zeros_like(q)
    d = np.zeros(q.shape[:-1], dtype=q.dtype)
    for c in range(n):
        d[..., c] = q[..., c, c] - sum(L[..., c, m] * L[..., c, m] * d[..., m] for m in range(c))
        L[..., c, c] = 1
        for r in range(c + 1, n):
            L[..., r, c] = (q[..., r, c] - sum(L[..., r, m] * L[..., c, m] * d[..., m] for m in range(c))) / d[..., c]
    y = np.array(rhs)
    for i in range(n):
        for m in range(i):
            y[..., i, :] = y[..., i, :] - L[..., i, m, None] * y[..., m, :]
    y = y / d[..., :, None]
    for i in range(n - 1, -1, -1):
        for m in range(i + 1, n):
            y[..., i, :] = y[..., i, :] - L[..., m, i, None] * y[..., m, :]
    return y


def update(Pm, H, V):
    """One measurement update: (L (..., 15, ny), P+ (..., 15, 15)) from the prior Pm, Joseph form."""
    S = H @ Pm @ H.T + np.diag(V)
    L = _t(ldl_solve(S, H @ Pm))  # L = P H' S^-1, S and P symmetric
    IL = np.eye(NX, dtype=Pm.dtype) - L @ H
    return L, sym(IL @ Pm @ _t(IL) + (L * V) @ _t(L))


def recursion(A, B, K, H, V, Sigma0, W=None):
    """The header's recursion on blocks A (..., N-1, 15, 15), B (..., N-1, 15, 4), gains K (..., N-1, 4, 15) or None (the
    filter alone), H (ny, 15), V (ny,), Sigma0 (..., 15, 15) or (15, 15), W (15,) or None.  Returns a dict: L (..., N, 15,
    ny), Pm = P^-, Pp = P^+ (..., N, 15, 15), and with K also M and X = M + P^+."""
    A = np.asarray(A)
    dt = A.dtype
    B, H, V = np.asarray(B, dtype=dt), np.asarray(H, dtype=dt), np.asarray(V, dtype=dt)
    Kd = None if K is None else np.asarray(K, dtype=dt)
    lead, n1 = A.shape[:-3], A.shape[-3]
    N, ny = n1 + 1, H.shape[0]
    Wm = np.zeros((NX, NX), dtype=dt) if W is None else np.diag(np.asarray(W, dtype=dt))
    P = np.broadcast_to(sym(np.asarray(Sigma0, dtype=dt)), lead + (NX, NX))
    Mm = np.zeros(lead + (NX, NX), dtype=dt)
    out = {"L": np.zeros(lead + (N, NX, ny), dtype=dt)}
    for name in ("Pm", "Pp") + (() if Kd is None else ("M", "X")):
        out[name] = np.zeros(lead + (N, NX, NX), dtype=dt)
    for k in range(N):
        L, Pp = update(P, H, V)
        out["L"][..., k, :, :], out["Pm"][..., k, :, :], out["Pp"][..., k, :, :] = L, P, Pp
        if Kd is not None:
            M = Mm + (P - Pp)
            out["M"][..., k, :, :], out["X"][..., k, :, :] = M, M + Pp
        if k < n1:
            a = A[..., k, :, :]
            P = sym(a @ Pp @ _t(a) + Wm)
            if Kd is not None:
                acl = a - B[..., k, :, :] @ Kd[..., k, :, :]
                Mm = sym(acl @ M @ _t(acl))
    return out


def joint(A, B, K, H, V, Sigma0, Lgain, W=None):
    """X_k (..., N, 15, 15) from the 30 x 30 covariance J of z = (dx, xhat^-), the true state and the estimate before the
    knot's measurement, under the filter's gains Lgain and dF = -K xhat^+; nothing here assumes that estimate and error are
    orthogonal.  With xhat^+ = xhat^- + L (H (dx - xhat^-) + v):
        dx+     = A dx - B K xhat^+ + w
        xhat^-+ = (A - B K) xhat^+
    J_0 = [[Sigma0, 0], [0, 0]]."""
    A = np.asarray(A)
    dt = A.dtype
    B, K, H, V, Lgain = (np.asarray(a, dtype=dt) for a in (B, K, H, V, Lgain))
    lead, n1 = A.shape[:-3], A.shape[-3]
    Wd = np.zeros(NX, dtype=dt) if W is None else np.asarray(W, dtype=dt)
    J = np.zeros(lead + (2 * NX, 2 * NX), dtype=dt)
    J[..., :NX, :NX] = np.asarray(Sigma0, dtype=dt)
    X = np.zeros(lead + (n1 + 1, NX, NX), dtype=dt)
    I = np.eye(NX, dtype=dt)
    for k in range(n1 + 1):
        X[..., k, :, :] = J[..., :NX, :NX]
        if k == n1:
            break
        L = Lgain[..., k, :, :]
        a, bk = A[..., k, :, :], B[..., k, :, :] @ K[..., k, :, :]
        LH = L @ H
        # xhat^+ = LH dx + (I - LH) xhat^- + L v
        E = np.concatenate([LH, I - LH], axis=-1)                         # (..., 15, 30)
        Tz = np.concatenate([np.concatenate([a, np.zeros_like(a)], axis=-1) - bk @ E, (a - bk) @ E], axis=-2)
        Tv = np.concatenate([-bk @ L, (a - bk) @ L], axis=-2)             # (..., 30, ny)
        J = Tz @ J @ _t(Tz) + (Tv * V) @ _t(Tv)
        J[..., :NX, :NX] = J[..., :NX, :NX] + np.diag(Wd)
    return X


def marginals(X, M, K, theta, lb):
    """marg (..., N, 8) of the header: tracking_cov_ref.marginals on X, with the applied-force variances diag(K M K')."""
    out = CR.marginals(X, None, theta, lb)
    if K is not None:
        K = np.asarray(K, dtype=X.dtype)
        N = X.shape[-3]
        out[..., : N - 1, 1:5] = np.einsum("...mi,...ij,...mj->...m", K, M[..., : N - 1, :, :], K)
    return out


def guarded(F, T, events, K, H, V, Sigma0, W, theta, lb):
    """The guarded form on rollout_guarded_sweep_ref.blocks()'s (F, T): recursion()'s dict plus marg (B, N, 8) and event_var
    (B, 2) = c' M c + t_x' P^+ t_x at the touchdown knot and the same with e_14 added to both (K None: neither)."""
    A, Bm = TG.split(F)
    out = recursion(A, Bm, K, H, V, Sigma0, W)
    if K is None:
        return out
    dt = F.dtype
    Kd = np.asarray(K, dtype=dt)
    out["marg"] = marginals(out["X"], out["M"], Kd, np.asarray(theta), np.asarray(lb)[:, None])
    c = TG.event_coefficients(T, events, Kd)
    tx = np.asarray(T)[:, :NX]
    var = np.zeros((len(F), 2), dtype=dt)
    e14 = np.zeros(NX, dtype=dt)
    e14[14] = 1
    for b in range(len(F)):
        ks = int(events[b, 0])
        if ks >= 0:
            M, P = out["M"][b, ks], out["Pp"][b, ks]
            c1, t1 = c[b] + e14, tx[b] + e14
            var[b] = c[b] @ M @ c[b] + tx[b] @ P @ tx[b], c1 @ M @ c1 + t1 @ P @ t1
    out["event_var"] = var
    return out
