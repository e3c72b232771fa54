"""numpy yardstick of qln_tracking_lqr_guarded / qln_tracking_covariance_guarded (include/qln_evaluator.h): the Riccati and
the covariance recursion through the guard-triggered touchdown.  Not a test module.

Nothing of the composite step is restated here: rollout_guarded_sweep_ref.blocks() gives [A_k B_k] per knot and
T = d tau / d (x, u, theta) by complex step, with the saltation term inside, and tracking_ref.riccati /
tracking_cov_ref.propagate / marginals run unchanged on them.  event_var comes from T.  Besides that, a longdouble
restatement of both recursions (np.linalg.solve has no longdouble: a hand-written 4x4 L D L'), used only to measure how far
the float64 yardstick is from it."""
import numpy as np

from tests import rollout_guarded_sweep_ref as SR
from tests import tracking_cov_ref as CR
from tests import tracking_ref as TR

NX, NU = 15, 4


def split(F):
    """[A B G] (..., 15, 24) -> A (..., 15, 15), B (..., 15, 4)."""
    return F[..., :NX], F[..., NX:NX + NU]


def riccati(F, Q, R, Qf):
    """K (B, N-1, 4, 15), P (B, N, 15, 15) on the guarded blocks F (B, N-1, 15, 24)."""
    A, Bm = split(np.asarray(F, dtype=np.float64))
    return TR.riccati(A, Bm, Q, R, Qf)


def _solve4(q, rhs):
    """q (..., 4, 4) symmetric positive definite, rhs (..., 4, n): q^-1 rhs by L D L', any real dtype."""
    L = np.zeros_like(q)
    d = np.zeros(q.shape[:-1], dtype=q.dtype)
    for c in range(NU):
        d[..., c] = q[..., c, c] - sum(L[..., c, m] * L[..., c, m] * d[..., m] for m in range(c))
        L[..., c, c] = 1
        for r in range(c + 1, NU):
            L[..., r, c] = (q[..., r, c] - sum(L[..., r, m] * L[..., c, m] * d[..., m] for m in range(c))) / d[..., c]
    y = np.array(rhs)
    for i in range(NU):
        for m in range(i):
            y[..., i, :] = y[..., i, :] - L[..., i, m, None] * y[..., m, :]
    y = y / d[..., :, None]
    for i in range(NU - 1, -1, -1):
        for m in range(i + 1, NU):
            y[..., i, :] = y[..., i, :] - L[..., m, i, None] * y[..., m, :]
    return y


def riccati_extended(F, Q, R, Qf):
    """tracking_ref.riccati in the dtype of F (longdouble blocks), the 4x4 solve by _solve4."""
    A, Bm = split(F)
    dt = F.dtype
    n1 = A.shape[-3]
    Q, R, Qf = (np.asarray(a, dtype=dt) for a in (Q, R, Qf))
    Pk = np.broadcast_to(np.diag(Qf), A.shape[:-3] + (NX, NX)).copy()
    K = np.zeros(A.shape[:-3] + (n1, NU, NX), dtype=dt)
    P = np.zeros(A.shape[:-3] + (n1 + 1, NX, NX), dtype=dt)
    P[..., n1, :, :] = Pk
    tr = lambda M: np.swapaxes(M, -1, -2)  # noqa: E731
    for k in range(n1 - 1, -1, -1):
        a, b = A[..., k, :, :], Bm[..., k, :, :]
        quu = np.diag(R) + tr(b) @ Pk @ b
        qux = tr(b) @ Pk @ a
        kk = _solve4(quu, qux)
        Pk = np.diag(Q) + tr(a) @ Pk @ a - tr(qux) @ kk
        Pk = (Pk + tr(Pk)) / 2
        K[..., k, :, :], P[..., k, :, :] = kk, Pk
    return K, P


def event_coefficients(T, events, K):
    """c (B, 15) with d tau = c . dx_k* under dF = -K_k* dx: T_x - K_k*' T_F (K None: T_x); zero rows without a touchdown."""
    T = np.asarray(T)
    c = np.array(T[:, :NX])
    if K is not None:
        for b in range(len(T)):
            ks = int(events[b, 0])
            if ks >= 0:
                c[b] = c[b] - np.asarray(K)[b, ks].T @ T[b, NX:NX + NU]
    return c


def covariance(F, T, events, K, Sigma0, W, theta, lb):
    """Sigma (B, N, 15, 15), marg (B, N, 8) and event_var (B, 2) on the guarded blocks, in the dtype of F.  Sigma0 (15, 15) or
    (B, 15, 15), theta (B, N) the body angles of the trajectory, lb (B,) the problems' body lengths."""
    A, Bm = split(F)
    Kd = None if K is None else np.asarray(K, dtype=F.dtype)
    S = CR.propagate(A, Bm, Kd, np.asarray(Sigma0, dtype=F.dtype), None if W is None else np.asarray(W, dtype=F.dtype))
    marg = CR.marginals(S, Kd, np.asarray(theta), np.asarray(lb)[:, None])
    c = event_coefficients(T, events, Kd)
    var = np.zeros((len(F), 2), dtype=F.dtype)
    for b in range(len(F)):
        ks = int(events[b, 0])
        if ks >= 0:
            c1 = np.array(c[b])
            c1[14] += 1
            var[b] = c[b] @ S[b, ks] @ c[b], c1 @ S[b, ks] @ c1
    return S, marg, var


def lq_cost(Zd, N, Q, R, Qf):
    """The LQ cost of the tangent trajectories Zd (B, n_nlp), per problem: sum_k dx_k'Q dx_k + dF_k'R dF_k, and Qf at the end."""
    Zd = np.asarray(Zd)
    z = np.concatenate([Zd, np.zeros((len(Zd), 5), dtype=Zd.dtype)], axis=1).reshape(len(Zd), N, 20)
    return (np.sum(z[:, : N - 1, :NX] ** 2 * Q, axis=(1, 2)) + np.sum(z[:, : N - 1, NX:NX + NU] ** 2 * R, axis=(1, 2)) +
            np.sum(z[:, N - 1, :NX] ** 2 * Qf, axis=1))


def distances(N, init_mode, Zout, th, events, K, Q, R, Qf, Sigma0, W):
    """How far the float64 yardstick is from its longdouble restatement at one case: (K, P, Sigma) in knot_rel and (marg,
    event_var) in entry_rel, on blocks taken in both precisions."""
    F, T = SR.blocks(N, init_mode, Zout, th, events)
    Fl, Tl = SR.blocks(N, init_mode, Zout, th, events, ctype=np.clongdouble)
    theta = np.asarray(Zout)[:, 2::20]
    Kr, Pr = riccati(F, Q, R, Qf)
    Kl, Pl = riccati_extended(Fl, Q, R, Qf)
    S, mg, var = covariance(F, T, events, K, Sigma0, W, theta, th[:, 3])
    Sl, mgl, varl = covariance(Fl, Tl, events, K, Sigma0, W, theta.astype(np.longdouble), th[:, 3].astype(np.longdouble))
    return (CR.knot_rel(Kr, Kl), CR.knot_rel(Pr, Pl), CR.knot_rel(S, Sl), CR.entry_rel(mg, mgl), CR.entry_rel(var, varl))
