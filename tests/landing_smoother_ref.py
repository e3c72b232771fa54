"""numpy yardstick of qln_landing_smoother / qln_landing_smoother_guarded (include/qln_evaluator.h): the fixed-interval smoother
of a flown landing.  Not a test module.  dtype-generic, as tracking_kalman_ref: the arrays keep the dtype they come in with
(float64, or longdouble to measure the recursion's own rounding), and leading dimensions broadcast, so one set of blocks and
gains smooths a whole batch of records.

bryson_frazier() is the statement of the header.  Two checks on it, neither sharing its algebra: rts(), the classical
Rauch-Tung-Striebel recursion, which needs the inverse of P^-_{k+1} (tracking_kalman_ref.ldl_solve) and so a regular prior,
and stacked(), the dense MAP solve of the whole linear-Gaussian problem in its 15 N unknowns.  filter_means() runs the
filter's means on the linear model, which is what makes a record (Xhat, innov) for them."""
import numpy as np

from tests import tracking_guarded_ref as TG
from tests import tracking_kalman_ref as KR

NX = KR.NX
_t, sym = KR._t, KR.sym


def _mv(M, v):
    return (M @ v[..., None])[..., 0]


def bryson_frazier(A, L, Pp, H, V, Xhat, innov):
    """The header's recursion.  A (..., N-1, 15, 15), L (..., N, 15, ny) and Pp (..., N, 15, 15) the filter's gains and P^+,
    H (ny, 15), V (ny,), Xhat (..., N, 15), innov (..., N, ny).  Returns (Xs (..., N, 15), Ps (..., N, 15, 15))."""
    A = np.asarray(A)
    dt = A.dtype
    L, Pp, H, V, Xhat, innov = (np.asarray(a, dtype=dt) for a in (L, Pp, H, V, Xhat, innov))
    N = L.shape[-3]
    I = np.eye(NX, dtype=dt)
    q = np.zeros(NX, dtype=dt)
    Th = np.zeros((NX, NX), dtype=dt)
    Xs, Ps = [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        P, Lk = Pp[..., k, :, :], L[..., k, :, :]
        Xs[k] = Xhat[..., k, :] + _mv(P, q)
        Ps[k] = sym(P - P @ Th @ P)
        if k == 0:
            break
        C = I - Lk @ H
        e = innov[..., k, :] - _mv(H, _mv(Lk, innov[..., k, :]))
        r = _mv(H.T, e / V) + _mv(_t(C), q)
        Lam = sym((H.T / V) @ H @ C + _t(C) @ Th @ C)
        a = A[..., k - 1, :, :]
        q = _mv(_t(a), r)
        Th = _t(a) @ Lam @ a
    lead = np.broadcast_shapes(*(x.shape[:-1] for x in Xs))
    Xs = np.stack([np.broadcast_to(x, lead + (NX,)) for x in Xs], axis=-2)
    lead = np.broadcast_shapes(*(p.shape[:-2] for p in Ps))
    return Xs, np.stack([np.broadcast_to(p, lead + (NX, NX)) for p in Ps], axis=-3)


def rts(A, L, Pm, Pp, Xhat, innov):
    """The classical recursion on the same record: with G_k = P^+_k A_k' (P^-_{k+1})^-1 and the prediction read back from the
    record, xhat^-_{k+1} = Xhat_{k+1} - L_{k+1} innov_{k+1},
        Xs_k = Xhat_k + G_k (Xs_{k+1} - xhat^-_{k+1}),   Ps_k = P^+_k + G_k (Ps_{k+1} - P^-_{k+1}) G_k'.
    P^-_{k+1} must be regular."""
    A = np.asarray(A)
    dt = A.dtype
    L, Pm, Pp, Xhat, innov = (np.asarray(a, dtype=dt) for a in (L, Pm, Pp, Xhat, innov))
    N = L.shape[-3]
    Xs, Ps = [None] * N, [None] * N
    Xs[N - 1], Ps[N - 1] = Xhat[..., N - 1, :], sym(Pp[..., N - 1, :, :])
    for k in range(N - 2, -1, -1):
        a, P, Pn = A[..., k, :, :], Pp[..., k, :, :], Pm[..., k + 1, :, :]
        G = _t(KR.ldl_solve(Pn, a @ P))
        pred = Xhat[..., k + 1, :] - _mv(L[..., k + 1, :, :], innov[..., k + 1, :])
        Xs[k] = Xhat[..., k, :] + _mv(G, Xs[k + 1] - pred)
        Ps[k] = sym(P + G @ (Ps[k + 1] - Pn) @ _t(G))
    lead = np.broadcast_shapes(*(x.shape[:-1] for x in Xs))
    Xs = np.stack([np.broadcast_to(x, lead + (NX,)) for x in Xs], axis=-2)
    lead = np.broadcast_shapes(*(p.shape[:-2] for p in Ps))
    return Xs, np.stack([np.broadcast_to(p, lead + (NX, NX)) for p in Ps], axis=-3)


def filter_means(A, L, H, m0, y, c=None):
    """The filter's means on the linear model x_{k+1} = A_k x_k + c_k + w_k, y_k = H x_k + v_k, from the prior mean m0 and the
    measurements y (..., N, ny) under the gains L: (Xhat (..., N, 15), innov (..., N, ny))."""
    A = np.asarray(A)
    dt = A.dtype
    L, H, y = np.asarray(L, dtype=dt), np.asarray(H, dtype=dt), np.asarray(y, dtype=dt)
    N = L.shape[-3]
    pred = np.asarray(m0, dtype=dt)
    Xhat, innov = [], []
    for k in range(N):
        innov.append(y[..., k, :] - _mv(H, pred))
        Xhat.append(pred + _mv(L[..., k, :, :], innov[-1]))
        if k < N - 1:
            pred = _mv(A[..., k, :, :], Xhat[-1]) + (0 if c is None else np.asarray(c, dtype=dt)[..., k, :])
    return np.stack(Xhat, axis=-2), np.stack(innov, axis=-2)


def stacked(A, H, V, Sigma0, W, m0, y, c=None):
    """The dense MAP solve: the mean and the covariance of (x_0 .. x_{N-1}) given every y_k, from the normal equations of
        (x_0 - m0)' Sigma0^-1 (.) + sum_k (x_{k+1} - A_k x_k - c_k)' diag(W)^-1 (.) + sum_k (y_k - H x_k)' diag(V)^-1 (.)
    in n N unknowns, n = A.shape[-1] (15, or fewer with slots eliminated).  Sigma0 and W must be regular.  One problem, no
    leading dimensions.  Returns (Xs (N, n), Ps (N, n, n)), the diagonal blocks of the inverse."""
    A = np.asarray(A)
    dt = A.dtype
    H, V, Sigma0, W, m0, y = (np.asarray(a, dtype=dt) for a in (H, V, Sigma0, W, m0, y))
    n, N = A.shape[-1], y.shape[0]
    I = np.eye(n, dtype=dt)
    J = np.zeros((n * N, n * N), dtype=dt)
    g = np.zeros((n * N, 1), dtype=dt)
    S0i = KR.ldl_solve(Sigma0, I)
    Wi = np.diag(1 / W)
    HVH, HV = (H.T / V) @ H, H.T / V
    s = lambda k: slice(n * k, n * (k + 1))  # noqa: E731
    J[s(0), s(0)] += S0i
    g[s(0), 0] += S0i @ m0
    for k in range(N):
        J[s(k), s(k)] += HVH
        g[s(k), 0] += HV @ y[k]
        if k < N - 1:
            a = A[k]
            ck = np.zeros(n, dtype=dt) if c is None else np.asarray(c, dtype=dt)[k]
            J[s(k + 1), s(k + 1)] += Wi
            J[s(k), s(k)] += a.T @ Wi @ a
            J[s(k + 1), s(k)] -= Wi @ a
            J[s(k), s(k + 1)] -= a.T @ Wi
            g[s(k + 1), 0] += Wi @ ck
            g[s(k), 0] -= a.T @ Wi @ ck
    J = (J + J.T) / 2
    sol = KR.ldl_solve(J, np.concatenate([g, np.eye(n * N, dtype=dt)], axis=1))
    Xs = sol[:, 0].reshape(N, n)
    Ps = np.stack([sol[s(k), 1 + n * k: 1 + n * (k + 1)] for k in range(N)])
    return Xs, (Ps + _t(Ps)) / 2


def guarded(F, L, Pp, H, V, Xhat, innov):
    """The guarded form on rollout_guarded_sweep_ref.blocks()'s F (B, N-1, 15, 19): the touchdown knot's block is the
    composite A*, and the recursion is the same."""
    A, _ = TG.split(F)
    return bryson_frazier(A, L, Pp, H, V, Xhat, innov)
