"""numpy yardstick of qln_landing_filter / qln_landing_filter_guarded (include/qln_evaluator.h): the estimator of the
estimate-feedback roll-out run on a record -- measurements Y and the applied forces in Zrec's control slots -- and the score of
that record under the filter.  Not a test module.  A restatement of the header's section in any real dtype (float64, longdouble),
vectorised over the batch and built on rollout_estimated_ref's pieces (_Lander, rollout_ref.model_step), so that on the record
of rollout_estimated_ref.rollout its Xhat and innov are that call's, operation for operation up to the subtraction that forms Y.

The guarded form returns the estimator's guard MARGIN, as rollout_estimated_ref does and for its reason.

score() is the header's score of one knot from the gains alone; linear() runs the same recursion on a linear model (blocks A and
offsets c), which is what the dense Gaussian density of the stacked measurements is compared with."""
import numpy as np

from oracle import np_oracle as O
from tests import rollout_estimated_ref as ER
from tests import rollout_ref as RR

NY = 8
STRIDE = ER.STRIDE


def measurements(Zout, Zref, H, vnoise=None):
    """Y (B, N, ny) in the form the roll-out forms it: H (x_k - x_ref,k) + v_k, from a flown or recorded state trajectory"""
    Zout, Zref, H = np.asarray(Zout), np.asarray(Zref), np.asarray(H)
    B = Zout.shape[0]
    N = (Zout.shape[1] + 5) // 20
    k = 20 * np.arange(N)[:, None] + np.arange(15)[None, :]
    y = (Zout[:, k] - Zref[:, k]) @ H.T
    return y if vnoise is None else y + np.asarray(vnoise).reshape(B, N, -1)


def score(Lk, H, V, innov):
    """{nis, ldS} of one knot: Lk (..., 15, ny), H (ny, 15), V (ny,), innov (..., ny), on eight rows as the header states them
    (the rows behind ny: zero rows of H, zero columns of L, V = 1).  nis = sum_r innov[r] e[r] / V[r] with e = innov - H (L innov);
    ldS = - sum log d_i, d the pivots of the right-looking L D L' of the lower triangle of diag(1/V) (I - H L), NaN where a
    pivot is not > 0."""
    dt = Lk.dtype.type
    ny = H.shape[0]
    lead = Lk.shape[:-2]
    H8 = np.zeros((NY, 15), dtype=dt)
    H8[:ny] = H
    L8 = np.zeros(lead + (15, NY), dtype=dt)
    L8[..., :ny] = Lk
    iv = np.ones(NY, dtype=dt)
    iv[:ny] = dt(1) / V
    i8 = np.zeros(lead + (NY,), dtype=dt)
    i8[..., :ny] = innov
    g = (L8 @ i8[..., None])[..., 0]
    e = i8 - (H8 @ g[..., None])[..., 0]
    nis = (i8 * e * iv).sum(axis=-1)
    G = iv[:, None] * (np.eye(NY, dtype=dt) - H8 @ L8)
    G = np.tril(G).copy()
    lds = np.zeros(lead, dtype=dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(NY):
            d = G[..., j, j]
            lds = lds + np.where(d > 0, np.log(np.where(d > 0, d, 1)), np.nan)
            for i in range(j + 1, NY):
                lij = G[..., i, j] / d
                for c in range(j + 1, i + 1):
                    G[..., i, c] = G[..., i, c] - lij * G[..., c, j]
    return nis, -lds


def _group(N, step_hat, Zref, Zrec, Lgain, H, V, Y, xhat0, th_hat, dt):
    """The header's loop for problems that share their step: step_hat(k, xhat, u, th_hat)."""
    B, ny = Zref.shape[0], H.shape[0]
    xh = (Zref[:, :15] if xhat0 is None else xhat0).astype(dt)
    Xhat, innov = np.zeros((B, N, 15), dtype=dt), np.zeros((B, N, ny), dtype=dt)
    sc = np.zeros((B, N, 2), dtype=dt)
    for k in range(N):
        xr = Zref[:, 20 * k: 20 * k + 15]
        innov[:, k] = Y[:, k] - (xh - xr) @ H.T
        xh = xh + np.einsum("bir,br->bi", Lgain[:, k], innov[:, k])
        Xhat[:, k] = xh
        if V is not None:
            sc[:, k, 0], sc[:, k, 1] = score(Lgain[:, k], H, V, innov[:, k])
        if k == N - 1:
            break
        u = Zrec[:, 20 * k + 15: 20 * k + 20].copy()
        xh = step_hat(k, xh, u, th_hat)
    return Xhat, innov, sc


def loglik(sc, ny):
    """-1/2 sum_k (nis_k + ldS_k + ny log 2 pi), summed in knot order"""
    dt = sc.dtype.type
    acc = np.zeros(sc.shape[:-2], dtype=dt)
    for k in range(sc.shape[-2]):
        acc = acc + ((sc[..., k, 0] + sc[..., k, 1]) + dt(ny) * np.log(dt(8) * np.arctan(dt(1))))
    return dt(-0.5) * acc


def replay(N, init_mode, Zref, Zrec, Lgain, H, Y, th_hat, V=None, xhat0=None, k_trans=None, guarded=False, dtype=np.float64):
    """Zref, Zrec (B, n_nlp), Lgain (B, N, 15, ny), H (ny, 15), Y (B, N, ny), th_hat (4,) the handle's model, V (ny,) or None (no
    score), xhat0 (B, 15) or None; init_mode and (knot schedule) k_trans an int or (B,).  Returns a dict in `dtype`: Xhat
    (B, N, 15), innov (B, N, ny), and with V score (B, N, 2) and loglik (B,); guarded also events_hat (B, 8) and margin_hat (B,)."""
    dt = np.dtype(dtype).type
    Zref = np.asarray(Zref)
    B = Zref.shape[0]
    cast = lambda a: None if a is None else np.asarray(a).astype(dt)  # noqa: E731
    Zref, Zrec, Lgain, H, Y, V, xhat0 = (cast(a) for a in (Zref, Zrec, Lgain, H, Y, V, xhat0))
    Y = Y.reshape(B, N, -1)
    th_hat = np.broadcast_to(np.asarray(th_hat), (B, 4)).astype(dt)
    im = np.broadcast_to(np.asarray(init_mode), (B,))
    kt = np.zeros(B, dtype=int) if guarded else np.broadcast_to(np.asarray(k_trans), (B,))
    ny = H.shape[0]
    out = dict(Xhat=np.zeros((B, N, 15), dtype=dt), innov=np.zeros((B, N, ny), dtype=dt))
    sc = np.zeros((B, N, 2), dtype=dt)
    if guarded:
        out.update(events_hat=np.zeros((B, STRIDE), dtype=dt), margin_hat=np.zeros(B, dtype=dt))
    for mode, ktr in sorted({(int(m), int(t)) for m, t in zip(im, kt)}):
        i = np.flatnonzero((im == mode) & (kt == ktr))
        if guarded:
            hat = ER._Lander(mode, len(i), dt)
            step = hat.step
        else:
            modes, jumps = O.knot_modes(N, ktr, mode)
            step = lambda k, x, u, t: RR.model_step(int(modes[k]), bool(jumps[k]), x, u, t)  # noqa: E731
        xh, iv, s = _group(N, step, Zref[i], Zrec[i], Lgain[i], H, V, Y[i], None if xhat0 is None else xhat0[i], th_hat[i], dt)
        out["Xhat"][i], out["innov"][i], sc[i] = xh, iv, s
        if guarded:
            out["events_hat"][i], out["margin_hat"][i] = hat.ev, hat.margin
    if V is not None:
        out["score"], out["loglik"] = sc, loglik(sc, ny)
    return out


def linear(A, L, H, V, m0, y, c=None):
    """The same recursion on the linear model x_{k+1} = A_k x_k + c_k + w_k, y_k = H x_k + v_k from the prior mean m0, under the
    gains L (..., N, 15, ny): (Xhat, innov, score (..., N, 2), loglik)."""
    A = np.asarray(A)
    dt = A.dtype
    L, H, V, y = (np.asarray(a, dtype=dt) for a in (L, H, V, y))
    N = L.shape[-3]
    mv = lambda M, v: (M @ v[..., None])[..., 0]  # noqa: E731
    pred = np.asarray(m0, dtype=dt)
    Xhat, innov, sc = [], [], []
    for k in range(N):
        iv = y[..., k, :] - mv(H, pred)
        xh = pred + mv(L[..., k, :, :], iv)
        Lk = np.broadcast_to(L[..., k, :, :], iv.shape[:-1] + L.shape[-2:])
        sc.append(np.stack(score(Lk, H, V, iv), axis=-1))
        innov.append(iv)
        Xhat.append(xh)
        if k < N - 1:
            pred = mv(A[..., k, :, :], xh) + (0 if c is None else np.asarray(c, dtype=dt)[..., k, :])
    sc = np.stack(sc, axis=-2)
    return np.stack(Xhat, axis=-2), np.stack(innov, axis=-2), sc, loglik(sc, H.shape[0])
