"""numpy yardstick of qln_tracking_rollout_estimated / qln_tracking_rollout_estimated_guarded (include/qln_evaluator.h): the
nonlinear hybrid plant and the estimator rolled out together, the forces fed back from the estimate.  Not a test module.  A
restatement of the header's section in any real dtype (float64, longdouble), vectorised over the batch and built on
rollout_ref.model_step and rollout_guarded_ref.guard, so that with Lgain = 0 its Zout is rollout_ref.rollout(K = None) /
rollout_guarded_ref.rollout(K = None) operation for operation.

The guarded form returns the plant's and the estimator's guard MARGINS, as rollout_guarded_ref does and for its reason: the
touchdown knot is a discrete decision, and a comparison of two correct implementations means something only away from the
decision's boundaries -- here the plant's and the estimator's."""
import numpy as np

from oracle import np_oracle as O
from tests import rollout_guarded_ref as GR
from tests import rollout_ref as RR

STRIDE = GR.STRIDE
JUMP = GR.JUMP


class _Lander:
    """One of the two hybrid systems of the guarded form (the plant, or the estimator): its contact state, its touchdown
    record and its guard margin, for a group of problems that start in mode im.  step() is one knot of
    rollout_guarded_ref._rollout_mode."""

    def __init__(self, im, B, dt):
        self.im = im
        self.iy, self.iv, self.iF, self.ix, self.ivx = (6, 13, 3, 5, 12) if im == 1 else (4, 11, 1, 3, 10)
        self.landed = np.zeros(B, dtype=bool)
        self.ev = np.zeros((B, STRIDE), dtype=dt)
        self.ev[:, 0], self.ev[:, 6] = -1, np.inf
        self.margin = np.full(B, np.inf, dtype=dt)

    def step(self, k, x, u, th):
        im, landed, ev = self.im, self.landed, self.ev
        h = u[:, 4]
        standing = np.where(landed, np.fmin(u[:, 1], u[:, 3]), u[:, 1] if im == 1 else u[:, 3])
        ev[:, 6] = np.fmin(ev[:, 6], standing)
        hit, tau, m = GR.guard(x[:, self.iy], x[:, self.iv], -u[:, self.iF] / th[:, 2] + th[:, 0], h)
        hit &= ~landed
        self.margin = np.where(landed, self.margin, np.minimum(self.margin, m))
        ut = u.copy()
        ut[:, 4] = np.where(hit, tau, h)
        xf = RR.model_step(im, False, x, ut, th)
        xm = xf.copy()
        xm[:, JUMP] = 0
        ut[:, 4] = h - tau
        xt = RR.model_step(3, False, xm, ut, th)
        xt[:, 14] = x[:, 14] + h
        x3 = RR.model_step(3, False, x, u, th)
        hk = np.flatnonzero(hit)
        ev[hk, 0], ev[hk, 1], ev[hk, 2] = k, tau[hk], x[hk, 14] + tau[hk]
        ev[hk, 3], ev[hk, 4], ev[hk, 5] = xf[hk, self.ix], xf[hk, self.ivx], xf[hk, self.iv]
        xn = np.where(landed[:, None], x3, np.where(hit[:, None], xt, xf))
        self.landed = landed | hit
        return xn


def _group(N, step_plant, step_hat, Zref, K, Lgain, H, vnoise, wnoise, x0, xhat0, th, th_hat, dt):
    """The header's loop for problems that share their steps: step_plant(k, x, u, th) and step_hat(k, xhat, u, th_hat)."""
    B, ny = Zref.shape[0], H.shape[0]
    x, xh = x0.astype(dt), (Zref[:, :15] if xhat0 is None else xhat0).astype(dt)
    Zo = np.zeros((B, 20 * N - 5), dtype=dt)
    Xhat, innov = np.zeros((B, N, 15), dtype=dt), np.zeros((B, N, ny), dtype=dt)
    Zo[:, :15] = x
    for k in range(N):
        xr = Zref[:, 20 * k: 20 * k + 15]
        y = (x - xr) @ H.T
        if vnoise is not None:
            y = y + vnoise[:, k]
        innov[:, k] = y - (xh - xr) @ H.T
        xh = xh + np.einsum("bir,br->bi", Lgain[:, k], innov[:, k])
        Xhat[:, k] = xh
        if k == N - 1:
            break
        u = Zref[:, 20 * k + 15: 20 * k + 20].copy()
        if K is not None:
            u[:, :4] = u[:, :4] - np.einsum("...mj,...j->...m", K[:, k], xh - xr)
        Zo[:, 20 * k + 15: 20 * k + 20] = u
        x = step_plant(k, x, u, th)
        if wnoise is not None:
            x = x + wnoise[:, k]
        Zo[:, 20 * (k + 1): 20 * (k + 1) + 15] = x
        xh = step_hat(k, xh, u, th_hat)
    return Zo, Xhat, innov


def rollout(N, init_mode, Zref, K, Lgain, H, x0, th, th_hat, vnoise=None, wnoise=None, xhat0=None, k_trans=None, guarded=False,
            dtype=np.float64):
    """Zref (B, n_nlp), K (B, N-1, 4, 15) or None, Lgain (B, N, 15, ny), H (ny, 15), x0 (B, 15), th (4,) or (B, 4) the plant's
    (g, mb, mf, lb), th_hat (4,) the handle's, vnoise (B, N, ny), wnoise (B, N-1, 15) and xhat0 (B, 15) or None; init_mode and
    (knot schedule) k_trans an int or (B,).  Returns a dict in `dtype`: Zout (B, n_nlp), Xhat (B, N, 15), innov (B, N, ny), and
    guarded also events, events_hat (B, 8) and margin, margin_hat (B,)."""
    dt = np.dtype(dtype).type
    Zref = np.asarray(Zref)
    B = Zref.shape[0]
    cast = lambda a: None if a is None else np.asarray(a).astype(dt)  # noqa: E731
    Zref, K, Lgain, H, x0, vnoise, wnoise, xhat0 = (cast(a) for a in (Zref, K, Lgain, H, x0, vnoise, wnoise, xhat0))
    th = np.broadcast_to(np.asarray(th), (B, 4)).astype(dt)
    th_hat = np.broadcast_to(np.asarray(th_hat), (B, 4)).astype(dt)
    im = np.broadcast_to(np.asarray(init_mode), (B,))
    kt = np.zeros(B, dtype=int) if guarded else np.broadcast_to(np.asarray(k_trans), (B,))
    ny = H.shape[0]
    out = dict(Zout=np.zeros((B, 20 * N - 5), dtype=dt), Xhat=np.zeros((B, N, 15), dtype=dt), innov=np.zeros((B, N, ny), dtype=dt))
    if guarded:
        out.update(events=np.zeros((B, STRIDE), dtype=dt), events_hat=np.zeros((B, STRIDE), dtype=dt),
                   margin=np.zeros(B, dtype=dt), margin_hat=np.zeros(B, dtype=dt))
    for mode, ktr in sorted({(int(m), int(t)) for m, t in zip(im, kt)}):
        i = np.flatnonzero((im == mode) & (kt == ktr))
        sub = lambda a: None if a is None else a[i]  # noqa: E731
        if guarded:
            plant, hat = _Lander(mode, len(i), dt), _Lander(mode, len(i), dt)
            steps = (plant.step, hat.step)
        else:
            modes, jumps = O.knot_modes(N, ktr, mode)
            one = lambda k, x, u, t: RR.model_step(int(modes[k]), bool(jumps[k]), x, u, t)  # noqa: E731
            steps = (one, one)
        zo, xh, iv = _group(N, steps[0], steps[1], Zref[i], sub(K), Lgain[i], H, sub(vnoise), sub(wnoise), x0[i], sub(xhat0),
                            th[i], th_hat[i], dt)
        out["Zout"][i], out["Xhat"][i], out["innov"][i] = zo, xh, iv
        if guarded:
            out["events"][i], out["events_hat"][i] = plant.ev, hat.ev
            out["margin"][i], out["margin_hat"][i] = plant.margin, hat.margin
    return out


def linear_joint(A, Bm, K, Lgain, H, dx0, vnoise=None, wnoise=None, xhat0=None):
    """The linear recursion of the deviations (dx, xhat^-) from a nominal with blocks A (..., N-1, 15, 15), Bm (..., N-1, 15, 4),
    driven by the samples: tracking_kalman_ref.joint's transition,
        xhat+ = xhat^- + L (H (dx - xhat^-) + v),   dx' = A dx - B K xhat+ + w,   xhat^-' = (A - B K) xhat+.
    Returns (dx (..., N, 15), xhat+ (..., N, 15), innov (..., N, ny))."""
    n1 = A.shape[-3]
    mv = lambda M, v: np.einsum("...ij,...j->...i", M, v)  # noqa: E731
    dx = np.array(dx0, dtype=np.float64)
    xh = np.zeros_like(dx) if xhat0 is None else np.array(xhat0, dtype=np.float64)
    X, Xh, Iv = [], [], []
    for k in range(n1 + 1):
        iv = (dx - xh) @ H.T
        if vnoise is not None:
            iv = iv + vnoise[..., k, :]
        xh = xh + mv(Lgain[..., k, :, :], iv)
        X.append(dx)
        Xh.append(xh)
        Iv.append(iv)
        if k == n1:
            break
        f = -mv(Bm[..., k, :, :], mv(K[..., k, :, :], xh)) if K is not None else 0.0
        dx = mv(A[..., k, :, :], dx) + f
        if wnoise is not None:
            dx = dx + wnoise[..., k, :]
        xh = mv(A[..., k, :, :], xh) + f
    return np.stack(X, axis=-2), np.stack(Xh, axis=-2), np.stack(Iv, axis=-2)


def direction_ratios(samples, cov, W):
    """For each direction w of W (n, d): the sample variance of w'x over w' cov w; samples (S, d) deviations of known mean zero
    are NOT assumed -- the sample mean is removed (ddof = 1), as tests/test_gpu_tracking_cov.py does."""
    return np.array([np.var(samples @ w, ddof=1) / (w @ cov @ w) for w in W])
