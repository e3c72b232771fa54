"""numpy yardstick of qln_tracking_rollout_guarded (include/qln_evaluator.h): the closed-loop roll-out in which touchdown
happens when the free foot reaches the ground.  A restatement of the header's section in any real dtype (float64,
longdouble), vectorised over the batch and built on rollout_ref.model_step -- the step the knot-scheduled yardstick takes
at a model -- so that before the touchdown it is rollout_ref.rollout(k_trans = N + 1) operation for operation.

Besides Zout and the event records it returns a MARGIN per problem.  The touchdown knot is a discrete decision: two correct
implementations that differ by an ulp may take it differently when the decision is close, so a comparison of the results
means something only away from the decision's boundaries.  The margin is the smallest, over the steps up to and including
the touchdown's, of the distances to them: |tau - h| / h (tau taken even when it exceeds h), tau / h, |disc| / v^2, and
|y| where y <= 0."""
import numpy as np

from tests import rollout_ref as RR

STRIDE = 8  # QLN_TOUCHDOWN_INFO_STRIDE
JUMP = [4, 6, 10, 11, 12, 13]


def guard(y, v, a, h):
    """The header's guard, elementwise on arrays of one dtype: (touchdown, tau, the step's margin)."""
    inf = np.array(np.inf, dtype=y.dtype)
    with np.errstate(all="ignore"):
        below = y <= 0
        disc = v * v - 2 * a * y
        den = -v + np.sqrt(disc)
        root = ~below & (disc >= 0) & (den > 0)
        tau = np.where(root, 2 * y / den, 0)
        hit = below | (root & (tau <= h))
        m_root = np.where(root, np.minimum(np.abs(tau - h) / h, tau / h), inf)
        margin = np.where(below, np.abs(y), np.minimum(np.abs(disc) / (v * v), m_root))
    return hit, tau.astype(y.dtype), margin


def _rollout_mode(N, im, Zref, K, x0, th, dt):
    """Every problem starts in mode im."""
    B = Zref.shape[0]
    iy, iv, iF, ix, ivx = (6, 13, 3, 5, 12) if im == 1 else (4, 11, 1, 3, 10)
    Zref, x, th = Zref.astype(dt), x0.astype(dt), th.astype(dt)
    K = None if K is None else K.astype(dt)
    Zo = np.zeros((B, 20 * N - 5), dtype=dt)
    Zo[:, :15] = x
    landed = np.zeros(B, dtype=bool)
    ev = np.zeros((B, STRIDE), dtype=dt)
    ev[:, 0], ev[:, 6] = -1, np.inf
    margin = np.full(B, np.inf, dtype=dt)
    pre = np.full((B, 15), np.nan, dtype=dt)
    for k in range(N - 1):
        u = Zref[:, 20 * k + 15: 20 * k + 20].copy()
        if K is not None:
            u[:, :4] = u[:, :4] - np.einsum("...mj,...j->...m", K[:, k], x - Zref[:, 20 * k: 20 * k + 15])
        Zo[:, 20 * k + 15: 20 * k + 20] = u
        h = u[:, 4]
        standing = np.where(landed, np.fmin(u[:, 1], u[:, 3]), u[:, 1] if im == 1 else u[:, 3])
        ev[:, 6] = np.fmin(ev[:, 6], standing)
        hit, tau, m = guard(x[:, iy], x[:, iv], -u[:, iF] / th[:, 2] + th[:, 0], h)
        hit &= ~landed
        margin = np.where(landed, margin, np.minimum(margin, m))
        # flight mode: the whole step, or its part up to the touchdown
        ut = u.copy()
        ut[:, 4] = np.where(hit, tau, h)
        xf = RR.model_step(im, False, x, ut, th)
        # the touchdown's jump map and the rest of its step in mode 3 (computed for every problem, kept where hit)
        xm = xf.copy()
        xm[:, JUMP] = 0
        ut[:, 4] = h - tau
        xt = RR.model_step(3, False, xm, ut, th)
        xt[:, 14] = x[:, 14] + h
        # mode 3: the problems that landed before this knot
        x3 = RR.model_step(3, False, x, u, th)
        hk = np.flatnonzero(hit)
        pre[hk] = xf[hk]
        ev[hk, 0], ev[hk, 1], ev[hk, 2] = k, tau[hk], x[hk, 14] + tau[hk]
        ev[hk, 3], ev[hk, 4], ev[hk, 5] = xf[hk, ix], xf[hk, ivx], xf[hk, iv]
        x = np.where(landed[:, None], x3, np.where(hit[:, None], xt, xf))
        landed = landed | hit
        Zo[:, 20 * (k + 1): 20 * (k + 1) + 15] = x
    return Zo, ev, margin, pre


def rollout(N, init_mode, Zref, K, x0, th, dtype=np.float64):
    """Zref (B, n_nlp), K (B, N-1, 4, 15) or None, x0 (B, 15), th (4,) or (B, 4) = (g, mb, mf, lb), init_mode an int or
    (B,).  Returns, in `dtype`: Zout (B, n_nlp), events (B, 8), margins (B,) and pre (B, 15), the state just before the jump
    map (NaN without a touchdown)."""
    dt = np.dtype(dtype).type
    Zref, x0 = np.asarray(Zref), np.asarray(x0)
    B = Zref.shape[0]
    th = np.broadcast_to(np.asarray(th), (B, 4))
    im = np.broadcast_to(np.asarray(init_mode), (B,))
    Zo = np.zeros((B, 20 * N - 5), dtype=dt)
    ev, mg, pre = np.zeros((B, STRIDE), dtype=dt), np.zeros(B, dtype=dt), np.zeros((B, 15), dtype=dt)
    for mode in (1, 2):
        i = np.flatnonzero(im == mode)
        if len(i):
            Zo[i], ev[i], mg[i], pre[i] = _rollout_mode(N, mode, Zref[i], None if K is None else np.asarray(K)[i], x0[i],
                                                        th[i], dt)
    return Zo, ev, mg, pre
