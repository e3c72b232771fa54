"""numpy yardstick of the contact-aware force limits (include/qln_evaluator.h): qln_tracking_rollout_limited, its sweeps and its
gain design.  Not a test module.

The roll-out is a restatement of the header's section in any real dtype (float64, longdouble), vectorised over the batch: the
guarded one is rollout_guarded_ref._rollout_mode with the clamp between the feedback law and everything that reads the
forces, operation for operation, so that with infinite limits the two are equal exactly; the knot-scheduled one is
rollout_ref.rollout at a model with the same clamp.  Nothing of the derivative is restated: the sweeps and the Riccati
recursion are the existing block-taking yardsticks on blocks whose B columns are masked by the saturation record
(mask_blocks), with the applied forces' slots of Zout_dot / Zbar masked the same way (a clamped force is a constant).

Besides the guard's margin (rollout_guarded_ref) the roll-out returns a FORCE margin per problem: the active set is a discrete
decision too, and the smallest |F - limit| / max(1, |F|) over knots and channels says how far the problem is from taking it
differently."""
import numpy as np

from oracle import np_oracle as O
from tests import rollout_guarded_ref as GR
from tests import rollout_guarded_sweep_ref as SR
from tests import rollout_ref as RR

N_LIM = 8  # QLN_FORCE_LIMITS_N
INF = np.inf
NO_LIMITS = np.array([-INF, INF] * 4)
# the issue's test limits: {free_x, free_y, stand_x, stand_y} as {lo, hi} pairs
TEST_LIMITS = np.array([-0.3, 0.3, -0.05, 49.5, -0.4, 0.4, 48.6, 98.15])
POW4 = np.array([1, 4, 16, 64])


def clamp(F, stand1, stand2, lim):
    """The header's clamp on F (B, 4), stand1 / stand2 (B,) bool: (F_applied, s (B, 4) int in {0, 1, 2}, margin (B,))."""
    dt = F.dtype
    lim = np.asarray(lim, dtype=dt)
    stand = np.stack([stand1, stand1, stand2, stand2], axis=1)
    ax = np.array([0, 2, 0, 2])
    lo = np.where(stand, lim[4 + ax], lim[ax])
    hi = np.where(stand, lim[5 + ax], lim[1 + ax])
    with np.errstate(invalid="ignore"):
        below, above = F < lo, F > hi
        s = np.where(below, 1, np.where(above, 2, 0))
        Fa = np.where(below, lo, np.where(above, hi, F)).astype(dt)
        size = np.maximum(1, np.abs(F))
        d = np.minimum(np.abs(F - lo), np.abs(F - hi)) / size
        d = np.where(np.isnan(d), np.inf, d)
    return Fa, s, d.min(axis=1)


def _feedback(Zref, K, x, k):
    u = Zref[:, 20 * k + 15: 20 * k + 20].copy()
    if K is not None:
        u[:, :4] = u[:, :4] - np.einsum("...mj,...j->...m", K[:, k], x - Zref[:, 20 * k: 20 * k + 15])
    return u


def _guarded_mode(N, im, Zref, K, x0, th, lim, dt):
    """rollout_guarded_ref._rollout_mode with the clamp: every problem starts in mode im."""
    B = Zref.shape[0]
    iy, iv, iF, ix, ivx = (6, 13, 3, 5, 12) if im == 1 else (4, 11, 1, 3, 10)
    Zref, x, th = Zref.astype(dt), x0.astype(dt), th.astype(dt)
    K = None if K is None else K.astype(dt)
    Zo = np.zeros((B, 20 * N - 5), dtype=dt)
    Zo[:, :15] = x
    landed = np.zeros(B, dtype=bool)
    ev = np.zeros((B, GR.STRIDE), dtype=dt)
    ev[:, 0], ev[:, 6] = -1, np.inf
    margin = np.full(B, np.inf, dtype=dt)
    fmargin = np.full(B, np.inf, dtype=dt)
    sat = np.zeros((B, N - 1))
    for k in range(N - 1):
        u = _feedback(Zref, K, x, k)
        # the clamp: foot 1 stands in modes 1 and 3, foot 2 in modes 2 and 3, by the mode at the knot's start
        u[:, :4], s, fm = clamp(u[:, :4], landed | (im == 1), landed | (im == 2), lim)
        sat[:, k] = s @ POW4
        fmargin = np.minimum(fmargin, fm)
        Zo[:, 20 * k + 15: 20 * k + 20] = u
        h = u[:, 4]
        standing = np.where(landed, np.fmin(u[:, 1], u[:, 3]), u[:, 1] if im == 1 else u[:, 3])
        ev[:, 6] = np.fmin(ev[:, 6], standing)
        hit, tau, m = GR.guard(x[:, iy], x[:, iv], -u[:, iF] / th[:, 2] + th[:, 0], h)
        hit &= ~landed
        margin = np.where(landed, margin, np.minimum(margin, m))
        ut = u.copy()
        ut[:, 4] = np.where(hit, tau, h)
        xf = RR.model_step(im, False, x, ut, th)
        xm = xf.copy()
        xm[:, GR.JUMP] = 0
        ut[:, 4] = h - tau
        xt = RR.model_step(3, False, xm, ut, th)
        xt[:, 14] = x[:, 14] + h
        x3 = RR.model_step(3, False, x, u, th)
        hk = np.flatnonzero(hit)
        ev[hk, 0], ev[hk, 1], ev[hk, 2] = k, tau[hk], x[hk, 14] + tau[hk]
        ev[hk, 3], ev[hk, 4], ev[hk, 5] = xf[hk, ix], xf[hk, ivx], xf[hk, iv]
        x = np.where(landed[:, None], x3, np.where(hit[:, None], xt, xf))
        landed = landed | hit
        Zo[:, 20 * (k + 1): 20 * (k + 1) + 15] = x
    return Zo, ev, sat, margin, fmargin


def _scheduled_mode(N, kt, im, Zref, K, x0, th, lim, dt):
    """rollout_ref.rollout at the models th on the schedule (kt, im), with the clamp."""
    modes, jumps = O.knot_modes(N, kt, im)
    B = Zref.shape[0]
    Zref, x, th = Zref.astype(dt), x0.astype(dt), th.astype(dt)
    K = None if K is None else K.astype(dt)
    Zo = np.zeros((B, 20 * N - 5), dtype=dt)
    Zo[:, :15] = x
    sat = np.zeros((B, N - 1))
    fmargin = np.full(B, np.inf, dtype=dt)
    for k in range(N - 1):
        u = _feedback(Zref, K, x, k)
        m = int(modes[k])
        u[:, :4], s, fm = clamp(u[:, :4], np.full(B, m in (1, 3)), np.full(B, m in (2, 3)), lim)
        sat[:, k] = s @ POW4
        fmargin = np.minimum(fmargin, fm)
        Zo[:, 20 * k + 15: 20 * k + 20] = u
        x = RR.model_step(m, bool(jumps[k]), x, u, th)
        Zo[:, 20 * (k + 1): 20 * (k + 1) + 15] = x
    return Zo, sat, fmargin


def rollout(N, init_mode, Zref, K, x0, th, lim, dtype=np.float64):
    """The guarded limited roll-out.  Arguments as rollout_guarded_ref.rollout, lim (8,).  Returns, in `dtype`: Zout (B, n_nlp),
    events (B, 8), sat (B, N-1) float64 codes, the guard's margins (B,) and the force margins (B,)."""
    dt = np.dtype(dtype).type
    Zref, x0 = np.asarray(Zref), np.asarray(x0)
    B = Zref.shape[0]
    th = np.broadcast_to(np.asarray(th), (B, 4))
    im = np.broadcast_to(np.asarray(init_mode), (B,))
    Zo = np.zeros((B, 20 * N - 5), dtype=dt)
    ev, sat = np.zeros((B, GR.STRIDE), dtype=dt), np.zeros((B, N - 1))
    mg, fm = np.zeros(B, dtype=dt), np.zeros(B, dtype=dt)
    for mode in (1, 2):
        i = np.flatnonzero(im == mode)
        if len(i):
            Zo[i], ev[i], sat[i], mg[i], fm[i] = _guarded_mode(N, mode, Zref[i], None if K is None else np.asarray(K)[i], x0[i],
                                                              th[i], lim, dt)
    return Zo, ev, sat, mg, fm


def rollout_scheduled(N, k_trans, init_mode, Zref, K, x0, th, lim, dtype=np.float64):
    """The knot-scheduled limited roll-out; k_trans and init_mode ints or (B,).  Returns Zout, sat, the force margins."""
    dt = np.dtype(dtype).type
    Zref, x0 = np.asarray(Zref), np.asarray(x0)
    B = Zref.shape[0]
    th = np.broadcast_to(np.asarray(th), (B, 4))
    im = np.broadcast_to(np.asarray(init_mode), (B,))
    kt = np.broadcast_to(np.asarray(k_trans), (B,))
    Zo, sat, fm = np.zeros((B, 20 * N - 5), dtype=dt), np.zeros((B, N - 1)), np.zeros(B, dtype=dt)
    for key in sorted(set(zip(kt.tolist(), im.tolist()))):
        i = np.flatnonzero((kt == key[0]) & (im == key[1]))
        Zo[i], sat[i], fm[i] = _scheduled_mode(N, key[0], key[1], Zref[i], None if K is None else np.asarray(K)[i], x0[i], th[i],
                                               lim, dt)
    return Zo, sat, fm


def unpack(sat):
    """codes (..., ) -> digits s_m (..., 4) in {0, 1, 2}."""
    c = np.asarray(sat).astype(np.int64)
    return (c[..., None] // POW4) % 4


def free_channels(sat):
    """(B, N-1, 4) bool: the channel did not ride a limit."""
    return unpack(sat) == 0


def mask_blocks(F, sat):
    """[A B (G)] (B, N-1, 15, 20 | 24) with the B columns of the saturated channels set to zero."""
    Fm = np.array(F)
    Fm[..., 15:19] = np.where(free_channels(sat)[:, :, None, :], Fm[..., 15:19], 0)
    return Fm


def mask_forces(Z, sat):
    """A Z-like (B, n_nlp) array with the force slots of the saturated channels set to zero."""
    B, n1 = np.asarray(sat).shape
    Zm = np.array(Z)
    v = Zm[:, : 20 * n1].reshape(B, n1, 20)
    v[:, :, 15:19] = np.where(free_channels(sat), v[:, :, 15:19], 0)
    Zm[:, : 20 * n1] = v.reshape(B, -1)
    return Zm


def mask_gains(K, sat):
    """K (B, N-1, 4, 15) with the rows of the saturated channels set to zero."""
    return np.where(free_channels(sat)[..., None], np.asarray(K), 0)


def sweep_jvp(F, T, events, sat, Zref, K, Zout, Zref_dot=None, K_dot=None, x0_dot=None, model_dot=None):
    """The forward sweep at fixed active set on blocks F (B, N-1, 15, 24): rollout_ref.sweep_jvp on the masked blocks, dF's
    slots masked, and event_dot from T (None: the knot-scheduled sweep, no record) on the masked tangent."""
    zd = mask_forces(RR.sweep_jvp(mask_blocks(F, sat), Zref, K, Zout, Zref_dot, K_dot, x0_dot, model_dot), sat)
    if T is None:
        return zd, None
    ed = np.zeros((len(zd), GR.STRIDE))
    for b in range(len(zd)):
        ks = int(events[b, 0])
        if ks >= 0:
            d = zd[b, 20 * ks: 20 * ks + 20]
            dtau = T[b, :20] @ d + (0.0 if model_dot is None else T[b, 20:] @ np.asarray(model_dot)[b])
            ed[b, 1], ed[b, 2] = dtau, d[14] + dtau
    return zd, ed


def sweep_vjp(F, sat, Zref, K, Zout, Zbar):
    """The reverse sweep at fixed active set: rollout_guarded_sweep_ref.sweep_vjp on the masked blocks with the saturated
    channels' slots of Zbar masked (their ubar goes nowhere)."""
    return SR.sweep_vjp(mask_blocks(F, sat), Zref, K, Zout, mask_forces(Zbar, sat))


def scheduled_blocks(N, k_trans, init_mode, Zout, th, ctype=np.complex128, eps=1e-30):
    """[A_k B_k G_k] (B, N-1, 15, 24) of the knot-scheduled roll-out at the models th, by complex step; k_trans and init_mode
    ints or (B,)."""
    rt = np.real(np.zeros(1, dtype=ctype)).dtype
    Zout, th = np.asarray(Zout, dtype=rt), np.asarray(th, dtype=rt)
    B = len(Zout)
    kt, im = np.broadcast_to(np.asarray(k_trans), (B,)), np.broadcast_to(np.asarray(init_mode), (B,))
    n = 20 + RR.NP
    seed = (1j * eps * np.eye(n)).astype(ctype)
    F = np.zeros((B, N - 1, 15, n), dtype=rt)
    for b in range(B):
        modes, jumps = O.knot_modes(N, int(kt[b]), int(im[b]))
        for k in range(N - 1):
            z = Zout[b, None, 20 * k: 20 * k + 20] + seed[:, :20]
            t = th[b][None, :] + seed[:, 20:]
            F[b, k] = (RR.model_step(int(modes[k]), bool(jumps[k]), z[:, :15], z[:, 15:], t).imag / eps).T
    return F


def central_difference(N, init_mode, Zref, K, x0, th, lim, dirs, t=1e-7):
    """Longdouble central differences of the guarded limited roll-out along dirs = (Zref_dot, K_dot, x0_dot, model_dot), each
    None for zero, as rollout_guarded_sweep_ref.central_difference: (Zout_dot (B, n), event_dot (B, 8) with entries 1:3
    filled, same (B,): the touchdown knot and every knot's saturation code are the same at +t, 0 and -t)."""
    L = np.longdouble
    zd, kd, xd, md = dirs

    def at(s):
        add = lambda a, d: None if a is None else (a.astype(L) if d is None else a.astype(L) + L(s) * d.astype(L))  # noqa: E731
        return rollout(N, init_mode, add(Zref, zd), add(K, kd), add(x0, xd), add(np.broadcast_to(th, (len(Zref), 4)), md), lim,
                       dtype=L)

    (zp, ep, sp, _, _), (z0, e0, s0, _, _), (zm, em, sm, _, _) = at(t), at(0), at(-t)
    same = (ep[:, 0] == e0[:, 0]) & (em[:, 0] == e0[:, 0]) & np.all(sp == s0, axis=1) & np.all(sm == s0, axis=1)
    ed = np.zeros((len(Zref), GR.STRIDE))
    ed[:, 1:3] = ((ep[:, 1:3] - em[:, 1:3]) / (2 * L(t))).astype(np.float64)
    return ((zp - zm) / (2 * L(t))).astype(np.float64), ed, same
