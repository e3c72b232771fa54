"""numpy yardstick of qln_tracking_rollout_guarded_jvp / _vjp (include/qln_evaluator.h): the forward and reverse sweeps
through the guard-triggered touchdown.  Not a test module.

The composite step of the touchdown knot is a dtype-generic function on rollout_ref.model_step, with tau taken from the
header's closed form of the state, the forces and the model, so that a complex or longdouble perturbation carries through
it: its complex-step derivative holds the saltation term without anybody writing that term down.  [A B G] per knot is taken
by complex step at a FROZEN touchdown knot (the knot is what the event record says; modes before and behind it follow), and
rollout_ref.sweep_jvp / sweep_vjp then run unchanged on those blocks.  event_dot comes from the same complex step.  With
freeze_tau the composite step holds tau at its value instead: the blocks a sweep without the saltation term would use."""
import numpy as np

from tests import rollout_guarded_ref as GR
from tests import rollout_ref as RR

NX, NP = RR.NX, RR.NP
JUMP = GR.JUMP


def foot(im):
    """(iy, iv, iF): the free foot's height and vertical velocity in x and its vertical force in u (mode 1 frees foot 2)."""
    return (6, 13, 3) if int(im) == 1 else (4, 11, 1)


def touchdown_time(im, x, u, th):
    """tau of the header's guard at a knot that lands, any dtype (complex: the branches follow the real parts):
    0 where y <= 0, else 2 y / (-v + sqrt(v^2 - 2 a y)) with a = -F_y / mf + g."""
    iy, iv, iF = foot(im)
    y, v = x[..., iy], x[..., iv]
    a = -u[..., iF] / th[..., 2] + th[..., 0]
    with np.errstate(all="ignore"):
        disc = v * v - 2 * a * y
        den = -v + np.sqrt(disc)
        return np.where(np.real(y) <= 0, 0 * y, 2 * y / den)


def composite_step(im, x, u, th, tau=None):
    """The touchdown knot's step: RK4 over tau in mode im, the jump map, RK4 over h - tau in mode 3, the forces held, the
    clock advanced by h.  x (..., 15), u (..., 5), th (..., 4), any dtype; tau None: the closed form of (x, u, th), else the
    given value, held.  Returns (x_next, tau)."""
    x, u, th = np.asarray(x), np.asarray(u), np.asarray(th)
    if tau is None:
        tau = touchdown_time(im, x, u, th)
    dt = np.result_type(x.dtype, u.dtype, th.dtype, np.asarray(tau).dtype)
    lead = np.broadcast_shapes(x.shape[:-1], u.shape[:-1], th.shape[:-1])
    h = u[..., 4]
    ut = np.array(np.broadcast_to(u, lead + (5,)), dtype=dt)
    ut[..., 4] = tau
    xf = RR.model_step(int(im), False, x, ut, th)
    xm = np.array(xf)
    xm[..., JUMP] = 0
    ut[..., 4] = h - tau
    xt = RR.model_step(3, False, xm, ut, th)
    xt[..., 14] = x[..., 14] + h
    return xt, tau


def blocks(N, init_mode, Zout, th, events, freeze_tau=False, ctype=np.complex128, eps=1e-30):
    """[A_k B_k G_k] (B, N-1, 15, 24) of the guarded roll-out at Zout's knots (B, n_nlp), models th (B, 4) and the touchdown
    knots of events (B, 8), by complex step at a frozen knot; and T (B, 24), d tau / d (x_k*, u_k*, theta) at the touchdown
    knot (zero rows without one).  init_mode an int or (B,).  ctype complex128, or clongdouble for an extended-precision
    restatement (Zout and th may then be longdouble)."""
    rt = np.real(np.zeros(1, dtype=ctype)).dtype
    Zout, th = np.asarray(Zout, dtype=rt), np.asarray(th, dtype=rt)
    B = Zout.shape[0]
    im = np.broadcast_to(np.asarray(init_mode), (B,))
    n = 20 + NP
    F, T = np.zeros((B, N - 1, NX, n), dtype=rt), np.zeros((B, n), dtype=rt)
    seed = (1j * eps * np.eye(n)).astype(ctype)
    Zk = np.concatenate([Zout, np.zeros((B, 5), dtype=rt)], axis=1).reshape(B, N, 20)[:, : N - 1]
    for b in range(B):
        ks = int(events[b, 0])
        ks = ks if 0 <= ks <= N - 2 else N - 1  # no touchdown: every knot is "before" it
        z = Zk[b][:, None, :] + seed[None, :, :20]   # (N-1, n, 20)
        t = th[b][None, None, :] + seed[None, :, 20:]  # (1, n, 4)
        for mode, sl in ((int(im[b]), slice(0, ks)), (3, slice(ks + 1, N - 1))):
            if sl.start < sl.stop:
                d = RR.model_step(mode, False, z[sl, :, :15], z[sl, :, 15:], t).imag / eps
                F[b, sl] = np.swapaxes(d, -1, -2)
        if ks <= N - 2:
            zk = z[ks]
            tau = np.asarray(events[b, 1], dtype=rt) if freeze_tau else None
            xn, tk = composite_step(int(im[b]), zk[:, :15], zk[:, 15:], t[0], tau)
            F[b, ks] = (xn.imag / eps).T
            if not freeze_tau:
                T[b] = np.imag(tk) / eps
    return F, T


def sweep_jvp(F, T, events, Zref, K, Zout, Zref_dot=None, K_dot=None, x0_dot=None, model_dot=None):
    """rollout_ref.sweep_jvp on the guarded blocks, and event_dot (B, 8) from T: entry 1 is d tau, entry 2 the touchdown
    clock's tangent dx_k*[14] + d tau, the rest zeros."""
    zd = RR.sweep_jvp(F, Zref, K, Zout, Zref_dot, K_dot, x0_dot, model_dot)
    B = zd.shape[0]
    ed = np.zeros((B, GR.STRIDE))
    for b in range(B):
        ks = int(events[b, 0])
        if ks < 0:
            continue
        d = zd[b, 20 * ks: 20 * ks + 20]
        dtau = T[b, :20] @ d + (0.0 if model_dot is None else T[b, 20:] @ np.asarray(model_dot)[b])
        ed[b, 1], ed[b, 2] = dtau, d[14] + dtau
    return zd, ed


def sweep_vjp(F, Zref, K, Zout, Zbar):
    """rollout_ref.sweep_vjp per problem on the guarded blocks: (Zref_bar (B, n), K_bar (B, N-1, 4, 15) or None, x0_bar
    (B, 15), model_bar (B, 4))."""
    outs = [RR.sweep_vjp(F[b], Zref[b], None if K is None else K[b], Zout[b], Zbar[b]) for b in range(len(F))]
    zb, kb, xb, mb = (None if o[0] is None else np.stack(o) for o in zip(*outs))
    return zb, kb, xb, mb


def sweep_jvp_extended(F, K, Zref, Zout, Zref_dot, K_dot, x0_dot, model_dot):
    """The forward recursion in the dtype of F (longdouble blocks: an extended-precision restatement), every tangent given;
    used only to measure how far the float64 yardstick is from it."""
    dt = F.dtype
    n1 = F.shape[1]
    ld = lambda a: None if a is None else np.asarray(a, dtype=dt)  # noqa: E731
    K, Zref, Zout, zd, K_dot, dx, md = (ld(a) for a in (K, Zref, Zout, Zref_dot, K_dot, x0_dot, model_dot))
    out = np.zeros_like(Zout)
    mv = lambda M, v: np.einsum("...ij,...j->...i", M, v)  # noqa: E731
    for k in range(n1):
        xs, us = slice(20 * k, 20 * k + 15), slice(20 * k + 15, 20 * k + 20)
        du = zd[:, us].copy()
        if K is not None:
            du[:, :4] -= mv(K[:, k], dx - zd[:, xs])
            if K_dot is not None:
                du[:, :4] -= mv(K_dot[:, k], Zout[:, xs] - Zref[:, xs])
        out[:, xs], out[:, us] = dx, du
        dx = mv(F[:, k, :, :15], dx) + mv(F[:, k, :, 15:20], du) + mv(F[:, k, :, 20:], md)
    out[:, 20 * n1:] = dx
    return out


def sweep_vjp_extended(F, K, Zref, Zout, Zbar):
    """The reverse recursion in the dtype of F, batched: (Zref_bar, K_bar or None, x0_bar, model_bar); as sweep_jvp_extended,
    used only to measure the float64 yardstick's own distance."""
    dt = F.dtype
    n1 = F.shape[1]
    ld = lambda a: None if a is None else np.asarray(a, dtype=dt)  # noqa: E731
    K, Zref, Zout, Zbar = (ld(a) for a in (K, Zref, Zout, Zbar))
    B = len(F)
    zb = np.zeros_like(Zbar)
    kb = None if K is None else np.zeros_like(K)
    mb = np.zeros((B, NP), dtype=dt)
    tv = lambda M, v: np.einsum("...ji,...j->...i", M, v)  # noqa: E731
    lam = Zbar[:, 20 * n1:].copy()
    for k in range(n1 - 1, -1, -1):
        xs, us = slice(20 * k, 20 * k + 15), slice(20 * k + 15, 20 * k + 20)
        mb += tv(F[:, k, :, 20:], lam)
        ubar = Zbar[:, us] + tv(F[:, k, :, 15:20], lam)
        zb[:, us] = ubar
        kub = np.zeros((B, NX), dtype=dt) if K is None else tv(K[:, k], ubar[:, :4])
        zb[:, xs] = kub
        if K is not None:
            kb[:, k] = -np.einsum("bm,bj->bmj", ubar[:, :4], Zout[:, xs] - Zref[:, xs])
        lam = Zbar[:, xs] + tv(F[:, k, :, :15], lam) - kub
    return zb, kb, lam, mb


def directions(seed, B, N, with_gains, scale=1.0):
    """One random direction of all four inputs: (Zref_dot (B, n), K_dot or None, x0_dot (B, 15), model_dot (B, 4)), normal
    draws times scale; the model's is relative to TC.SECOND's size so that no parameter dominates."""
    from tests import tracking_cases as TC

    rng = np.random.default_rng(seed)
    zd = scale * rng.normal(size=(B, 20 * N - 5))
    kd = scale * rng.normal(size=(B, N - 1, 4, 15)) if with_gains else None
    xd = scale * rng.normal(size=(B, 15))
    md = scale * rng.normal(size=(B, NP)) * np.abs(np.asarray(TC.SECOND, dtype=np.float64))
    return zd, kd, xd, md


def central_difference(N, init_mode, Zref, K, x0, th, dirs, t=1e-7):
    """Longdouble central differences of rollout_guarded_ref.rollout along dirs = (Zref_dot, K_dot, x0_dot, model_dot), each
    None for zero: (Zout_dot (B, n), event_dot (B, 8) with entries 1:3 filled, same (B,): the touchdown knot is the same at
    +t, 0 and -t)."""
    L = np.longdouble
    zd, kd, xd, md = dirs

    def at(s):
        add = lambda a, d: None if a is None else (a.astype(L) if d is None else a.astype(L) + L(s) * d.astype(L))  # noqa: E731
        return GR.rollout(N, init_mode, add(Zref, zd), add(K, kd), add(x0, xd), add(np.broadcast_to(th, (len(Zref), 4)), md),
                          dtype=L)

    (zp, ep, _, _), (z0, e0, _, _), (zm, em, _, _) = at(t), at(0), at(-t)
    same = (ep[:, 0] == e0[:, 0]) & (em[:, 0] == e0[:, 0])
    ed = np.zeros((len(Zref), GR.STRIDE))
    ed[:, 1:3] = ((ep[:, 1:3] - em[:, 1:3]) / (2 * L(t))).astype(np.float64)
    return ((zp - zm) / (2 * L(t))).astype(np.float64), ed, same


def worst(got, ref):
    """max |got - ref| / max(1, |ref|), elementwise."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if got.size else 0.0
