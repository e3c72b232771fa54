"""numpy yardstick of qln_tracking_rollout, qln_tracking_rollout_model and their forward and reverse sweeps
(include/qln_evaluator.h): the closed-loop roll-out, dtype-generic so that the whole map can be differentiated by complex
step; the step blocks [A B] (15x20) or, with a plant model th = (g, mb, mf, lb), [A B G] (15x24), from the evaluator's
Jacobian with the jump knot's clock row restored or by complex step; and the two sweeps on either kind of block.

The step is stated twice, on purpose.  oracle_step is oracle/np_oracle.py's rk4 + jump_map, pinned to the reference, with
the model in np_oracle's module constants, which its model() context casts to float.  model_step restates those few lines
with the model as arguments, so that it can carry a complex parameter.  At a real model the two roll-outs are equal
exactly (tests/test_rollout_model_host.py): that comparison is what holds the restatement, so the two stay apart."""
import numpy as np

from oracle import np_oracle as O

NX, NU, NP = 15, 4, 4


def oracle_step(mode, jump, x, u):
    """Phi of np_oracle: the RK4 step of `mode` followed, if jump, by the jump map; x (..., 15), u (..., 5)."""
    xn = O.rk4(int(mode), x, u)
    return O.jump_map(xn) if jump else xn


def dynamics(mode, s, u, th):
    """The continuous dynamics of contact mode `mode` at model th; s (..., 14), u (..., 5), th (..., 4) -> (..., 14)."""
    s, u, th = np.asarray(s), np.asarray(u), np.asarray(th)
    g, mb, mf, lb = th[..., 0], th[..., 1], th[..., 2], th[..., 3]
    ib = mb * (lb * lb) / 12
    lead = np.broadcast_shapes(s.shape[:-1], u.shape[:-1], th.shape[:-1])
    out = np.zeros(lead + (14,), dtype=np.result_type(s.dtype, u.dtype, th.dtype))
    F1x, F1y, F2x, F2y = u[..., 0], u[..., 1], u[..., 2], u[..., 3]
    out[..., 0:3] = s[..., 7:10]
    if mode == 2:
        out[..., 3:5] = s[..., 10:12]
        out[..., 10] = -F1x / mf
        out[..., 11] = -F1y / mf + g
    if mode == 1:
        out[..., 5:7] = s[..., 12:14]
        out[..., 12] = -F2x / mf
        out[..., 13] = -F2y / mf + g
    out[..., 7] = (F1x + F2x) / mb
    out[..., 8] = (F1y + F2y) / mb + g
    tau = -F1x * (s[..., 4] - s[..., 1]) + F1y * (s[..., 3] - s[..., 0]) - F2x * (s[..., 6] - s[..., 1]) + F2y * (s[..., 5] - s[..., 0])
    out[..., 9] = tau / ib
    return out


def model_step(mode, jump, x, u, th):
    """Phi at model th: the RK4 step of `mode` followed, if jump, by the jump map; x (..., 15), u (..., 5), th (..., 4)."""
    x, u = np.asarray(x), np.asarray(u)
    h = u[..., 4:5]
    s = x[..., :14]
    f1 = dynamics(mode, s, u, th)
    f2 = dynamics(mode, s + 0.5 * h * f1, u, th)
    f3 = dynamics(mode, s + 0.5 * h * f2, u, th)
    f4 = dynamics(mode, s + h * f3, u, th)
    sn = s + (h / 6.0) * (f1 + 2 * f2 + 2 * f3 + f4)
    xn = np.concatenate([sn, np.broadcast_to(x[..., 14:15] + u[..., 4:5], sn.shape[:-1] + (1,))], axis=-1)
    if jump:
        xn[..., [4, 6, 10, 11, 12, 13]] = 0.0
    return xn


def _step(mode, jump, x, u, th):
    return oracle_step(mode, jump, x, u) if th is None else model_step(int(mode), bool(jump), x, u, th)


def rollout(N, k_trans, init_mode, Zref, K, x0, th=None):
    """qln_tracking_rollout (th None: the oracle's step) or qln_tracking_rollout_model (th (..., 4)) in numpy, any dtype,
    complex included: Zref (..., n_nlp), K (..., N-1, 4, 15) or None, x0 (..., 15), one mode schedule for every leading
    index; returns Zout (..., n_nlp)."""
    modes, jumps = O.knot_modes(N, k_trans, init_mode)
    Zref, x0 = np.asarray(Zref), np.asarray(x0)
    th = None if th is None else np.asarray(th)
    given = [Zref, x0] + ([] if th is None else [th])
    dt = np.result_type(np.float64 if K is None else np.asarray(K).dtype, *(a.dtype for a in given))
    lead = np.broadcast_shapes(*(a.shape[:-1] for a in given))
    Zo = np.zeros(lead + (20 * N - 5,), dtype=dt)
    x = np.broadcast_to(x0, lead + (15,)).astype(dt)
    Zo[..., :15] = x
    for k in range(N - 1):
        u = np.array(np.broadcast_to(Zref[..., 20 * k + 15: 20 * k + 20], lead + (5,)), dtype=dt)
        if K is not None:
            e = x - Zref[..., 20 * k: 20 * k + 15]
            u[..., :4] = u[..., :4] - (np.einsum("...mj,...j->...m", K[..., k, :, :], e) if lead else K[k] @ e)
        Zo[..., 20 * k + 15: 20 * k + 20] = u
        x = _step(modes[k], jumps[k], x, u, th)
        Zo[..., 20 * (k + 1): 20 * (k + 1) + 15] = x
    return Zo


def evaluator_blocks(blocks, k_trans):
    """Evaluator step blocks (N-1, 15, 20) -> the derivative the roll-out applies: at the jump knot quirk Q1's mask zeroes
    row 14, the jump map keeps the clock, so row 14 is restored at x[14] and at h (tracking_ref.blocks_from_dense restores
    only the first: TVLQR holds h fixed)."""
    F = np.array(blocks, dtype=np.float64, copy=True)
    kj = int(k_trans) - 2  # 0-based jump knot
    if 0 <= kj < len(F):
        F[kj, 14, 14] = 1.0
        F[kj, 14, 19] = 1.0
    return F


def complex_step_blocks(N, k_trans, init_mode, Zout, th=None, eps=1e-30):
    """d Phi_k / d(x_k, u_k), (..., N-1, 15, 20), or with th (..., 4) [A_k B_k G_k] = d Phi_k / d(x_k, u_k, th),
    (..., N-1, 15, 24), at Zout's knots (..., n_nlp), by complex step (exact to rounding).  One mode schedule for every
    leading index."""
    Zout = np.asarray(Zout, dtype=np.float64)
    th = None if th is None else np.asarray(th, dtype=np.float64)
    modes, jumps = O.knot_modes(N, k_trans, init_mode)
    n = 20 if th is None else 20 + NP
    out = np.zeros(Zout.shape[:-1] + (N - 1, NX, n))
    seed = 1j * eps * np.eye(n)
    for k in range(N - 1):
        z = Zout[..., None, 20 * k: 20 * k + 20] + seed[:, :20]         # (..., n, 20)
        t = None if th is None else th[..., None, :] + seed[:, 20:]     # (..., n, 4)
        d = _step(modes[k], jumps[k], z[..., :15], z[..., 15:], t).imag / eps  # (..., n, 15)
        out[..., k, :, :] = np.swapaxes(d, -1, -2)
    return out


def central_difference_G(mode, jump, x, u, th, rel=1e-5):
    """G = d Phi / d th (15, 4) by central differences with a step of rel |th_p| in each parameter."""
    th = np.asarray(th, dtype=np.float64)
    G = np.zeros((NX, NP))
    for p in range(NP):
        e = np.zeros(NP)
        e[p] = rel * abs(th[p])
        G[:, p] = (model_step(mode, jump, x, u, th + e) - model_step(mode, jump, x, u, th - e)) / (2 * e[p])
    return G


def sweep_vjp(F, Zref, K, Zout, Zbar):
    """The header's reverse sweep on blocks F (N-1, 15, 20) or (N-1, 15, 24) for one problem (vectors of length n_nlp, K
    (N-1, 4, 15) or None): returns (Zref_bar (n_nlp,), K_bar (N-1, 4, 15) or None, x0_bar (15,), model_bar (4,), or None
    for blocks without G)."""
    n1 = len(F)
    Zref, Zout, Zbar = (np.asarray(v, dtype=np.float64) for v in (Zref, Zout, Zbar))
    zref_bar = np.zeros(20 * n1 + 15)
    k_bar = None if K is None else np.zeros((n1, NU, NX))
    model_bar = np.zeros(NP) if F.shape[-1] > 20 else None
    lam = Zbar[20 * n1: 20 * n1 + 15].copy()
    for k in range(n1 - 1, -1, -1):
        A, Bm = F[k, :, :15], F[k, :, 15:20]
        if model_bar is not None:
            model_bar += F[k, :, 20:].T @ lam
        ubar = Zbar[20 * k + 15: 20 * k + 20] + Bm.T @ lam
        zref_bar[20 * k + 15: 20 * k + 20] = ubar
        kub = np.zeros(NX) if K is None else K[k].T @ ubar[:4]
        zref_bar[20 * k: 20 * k + 15] = kub
        if K is not None:
            k_bar[k] = -np.outer(ubar[:4], Zout[20 * k: 20 * k + 15] - Zref[20 * k: 20 * k + 15])
        lam = Zbar[20 * k: 20 * k + 15] + A.T @ lam - kub
    return zref_bar, k_bar, lam, model_bar


def sweep_jvp(F, Zref, K, Zout, Zref_dot=None, K_dot=None, x0_dot=None, model_dot=None):
    """The header's forward sweep on blocks F (..., N-1, 15, 20) or, for a model's tangent, (..., N-1, 15, 24); Z-like
    (..., n_nlp), K and K_dot (..., N-1, 4, 15), x0_dot (..., 15), model_dot (..., 4); a tangent that is None is zero.
    Returns Zout_dot (..., n_nlp)."""
    F = np.asarray(F)
    n1 = F.shape[-3]
    Zref, Zout = np.asarray(Zref, dtype=np.float64), np.asarray(Zout, dtype=np.float64)
    zd = np.zeros_like(Zout) if Zref_dot is None else np.asarray(Zref_dot, dtype=np.float64)
    out = np.zeros_like(Zout)
    dx = np.zeros(Zout.shape[:-1] + (NX,)) if x0_dot is None else np.array(x0_dot, dtype=np.float64)
    md = None if model_dot is None else np.asarray(model_dot, dtype=np.float64)
    mv = lambda M, v: np.einsum("...ij,...j->...i", M, v)  # noqa: E731
    for k in range(n1):
        xs, us = slice(20 * k, 20 * k + 15), slice(20 * k + 15, 20 * k + 20)
        du = zd[..., us].copy()
        if K is not None:
            du[..., :4] -= mv(K[..., k, :, :], dx - zd[..., xs])
            if K_dot is not None:
                du[..., :4] -= mv(K_dot[..., k, :, :], Zout[..., xs] - Zref[..., xs])
        out[..., xs] = dx
        out[..., us] = du
        Fk = F[..., k, :, :]
        dx = mv(Fk[..., :15], dx) + mv(Fk[..., 15:20], du)
        if md is not None:
            dx = dx + mv(Fk[..., 20:], md)
    out[..., 20 * n1:] = dx
    return out


def jvp_complex_step(N, k_trans, init_mode, Zref, K, x0, th=None, Zref_dot=None, K_dot=None, x0_dot=None, model_dot=None,
                     eps=1e-30):
    """d/dt rollout(Zref + t Zref_dot, K + t K_dot, x0 + t x0_dot, th + t model_dot) at t = 0: one complex roll-out."""
    zr = np.asarray(Zref, dtype=np.complex128)
    xx = np.asarray(x0, dtype=np.complex128)
    tt = None if th is None else np.asarray(th, dtype=np.complex128)
    kk = None if K is None else np.asarray(K, dtype=np.complex128)
    if Zref_dot is not None:
        zr = zr + 1j * eps * np.asarray(Zref_dot)
    if K_dot is not None:
        kk = kk + 1j * eps * np.asarray(K_dot)
    if x0_dot is not None:
        xx = xx + 1j * eps * np.asarray(x0_dot)
    if model_dot is not None:
        tt = tt + 1j * eps * np.asarray(model_dot)
    return rollout(N, k_trans, init_mode, zr, kk, xx, tt).imag / eps


def vjp_complex_step(N, k_trans, init_mode, Zref, K, x0, Zbar, eps=1e-30):
    """<rollout(Zref, K, x0), Zbar> differentiated by complex step in every scalar of Zref, K and x0: one roll-out per
    scalar.  Returns (Zref_bar, K_bar or None, x0_bar)."""
    Zref = np.asarray(Zref, dtype=np.float64)
    x0 = np.asarray(x0, dtype=np.float64)
    f = lambda zr, kk, xx: np.dot(rollout(N, k_trans, init_mode, zr, kk, xx), Zbar).imag / eps  # noqa: E731
    zb = np.zeros_like(Zref)
    for i in range(len(Zref)):
        z = Zref.astype(np.complex128)
        z[i] += 1j * eps
        zb[i] = f(z, K, x0)
    kb = None
    if K is not None:
        K = np.asarray(K, dtype=np.float64)
        kb = np.zeros(K.size)
        for i in range(K.size):
            kk = K.astype(np.complex128).reshape(-1)
            kk[i] += 1j * eps
            kb[i] = f(Zref, kk.reshape(K.shape), x0)
        kb = kb.reshape(K.shape)
    xb = np.zeros(NX)
    for i in range(NX):
        xx = x0.astype(np.complex128)
        xx[i] += 1j * eps
        xb[i] = f(Zref, K, xx)
    return zb, kb, xb


def draw_models(B, seed, around, spread=0.1):
    """(B, 4) models drawn uniformly within +-spread (relative) of `around`."""
    rng = np.random.default_rng(seed)
    return np.asarray(around) * (1.0 + spread * rng.uniform(-1.0, 1.0, size=(B, NP)))


def identify_model(sens, zout_of, target, th0, iters):
    """Gauss-Newton fit of the model per problem, the numpy statement of examples/identify_model.py's loop: from th0 (B, 4),
    repeat th -= argmin_d |J d - r| with r = zout_of(th) - target (B, n) and J = sens(th) (B, n, 4), the four model
    tangents d Zout / d (g, mb, mf, lb), columns scaled by th0.  Returns th (B, 4)."""
    th = np.array(th0, dtype=np.float64)
    scale = np.abs(th0)
    for _ in range(iters):
        r = zout_of(th) - target
        J = sens(th) * scale[:, None, :]
        JtJ = np.einsum("bni,bnj->bij", J, J)
        Jtr = np.einsum("bni,bn->bi", J, r)
        th -= scale * np.linalg.solve(JtJ, Jtr[..., None])[..., 0]
    return th


def rel(got, ref):
    """Relative norm of the difference (exact zeros compare as zero)."""
    got, ref = np.asarray(got), np.asarray(ref)
    d = np.linalg.norm(got - ref)
    return float(d / max(np.linalg.norm(ref), 1e-300)) if d else 0.0
