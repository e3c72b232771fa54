"""numpy yardstick of qln_tracking_rollout_vjp (include/qln_evaluator.h): the reverse sweep of the closed-loop roll-out on
dense 15x20 step blocks, the blocks from two sources (the evaluator's Jacobian with the jump knot's clock row restored, and
complex-step differentiation of oracle/np_oracle.py's rk4 + jump_map), and the roll-out itself in numpy, dtype-generic, so
that the whole map can be differentiated by complex step."""
import numpy as np

NX, NU = 15, 4


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


def _step(mode, jump, x, u):
    from oracle import np_oracle as O

    xn = O.rk4(int(mode), x, u)
    return O.jump_map(xn) if jump else xn


def complex_step_blocks(N, k_trans, init_mode, Zout, eps=1e-30):
    """d Phi_k / d(x_k, u_k) (N-1, 15, 20) at Zout's knots, by complex step of rk4 + jump_map (exact to rounding)."""
    from oracle import np_oracle as O

    Zout = np.asarray(Zout, dtype=np.float64)
    modes, jumps = O.knot_modes(N, k_trans, init_mode)
    out = np.zeros((N - 1, NX, 20))
    for k in range(N - 1):
        z = np.broadcast_to(Zout[20 * k: 20 * k + 20], (20, 20)).astype(np.complex128)
        z = z + 1j * eps * np.eye(20)
        out[k] = _step(modes[k], jumps[k], z[:, :15], z[:, 15:]).imag.T / eps
    return out


def sweep(F, Zref, K, Zout, Zbar):
    """The header's reverse sweep on blocks F (N-1, 15, 20) for one problem (vectors of length n_nlp, K (N-1, 4, 15) or
    None): returns (Zref_bar (n_nlp,), K_bar (N-1, 4, 15) or None, x0_bar (15,))."""
    n1 = len(F)
    N = n1 + 1
    Zref, Zout, Zbar = (np.asarray(v, dtype=np.float64) for v in (Zref, Zout, Zbar))
    zref_bar = np.zeros(20 * N - 5)
    k_bar = None if K is None else np.zeros((n1, NU, NX))
    lam = Zbar[20 * n1: 20 * n1 + 15].copy()
    for k in range(n1 - 1, -1, -1):
        A, Bm = F[k, :, :15], F[k, :, 15:]
        ubar = Zbar[20 * k + 15: 20 * k + 20] + Bm.T @ lam
        zref_bar[20 * k + 15: 20 * k + 20] = ubar
        kub = np.zeros(NX) if K is None else K[k].T @ ubar[:4]
        zref_bar[20 * k: 20 * k + 15] = kub
        if K is not None:
            k_bar[k] = -np.outer(ubar[:4], Zout[20 * k: 20 * k + 15] - Zref[20 * k: 20 * k + 15])
        lam = Zbar[20 * k: 20 * k + 15] + A.T @ lam - kub
    return zref_bar, k_bar, lam


def rollout(N, k_trans, init_mode, Zref, K, x0):
    """qln_tracking_rollout in numpy for one problem (any dtype, complex included): returns Zout (n_nlp,)."""
    from oracle import np_oracle as O

    modes, jumps = O.knot_modes(N, k_trans, init_mode)
    dt = np.result_type(np.asarray(Zref).dtype, np.asarray(x0).dtype, np.float64 if K is None else np.asarray(K).dtype)
    Zo = np.zeros(20 * N - 5, dtype=dt)
    x = np.asarray(x0, dtype=dt)
    Zo[:15] = x
    for k in range(N - 1):
        u = np.array(Zref[20 * k + 15: 20 * k + 20], dtype=dt)
        if K is not None:
            u[:4] = u[:4] - K[k] @ (x - Zref[20 * k: 20 * k + 15])
        Zo[20 * k + 15: 20 * k + 20] = u
        x = _step(modes[k], jumps[k], x, u)
        Zo[20 * (k + 1): 20 * (k + 1) + 15] = x
    return Zo


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


def rel(got, ref):
    """Relative norm of the difference (exact zeros compare as zero)."""
    got, ref = np.asarray(got), np.asarray(ref)
    d = np.linalg.norm(got - ref)
    return float(d / max(np.linalg.norm(ref), 1e-300)) if d else 0.0
