"""Symbolic oracle of the Lagrangian Hessian (qln_eval_hessian_lagrangian), built from oracle/np_oracle.py.

The step `rk4`, the jump mask `JUMP_DIAG` and `stagecost` of np_oracle are called on object arrays of sympy symbols
and expanded; the Hessian of

    sigma * h * stagecost(cost_k, x_k, u_k) + mu_dyn,k . (M_k rk4_mode(x_k, u_k))

is differentiated symbolically for every contact mode with and without the jump mask.  The clearance term
mu_clr,k * c''(theta_k) follows quirk Q3's branch and is added numerically (`clearance_curvature`).  `step_pattern`
is the union of the lower-triangle entries that are not identically zero; `step_values` evaluates every entry of a
block, vectorised over knots, through sympy.lambdify -- the value oracle of the GPU tests.
"""
from __future__ import annotations

import functools

import numpy as np
import sympy as sp

from oracle import np_oracle as npo

Z_SYMS = sp.symbols("z0:20")
MU_SYMS = sp.symbols("mu0:15")
SIGMA = sp.Symbol("sigma")
COST_SYMS = sp.symbols("c0:41")
CASES = [(mode, jump) for mode in (1, 2, 3) for jump in (False, True) if not (mode == 3 and jump)]


def lagrangian_hessian(mode: int, jump: bool):
    """Lower triangle {(row, col): expression} of the knot's Lagrangian without the clearance term, for the model
    constants np_oracle holds at the time of the call (they are part of the cache key: the expansions bake them in)."""
    return _lagrangian_hessian(mode, jump, npo.constants())


@functools.lru_cache(maxsize=None)
def _lagrangian_hessian(mode: int, jump: bool, consts):
    assert consts == npo.constants()
    z = np.array(Z_SYMS, dtype=object)
    x, u = z[:15], z[15:]
    step = npo.rk4(mode, x, u)
    mask = npo.JUMP_DIAG if jump else np.ones(15)
    dyn = sum(MU_SYMS[i] * step[i] for i in range(15) if mask[i] != 0)
    obj = SIGMA * u[4] * npo.stagecost(np.array(COST_SYMS, dtype=object), x, u)
    L = sp.expand(dyn + obj)
    out = {}
    for c in range(20):
        dc = sp.diff(L, Z_SYMS[c])
        for r in range(c, 20):
            e = sp.expand(sp.diff(dc, Z_SYMS[r]))
            if e != 0:
                out[(r, c)] = e
    return out


def step_pattern():
    """Union over modes / jump of the structurally non-zero lower-triangle entries, column-major, with (2, 2) (the
    clearance row's theta curvature, which the objective's diagonal holds too)."""
    ent = {(2, 2)}
    for case in CASES:
        ent |= set(lagrangian_hessian(*case))
    return sorted(ent, key=lambda rc: (rc[1], rc[0]))


def _lambdified(mode: int, jump: bool):
    return _lambdified_for(mode, jump, npo.constants())


@functools.lru_cache(maxsize=None)
def _lambdified_for(mode: int, jump: bool, consts):
    H = _lagrangian_hessian(mode, jump, consts)
    args = list(Z_SYMS) + list(MU_SYMS) + [SIGMA] + list(COST_SYMS)
    return {rc: sp.lambdify(args, e, "numpy") for rc, e in H.items()}


def clearance_curvature(theta, lb=None):
    """d/dtheta of jac_c!'s clearance entry (quirk Q3): +(lb/2) sin(theta) for theta > 0, -(lb/2) sin(theta) otherwise;
    lb = None reads np_oracle's LB at the time of the call."""
    lb = npo.LB if lb is None else lb
    theta = np.asarray(theta, dtype=np.float64)
    return np.where(theta > 0, (lb / 2) * np.sin(theta), -((lb / 2) * np.sin(theta)))


def step_values(mode, jump, z, mu, mu_c, sigma, cost):
    """Values of the 55 pattern entries for knots of one (mode, jump) case.
    z: (K, 20), mu: (K, 15) (unmasked: the mask is in the expressions), mu_c: (K,), sigma: (K,), cost: (K, 41)."""
    z, mu, cost = (np.asarray(a, dtype=np.float64) for a in (z, mu, cost))
    K = z.shape[0]
    fns = _lambdified(mode, jump)
    args = [z[:, i] for i in range(20)] + [mu[:, i] for i in range(15)] + [np.asarray(sigma, dtype=np.float64)] + \
        [cost[:, i] for i in range(41)]
    pat = step_pattern()
    out = np.zeros((K, len(pat)))
    for j, rc in enumerate(pat):
        if rc in fns:
            out[:, j] = np.broadcast_to(fns[rc](*args), (K,))
    out[:, pat.index((2, 2))] += np.asarray(mu_c) * clearance_curvature(z[:, 2])
    return out


def problem_hvals(N, k_trans, init_mode, Zb, mu_b, sigma, cost_b):
    """All 55(N-1)+15 values of one problem: Zb (n_nlp,), mu_b: its constraint vector's multipliers (m_nlp,) in cinds
    order, cost_b: (N, 41)."""
    Zb = np.asarray(Zb, dtype=np.float64)
    mu_b = np.asarray(mu_b, dtype=np.float64)
    cost_b = np.asarray(cost_b, dtype=np.float64).reshape(N, 41)
    m_nlp = 18 * N - k_trans + 16
    o_clr = m_nlp - N
    zk = np.stack([Zb[20 * k: 20 * k + 20] for k in range(N - 1)])
    mu_dyn = mu_b[29: 29 + 15 * (N - 1)].reshape(N - 1, 15)
    mu_c = mu_b[o_clr: o_clr + N]
    modes, jumps = npo.knot_modes(N, k_trans, init_mode)
    blocks = np.zeros((N - 1, 55))
    for mode, jump in CASES:
        sel = (modes == mode) & (jumps == jump)
        if sel.any():
            blocks[sel] = step_values(mode, jump, zk[sel], mu_dyn[sel], mu_c[:-1][sel], np.full(sel.sum(), sigma),
                                      cost_b[:-1][sel])
    term = sigma * cost_b[N - 1, :15]
    term = term + 0.0
    term[2] += mu_c[-1] * clearance_curvature(Zb[20 * (N - 1) + 2])
    return np.concatenate([blocks.reshape(-1), term])


def batch_hvals(N, k_trans, init_mode, Z, mu, c_off, sigma, cost):
    """Segments (P, 55(N-1)+15) of P problems with a common N at once (the full-size tests).  Z: (P, >= n_nlp),
    mu: the flat multiplier buffer in the layout of c (problem p at c_off[p]), sigma: (P,), cost: (N, 41) shared or
    (P, N, 41)."""
    Z = np.asarray(Z, dtype=np.float64)
    P = Z.shape[0]
    kt = np.asarray(k_trans, dtype=np.int64).reshape(P)
    im = np.asarray(init_mode, dtype=np.int64).reshape(P)
    c_off = np.asarray(c_off, dtype=np.int64).reshape(P)
    cost = np.asarray(cost, dtype=np.float64)
    cost = np.broadcast_to(cost, (P, N, 41)) if cost.ndim == 2 else cost
    zk = np.stack([Z[:, 20 * k: 20 * k + 20] for k in range(N - 1)], axis=1)          # (P, N-1, 20)
    dyn_idx = c_off[:, None] + 29 + np.arange(15 * (N - 1))[None, :]
    mu_dyn = np.asarray(mu)[dyn_idx].reshape(P, N - 1, 15)
    o_clr = c_off + 17 * N - kt + 16
    mu_c = np.asarray(mu)[o_clr[:, None] + np.arange(N)[None, :]]                      # (P, N)
    K = np.arange(1, N)[None, :]
    modes = np.where(K <= kt[:, None] - 1, im[:, None], 3)
    jumps = K == kt[:, None] - 1
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64).reshape(P, 1), (P, N - 1))
    blocks = np.zeros((P, N - 1, 55))
    for mode, jump in CASES:
        sel = (modes == mode) & (jumps == jump)
        if sel.any():
            blocks[sel] = step_values(mode, jump, zk[sel], mu_dyn[sel], mu_c[:, :-1][sel], sig[sel], cost[:, :-1][sel])
    term = np.asarray(sigma, dtype=np.float64).reshape(P, 1) * cost[:, N - 1, :15]
    term[:, 2] += mu_c[:, -1] * clearance_curvature(Z[:, 20 * (N - 1) + 2])
    return np.concatenate([blocks.reshape(P, -1), term], axis=1)
