"""numpy yardstick of qln_tracking_rollout_estimated_jvp / _vjp and their _guarded forms (include/qln_evaluator.h): the forward
and reverse sweeps through the estimate-feedback roll-out, at fixed noise samples.  Not a test module.

The header's two recursions, batched, in the dtype of the blocks they are given.  The blocks are taken by complex step, once per
chain: the plant's [A B G] at Zout's (x_k, u_k) with the plant's models and the plant's event record, the estimator's at
(Xhat_k, Zout's u_k) with the handle's model and the estimator's record -- rollout_guarded_sweep_ref.blocks for the guarded
forms (whose composite step carries the saltation term without anybody writing it down), the same construction on the handle's
knot schedule for the knot-scheduled ones.  With ctype = clongdouble everything is an extended-precision restatement, used only
to measure how far the float64 yardstick is from it.  case() and directions() are what the CPU and the GPU tests share, so that
the seeds checked on the CPU are the ones the GPU runs."""
import numpy as np

from oracle import np_oracle as O
from tests import rollout_estimated_cases as EC
from tests import rollout_estimated_ref as ER
from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_sweep_ref as SR
from tests import rollout_ref as RR
from tests import tracking_cases as TC

NX, NP, STRIDE = RR.NX, RR.NP, ER.STRIDE
worst = SR.worst


def estimate_knots(Zout, Xhat):
    """The trajectory the estimator's blocks are formed at: Xhat's states with Zout's applied controls, in the layout of Z."""
    Zout = np.asarray(Zout)
    B, N = Xhat.shape[0], Xhat.shape[1]
    z = np.concatenate([Zout, np.zeros((B, 5), dtype=Zout.dtype)], axis=1).reshape(B, N, 20).copy()
    z[:, :, :15] = Xhat
    return z.reshape(B, 20 * N)[:, : 20 * N - 5]


def scheduled_blocks(N, k_trans, init_mode, Z, th, ctype=np.complex128, eps=1e-30):
    """[A_k B_k G_k] (B, N-1, 15, 24) of the knot-scheduled step at Z's knots (B, n_nlp) and models th (B, 4) by complex step,
    k_trans and init_mode an int or (B,): rollout_ref.complex_step_blocks per schedule, in ctype's real dtype."""
    rt = np.real(np.zeros(1, dtype=ctype)).dtype
    Z, th = np.asarray(Z, dtype=rt), np.asarray(th, dtype=rt)
    B = Z.shape[0]
    kt, im = np.broadcast_to(np.asarray(k_trans), (B,)), np.broadcast_to(np.asarray(init_mode), (B,))
    n = 20 + NP
    F = np.zeros((B, N - 1, NX, n), dtype=rt)
    seed = (1j * eps * np.eye(n)).astype(ctype)
    for b in range(B):
        modes, jumps = O.knot_modes(N, int(kt[b]), int(im[b]))
        for k in range(N - 1):
            z = Z[b, None, 20 * k: 20 * k + 20] + seed[:, :20]
            t = th[b][None, :] + seed[:, 20:]
            F[b, k] = (RR.model_step(int(modes[k]), bool(jumps[k]), z[:, :15], z[:, 15:], t).imag / eps).T
    return F


def chain_blocks(N, init_mode, k_trans, Zout, Xhat, th, th_hat, guarded, events=None, events_hat=None, ctype=np.complex128):
    """The two chains' blocks: dict(Fp, Fe (B, N-1, 15, 24), Tp, Te (B, 24) -- d tau of each chain's touchdown knot, zeros for
    the knot-scheduled forms).  th (B, 4) the plant's models, th_hat (4,) the handle's."""
    B = len(Zout)
    th = np.broadcast_to(np.asarray(th), (B, NP))
    thh = np.broadcast_to(np.asarray(th_hat), (B, NP))
    Zhat = estimate_knots(Zout, Xhat)
    if guarded:
        Fp, Tp = SR.blocks(N, init_mode, Zout, th, events, ctype=ctype)
        Fe, Te = SR.blocks(N, init_mode, Zhat, thh, events_hat, ctype=ctype)
    else:
        Fp = scheduled_blocks(N, k_trans, init_mode, Zout, th, ctype)
        Fe = scheduled_blocks(N, k_trans, init_mode, Zhat, thh, ctype)
        Tp = Te = np.zeros((B, 20 + NP), dtype=Fp.dtype)
    return dict(Fp=Fp, Fe=Fe, Tp=Tp, Te=Te)


_mv = lambda M, v: np.einsum("...ij,...j->...i", M, v)  # noqa: E731
_tv = lambda M, v: np.einsum("...ji,...j->...i", M, v)  # noqa: E731


def _knots(a, N):
    """(B, n_nlp) -> views (B, N, 20) of a zero-padded copy"""
    a = np.asarray(a)
    return np.concatenate([a, np.zeros((a.shape[0], 5), dtype=a.dtype)], axis=1).reshape(a.shape[0], N, 20)


def sweep_jvp(blk, Zref, K, Lgain, H, Zout, Xhat, innov, Zref_dot=None, K_dot=None, Lgain_dot=None, x0_dot=None, xhat0_dot=None,
              model_dot=None, events=None, events_hat=None):
    """The header's forward recursion on blk = chain_blocks(...), in the blocks' dtype.  A tangent that is None is zero, except
    xhat0_dot: None is dxm_0 = x_ref_dot,0.  Returns dict(Zout_dot (B, n_nlp), Xhat_dot (B, N, 15), innov_dot (B, N, ny),
    event_dot, event_hat_dot (B, 8): entry 1 d tau, entry 2 the touchdown clock's tangent, of the plant and of the estimator)."""
    Fp, Fe = blk["Fp"], blk["Fe"]
    dt = Fp.dtype
    B, n1 = Fp.shape[0], Fp.shape[1]
    N = n1 + 1
    ld = lambda a: None if a is None else np.asarray(a, dtype=dt)  # noqa: E731
    Zref, K, Lgain, H, Zout, Xhat, innov, zd, kd, Ld, dx, dxm, md = (
        ld(a) for a in (Zref, K, Lgain, H, Zout, Xhat, innov, Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot))
    zr = _knots(Zref, N)
    zdk = np.zeros((B, N, 20), dtype=dt) if zd is None else _knots(zd, N)
    dx = np.zeros((B, NX), dtype=dt) if dx is None else dx.copy()
    dxm = zdk[:, 0, :15].copy() if dxm is None else dxm.copy()
    md = np.zeros((B, NP), dtype=dt) if md is None else md
    out = np.zeros((B, N, 20), dtype=dt)
    Xd, Id = np.zeros((B, N, NX), dtype=dt), np.zeros((B, N, H.shape[0]), dtype=dt)
    for k in range(N):
        Id[:, k] = (dx - dxm) @ H.T
        dxh = dxm + _mv(Lgain[:, k], Id[:, k])
        if Ld is not None:
            dxh = dxh + _mv(Ld[:, k], innov[:, k])
        Xd[:, k], out[:, k, :15] = dxh, dx
        if k == N - 1:
            break
        du = zdk[:, k, 15:].copy()
        if K is not None:
            du[:, :4] -= _mv(K[:, k], dxh - zdk[:, k, :15])
            if kd is not None:
                du[:, :4] -= _mv(kd[:, k], Xhat[:, k] - zr[:, k, :15])
        out[:, k, 15:] = du
        dx = _mv(Fp[:, k, :, :15], dx) + _mv(Fp[:, k, :, 15:20], du) + _mv(Fp[:, k, :, 20:], md)
        dxm = _mv(Fe[:, k, :, :15], dxh) + _mv(Fe[:, k, :, 15:20], du)
    ed, eh = np.zeros((B, STRIDE), dtype=dt), np.zeros((B, STRIDE), dtype=dt)
    for rec, ev, T, states, with_model in ((ed, events, blk["Tp"], out[:, :, :15], True), (eh, events_hat, blk["Te"], Xd, False)):
        if ev is None:
            continue
        for b in range(B):
            ks = int(ev[b, 0])
            if ks < 0 or ks > N - 2:
                continue
            dtau = T[b, :15] @ states[b, ks] + T[b, 15:20] @ out[b, ks, 15:] + (T[b, 20:] @ md[b] if with_model else 0)
            rec[b, 1], rec[b, 2] = dtau, states[b, ks, 14] + dtau
    return dict(Zout_dot=out.reshape(B, 20 * N)[:, : 20 * N - 5], Xhat_dot=Xd, innov_dot=Id, event_dot=ed, event_hat_dot=eh)


def sweep_vjp(blk, Zref, K, Lgain, H, Zout, Xhat, innov, Zbar, Xhat_bar=None, innov_bar=None, with_xhat0=True):
    """The header's reverse recursion on blk, in the blocks' dtype.  Returns dict(Zref_bar (B, n_nlp), K_bar or None, Lgain_bar
    (B, N, 15, ny), x0_bar, xhat0_bar (B, 15) -- None without with_xhat0, and then added to Zref_bar's x_0 slot -- and model_bar
    (B, 4))."""
    Fp, Fe = blk["Fp"], blk["Fe"]
    dt = Fp.dtype
    B, n1 = Fp.shape[0], Fp.shape[1]
    N = n1 + 1
    ld = lambda a: None if a is None else np.asarray(a, dtype=dt)  # noqa: E731
    Zref, K, Lgain, H, Zout, Xhat, innov, Zbar, Xb, Ib = (ld(a) for a in (Zref, K, Lgain, H, Zout, Xhat, innov, Zbar, Xhat_bar,
                                                                         innov_bar))
    ny = H.shape[0]
    zr, zb = _knots(Zref, N), _knots(Zbar, N)
    Xb = np.zeros((B, N, NX), dtype=dt) if Xb is None else Xb
    Ib = np.zeros((B, N, ny), dtype=dt) if Ib is None else Ib
    zrb = np.zeros((B, N, 20), dtype=dt)
    kb = None if K is None else np.zeros_like(K)
    lb = np.zeros((B, N, NX, ny), dtype=dt)
    mb = np.zeros((B, NP), dtype=dt)
    lam, lamm = np.zeros((B, NX), dtype=dt), np.zeros((B, NX), dtype=dt)
    for k in range(N - 1, -1, -1):
        xhb = Xb[:, k].copy()
        ax = np.zeros((B, NX), dtype=dt)
        if k < N - 1:
            ubar = zb[:, k, 15:] + _tv(Fp[:, k, :, 15:20], lam) + _tv(Fe[:, k, :, 15:20], lamm)
            ax = _tv(Fp[:, k, :, :15], lam)
            mb += _tv(Fp[:, k, :, 20:], lam)
            kub = np.zeros((B, NX), dtype=dt) if K is None else _tv(K[:, k], ubar[:, :4])
            xhb = xhb + _tv(Fe[:, k, :, :15], lamm) - kub
            zrb[:, k, 15:], zrb[:, k, :15] = ubar, kub
            if K is not None:
                kb[:, k] = -np.einsum("bm,bj->bmj", ubar[:, :4], Xhat[:, k] - zr[:, k, :15])
        ib = Ib[:, k] + _tv(Lgain[:, k], xhb)
        if innov is not None:
            lb[:, k] = np.einsum("bj,br->bjr", xhb, innov[:, k])
        hib = ib @ H
        lam = zb[:, k, :15] + ax + hib
        lamm = xhb - hib
    if not with_xhat0:
        zrb[:, 0, :15] += lamm
    return dict(Zref_bar=zrb.reshape(B, 20 * N)[:, : 20 * N - 5], K_bar=kb, Lgain_bar=lb if innov is not None else None,
                x0_bar=lam, xhat0_bar=lamm if with_xhat0 else None, model_bar=mb)


TANGENTS = ("Zref_dot", "K_dot", "Lgain_dot", "x0_dot", "xhat0_dot", "model_dot")
SCALE = 1e-2  # tangents of the size of the cases' own perturbations (tests/test_rollout_guarded_sweeps_host.py)


def directions(seed, B, N, ny, scale=SCALE):
    """One random direction of all six inputs and one cotangent of all three outputs, normal draws times scale; the model's
    tangent relative to TC.SECOND's size, the filter gains' at their own scale (rollout_estimated_cases.draws)."""
    rng = np.random.default_rng(seed)
    d = dict(Zref_dot=scale * rng.normal(size=(B, 20 * N - 5)), K_dot=scale * rng.normal(size=(B, N - 1, 4, 15)),
             Lgain_dot=scale * rng.normal(size=(B, N, 15, ny)), x0_dot=scale * rng.normal(size=(B, 15)),
             xhat0_dot=scale * rng.normal(size=(B, 15)), model_dot=scale * rng.normal(size=(B, NP)) * np.abs(TC.SECOND))
    c = dict(Zbar=scale * rng.normal(size=(B, 20 * N - 5)), Xhat_bar=scale * rng.normal(size=(B, N, 15)),
             innov_bar=scale * rng.normal(size=(B, N, ny)))
    return d, c


def case(N, init_mode, k_trans, B, ny, guarded, seed=None):
    """Host inputs of one case: (batch, inp) with inp = dict(Zref, K, Lgain, H, vnoise, wnoise, x0, xhat0, model) -- the guarded
    roll-out's case (rollout_guarded_cases.case: touchdowns spread over the knots, one problem that never lands) or a batch on
    the knot schedule k_trans, random gains and per-problem models, and rollout_estimated_cases.draws for the filter's side."""
    seed = 1000 * N + 100 * init_mode + 10 * k_trans + ny + (5 if guarded else 0) if seed is None else seed
    if guarded:
        batch, Zref, K, x0, th = GC.case(N, init_mode, B, True, True, seed=seed)
    else:
        batch = TC.batch(B, N, k_trans, init_mode, seed=seed)
        rng = np.random.default_rng(seed + 7)
        Zref = np.ascontiguousarray(batch.Z, dtype=np.float64)
        x0 = Zref[:, :15] + 1e-2 * rng.normal(size=(B, 15))
        K = 0.05 * rng.normal(size=(B, N - 1, 4, 15))
        th = RR.draw_models(B, seed + 2, TC.SECOND)
    d = EC.draws(seed + 3, B, N, ny)
    return batch, dict(Zref=Zref, K=K, Lgain=d["Lgain"], H=d["H"], vnoise=d["vnoise"], wnoise=d["wnoise"], x0=x0,
                       xhat0=Zref[:, :15] + d["dxhat0"], model=th)


def rollout(batch, inp, guarded, dtype=np.float64, **replace):
    """rollout_estimated_ref.rollout of a case's inputs (some replaced), the handle's model TC.SECOND."""
    a = dict(inp, **replace)
    return ER.rollout(batch.N, np.asarray(batch.init_mode), a["Zref"], a["K"], a["Lgain"], a["H"], a["x0"],
                      TC.SECOND if a["model"] is None else a["model"], TC.SECOND, a["vnoise"], a["wnoise"], a["xhat0"],
                      np.asarray(batch.k_trans), guarded, dtype)


def central_difference(batch, inp, guarded, dirs, t=1e-6):
    """Longdouble central differences of rollout_estimated_ref.rollout along dirs (a dict of TANGENTS, None for zero; with
    xhat0 None in inp the estimate follows Zref).  Returns (dict(Zout_dot, Xhat_dot, innov_dot, event_dot, event_hat_dot), same
    (B,): the plant's and the estimator's touchdown knots are those of the centre at both offsets)."""
    L = np.longdouble
    names = dict(Zref="Zref_dot", K="K_dot", Lgain="Lgain_dot", x0="x0_dot", xhat0="xhat0_dot", model="model_dot")

    def at(s):
        rep = {}
        for name, dot in names.items():
            a, d = inp[name], dirs.get(dot)
            if a is None:
                a = np.tile(TC.SECOND, (batch.B, 1)) if name == "model" and d is not None else None
            if a is not None:
                rep[name] = np.asarray(a).astype(L) if d is None else np.asarray(a).astype(L) + L(s) * np.asarray(d).astype(L)
        return rollout(batch, inp, guarded, L, **rep)

    p, c, m = at(t), at(0), at(-t)
    q = lambda n: ((p[n] - m[n]) / (2 * L(t))).astype(np.float64)  # noqa: E731
    out = dict(Zout_dot=q("Zout"), Xhat_dot=q("Xhat"), innov_dot=q("innov"))
    same = np.ones(batch.B, dtype=bool)
    if guarded:
        for rec, dot in (("events", "event_dot"), ("events_hat", "event_hat_dot")):
            same &= (p[rec][:, 0] == c[rec][:, 0]) & (m[rec][:, 0] == c[rec][:, 0])
            ed = np.zeros((batch.B, STRIDE))
            ed[:, 1:3] = q(rec)[:, 1:3]
            out[dot] = ed
    return out, same
