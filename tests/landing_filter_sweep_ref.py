"""numpy yardstick of qln_landing_filter_jvp / _vjp and their _guarded forms (include/qln_evaluator.h): the forward and reverse
sweeps through the filter on recorded data and through its score, at fixed gains.  Not a test module.

The header's two recursions, batched, in the dtype of the blocks they are given.  The blocks [A^e B^e G^e] are taken by complex
step at (Xhat_k, Zrec's u_k, model[b]): rollout_estimated_sweep_ref.scheduled_blocks on the handle's knot schedule,
rollout_guarded_sweep_ref.blocks at the estimator's own touchdown knot for the guarded forms (whose composite step carries the
saltation term without anybody writing it down), both evaluated at estimate_knots(Zrec, Xhat).  With ctype = clongdouble
everything is an extended-precision restatement, used only to measure how far the float64 yardstick is from it.  record(),
directions() and central_difference() are what the CPU and the GPU tests share, so that the seeds checked on the CPU are the ones
the GPU runs."""
import numpy as np

from tests import landing_filter_ref as FR
from tests import rollout_estimated_sweep_ref as ES
from tests import rollout_guarded_sweep_ref as SR
from tests import rollout_ref as RR
from tests import tracking_cases as TC

NX, NP, STRIDE = ES.NX, ES.NP, ES.STRIDE
worst = SR.worst
TANGENTS = ("Y_dot", "Zrec_dot", "Lgain_dot", "xhat0_dot", "model_dot")
COTANGENTS = ("Xhat_bar", "innov_bar", "nis_bar", "loglik_bar")
V_OF = lambda ny: 1e-2 * (1.0 + 0.25 * np.arange(ny))  # noqa: E731  the measurement variances of the cases: no two alike

_mv, _tv = ES._mv, ES._tv


def blocks(N, init_mode, k_trans, Zrec, Xhat, model, guarded, events_hat=None, ctype=np.complex128):
    """(F (B, N-1, 15, 24), T (B, 24)): the estimator's blocks at (Xhat_k, Zrec's u_k, model[b]) and d tau of its touchdown knot
    (zeros for the knot-scheduled forms).  model (B, 4) or (4,)."""
    B = len(Zrec)
    th = np.broadcast_to(np.asarray(model), (B, NP))
    Zhat = ES.estimate_knots(Zrec, Xhat)
    if guarded:
        return SR.blocks(N, init_mode, Zhat, th, events_hat, ctype=ctype)
    F = ES.scheduled_blocks(N, k_trans, init_mode, Zhat, th, ctype)
    return F, np.zeros((B, 20 + NP), dtype=F.dtype)


def _residual(Lk, H, iv, innov):
    """e = innov - H (L innov) and w = innov / V"""
    return innov - _mv(Lk, innov) @ H.T, innov * iv


def sweep_jvp(F, T, Lgain, H, innov=None, V=None, events_hat=None, Y_dot=None, Zrec_dot=None, Lgain_dot=None, xhat0_dot=None,
              model_dot=None):
    """The header's forward recursion in the blocks' dtype.  A tangent that is None is zero.  Returns dict(Xhat_dot (B, N, 15),
    innov_dot (B, N, ny), event_hat_dot (B, 8), and with V nis_dot (B, N) and loglik_dot (B,))."""
    dt = F.dtype
    B, N = F.shape[0], F.shape[1] + 1
    ld = lambda a: None if a is None else np.asarray(a, dtype=dt)  # noqa: E731
    Lgain, H, innov, V, Yd, zd, Ld, dxm, md = (ld(a) for a in (Lgain, H, innov, V, Y_dot, Zrec_dot, Lgain_dot, xhat0_dot, model_dot))
    ny = H.shape[0]
    assert V is None or Ld is None, "the score's tangent is taken at fixed gains"
    Yd = np.zeros((B, N, ny), dtype=dt) if Yd is None else Yd.reshape(B, N, ny)
    zdk = np.zeros((B, N, 20), dtype=dt) if zd is None else ES._knots(zd, N)
    dxm = np.zeros((B, NX), dtype=dt) if dxm is None else dxm.copy()
    md = np.zeros((B, NP), dtype=dt) if md is None else md
    Xd, Id = np.zeros((B, N, NX), dtype=dt), np.zeros((B, N, ny), dtype=dt)
    nd = np.zeros((B, N), dtype=dt)
    du_all = zdk[:, :, 15:]
    for k in range(N):
        din = Yd[:, k] - dxm @ H.T
        dxh = dxm + _mv(Lgain[:, k], din)
        if Ld is not None:
            dxh = dxh + _mv(Ld[:, k], innov[:, k])
        Xd[:, k], Id[:, k] = dxh, din
        if V is not None:
            e, _ = _residual(Lgain[:, k], H, 1 / V, innov[:, k])
            de = din - _mv(Lgain[:, k], din) @ H.T
            nd[:, k] = ((din * e + innov[:, k] * de) / V).sum(axis=-1)
        if k == N - 1:
            break
        dxm = _mv(F[:, k, :, :15], dxh) + _mv(F[:, k, :, 15:20], du_all[:, k]) + _mv(F[:, k, :, 20:], md)
    eh = np.zeros((B, STRIDE), dtype=dt)
    if events_hat is not None:
        for b in range(B):
            ks = int(events_hat[b, 0])
            if 0 <= ks <= N - 2:
                dtau = T[b, :15] @ Xd[b, ks] + T[b, 15:20] @ du_all[b, ks] + T[b, 20:] @ md[b]
                eh[b, 1], eh[b, 2] = dtau, Xd[b, ks, 14] + dtau
    out = dict(Xhat_dot=Xd, innov_dot=Id, event_hat_dot=eh)
    if V is not None:
        acc = np.zeros(B, dtype=dt)
        for k in range(N):
            acc = acc + nd[:, k]
        out.update(nis_dot=nd, loglik_dot=dt.type(-0.5) * acc)
    return out


def sweep_vjp(F, Lgain, H, innov=None, V=None, Xhat_bar=None, innov_bar=None, nis_bar=None, loglik_bar=None, with_gain=None):
    """The header's reverse recursion in the blocks' dtype.  A cotangent that is None is zero.  Returns dict(Y_bar (B, N, ny),
    Zrec_bar (B, n_nlp), Lgain_bar (B, N, 15, ny) or None (with_gain, default: innov given and no score cotangent), xhat0_bar
    (B, 15), model_bar (B, 4))."""
    dt = F.dtype
    B, N = F.shape[0], F.shape[1] + 1
    ld = lambda a: None if a is None else np.asarray(a, dtype=dt)  # noqa: E731
    Lgain, H, innov, V, Xb, Ib, Nb, Lb = (ld(a) for a in (Lgain, H, innov, V, Xhat_bar, innov_bar, nis_bar, loglik_bar))
    ny = H.shape[0]
    score = Nb is not None or Lb is not None
    with_gain = (innov is not None and not score) if with_gain is None else with_gain
    assert not (score and with_gain), "the score's cotangent is taken at fixed gains"
    Xb = np.zeros((B, N, NX), dtype=dt) if Xb is None else Xb
    Ib = np.zeros((B, N, ny), dtype=dt) if Ib is None else Ib.reshape(B, N, ny)
    nb = (np.zeros((B, N), dtype=dt) if Nb is None else Nb) - (np.zeros(B, dtype=dt) if Lb is None else Lb)[:, None] / 2
    zb = np.zeros((B, N, 20), dtype=dt)
    lgb = np.zeros((B, N, NX, ny), dtype=dt) if with_gain else None
    mb = np.zeros((B, NP), dtype=dt)
    Yb = np.zeros((B, N, ny), dtype=dt)
    lamm = np.zeros((B, NX), dtype=dt)
    for k in range(N - 1, -1, -1):
        xhb = Xb[:, k].copy()
        if k < N - 1:
            zb[:, k, 15:] = _tv(F[:, k, :, 15:20], lamm)
            xhb = xhb + _tv(F[:, k, :, :15], lamm)
            mb += _tv(F[:, k, :, 20:], lamm)
        ib = Ib[:, k] + _tv(Lgain[:, k], xhb)
        if score:
            e, w = _residual(Lgain[:, k], H, 1 / V, innov[:, k])
            ib = ib + nb[:, k, None] * ((e / V + w) - _tv(Lgain[:, k], w @ H))
        if with_gain:
            lgb[:, k] = np.einsum("bj,br->bjr", xhb, innov[:, k])
        Yb[:, k] = ib
        lamm = xhb - ib @ H
    return dict(Y_bar=Yb, Zrec_bar=zb.reshape(B, 20 * N)[:, : 20 * N - 5], Lgain_bar=lgb, xhat0_bar=lamm, model_bar=mb)


def inner(cot, fwd, rev, dirs):
    """(lhs, rhs) of the adjoint identity; absent entries count as zero"""
    dot = lambda a, b: 0.0 if a is None or b is None else float(np.dot(np.asarray(a, float).ravel(), np.asarray(b, float).ravel()))  # noqa: E731
    lhs = sum(dot(cot.get(c), fwd.get(c[:-4] + "_dot")) for c in COTANGENTS)
    rhs = sum(dot(rev.get(t[:-4] + "_bar"), dirs.get(t)) for t in TANGENTS)
    return lhs, rhs


SCALE = ES.SCALE


def directions(seed, B, N, ny, scale=SCALE):
    """One random direction of all five inputs and one cotangent of all four outputs; Zrec_dot with NaN-free state slots (they
    are not read), the model's tangent relative to TC.SECOND's size."""
    rng = np.random.default_rng(seed)
    d = dict(Y_dot=scale * rng.normal(size=(B, N, ny)), Zrec_dot=scale * rng.normal(size=(B, 20 * N - 5)),
             Lgain_dot=scale * rng.normal(size=(B, N, 15, ny)), xhat0_dot=scale * rng.normal(size=(B, 15)),
             model_dot=scale * rng.normal(size=(B, NP)) * np.abs(TC.SECOND))
    c = dict(Xhat_bar=scale * rng.normal(size=(B, N, 15)), innov_bar=scale * rng.normal(size=(B, N, ny)),
             nis_bar=scale * rng.normal(size=(B, N)), loglik_bar=scale * rng.normal(size=(B,)))
    return d, c


def record(N, init_mode, k_trans, B, ny, guarded, seed=None):
    """Host inputs of one case: (batch, rec) with rec = dict(Zref, Zrec, Lgain, H, V, Y, xhat0, model): the record of
    rollout_estimated_sweep_ref.case's flight (its Zout and its noisy measurements), flown in float64 numpy, and a generic model
    per record: the flight's own."""
    batch, inp = ES.case(N, init_mode, k_trans, B, ny, guarded, seed)
    flown = ES.rollout(batch, inp, guarded)
    Y = FR.measurements(flown["Zout"], inp["Zref"], inp["H"], inp["vnoise"])
    return batch, dict(Zref=inp["Zref"], Zrec=np.ascontiguousarray(flown["Zout"], dtype=np.float64), Lgain=inp["Lgain"], H=inp["H"],
                       V=V_OF(ny), Y=np.ascontiguousarray(Y, dtype=np.float64), xhat0=inp["xhat0"], model=inp["model"])


def replay(batch, rec, guarded, dtype=np.float64, **replace):
    """landing_filter_ref.replay of a record (some inputs replaced), with the score"""
    a = dict(rec, **replace)
    return FR.replay(batch.N, np.asarray(batch.init_mode), a["Zref"], a["Zrec"], a["Lgain"], a["H"], a["Y"], a["model"], a["V"],
                     a["xhat0"], np.asarray(batch.k_trans), guarded, dtype)


def central_difference(batch, rec, guarded, dirs, t=1e-6, dtype=np.longdouble):
    """Central differences of landing_filter_ref.replay along dirs (a dict of TANGENTS, None or absent for zero), in dtype.
    Returns (dict(Xhat_dot, innov_dot, nis_dot, loglik_dot, event_hat_dot), same (B,): the estimator's touchdown knot is the
    centre's at both offsets)."""
    L = np.dtype(dtype).type
    names = dict(Y="Y_dot", Zrec="Zrec_dot", Lgain="Lgain_dot", xhat0="xhat0_dot", model="model_dot")

    def at(s):
        rep = {}
        for name, dot in names.items():
            d = dirs.get(dot)
            a = np.asarray(rec[name]).astype(L)
            rep[name] = a if d is None else a + L(s) * np.asarray(d).astype(L).reshape(a.shape)
        return replay(batch, rec, guarded, L, **rep)

    p, c, m = at(t), at(0), at(-t)
    q = lambda x, y: ((x - y) / (2 * L(t))).astype(np.float64)  # noqa: E731
    out = dict(Xhat_dot=q(p["Xhat"], m["Xhat"]), innov_dot=q(p["innov"], m["innov"]),
               nis_dot=q(p["score"][..., 0], m["score"][..., 0]))
    # at fixed gains log det S_k does not move: loglik's quotient is that of -1/2 sum nis
    out["loglik_dot"] = q(p["loglik"], m["loglik"])
    same = np.ones(batch.B, dtype=bool)
    if guarded:
        same &= (p["events_hat"][:, 0] == c["events_hat"][:, 0]) & (m["events_hat"][:, 0] == c["events_hat"][:, 0])
        ed = np.zeros((batch.B, STRIDE))
        ed[:, 1:3] = q(p["events_hat"], m["events_hat"])[:, 1:3]
        out["event_hat_dot"] = ed
    return out, same, c
