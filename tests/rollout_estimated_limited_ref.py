"""numpy yardstick of qln_tracking_rollout_estimated_limited and its sweeps (include/qln_evaluator.h): the estimate-feedback
roll-out within contact-aware force limits.  Not a test module.

The roll-out is rollout_estimated_ref._group's loop, operation for operation, with rollout_limited_ref.clamp between the
feedback law and everything that reads the forces: Zout's u_k, the plant's guard and step and the estimator's guard and step.
The contact mode that picks the limits is the PLANT's: its _Lander's `landed` at the start of the knot (guarded), or the
handle's knot schedule.  It works in any real dtype, and with NO_LIMITS it equals rollout_estimated_ref.rollout exactly.
Besides the two guard margins of rollout_estimated_ref it returns the force margin of rollout_limited_ref.

Nothing of the derivative is restated: the sweeps are rollout_estimated_sweep_ref.sweep_jvp / sweep_vjp on blocks whose force
columns are masked by sat in both chains and in both dtau rows, with the force slots of Zout_dot / Zbar masked -- a clamped
force is a constant -- which is rollout_limited_ref's construction."""
import itertools

import numpy as np

from oracle import np_oracle as O
from tests import rollout_estimated_cases as EC
from tests import rollout_estimated_ref as ER
from tests import rollout_estimated_sweep_ref as ES
from tests import rollout_guarded_cases as GC
from tests import rollout_limited_ref as LR
from tests import rollout_ref as RR
from tests import tracking_cases as TC

NO_LIMITS, TEST_LIMITS = LR.NO_LIMITS, LR.TEST_LIMITS
STRIDE = ER.STRIDE


def _group(N, step_plant, step_hat, stands, Zref, K, Lgain, H, vnoise, wnoise, x0, xhat0, th, th_hat, lim, dt):
    """rollout_estimated_ref._group with the clamp; stands(k) -> (stand1, stand2) (B,) bool, the plant's feet at knot k's start."""
    B, ny = Zref.shape[0], H.shape[0]
    x, xh = x0.astype(dt), (Zref[:, :15] if xhat0 is None else xhat0).astype(dt)
    Zo = np.zeros((B, 20 * N - 5), dtype=dt)
    Xhat, innov = np.zeros((B, N, 15), dtype=dt), np.zeros((B, N, ny), dtype=dt)
    sat = np.zeros((B, N - 1))
    fmargin = np.full(B, np.inf, dtype=dt)
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
        s1, s2 = stands(k)
        u[:, :4], s, fm = LR.clamp(u[:, :4], s1, s2, lim)
        sat[:, k] = s @ LR.POW4
        fmargin = np.minimum(fmargin, fm)
        Zo[:, 20 * k + 15: 20 * k + 20] = u
        x = step_plant(k, x, u, th)
        if wnoise is not None:
            x = x + wnoise[:, k]
        Zo[:, 20 * (k + 1): 20 * (k + 1) + 15] = x
        xh = step_hat(k, xh, u, th_hat)
    return Zo, Xhat, innov, sat, fmargin


def rollout(N, init_mode, Zref, K, Lgain, H, x0, th, th_hat, lim, vnoise=None, wnoise=None, xhat0=None, k_trans=None,
            guarded=False, dtype=np.float64):
    """Arguments as rollout_estimated_ref.rollout, with lim (8,).  Returns its dict in `dtype`, with sat (B, N-1) float64 codes
    and fmargin (B,) added."""
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
    out = dict(Zout=np.zeros((B, 20 * N - 5), dtype=dt), Xhat=np.zeros((B, N, 15), dtype=dt), innov=np.zeros((B, N, ny), dtype=dt),
               sat=np.zeros((B, N - 1)), fmargin=np.zeros(B, dtype=dt))
    if guarded:
        out.update(events=np.zeros((B, STRIDE), dtype=dt), events_hat=np.zeros((B, STRIDE), dtype=dt),
                   margin=np.zeros(B, dtype=dt), margin_hat=np.zeros(B, dtype=dt))
    for mode, ktr in sorted({(int(m), int(t)) for m, t in zip(im, kt)}):
        i = np.flatnonzero((im == mode) & (kt == ktr))
        sub = lambda a: None if a is None else a[i]  # noqa: E731
        if guarded:
            plant, hat = ER._Lander(mode, len(i), dt), ER._Lander(mode, len(i), dt)
            steps = (plant.step, hat.step)
            # foot 1 stands in modes 1 and 3, foot 2 in modes 2 and 3: the plant's mode at the knot's start
            stands = lambda k, p=plant, m=mode: (p.landed | (m == 1), p.landed | (m == 2))  # noqa: E731
        else:
            modes, jumps = O.knot_modes(N, ktr, mode)
            one = lambda k, x, u, t: RR.model_step(int(modes[k]), bool(jumps[k]), x, u, t)  # noqa: E731
            steps = (one, one)
            stands = lambda k, n=len(i): (np.full(n, int(modes[k]) in (1, 3)), np.full(n, int(modes[k]) in (2, 3)))  # noqa: E731
        zo, xh, iv, sat, fm = _group(N, steps[0], steps[1], stands, Zref[i], sub(K), Lgain[i], H, sub(vnoise), sub(wnoise),
                                     x0[i], sub(xhat0), th[i], th_hat[i], lim, dt)
        out["Zout"][i], out["Xhat"][i], out["innov"][i], out["sat"][i], out["fmargin"][i] = zo, xh, iv, sat, fm
        if guarded:
            out["events"][i], out["events_hat"][i] = plant.ev, hat.ev
            out["margin"][i], out["margin_hat"][i] = plant.margin, hat.margin
    return out


def case_rollout(batch, inp, lim, guarded, dtype=np.float64, **replace):
    """rollout of a case's inputs (rollout_estimated_sweep_ref.case; some replaced), the handle's model TC.SECOND."""
    a = dict(inp, **replace)
    return rollout(batch.N, np.asarray(batch.init_mode), a["Zref"], a["K"], a["Lgain"], a["H"], a["x0"],
                   TC.SECOND if a["model"] is None else a["model"], TC.SECOND, lim, a["vnoise"], a["wnoise"], a["xhat0"],
                   np.asarray(batch.k_trans), guarded, dtype)


def left_out(r, margin):
    """(B,) bool: the problem is within `margin` of one of its discrete decisions -- a guard of either system, or a limit."""
    out = np.asarray(r["fmargin"], dtype=np.float64) < margin
    if "margin" in r:
        out |= (np.asarray(r["margin"], dtype=np.float64) < margin) | (np.asarray(r["margin_hat"], dtype=np.float64) < margin)
    return out


def mask_chain_blocks(blk, sat, events=None, events_hat=None):
    """chain_blocks' dict with the force columns of the saturated channels set to zero: in both chains' blocks, and in each
    chain's dtau row by the code of that chain's own touchdown knot."""
    out = dict(blk, Fp=LR.mask_blocks(blk["Fp"], sat), Fe=LR.mask_blocks(blk["Fe"], sat))
    free = LR.free_channels(sat)
    for name, ev in (("Tp", events), ("Te", events_hat)):
        T = np.array(blk[name])
        if ev is not None:
            for b in range(len(T)):
                ks = int(ev[b, 0])
                if 0 <= ks < free.shape[1]:
                    T[b, 15:19] = np.where(free[b, ks], T[b, 15:19], 0)
        out[name] = T
    return out


def sweep_jvp(blk, sat, Zref, K, Lgain, H, Zout, Xhat, innov, events=None, events_hat=None, **tangents):
    """The forward sweep at fixed active set: rollout_estimated_sweep_ref.sweep_jvp on the masked blocks, dF's slots masked."""
    r = ES.sweep_jvp(mask_chain_blocks(blk, sat, events, events_hat), Zref, K, Lgain, H, Zout, Xhat, innov, events=events,
                     events_hat=events_hat, **tangents)
    r["Zout_dot"] = LR.mask_forces(r["Zout_dot"], sat)
    return r


def sweep_vjp(blk, sat, Zref, K, Lgain, H, Zout, Xhat, innov, Zbar, Xhat_bar=None, innov_bar=None, with_xhat0=True):
    """The reverse sweep at fixed active set: rollout_estimated_sweep_ref.sweep_vjp on the masked blocks with the saturated
    channels' slots of Zbar masked (their ubar goes nowhere)."""
    return ES.sweep_vjp(mask_chain_blocks(blk, sat), Zref, K, Lgain, H, Zout, Xhat, innov, LR.mask_forces(Zbar, sat), Xhat_bar,
                        innov_bar, with_xhat0)


def central_difference(batch, inp, lim, guarded, dirs, t=1e-6):
    """Longdouble central differences of the roll-out along dirs, as rollout_estimated_sweep_ref.central_difference.  Returns
    (dict of the tangents of the outputs, same (B,): both touchdown knots and every saturation code are the centre's at both
    offsets)."""
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
        return case_rollout(batch, inp, lim, guarded, L, **rep)

    p, c, m = at(t), at(0), at(-t)
    q = lambda n: ((p[n] - m[n]) / (2 * L(t))).astype(np.float64)  # noqa: E731
    out = dict(Zout_dot=q("Zout"), Xhat_dot=q("Xhat"), innov_dot=q("innov"))
    same = np.all(p["sat"] == c["sat"], axis=1) & np.all(m["sat"] == c["sat"], axis=1)
    if guarded:
        for rec, dot in (("events", "event_dot"), ("events_hat", "event_hat_dot")):
            same &= (p[rec][:, 0] == c[rec][:, 0]) & (m[rec][:, 0] == c[rec][:, 0])
            ed = np.zeros((batch.B, STRIDE))
            ed[:, 1:3] = q(rec)[:, 1:3]
            out[dot] = ed
    return out, same, c


# ---- what the CPU and the GPU tests share: the cases, so that the seeds checked on the CPU are the ones the GPU runs ----------
NYS = EC.NYS
FLAGS = list(itertools.product((False, True), repeat=4))  # with K, model, wnoise, xhat0
SCHEDULED = [s for s in TC.SHAPES if s[1] in (2, 3, 40, 61)] + [(70, 12, 5, 0)]  # (B, N, k_trans, init_mode); the last is ragged
GUARDED = [("shape",) + s for s in GC.SHAPES] + [("ragged", 12, 0, 70)]      # (kind, N, init_mode, B)
MARGIN, LEFT_OUT = GC.MARGIN, GC.LEFT_OUT
FORCE_PUSH = np.array([5.0, 200.0, 5.0, 200.0])  # N, on (F1x, F1y, F2x, F2y): see scheduled_case


def call_inputs(seed, B, N, ny, Zref, flags, th_all):
    """Host inputs of one call: K = 0.05 N(0, 1), filter gains and noise of rollout_estimated_cases.draws."""
    wk, wm, ww, wx = flags
    d = EC.draws(seed, B, N, ny)
    rng = np.random.default_rng(seed + 1)
    return dict(K=0.05 * rng.normal(size=(B, N - 1, 4, 15)) if wk else None, model=th_all if wm else None, Lgain=d["Lgain"],
                H=d["H"], vnoise=d["vnoise"], wnoise=d["wnoise"] if ww else None, xhat0=Zref[:, :15] + d["dxhat0"] if wx else None)


def scheduled_case(B, N, k_trans, init_mode):
    """(batch, Zref, x0, th_all, seed) of a knot-scheduled case; init_mode 0: the ragged batch of two blocks.
    The reference is problem_gen's, except that at knot 0 -- the one knot every shape has -- the last problem's reference asks for
    FORCE_PUSH less and the one before it for FORCE_PUSH more on every channel, as rollout_guarded_cases.case gives its last
    problem a reference of its own.  The generator's forces sit near the plan's (a standing foot's F_y around half the weight)
    and K = 0.05 N(0, 1) on deviations of 1e-2 moves them by 2e-3 N, so without this a shape with one knot and three problems
    rides no upper limit under TEST_LIMITS (and one of them no limit at all) and would pass with no clamp active.  FORCE_PUSH
    is four times the widest pair of TEST_LIMITS (49.55 N in F_y, 0.8 N in F_x) and more than any force of the generator's plans
    (|F_x| < 1 N, |F_y| < 100 N: asserted below), so whatever the foot's contact state the one problem is below every lower limit and the other above every
    upper one: each case holds codes 1, 2 and 0.  One knot of 0.01 to 0.02 s at a capped force does not move the loop's size."""
    batch = TC.batch(B, N, k_trans, 1, seed=3, ragged=True) if init_mode == 0 else TC.batch(B, N, k_trans, init_mode, seed=N + k_trans)
    Zref = np.array(batch.Z, dtype=np.float64)  # a copy: the batch keeps the generator's plan
    assert (np.abs(Zref[:, 15:19]) < np.array([1.0, 100.0, 1.0, 100.0])).all()
    Zref[B - 1, 15:19] -= FORCE_PUSH
    Zref[B - 2, 15:19] += FORCE_PUSH
    seed = 100 * N + 10 * int(batch.k_trans[0]) + int(batch.init_mode[0])
    x0 = Zref[:, :15] + 1e-2 * np.random.default_rng(seed).normal(size=(B, 15))
    return batch, Zref, x0, RR.draw_models(B, seed + 2, TC.SECOND), seed


def guarded_case(kind, N, im, B):
    """(batch, Zref, x0, th_all, seed) of a guarded case: rollout_guarded_cases.case, or its ragged case."""
    if kind == "ragged":
        batch, Zref, _, x0, th = GC.ragged_case(B=B, N=N)
        return batch, Zref, x0, th, 3
    batch, Zref, _, x0, th = GC.case(N, im, B, True, True)
    return batch, Zref, x0, th, GC.seed_of(N, im, True, True)


def call_rollout(batch, Zref, inp, x0, lim, guarded, dtype=np.float64):
    """The yardstick on a call's inputs, the handle's model TC.SECOND."""
    return rollout(batch.N, np.asarray(batch.init_mode), Zref, inp["K"], inp["Lgain"], inp["H"], x0,
                   TC.SECOND if inp["model"] is None else inp["model"], TC.SECOND, lim, inp["vnoise"], inp["wnoise"], inp["xhat0"],
                   np.asarray(batch.k_trans), guarded, dtype)


def digit_shares(sat):
    """The shares of (knot, channel) pairs that are free, on the lower and on the upper limit."""
    s = LR.unpack(sat)
    return tuple(float((s == v).mean()) for v in (0, 1, 2))
