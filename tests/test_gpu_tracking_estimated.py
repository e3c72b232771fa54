"""qln_tracking_rollout_estimated / qln_tracking_rollout_estimated_guarded on the GPU: the plant and the estimator rolled out
together, the forces fed back from the estimate (include/qln_evaluator.h).  The yardstick is tests/rollout_estimated_ref.py,
held on the CPU by tests/test_rollout_estimated_host.py.  Besides it the kernel is held without an oracle: with Lgain = 0 it is
bit for bit the roll-out it is built from, three sensor rows are bit for bit eight rows with zero rows and columns written out,
every subset of optional outputs has the bits of the full call, and the host forms have the bits of the device forms.  And the
whole pipeline -- solve, nominal roll-out, gains, filter, the sampled loop -- is set against the covariances it predicts."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import estimation_cases as EF
from tests import rollout_estimated_cases as EC
from tests import rollout_estimated_ref as ER
from tests import rollout_guarded_cases as GC
from tests import rollout_ref as RR
from tests import tracking_cases as TC

pytestmark = pytest.mark.gpu
_time_limit = EF.time_limit(600)

BAR = 1e-10  # the family's bar (tests/test_gpu_tracking.py, tests/test_gpu_rollout_guarded.py)
SHAPES = [s for s in TC.SHAPES if s[1] in (2, 3, 40, 61)]
FLAGS = list(itertools.product((False, True), repeat=4))  # with K, model, wnoise, xhat0


def _inputs(seed, B, N, ny, Zref, flags, th_all):
    """Host inputs of one call: random gains, filter gains and noise (tests/rollout_estimated_cases.draws)."""
    wk, wm, ww, wx = flags
    d = EC.draws(seed, B, N, ny)
    rng = np.random.default_rng(seed + 1)
    return dict(K=0.05 * rng.normal(size=(B, N - 1, 4, 15)) if wk else None, model=th_all if wm else None, Lgain=d["Lgain"], H=d["H"],
                vnoise=d["vnoise"], wnoise=d["wnoise"] if ww else None, xhat0=Zref[:, :15] + d["dxhat0"] if wx else None)


def _call(nlp, Zref_d, inp, x0, guarded, **kw):
    return nlp.tracking_rollout_estimated(Zref_d, EF.dev(inp["K"]), EF.dev(inp["Lgain"]), inp["H"], EF.dev(inp["vnoise"]), EF.dev(inp["wnoise"]),
                                          EF.dev(x0), EF.dev(inp["xhat0"]), EF.dev(inp["model"]), guarded=guarded, with_innovations=True, **kw)


def _yardstick(nlp, Zref, inp, x0, guarded):
    th_hat = np.array(nlp.model.plant_parameters())
    return ER.rollout(nlp.N, nlp.init_mode, Zref, inp["K"], inp["Lgain"], inp["H"], x0, th_hat if inp["model"] is None else inp["model"],
                      th_hat, inp["vnoise"], inp["wnoise"], inp["xhat0"], nlp.k_trans, guarded)


def _errors(nlp, got, ref, keep=None):
    keep = slice(None) if keep is None else keep
    names = ("Zout", "Xhat", "innov") + (("events", "events_hat") if len(got) > 3 else ())
    host = [TC.rows(nlp, got[0])] + [t.cpu().numpy() for t in got[1:]]
    return {n: RR.rel(h[keep], ref[n][keep]) for n, h in zip(names, host)}


# ---- 1. against the yardstick --------------------------------------------------------------------------------------------
def _check_scheduled(batch, tag, **kw):
    nlp = TC.nlp(batch, TC.SECOND_MODEL, **kw)
    B, N = nlp.B, nlp.N
    Zref = np.ascontiguousarray(batch.Z, dtype=np.float64)
    Zref_d = nlp.upload_Z(batch.Z)
    seed = 100 * N + 10 * int(nlp.k_trans[0]) + int(nlp.init_mode[0])
    x0 = Zref[:, :15] + 1e-2 * np.random.default_rng(seed).normal(size=(B, 15))
    th_all = RR.draw_models(B, seed + 2, TC.SECOND)
    worst = {}
    for ny in EC.NYS:
        for flags in FLAGS:
            inp = _inputs(seed + ny, B, N, ny, Zref, flags, th_all)
            got = _call(nlp, Zref_d, inp, x0, False)
            assert got[1].shape == (B, N, 15) and got[2].shape == (B, N, ny)
            for n, e in _errors(nlp, got, _yardstick(nlp, Zref, inp, x0, False)).items():
                worst[n] = max(worst.get(n, 0.0), e)
    print(f"estimated {tag}: worst over ny in {EC.NYS} and the 16 combinations of K, model, wnoise, xhat0: " +
          ", ".join(f"{n} {e:.2e}" for n, e in worst.items()))
    assert all(e <= BAR for e in worst.values()), worst


@pytest.mark.parametrize("B,N,k_trans,init_mode", SHAPES)
def test_knot_scheduled_form_matches_the_yardstick(B, N, k_trans, init_mode):
    """Zout, Xhat and innov in rollout_ref.rel, within 1e-10, on random gains, filter gains and noise.  Measured worst values:
    profiles/tracking_estimated_tests.txt."""
    _check_scheduled(TC.batch(B, N, k_trans, init_mode, seed=N + k_trans), f"B={B} N={N} k_trans={k_trans} mode={init_mode}")


def test_knot_scheduled_form_on_a_ragged_batch_with_a_padded_stride():
    """Two blocks, per-problem k_trans and init_mode, z_stride beyond n_nlp: the padding is never written."""
    import torch

    N, B = 12, 70
    batch = TC.batch(B, N, 5, 1, seed=3, ragged=True)
    _check_scheduled(batch, f"ragged B={B} N={N} z_stride={20 * N + 3}", z_stride=20 * N + 3)
    nlp = TC.nlp(batch, TC.SECOND_MODEL, z_stride=20 * N + 3)
    inp = _inputs(1, B, N, 3, np.asarray(batch.Z, dtype=np.float64), (True, False, True, False), None)
    out = torch.full((nlp.dims.z_total,), 7.0, dtype=torch.float64, device="cuda")
    _call(nlp, nlp.upload_Z(batch.Z), inp, None, False, out=out)
    assert bool((out.view(B, -1)[:, nlp.n_nlp:] == 7.0).all()) and not bool((out.view(B, -1)[:, :nlp.n_nlp] == 7.0).any())


def _guarded_case(kind, N, im, B):
    if kind == "ragged":
        batch, Zref, _, x0, th = GC.ragged_case()
        return batch, Zref, x0, th, 3
    batch, Zref, _, x0, th = GC.case(N, im, B, True, True)
    return batch, Zref, x0, th, GC.seed_of(N, im, True, True)


@pytest.mark.parametrize("kind,N,im,B", [("shape",) + s for s in GC.SHAPES] + [("ragged", 12, 0, 70)])
def test_guarded_form_matches_the_yardstick(kind, N, im, B):
    """The same with both event records.  A problem whose plant or estimator is closer than MARGIN to one of its guard's
    boundaries is left out -- at most LEFT_OUT of a case, checked on the yardstick before the GPU is asked."""
    batch, Zref, x0, th_all, seed = _guarded_case(kind, N, im, B)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Zref_d = nlp.upload_Z(Zref)
    worst, left = {}, 0
    for ny in EC.NYS:
        for flags in FLAGS:
            inp = _inputs(seed + ny, B, N, ny, Zref, flags, th_all)
            ref = _yardstick(nlp, Zref, inp, x0, True)
            keep = np.minimum(ref["margin"], ref["margin_hat"]) >= GC.MARGIN
            assert keep.mean() >= 1 - GC.LEFT_OUT, (ny, flags, int((~keep).sum()))
            left = max(left, int((~keep).sum()))
            got = _call(nlp, Zref_d, inp, x0, True)
            for n, e in _errors(nlp, got, ref, keep).items():
                worst[n] = max(worst.get(n, 0.0), e)
            assert (ref["events"][:, 0] >= 0).any()
    print(f"estimated guarded {kind} N={N} mode={im} B={B}: worst over ny and the 16 combinations: " +
          ", ".join(f"{n} {e:.2e}" for n, e in worst.items()) + f"; at most {left} problems left out of a call")
    assert all(e <= BAR for e in worst.values()), worst


# ---- 2. reductions, exact in every value ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,k_trans,init_mode", [SHAPES[1], SHAPES[4], SHAPES[6], SHAPES[12]])
def test_without_filter_gains_the_call_is_the_model_roll_out(B, N, k_trans, init_mode):
    """Lgain = 0, xhat0 None and Zref a trajectory of the handle's model: the estimate stays on Zref, so whatever K is, Zout has
    the bits of tracking_rollout_model(Zref, None, x0, model)."""
    import torch

    batch = TC.batch(B, N, k_trans, init_mode, seed=N)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Zref_d = nlp.tracking_rollout_model(nlp.upload_Z(batch.Z), None, None, None)
    Zref = TC.rows(nlp, Zref_d)
    rng = np.random.default_rng(N)
    x0 = EF.dev(Zref[:, :15] + 1e-2 * rng.normal(size=(B, 15)))
    for ny, wm in ((8, True), (3, False)):
        model = EF.dev(RR.draw_models(B, N, TC.SECOND)) if wm else None
        d = EC.draws(N, B, N, ny)
        Zout, Xhat, innov = nlp.tracking_rollout_estimated(Zref_d, TC.gains(nlp, N), EF.dev(np.zeros_like(d["Lgain"])), d["H"],
                                                           EF.dev(d["vnoise"]), None, x0, None, model, with_innovations=True)
        assert torch.equal(Zout, nlp.tracking_rollout_model(Zref_d, None, x0, model))
        assert np.array_equal(Xhat.cpu().numpy(), np.concatenate([Zref, np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15])
        assert bool(innov.any())


@pytest.mark.parametrize("N,im,B", [GC.SHAPES[2], GC.SHAPES[4], GC.SHAPES[6]])
def test_without_filter_gains_the_guarded_call_is_the_guarded_roll_out(N, im, B):
    import torch

    batch, Zref, _, x0, th = GC.case(N, im, B, True, True)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Zref_d, ev_ref = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), None, None, None)
    for ny, wm in ((8, True), (1, False)):
        model = EF.dev(th) if wm else None
        d = EC.draws(N, B, N, ny)
        Zout, _, _, ev, evh = nlp.tracking_rollout_estimated(Zref_d, TC.gains(nlp, N), EF.dev(np.zeros_like(d["Lgain"])), d["H"],
                                                             EF.dev(d["vnoise"]), None, EF.dev(x0), None, model, guarded=True)
        Zg, evg = nlp.tracking_rollout_guarded(Zref_d, None, EF.dev(x0), model)
        assert torch.equal(Zout, Zg) and torch.equal(ev, evg)
        assert torch.equal(evh, ev_ref)  # the estimator flies the reference's own landing
    assert bool((ev_ref[:, 0] >= 0).any())


@pytest.mark.parametrize("guarded", [False, True])
def test_three_rows_are_eight_rows_with_zero_rows_and_columns(guarded):
    import torch

    N, im, B = 40, 1, 9
    batch, Zref, K, x0, th = GC.case(N, im, B, True, True)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    inp = _inputs(5, B, N, 3, Zref, (True, True, True, True), th)
    inp["K"] = K
    big = dict(inp)
    big["H"], big["Lgain"], big["vnoise"] = np.zeros((8, 15)), np.zeros((B, N, 15, 8)), np.random.default_rng(1).normal(size=(B, N, 8))
    big["H"][:3], big["Lgain"][..., :3], big["vnoise"][..., :3] = inp["H"], inp["Lgain"], inp["vnoise"]
    Zref_d = nlp.upload_Z(Zref)
    a, b = _call(nlp, Zref_d, inp, x0, guarded), _call(nlp, Zref_d, big, x0, guarded)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2][..., :3])
    for p, q in zip(a[3:], b[3:]):
        assert torch.equal(p, q)


@pytest.mark.parametrize("guarded", [False, True])
def test_every_subset_of_optional_outputs_has_the_bits_of_the_full_call(guarded):
    import torch

    N, im, B = 8, 1, 48
    batch, Zref, K, x0, th = GC.case(N, im, B, True, True)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    inp = _inputs(6, B, N, 3, Zref, (True, True, True, True), th)
    Zref_d = nlp.upload_Z(Zref)
    full = _call(nlp, Zref_d, inp, x0, guarded)
    for we, wi, wv in itertools.product((False, True), repeat=3):
        if guarded or wv:
            part = nlp.tracking_rollout_estimated(Zref_d, EF.dev(inp["K"]), EF.dev(inp["Lgain"]), inp["H"], EF.dev(inp["vnoise"]),
                                                  EF.dev(inp["wnoise"]), EF.dev(x0), EF.dev(inp["xhat0"]), EF.dev(inp["model"]), guarded=guarded,
                                                  with_estimate=we, with_innovations=wi, with_events=wv)
            assert torch.equal(part[0], full[0])
            for p, f, asked in zip(part[1:], full[1:], (we, wi, wv, wv)):
                assert (p is None and not asked) or torch.equal(p, f)
    if guarded:  # one record without the other
        from quadruped_landing_amd import _lib

        ev = torch.zeros_like(full[3])
        out = torch.zeros_like(full[0])
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        t = {n: EF.dev(inp[n]) for n in ("K", "Lgain", "H", "vnoise", "wnoise", "xhat0", "model")}  # alive through the calls
        t["x0"] = EF.dev(x0)
        args = [p(t["K"]), p(t["Lgain"]), p(t["H"]), 3] + [p(t[n]) for n in ("vnoise", "wnoise", "x0", "xhat0", "model")]
        for which in (0, 1):
            recs = [None, None]
            recs[which] = p(ev)
            _lib.check(_lib.lib().qln_tracking_rollout_estimated_guarded(nlp._h, p(Zref_d), *args, p(out), None, None, *recs))
            assert torch.equal(out, full[0]) and torch.equal(ev, full[3 + which])


@pytest.mark.parametrize("B", [5, 1024])  # mapped pinned buffers (small batch) and staged device copies
def test_host_forms_give_the_device_forms_bits_after_other_host_calls_left_nans_behind(B):
    N = 12
    batch, Zref, K, x0, th = GC.ragged_case(B=B, N=N)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Zref_d = nlp.upload_Z(Zref)
    zr = Zref_d.cpu().numpy()
    nan = lambda *s: np.full(s, np.nan)  # noqa: E731
    for ny, guarded in ((3, False), (8, True), (1, True)):
        inp = _inputs(B + ny, B, N, ny, Zref, (True, True, True, True), th)
        inp["K"] = K
        with np.errstate(all="ignore"):  # the roles this call reads and writes now hold NaN
            nlp.tracking_rollout_estimated_host(nan(*zr.shape), nan(*K.shape), nan(B, N, 15, 8), np.ones((8, 15)), nan(B, N, 8),
                                                nan(B, N - 1, 15), nan(B, 15), nan(B, 15), None, guarded=True, with_innovations=True)
        dev = _call(nlp, Zref_d, inp, x0, guarded)
        for _ in range(2):
            host = nlp.tracking_rollout_estimated_host(zr, inp["K"], inp["Lgain"], inp["H"], inp["vnoise"], inp["wnoise"], x0,
                                                       inp["xhat0"], inp["model"], guarded=guarded, with_innovations=True)
            for d, h in zip(dev, host):
                assert np.array_equal(h.reshape(-1), d.cpu().numpy().reshape(-1))
        part = nlp.tracking_rollout_estimated_host(zr, None, inp["Lgain"], inp["H"], guarded=guarded, with_estimate=False)
        assert part[1] is None and part[2] is None and np.isfinite(part[0]).all()


# ---- 3. the sampled loop against the predicted covariances ---------------------------------------------------------------
@pytest.mark.parametrize("guarded", [False, True])
def test_monte_carlo_of_4096_noisy_landings_through_the_library(guarded):
    """tests/test_rollout_estimated_host.py's two experiments through the library at S = 4 096: solve, the nominal roll-out,
    tracking_lqr / _guarded, tracking_kalman / _guarded, then the estimate-feedback roll-out under drawn noise.  At every knot
    and along 32 directions each, the sample variances of the true state's deviation, of the estimation error Zout - Xhat and
    of the innovation over the predicted X_k, P^+_k and S_k lie within 1 +- 5 sqrt(2 / (S - 1)); guarded, so does the plant's
    touchdown clock over event_var[1].  The prediction is made at a fixed touchdown knot: it applies to the samples whose plant
    and estimator land in the nominal's knot, and the test asserts that for this seed that is all of them."""
    import torch

    from quadruped_landing_amd import nlp as NL, problem_gen as PG

    S = EC.MC_S
    sd, W, seed = EC.MC_SETTINGS[0]
    nb = PG.notebook_problem()
    N = nb.N
    one, many = EC.handle_pair(nb, S)
    Zs = one.upload_Z(nb.Z)
    one.solve(Zs)
    H, V = EC.sensors(), np.full(8, sd * sd)
    S0, dx0, v, w, Wx, Wy = EC.mc_draws(seed, N, sd, W)
    x0 = nb.x0.reshape(1, 15).copy()
    if guarded:
        x0[0, 6] += EC.MC_HEIGHT
        Zn, ev = one.tracking_rollout_guarded(Zs, None, EF.dev(x0))
        K, _ = one.tracking_lqr_guarded(Zn, ev, EC.Q, EC.R, EC.Q, with_cost_to_go=False)
        L, Pe, Sig, _, var = one.tracking_kalman_guarded(Zn, ev, H, V, K, S0, W, with_marginals=False)
    else:
        Zn = one.tracking_rollout(Zs, None, EF.dev(x0))
        K, _ = one.tracking_lqr(Zn, EC.Q, EC.R, EC.Q, with_cost_to_go=False)
        L, Pe, Sig, _ = one.tracking_kalman(Zn, H, V, K, S0, W, with_marginals=False)
    zn = TC.rows(one, Zn)[0]
    Pp, X, Lh = NL.unpack_covariance(Pe)[0], NL.unpack_covariance(Sig)[0], L.cpu().numpy()[0]
    # P^+ = (I - L H) P^-: the prior, and with it S_k = H P^-_k H' + V, from what the call returns
    Pm = np.linalg.solve(np.eye(15) - Lh @ H, Pp)
    tile = lambda t: t.expand(S, *t.shape[1:]).contiguous()  # noqa: E731
    got = many.tracking_rollout_estimated(many.upload_Z(np.tile(zn, (S, 1))), tile(K), tile(L), H, EF.dev(v), EF.dev(w), EF.dev(x0 + dx0),
                                          guarded=guarded, with_innovations=True)
    torch.cuda.synchronize()
    zo, xh, iv = TC.rows(many, got[0]), got[1].cpu().numpy(), got[2].cpu().numpy()
    assert np.isfinite(zo).all() and np.isfinite(xh).all()
    worst = EC.mc_worst(zo, xh, iv, zn, X, Pp, EC.innovation_covariances(Pm, H, V), Wx, Wy)
    print(f"Monte Carlo through the library, guarded={guarded}, S={S}, sensor sd {sd:.0e}: worst |ratio - 1| X {worst['X']:.4f}, "
          f"P+ {worst['P+']:.4f}, S {worst['S']:.4f}; band {EC.band():.4f}")
    if guarded:
        evn, evp, evh = ev.cpu().numpy()[0], got[3].cpu().numpy(), got[4].cpu().numpy()
        differing = float(np.mean(evp[:, 0] != evh[:, 0]))
        clock = float(np.var(evp[:, 2], ddof=1) / var.cpu().numpy()[0, 1])
        print(f"  nominal touchdown in knot {evn[0]:.0f} at tau / h = {evn[1] / zn[20 * int(evn[0]) + 19]:.2f}; plant and estimator "
              f"land in different knots in {differing:.4f} of the samples; touchdown-clock variance over event_var[1]: {clock:.4f}")
        # the prediction holds the touchdown knot fixed: it says nothing of a sample that lands elsewhere
        assert differing == 0.0 and (evp[:, 0] == evn[0]).all(), "the fixed-knot prediction does not apply to these samples"
        assert abs(clock - 1.0) <= EC.band(), clock
    assert max(worst.values()) <= EC.band(), worst


# ---- 4. refusals and one full-size run -----------------------------------------------------------------------------------
def test_invalid_arguments_are_refused():
    import torch

    from quadruped_landing_amd import _lib

    N, im, B = 5, 2, 32
    batch, Zref, K, x0, th = GC.case(N, im, B, True, True)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    L, h, INV, OK = _lib.lib(), nlp._h, _lib.QLN_ERR_INVALID_ARGUMENT, _lib.QLN_OK
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    Zr, Kd, Lg, Hd, vn, wn = nlp.upload_Z(Zref), EF.dev(K), f64(B, N, 15, 8), f64(8, 15), f64(B, N, 8), f64(B, N - 1, 15)
    xd, xh, md = EF.dev(x0), EF.dev(x0), EF.dev(th)
    Zo, Xo, Io, ev, eh = nlp.new_Z(), f64(B, N, 15), f64(B, N, 8), f64(B, 8), f64(B, 8)
    est, gst = L.qln_tracking_rollout_estimated, L.qln_tracking_rollout_estimated_guarded

    def call(fn=est, Zref=Zr, K=Kd, Lgain=Lg, H=Hd, ny=8, v=vn, w=wn, x0=xd, xhat0=xh, model=md, Zout=Zo, Xhat=Xo, innov=Io, tail=()):
        return fn(h, p(Zref), p(K), p(Lgain), p(H), ny, p(v), p(w), p(x0), p(xhat0), p(model), p(Zout), p(Xhat), p(innov), *tail)

    assert call() == OK and call(tail=(p(ev), p(eh)), fn=gst) == OK
    assert call(K=None, v=None, w=None, x0=None, xhat0=None, model=None, Xhat=None, innov=None) == OK
    for ny in (0, 9):
        assert call(ny=ny) == INV and b"ny must be" in L.qln_last_error()
    for name in ("Zref", "Zout", "Lgain", "H"):
        assert call(**{name: None}) == INV and b"null" in L.qln_last_error(), name
    # overlaps: every output against an input, and against another output
    assert call(Zout=Zr) == INV and b"overlaps" in L.qln_last_error()
    assert call(Xhat=Lg) == INV and call(innov=vn) == INV and call(Xhat=wn) == INV and call(innov=Hd) == INV
    assert call(Xhat=xd) == INV and call(innov=xh) == INV and call(Xhat=md) == INV and call(Zout=Kd) == INV
    assert call(innov=Xo) == INV and b"two outputs" in L.qln_last_error()
    assert call(Xhat=Zo) == INV
    assert call(fn=gst, tail=(p(ev), p(ev))) == INV and call(fn=gst, tail=(p(Xo), None)) == INV
    assert call(fn=gst, tail=(None, p(md))) == INV
    torch.cuda.synchronize()
    # host forms: the same, the values of H and of the models
    a = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    zr, zo, Lh, Hh = Zr.cpu().numpy(), np.zeros(nlp.dims.z_total), np.zeros((B, N, 15, 8)), np.zeros((8, 15))
    hst, hgs = L.qln_tracking_rollout_estimated_host, L.qln_tracking_rollout_estimated_guarded_host

    def hcall(fn=hst, H=Hh, ny=8, model=th, Lgain=Lh, tail=()):
        return fn(h, a(zr), a(K), a(Lgain), a(H), ny, None, None, a(x0), None, a(model), a(zo), None, None, *tail)

    assert hcall() == OK and hcall(fn=hgs, tail=(None, None)) == OK
    assert hcall(ny=9) == INV and hcall(Lgain=None) == INV and hcall(H=None) == INV
    for value in (np.nan, np.inf):
        bad = Hh.copy()
        bad[7, 14] = value
        assert hcall(H=bad) == INV and b"H is not finite" in L.qln_last_error()
        assert hcall(H=bad, ny=7) == OK  # behind ny: not read
        assert hcall(fn=hgs, H=bad, tail=(None, None)) == INV
    for entry, value in ((0, np.nan), (1, 0.0), (3, np.inf)):
        bad = np.array(th)
        bad[3, entry] = value
        assert hcall(model=bad) == INV and hcall(fn=hgs, model=bad, tail=(None, None)) == INV, (entry, value)
    # the Python layer refuses a malformed H and a missing Lgain before any call
    with pytest.raises(ValueError):
        nlp.tracking_rollout_estimated(Zr, Kd, Lg, np.ones((9, 15)))
    with pytest.raises(ValueError):
        nlp.tracking_rollout_estimated(Zr, Kd, None, np.ones((8, 15)))


def test_full_size_every_problem():
    """B = 65 536, N = 40, every input and output, one launch; every problem against the yardstick, in chunks.  ny = 3 keeps
    the drawn filter gains under a gigabyte; the kernel's path does not depend on ny."""
    from quadruped_landing_amd import problem_gen as PG

    B, N, ny, chunk = 65536, 40, 3, 8192
    batch = PG.make_batch(B, N, 14, 1, seed=2)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Zref = np.ascontiguousarray(batch.Z, dtype=np.float64)
    x0 = Zref[:, :15] + 1e-2 * np.random.default_rng(2).normal(size=(B, 15))
    inp = _inputs(3, B, N, ny, Zref, (True, True, True, True), RR.draw_models(B, 4, TC.SECOND))
    got = _call(nlp, nlp.upload_Z(batch.Z), inp, x0, False)
    host = dict(Zout=TC.rows(nlp, got[0]), Xhat=got[1].cpu().numpy(), innov=got[2].cpu().numpy())
    th_hat = np.array(nlp.model.plant_parameters())
    worst = dict.fromkeys(host, 0.0)
    for s in range(0, B, chunk):
        c = slice(s, s + chunk)
        ref = ER.rollout(N, nlp.init_mode[c], Zref[c], inp["K"][c], inp["Lgain"][c], inp["H"], x0[c], inp["model"][c], th_hat,
                         inp["vnoise"][c], inp["wnoise"][c], inp["xhat0"][c], nlp.k_trans[c])
        for n in host:
            worst[n] = max(worst[n], RR.rel(host[n][c], ref[n]))
    print(f"estimated full size B={B} N={N} ny={ny}: " + ", ".join(f"{n} {e:.2e}" for n, e in worst.items()))
    assert all(e <= BAR for e in worst.values()), worst
