"""qln_tracking_lqr_guarded / qln_tracking_covariance_guarded on the GPU: TVLQR gains and covariances through the guard-triggered
touchdown (include/qln_evaluator.h).  The yardstick is tests/tracking_guarded_ref.py -- tracking_ref.riccati and
tracking_cov_ref.propagate on the complex-step blocks of tests/rollout_guarded_sweep_ref.py -- held on the CPU by
tests/test_tracking_guarded_host.py.  Besides it the kernels are held without an oracle to the guarded sweeps' own kernels,
and bit for bit to qln_tracking_lqr / qln_tracking_covariance where no problem lands.  The cases and their seeds are
tests/rollout_guarded_cases.py's."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import estimation_cases as EF
from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_sweep_ref as SR
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR
from tests import tracking_guarded_ref as TG

pytestmark = pytest.mark.gpu
_time_limit = EF.time_limit(600)

BAR = 1e-10  # the unguarded tests' bar (tests/test_gpu_tracking.py, tests/test_gpu_tracking_cov.py)
# The two comparisons between the GPU's own kernels: ten times what the same comparisons leave in numpy
# (tests/test_tracking_guarded_host.py, the same cases: 8.15e-15 of the LQ cost, 1.46e-14 of the quadratic form).  Measured on
# the GPU: 1.2e-14 and 1.22e-13 (N = 61 with gains: sixty knots of closed loop under random gains).
COST_BAR = 10 * 8.15e-15
DUALITY_BAR = 10 * 1.46e-14

SHAPE_CASES = [("shape", N, im, B, wg) for (N, im, B) in GC.SHAPES for wg in (False, True)]
CASES = SHAPE_CASES + [("ragged", 12, 0, 70, True), ("tau0", 5, 1, 3, False), ("tau0", 5, 2, 3, False)]


def _inputs(kind, N, im, B, wg):
    """with gains: feedback and per-problem models; without: open loop at the handle's model (model == NULL)"""
    if kind == "shape":
        batch, Zref, K, x0, th = GC.case(N, im, B, wg, wg)
        return batch, Zref, K, x0, th, im, wg
    if kind == "ragged":
        batch, Zref, K, x0, th = GC.ragged_case()
        return batch, Zref, K, x0, th, np.asarray(batch.init_mode), True
    batch, Zref, x0, th = GC.tau_zero_case(N, im)
    return batch, Zref, None, x0, th, im, False


@functools.lru_cache(maxsize=None)
def _run(kind, N, im, B, wg):
    """One case: the GPU's guarded roll-out, the yardstick's blocks at the GPU's own Zout and events, the yardstick's gains
    and covariances on them and its own float64-to-longdouble distance, and the GPU's.  Shared by the tests of the case;
    nothing here is changed afterwards."""
    from quadruped_landing_amd import nlp as NL

    batch, Zref, K, x0, th, ims, wm = _inputs(kind, N, im, B, wg)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    dev = dict(Zref=nlp.upload_Z(Zref), K=EF.dev(K), x0=EF.dev(x0), model=EF.dev(th) if wm else None)
    Zout, ev = nlp.tracking_rollout_guarded(dev["Zref"], dev["K"], dev["x0"], dev["model"])
    zo, evh = TC.rows(nlp, Zout), ev.cpu().numpy()
    rng = np.random.default_rng(GC.seed_of(N, im, wg, wm) + 41)
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    F, T = SR.blocks(N, ims, zo, th, evh)
    Kr, Pr = TG.riccati(F, TC.QW, TC.R, TC.QFW)
    Sr, mr, vr = TG.covariance(F, T, evh, K, S0, W, zo[:, 2::20], th[:, 3])
    dist = TG.distances(N, ims, zo, th, evh, K, TC.QW, TC.R, TC.QFW, S0, W)
    dev.update(Zout=Zout, ev=ev)
    Kg, Pg = nlp.tracking_lqr_guarded(Zout, ev, TC.QW, TC.R, TC.QFW, dev["model"])
    Sg, mg, vg = nlp.tracking_covariance_guarded(Zout, ev, dev["K"], S0, W, dev["model"])
    got = dict(K=Kg, P=Pg, S=Sg, marg=mg, var=vg, Kh=Kg.cpu().numpy(), Ph=NL.unpack_cost_to_go(Pg), Sh=NL.unpack_covariance(Sg),
               margh=mg.cpu().numpy(), varh=vg.cpu().numpy())
    host = dict(Zref=Zref, K=K, x0=x0, th=th, Zout=zo, ev=evh, S0=S0, W=W, F=F, T=T, Kr=Kr, Pr=Pr, Sr=Sr, mr=mr, vr=vr)
    return nlp, dev, host, got, dist


# ---- 1. against the yardstick --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,im,B,wg", CASES)
def test_gains_and_covariances_match_the_yardstick(kind, N, im, B, wg):
    """K, P, Sigma in knot_rel and marg, event_var in entry_rel against the numpy recursions on complex-step blocks of the
    composite step, every problem included: within 1e-10, or 100 times the yardstick's own float64-to-longdouble distance
    where that is more (it is not: the largest is 3.5e-13).  Measured worst on the GPU: K 3.0e-13 (N = 61), P 2.9e-14,
    Sigma 1.6e-14, marg 1.4e-13, event_var 2.7e-15."""
    nlp, d, h, g, dist = _run(kind, N, im, B, wg)
    errs = (CR.knot_rel(g["Kh"], h["Kr"]), CR.knot_rel(g["Ph"], h["Pr"]), CR.knot_rel(g["Sh"], h["Sr"]),
            CR.entry_rel(g["margh"], h["mr"]), CR.entry_rel(g["varh"], h["vr"]))
    bars = [max(BAR, 100 * x) for x in dist]
    print(f"{kind} N={N} mode={im} B={B} K={wg}: K {errs[0]:.2e}, P {errs[1]:.2e}, Sigma {errs[2]:.2e}, marg {errs[3]:.2e}, "
          f"event_var {errs[4]:.2e}; yardstick to longdouble {max(dist):.2e}; bars {max(bars):.2e}")
    assert all(e <= b for e, b in zip(errs, bars)), (errs, bars)
    land = h["ev"][:, 0] >= 0
    assert land.any() and not g["varh"][~land].any()
    if kind == "shape":
        assert (~land).any() and (g["varh"][land, 1] > 0).all()
    if kind == "tau0":  # the guard's first branch: tau does not move, and the clock's variance is Sigma_0[14][14]
        assert not g["varh"][:, 0].any() and np.array_equal(g["varh"][:, 1], h["S0"][:, 14, 14])
    if h["K"] is None:
        assert not g["margh"][:, :, 1:5].any()


@pytest.mark.parametrize("kind,N,im,B,wg", CASES)
def test_cost_to_go_and_covariances_are_exactly_symmetric(kind, N, im, B, wg):
    _, _, _, g, _ = _run(kind, N, im, B, wg)
    assert np.array_equal(g["Ph"], np.swapaxes(g["Ph"], -1, -2)) and np.array_equal(g["Sh"], np.swapaxes(g["Sh"], -1, -2))


# ---- 2. no touchdown: bit for bit the knot-scheduled kernels -------------------------------------------------------------
@pytest.mark.parametrize("N,im,B", [(8, 1, 48), (40, 2, 9), (5, 2, 32)])
def test_a_batch_that_never_lands_is_bitwise_the_knot_scheduled_calls_of_a_handle_that_never_switches(N, im, B):
    """model == NULL and the handle's model passed explicitly, against qln_tracking_lqr / qln_tracking_covariance of a handle
    with k_trans = N + 1."""
    import torch

    batch, Zref, K, x0, th = GC.case(N, im, B, True, False)
    iy, iv = GC.free_foot(im)
    Zref[:, 15 + (3 if im == 1 else 1)::20] = -2.0  # every problem gets the last problem's pulling reference
    x0[:, iy], x0[:, iv] = 0.3, 0.0
    nlp, never = TC.nlp(batch, TC.SECOND_MODEL), TC.nlp(GC.with_k_trans(batch, N + 1), TC.SECOND_MODEL)
    dZ, dK, dx = nlp.upload_Z(Zref), EF.dev(K), EF.dev(x0)
    Zout, ev = nlp.tracking_rollout_guarded(dZ, dK, dx)
    assert bool((ev[:, 0] == -1).all())
    rng = np.random.default_rng(N)
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    Kr, Pr = never.tracking_lqr(Zout, TC.QW, TC.R, TC.QFW)
    for model in (None, EF.dev(np.tile(TC.SECOND, (B, 1)))):
        Kg, Pg = nlp.tracking_lqr_guarded(Zout, ev, TC.QW, TC.R, TC.QFW, model)
        assert torch.equal(Kg, Kr) and torch.equal(Pg, Pr)
        for k_ in (dK, None):
            Sr, mr = never.tracking_covariance(Zout, k_, S0, W)
            Sg, mg, vg = nlp.tracking_covariance_guarded(Zout, ev, k_, S0, W, model)
            assert torch.equal(Sg, Sr) and torch.equal(mg, mr) and not bool(vg.any())


# ---- 3. without numpy blocks: the guarded sweeps' own kernels ------------------------------------------------------------
@pytest.mark.parametrize("kind,N,im,B,wg", CASES)
def test_cost_to_go_is_the_lq_cost_of_the_gpu_tangent_sweep_under_the_returned_gains(kind, N, im, B, wg):
    """x' P_0 x against the LQ cost accumulated from qln_tracking_rollout_guarded_jvp's Zout_dot with x0_dot = x under the
    returned K: no oracle."""
    nlp, d, h, g, _ = _run(kind, N, im, B, wg)
    x = np.random.default_rng(N + B).normal(size=(B, 15))
    zd, _ = nlp.tracking_rollout_guarded_jvp(d["Zout"], d["Zout"], d["ev"], g["K"], d["model"], x0_dot=EF.dev(x))
    cost = TG.lq_cost(TC.rows(nlp, zd), N, TC.QW, TC.R, TC.QFW)
    quad = np.einsum("bi,bij,bj->b", x, g["Ph"][:, 0], x)
    w = float(np.max(np.abs(cost - quad) / np.abs(cost)))
    print(f"{kind} N={N} mode={im} B={B} K={wg}: x'P_0 x against the GPU sweep's LQ cost {w:.2e}; bar {COST_BAR:.2e}")
    assert w <= COST_BAR


@pytest.mark.parametrize("kind,N,im,B,wg", CASES)
def test_a_knots_quadratic_form_is_the_gpu_reverse_sweeps_x0_bar_in_sigma0(kind, N, im, B, wg):
    """W = 0: zbar' Sigma_k zbar = x0_bar' Sigma0 x0_bar with x0_bar from qln_tracking_rollout_guarded_vjp of a cotangent on
    x_k alone, as tests/test_gpu_tracking_cov.py does with the plain VJP: no oracle."""
    from quadruped_landing_amd import nlp as NL

    nlp, d, h, g, _ = _run(kind, N, im, B, wg)
    S, _, _ = nlp.tracking_covariance_guarded(d["Zout"], d["ev"], d["K"], h["S0"], None, d["model"], with_marginals=False,
                                              with_event_var=False)
    Sh = NL.unpack_covariance(S)
    rng = np.random.default_rng(3 * N + B)
    worst = 0.0
    for k in sorted({N - 1, N // 2 + 1} & set(range(1, N))):
        Zbar = np.zeros_like(h["Zout"])
        Zbar[:, 20 * k: 20 * k + 15] = rng.normal(size=(B, 15))
        _, _, xb, _ = nlp.tracking_rollout_guarded_vjp(d["Zref"], d["Zout"], d["ev"], nlp.upload_Z(Zbar), d["K"], d["model"],
                                                       want=("x0",))
        xb = xb.cpu().numpy()
        zk = Zbar[:, 20 * k: 20 * k + 15]
        lhs, rhs = np.einsum("bi,bij,bj->b", zk, Sh[:, k], zk), np.einsum("bi,bij,bj->b", xb, h["S0"], xb)
        worst = max(worst, float(np.max(np.abs(lhs - rhs) / np.abs(rhs))))
    print(f"{kind} N={N} mode={im} B={B} K={wg}: zbar'Sigma_k zbar against x0_bar'Sigma0 x0_bar {worst:.2e}; bar {DUALITY_BAR:.2e}")
    assert worst <= DUALITY_BAR


# ---- 4. forms and arguments ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"z_stride": 20 * 12 + 3, "align": 7}])
def test_host_forms_equal_device_forms(kw):
    batch, Zref, K, x0, th = GC.ragged_case()
    B = batch.B
    nlp = TC.nlp(batch, TC.SECOND_MODEL, **kw)
    dZ, dK, dx, dm = nlp.upload_Z(Zref), EF.dev(K), EF.dev(x0), EF.dev(th)
    Zout, ev = nlp.tracking_rollout_guarded(dZ, dK, dx, dm)
    rng = np.random.default_rng(12)
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    zh, evh = Zout.cpu().numpy(), ev.cpu().numpy()
    Kg, Pg = nlp.tracking_lqr_guarded(Zout, ev, TC.QW, TC.R, TC.QFW, dm)
    Kh, Ph = nlp.tracking_lqr_guarded_host(zh, evh, TC.QW, TC.R, TC.QFW, th)
    assert np.array_equal(Kh, Kg.cpu().numpy()) and np.array_equal(Ph, Pg.cpu().numpy())
    for k_ in (K, None):
        Sg, mg, vg = nlp.tracking_covariance_guarded(Zout, ev, EF.dev(k_), S0, W, dm)
        Sh, mh, vh = nlp.tracking_covariance_guarded_host(zh, evh, k_, S0, W, th)
        assert np.array_equal(Sh, Sg.cpu().numpy()) and np.array_equal(mh, mg.cpu().numpy()) and np.array_equal(vh, vg.cpu().numpy())
    assert (evh[:, 0] >= 0).any() and vh[evh[:, 0] >= 0, 1].min() > 0


def test_which_outputs_are_asked_for_does_not_change_the_others_bits():
    import torch

    nlp, d, h, g, _ = _run("shape", 40, 1, 9, True)
    K2, P2 = nlp.tracking_lqr_guarded(d["Zout"], d["ev"], TC.QW, TC.R, TC.QFW, d["model"], with_cost_to_go=False)
    assert P2 is None and torch.equal(K2, g["K"])
    for ws, wm, wv in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        S, mg, v = nlp.tracking_covariance_guarded(d["Zout"], d["ev"], d["K"], h["S0"], h["W"], d["model"], with_sigma=ws,
                                                   with_marginals=wm, with_event_var=wv)
        for got, ref, asked in ((S, g["S"], ws), (mg, g["marg"], wm), (v, g["var"], wv)):
            assert (got is None and not asked) or torch.equal(got, ref)


def test_invalid_arguments_are_refused():
    import torch

    from quadruped_landing_amd import _lib

    batch, Zref, K, x0, th = GC.case(5, 2, 32, True, True)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    L, h, INV, OK = _lib.lib(), nlp._h, _lib.QLN_ERR_INVALID_ARGUMENT, _lib.QLN_OK
    B, N = nlp.B, nlp.N
    dZ, dK, dm = nlp.upload_Z(Zref), EF.dev(K), EF.dev(th)
    Zout, ev = nlp.tracking_rollout_guarded(dZ, dK, EF.dev(x0), dm)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    Ko, Po, So, mo, vo, S0 = f64(B, N - 1, 4, 15), f64(B, N, 120), f64(B, N, 120), f64(B, N, 8), f64(B, 2), f64(120)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    a = lambda v: v.ctypes.data  # noqa: E731
    Q, R, Qf = (np.ascontiguousarray(w, dtype=np.float64) for w in (TC.QW, TC.R, TC.QFW))
    lqr, cov = L.qln_tracking_lqr_guarded, L.qln_tracking_covariance_guarded
    assert lqr(h, p(Zout), None, None, a(Q), a(R), a(Qf), p(Ko), p(Po)) == INV  # NULL event
    assert b"event" in L.qln_last_error()
    assert lqr(h, None, None, p(ev), a(Q), a(R), a(Qf), p(Ko), None) == INV
    assert lqr(h, p(Zout), None, p(ev), a(Q), a(R), a(Qf), None, None) == INV
    assert lqr(h, p(Zout), None, p(ev), a(Q), a(np.array([1.0, 0.0, 1.0, 1.0])), a(Qf), p(Ko), None) == INV  # R not > 0
    assert lqr(h, p(Zout), None, p(ev), a(Q), a(R), a(Qf), p(Zout), None) == INV  # K overlaps Ztraj
    assert lqr(h, p(Zout), None, p(ev), a(Q), a(R), a(Qf), p(Ko), p(ev)) == INV  # P overlaps event
    assert b"overlaps" in L.qln_last_error()
    assert lqr(h, p(Zout), p(dm), p(ev), a(Q), a(R), a(Qf), p(Ko), p(dm)) == INV  # P overlaps model
    assert lqr(h, p(Zout), p(dm), p(ev), a(Q), a(R), a(Qf), p(Ko), p(Po)) == OK
    assert cov(h, p(Zout), None, None, None, p(S0), 1, None, p(So), p(mo), None) == INV  # NULL event
    assert b"event" in L.qln_last_error()
    assert cov(h, p(Zout), None, None, p(ev), p(S0), 1, None, None, None, None) == INV  # nothing asked for
    assert cov(h, p(Zout), None, None, p(ev), p(S0), 2, None, p(So), None, None) == INV  # sigma0_batch
    assert cov(h, p(Zout), None, None, p(ev), p(S0), 1, None, p(So), None, p(ev)) == INV  # event_var overlaps event
    assert cov(h, p(Zout), None, None, p(ev), p(S0), 1, None, p(So), None, p(So)) == INV  # two outputs overlap
    assert cov(h, p(Zout), None, p(dm), p(ev), p(S0), 1, None, p(dm), None, None) == INV  # Sigma overlaps model
    assert cov(h, p(Zout), p(dK), p(dm), p(ev), p(S0), 1, None, None, None, p(vo)) == OK  # event_var alone
    assert cov(h, p(Zout), p(dK), p(dm), p(ev), p(S0), 1, None, p(So), p(mo), p(vo)) == OK
    torch.cuda.synchronize()
    # host forms: the same, and the values of the record and of the models
    zo, evh, S0h = Zout.cpu().numpy(), ev.cpu().numpy(), np.zeros(120)
    Kh, Sh = np.zeros((B, N - 1, 4, 15)), np.zeros((B, N, 120))
    hl, hc = L.qln_tracking_lqr_guarded_host, L.qln_tracking_covariance_guarded_host
    assert hl(h, a(zo), None, None, a(Q), a(R), a(Qf), a(Kh), None) == INV
    assert hc(h, a(zo), None, None, None, a(S0h), 1, None, a(Sh), None, None) == INV
    for entry, value in ((0, 0.5), (0, -2.0), (0, float(N - 1)), (0, np.nan), (1, -1e-3), (1, np.inf), (1, np.nan)):
        bad = np.array(evh)
        bad[B - 2, entry] = value
        assert hl(h, a(zo), None, a(bad), a(Q), a(R), a(Qf), a(Kh), None) == INV, (entry, value)
        assert hc(h, a(zo), None, None, a(bad), a(S0h), 1, None, a(Sh), None, None) == INV, (entry, value)
    for entry, value in ((0, np.nan), (1, 0.0), (2, -0.1), (3, np.inf)):
        bad = np.array(th)
        bad[3, entry] = value
        assert hl(h, a(zo), a(bad), a(evh), a(Q), a(R), a(Qf), a(Kh), None) == INV, (entry, value)
        assert hc(h, a(zo), None, a(bad), a(evh), a(S0h), 1, None, a(Sh), None, None) == INV, (entry, value)
    assert not Kh.any() and not Sh.any()
    assert hl(h, a(zo), a(th), a(evh), a(Q), a(R), a(Qf), a(Kh), None) == OK
    assert hc(h, a(zo), None, a(th), a(evh), a(S0h), 1, None, a(Sh), None, None) == OK
