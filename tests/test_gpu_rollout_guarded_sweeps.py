"""qln_tracking_rollout_guarded_jvp / _vjp on the GPU: the forward and reverse sweeps through the guard-triggered touchdown
(include/qln_evaluator.h).  The yardstick is tests/rollout_guarded_sweep_ref.py, held on the CPU by
tests/test_rollout_guarded_sweeps_host.py; besides it the kernels are held without an oracle by the adjoint identity, by
central differences of the GPU's own guarded roll-out, and bit for bit by the _model_ sweeps where no problem lands.  The
cases and their seeds are tests/rollout_guarded_cases.py's."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_sweep_ref as SR
from tests import tracking_cases as TC

pytestmark = pytest.mark.gpu

SWEEP_BAR = 1e-12        # the project's bar for a sweep against numpy, of max(1, |ref|) (tests/test_gpu_rollout_jvp.py)
DIRECTION_SCALE = 1e-2   # tests/test_rollout_guarded_sweeps_host.py: tangents of the size of the cases' own perturbations
# Test 3.  The same difference quotient in float64 numpy (rollout_guarded_ref.rollout at x0 +- FD_EPS x0_dot against the
# yardstick's sweep, every shape of GC.SHAPES with gains and models) leaves 2.3e-11 .. 2.5e-10 of max(1, |ref|) at 1e-4, its
# best step (1e-3: up to 4.9e-9, truncation; 1e-5: up to 2.4e-9, rounding): the bar is ten times the worst.
FD_EPS = 1e-4
FD_CPU_WORST = 2.51e-10
FD_BAR = 10 * FD_CPU_WORST

SHAPE_CASES = [("shape", N, im, B, wg, wm) for (N, im, B) in GC.SHAPES for wg, wm in ((False, False), (True, True))]
CASES = SHAPE_CASES + [("ragged", 12, 0, 70, True, True), ("tau0", 5, 1, 3, False, False), ("tau0", 5, 2, 3, False, False)]
# which tangents are present: every combination with an instantiation of its own (K, K_dot, Zref_dot; x0_dot and model_dot
# are run-time arguments of every one and always given here)
JVP_COMBOS = {True: [(True, True), (True, False), (False, True), (False, False)], False: [(False, True), (False, False)]}


def _dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(kind, N, im, B, wg, wm):
    if kind == "shape":
        batch, Zref, K, x0, th = GC.case(N, im, B, wg, wm)
        return batch, Zref, K, x0, th, im
    if kind == "ragged":
        batch, Zref, K, x0, th = GC.ragged_case()
        return batch, Zref, K, x0, th, np.asarray(batch.init_mode)
    batch, Zref, x0, th = GC.tau_zero_case(N, im)
    return batch, Zref, None, x0, th, im


@functools.lru_cache(maxsize=None)
def _run(kind, N, im, B, wg, wm):
    """One case: the GPU's guarded roll-out, the yardstick's blocks at the GPU's own Zout and events, one direction and one
    cotangent, the yardstick's sweeps along them and its own float64-to-longdouble distance.  Shared by the tests of the
    case; nothing here is changed afterwards."""
    batch, Zref, K, x0, th, ims = _inputs(kind, N, im, B, wg, wm)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    dev = dict(Zref=nlp.upload_Z(Zref), K=_dev(K), x0=_dev(x0), model=_dev(th) if wm else None)
    Zout, ev = nlp.tracking_rollout_guarded(dev["Zref"], dev["K"], dev["x0"], dev["model"])
    zo, evh = TC.rows(nlp, Zout), ev.cpu().numpy()
    F, T = SR.blocks(N, ims, zo, th, evh)
    zd, kd, xd, md = SR.directions(GC.seed_of(N, im, wg, wm) + 31, B, N, K is not None, DIRECTION_SCALE)
    Zbar = DIRECTION_SCALE * np.random.default_rng(GC.seed_of(N, im, wg, wm) + 37).normal(size=zo.shape)
    # the yardstick's own distance to its extended-precision restatement, along the full direction and cotangent
    Fl, _ = SR.blocks(N, ims, zo, th, evh, ctype=np.clongdouble)
    ref_j, _ = SR.sweep_jvp(F, T, evh, Zref, K, zo, zd, kd, xd, md)
    ref_v = SR.sweep_vjp(F, Zref, K, zo, Zbar)
    dist = max([SR.worst(ref_j, SR.sweep_jvp_extended(Fl, K, Zref, zo, zd, kd, xd, md))] +
               [SR.worst(a, b) for a, b in zip(ref_v, SR.sweep_vjp_extended(Fl, K, Zref, zo, Zbar)) if a is not None])
    bar = max(SWEEP_BAR, 100 * dist)
    if bar > SWEEP_BAR:
        print(f"{kind} N={N} mode={im} B={B}: the yardstick is {dist:.2e} from its longdouble restatement: bar {bar:.2e}")
    host = dict(Zref=Zref, K=K, x0=x0, th=th, Zout=zo, ev=evh, zd=zd, kd=kd, xd=xd, md=md, Zbar=Zbar, F=F, T=T)
    dev.update(Zout=Zout, ev=ev, zd=nlp.upload_Z(zd), kd=_dev(kd), xd=_dev(xd), md=_dev(md), Zbar=nlp.upload_Z(Zbar))
    return nlp, dev, host, bar


# ---- 1. against the yardstick, every instantiation ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,im,B,wg,wm", CASES)
def test_sweeps_match_the_yardstick_in_every_combination_of_tangents(kind, N, im, B, wg, wm):
    """Device JVP and VJP at the GPU's own Zout and events against the numpy sweeps on complex-step blocks of the composite
    step, within 1e-12 of max(1, |ref|) -- or 100 times the yardstick's own float64-to-longdouble distance where that is more
    (printed when it is: 1.08e-14 for N = 61 with gains, bar 1.08e-12 there; 1e-12 everywhere else).  The GPU's worst is
    9.8e-15."""
    nlp, d, h, bar = _run(kind, N, im, B, wg, wm)
    worst = 0.0
    for has_kd, has_zd in JVP_COMBOS[h["K"] is not None]:
        got, _ = nlp.tracking_rollout_guarded_jvp(d["Zref"], d["Zout"], d["ev"], d["K"], d["model"], d["zd"] if has_zd else None,
                                                  d["kd"] if has_kd else None, d["xd"], d["md"])
        ref, _ = SR.sweep_jvp(h["F"], h["T"], h["ev"], h["Zref"], h["K"], h["Zout"], h["zd"] if has_zd else None,
                              h["kd"] if has_kd else None, h["xd"], h["md"])
        w = SR.worst(TC.rows(nlp, got), ref)
        print(f"{kind} N={N} mode={im} B={B} K={wg} models={wm}: jvp K_dot={has_kd} Zref_dot={has_zd}: {w:.2e}")
        worst = max(worst, w)
    zb, kb, xb, mb = nlp.tracking_rollout_guarded_vjp(d["Zref"], d["Zout"], d["ev"], d["Zbar"], d["K"], d["model"])
    rz, rk, rx, rm = SR.sweep_vjp(h["F"], h["Zref"], h["K"], h["Zout"], h["Zbar"])
    wv = [SR.worst(TC.rows(nlp, zb), rz), SR.worst(TC.to_np(xb), rx), SR.worst(TC.to_np(mb), rm)]
    if h["K"] is not None:
        wv.append(SR.worst(TC.to_np(kb), rk))
    print(f"{kind} N={N} mode={im} B={B} K={wg} models={wm}: vjp Zref_bar, x0_bar, model_bar, K_bar {wv}; bar {bar:.2e}")
    assert max(worst, *wv) <= bar, (worst, wv, bar)
    assert (h["ev"][:, 0] >= 0).any()


# ---- 2. the adjoint identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,im,B,wg,wm", CASES)
def test_adjoint_identity_between_the_two_kernels(kind, N, im, B, wg, wm):
    """<Zbar, J d> = <J' Zbar, d> with model_bar included: no oracle involved."""
    import torch

    nlp, d, h, _ = _run(kind, N, im, B, wg, wm)
    got, _ = nlp.tracking_rollout_guarded_jvp(d["Zref"], d["Zout"], d["ev"], d["K"], d["model"], d["zd"], d["kd"], d["xd"], d["md"])
    zb, kb, xb, mb = nlp.tracking_rollout_guarded_vjp(d["Zref"], d["Zout"], d["ev"], d["Zbar"], d["K"], d["model"])
    lhs = float(torch.dot(d["Zbar"], got))
    rhs = float(torch.dot(zb, d["zd"]) + torch.dot(xb.view(-1), d["xd"].view(-1)) + torch.dot(mb.view(-1), d["md"].view(-1)))
    if h["K"] is not None:
        rhs += float(torch.dot(kb.view(-1), d["kd"].view(-1)))
    print(f"{kind} N={N} mode={im} B={B} K={wg}: <Zbar, J d> {lhs:.15e}, <J' Zbar, d> {rhs:.15e}, "
          f"difference {abs(lhs - rhs) / (abs(lhs) + abs(rhs)):.2e}")
    assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs)), (lhs, rhs)


# ---- 3. central differences of the GPU's own guarded roll-out ------------------------------------------------------------
@pytest.mark.parametrize("N,im,B", GC.SHAPES)
def test_jvp_in_an_x0_direction_matches_central_differences_of_the_gpu_rollout(N, im, B):
    """No oracle: (rollout(x0 + eps d) - rollout(x0 - eps d)) / (2 eps) on the GPU against Zout_dot, on the problems whose
    touchdown knot is the same at both ends.  A sweep without the tau term misses by more than 1e-2 at N = 40 and 61
    (tests/test_rollout_guarded_sweeps_host.py)."""
    nlp, d, h, _ = _run("shape", N, im, B, True, True)
    got, _ = nlp.tracking_rollout_guarded_jvp(d["Zref"], d["Zout"], d["ev"], d["K"], d["model"], x0_dot=d["xd"])
    zp, ep = nlp.tracking_rollout_guarded(d["Zref"], d["K"], d["x0"] + FD_EPS * d["xd"], d["model"])
    zm, em = nlp.tracking_rollout_guarded(d["Zref"], d["K"], d["x0"] - FD_EPS * d["xd"], d["model"])
    same = (ep.cpu().numpy()[:, 0] == h["ev"][:, 0]) & (em.cpu().numpy()[:, 0] == h["ev"][:, 0])
    assert (~same).sum() <= GC.LEFT_OUT * B, f"{(~same).sum()} of {B} problems change their touchdown knot over the step"
    fd = (TC.rows(nlp, zp) - TC.rows(nlp, zm)) / (2 * FD_EPS)
    w = SR.worst(TC.rows(nlp, got)[same], fd[same])
    print(f"N={N} mode={im} B={B}: GPU quotient against Zout_dot {w:.2e} of max(1, |ref|); bar {FD_BAR:.2e}; left out "
          f"{(~same).sum()}")
    assert w <= FD_BAR and (h["ev"][same, 0] >= 0).any()


# ---- 4. no touchdown: bit for bit the _model_ sweeps ---------------------------------------------------------------------
@pytest.mark.parametrize("N,im,B,wm", [(8, 1, 48, True), (40, 2, 9, True), (5, 2, 32, False)])
def test_a_batch_that_never_lands_is_bitwise_the_model_sweeps_of_a_handle_that_never_switches(N, im, B, wm):
    import torch

    batch, Zref, K, x0, th = GC.case(N, im, B, True, wm)
    iy, iv = GC.free_foot(im)
    Zref[:, 15 + (3 if im == 1 else 1)::20] = -2.0  # every problem gets the last problem's pulling reference
    x0[:, iy], x0[:, iv] = 0.3, 0.0
    nlp, never = TC.nlp(batch, TC.SECOND_MODEL), TC.nlp(GC.with_k_trans(batch, N + 1), TC.SECOND_MODEL)
    dZ, dK, dx, dm = nlp.upload_Z(Zref), _dev(K), _dev(x0), _dev(th) if wm else None
    Zout, ev = nlp.tracking_rollout_guarded(dZ, dK, dx, dm)
    assert bool((ev[:, 0] == -1).all())
    zd, kd, xd, md = SR.directions(3, B, N, True, DIRECTION_SCALE)
    zd, kd, xd, md = nlp.upload_Z(zd), _dev(kd), _dev(xd), _dev(md)
    Zbar = nlp.upload_Z(np.random.default_rng(4).normal(size=Zref.shape))
    for k_, kd_ in ((dK, kd), (dK, None), (None, None)):
        got, ed = nlp.tracking_rollout_guarded_jvp(dZ, Zout, ev, k_, dm, zd, kd_, xd, md)
        ref = never.tracking_rollout_model_jvp(dZ, Zout, k_, dm, zd, kd_, xd, md)
        assert torch.equal(got, ref) and not bool(ed.any())
        outs = nlp.tracking_rollout_guarded_vjp(dZ, Zout, ev, Zbar, k_, dm)
        refs = never.tracking_rollout_model_vjp(dZ, Zout, Zbar, k_, dm)
        for a, b in zip(outs, refs):
            assert (a is None and b is None) or torch.equal(a, b)


# ---- 5. event_dot --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,im,B,wg,wm", CASES)
def test_event_dot_matches_the_yardstick_and_is_zero_without_a_touchdown(kind, N, im, B, wg, wm):
    nlp, d, h, bar = _run(kind, N, im, B, wg, wm)
    _, ed = nlp.tracking_rollout_guarded_jvp(d["Zref"], d["Zout"], d["ev"], d["K"], d["model"], d["zd"], d["kd"], d["xd"], d["md"])
    _, ref = SR.sweep_jvp(h["F"], h["T"], h["ev"], h["Zref"], h["K"], h["Zout"], h["zd"], h["kd"], h["xd"], h["md"])
    got = ed.cpu().numpy()
    w = SR.worst(got, ref)
    print(f"{kind} N={N} mode={im} B={B} K={wg}: event_dot {w:.2e}; bar {bar:.2e}")
    assert w <= bar
    assert not got[:, [0, 3, 4, 5, 6, 7]].any() and not got[h["ev"][:, 0] < 0].any()
    if kind == "shape":
        assert (h["ev"][:, 0] < 0).any() and np.abs(got[h["ev"][:, 0] >= 0, 1]).min() > 0
    if kind == "tau0":
        assert not got[:, 1].any() and np.array_equal(got[:, 2], h["xd"][:, 14])


# ---- 6. forms and arguments ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"z_stride": 20 * 12 + 3, "align": 7}])
def test_host_forms_equal_device_forms_and_padding_is_untouched(kw):
    import torch

    batch, Zref, K, x0, th = GC.ragged_case()
    B, N = batch.B, batch.N
    nlp = TC.nlp(batch, TC.SECOND_MODEL, **kw)
    n, zs = nlp.n_nlp, nlp.z_stride
    dZ, dK, dx, dm = nlp.upload_Z(Zref), _dev(K), _dev(x0), _dev(th)
    Zout, ev = nlp.tracking_rollout_guarded(dZ, dK, dx, dm)
    zd, kd, xd, md = SR.directions(8, B, N, True, DIRECTION_SCALE)
    Zbar = np.random.default_rng(9).normal(size=Zref.shape)
    pad = lambda a: np.concatenate([a, np.zeros((B, zs - n))], axis=1).reshape(-1)  # noqa: E731
    sentinel = torch.full((B * zs,), -7.25, dtype=torch.float64, device="cuda")
    got, ed = nlp.tracking_rollout_guarded_jvp(dZ, Zout, ev, dK, dm, nlp.upload_Z(zd), _dev(kd), _dev(xd), _dev(md), out=sentinel)
    assert got is sentinel and bool((got.view(B, zs)[:, n:] == -7.25).all())
    zh, evh = Zout.cpu().numpy(), ev.cpu().numpy()
    hj, hed = nlp.tracking_rollout_guarded_jvp_host(pad(Zref), zh, evh, K, th, pad(zd), kd, xd, md)
    assert np.array_equal(hj.reshape(B, zs)[:, :n], TC.rows(nlp, got)) and np.array_equal(hed, ed.cpu().numpy())
    assert not hj.reshape(B, zs)[:, n:].any()
    zb, kb, xb, mb = nlp.tracking_rollout_guarded_vjp(dZ, Zout, ev, nlp.upload_Z(Zbar), dK, dm)
    hz, hk, hx, hm = nlp.tracking_rollout_guarded_vjp_host(pad(Zref), zh, evh, pad(Zbar), K, th)
    assert np.array_equal(hz.reshape(B, zs)[:, :n], TC.rows(nlp, zb)) and not hz.reshape(B, zs)[:, n:].any()
    assert np.array_equal(hk, TC.to_np(kb)) and np.array_equal(hx, TC.to_np(xb)) and np.array_equal(hm, TC.to_np(mb))


def test_invalid_arguments_are_refused():
    import torch

    from quadruped_landing_amd import _lib

    batch, Zref, K, x0, th = GC.case(5, 2, 32, True, True)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    L, h, INV = _lib.lib(), nlp._h, _lib.QLN_ERR_INVALID_ARGUMENT
    dZ, dx = nlp.upload_Z(Zref), _dev(x0)
    Zout, ev = nlp.tracking_rollout_guarded(dZ, None, dx)
    out, xd, xb = nlp.new_Z(), _dev(np.ones((nlp.B, 15))), torch.zeros((nlp.B, 15), dtype=torch.float64, device="cuda")
    ed = torch.zeros_like(ev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    jvp, vjp = L.qln_tracking_rollout_guarded_jvp, L.qln_tracking_rollout_guarded_vjp
    assert jvp(h, p(dZ), None, p(Zout), None, None, None, None, p(xd), None, p(out), None) == INV  # NULL event
    assert b"event" in L.qln_last_error()
    assert vjp(h, p(dZ), None, p(Zout), None, None, p(dZ), None, None, p(xb), None) == INV
    assert jvp(h, p(dZ), None, p(Zout), None, p(ev), None, None, None, None, p(out), None) == INV   # no tangent
    assert jvp(h, p(dZ), None, p(Zout), None, p(ev), None, p(dZ), p(xd), None, p(out), None) == INV  # K_dot without K
    assert jvp(h, p(dZ), None, p(Zout), None, p(ev), None, None, p(xd), None, p(Zout), None) == INV  # Zout_dot overlaps Zout
    assert jvp(h, p(dZ), None, p(Zout), None, p(ev), None, None, p(xd), None, p(out), p(ev)) == INV  # event_dot overlaps event
    assert b"overlaps" in L.qln_last_error()
    assert vjp(h, p(dZ), None, p(Zout), None, p(ev), p(dZ), None, None, p(ev), None) == INV         # x0_bar overlaps event
    assert jvp(h, p(dZ), None, p(Zout), None, p(ev), None, None, p(xd), None, p(out), p(ed)) == _lib.QLN_OK
    assert vjp(h, p(dZ), None, p(Zout), None, p(ev), p(dZ), None, None, p(xb), None) == _lib.QLN_OK
    # host forms: the same, and the record's values
    Zh, zo, evh = np.ascontiguousarray(TC.rows(nlp, dZ)).reshape(-1), Zout.cpu().numpy(), ev.cpu().numpy()
    oh, xdh, xbh = np.zeros(nlp.dims.z_total), np.ones((nlp.B, 15)), np.zeros((nlp.B, 15))
    a = lambda v: v.ctypes.data  # noqa: E731
    hj, hv = L.qln_tracking_rollout_guarded_jvp_host, L.qln_tracking_rollout_guarded_vjp_host
    assert hj(h, a(Zh), None, a(zo), None, None, None, None, a(xdh), None, a(oh), None) == INV
    assert hv(h, a(Zh), None, a(zo), None, None, a(Zh), None, None, a(xbh), None) == INV
    for entry, value in ((0, 0.5), (0, -2.0), (0, float(nlp.N - 1)), (0, np.nan), (1, -1e-3), (1, np.inf), (1, np.nan)):
        bad = np.array(evh)
        bad[nlp.B - 2, entry] = value
        before = oh.copy()
        assert hj(h, a(Zh), None, a(zo), None, a(bad), None, None, a(xdh), None, a(oh), None) == INV, (entry, value)
        assert hv(h, a(Zh), None, a(zo), None, a(bad), a(Zh), None, None, a(xbh), None) == INV, (entry, value)
        assert np.array_equal(oh, before) and not xbh.any()
    assert hj(h, a(Zh), None, a(zo), None, a(evh), None, None, a(xdh), None, a(oh), None) == _lib.QLN_OK
    assert hv(h, a(Zh), None, a(zo), None, a(evh), a(Zh), None, None, a(xbh), None) == _lib.QLN_OK


# ---- 7. torch autograd ---------------------------------------------------------------------------------------------------
def test_differentiable_rollout_guarded_backward_forward_ad_and_a_first_adam_step():
    import torch
    import torch.autograd.forward_ad as fwAD

    nlp, d, h, _ = _run("shape", 40, 1, 9, True, True)
    n = nlp.n_nlp
    leaves = [d[k].clone().requires_grad_(True) for k in ("Zref", "K", "x0", "model")]
    Zout, ev = nlp.differentiable_rollout(*leaves, guarded=True)
    assert torch.equal(Zout, d["Zout"]) and torch.equal(ev, d["ev"]) and not ev.requires_grad
    Zout.backward(d["Zbar"])
    zb, kb, xb, mb = nlp.tracking_rollout_guarded_vjp(d["Zref"], d["Zout"], d["ev"], d["Zbar"], d["K"], d["model"])
    for leaf, ref in zip(leaves, (zb, kb, xb, mb)):
        assert torch.equal(leaf.grad.reshape(-1), ref.reshape(-1))
    with fwAD.dual_level():
        duals = [fwAD.make_dual(d[k], d[t].reshape(d[k].shape)) for k, t in (("Zref", "zd"), ("K", "kd"), ("x0", "xd"), ("model", "md"))]
        out, _ = nlp.differentiable_rollout(*duals, guarded=True)
        tangent = fwAD.unpack_dual(out).tangent
    ref, _ = nlp.tracking_rollout_guarded_jvp(d["Zref"], d["Zout"], d["ev"], d["K"], d["model"], d["zd"], d["kd"], d["xd"], d["md"])
    assert torch.equal(tangent, ref)
    out, tangent = torch.func.jvp(lambda a, b_, c, m: nlp.differentiable_rollout(a, b_, c, m, guarded=True)[0],
                                  tuple(d[k] for k in ("Zref", "K", "x0", "model")),
                                  (d["zd"], d["kd"], d["xd"].reshape(d["x0"].shape), d["md"].reshape(d["model"].shape)))
    assert torch.equal(out, d["Zout"]) and torch.equal(tangent, ref)
    # Adam's first step on K through it: the terminal error moves the way the VJP says
    xN_ref = d["Zref"].view(nlp.B, -1)[:, n - 15: n]
    loss_of = lambda Z: ((Z.view(nlp.B, -1)[:, n - 15: n] - xN_ref) ** 2).sum()  # noqa: E731
    Kp = d["K"].clone().requires_grad_(True)
    opt = torch.optim.Adam([Kp], lr=1e-4)
    Z0, ev0 = nlp.differentiable_rollout(d["Zref"], Kp, d["x0"], d["model"], guarded=True)
    loss0 = loss_of(Z0)
    loss0.backward()
    grad = Kp.grad.clone()
    before = Kp.detach().clone()
    opt.step()
    predicted = float((grad * (Kp.detach() - before)).sum())
    Z1, ev1 = nlp.tracking_rollout_guarded(d["Zref"], Kp.detach(), d["x0"], d["model"])
    actual = float(loss_of(Z1) - loss0.detach())
    print(f"Adam's first step on K: predicted change of the terminal error {predicted:.3e}, actual {actual:.3e}")
    assert torch.equal(ev1[:, 0], ev0[:, 0]) and predicted < 0 and actual < 0 and abs(actual - predicted) <= 0.1 * abs(predicted)
