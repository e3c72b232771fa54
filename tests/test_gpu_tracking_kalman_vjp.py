"""qln_noise_design_vjp / _guarded_vjp on the GPU: the reverse sweep through the design of the Kalman filter
(include/qln_evaluator.h), at the gains the GPU's own tracking_kalman* returned.  The yardstick is
tests/tracking_kalman_vjp_ref.py, held on the CPU by tests/test_tracking_kalman_vjp_host.py; it runs on the evaluator's dense
blocks, and for the guarded call on the complex-step blocks of tests/rollout_guarded_sweep_ref.py.  No bar here is a number chosen
in advance: the kernel's distance from the longdouble yardstick is set against the float64 numpy yardstick's own on the same
case, the duality of the two kernels and the linearity against what the float64 numpy pair leaves, ten times each.  Besides that
the kernel is held bit for bit: a NULL cotangent is explicit zeros, every subset of outputs has the full call's bits, ny rows are
eight rows with zeros written out, the host forms have the device forms' bits, NaN where nothing is read changes nothing, and a
batch that never lands is the knot-scheduled call.  Shapes: tests/estimation_cases.py's kinds at N = 5 and 17, B no
multiple of four.  Worst figures: profiles/tracking_kalman_vjp_tests.txt.

The kernel reads every knot of Lgain whatever the cotangents are (a zero cotangent takes the path of a given one), so there is no
case with NaN in the gains behind the last knot that carries a cotangent."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import estimation_cases as EF
from tests import landing_filter_sweep_ref as FS
from tests import rollout_guarded_cases as GC
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR
from tests import tracking_guarded_ref as TG
from tests import tracking_kalman_sweep_ref as KS
from tests import tracking_kalman_vjp_ref as KV

pytestmark = pytest.mark.gpu
_time_limit = EF.time_limit(300)

OUT = KV.OUT
COT = ("Lgain_bar", "Pest_bar", "logdet_bar")
LD = np.longdouble
FLOOR = 1e-13  # of the output's largest entry: the least distance a ratio is taken with

# (kind, B, N, k_trans, init_mode, ny, the handle at TC.SECOND_MODEL): a partly filled wave, a second wave with one or two rows
CASES = [("shape", 3, 5, 3, 2, 3, False), ("shape", 5, 17, 6, 1, 8, True), ("shape", 6, 17, 18, 2, 1, False),
         ("ragged", 9, 5, 3, 1, 8, True)]
# (N, init_mode, B, a model per problem, ny); the handle is at TC.SECOND_MODEL
GUARDED = [(5, 2, 6, True, 3), (17, 1, 3, False, 8), (17, 1, 3, True, 1)]


def _host(res):
    return {k: TC.to_np(v) for k, v in res.items()}


def _cast(dt, *a):
    return tuple(None if x is None else np.asarray(x).astype(dt) for x in a)


@functools.lru_cache(maxsize=None)
def _run(kind, B, N, k_trans, im, ny, second):
    """One knot-scheduled case: the handle, the GPU's own design, one set of cotangents, the GPU's sweep and the two yardsticks
    (float64 and longdouble) on the evaluator's dense blocks at the same Zout.  Shared by the case's tests, never changed."""
    d = EF.scheduled_design(kind, B, N, k_trans, im, ny, 5, **({"model": TC.SECOND_MODEL} if second else {}))
    nlp, Zout, H, V, S0, W = d.nlp, d.Zout, d.H, d.V, d.S0, d.W
    L = nlp.tracking_kalman(Zout, H, V, None, S0, W)[0]
    cot = KV.cotangents(d.seed + 11, N, ny, (B,))
    dcot = tuple(EF.dev(c) for c in cot)
    got = nlp.tracking_kalman_vjp(Zout, L, H, V, *dcot)
    lo, hi = EF.in_both_precisions(KV.sweep, d.A, H, V, TC.to_np(L), *cot)
    inp = dict(Zout=Zout, L=L, H=H, V=V, S0=S0, W=W, cot=cot, dcot=dcot, A=d.A, kw={})
    return nlp, inp, got, lo, hi


@functools.lru_cache(maxsize=None)
def _run_guarded(N, im, B, wm, ny):
    d = EF.guarded_design("shape", N, im, B, True, wm, ny)
    nlp, Zout, ev, dm, H, V, S0, W = d.nlp, d.Zout, d.ev, d.model, d.H, d.V, d.S0, d.W
    L = nlp.tracking_kalman_guarded(Zout, ev, H, V, None, S0, W, dm)[0]
    cot = KV.cotangents(N + B, N, ny, (B,))
    dcot = tuple(EF.dev(c) for c in cot)
    kw = dict(events=ev, model=dm, guarded=True)
    got = nlp.tracking_kalman_vjp(Zout, L, H, V, *dcot, **kw)
    A, _ = TG.split(d.F)
    lo, hi = EF.in_both_precisions(KV.sweep, A, H, V, TC.to_np(L), *cot)
    inp = dict(Zout=Zout, ev=ev, evh=d.evh, model=dm, th=d.th, L=L, H=H, V=V, S0=S0, W=W, cot=cot, dcot=dcot, A=A, kw=kw)
    return nlp, inp, got, lo, hi


def _check(tag, got, lo, hi):
    g = _host(got)
    line = []
    for k in OUT:
        assert np.isfinite(g[k]).all()
        e, _ = KV.out_rel(g[k], hi[k])
        own, _ = KV.out_rel(lo[k], hi[k])
        line.append(f"{k} {e:.2e} ({own:.2e})")
        assert max(e, FLOOR) <= 10 * max(own, FLOOR), (k, e, own)
    print(f"design vjp {tag}: the kernel to the longdouble yardstick (the float64 yardstick to it): " + ", ".join(line))


# ---- 1. against the yardstick --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,second", CASES)
def test_sweep_matches_the_yardstick(kind, B, N, k_trans, im, ny, second):
    """Each output's worst entry, relative to the output's largest, against the longdouble yardstick: at most ten times the
    float64 yardstick's own distance, both floored at 1e-13."""
    nlp, inp, got, lo, hi = _run(kind, B, N, k_trans, im, ny, second)
    assert got["Sigma0"].shape == (B, 120) and got["W"].shape == (B, 15) and got["V"].shape == (B, ny)
    _check(f"{kind} B={B} N={N} k_trans={k_trans} mode={im} ny={ny} second={second}", got, lo, hi)


@pytest.mark.parametrize("N,im,B,wm,ny", GUARDED)
def test_guarded_sweep_matches_the_yardstick(N, im, B, wm, ny):
    """On the complex-step blocks of the composite step, with and without a model per problem; the handle is at TC.SECOND_MODEL."""
    nlp, inp, got, lo, hi = _run_guarded(N, im, B, wm, ny)
    assert (inp["evh"][:, 0] >= 0).any()
    _check(f"guarded N={N} mode={im} B={B} models={wm} ny={ny}", got, lo, hi)


# ---- 2. duality between the two kernels ----------------------------------------------------------------------------------
def _duality(nlp, inp, got, tag):
    """The GPU's forward sweep along a random direction against the GPU's reverse sweep on the case's cotangents: the gap of
    the two sides relative to the sum of the left side's magnitudes, worst problem, against the float64 numpy pair's."""
    B, N, ny = nlp.B, nlp.N, inp["H"].shape[0]
    S0d, Wd, Vd = KS.directions(N + 3 * ny, ny, (B,))
    fwd = nlp.tracking_kalman_jvp(inp["Zout"], inp["L"], inp["H"], inp["V"], S0d, Wd, Vd, **inp["kw"])
    from quadruped_landing_amd import nlp as NL

    f = dict(Ld=TC.to_np(fwd["Lgain"]), Pd=NL.unpack_covariance(fwd["Pest"]), logdet=TC.to_np(fwd["logdet"]))

    def gap(f, r):
        lhs, rhs = KV.inner(inp["cot"], f, r, (S0d, Wd, Vd))
        mag, _ = KV.inner(tuple(np.abs(c) for c in inp["cot"]), {k: np.abs(v) for k, v in f.items()}, r, (S0d, Wd, Vd))
        return float(np.max(np.abs(lhs - rhs) / mag))

    gpu = gap(f, _host(got))
    Lh = TC.to_np(inp["L"])
    own = gap(KS.sweep(inp["A"], inp["H"], inp["V"], Lh, S0d, Wd, Vd), KV.sweep(inp["A"], inp["H"], inp["V"], Lh, *inp["cot"]))
    print(f"duality {tag}: the two kernels {gpu:.2e}, the float64 numpy pair {own:.2e}, of the left side's magnitudes")
    assert gpu <= 10 * own, (gpu, own)


@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,second", CASES)
def test_duality_of_the_two_kernels(kind, B, N, k_trans, im, ny, second):
    nlp, inp, got, _, _ = _run(kind, B, N, k_trans, im, ny, second)
    _duality(nlp, inp, got, f"{kind} B={B} N={N} ny={ny}")


@pytest.mark.parametrize("N,im,B,wm,ny", GUARDED)
def test_guarded_duality_of_the_two_kernels(N, im, B, wm, ny):
    nlp, inp, got, _, _ = _run_guarded(N, im, B, wm, ny)
    _duality(nlp, inp, got, f"guarded N={N} B={B} ny={ny}")


# ---- 3. bit for bit ------------------------------------------------------------------------------------------------------
def _both(i):
    return [(_run, CASES[i]), (_run_guarded, GUARDED[i % len(GUARDED)])]


@pytest.mark.parametrize("form", [0, 1], ids=["scheduled", "guarded"])
def test_a_null_cotangent_is_explicit_zeros(form):
    import torch

    run, case = _both(1)[form]
    nlp, inp, _, _, _ = run(*case)
    zeros = tuple(torch.zeros_like(c) for c in inp["dcot"])
    for keep in (s for k in (1, 2) for s in itertools.combinations(range(3), k)):
        some = nlp.tracking_kalman_vjp(inp["Zout"], inp["L"], inp["H"], inp["V"],
                                       *(inp["dcot"][i] if i in keep else None for i in range(3)), **inp["kw"])
        full = nlp.tracking_kalman_vjp(inp["Zout"], inp["L"], inp["H"], inp["V"],
                                       *(inp["dcot"][i] if i in keep else zeros[i] for i in range(3)), **inp["kw"])
        assert all(torch.equal(some[k], full[k]) for k in OUT), keep


@pytest.mark.parametrize("form", [0, 1], ids=["scheduled", "guarded"])
def test_every_subset_of_outputs_has_the_bits_of_the_full_call(form):
    import torch

    run, case = _both(0)[form]
    nlp, inp, got, _, _ = run(*case)
    for want in (c for k in (1, 2) for c in itertools.combinations(OUT, k)):
        part = nlp.tracking_kalman_vjp(inp["Zout"], inp["L"], inp["H"], inp["V"], *inp["dcot"], want=want, **inp["kw"])
        assert sorted(part) == sorted(want)
        assert all(torch.equal(part[k], got[k]) for k in want)
    red = nlp.tracking_kalman_vjp(inp["Zout"], inp["L"], inp["H"], inp["V"], *inp["dcot"], reduce=True, **inp["kw"])
    assert red["W"].shape == (15,) and red["V"].shape == (inp["H"].shape[0],) and torch.equal(red["Sigma0"], got["Sigma0"])
    assert torch.equal(red["W"], got["W"].sum(0)) and torch.equal(red["V"], got["V"].sum(0))


@pytest.mark.parametrize("form", [0, 1], ids=["scheduled", "guarded"])
def test_three_rows_are_eight_rows_with_zeros_written_out(form):
    import torch

    run, case = [(_run, CASES[0]), (_run_guarded, GUARDED[0])][form]
    nlp, inp, got, _, _ = run(*case)
    B, N = nlp.B, nlp.N
    assert inp["H"].shape[0] == 3
    H8, V8 = np.zeros((8, 15)), np.ones(8)
    H8[:3], V8[:3] = inp["H"], inp["V"]
    L8, Lb8 = (torch.zeros((B, N, 15, 8), dtype=torch.float64, device="cuda") for _ in range(2))
    L8[..., :3], Lb8[..., :3] = inp["L"], inp["dcot"][0]
    g8 = nlp.tracking_kalman_vjp(inp["Zout"], L8.contiguous(), H8, V8, Lb8.contiguous(), inp["dcot"][1], inp["dcot"][2], **inp["kw"])
    assert torch.equal(g8["Sigma0"], got["Sigma0"]) and torch.equal(g8["W"], got["W"])
    assert torch.equal(g8["V"][:, :3], got["V"])


@pytest.mark.parametrize("guarded", [False, True])
def test_host_forms_have_the_device_forms_bits_and_nan_where_nothing_is_read_changes_none(guarded):
    """z_stride = n_nlp + 2 is odd and leaves two slots of padding per problem.  NaN goes where nothing is read: that padding and
    the whole last knot (it has an update and no step).  The host form runs behind other host calls that left NaN in the staging
    buffers it shares by role."""
    import torch

    N, B, ny = 12, 70, 3
    batch, Zref, K, x0, th = GC.ragged_case(B=B, N=N)
    nlp = TC.nlp(batch, TC.SECOND_MODEL, z_stride=20 * N - 5 + 2)
    dm = EF.dev(th)
    Zout, ev = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), EF.dev(K), EF.dev(x0), dm)
    rng = np.random.default_rng(B)
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    H, V = EF.measurement(rng, ny)
    cot = KV.cotangents(3, N, ny, (B,))
    dcot = tuple(EF.dev(c) for c in cot)
    kw = dict(events=ev, model=dm, guarded=True) if guarded else {}
    L = (nlp.tracking_kalman_guarded(Zout, ev, H, V, None, S0, W, dm) if guarded else nlp.tracking_kalman(Zout, H, V, None, S0, W))[0]
    dev = nlp.tracking_kalman_vjp(Zout, L, H, V, *dcot, **kw)
    Zn = Zout.clone().view(B, -1)
    Zn[:, 20 * (N - 1):] = float("nan")
    again = nlp.tracking_kalman_vjp(Zn.reshape(-1), L, H, V, *dcot, **kw)
    assert all(torch.equal(again[k], dev[k]) for k in OUT)
    zh, evh, Lh = Zout.cpu().numpy(), ev.cpu().numpy(), L.cpu().numpy()
    nan = lambda *s: np.full(s, np.nan)  # noqa: E731
    with np.errstate(all="ignore"):
        nlp.tracking_kalman_host(nan(*zh.shape), np.ones((8, 15)), 1.0, None, nan(B, 120), None)
        nlp.tracking_kalman_jvp_host(nan(*zh.shape), nan(B, N, 15, 8), np.ones((8, 15)), 1.0, nan(B, 120), None, None)
    hkw = dict(events=evh, model=th, guarded=True) if guarded else {}
    host = nlp.tracking_kalman_vjp_host(zh, Lh, H, V, *cot, **hkw)
    for k in OUT:
        assert host[k].shape == dev[k].shape and np.array_equal(host[k], dev[k].cpu().numpy()), k
    one = nlp.tracking_kalman_vjp_host(zh, Lh, H, V, None, None, cot[2], want=("V",), **hkw)
    ref = nlp.tracking_kalman_vjp(Zout, L, H, V, None, None, dcot[2], want=("V",), **kw)
    assert sorted(one) == ["V"] and np.array_equal(one["V"], ref["V"].cpu().numpy())


@pytest.mark.parametrize("N,im,B", [(5, 2, 6), (17, 1, 3)])
def test_a_batch_that_never_lands_is_bitwise_the_knot_scheduled_call_of_a_handle_that_never_switches(N, im, B):
    import torch

    batch, Zref, K, x0, th = GC.case(N, im, B, True, False)
    iy, iv = GC.free_foot(im)
    Zref[:, 15 + (3 if im == 1 else 1)::20] = -2.0  # every problem gets the last problem's pulling reference
    x0[:, iy], x0[:, iv] = 0.3, 0.0
    nlp, never = TC.nlp(batch, TC.SECOND_MODEL), TC.nlp(GC.with_k_trans(batch, N + 1), TC.SECOND_MODEL)
    Zout, ev = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), EF.dev(K), EF.dev(x0))
    assert bool((ev[:, 0] == -1).all())
    rng = np.random.default_rng(N)
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    H, V = EF.measurement(rng, 3)
    dcot = tuple(EF.dev(c) for c in KV.cotangents(N, N, 3, (B,)))
    L = never.tracking_kalman(Zout, H, V, None, S0, W)[0]
    ref = never.tracking_kalman_vjp(Zout, L, H, V, *dcot)
    for model in (None, EF.dev(np.tile(TC.SECOND, (B, 1)))):
        got = nlp.tracking_kalman_vjp(Zout, L, H, V, *dcot, events=ev, model=model, guarded=True)
        assert all(torch.equal(got[k], ref[k]) for k in OUT)


# ---- 4. exact zeros and linearity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1], ids=["scheduled", "guarded"])
def test_a_cotangent_of_knot_0s_covariance_alone_leaves_exact_zeros_in_wdiag_bar(form):
    import torch

    run, case = _both(1)[form]
    nlp, inp, _, _, _ = run(*case)
    Pb = torch.zeros_like(inp["dcot"][1])
    Pb[:, 0] = inp["dcot"][1][:, 0]
    got = nlp.tracking_kalman_vjp(inp["Zout"], inp["L"], inp["H"], inp["V"], None, Pb, None, **inp["kw"])
    assert not bool(got["W"].any()) and bool(got["Sigma0"].any()) and bool(got["V"].any())


@pytest.mark.parametrize("form", [0, 1], ids=["scheduled", "guarded"])
def test_the_sweep_is_linear_in_the_cotangents(form):
    """sweep(a c1 + b c2) against a sweep(c1) + b sweep(c2), each output's worst entry relative to its largest.  The two sides
    differ by rounding alone, and how much rounding this check leaves is measured on the float64 yardstick, on the same
    cotangents and blocks: the kernel, whose sums run in another order, is allowed ten times that."""
    run, case = _both(2)[form]
    nlp, inp, got, _, _ = run(*case)
    B, N, ny = nlp.B, nlp.N, inp["H"].shape[0]
    a, b = 0.7, -1.3
    c1, c2 = inp["cot"], KV.cotangents(4242 + N, N, ny, (B,))
    mix = tuple(a * x + b * y for x, y in zip(c1, c2))
    dev = lambda c: _host(nlp.tracking_kalman_vjp(inp["Zout"], inp["L"], inp["H"], inp["V"], *(EF.dev(x) for x in c), **inp["kw"]))  # noqa: E731
    g1, g2, gm = _host(got), dev(c2), dev(mix)
    Lh = TC.to_np(inp["L"])
    y1, y2, ym = (KV.sweep(inp["A"], inp["H"], inp["V"], Lh, *c) for c in (c1, c2, mix))
    for k in OUT:
        gpu, _ = KV.out_rel(gm[k], a * g1[k] + b * g2[k])
        own, _ = KV.out_rel(ym[k], a * y1[k] + b * y2[k])
        print(f"linearity {'guarded' if form else 'scheduled'} B={B} N={N} ny={ny} {k}: the kernel {gpu:.2e}, the float64 yardstick {own:.2e}")
        assert gpu <= 10 * own, (k, gpu, own)


# ---- 5. the gradient of the likelihood -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _record(guarded):
    """A flown record (landing_filter_sweep_ref.record) at N = 5, ny = 3; the design runs along the record's reference at the
    handle's model and schedule, the filter replays the record at the records' own models.  The GPU's design, filter and
    gradient, and everything the numpy compositions need at the GPU's own gains, estimates and innovations."""
    N, ny, B = 5, 3, 5
    batch, rec = FS.record(N, 1, max(2, N // 3), B, ny, guarded, seed=40 + N)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    H, V = rec["H"], 1e-4 * (1.0 + 0.25 * np.arange(ny))
    rng = np.random.default_rng(N)
    S0, W = 1e-4 * CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-6, size=15)
    Zref, Zrec = nlp.upload_Z(rec["Zref"]), nlp.upload_Z(rec["Zrec"])
    Y, xh0, model = EF.dev(rec["Y"]), EF.dev(rec["xhat0"]), EF.dev(rec["model"])
    L = nlp.tracking_kalman(Zref, H, V, None, S0, W)[0]
    filt = nlp.landing_filter_guarded if guarded else nlp.landing_filter
    f = filt(Zref, Zrec, L, H, Y, V, xh0, model=model)
    evh = f[4] if guarded else None
    args = (Zref, Zref, Zrec, L, H, V, f[0], f[1])
    kw = dict(events_hat=evh, guarded=guarded, filter_model=model)
    grad = nlp.landing_loglik_grad(*args, **kw)
    blocks, zr = TC.evaluator_blocks(nlp, Zref), TC.rows(nlp, Zref)
    A = np.stack([blocks(b, zr[b])[:, :, :15] for b in range(B)])
    im, kt = np.asarray(batch.init_mode), np.asarray(batch.k_trans)
    Lh, Xh, ih = TC.to_np(L), TC.to_np(f[0]), TC.to_np(f[1])
    eh = None if evh is None else evh.cpu().numpy()
    F, T = FS.blocks(N, im, kt, rec["Zrec"], Xh, rec["model"], guarded, eh)
    return dict(nlp=nlp, args=args, kw=kw, grad=grad, A=A, F=F, T=T, L=Lh, innov=ih, H=H, V=V, evh=eh, ny=ny, B=B)


def _numpy_grad(r, dt):
    F, A, L, innov = _cast(dt, r["F"], r["A"], r["L"], r["innov"])
    vjp = lambda ib: FS.sweep_vjp(F, L, r["H"], innov, None, innov_bar=ib)["Lgain_bar"]  # noqa: E731
    return KV.loglik_grad(A, F, L, r["H"], r["V"].astype(dt), innov, vjp)


@pytest.mark.parametrize("guarded", [False, True])
def test_landing_loglik_grad_against_forward_mode_on_the_unit_directions(guarded):
    """Each entry of the W and V gradients, summed over nothing (per record), against the GPU's landing_loglik_jvp along that
    entry's unit direction: 15 + 3 forward calls.  The distance, relative to the record's largest entry, is allowed ten times
    the disagreement of the two numpy compositions (loglik_grad and the forward composite) on the same case."""
    r = _record(guarded)
    nlp, ny, B = r["nlp"], r["ny"], r["B"]
    g = _host(r["grad"])
    assert g["Sigma0"].shape == (B, 120) and g["W"].shape == (B, 15) and g["V"].shape == (B, ny)
    gn = _numpy_grad(r, np.float64)
    fwd, fwd_np = [], []
    for p in range(15 + ny):
        Wd, Vd = np.zeros(15), np.zeros(ny)
        (Wd if p < 15 else Vd)[p - 15 if p >= 15 else p] = 1.0
        fwd.append(TC.to_np(nlp.landing_loglik_jvp(*r["args"], None, Wd, Vd, **r["kw"])[0]))
        s = KS.sweep(r["A"], r["H"], r["V"], r["L"], None, Wd, Vd)
        f = FS.sweep_jvp(r["F"], r["T"], r["L"], r["H"], r["innov"], None, r["evh"], Lgain_dot=s["Ld"])
        fwd_np.append(KS.composite(r["innov"], f["innov_dot"], r["L"], s["Ld"], r["H"], r["V"], Vd, s["logdet"])[0])
    fwd, fwd_np = np.stack(fwd, axis=1), np.stack(fwd_np, axis=1)  # (B, 15 + ny)
    rev, rev_np = np.concatenate([g["W"], g["V"]], axis=1), np.concatenate([gn["W"], gn["V"]], axis=1)
    dist = lambda x, y: float(np.max(np.abs(x - y) / np.abs(y).max(axis=1, keepdims=True)))  # noqa: E731
    gpu, own = dist(rev, fwd), dist(rev_np, fwd_np)
    print(f"loglik gradient guarded={guarded}: reverse to forward mode on the GPU {gpu:.2e}, in float64 numpy {own:.2e}, of the "
          "record's largest entry")
    assert gpu <= 10 * own, (gpu, own)


@pytest.mark.parametrize("guarded", [False, True])
def test_landing_loglik_grad_against_the_numpy_composition(guarded):
    """At the GPU's own gains, estimates and innovations: each output's worst entry relative to its largest against the
    longdouble numpy composition, at most ten times the float64 numpy composition's own distance, both floored at 1e-13."""
    r = _record(guarded)
    g, lo, hi = _host(r["grad"]), _numpy_grad(r, np.float64), _numpy_grad(r, LD)
    for k in OUT:
        e, _ = KV.out_rel(g[k], hi[k])
        own, _ = KV.out_rel(lo[k], hi[k])
        print(f"loglik gradient guarded={guarded} {k}: the GPU to the longdouble composition {e:.2e}, float64 numpy {own:.2e}")
        assert max(e, FLOOR) <= 10 * max(own, FLOOR), (k, e, own)


# ---- 6. refusals that need the handle ------------------------------------------------------------------------------------
def test_refusals_behind_the_handle():
    import torch

    from quadruped_landing_amd import _lib

    nlp, inp, got, _, _ = _run_guarded(*GUARDED[0])
    L, h, INV, OK = _lib.lib(), nlp._h, _lib.QLN_ERR_INVALID_ARGUMENT, _lib.QLN_OK
    B, N, ny = nlp.B, nlp.N, inp["H"].shape[0]
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    a = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    Hd = EF.dev(inp["H"])
    Lb, Pb, lb = inp["dcot"]
    S0b, Wb, Vb = f64(B, 120), f64(B, 15), f64(B, ny)
    V = inp["V"]
    vjp, gvjp = L.qln_noise_design_vjp, L.qln_noise_design_guarded_vjp
    Z, Lg, ev, dm = inp["Zout"], inp["L"], inp["ev"], inp["model"]
    assert vjp(h, None, p(Lg), p(Hd), ny, a(V), p(Lb), p(Pb), p(lb), p(S0b), None, None) == INV
    assert b"null Zout" in L.qln_last_error()
    assert gvjp(h, p(Z), p(dm), None, p(Lg), p(Hd), ny, a(V), p(Lb), p(Pb), p(lb), p(S0b), None, None) == INV
    assert b"null event" in L.qln_last_error()
    for outs in ((p(Lg), None, None), (None, p(Z), None), (None, None, p(lb)), (p(Hd), None, None), (p(Pb), None, None)):
        assert vjp(h, p(Z), p(Lg), p(Hd), ny, a(V), p(Lb), p(Pb), p(lb), *outs) == INV
        assert b"overlaps an input" in L.qln_last_error()
    assert vjp(h, p(Z), p(Lg), p(Hd), ny, a(V), p(Lb), p(Pb), p(lb), p(S0b), p(S0b), None) == INV
    assert b"two outputs" in L.qln_last_error()
    assert gvjp(h, p(Z), p(dm), p(ev), p(Lg), p(Hd), ny, a(V), p(Lb), p(Pb), p(lb), None, None, p(ev)) == INV
    assert gvjp(h, p(Z), p(dm), p(ev), p(Lg), p(Hd), ny, a(V), p(Lb), p(Pb), p(lb), p(S0b), p(Wb), p(Vb)) == OK
    torch.cuda.synchronize()
    assert all(torch.equal(x, got[k]) for x, k in zip((S0b, Wb, Vb), OUT))
    # host forms: the same, and the values of H, of the record and of the models
    zo, evh, th, Lh, Hh = Z.cpu().numpy(), inp["evh"], dm.cpu().numpy(), Lg.cpu().numpy(), np.array(inp["H"])
    Lbh, So = inp["cot"][0], np.zeros((B, 120))
    hj, hg = L.qln_noise_design_vjp_host, L.qln_noise_design_guarded_vjp_host
    for value in (np.nan, np.inf):
        bad = Hh.copy()
        bad[ny - 1, 14] = value
        assert hj(h, a(zo), a(Lh), a(bad), ny, a(V), a(Lbh), None, None, a(So), None, None) == INV
        assert b"H is not finite" in L.qln_last_error()
    for entry, value in ((0, 0.5), (0, float(N - 1)), (1, -1e-3), (1, np.nan)):
        bad = np.array(evh)
        bad[B - 2, entry] = value
        assert hg(h, a(zo), None, a(bad), a(Lh), a(Hh), ny, a(V), a(Lbh), None, None, a(So), None, None) == INV, (entry, value)
    for entry, value in ((0, np.nan), (1, 0.0), (3, np.inf)):
        bad = np.array(th)
        bad[3, entry] = value
        assert hg(h, a(zo), a(bad), a(evh), a(Lh), a(Hh), ny, a(V), a(Lbh), None, None, a(So), None, None) == INV, (entry, value)
    assert hg(h, a(zo), a(th), a(evh), a(Lh), a(Hh), ny, a(V), a(Lbh), None, None, a(So), None, None) == OK
    # the Python layer's own rules
    with pytest.raises(ValueError):
        nlp.tracking_kalman_vjp(Z, Lg, inp["H"], V)  # no cotangent
    with pytest.raises(ValueError):
        nlp.tracking_kalman_vjp(Z, Lg, inp["H"], V, Lb, want=("Sigma0", "bogus"))
    with pytest.raises(ValueError):
        nlp.tracking_kalman_vjp(Z, Lg, inp["H"], V, Lb, want=())
