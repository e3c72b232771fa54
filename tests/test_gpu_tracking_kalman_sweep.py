"""qln_kalman_design_jvp / _guarded_jvp on the GPU: the forward sweep through the design of the Kalman filter
(include/qln_evaluator.h), at the gains the GPU's own tracking_kalman* returned.  The yardstick is
tests/tracking_kalman_sweep_ref.py, held on the CPU by tests/test_tracking_kalman_sweep_host.py; it runs on the evaluator's
dense blocks, and for the guarded call on the complex-step blocks of tests/rollout_guarded_sweep_ref.py.  Besides it the kernel
is held without an oracle: with zero gains it is bit for bit the open-loop covariance sweep, ny rows are eight rows with zeros
written out, every subset of outputs has the full call's bits, the host forms have the device forms' bits, it is linear in the
direction, and it agrees with central differences of the GPU's own design and of the GPU's own log-likelihood under redesign.
Shapes: tests/estimation_cases.py's.  Worst figures: profiles/tracking_kalman_jvp_tests.txt."""
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

pytestmark = pytest.mark.gpu
_time_limit = EF.time_limit(300)

BAR = 1e-10  # the family's bar; raised to 100 x the yardstick's own float64-to-longdouble distance where that is larger
OUT = ("Lgain", "Pest", "logdet")

# EF.design_shapes() and (a Sigma0_dot per problem, the handle at TC.SECOND_MODEL): the first takes turns, the second is one case
CASES = [c + (i % 4 < 2, i == 21) for i, c in enumerate(EF.design_shapes())] + [EF.RAGGED[0] + (True, False), EF.RAGGED[1] + (False, True)]
GUARDED = [s[1:] + (wm,) for s in EF.GUARDED_SHAPES for wm in (False, True)]  # (N, init_mode, B, a model per problem)


def _host(res):
    from quadruped_landing_amd import nlp as NL

    return dict(Ld=TC.to_np(res["Lgain"]), Pd=NL.unpack_covariance(res["Pest"]), logdet=TC.to_np(res["logdet"]))


def _reference(A_of, B, H, V, Lh, S0d, Wd, Vd, per_problem):
    """The float64 yardstick per problem at the GPU's gains, and its worst distance to its longdouble restatement per measure"""
    refs, dist = [], np.zeros(3)
    for b in range(B):
        A = A_of(b)
        s0d = S0d[b] if per_problem else S0d
        lo, hi = EF.in_both_precisions(KS.sweep, A, H, V, Lh[b], s0d, Wd, Vd)
        dist = np.maximum(dist, KS.errors(lo, hi))
        refs.append(lo)
    return {n: np.stack([r[n] for r in refs]) for n in ("Ld", "Pd", "logdet")}, dist


@functools.lru_cache(maxsize=None)
def _run(kind, B, N, k_trans, im, ny, per_problem, second):
    """One knot-scheduled case: the handle, the GPU's own design, one direction, the GPU's sweep and the yardstick's on the
    evaluator's dense blocks at the same Zout.  Shared by the case's tests, never changed."""
    d = EF.scheduled_design(kind, B, N, k_trans, im, ny, 5, **({"model": TC.SECOND_MODEL} if second else {}))
    nlp, Zout, H, V, S0, W = d.nlp, d.Zout, d.H, d.V, d.S0, d.W
    L, Pe, _, _ = nlp.tracking_kalman(Zout, H, V, None, S0, W)
    S0d, Wd, Vd = KS.directions(d.seed + 9, ny, (B,) if per_problem else ())
    got = nlp.tracking_kalman_jvp(Zout, L, H, V, S0d, Wd, Vd)
    ref, dist = _reference(lambda b: d.blocks(b, d.zo[b])[:, :, :15], B, H, V, TC.to_np(L), S0d, Wd, Vd, per_problem)
    inp = dict(Zout=Zout, L=L, H=H, V=V, S0=S0, W=W, S0d=S0d, Wd=Wd, Vd=Vd, blocks=d.blocks, zo=d.zo)
    return nlp, inp, got, ref, dist


@functools.lru_cache(maxsize=None)
def _run_guarded(N, im, B, wm):
    d = EF.guarded_design("shape", N, im, B, True, wm)
    nlp, Zout, ev, dm, H, V, S0, W = d.nlp, d.Zout, d.ev, d.model, d.H, d.V, d.S0, d.W
    L, Pe = nlp.tracking_kalman_guarded(Zout, ev, H, V, None, S0, W, dm)[:2]
    S0d, Wd, Vd = KS.directions(N + B, H.shape[0], (B,))
    got = nlp.tracking_kalman_jvp(Zout, L, H, V, S0d, Wd, Vd, events=ev, model=dm, guarded=True)
    A, _ = TG.split(d.F)
    ref, dist = _reference(lambda b: A[b], B, H, V, TC.to_np(L), S0d, Wd, Vd, True)
    inp = dict(Zout=Zout, ev=ev, evh=d.evh, model=dm, L=L, H=H, V=V, S0=S0, W=W, S0d=S0d, Wd=Wd, Vd=Vd)
    return nlp, inp, got, ref, dist


def _check(tag, got, ref, dist):
    g = _host(got)
    errs = KS.errors(g, ref)
    bars = [max(BAR, 100 * d) for d in dist]
    print(f"design sweep {tag}: Lgain_dot {errs[0]:.2e}, Pest_dot {errs[1]:.2e}, logdet_dot {errs[2]:.2e}; yardstick to longdouble "
          + ", ".join(f"{d:.2e}" for d in dist) + "; bars " + ", ".join(f"{b:.1e}" for b in bars))
    assert all(e <= b for e, b in zip(errs, bars)), (errs, bars)
    assert np.array_equal(g["Pd"], np.swapaxes(g["Pd"], -1, -2))
    assert all(np.isfinite(g[n]).all() for n in g)


# ---- 1. against the yardstick --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem,second", CASES)
def test_sweep_matches_the_yardstick(kind, B, N, k_trans, im, ny, per_problem, second):
    """Lgain_dot and Pest_dot in knot_rel, logdet_dot in entry_rel, every problem and knot included."""
    nlp, inp, got, ref, dist = _run(kind, B, N, k_trans, im, ny, per_problem, second)
    assert got["Lgain"].shape == (B, N, 15, ny) and got["Pest"].shape == (B, N, 120) and got["logdet"].shape == (B, N)
    _check(f"{kind} B={B} N={N} k_trans={k_trans} mode={im} ny={ny} sigma0_batch={B if per_problem else 1} second={second}",
           got, ref, dist)


@pytest.mark.parametrize("N,im,B,wm", GUARDED)
def test_guarded_sweep_matches_the_yardstick(N, im, B, wm):
    """On the complex-step blocks of the composite step, with and without a model per problem; the handle is at TC.SECOND_MODEL."""
    nlp, inp, got, ref, dist = _run_guarded(N, im, B, wm)
    assert (inp["evh"][:, 0] >= 0).any()
    _check(f"guarded N={N} mode={im} B={B} models={wm} ny={inp['H'].shape[0]}", got, ref, dist)


# ---- 2. no oracle, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem,second", [CASES[0], CASES[9], CASES[20], CASES[31], CASES[32]])
def test_with_zero_gains_pest_dot_is_the_open_loop_covariance_sweep(kind, B, N, k_trans, im, ny, per_problem, second):
    import torch

    nlp, inp, _, _, _ = _run(kind, B, N, k_trans, im, ny, per_problem, second)
    Wp = np.abs(inp["Wd"])
    got = nlp.tracking_kalman_jvp(inp["Zout"], torch.zeros_like(inp["L"]), inp["H"], inp["V"], inp["S0d"], Wp, None)
    Sr, _ = nlp.tracking_covariance(inp["Zout"], None, inp["S0d"], Wp, with_marginals=False)
    assert torch.equal(got["Pest"], Sr)
    assert bool(torch.isfinite(got["Lgain"]).all()) and bool(torch.isfinite(got["logdet"]).all())
    # Lgain_dot is then Pd^- H' / V: driven by Sigma0_dot at knot 0
    s0d = inp["S0d"] if per_problem else np.broadcast_to(inp["S0d"], (B, 15, 15))
    want = np.einsum("bij,rj->bir", s0d, inp["H"]) / inp["V"]
    assert CR.knot_rel(TC.to_np(got["Lgain"])[:, :1], want[:, None]) <= 1e-14


@pytest.mark.parametrize("N,im,B,wm", [(8, 1, 48, True), (40, 2, 9, True), (5, 2, 32, False)])
def test_guarded_with_zero_gains_pest_dot_is_the_guarded_open_loop_covariance_sweep(N, im, B, wm):
    import torch

    nlp, inp, _, _, _ = _run_guarded(N, im, B, wm)
    Wp = np.abs(inp["Wd"])
    got = nlp.tracking_kalman_jvp(inp["Zout"], torch.zeros_like(inp["L"]), inp["H"], inp["V"], inp["S0d"], Wp, None,
                                  events=inp["ev"], model=inp["model"], guarded=True)
    Sr = nlp.tracking_covariance_guarded(inp["Zout"], inp["ev"], None, inp["S0d"], Wp, inp["model"], with_marginals=False,
                                         with_event_var=False)[0]
    assert torch.equal(got["Pest"], Sr) and bool(torch.isfinite(got["logdet"]).all())


@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem,second", [c for c in CASES if c[5] == 3][::3])
def test_three_rows_are_eight_rows_with_zeros_written_out(kind, B, N, k_trans, im, ny, per_problem, second):
    import torch

    nlp, inp, got, _, _ = _run(kind, B, N, k_trans, im, ny, per_problem, second)
    H8, V8, Vd8 = np.zeros((8, 15)), np.ones(8), np.zeros(8)
    H8[:3], V8[:3], Vd8[:3] = inp["H"], inp["V"], inp["Vd"]
    L8 = torch.zeros((B, N, 15, 8), dtype=torch.float64, device="cuda")
    L8[..., :3] = inp["L"]
    g8 = nlp.tracking_kalman_jvp(inp["Zout"], L8.contiguous(), H8, V8, inp["S0d"], inp["Wd"], Vd8)
    assert torch.equal(g8["Pest"], got["Pest"]) and torch.equal(g8["logdet"], got["logdet"])
    assert torch.equal(g8["Lgain"][..., :3], got["Lgain"]) and not bool(g8["Lgain"][..., 3:].any())


def _subsets():
    return [c for k in (1, 2) for c in itertools.combinations(OUT, k)]


@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem,second", [CASES[2], CASES[21], CASES[32]])
def test_every_subset_of_outputs_has_the_bits_of_the_full_call(kind, B, N, k_trans, im, ny, per_problem, second):
    import torch

    nlp, inp, got, _, _ = _run(kind, B, N, k_trans, im, ny, per_problem, second)
    for want in _subsets():
        part = nlp.tracking_kalman_jvp(inp["Zout"], inp["L"], inp["H"], inp["V"], inp["S0d"], inp["Wd"], inp["Vd"], want=want)
        assert sorted(part) == sorted(want)
        assert all(torch.equal(part[k], got[k]) for k in want)


def test_guarded_subsets_of_outputs_have_the_bits_of_the_full_call():
    import torch

    nlp, inp, got, _, _ = _run_guarded(40, 1, 9, True)
    for want in _subsets():
        part = nlp.tracking_kalman_jvp(inp["Zout"], inp["L"], inp["H"], inp["V"], inp["S0d"], inp["Wd"], inp["Vd"],
                                       events=inp["ev"], model=inp["model"], guarded=True, want=want)
        assert all(torch.equal(part[k], got[k]) for k in want)


@pytest.mark.parametrize("guarded", [False, True])
def test_host_forms_have_the_device_forms_bits_and_nan_where_nothing_is_read_changes_none(guarded):
    """z_stride = n_nlp + 2 is odd and leaves two slots of padding per problem.  NaN goes where nothing is read: that padding and
    the last knot's states (the last knot has an update and no step).  The host form runs behind other host calls that left NaN
    in the staging buffers it shares by role."""
    import torch

    N, B, ny = 12, 70, 3
    batch, Zref, K, x0, th = GC.ragged_case(B=B, N=N)
    nlp = TC.nlp(batch, TC.SECOND_MODEL, z_stride=20 * N - 5 + 2)
    dm = EF.dev(th)
    Zout, ev = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), EF.dev(K), EF.dev(x0), dm)
    rng = np.random.default_rng(B)
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    H, V = EF.measurement(rng, ny)
    S0d, Wd, Vd = KS.directions(3, ny, (B,))
    kw = dict(events=ev, model=dm, guarded=True) if guarded else {}
    L = (nlp.tracking_kalman_guarded(Zout, ev, H, V, None, S0, W, dm) if guarded else nlp.tracking_kalman(Zout, H, V, None, S0, W))[0]
    dev = nlp.tracking_kalman_jvp(Zout, L, H, V, S0d, Wd, Vd, **kw)
    Zn = Zout.clone().view(B, -1)
    Zn[:, 20 * N - 5:] = float("nan")
    Zn[:, 20 * (N - 1): 20 * (N - 1) + 15] = float("nan")
    again = nlp.tracking_kalman_jvp(Zn.reshape(-1), L, H, V, S0d, Wd, Vd, **kw)
    assert all(torch.equal(again[k], dev[k]) for k in OUT)
    zh, evh, Lh = Zout.cpu().numpy(), ev.cpu().numpy(), L.cpu().numpy()
    nan = lambda *s: np.full(s, np.nan)  # noqa: E731
    with np.errstate(all="ignore"):
        nlp.tracking_kalman_host(nan(*zh.shape), np.ones((8, 15)), 1.0, None, nan(B, 120), None)
    hkw = dict(events=evh, model=th, guarded=True) if guarded else {}
    host = nlp.tracking_kalman_jvp_host(zh, Lh, H, V, S0d, Wd, Vd, **hkw)
    for k in OUT:
        assert np.array_equal(host[k], dev[k].cpu().numpy()), k
    one = nlp.tracking_kalman_jvp_host(zh, Lh, H, V, S0d[0], None, None, want=("logdet",), **hkw)
    ref = nlp.tracking_kalman_jvp(Zout, L, H, V, S0d[0], None, None, want=("logdet",), **kw)
    assert sorted(one) == ["logdet"] and np.array_equal(one["logdet"], ref["logdet"].cpu().numpy())


@pytest.mark.parametrize("N,im,B", [(8, 1, 48), (5, 2, 32)])
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
    S0d, Wd, Vd = KS.directions(N, 3, (B,))
    L = never.tracking_kalman(Zout, H, V, None, S0, W)[0]
    ref = never.tracking_kalman_jvp(Zout, L, H, V, S0d, Wd, Vd)
    for model in (None, EF.dev(np.tile(TC.SECOND, (B, 1)))):
        got = nlp.tracking_kalman_jvp(Zout, L, H, V, S0d, Wd, Vd, events=ev, model=model, guarded=True)
        assert all(torch.equal(got[k], ref[k]) for k in OUT)


# ---- 3. linearity and zeros ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem,second", [CASES[5], CASES[22], CASES[33]])
def test_the_sweep_is_linear_in_the_direction(kind, B, N, k_trans, im, ny, per_problem, second):
    """sweep(a d1 + b d2) against a sweep(d1) + b sweep(d2), worst of the three measures over all problems.  The two sides
    differ by rounding alone, and how much rounding this check leaves is measured on the float64 yardstick, on the same
    directions and blocks: the kernel, whose sums run in another order, is allowed ten times that."""
    nlp, inp, got, _, _ = _run(kind, B, N, k_trans, im, ny, per_problem, second)
    a, b = 0.7, -1.3
    d1 = (inp["S0d"], inp["Wd"], inp["Vd"])
    d2 = KS.directions(4242 + N, ny, (B,) if per_problem else ())
    mix = tuple(a * x + b * y for x, y in zip(d1, d2))
    run = lambda d: _host(nlp.tracking_kalman_jvp(inp["Zout"], inp["L"], inp["H"], inp["V"], *d))  # noqa: E731
    g1, g2, gm = _host(got), run(d2), run(mix)
    gpu = max(KS.errors(gm, {n: a * g1[n] + b * g2[n] for n in gm}))
    Lh = TC.to_np(inp["L"])
    own = 0.0
    for p in range(B):
        A = inp["blocks"](p, inp["zo"][p])[:, :, :15]
        pick = lambda d: (d[0][p] if per_problem else d[0], d[1], d[2])  # noqa: E731
        y1, y2, ym = (KS.sweep(A, inp["H"], inp["V"], Lh[p], *pick(d)) for d in (d1, d2, mix))
        own = max(own, *KS.errors(ym, {n: a * y1[n] + b * y2[n] for n in ym}))
    print(f"linearity B={B} N={N} ny={ny}: the kernel {gpu:.2e}, the float64 yardstick {own:.2e}")
    assert gpu <= 10 * own, (gpu, own)


def test_a_direction_behind_ny_cannot_be_expressed_and_process_noise_alone_leaves_knot_zero_at_zero():
    """V_dot has ny entries in the binding (a longer one is refused there), and the C entry reads ny of them: what stands behind
    is not a direction.  With W_dot alone the first knot's three outputs are exact zeros."""
    nlp, inp, got, _, _ = _run(*CASES[22])
    ny = inp["H"].shape[0]
    with pytest.raises(ValueError):
        nlp.tracking_kalman_jvp(inp["Zout"], inp["L"], inp["H"], inp["V"], None, None, np.ones(ny + 1))
    from quadruped_landing_amd import _lib

    B, N = nlp.B, nlp.N
    import torch

    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    Hd, V8, vd = EF.dev(inp["H"]), np.ones(8), np.zeros(8)
    V8[:ny], vd[:ny] = inp["V"], inp["Vd"]
    outs = []
    for tail in (0.0, 5.0):
        vd[ny:] = tail
        Ld, Pd, ld = f64(B, N, 15, ny), f64(B, N, 120), f64(B, N)
        rc = _lib.lib().qln_kalman_design_jvp(nlp._h, inp["Zout"].data_ptr(), inp["L"].data_ptr(), Hd.data_ptr(), ny,
                                               V8.ctypes.data, None, 1, None, vd.ctypes.data, Ld.data_ptr(), Pd.data_ptr(),
                                               ld.data_ptr())
        assert rc == _lib.QLN_OK
        outs.append((Ld, Pd, ld))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    only_w = nlp.tracking_kalman_jvp(inp["Zout"], inp["L"], inp["H"], inp["V"], None, inp["Wd"], None)
    assert all(not bool(only_w[k][:, 0].any()) for k in OUT)
    assert bool(only_w["Pest"][:, 1].any())


# ---- 4. the GPU's own quotient -------------------------------------------------------------------------------------------
STEPS = (1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6)


@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem,second", [CASES[16], CASES[33]])
def test_central_differences_of_the_gpus_own_design(kind, B, N, k_trans, im, ny, per_problem, second):
    """Central differences of the GPU's tracking_kalman (the filter alone) along the combined direction against the sweep's
    Lgain_dot and Pest_dot (the design does not return log det S_k).  The bar is ten times the error the same quotient leaves
    in float64 numpy at its best step, formed again on every run."""
    from quadruped_landing_amd import nlp as NL

    nlp, inp, got, ref, _ = _run(kind, B, N, k_trans, im, ny, per_problem, second)
    S0, W, V, S0d, Wd, Vd = (inp[k] for k in ("S0", "W", "V", "S0d", "Wd", "Vd"))
    s0d = S0d if per_problem else S0d[None]

    def cpu(t):
        worst = np.zeros(2)
        for b in range(B):
            A = inp["blocks"](b, inp["zo"][b])[:, :, :15]
            q = KS.design_quotient(A, inp["H"], V, S0[b], W, s0d[b if per_problem else 0], Wd, Vd, t, np.float64)
            worst = np.maximum(worst, (CR.knot_rel(q["Ld"], ref["Ld"][b]), CR.knot_rel(q["Pd"], ref["Pd"][b])))
        return worst

    table = np.array([cpu(t) for t in STEPS])
    g = _host(got)
    for col, name in enumerate(("Ld", "Pd")):
        i = int(np.argmin(table[:, col]))
        t = STEPS[i]
        p = nlp.tracking_kalman(inp["Zout"], inp["H"], V + t * Vd, None, S0 + t * s0d, W + t * Wd)
        m = nlp.tracking_kalman(inp["Zout"], inp["H"], V - t * Vd, None, S0 - t * s0d, W - t * Wd)
        if name == "Ld":
            q = (TC.to_np(p[0]) - TC.to_np(m[0])) / (2 * t)
        else:
            q = (NL.unpack_covariance(p[1]) - NL.unpack_covariance(m[1])) / (2 * t)
        e = CR.knot_rel(g[name], q)
        print(f"the GPU's quotient B={B} N={N} ny={ny}, {name}: {e:.2e} at t = {t:.0e}; float64 numpy leaves {table[i, col]:.2e}")
        assert e <= 10 * table[i, col], (name, e, table[:, col])


# ---- 5. the composite ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,guarded", [(5, False), (17, False), (5, True), (17, True)])
def test_landing_loglik_jvp_against_the_gpus_loglik_under_redesign(N, guarded):
    """A flown record (landing_filter_sweep_ref.record); the design runs along the record's reference at the handle's model and
    schedule, the filter replays the record at the records' own models.  loglik_dot against central differences of the GPU's
    loglik with the gains designed again at both offsets; no estimator's touchdown knot moves.  The bar is ten times the error
    the same quotient leaves in float64 numpy (the design on the evaluator's blocks, landing_filter_ref's replay) at its best
    step, against the numpy composition."""
    ny, B = 3, 5
    batch, rec = FS.record(N, 1, max(2, N // 3), B, ny, guarded, seed=40 + N)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    H, V = rec["H"], 1e-4 * (1.0 + 0.25 * np.arange(ny))
    rng = np.random.default_rng(N)
    S0, W = 1e-4 * CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-6, size=15)
    S0d, Wd, Vd = KS.directions(7 + N, ny, (B,))
    S0d, Wd, Vd = 1e-4 * S0d, 1e-4 * Wd, 1e-4 * Vd
    Zref, Zrec = nlp.upload_Z(rec["Zref"]), nlp.upload_Z(rec["Zrec"])
    Y, xh0, model = EF.dev(rec["Y"]), EF.dev(rec["xhat0"]), EF.dev(rec["model"])
    filt = nlp.landing_filter_guarded if guarded else nlp.landing_filter

    def gpu(s):
        L = nlp.tracking_kalman(Zref, H, V + s * Vd, None, S0 + s * S0d, W + s * Wd)[0]
        return (L,) + tuple(filt(Zref, Zrec, L, H, Y, V + s * Vd, xh0, model=model))

    c = gpu(0.0)
    ll, nd, ld = nlp.landing_loglik_jvp(Zref, Zref, Zrec, c[0], H, V, c[1], c[2], S0d, Wd, Vd,
                                        events_hat=c[5] if guarded else None, guarded=guarded, filter_model=model)
    assert ll.shape == (B,) and nd.shape == (B, N) and ld.shape == (B, N)
    # float64 numpy: the same quotient and the composition it is compared with, on the evaluator's blocks along Zref
    blocks, zr = TC.evaluator_blocks(nlp, Zref), TC.rows(nlp, Zref)
    A = np.stack([blocks(b, zr[b])[:, :, :15] for b in range(B)])
    im, kt = np.asarray(batch.init_mode), np.asarray(batch.k_trans)

    def cpu(s):
        d = KS.design(A, H, V + s * Vd, S0 + s * S0d, W + s * Wd, np.float64)
        return d, FS.replay(batch, rec, guarded, Lgain=d["L"], V=V + s * Vd)

    d0, r0 = cpu(0.0)
    F, T = FS.blocks(N, im, kt, rec["Zrec"], r0["Xhat"], rec["model"], guarded, r0.get("events_hat"))
    s = KS.sweep(A, H, V, d0["L"], S0d, Wd, Vd)
    f = FS.sweep_jvp(F, T, d0["L"], H, r0["innov"], None, r0.get("events_hat"), Lgain_dot=s["Ld"])
    ll_np, _ = KS.composite(r0["innov"], f["innov_dot"], d0["L"], s["Ld"], H, V, Vd, s["logdet"])
    left = []
    for t in STEPS:
        p, m = cpu(t)[1], cpu(-t)[1]
        left.append(CR.entry_rel((p["loglik"] - m["loglik"]) / (2 * t), ll_np))
    i = int(np.argmin(left))
    t = STEPS[i]
    p, m = gpu(t), gpu(-t)
    if guarded:
        assert bool((p[5][:, 0] == c[5][:, 0]).all()) and bool((m[5][:, 0] == c[5][:, 0]).all())
    q = (TC.to_np(p[4]) - TC.to_np(m[4])) / (2 * t)
    e = CR.entry_rel(TC.to_np(ll), q)
    print(f"loglik under redesign N={N} guarded={guarded}: landing_loglik_jvp to the GPU's quotient {e:.2e} at t = {t:.0e}; "
          f"float64 numpy leaves {left[i]:.2e}; to the numpy composition {CR.entry_rel(TC.to_np(ll), ll_np):.2e}")
    assert e <= 10 * left[i], (e, left)


# ---- 6. refusals that need the handle ------------------------------------------------------------------------------------
def test_refusals_behind_the_handle():
    import torch

    from quadruped_landing_amd import _lib

    nlp, inp, got, _, _ = _run_guarded(5, 2, 32, True)
    L, h, INV, OK = _lib.lib(), nlp._h, _lib.QLN_ERR_INVALID_ARGUMENT, _lib.QLN_OK
    B, N, ny = nlp.B, nlp.N, inp["H"].shape[0]
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    a = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    Hd, S0d = EF.dev(inp["H"]), f64(B, 120)
    Ld, Pd, ld = f64(B, N, 15, ny), f64(B, N, 120), f64(B, N)
    V, Wd, Vd = inp["V"], inp["Wd"], inp["Vd"]
    jvp, gjvp = L.qln_kalman_design_jvp, L.qln_kalman_design_guarded_jvp
    Z, Lg, ev, dm = inp["Zout"], inp["L"], inp["ev"], inp["model"]
    assert jvp(h, p(Z), p(Lg), p(Hd), ny, a(V), p(S0d), 2, a(Wd), a(Vd), p(Ld), None, None) == INV
    assert b"sigma0_batch" in L.qln_last_error()
    assert jvp(h, p(Z), p(Lg), p(Hd), ny, a(V), None, 2, a(Wd), a(Vd), p(Ld), None, None) == OK  # not read without Sigma0_dot
    assert jvp(h, None, p(Lg), p(Hd), ny, a(V), p(S0d), 1, a(Wd), a(Vd), p(Ld), None, None) == INV
    assert b"null Zout" in L.qln_last_error()
    assert gjvp(h, p(Z), p(dm), None, p(Lg), p(Hd), ny, a(V), p(S0d), 1, a(Wd), a(Vd), p(Ld), None, None) == INV
    assert b"null event" in L.qln_last_error()
    for outs in ((p(Lg), None, None), (None, p(Z), None), (None, None, p(S0d)), (p(Hd), None, None)):  # over an input
        assert jvp(h, p(Z), p(Lg), p(Hd), ny, a(V), p(S0d), B, a(Wd), a(Vd), *outs) == INV
        assert b"overlaps an input" in L.qln_last_error()
    assert jvp(h, p(Z), p(Lg), p(Hd), ny, a(V), p(S0d), B, a(Wd), a(Vd), p(Pd), p(Pd), None) == INV
    assert b"two outputs" in L.qln_last_error()
    assert gjvp(h, p(Z), p(dm), p(ev), p(Lg), p(Hd), ny, a(V), p(S0d), B, a(Wd), a(Vd), None, None, p(ev)) == INV
    assert gjvp(h, p(Z), p(dm), p(ev), p(Lg), p(Hd), ny, a(V), p(S0d), B, a(Wd), a(Vd), p(Ld), p(Pd), p(ld)) == OK
    torch.cuda.synchronize()
    # host forms: the same, and the values of H, of the record and of the models
    zo, evh, th, Lh, Hh = Z.cpu().numpy(), inp["evh"], dm.cpu().numpy(), Lg.cpu().numpy(), np.array(inp["H"])
    S0h, Lo = np.zeros((B, 120)), np.zeros((B, N, 15, ny))
    hj, hg = L.qln_kalman_design_jvp_host, L.qln_kalman_design_guarded_jvp_host
    assert hj(h, a(zo), a(Lh), a(Hh), ny, a(V), a(S0h), 3, a(Wd), a(Vd), a(Lo), None, None) == INV
    for value in (np.nan, np.inf):
        bad = Hh.copy()
        bad[ny - 1, 14] = value
        assert hj(h, a(zo), a(Lh), a(bad), ny, a(V), a(S0h), B, a(Wd), a(Vd), a(Lo), None, None) == INV
        assert b"H is not finite" in L.qln_last_error()
    for entry, value in ((0, 0.5), (0, float(N - 1)), (1, -1e-3), (1, np.nan)):
        bad = np.array(evh)
        bad[B - 2, entry] = value
        assert hg(h, a(zo), None, a(bad), a(Lh), a(Hh), ny, a(V), a(S0h), B, a(Wd), a(Vd), a(Lo), None, None) == INV, (entry, value)
    for entry, value in ((0, np.nan), (1, 0.0), (3, np.inf)):
        bad = np.array(th)
        bad[3, entry] = value
        assert hg(h, a(zo), a(bad), a(evh), a(Lh), a(Hh), ny, a(V), a(S0h), B, a(Wd), a(Vd), a(Lo), None, None) == INV, (entry, value)
    assert hg(h, a(zo), a(th), a(evh), a(Lh), a(Hh), ny, a(V), a(S0h), B, a(Wd), a(Vd), a(Lo), None, None) == OK
    # the Python layer's own rules
    with pytest.raises(ValueError):
        nlp.tracking_kalman_jvp(Z, Lg, inp["H"], V)  # no direction
    with pytest.raises(ValueError):
        nlp.tracking_kalman_jvp(Z, Lg, inp["H"], V, None, Wd, None, want=("Lgain", "bogus"))
    with pytest.raises(ValueError):
        nlp.tracking_kalman_jvp(Z, Lg, inp["H"], V, None, [np.nan] * 15, None)
