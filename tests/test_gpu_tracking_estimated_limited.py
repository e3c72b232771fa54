"""qln_tracking_rollout_estimated_limited and its sweeps on the GPU: the estimate-feedback roll-out within contact-aware force
limits (include/qln_evaluator.h).  The yardstick is tests/rollout_estimated_limited_ref.py, held on the CPU by
tests/test_rollout_estimated_limited_host.py, which also runs every case of this module on the yardstick alone.  Besides it the
kernels are held without an oracle: by the five exact reductions of the header, by the clamp's own properties, by the duality
identity between the two sweeps, by exact zeros on the saturated channels, by the host forms and through torch autograd."""
import functools
import itertools

import numpy as np
import pytest

from tests import estimation_cases as EF
from tests import rollout_estimated_limited_ref as XR
from tests import rollout_estimated_sweep_ref as ES
from tests import rollout_limited_ref as LR
from tests import rollout_ref as RR
from tests import tracking_cases as TC
from tests.estimation_cases import JVP_OUT, VJP_OUT

pytestmark = pytest.mark.gpu
_time_limit = EF.time_limit(600)

BAR = 1e-10          # the family's bar for a roll-out, in rollout_ref.rel (tests/test_gpu_tracking_estimated.py)
SWEEP_BAR = 1e-12    # the family's bar for a sweep against numpy, of max(1, |ref|) (tests/test_gpu_tracking_estimated_sweeps.py)
DUALITY_BAR = 1e-12  # the family's bar for the duality identity between the two kernels
LIM = XR.TEST_LIMITS
ALL = [(False,) + c for c in XR.SCHEDULED] + [(True,) + c for c in XR.GUARDED]
# the sweeps' cases: tests/test_gpu_tracking_estimated_sweeps.py's (guarded, N, init_mode, k_trans, B, ny)
SWEEPS = [(False, 5, 1, 2, 7, 3), (False, 5, 2, 4, 67, 8), (False, 5, 1, 5, 67, 1), (True, 5, 1, 2, 7, 3), (True, 5, 2, 2, 67, 8),
          (True, 5, 1, 2, 67, 1), (False, 61, 1, 21, 5, 8), (True, 61, 1, 21, 5, 3)]
SWEEP_FLAGS = list(itertools.product((False, True), repeat=3))  # with K, model, xhat0
NAMES = ("Zout", "Xhat", "innov", "events", "events_hat", "sat")


def _call(nlp, Zref_d, inp, x0, guarded, lim=LIM, **kw):
    return nlp.tracking_rollout_estimated_limited(Zref_d, lim, EF.dev(inp["K"]), EF.dev(inp["Lgain"]), inp["H"], EF.dev(inp["vnoise"]),
                                                  EF.dev(inp["wnoise"]), EF.dev(x0), EF.dev(inp["xhat0"]), EF.dev(inp["model"]),
                                                  guarded=guarded, with_innovations=True, **kw)


def _host(nlp, got):
    return {n: (TC.rows(nlp, t) if n == "Zout" else t.cpu().numpy()) for n, t in zip(NAMES, got) if t is not None}


@functools.lru_cache(maxsize=None)
def _case(case):
    guarded = case[0]
    batch, Zref, x0, th, seed = XR.guarded_case(*case[1:]) if guarded else XR.scheduled_case(*case[1:])
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    return batch, Zref, x0, th, seed, nlp, nlp.upload_Z(Zref)


# ---- 2 and 3. against the yardstick, and the clamp's own properties -------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=str)
def test_roll_out_matches_the_yardstick_and_keeps_the_clamps_properties(case):
    """Every ny in {1, 3, 8} and every combination of K, model, wnoise and xhat0 under TEST_LIMITS.  Zout, Xhat, innov and both
    records within 1e-10 in rollout_ref.rel; sat and both touchdown knots equal.  A problem is left out only if one of its
    guard margins or its force margin is below MARGIN on the yardstick, at most LEFT_OUT of a case, decided before the GPU is
    asked.  Every call's yardstick sat holds codes 0, 1 and 2.  Every applied force is inside its pair, a clamped force has the
    limit's bits, and the plant's record's entry 6 is >= stand_y_lo.  Measured worst values: profiles/tracking_estimated_limited_tests.txt."""
    guarded = case[0]
    batch, Zref, x0, th, seed, nlp, Zref_d = _case(case)
    B, N = nlp.B, nlp.N
    worst, left = {}, 0
    for ny in XR.NYS:
        for flags in XR.FLAGS:
            inp = XR.call_inputs(seed + ny, B, N, ny, Zref, flags, th)
            ref = XR.call_rollout(batch, Zref, inp, x0, LIM, guarded)
            out = XR.left_out(ref, XR.MARGIN)
            assert out.mean() <= XR.LEFT_OUT, (ny, flags, int(out.sum()))
            left, keep = max(left, int(out.sum())), ~out
            assert min(XR.digit_shares(ref["sat"])) > 0, (ny, flags)  # channels free, on a lower and on an upper limit
            got = _host(nlp, _call(nlp, Zref_d, inp, x0, guarded))
            assert np.array_equal(got["sat"][keep], ref["sat"][keep]), (ny, flags)
            for n in ("Zout", "Xhat", "innov") + (("events", "events_hat") if guarded else ()):
                worst[n] = max(worst.get(n, 0.0), RR.rel(got[n][keep], ref[n][keep]))
            if guarded:
                assert np.array_equal(got["events"][keep, 0], ref["events"][keep, 0])
                assert np.array_equal(got["events_hat"][keep, 0], ref["events_hat"][keep, 0])
                assert (got["events"][:, 6] >= LIM[6]).all()
            else:
                assert "events" not in got and "events_hat" not in got
            # the clamp, on the GPU's own record: the plant's mode at each knot's start picks the pair
            F = np.concatenate([got["Zout"], np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :-1, 15:19]
            s = LR.unpack(got["sat"])
            if guarded:
                ks = got["events"][:, 0]
                landed = (ks[:, None] >= 0) & (np.arange(N - 1)[None, :] > ks[:, None])
                im = np.asarray(batch.init_mode)[:, None]
                stand1, stand2 = landed | (im == 1), landed | (im == 2)
            else:
                from oracle import np_oracle as O

                modes = np.stack([O.knot_modes(N, int(kt), int(m))[0] for kt, m in zip(batch.k_trans, batch.init_mode)])
                stand1, stand2 = np.isin(modes, (1, 3)), np.isin(modes, (2, 3))
            stand = np.stack([stand1, stand1, stand2, stand2], axis=-1)
            ax = np.array([0, 2, 0, 2])
            lo, hi = np.where(stand, LIM[4 + ax], LIM[ax]), np.where(stand, LIM[5 + ax], LIM[1 + ax])
            assert ((F >= lo) & (F <= hi)).all()
            assert np.array_equal(F[s == 1], lo[s == 1]) and np.array_equal(F[s == 2], hi[s == 2])
    print(f"estimated limited {case}: worst over ny in {XR.NYS} and the 16 combinations of K, model, wnoise, xhat0: " +
          ", ".join(f"{n} {e:.2e}" for n, e in worst.items()) + f"; at most {left} problems left out of a call")
    assert all(e <= BAR for e in worst.values()), worst


@pytest.mark.parametrize("case", ALL, ids=str)
def test_every_case_has_channels_on_both_limits_and_free_ones(case):
    """Over a case's calls the yardstick's sat holds code 1, code 2 and code 0, so that no case passes with no clamp active;
    the roll-out test above asserts the same of every single call.  The guarded cases hold them by
    rollout_guarded_cases.case's own reference; the knot-scheduled ones by the two problems whose reference is pushed past
    every limit at knot 0 (rollout_estimated_limited_ref.scheduled_case), without which the shapes with one knot and three
    problems would ride no upper limit."""
    guarded = case[0]
    batch, Zref, x0, th, seed, nlp, _ = _case(case)
    every = []
    for ny in XR.NYS:
        for flags in XR.FLAGS:
            inp = XR.call_inputs(seed + ny, nlp.B, nlp.N, ny, Zref, flags, th)
            every.append(XR.call_rollout(batch, Zref, inp, x0, LIM, guarded)["sat"])
    free, lower, upper = XR.digit_shares(np.concatenate(every))
    print(f"{case}: free {free:.3f}, lower {lower:.3f}, upper {upper:.3f}")
    assert free > 0 and lower > 0 and upper > 0, (free, lower, upper)


# ---- 1. the exact reductions ----------------------------------------------------------------------------------------------
RED = [ALL[3], ALL[6], ALL[13], ALL[17], ALL[19], ALL[22]]


@pytest.mark.parametrize("case", RED, ids=str)
def test_reduction_1_infinite_limits_give_the_unlimited_calls_bits(case):
    import torch

    guarded = case[0]
    batch, Zref, x0, th, seed, nlp, Zref_d = _case(case)
    for ny, flags in ((8, XR.FLAGS[-1]), (3, XR.FLAGS[5]), (1, XR.FLAGS[0])):
        inp = XR.call_inputs(seed + ny, nlp.B, nlp.N, ny, Zref, flags, th)
        got = _call(nlp, Zref_d, inp, x0, guarded, lim=XR.NO_LIMITS)
        ref = nlp.tracking_rollout_estimated(Zref_d, EF.dev(inp["K"]), EF.dev(inp["Lgain"]), inp["H"], EF.dev(inp["vnoise"]),
                                             EF.dev(inp["wnoise"]), EF.dev(x0), EF.dev(inp["xhat0"]), EF.dev(inp["model"]), guarded=guarded,
                                             with_innovations=True)
        for g, r in zip(got, ref):
            assert torch.equal(g, r)
        assert got[3] is None or guarded
        assert not bool(got[5].any())


@pytest.mark.parametrize("case", RED, ids=str)
def test_reduction_3_without_gains_and_process_noise_the_plant_flies_the_limited_roll_out(case):
    """K None and wnoise None: Zout, the plant's record and sat are tracking_rollout_limited's bits, whatever Lgain, H, vnoise
    and xhat0 are."""
    import torch

    guarded = case[0]
    batch, Zref, x0, th, seed, nlp, Zref_d = _case(case)
    for ny, wm, wx in ((8, True, True), (1, False, False)):
        inp = XR.call_inputs(seed + ny, nlp.B, nlp.N, ny, Zref, (False, wm, False, wx), th)
        got = _call(nlp, Zref_d, inp, x0, guarded)
        zo, ev, sat = nlp.tracking_rollout_limited(Zref_d, LIM, None, EF.dev(x0), EF.dev(inp["model"]), guarded=guarded)
        assert torch.equal(got[0], zo) and torch.equal(got[5], sat) and bool(sat.any())
        assert (ev is None and got[3] is None) or torch.equal(got[3], ev)


@pytest.mark.parametrize("case", [c for c in RED if not c[0]], ids=str)
def test_reduction_4_without_filter_gains_the_scheduled_estimate_stays_on_the_limited_nominal(case):
    """Lgain = 0, xhat0 None, wnoise None and Zref the limited open-loop roll-out under the handle's model: the estimate stays
    on Zref, and Zout and sat are tracking_rollout_limited(Zref, None, x0, model)'s bits whatever K is."""
    import torch

    batch, Zref, x0, th, seed, nlp, Zref_d = _case(case)
    B, N = nlp.B, nlp.N
    nominal, _, _ = nlp.tracking_rollout_limited(Zref_d, LIM)
    for ny, wm in ((8, True), (3, False)):
        inp = XR.call_inputs(seed + ny, B, N, ny, Zref, (True, wm, False, False), th)
        inp["Lgain"] = np.zeros_like(inp["Lgain"])
        got = _call(nlp, nominal, inp, x0, False)
        zo, _, sat = nlp.tracking_rollout_limited(nominal, LIM, None, EF.dev(x0), EF.dev(inp["model"]))
        assert torch.equal(got[0], zo) and torch.equal(got[5], sat)
        zr = np.concatenate([TC.rows(nlp, nominal), np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15]
        assert np.array_equal(got[1].cpu().numpy(), zr)


@pytest.mark.parametrize("guarded", [False, True])
def test_reduction_5_three_rows_are_eight_rows_with_zeros_and_every_subset_of_outputs_has_the_full_calls_bits(guarded):
    import torch

    case = (True, "shape", 8, 1, 48) if guarded else (False, 9, 40, 14, 1)
    batch, Zref, x0, th, seed, nlp, Zref_d = _case(case)
    B, N = nlp.B, nlp.N
    inp = XR.call_inputs(seed + 3, B, N, 3, Zref, XR.FLAGS[-1], th)
    big = dict(inp)
    big["H"], big["Lgain"], big["vnoise"] = np.zeros((8, 15)), np.zeros((B, N, 15, 8)), np.random.default_rng(1).normal(size=(B, N, 8))
    big["H"][:3], big["Lgain"][..., :3], big["vnoise"][..., :3] = inp["H"], inp["Lgain"], inp["vnoise"]
    full, b = _call(nlp, Zref_d, inp, x0, guarded), _call(nlp, Zref_d, big, x0, guarded)
    for n, p, q in zip(NAMES, full, b):
        assert (p is None and q is None) or torch.equal(p, q[..., :3] if n == "innov" else q), n
    assert bool(full[5].any())
    for we, wi, wv, ws in itertools.product((False, True), repeat=4):
        part = nlp.tracking_rollout_estimated_limited(Zref_d, LIM, EF.dev(inp["K"]), EF.dev(inp["Lgain"]), inp["H"], EF.dev(inp["vnoise"]),
                                                      EF.dev(inp["wnoise"]), EF.dev(x0), EF.dev(inp["xhat0"]), EF.dev(inp["model"]),
                                                      guarded=guarded, with_estimate=we, with_innovations=wi, with_events=wv,
                                                      with_sat=ws)
        assert torch.equal(part[0], full[0])
        for p, f, asked in zip(part[1:], full[1:], (we, wi, wv and guarded, wv and guarded, ws)):
            assert (p is None and not asked) or torch.equal(p, f)


# ---- 4. the sweeps ----------------------------------------------------------------------------------------------------------
def _jvp(nlp, d, dirs, sat=None, limited=True, **kw):
    if limited:
        return nlp.tracking_rollout_estimated_limited_jvp(d["Zref"], d["K"], d["Lgain"], d["H"], d["Zout"], d["Xhat"],
                                                          d["sat"] if sat is None else sat, d["innov"], d["model"], d["events"],
                                                          d["events_hat"], **dirs, **kw)
    return nlp.tracking_rollout_estimated_jvp(d["Zref"], d["K"], d["Lgain"], d["H"], d["Zout"], d["Xhat"], d["innov"], d["model"],
                                              d["events"] is not None, d["events"], d["events_hat"], **dirs, **kw)


def _vjp(nlp, d, cot, want, sat=None, limited=True):
    if limited:
        return nlp.tracking_rollout_estimated_limited_vjp(d["Zref"], d["K"], d["Lgain"], d["H"], d["Zout"], d["Xhat"],
                                                          d["sat"] if sat is None else sat, cot["Zbar"], d["innov"], d["model"],
                                                          d["events"], d["events_hat"], cot["Xhat_bar"], cot["innov_bar"], want)
    return nlp.tracking_rollout_estimated_vjp(d["Zref"], d["K"], d["Lgain"], d["H"], d["Zout"], d["Xhat"], cot["Zbar"], d["innov"],
                                              d["model"], d["events"] is not None, d["events"], d["events_hat"], cot["Xhat_bar"],
                                              cot["innov_bar"], want)


@functools.lru_cache(maxsize=None)
def _run(guarded, N, im, kt, B, ny, flags):
    """One sweep case under one combination of present inputs: the GPU's limited roll-out, the yardstick's blocks at the GPU's
    own trajectory, records and sat, one direction and one cotangent, the yardstick's sweeps along them and its own
    float64-to-longdouble distance.  Shared by the tests of the case; nothing here is changed afterwards."""
    wk, wm, wx = flags
    batch, inp = ES.case(N, im, kt, B, ny, guarded)
    inp = dict(inp, K=inp["K"] if wk else None, model=inp["model"] if wm else None, xhat0=inp["xhat0"] if wx else None)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    d = {k: EF.dev(inp[k]) for k in ("K", "Lgain", "vnoise", "wnoise", "x0", "xhat0", "model")}
    d["Zref"], d["H"] = nlp.upload_Z(inp["Zref"]), inp["H"]
    got = nlp.tracking_rollout_estimated_limited(d["Zref"], LIM, d["K"], d["Lgain"], d["H"], d["vnoise"], d["wnoise"], d["x0"],
                                                 d["xhat0"], d["model"], guarded=guarded, with_innovations=True)
    d.update(zip(NAMES, got))
    h = dict(inp, **_host(nlp, got))
    h.setdefault("events"), h.setdefault("events_hat")
    th = TC.SECOND if inp["model"] is None else inp["model"]
    blocks = lambda ctype: ES.chain_blocks(N, np.asarray(batch.init_mode), np.asarray(batch.k_trans), h["Zout"], h["Xhat"], th,  # noqa: E731
                                           TC.SECOND, guarded, h["events"], h["events_hat"], ctype=ctype)
    blk, blkl = blocks(np.complex128), blocks(np.clongdouble)
    dirs, cot = ES.directions(1000 * N + 10 * kt + ny, B, N, ny)
    dirs = EF.present(inp, dirs)
    args = (h["sat"], h["Zref"], h["K"], h["Lgain"], h["H"], h["Zout"], h["Xhat"], h["innov"])
    ev = dict(events=h["events"], events_hat=h["events_hat"])
    ref_j, ref_v = XR.sweep_jvp(blk, *args, **dirs, **ev), XR.sweep_vjp(blk, *args, **cot, with_xhat0=wx)
    ext_j, ext_v = XR.sweep_jvp(blkl, *args, **dirs, **ev), XR.sweep_vjp(blkl, *args, **cot, with_xhat0=wx)
    dist = max([ES.worst(ref_j[k], ext_j[k]) for k in ref_j] + [ES.worst(ref_v[k], ext_v[k]) for k in ref_v if ref_v[k] is not None])
    bar = max(SWEEP_BAR, 100 * dist)
    if bar > SWEEP_BAR:
        print(f"guarded={guarded} N={N} B={B} flags={flags}: the yardstick is {dist:.2e} from its longdouble restatement: bar {bar:.2e}")
    return dict(nlp=nlp, d=d, h=h, dirs=dirs, cot=cot, ddirs=EF.upload(nlp, dirs), dcot=EF.upload(nlp, cot), ref_j=ref_j, ref_v=ref_v,
                bar=bar)


@pytest.mark.parametrize("guarded,N,im,kt,B,ny", SWEEPS)
def test_sweeps_match_the_yardstick_and_saturated_channels_get_exact_zeros(guarded, N, im, kt, B, ny):
    """Device JVP and VJP at the GPU's own trajectory and active set against the numpy sweeps on masked complex-step blocks,
    within max(1e-12, 100 x the float64 yardstick's distance to its longdouble restatement) of max(1, |ref|), in the eight
    combinations of K, model and xhat0.  The saturated channels' slots of Zout_dot, their rows of K_bar and their force slots of
    Zref_bar are exact zeros."""
    worst = 0.0
    for flags in SWEEP_FLAGS:
        r = _run(guarded, N, im, kt, B, ny, flags)
        nlp, d, h, wx = r["nlp"], r["d"], r["h"], flags[2]
        got = EF.host(nlp, JVP_OUT, _jvp(nlp, d, r["ddirs"]))
        assert ("event_dot" in got) == guarded and ("event_hat_dot" in got) == guarded
        gotv = EF.host(nlp, VJP_OUT, _vjp(nlp, d, r["dcot"], EF.want(h, wx)))
        assert ("xhat0_bar" in gotv) == wx and ("K_bar" in gotv) == flags[0]
        wj = {n: ES.worst(got[n], r["ref_j"][n]) for n in got}
        wv = {n: ES.worst(gotv[n], r["ref_v"][n]) for n in gotv}
        w = max(*wj.values(), *wv.values())
        worst = max(worst, w)
        assert w <= r["bar"], (flags, wj, wv, r["bar"])
        held = ~LR.free_channels(h["sat"])
        assert held.any() and (~held).any()
        slots = lambda z: np.concatenate([z, np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :-1, 15:19]  # noqa: E731
        assert not slots(got["Zout_dot"])[held].any() and not slots(gotv["Zref_bar"])[held].any()
        assert slots(gotv["Zref_bar"])[~held].all()
        if flags[0]:
            assert not gotv["K_bar"][held].any() and gotv["K_bar"][~held].any()
    print(f"limited sweeps guarded={guarded} N={N} mode={im} k_trans={kt} B={B} ny={ny}: worst of both sweeps over the 8 combinations "
          f"{worst:.2e}; bar {r['bar']:.2e}")
    if guarded:
        assert (h["events"][:, 0] >= 0).any() and (h["events_hat"][:, 0] >= 0).any()


@pytest.mark.parametrize("wx", [True, False])
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", SWEEPS)
def test_duality_between_the_two_kernels(guarded, N, im, kt, B, ny, wx):
    """<Zbar, Zout_dot> + <Xhat_bar, Xhat_dot> + <innov_bar, innov_dot> = the six products on the other side: no oracle."""
    import torch

    r = _run(guarded, N, im, kt, B, ny, (True, True, wx))
    nlp, d = r["nlp"], r["d"]
    fwd = dict(zip(JVP_OUT, _jvp(nlp, d, r["ddirs"])))
    rev = dict(zip(VJP_OUT, _vjp(nlp, d, r["dcot"], EF.want(r["h"], wx))))
    dot = lambda a, b_: float(torch.dot(a.reshape(-1), b_.reshape(-1)))  # noqa: E731
    lhs = sum(dot(r["dcot"][c], fwd[o]) for c, o in (("Zbar", "Zout_dot"), ("Xhat_bar", "Xhat_dot"), ("innov_bar", "innov_dot")))
    rhs = sum(dot(rev[k[:-4] + "_bar"], v) for k, v in r["ddirs"].items())
    print(f"limited guarded={guarded} N={N} B={B} ny={ny} xhat0={wx}: lhs {lhs:.15e}, rhs {rhs:.15e}, difference "
          f"{abs(lhs - rhs) / (abs(lhs) + abs(rhs)):.2e}")
    assert abs(lhs - rhs) <= DUALITY_BAR * (abs(lhs) + abs(rhs)), (lhs, rhs)


@pytest.mark.parametrize("guarded,N,im,kt,B,ny", [SWEEPS[1], SWEEPS[4], SWEEPS[6], SWEEPS[7]])
def test_reduction_2_an_empty_active_set_gives_the_estimated_sweeps_bits(guarded, N, im, kt, B, ny):
    import torch

    for flags in ((True, True, True), (False, False, False)):
        r = _run(guarded, N, im, kt, B, ny, flags)
        nlp, d = r["nlp"], r["d"]
        zero = torch.zeros_like(d["sat"])
        for a, b in zip(_jvp(nlp, d, r["ddirs"], sat=zero), _jvp(nlp, d, r["ddirs"], limited=False)):
            assert (a is None and b is None) or torch.equal(a, b)
        want = EF.want(r["h"], flags[2])
        for a, b in zip(_vjp(nlp, d, r["dcot"], want, sat=zero), _vjp(nlp, d, r["dcot"], want, limited=False)):
            assert (a is None and b is None) or torch.equal(a, b)
        # and a sweep at the record differs from it: the mask is read
        assert not torch.equal(_jvp(nlp, d, r["ddirs"])[0], _jvp(nlp, d, r["ddirs"], sat=zero)[0])


@pytest.mark.parametrize("guarded,N,im,kt,B", [(False, 5, 1, 3, 67), (True, 5, 2, 2, 67)])
def test_reduction_5_in_the_sweeps_three_rows_are_eight_rows_with_zeros_and_subsets_keep_their_bits(guarded, N, im, kt, B):
    import torch

    r = _run(guarded, N, im, kt, B, 3, (True, True, True))
    nlp, d, h = r["nlp"], r["d"], r["h"]
    dirs, cot = r["dirs"], r["cot"]
    pad = lambda a, axis: np.concatenate([a, np.zeros(a.shape[:axis] + (5,) + a.shape[axis + 1:])], axis=axis)  # noqa: E731
    d8 = dict(d, Lgain=EF.dev(pad(h["Lgain"], 3)), H=pad(h["H"], 0), innov=EF.dev(pad(h["innov"], 2)))
    dirs8, cot8 = dict(dirs, Lgain_dot=pad(dirs["Lgain_dot"], 3)), dict(cot, innov_bar=pad(cot["innov_bar"], 2))
    full = _jvp(nlp, d, r["ddirs"])
    for x, y, name in zip(full, _jvp(nlp, d8, EF.upload(nlp, dirs8)), JVP_OUT):
        assert (x is None and y is None and not guarded) or torch.equal(x, y[..., :3] if name == "innov_dot" else y), name
    want = EF.want(h, True)
    fullv = _vjp(nlp, d, r["dcot"], want)
    for x, y, name in zip(fullv, _vjp(nlp, d8, EF.upload(nlp, cot8), want), VJP_OUT):
        assert torch.equal(x, y[..., :3] if name == "Lgain_bar" else y), name
    for we, wi, wd in itertools.product((False, True), repeat=3):
        part = _jvp(nlp, d, r["ddirs"], with_estimate=we, with_innovations=wi, with_event_dot=wd)
        for x, y, on in zip(part, full, (True, we, wi, wd and guarded, wd and guarded)):
            assert (x is None and not on) or torch.equal(x, y)
    rest = ("Zref", "K", "Lgain", "x0", "model")
    for k in range(len(rest)):
        for sub in itertools.combinations(rest, k):
            part = _vjp(nlp, d, r["dcot"], sub + ("xhat0",))
            for x, y, n in zip(part, fullv, ("Zref", "K", "Lgain", "x0", "xhat0", "model")):
                assert (x is None and n not in sub and n != "xhat0") or torch.equal(x, y), (sub, n)


# ---- 5. torch autograd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,wx", [(False, True), (True, True), (True, False)])
def test_differentiable_estimated_rollout_with_limits_runs_the_limited_sweeps_in_both_modes(guarded, wx):
    import torch
    import torch.autograd.forward_ad as fwAD

    r = _run(guarded, 5, 2, 4 if not guarded else 2, 67, 8, (True, True, wx))
    nlp, d, dd, dc = r["nlp"], r["d"], r["ddirs"], r["dcot"]
    keys = ("Zref", "K", "Lgain", "x0", "xhat0", "model")
    leaves = {k: (None if d[k] is None else d[k].clone().requires_grad_(True)) for k in keys}
    call = lambda t: nlp.differentiable_estimated_rollout(t["Zref"], t["K"], t["Lgain"], d["H"], d["vnoise"], d["wnoise"], t["x0"],  # noqa: E731
                                                          t["xhat0"], t["model"], guarded=guarded, limits=LIM)
    out = call(leaves)
    assert len(out) == (6 if guarded else 4)
    for o, k in zip(out, ("Zout", "Xhat", "innov") + (("events", "events_hat") if guarded else ()) + ("sat",)):
        assert torch.equal(o, d[k]), k
    assert not any(o.requires_grad for o in out[3:]) and bool(out[-1].any())
    torch.autograd.backward(out[:3], [dc["Zbar"], dc["Xhat_bar"], dc["innov_bar"]])
    ref = _vjp(nlp, d, dc, EF.want(r["h"], wx))
    for k, g in zip(keys, ref):
        assert (leaves[k] is None and g is None) or torch.equal(leaves[k].grad.reshape(-1), g.reshape(-1)), k
    assert not torch.equal(ref[0], _vjp(nlp, d, dc, EF.want(r["h"], wx), limited=False)[0])  # and not the unlimited sweep
    refj = _jvp(nlp, d, dd)
    dot = lambda k: dd[k + "_dot"].reshape(d[k].shape)  # noqa: E731
    with fwAD.dual_level():
        duals = {k: (None if d[k] is None else fwAD.make_dual(d[k], dot(k))) for k in keys}
        tangents = [fwAD.unpack_dual(o).tangent for o in call(duals)[:3]]
    for t, g in zip(tangents, refj):
        assert torch.equal(t, g)
    present = [k for k in keys if d[k] is not None]
    fn = lambda *a: call(dict({k: None for k in keys}, **dict(zip(present, a))))[:3]  # noqa: E731
    outs, tangents = torch.func.jvp(fn, tuple(d[k] for k in present), tuple(dot(k) for k in present))
    for o, t, k, g in zip(outs, tangents, ("Zout", "Xhat", "innov"), refj):
        assert torch.equal(o, d[k]) and torch.equal(t, g)
    # backward against forward mode, gradcheck's statement at one direction and one cotangent
    lhs = sum(float(torch.dot(dc[c].reshape(-1), t.reshape(-1))) for c, t in zip(("Zbar", "Xhat_bar", "innov_bar"), tangents))
    rhs = sum(float(torch.dot(leaves[k].grad.reshape(-1), dot(k).reshape(-1))) for k in present)
    assert abs(lhs - rhs) <= DUALITY_BAR * (abs(lhs) + abs(rhs)), (lhs, rhs)


# ---- 6. the host forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 1024])  # mapped pinned buffers (small batch) and staged device copies
def test_host_forms_give_the_device_forms_bits_after_a_host_call_left_nans_behind(B):
    from tests import rollout_guarded_cases as GC

    N = 12
    batch, Zref, K, x0, th = GC.ragged_case(B=B, N=N)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Zref_d = nlp.upload_Z(Zref)
    zr = Zref_d.cpu().numpy()
    n, zs = nlp.n_nlp, nlp.z_stride
    nan = lambda *s: np.full(s, np.nan)  # noqa: E731
    pad = lambda a: np.concatenate([a, np.zeros((B, zs - n))], axis=1).reshape(-1)  # noqa: E731
    for ny, guarded in ((3, False), (8, True)):
        inp = XR.call_inputs(B + ny, B, N, ny, Zref, XR.FLAGS[-1], th)
        inp["K"] = K
        with np.errstate(all="ignore"):  # the roles this call reads and writes now hold NaN
            nlp.tracking_rollout_estimated_limited_host(nan(*zr.shape), LIM, nan(*K.shape), nan(B, N, 15, 8), np.ones((8, 15)),
                                                        nan(B, N, 8), nan(B, N - 1, 15), nan(B, 15), nan(B, 15), None, guarded=True,
                                                        with_innovations=True)
        dev = _call(nlp, Zref_d, inp, x0, guarded)
        host = nlp.tracking_rollout_estimated_limited_host(zr, LIM, inp["K"], inp["Lgain"], inp["H"], inp["vnoise"], inp["wnoise"],
                                                           x0, inp["xhat0"], inp["model"], guarded=guarded, with_innovations=True)
        for name, d_, h_ in zip(NAMES, dev, host):
            assert (d_ is None and h_ is None) or np.array_equal(h_.reshape(-1), d_.cpu().numpy().reshape(-1)), name
        assert host[5].any()
        # the sweeps, at that trajectory
        d = dict(zip(NAMES, dev), Zref=Zref_d, K=EF.dev(inp["K"]), Lgain=EF.dev(inp["Lgain"]), H=inp["H"], model=EF.dev(inp["model"]))
        h = dict(zip(NAMES, host))
        dirs, cot = ES.directions(8, B, N, ny)
        devj = _jvp(nlp, d, EF.upload(nlp, dirs))
        hostj = nlp.tracking_rollout_estimated_limited_jvp_host(zr, inp["K"], inp["Lgain"], inp["H"], h["Zout"], h["Xhat"], h["sat"],
                                                                h["innov"], inp["model"], h["events"], h["events_hat"],
                                                                **dict(dirs, Zref_dot=pad(dirs["Zref_dot"])))
        for name, x, y in zip(JVP_OUT, hostj, devj):
            assert (x is None and y is None) or np.array_equal(x.reshape(-1), y.cpu().numpy().reshape(-1)), name
        want = ("Zref", "K", "Lgain", "x0", "xhat0", "model")
        devv = _vjp(nlp, d, EF.upload(nlp, cot), want)
        hostv = nlp.tracking_rollout_estimated_limited_vjp_host(zr, inp["K"], inp["Lgain"], inp["H"], h["Zout"], h["Xhat"], h["sat"],
                                                                pad(cot["Zbar"]), h["innov"], inp["model"], h["events"],
                                                                h["events_hat"], cot["Xhat_bar"], cot["innov_bar"], want)
        for name, x, y in zip(VJP_OUT, hostv, devv):
            assert np.array_equal(x.reshape(-1), y.cpu().numpy().reshape(-1)), name


def test_invalid_arguments_are_refused_on_a_live_handle():
    import ctypes as C

    import torch

    from quadruped_landing_amd import _lib

    case = (True, "shape", 5, 2, 32)
    batch, Zref, x0, th, seed, nlp, Zr = _case(case)
    B, N = nlp.B, nlp.N
    L, h, INV, OK = _lib.lib(), nlp._h, _lib.QLN_ERR_INVALID_ARGUMENT, _lib.QLN_OK
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    Lg, Hd, Zo, Xo, ev, eh, sat = f64(B, N, 15, 8), f64(8, 15), nlp.new_Z(), f64(B, N, 15), f64(B, 8), f64(B, 8), f64(B, N - 1)
    lim = np.array(LIM)

    def call(guarded=1, event=ev, event_hat=eh, sat=sat, lim=lim, Xhat=Xo):
        return L.qln_tracking_rollout_estimated_limited(h, p(Zr), None, p(Lg), p(Hd), 8, None, None, None, None, None,
                                                        None if lim is None else lim.ctypes.data, guarded, p(Zo), p(Xhat), None,
                                                        p(event), p(event_hat), p(sat))

    assert call() == OK and call(sat=None, event=None, event_hat=None) == OK and call(guarded=0, event=None, event_hat=None) == OK
    assert call(guarded=0) == INV and call(guarded=0, event=None) == INV and call(lim=None) == INV
    assert call(sat=Zr) == INV and b"overlaps" in L.qln_last_error()
    assert call(sat=ev) == INV and call(Xhat=sat) == INV
    torch.cuda.synchronize()
    # the sweeps: sat among the inputs of the overlap rule, and its codes on the host
    zd, xd = nlp.new_Z(), f64(B, 15)
    args = lambda s: (h, p(Zr), None, p(Lg), p(Hd), 8, None, p(Zo), p(Xo), None, None, None, p(s))  # noqa: E731
    jv = lambda s, out: L.qln_tracking_rollout_estimated_limited_jvp(*args(s), None, None, None, p(xd), None, None, p(out), None,  # noqa: E731
                                                                     None, None, None)
    assert jv(sat, zd) == OK and jv(sat, sat) == INV and b"overlaps" in L.qln_last_error()
    zo, xh = Zo.cpu().numpy(), np.zeros((B, N, 15))
    for value in (3.0, 0.5, -1.0, 171.0, np.nan):
        bad = np.zeros((B, N - 1))
        bad[1, 2] = value
        with pytest.raises(_lib.QlnError):
            nlp.tracking_rollout_estimated_limited_jvp_host(zo, None, np.zeros((B, N, 15, 8)), np.ones((8, 15)), zo, xh, bad,
                                                            x0_dot=np.ones((B, 15)))
        with pytest.raises(_lib.QlnError):
            nlp.tracking_rollout_estimated_limited_vjp_host(zo, None, np.zeros((B, N, 15, 8)), np.ones((8, 15)), zo, xh, bad, zo)
