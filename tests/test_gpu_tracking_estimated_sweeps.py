"""qln_tracking_rollout_estimated_jvp / _vjp and their _guarded forms on the GPU: the forward and reverse sweeps through the
estimate-feedback roll-out (include/qln_evaluator.h).  The yardstick is tests/rollout_estimated_sweep_ref.py, held on the CPU
by tests/test_rollout_estimated_sweep_host.py.  Besides it the kernels are held without an oracle: by the adjoint identity
between them, bit for bit by the sibling sweeps where the filter gains are zero, by eight sensor rows with zeros written out,
by every subset of optional outputs, by the host forms, by central differences of the GPU's own roll-out where the plant and
the estimator land in different knots, and through torch autograd.  The cases and their seeds are the yardstick module's."""
import functools
import itertools

import numpy as np
import pytest

from tests import estimation_cases as EF
from tests import rollout_estimated_sweep_ref as ES
from tests import tracking_cases as TC
from tests.estimation_cases import JVP_OUT, VJP_OUT

pytestmark = pytest.mark.gpu
_time_limit = EF.time_limit(300)

SWEEP_BAR = 1e-12  # the project's bar for a sweep against numpy, of max(1, |ref|) (tests/test_gpu_rollout_guarded_sweeps.py)
# N = 5 with k_trans over 1..N and both init_modes, B = 7 (a part-filled wave) and 67 (several blocks, a ragged tail), ny over
# 1, 3, 8; one full-length case.  (guarded, N, init_mode, k_trans, B, ny); the guarded forms do not read k_trans.
SCHEDULED = [(False, 5, 1 + (kt + i) % 2, kt, (7, 67)[(kt + i) % 2], (1, 3, 8)[(kt + 2 * i) % 3]) for i in range(2)
             for kt in range(1, 6)]
GUARDED = [(True, 5, 1, 2, 7, 3), (True, 5, 2, 2, 67, 8), (True, 5, 1, 2, 67, 1), (True, 5, 2, 2, 7, 8)]
LONG = [(False, 61, 1, 21, 5, 8), (True, 61, 1, 21, 5, 3)]
CASES = SCHEDULED + GUARDED + LONG
FLAGS = list(itertools.product((False, True), repeat=3))  # with K, model, xhat0
# Test 4.  The same difference quotient in float64 numpy (rollout_estimated_ref.rollout at x0 +- FD_EPS x0_dot against the
# yardstick's sweep at the yardstick's own trajectory, the inputs of _split_case below, all 32 problems keeping both knots)
# leaves 6.39e-11 of max(1, |ref|) at 1e-4, its best step (1e-3: 2.4e-9, truncation; 1e-5: 5.0e-10, rounding): the bar is ten
# times that.  The test forms the number again on every run and holds it to the constant within a factor of two, so that the
# constant cannot go stale.
FD_EPS = 1e-4
FD_CPU_WORST = 6.39e-11
FD_BAR = 10 * FD_CPU_WORST


def _rollout(nlp, inp, guarded):
    """The GPU's roll-out of host inputs: (device dict, host dict) of its inputs and the trajectory."""
    d = {k: EF.dev(inp[k]) for k in ("K", "Lgain", "vnoise", "wnoise", "x0", "xhat0", "model")}
    d["Zref"], d["H"] = nlp.upload_Z(inp["Zref"]), inp["H"]
    got = nlp.tracking_rollout_estimated(d["Zref"], d["K"], d["Lgain"], d["H"], d["vnoise"], d["wnoise"], d["x0"], d["xhat0"],
                                         d["model"], guarded=guarded, with_innovations=True)
    d.update(zip(("Zout", "Xhat", "innov", "events", "events_hat"), got))
    d.setdefault("events"), d.setdefault("events_hat")
    h = dict(inp, Zout=TC.rows(nlp, d["Zout"]), Xhat=d["Xhat"].cpu().numpy(), innov=d["innov"].cpu().numpy(),
             events=TC.to_np(d["events"]), events_hat=TC.to_np(d["events_hat"]))
    return d, h


def _jvp(nlp, d, guarded, dirs, **kw):
    return nlp.tracking_rollout_estimated_jvp(d["Zref"], d["K"], d["Lgain"], d["H"], d["Zout"], d["Xhat"], d["innov"], d["model"],
                                              guarded, d["events"], d["events_hat"], **dirs, **kw)


def _vjp(nlp, d, guarded, cot, want=None, innov=True):
    return nlp.tracking_rollout_estimated_vjp(d["Zref"], d["K"], d["Lgain"], d["H"], d["Zout"], d["Xhat"], cot["Zbar"],
                                              d["innov"] if innov else None, d["model"], guarded, d["events"], d["events_hat"],
                                              cot["Xhat_bar"], cot["innov_bar"], want)


@functools.lru_cache(maxsize=None)
def _run(guarded, N, im, kt, B, ny, flags):
    """One case under one combination of present inputs: the GPU's roll-out, the yardstick's blocks at the GPU's own trajectory
    and records, one direction and one cotangent, the yardstick's sweeps along them and its own float64-to-longdouble distance.
    Shared by the tests of the case; nothing here is changed afterwards."""
    wk, wm, wx = flags
    batch, inp = ES.case(N, im, kt, B, ny, guarded)
    inp = dict(inp, K=inp["K"] if wk else None, model=inp["model"] if wm else None, xhat0=inp["xhat0"] if wx else None)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    d, h = _rollout(nlp, inp, guarded)
    th = TC.SECOND if inp["model"] is None else inp["model"]
    blocks = lambda ctype: ES.chain_blocks(N, np.asarray(batch.init_mode), np.asarray(batch.k_trans), h["Zout"], h["Xhat"], th,  # noqa: E731
                                           TC.SECOND, guarded, h["events"], h["events_hat"], ctype=ctype)
    blk, blkl = blocks(np.complex128), blocks(np.clongdouble)
    dirs, cot = ES.directions(1000 * N + 10 * kt + ny, B, N, ny)
    dirs = EF.present(inp, dirs)
    args = (h["Zref"], h["K"], h["Lgain"], h["H"], h["Zout"], h["Xhat"], h["innov"])
    ev = dict(events=h["events"], events_hat=h["events_hat"])
    ref_j, ref_v = ES.sweep_jvp(blk, *args, **dirs, **ev), ES.sweep_vjp(blk, *args, **cot, with_xhat0=wx)
    ext_j, ext_v = ES.sweep_jvp(blkl, *args, **dirs, **ev), ES.sweep_vjp(blkl, *args, **cot, with_xhat0=wx)
    dist = max([ES.worst(ref_j[k], ext_j[k]) for k in ref_j] + [ES.worst(ref_v[k], ext_v[k]) for k in ref_v if ref_v[k] is not None])
    bar = max(SWEEP_BAR, 100 * dist)
    if bar > SWEEP_BAR:
        print(f"guarded={guarded} N={N} B={B} flags={flags}: the yardstick is {dist:.2e} from its longdouble restatement: bar {bar:.2e}")
    return dict(nlp=nlp, d=d, h=h, blk=blk, dirs=dirs, cot=cot, ddirs=EF.upload(nlp, dirs), dcot=EF.upload(nlp, cot), ref_j=ref_j,
                ref_v=ref_v, bar=bar, args=args, ev=ev, batch=batch)


# ---- 1. against the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", CASES)
def test_sweeps_match_the_yardstick_in_every_combination_of_inputs(guarded, N, im, kt, B, ny):
    """Device JVP and VJP at the GPU's own trajectory against the numpy sweeps on complex-step blocks, within 1e-12 of
    max(1, |ref|) (or 100 times the yardstick's own float64-to-longdouble distance where that is more, printed when it is):
    every combination of present and absent among K, model, xhat0_dot / xhat0_bar and Lgain_dot / Lgain_bar with all the
    tangents that exist, and under the full combination each tangent alone.  Measured worst values:
    profiles/tracking_estimated_sweeps_tests.txt."""
    worst = 0.0
    for flags in FLAGS:
        r = _run(guarded, N, im, kt, B, ny, flags)
        nlp, d, h, wx = r["nlp"], r["d"], r["h"], flags[2]
        for lgain in (True, False):
            dirs = EF.present(h, r["dirs"], lgain)
            ref = r["ref_j"] if lgain else ES.sweep_jvp(r["blk"], *r["args"], **dirs, **r["ev"])
            got = EF.host(nlp, JVP_OUT, _jvp(nlp, d, guarded, EF.present(h, r["ddirs"], lgain)))
            wj = {n: ES.worst(got[n], ref[n]) for n in got}
            refv = r["ref_v"]
            gotv = EF.host(nlp, VJP_OUT, _vjp(nlp, d, guarded, r["dcot"], EF.want(h, wx, lgain), innov=lgain))
            assert ("Lgain_bar" in gotv) == lgain and ("xhat0_bar" in gotv) == wx and ("K_bar" in gotv) == flags[0]
            wv = {n: ES.worst(gotv[n], refv[n]) for n in gotv}
            w = max(*wj.values(), *wv.values())
            worst = max(worst, w)
            assert w <= r["bar"], (flags, lgain, wj, wv, r["bar"])
        if all(flags):
            for name in r["dirs"]:
                one = {name: r["dirs"][name]}
                if name != "xhat0_dot":
                    one["xhat0_dot"] = np.zeros((B, 15))  # a given xhat0 held fixed
                ref = ES.sweep_jvp(r["blk"], *r["args"], **one, **r["ev"])
                got = EF.host(nlp, JVP_OUT, _jvp(nlp, d, guarded, EF.upload(nlp, one)))
                w = max(ES.worst(got[n], ref[n]) for n in got)
                worst = max(worst, w)
                assert w <= r["bar"], (name, w, r["bar"])
    print(f"guarded={guarded} N={N} mode={im} k_trans={kt} B={B} ny={ny}: worst of both sweeps over the 16 combinations and the "
          f"single tangents {worst:.2e}; bar {r['bar']:.2e}")
    if guarded:
        assert (h["events"][:, 0] >= 0).any() and (h["events_hat"][:, 0] >= 0).any()


# ---- 2. the adjoint identity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wx", [True, False])
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", CASES)
def test_adjoint_identity_between_the_two_kernels(guarded, N, im, kt, B, ny, wx):
    """<Zbar, Zout_dot> + <Xhat_bar, Xhat_dot> + <innov_bar, innov_dot> = the six products on the other side, in both xhat0
    modes: no oracle involved."""
    import torch

    r = _run(guarded, N, im, kt, B, ny, (True, True, wx))
    nlp, d = r["nlp"], r["d"]
    fwd = dict(zip(JVP_OUT, _jvp(nlp, d, guarded, r["ddirs"])))
    rev = dict(zip(VJP_OUT, _vjp(nlp, d, guarded, r["dcot"], EF.want(r["h"], wx))))
    dot = lambda a, b_: float(torch.dot(a.reshape(-1), b_.reshape(-1)))  # noqa: E731
    lhs = sum(dot(r["dcot"][c], fwd[o]) for c, o in (("Zbar", "Zout_dot"), ("Xhat_bar", "Xhat_dot"), ("innov_bar", "innov_dot")))
    rhs = sum(dot(rev[k[:-4] + "_bar"], v) for k, v in r["ddirs"].items())
    assert (rev["xhat0_bar"] is None) == (not wx) and ("xhat0_dot" in r["ddirs"]) == wx
    print(f"guarded={guarded} N={N} B={B} ny={ny} xhat0={wx}: lhs {lhs:.15e}, rhs {rhs:.15e}, difference "
          f"{abs(lhs - rhs) / (abs(lhs) + abs(rhs)):.2e}")
    assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs)), (lhs, rhs)


# ---- 3. exact reductions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", [SCHEDULED[1], SCHEDULED[7], GUARDED[1], GUARDED[3], LONG[0], LONG[1]])
def test_without_filter_gains_the_plant_chain_is_bitwise_the_sibling_sweep(guarded, N, im, kt, B, ny):
    """Lgain = 0, no tangent of Lgain, xhat0 or Zref, and Zref a roll-out under the handle's model, so that Xhat is on Zref:
    the estimator's chain is zero, and Zout_dot is tracking_rollout_model_jvp's (tracking_rollout_guarded_jvp's with its
    event_dot) without gains on (x0_dot, model_dot), whatever K is; the reverse sweep's x0_bar and model_bar are the sibling's."""
    import torch

    batch, inp = ES.case(N, im, kt, B, ny, guarded)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Z0 = nlp.upload_Z(inp["Zref"])
    nominal = nlp.tracking_rollout_guarded(Z0)[0] if guarded else nlp.tracking_rollout_model(Z0)
    inp = dict(inp, Zref=TC.rows(nlp, nominal), Lgain=np.zeros_like(inp["Lgain"]), xhat0=None)
    d, h = _rollout(nlp, inp, guarded)
    zr = np.concatenate([h["Zref"], np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15]
    assert np.array_equal(h["Xhat"], zr)
    dirs, cot = ES.directions(5, B, N, ny)
    dd = EF.upload(nlp, {k: dirs[k] for k in ("x0_dot", "model_dot")})
    Zbar = nlp.upload_Z(cot["Zbar"])
    got = _jvp(nlp, d, guarded, dd)
    want = ("x0", "model")
    rev = nlp.tracking_rollout_estimated_vjp(d["Zref"], d["K"], d["Lgain"], d["H"], d["Zout"], d["Xhat"], Zbar, None, d["model"],
                                             guarded, d["events"], d["events_hat"], want=want)
    if guarded:
        ref, ed = nlp.tracking_rollout_guarded_jvp(d["Zref"], d["Zout"], d["events"], None, d["model"], None, None, dd["x0_dot"],
                                                   dd["model_dot"])
        assert torch.equal(got[3], ed) and bool(ed.any())
        _, _, xb, mb = nlp.tracking_rollout_guarded_vjp(d["Zref"], d["Zout"], d["events"], Zbar, None, d["model"])
    else:
        ref = nlp.tracking_rollout_model_jvp(d["Zref"], d["Zout"], None, d["model"], None, None, dd["x0_dot"], dd["model_dot"])
        _, _, xb, mb = nlp.tracking_rollout_model_vjp(d["Zref"], d["Zout"], Zbar, None, d["model"])
    assert torch.equal(got[0], ref) and bool(ref.any())
    assert not bool(got[1].any())  # the estimate's tangent is zero
    assert torch.equal(rev[3], xb) and torch.equal(rev[5], mb) and bool(mb.any())


@pytest.mark.parametrize("guarded,N,im,kt,B", [(False, 5, 1, 3, 67), (True, 5, 2, 2, 67), (False, 61, 1, 21, 5)])
def test_three_sensor_rows_are_bitwise_eight_rows_with_zeros(guarded, N, im, kt, B):
    import torch

    batch, inp = ES.case(N, im, kt, B, 3, guarded)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    d, h = _rollout(nlp, inp, guarded)
    dirs, cot = ES.directions(6, B, N, 3)
    pad = lambda a, axis: np.concatenate([a, np.zeros(a.shape[:axis] + (5,) + a.shape[axis + 1:])], axis=axis)  # noqa: E731
    d8 = dict(d, Lgain=EF.dev(pad(inp["Lgain"], 3)), H=pad(inp["H"], 0), innov=EF.dev(pad(h["innov"], 2)))
    dirs8, cot8 = dict(dirs, Lgain_dot=pad(dirs["Lgain_dot"], 3)), dict(cot, innov_bar=pad(cot["innov_bar"], 2))
    a, b = _jvp(nlp, d, guarded, EF.upload(nlp, dirs)), _jvp(nlp, d8, guarded, EF.upload(nlp, dirs8))
    for x, y, name in zip(a, b, JVP_OUT):
        assert torch.equal(x, y[..., :3] if name == "innov_dot" else y), name
    assert not bool(b[2][..., 3:].any())
    a, b = _vjp(nlp, d, guarded, EF.upload(nlp, cot)), _vjp(nlp, d8, guarded, EF.upload(nlp, cot8))
    for x, y, name in zip(a, b, VJP_OUT):
        assert torch.equal(x, y[..., :3] if name == "Lgain_bar" else y), name
    assert not bool(b[2][..., 3:].any())


@pytest.mark.parametrize("guarded,N,im,kt,B,ny", [SCHEDULED[3], GUARDED[1]])
def test_every_subset_of_optional_outputs_leaves_the_others_bits(guarded, N, im, kt, B, ny):
    import torch

    r = _run(guarded, N, im, kt, B, ny, (True, True, True))
    nlp, d = r["nlp"], r["d"]
    full = _jvp(nlp, d, guarded, r["ddirs"])
    for we, wi, wd in itertools.product((False, True), repeat=3):
        got = _jvp(nlp, d, guarded, r["ddirs"], with_estimate=we, with_innovations=wi, with_event_dot=wd)
        for x, y, on in zip(got, full, (True, we, wi, wd, wd)):
            assert (x is None and not on) or torch.equal(x, y)
    names = ("Zref", "K", "Lgain", "x0", "xhat0", "model")
    for wx in (True, False):  # with or without xhat0_bar is two modes of Zref_bar; the subsets are taken inside each
        rest = tuple(n for n in names if n != "xhat0")
        fullv = _vjp(nlp, d, guarded, r["dcot"], rest + (("xhat0",) if wx else ()))
        for k in range(len(rest)):
            for sub in itertools.combinations(rest, k):
                got = _vjp(nlp, d, guarded, r["dcot"], sub + (("xhat0",) if wx else ()), innov="Lgain" in sub)
                for x, y, n in zip(got, fullv, names):
                    assert (x is None and n not in sub and not (n == "xhat0" and wx)) or torch.equal(x, y), (sub, n)


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("kw", [{}, {"z_stride": 20 * 5 + 3, "align": 7}])
def test_host_forms_equal_device_forms_and_padding_is_untouched(guarded, kw):
    import torch

    N, B, ny = 5, 67, 3
    batch, inp = ES.case(N, 1, 3, B, ny, guarded)
    nlp = TC.nlp(batch, TC.SECOND_MODEL, **kw)
    n, zs = nlp.n_nlp, nlp.z_stride
    d, h = _rollout(nlp, inp, guarded)
    dirs, cot = ES.directions(8, B, N, ny)
    pad = lambda a: np.concatenate([a, np.zeros((B, zs - n))], axis=1).reshape(-1)  # noqa: E731
    sentinel = torch.full((B * zs,), -7.25, dtype=torch.float64, device="cuda")
    dev = _jvp(nlp, d, guarded, EF.upload(nlp, dirs), out=sentinel)
    assert dev[0] is sentinel and bool((sentinel.view(B, zs)[:, n:] == -7.25).all())
    hd = dict(dirs, Zref_dot=pad(dirs["Zref_dot"]))
    host = nlp.tracking_rollout_estimated_jvp_host(pad(h["Zref"]), h["K"], h["Lgain"], h["H"], pad(h["Zout"]), h["Xhat"], h["innov"],
                                                   h["model"], guarded, h["events"], h["events_hat"], **hd)
    assert len(host) == len(dev) == (5 if guarded else 3)
    for name, x, y in zip(JVP_OUT, host, dev):
        if name == "Zout_dot":
            assert np.array_equal(x.reshape(B, zs)[:, :n], TC.rows(nlp, y)) and not x.reshape(B, zs)[:, n:].any()
        else:
            assert np.array_equal(x, y.cpu().numpy()), name
    for wx in (True, False):
        want = EF.want(h, wx)
        dev = _vjp(nlp, d, guarded, EF.upload(nlp, cot), want)
        host = nlp.tracking_rollout_estimated_vjp_host(pad(h["Zref"]), h["K"], h["Lgain"], h["H"], pad(h["Zout"]), h["Xhat"],
                                                       pad(cot["Zbar"]), h["innov"], h["model"], guarded, h["events"],
                                                       h["events_hat"], cot["Xhat_bar"], cot["innov_bar"], want)
        for name, x, y in zip(VJP_OUT, host, dev):
            if name == "Zref_bar":
                assert np.array_equal(x.reshape(B, zs)[:, :n], TC.rows(nlp, y)) and not x.reshape(B, zs)[:, n:].any()
            else:
                assert (x is None and y is None) or np.array_equal(x, y.cpu().numpy()), name


# ---- 4. the plant and the estimator land in different knots ----------------------------------------------------------------
def _split_case():
    """A guarded case whose estimate starts with its free foot 0.03 m higher than the plant's: one and a half knots of fall at
    v = -1 m/s and h = 0.02 s, so the estimator lands later than the plant."""
    N, im, B, ny = 5, 1, 32, 8
    batch, inp = ES.case(N, im, 2, B, ny, True)
    xhat0 = inp["x0"].copy()
    xhat0[:, 6] += 0.03
    return batch, dict(inp, xhat0=xhat0), N, B, ny


def test_a_case_where_plant_and_estimator_land_in_different_knots():
    """Held to the yardstick, and to a central difference of the GPU's own roll-out in an x0 direction on the problems whose two
    touchdown knots stay put, within ten times what the same quotient leaves in float64 numpy (FD_CPU_WORST)."""
    batch, inp, N, B, ny = _split_case()
    dirs, _ = ES.directions(9, B, N, ny)
    xd = dirs["x0_dot"]
    one = dict(x0_dot=xd, xhat0_dot=np.zeros((B, 15)))
    # the CPU yardstick alone: the knots differ, and what the quotient leaves there
    c = ES.rollout(batch, inp, True)
    differ = (c["events"][:, 0] != c["events_hat"][:, 0]) & (c["events"][:, 0] >= 0) & (c["events_hat"][:, 0] >= 0)
    assert differ.sum() >= B // 4, int(differ.sum())
    p, m = ES.rollout(batch, inp, True, x0=inp["x0"] + FD_EPS * xd), ES.rollout(batch, inp, True, x0=inp["x0"] - FD_EPS * xd)
    same = np.ones(B, dtype=bool)
    for rec in ("events", "events_hat"):
        same &= (p[rec][:, 0] == c[rec][:, 0]) & (m[rec][:, 0] == c[rec][:, 0])
    blk = ES.chain_blocks(N, np.asarray(batch.init_mode), None, c["Zout"], c["Xhat"], inp["model"], TC.SECOND, True, c["events"],
                          c["events_hat"])
    ref = ES.sweep_jvp(blk, inp["Zref"], inp["K"], inp["Lgain"], inp["H"], c["Zout"], c["Xhat"], c["innov"], **one)
    cpu = max(ES.worst(ref["Zout_dot"][same], ((p["Zout"] - m["Zout"]) / (2 * FD_EPS))[same]),
              ES.worst(ref["Xhat_dot"][same], ((p["Xhat"] - m["Xhat"]) / (2 * FD_EPS))[same]))
    print(f"float64 numpy quotient against the yardstick's sweep: {cpu:.2e} (FD_CPU_WORST {FD_CPU_WORST:.2e}); "
          f"{int((differ & same).sum())} problems with different knots kept")
    assert cpu <= 2 * FD_CPU_WORST and (differ & same).any()
    # the GPU
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    d, h = _rollout(nlp, inp, True)
    differ = (h["events"][:, 0] != h["events_hat"][:, 0]) & (h["events"][:, 0] >= 0) & (h["events_hat"][:, 0] >= 0)
    assert differ.sum() >= B // 4
    blk = ES.chain_blocks(N, np.asarray(batch.init_mode), None, h["Zout"], h["Xhat"], inp["model"], TC.SECOND, True, h["events"],
                          h["events_hat"])
    dirs = EF.present(inp, dirs)
    ref = ES.sweep_jvp(blk, inp["Zref"], inp["K"], inp["Lgain"], inp["H"], h["Zout"], h["Xhat"], h["innov"], events=h["events"],
                       events_hat=h["events_hat"], **dirs)
    got = EF.host(nlp, JVP_OUT, _jvp(nlp, d, True, EF.upload(nlp, dirs)))
    w = max(ES.worst(got[n], ref[n]) for n in got)
    got1 = EF.host(nlp, JVP_OUT, _jvp(nlp, d, True, EF.upload(nlp, one)))
    dp, hp = _rollout(nlp, dict(inp, x0=inp["x0"] + FD_EPS * xd), True)
    dm, hm = _rollout(nlp, dict(inp, x0=inp["x0"] - FD_EPS * xd), True)
    same = np.ones(B, dtype=bool)
    for rec in ("events", "events_hat"):
        same &= (hp[rec][:, 0] == h[rec][:, 0]) & (hm[rec][:, 0] == h[rec][:, 0])
    fd = max(ES.worst(got1["Zout_dot"][same], ((hp["Zout"] - hm["Zout"]) / (2 * FD_EPS))[same]),
             ES.worst(got1["Xhat_dot"][same], ((hp["Xhat"] - hm["Xhat"]) / (2 * FD_EPS))[same]))
    print(f"different knots: against the yardstick {w:.2e}; GPU quotient against the GPU's sweep {fd:.2e}; bar {FD_BAR:.2e}; "
          f"{int((~same).sum())} of {B} left out")
    assert w <= SWEEP_BAR and fd <= FD_BAR and (differ & same).any()


# ---- 5. torch autograd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,wx", [(False, True), (True, True), (True, False)])
def test_differentiable_estimated_rollout_backward_and_forward_ad_are_the_sweeps_bit_for_bit(guarded, wx):
    import torch
    import torch.autograd.forward_ad as fwAD

    r = _run(guarded, 5, 2, 2, 67, 8, (True, True, wx))
    nlp, d, dd, dc = r["nlp"], r["d"], r["ddirs"], r["dcot"]
    keys = ("Zref", "K", "Lgain", "x0", "xhat0", "model")
    leaves = {k: (None if d[k] is None else d[k].clone().requires_grad_(True)) for k in keys}
    call = lambda t: nlp.differentiable_estimated_rollout(t["Zref"], t["K"], t["Lgain"], d["H"], d["vnoise"], d["wnoise"], t["x0"],  # noqa: E731
                                                          t["xhat0"], t["model"], guarded=guarded)
    out = call(leaves)
    assert len(out) == (5 if guarded else 3)
    for o, k in zip(out, ("Zout", "Xhat", "innov", "events", "events_hat")):
        assert torch.equal(o, d[k])
    assert not any(o.requires_grad for o in out[3:])
    torch.autograd.backward(out[:3], [dc["Zbar"], dc["Xhat_bar"], dc["innov_bar"]])
    ref = _vjp(nlp, d, guarded, dc, EF.want(r["h"], wx))
    for k, g in zip(keys, ref):
        assert (leaves[k] is None and g is None) or torch.equal(leaves[k].grad.reshape(-1), g.reshape(-1)), k
    refj = _jvp(nlp, d, guarded, dd)
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
