"""qln_landing_filter_model*, qln_landing_filter_jvp* and qln_landing_filter_vjp* on the GPU: the filter at a model of each
record's own and the forward and reverse sweeps through it and through its score (include/qln_evaluator.h).  The yardstick is
tests/landing_filter_sweep_ref.py, held on the CPU by tests/test_landing_filter_sweep_host.py.  Besides it the kernels are held
without an oracle: by the adjoint identity between them, bit for bit by the estimate-feedback sweeps on a flight's record, by
eight sensor rows with zeros written out, by every subset of optional outputs, by NaN where nothing is read, by the host forms,
by central differences of the GPU's own filter, through torch autograd, and by the refusals through the device entries.  The
cases and their seeds are the yardstick module's."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import estimation_cases as EF
from tests import landing_filter_sweep_ref as FS
from tests import rollout_estimated_sweep_ref as ES
from tests import rollout_guarded_cases as GC
from tests import rollout_ref as RR
from tests import tracking_cases as TC

pytestmark = pytest.mark.gpu
_time_limit = EF.time_limit(300)

BAR = 1e-10         # the filter's bar (tests/test_gpu_landing_filter.py)
SWEEP_BAR = 1e-12   # the project's bar for a sweep against numpy, of max(1, |ref|) (tests/test_gpu_rollout_guarded_sweeps.py)
# N = 5 with k_trans over 1..N and both init_modes, B = 7 (a part-filled wave) and 67 (several blocks, a ragged tail), ny over
# 1, 3, 8; two full-length cases.  (guarded, N, init_mode, k_trans, B, ny); the guarded forms do not read k_trans.
SCHEDULED = [(False, 5, 1 + (kt + i) % 2, kt, (7, 67)[(kt + i) % 2], (1, 3, 8)[(kt + 2 * i) % 3]) for i in range(2)
             for kt in range(1, 6)]
GUARDED = [(True, 5, 1, 2, 7, 3), (True, 5, 2, 2, 67, 8), (True, 5, 1, 2, 67, 1), (True, 5, 2, 2, 7, 8)]
LONG = [(False, 61, 1, 21, 5, 8), (True, 61, 1, 21, 5, 3)]
CASES = SCHEDULED + GUARDED + LONG
JVP_OUT = ("Xhat", "innov", "nis", "loglik", "event_hat")
VJP_OUT = ("Y", "Zrec", "Lgain", "xhat0", "model")
# Test 9.  The same difference quotient in float64 numpy (landing_filter_ref.replay at model +- FD_EPS model_dot and
# Y +- FD_EPS Y_dot against the yardstick's sweep at the yardstick's own trajectory, the records of FD_CASES) leaves
# 8.53e-10 of max(1, |ref|) at 1e-4, its best step (1e-3: 8.1e-8, truncation; 1e-5: 5.0e-9, 1e-6: 4.1e-8, rounding; the worst is
# loglik's, a sum of N ny terms divided by V): the bar is ten times that.  The test forms the number again on every run and holds
# it to the constant within a factor of two, so that the constant cannot go stale.
FD_CASES = [(False, 5, 2, 3, 32, 8), (True, 5, 1, 2, 32, 8)]
FD_EPS = 1e-4
FD_CPU_WORST = 8.53e-10
FD_BAR = 10 * FD_CPU_WORST


def _np(t):
    return None if t is None else t.cpu().numpy()


def _upload(nlp, d):
    return {k: (nlp.upload_Z(v) if k in ("Zrec_dot", "Zref", "Zrec") else EF.dev(v)) for k, v in d.items()}


def _filter(nlp, d, guarded, model="own", score=True, **replace):
    """The GPU's filter of a device record: (Xhat, innov, score, loglik, events_hat or None)"""
    a = dict(d, **replace)
    f = nlp.landing_filter_guarded if guarded else nlp.landing_filter
    out = f(a["Zref"], a["Zrec"], a["Lgain"], a["H"], a["Y"], a["V"] if score else None, a["xhat0"],
            model=a["model"] if isinstance(model, str) else model)
    return out if guarded else out + (None,)


def _point(d, got):
    return dict(d, Xhat=got[0], innov=got[1], events_hat=got[4])


def _jvp(nlp, p, guarded, dirs, want=None, score=True, **kw):
    given = {k: dirs.get(k) for k in FS.TANGENTS}
    return nlp.landing_filter_jvp(p["Zref"], p["Zrec"], p["Lgain"], p["H"], p["Xhat"], p["innov"], p["V"] if score else None,
                                  p["model"], p["events_hat"], guarded, want=want, **given, **kw)


def _vjp(nlp, p, guarded, cot, want=None, score=True, innov=True):
    given = {k: cot.get(k) for k in FS.COTANGENTS}
    return nlp.landing_filter_vjp(p["Zref"], p["Zrec"], p["Lgain"], p["H"], p["Xhat"], p["innov"] if innov else None,
                                  p["V"] if score else None, p["model"], p["events_hat"], guarded, want=want, **given)


def _host(nlp, out):
    return {k + ("_dot" if k in JVP_OUT else "_bar"): (TC.rows(nlp, v) if k == "Zrec" else _np(v)) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _run(guarded, N, im, kt, B, ny):
    """One case: the record, the GPU's filter at the records' own models, the yardstick's blocks at the GPU's own trajectory and
    record, one direction and one cotangent, and the yardstick's own float64-to-longdouble distance.  Shared by the tests of the
    case; nothing here is changed afterwards."""
    batch, rec = FS.record(N, im, kt, B, ny, guarded)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    d = _upload(nlp, {k: rec[k] for k in ("Zref", "Zrec", "Lgain", "Y", "xhat0", "model")})
    d["H"], d["V"] = rec["H"], rec["V"]
    got = _filter(nlp, d, guarded)
    p = _point(d, got)
    h = dict(rec, Xhat=_np(got[0]), innov=_np(got[1]), score=_np(got[2]), loglik=_np(got[3]), events_hat=_np(got[4]))
    mk = lambda ct: FS.blocks(N, np.asarray(batch.init_mode), np.asarray(batch.k_trans), rec["Zrec"], h["Xhat"], rec["model"],  # noqa: E731
                              guarded, h["events_hat"], ctype=ct)
    (F, T), (Fl, Tl) = mk(np.complex128), mk(np.clongdouble)
    dirs, cot = FS.directions(1000 * N + 10 * kt + ny, B, N, ny)
    fixed = {k: v for k, v in dirs.items() if k != "Lgain_dot"}
    j = lambda F_, T_: FS.sweep_jvp(F_, T_, rec["Lgain"], rec["H"], h["innov"], rec["V"], h["events_hat"], **fixed)  # noqa: E731
    v = lambda F_: FS.sweep_vjp(F_, rec["Lgain"], rec["H"], h["innov"], rec["V"], **cot)  # noqa: E731
    a, al, r, rl = j(F, T), j(Fl, Tl), v(F), v(Fl)
    dist = max([FS.worst(a[k], al[k]) for k in a] + [FS.worst(r[k], rl[k]) for k in r if r[k] is not None])
    bar = max(SWEEP_BAR, 100 * dist)
    if bar > SWEEP_BAR:
        print(f"guarded={guarded} N={N} B={B} ny={ny}: the yardstick is {dist:.2e} from its longdouble restatement: bar {bar:.2e}")
    return dict(nlp=nlp, batch=batch, rec=rec, d=d, p=p, h=h, F=F, T=T, dirs=dirs, cot=cot, ddirs=_upload(nlp, dirs),
                dcot=_upload(nlp, cot), bar=bar, got=got)


def _subsets(names):
    return [c for k in range(1, len(names) + 1) for c in itertools.combinations(names, k)]


# ---- 1. the filter at a model of the record's own --------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", CASES)
def test_the_filter_at_the_records_own_models_matches_the_yardstick(guarded, N, im, kt, B, ny):
    """landing_filter*(model=...) against landing_filter_ref.replay with that th_hat, in rollout_ref.rel within 1e-10; guarded, a
    problem whose estimator is closer than MARGIN to a boundary of its guard is left out, at most LEFT_OUT of a case."""
    r = _run(guarded, N, im, kt, B, ny)
    h, rec = r["h"], r["rec"]
    ref = FS.replay(r["batch"], rec, guarded)
    keep = ref["margin_hat"] >= GC.MARGIN if guarded else np.ones(B, dtype=bool)
    assert keep.mean() >= 1 - GC.LEFT_OUT, int((~keep).sum())
    err = {"Xhat": RR.rel(h["Xhat"][keep], ref["Xhat"][keep]), "innov": RR.rel(h["innov"][keep], ref["innov"][keep]),
           "nis": RR.rel(h["score"][keep][..., 0], ref["score"][keep][..., 0])}
    if guarded:
        err["event_hat"] = RR.rel(h["events_hat"][keep], ref["events_hat"][keep])
        assert (h["events_hat"][:, 0] >= 0).any()
    print(f"guarded={guarded} N={N} mode={im} k_trans={kt} B={B} ny={ny}: " + ", ".join(f"{n} {e:.2e}" for n, e in err.items()) +
          f"; {int((~keep).sum())} problems left out")
    assert all(e <= BAR for e in err.values()), err
    other = _filter(r["nlp"], r["d"], guarded, model=None)
    assert not np.array_equal(_np(other[0]), h["Xhat"])  # the records' models are not the handle's


@pytest.mark.parametrize("guarded,N,im,kt,B,ny", [SCHEDULED[1], SCHEDULED[7], GUARDED[1], LONG[0], LONG[1]])
def test_without_a_model_and_with_the_handles_values_written_out_the_filter_has_the_existing_calls_bits(guarded, N, im, kt, B, ny):
    import torch

    from quadruped_landing_amd import _lib

    r = _run(guarded, N, im, kt, B, ny)
    nlp, d = r["nlp"], r["d"]
    old = _filter(nlp, d, guarded, model=None)
    written = _filter(nlp, d, guarded, model=EF.dev(np.tile(TC.SECOND, (B, 1))))
    for a, b in zip(old, written):
        assert (a is None and b is None) or torch.equal(a, b)
    # the _model entry with model == NULL, which the Python layer never calls
    Hd, Vh = EF.dev(d["H"]), np.ascontiguousarray(d["V"])
    outs = [torch.zeros_like(t) for t in old if t is not None]
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    fn = getattr(_lib.lib(), "qln_landing_filter_guarded_model" if guarded else "qln_landing_filter_model")
    _lib.check(fn(nlp._h, ptr(d["Zref"]), ptr(d["Zrec"]), ptr(d["Lgain"]), ptr(Hd), ny, None, Vh.ctypes.data, ptr(d["Y"]),
                  ptr(d["xhat0"]), *(ptr(t) for t in outs)))
    for a, b in zip([t for t in old if t is not None], outs):
        assert torch.equal(a, b)


# ---- 2. both sweeps against the yardstick ------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", CASES)
def test_sweeps_match_the_yardstick_in_every_combination_of_tangents_and_cotangents(guarded, N, im, kt, B, ny):
    """Device JVP and VJP at the GPU's own trajectory against the numpy sweeps on complex-step blocks, within 1e-12 of
    max(1, |ref|) (or 100 times the yardstick's own float64-to-longdouble distance where that is more, printed when it is): all
    31 subsets of the five tangents (the score's tangents wherever Lgain_dot is absent) and all 15 subsets of the four
    cotangents (Lgain_bar wherever no score cotangent is present).  No problem is left out."""
    r = _run(guarded, N, im, kt, B, ny)
    nlp, p, h, rec = r["nlp"], r["p"], r["h"], r["rec"]
    worst = 0.0
    for sub in _subsets(FS.TANGENTS):
        score = "Lgain_dot" not in sub
        ref = FS.sweep_jvp(r["F"], r["T"], rec["Lgain"], rec["H"], h["innov"], rec["V"] if score else None, h["events_hat"],
                           **{k: r["dirs"][k] for k in sub})
        got = _host(nlp, _jvp(nlp, p, guarded, {k: r["ddirs"][k] for k in sub}, score=score))
        assert set(got) == set(ref) - (set() if guarded else {"event_hat_dot"}), (sub, sorted(got))
        w = {n: FS.worst(got[n], ref[n]) for n in got}
        worst = max(worst, *w.values())
        assert max(w.values()) <= r["bar"], (sub, w, r["bar"])
    for sub in _subsets(FS.COTANGENTS):
        score = "nis_bar" in sub or "loglik_bar" in sub
        ref = FS.sweep_vjp(r["F"], rec["Lgain"], rec["H"], h["innov"], rec["V"] if score else None, **{k: r["cot"][k] for k in sub})
        got = _host(nlp, _vjp(nlp, p, guarded, {k: r["dcot"][k] for k in sub}, score=score))
        assert ("Lgain_bar" in got) == (not score) and len(got) == (4 if score else 5)
        w = {n: FS.worst(got[n], ref[n]) for n in got}
        worst = max(worst, *w.values())
        assert max(w.values()) <= r["bar"], (sub, w, r["bar"])
    print(f"guarded={guarded} N={N} mode={im} k_trans={kt} B={B} ny={ny}: worst of both sweeps over the 31 + 15 combinations "
          f"{worst:.2e}; bar {r['bar']:.2e}")


# ---- 3. the adjoint identity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score", [True, False])
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", CASES)
def test_adjoint_identity_between_the_two_kernels(guarded, N, im, kt, B, ny, score):
    """<Xhat_bar, Xhat_dot> + <innov_bar, innov_dot> + <nis_bar, nis_dot> + <loglik_bar, loglik_dot> = the five products on the
    other side, with the score's terms (then without Lgain's) and without them (then with Lgain's): no oracle involved."""
    import torch

    r = _run(guarded, N, im, kt, B, ny)
    nlp, p = r["nlp"], r["p"]
    dirs = {k: v for k, v in r["ddirs"].items() if not (score and k == "Lgain_dot")}
    cot = {k: v for k, v in r["dcot"].items() if score or k in ("Xhat_bar", "innov_bar")}
    fwd = _jvp(nlp, p, guarded, dirs, score=score)
    rev = _vjp(nlp, p, guarded, cot, score=score)
    assert ("Lgain" in rev) == (not score) and ("nis" in fwd) == score
    dot = lambda a, b_: float(torch.dot(a.reshape(-1), b_.reshape(-1)))  # noqa: E731
    lhs = sum(dot(v, fwd[k[:-4]]) for k, v in cot.items())
    rhs = sum(dot(rev[k[:-4]], v) for k, v in dirs.items())
    print(f"guarded={guarded} N={N} B={B} ny={ny} score={score}: lhs {lhs:.15e}, rhs {rhs:.15e}, difference "
          f"{abs(lhs - rhs) / (abs(lhs) + abs(rhs)):.2e}")
    assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs)), (lhs, rhs)


# ---- 4. the replay against the estimate-feedback sweeps ----------------------------------------------------------------------
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", [SCHEDULED[1], SCHEDULED[7], GUARDED[1], GUARDED[3], LONG[0], LONG[1]])
def test_on_a_flights_record_the_sweeps_are_bitwise_the_estimators_chain_of_the_estimate_feedback_sweeps(guarded, N, im, kt, B, ny):
    """A closed-loop flight's record at the handle's model: with only xhat0_dot and Lgain_dot, Xhat_dot, innov_dot and
    event_hat_dot are those of tracking_rollout_estimated_jvp called with K = None (whose plant chain then stays zero), and
    xhat0_bar and Lgain_bar of the reverse sweep are that call's sibling's."""
    import torch

    batch, inp = ES.case(N, im, kt, B, ny, guarded)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Zref = nlp.upload_Z(inp["Zref"])
    dv = {k: EF.dev(inp[k]) for k in ("K", "Lgain", "vnoise", "wnoise", "x0", "xhat0", "model")}
    flown = nlp.tracking_rollout_estimated(Zref, dv["K"], dv["Lgain"], inp["H"], dv["vnoise"], dv["wnoise"], dv["x0"], dv["xhat0"],
                                           dv["model"], guarded=guarded, with_innovations=True)
    Zout, Xhat, innov = flown[:3]
    ev, eh = (flown[3], flown[4]) if guarded else (None, None)
    dirs, cot = FS.directions(5, B, N, ny)
    xd, ld = EF.dev(dirs["xhat0_dot"]), EF.dev(dirs["Lgain_dot"])
    Xb, Ib = EF.dev(cot["Xhat_bar"]), EF.dev(cot["innov_bar"])
    p = dict(Zref=Zref, Zrec=Zout, Lgain=dv["Lgain"], H=inp["H"], V=None, Xhat=Xhat, innov=innov, model=None, events_hat=eh)
    for with_l in (True, False):
        mine = _jvp(nlp, p, guarded, dict(xhat0_dot=xd, **({"Lgain_dot": ld} if with_l else {})), score=False)
        sib = nlp.tracking_rollout_estimated_jvp(Zref, None, dv["Lgain"], inp["H"], Zout, Xhat, innov, None, guarded, ev, eh,
                                                 Lgain_dot=ld if with_l else None, xhat0_dot=xd)
        assert not bool(sib[0].any())  # the plant's chain is zero
        assert torch.equal(mine["Xhat"], sib[1]) and torch.equal(mine["innov"], sib[2]) and bool(sib[1].any())
        if guarded:
            assert torch.equal(mine["event_hat"], sib[4]) and bool(sib[4].any())
        want = ("xhat0",) + (("Lgain",) if with_l else ())
        rev = _vjp(nlp, p, guarded, dict(Xhat_bar=Xb, innov_bar=Ib), want=want, score=False, innov=with_l)
        sibv = nlp.tracking_rollout_estimated_vjp(Zref, None, dv["Lgain"], inp["H"], Zout, Xhat, torch.zeros_like(Zout),
                                                  innov if with_l else None, None, guarded, ev, eh, Xb, Ib, want)
        assert torch.equal(rev["xhat0"], sibv[4]) and bool(sibv[4].any())
        if with_l:
            assert torch.equal(rev["Lgain"], sibv[2]) and bool(sibv[2].any())


# ---- 5. sensor rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,N,im,kt,B", [(False, 5, 1, 3, 67), (True, 5, 2, 2, 67), (False, 61, 1, 21, 5)])
def test_three_sensor_rows_are_bitwise_eight_rows_with_zeros(guarded, N, im, kt, B):
    import torch

    batch, rec = FS.record(N, im, kt, B, 3, guarded)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    d = _upload(nlp, {k: rec[k] for k in ("Zref", "Zrec", "Lgain", "Y", "xhat0", "model")})
    d["H"], d["V"] = rec["H"], rec["V"]
    p = _point(d, _filter(nlp, d, guarded))
    pad = lambda a, axis: np.concatenate([a, np.zeros(a.shape[:axis] + (5,) + a.shape[axis + 1:])], axis=axis)  # noqa: E731
    p8 = dict(p, Lgain=EF.dev(pad(rec["Lgain"], 3)), H=pad(rec["H"], 0), V=np.concatenate([rec["V"], np.ones(5)]),
              innov=EF.dev(pad(_np(p["innov"]), 2)))
    dirs, cot = FS.directions(6, B, N, 3)
    dirs8 = dict(dirs, Lgain_dot=pad(dirs["Lgain_dot"], 3), Y_dot=pad(dirs["Y_dot"], 2))
    cot8 = dict(cot, innov_bar=pad(cot["innov_bar"], 2))
    for score in (True, False):
        drop = "Lgain_dot" if score else None
        a = _jvp(nlp, p, guarded, {k: v for k, v in _upload(nlp, dirs).items() if k != drop}, score=score)
        b = _jvp(nlp, p8, guarded, {k: v for k, v in _upload(nlp, dirs8).items() if k != drop}, score=score)
        assert set(a) == set(b) and ("loglik" in a) == score
        for name in a:
            assert torch.equal(a[name], b[name][..., :3] if name == "innov" else b[name]), (score, name)
        assert not score or bool(a["nis"].any())
        c3 = {k: v for k, v in _upload(nlp, cot).items() if score or k in ("Xhat_bar", "innov_bar")}
        c8 = {k: v for k, v in _upload(nlp, cot8).items() if score or k in ("Xhat_bar", "innov_bar")}
        a, b = _vjp(nlp, p, guarded, c3, score=score), _vjp(nlp, p8, guarded, c8, score=score)
        assert set(a) == set(b) and ("Lgain" in a) == (not score)
        for name in a:
            assert torch.equal(a[name], b[name][..., :3] if name in ("Lgain", "Y") else b[name]), (score, name)
        assert not bool(b["Y"][..., 3:].any())
        if not score:
            assert not bool(b["Lgain"][..., 3:].any())


# ---- 6. optional outputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", [SCHEDULED[3], GUARDED[1]])
def test_every_subset_of_optional_outputs_leaves_the_others_bits(guarded, N, im, kt, B, ny):
    import torch

    r = _run(guarded, N, im, kt, B, ny)
    nlp, p = r["nlp"], r["p"]
    fixed = {k: v for k, v in r["ddirs"].items() if k != "Lgain_dot"}
    outs = JVP_OUT if guarded else JVP_OUT[:4]
    full = _jvp(nlp, p, guarded, fixed, want=outs)
    for sub in _subsets(outs):
        got = _jvp(nlp, p, guarded, fixed, want=sub, score=("nis" in sub or "loglik" in sub))
        assert set(got) == set(sub) and all(torch.equal(got[k], full[k]) for k in sub), sub
    gains = _jvp(nlp, p, guarded, r["ddirs"], want=("Xhat", "innov"), score=False)
    for sub in _subsets(("Xhat", "innov")):
        got = _jvp(nlp, p, guarded, r["ddirs"], want=sub, score=False)
        assert all(torch.equal(got[k], gains[k]) for k in sub), sub
    for score in (True, False):
        cot = {k: v for k, v in r["dcot"].items() if score or k in ("Xhat_bar", "innov_bar")}
        outs = tuple(o for o in VJP_OUT if not (score and o == "Lgain"))
        full = _vjp(nlp, p, guarded, cot, want=outs, score=score)
        for sub in _subsets(outs):
            got = _vjp(nlp, p, guarded, cot, want=sub, score=score, innov=score or "Lgain" in sub)
            assert set(got) == set(sub) and all(torch.equal(got[k], full[k]) for k in sub), (score, sub)


# ---- 7. what is not read, and exact zeros -------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", [SCHEDULED[3], GUARDED[1], LONG[1]])
def test_nan_where_nothing_is_read_changes_no_bit_and_the_stated_zeros_are_exact(guarded, N, im, kt, B, ny):
    """Not read: Zref altogether, the state slots of Zrec and of Zrec_dot, the last knot of both, entries 2.. of event_hat, and
    innov without Lgain's tangent and the score.  Exact zeros: Zrec_bar's state slots, event_hat_dot outside entries 1 and 2
    and for a problem that never lands."""
    import torch

    r = _run(guarded, N, im, kt, B, ny)
    nlp, p = r["nlp"], r["p"]
    nan = float("nan")
    states = (20 * torch.arange(N, device="cuda")[:, None] + torch.arange(15, device="cuda")[None, :]).reshape(-1)
    Zrec, Zd = p["Zrec"].clone(), r["ddirs"]["Zrec_dot"].clone()
    Zrec.view(B, -1)[:, states] = nan
    Zd.view(B, -1)[:, states] = nan
    q = dict(p, Zref=torch.full_like(p["Zref"], nan), Zrec=Zrec)
    if guarded:
        q["events_hat"] = p["events_hat"].clone()
        q["events_hat"][:, 2:] = nan
    fixed = {k: v for k, v in r["ddirs"].items() if k != "Lgain_dot"}
    a, b = _jvp(nlp, p, guarded, fixed), _jvp(nlp, q, guarded, dict(fixed, Zrec_dot=Zd))
    assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)
    qi = dict(q, innov=torch.full_like(p["innov"], nan))
    plain = {k: v for k, v in fixed.items()}
    a, b = _jvp(nlp, p, guarded, plain, score=False), _jvp(nlp, qi, guarded, dict(plain, Zrec_dot=Zd), score=False)
    assert all(torch.equal(a[k], b[k]) for k in a)
    if guarded:
        ed, ev = a["event_hat"], p["events_hat"]
        assert not bool(ed[:, 0].any()) and not bool(ed[:, 3:].any()) and bool(ed[:, 1:3].any())
        never = ev[:, 0] < 0
        assert not bool(ed[never].any())
    for score in (True, False):
        cot = {k: v for k, v in r["dcot"].items() if score or k in ("Xhat_bar", "innov_bar")}
        a = _vjp(nlp, p, guarded, cot, score=score)
        b = _vjp(nlp, q, guarded, cot, score=score, innov=score, want=tuple(k for k in a if k != "Lgain"))
        assert all(torch.equal(a[k], b[k]) for k in b), score
        zb = a["Zrec"].view(B, -1)
        assert not bool(zb[:, states].any()) and bool(zb[:, : nlp.n_nlp].any())


# ---- 8. host forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("kw", [{}, {"z_stride": 20 * 5 + 3, "align": 7}])
def test_host_forms_equal_device_forms_and_padding_is_untouched(guarded, kw):
    N, B, ny = 5, 67, 3
    batch, rec = FS.record(N, 1, 3, B, ny, guarded)
    nlp = TC.nlp(batch, TC.SECOND_MODEL, **kw)
    n, zs = nlp.n_nlp, nlp.z_stride
    d = _upload(nlp, {k: rec[k] for k in ("Zref", "Zrec", "Lgain", "Y", "xhat0", "model")})
    d["H"], d["V"] = rec["H"], rec["V"]
    got = _filter(nlp, d, guarded)
    p = _point(d, got)
    pad = lambda a: np.concatenate([a, np.full((B, zs - n), -7.25)], axis=1).reshape(-1)  # noqa: E731
    fh = nlp.landing_filter_guarded_host if guarded else nlp.landing_filter_host
    hostf = fh(pad(rec["Zref"]), pad(rec["Zrec"]), rec["Lgain"], rec["H"], rec["Y"], rec["V"], rec["xhat0"], model=rec["model"])
    for x, y in zip(hostf, got):
        assert np.array_equal(x, _np(y))
    hp = dict(Zref=pad(rec["Zref"]), Zrec=pad(rec["Zrec"]), Lgain=rec["Lgain"], H=rec["H"], V=rec["V"], Xhat=hostf[0], innov=hostf[1],
              model=rec["model"], events_hat=hostf[4] if guarded else None)
    dirs, cot = FS.directions(8, B, N, ny)
    for score in (True, False):
        dd = {k: v for k, v in dirs.items() if not (score and k == "Lgain_dot")}
        dev = _jvp(nlp, p, guarded, _upload(nlp, dd), score=score)
        given = {k: (pad(v) if k == "Zrec_dot" else v) for k, v in dd.items()}
        host = nlp.landing_filter_jvp_host(hp["Zref"], hp["Zrec"], hp["Lgain"], hp["H"], hp["Xhat"], hp["innov"],
                                           hp["V"] if score else None, hp["model"], hp["events_hat"], guarded, **given)
        assert set(host) == set(dev) and all(np.array_equal(host[k], _np(dev[k])) for k in dev), score
        cc = {k: v for k, v in cot.items() if score or k in ("Xhat_bar", "innov_bar")}
        dev = _vjp(nlp, p, guarded, _upload(nlp, cc), score=score)
        host = nlp.landing_filter_vjp_host(hp["Zref"], hp["Zrec"], hp["Lgain"], hp["H"], hp["Xhat"], hp["innov"],
                                           hp["V"] if score else None, hp["model"], hp["events_hat"], guarded, **cc)
        assert set(host) == set(dev)
        for k in dev:
            if k == "Zrec":
                assert np.array_equal(host[k].reshape(B, zs)[:, :n], TC.rows(nlp, dev[k])) and not host[k].reshape(B, zs)[:, n:].any()
                assert not bool(dev[k].view(B, zs)[:, n:].any())
            else:
                assert np.array_equal(host[k], _np(dev[k])), (score, k)


# ---- 9. central differences of the GPU's own filter ---------------------------------------------------------------------------
def _quotients(minus, plus, eps):
    return {k: (plus[k] - minus[k]) / (2 * eps) for k in ("Xhat", "innov", "loglik")}


def test_central_differences_of_the_gpus_own_filter_in_the_model_and_the_measurements():
    """landing_filter(model=...) at model +- FD_EPS model_dot and Y +- FD_EPS Y_dot against the forward sweep's Xhat_dot, innov_dot
    and loglik_dot, within ten times what the same quotient leaves in float64 numpy (FD_CPU_WORST, formed again here); a
    scheduled and a guarded case, no estimator's touchdown knot moving."""
    cpu_worst, gpu_worst = 0.0, 0.0
    for guarded, N, im, kt, B, ny in FD_CASES:
        batch, rec = FS.record(N, im, kt, B, ny, guarded)
        dirs, _ = FS.directions(9, B, N, ny)
        md, yd = dirs["model_dot"], dirs["Y_dot"]
        at = lambda s: dict(model=rec["model"] + s * md, Y=rec["Y"] + s * yd)  # noqa: E731
        # the CPU yardstick alone
        c, pl, mi = (FS.replay(batch, rec, guarded, **at(s)) for s in (0.0, FD_EPS, -FD_EPS))
        if guarded:
            assert (pl["events_hat"][:, 0] == c["events_hat"][:, 0]).all() and (mi["events_hat"][:, 0] == c["events_hat"][:, 0]).all()
        F, T = FS.blocks(N, np.asarray(batch.init_mode), np.asarray(batch.k_trans), rec["Zrec"], c["Xhat"], rec["model"], guarded,
                         c.get("events_hat"))
        ref = FS.sweep_jvp(F, T, rec["Lgain"], rec["H"], c["innov"], rec["V"], c.get("events_hat"), Y_dot=yd, model_dot=md)
        q = _quotients(mi, pl, FD_EPS)
        cpu_worst = max([cpu_worst] + [FS.worst(q[k], ref[k + "_dot"]) for k in q])
        # the GPU
        nlp = TC.nlp(batch, TC.SECOND_MODEL)
        d = _upload(nlp, {k: rec[k] for k in ("Zref", "Zrec", "Lgain", "Y", "xhat0", "model")})
        d["H"], d["V"] = rec["H"], rec["V"]
        run = lambda s: _filter(nlp, d, guarded, model=EF.dev(at(s)["model"]), Y=EF.dev(at(s)["Y"]))  # noqa: E731
        g0, gp, gm = run(0.0), run(FD_EPS), run(-FD_EPS)
        if guarded:
            assert bool((gp[4][:, 0] == g0[4][:, 0]).all()) and bool((gm[4][:, 0] == g0[4][:, 0]).all()) and bool((g0[4][:, 0] >= 0).any())
        names = dict(Xhat=0, innov=1, loglik=3)
        qg = _quotients({k: _np(gm[i]) for k, i in names.items()}, {k: _np(gp[i]) for k, i in names.items()}, FD_EPS)
        got = _jvp(nlp, _point(d, g0), guarded, dict(Y_dot=EF.dev(yd), model_dot=EF.dev(md)))
        w = {k: FS.worst(qg[k], _np(got[k])) for k in qg}
        gpu_worst = max(gpu_worst, *w.values())
        print(f"guarded={guarded}: the GPU's quotient against its forward sweep {w}")
    print(f"the float64 numpy quotient leaves {cpu_worst:.2e} (FD_CPU_WORST {FD_CPU_WORST:.2e}); the GPU's {gpu_worst:.2e}; bar {FD_BAR:.2e}")
    assert FD_CPU_WORST / 2 <= cpu_worst <= 2 * FD_CPU_WORST, cpu_worst
    assert gpu_worst <= FD_BAR, gpu_worst


# ---- 10. autograd -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded,N,im,kt,B,ny", [SCHEDULED[3], GUARDED[1]])
def test_autograd_backward_and_forward_mode_are_the_two_sweeps_bit_for_bit(guarded, N, im, kt, B, ny):
    import torch
    import torch.autograd.forward_ad as fwAD

    r = _run(guarded, N, im, kt, B, ny)
    nlp, d, p = r["nlp"], r["d"], r["p"]
    for score in (True, False):
        gains = d["Lgain"] if score else d["Lgain"].clone().requires_grad_()
        f = nlp.differentiable_landing_filter(d["Zref"], gains, d["H"], d["V"] if score else None, guarded)
        ins = [d[k].clone().requires_grad_() for k in ("Y", "Zrec", "xhat0", "model")]
        out = f(*ins)
        assert torch.equal(out[0], p["Xhat"]) and torch.equal(out[1], p["innov"]) and len(out) == 2 + score + guarded
        cot = {k: v for k, v in r["dcot"].items() if k != "nis_bar" and (score or k != "loglik_bar")}
        loss = (out[0] * cot["Xhat_bar"]).sum() + (out[1] * cot["innov_bar"]).sum()
        if score:
            assert torch.equal(out[2], r["got"][3])
            loss = loss + (out[2] * cot["loglik_bar"]).sum()
        loss.backward()
        want = ("Y", "Zrec", "xhat0", "model") + (() if score else ("Lgain",))
        ref = _vjp(nlp, p, guarded, cot, want=want, score=score)
        for t, k in zip(ins, want):
            assert torch.equal(t.grad.reshape(-1), ref[k].reshape(-1)), (score, k)
        if not score:  # the gains' gradient sits on the tensor the op was built with
            assert torch.equal(gains.grad.reshape(-1), ref["Lgain"].reshape(-1)) and bool(gains.grad.any())
        dirs = {k: v for k, v in r["ddirs"].items() if k != "Lgain_dot"}
        with fwAD.dual_level():
            duals = [fwAD.make_dual(d[k], dirs[k + "_dot"]) for k in ("Y", "Zrec", "xhat0", "model")]
            tang = [fwAD.unpack_dual(o).tangent for o in f(*duals)]
        refj = _jvp(nlp, p, guarded, dirs, want=("Xhat", "innov") + (("loglik",) if score else ()), score=score)
        assert torch.equal(tang[0], refj["Xhat"]) and torch.equal(tang[1], refj["innov"])
        if score:
            assert torch.equal(tang[2], refj["loglik"])
    with pytest.raises(RuntimeError, match="only without V"):
        lg = d["Lgain"].clone().requires_grad_()
        out = nlp.differentiable_landing_filter(d["Zref"], lg, d["H"], d["V"], guarded)(d["Y"], d["Zrec"], d["xhat0"], d["model"])
        out[2].sum().backward()


# ---- 11. refusals through the device entries ----------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded", [False, True])
def test_refusals_through_the_device_entries(guarded):
    from quadruped_landing_amd import _lib

    N, B, ny = 5, 7, 3
    r = _run(guarded, N, 1, 2, B, ny) if guarded else _run(False, N, 1, 4, 7, 3)
    nlp, p = r["nlp"], r["p"]
    fixed = {k: v for k, v in r["ddirs"].items() if k != "Lgain_dot"}
    inv = _lib.QLN_ERR_INVALID_ARGUMENT

    def refused(call, text):
        with pytest.raises(_lib.QlnError) as e:
            call()
        assert e.value.code == inv and text in str(e.value), str(e.value)

    refused(lambda: _jvp(nlp, p, guarded, {}), "every tangent is NULL")
    refused(lambda: _jvp(nlp, p, guarded, fixed, want=()), "every output is NULL")
    refused(lambda: _jvp(nlp, p, guarded, r["ddirs"], want=("Xhat", "nis")), "at fixed gains")
    refused(lambda: _jvp(nlp, p, guarded, r["ddirs"], want=("loglik",)), "at fixed gains")
    refused(lambda: _jvp(nlp, p, guarded, fixed, want=("nis",), score=False), "null Vdiag")
    refused(lambda: _jvp(nlp, dict(p, innov=None), guarded, fixed, want=("nis",)), "null innov")
    refused(lambda: _jvp(nlp, dict(p, innov=None), guarded, r["ddirs"], want=("Xhat",), score=False), "null innov")
    refused(lambda: _vjp(nlp, p, guarded, {}), "every cotangent is NULL")
    refused(lambda: _vjp(nlp, p, guarded, r["dcot"], want=()), "every output is NULL")
    refused(lambda: _vjp(nlp, p, guarded, r["dcot"], want=("Lgain", "Y")), "at fixed gains")
    refused(lambda: _vjp(nlp, p, guarded, r["dcot"], want=("Y",), score=False), "null Vdiag")
    refused(lambda: _vjp(nlp, p, guarded, r["dcot"], want=("Y",), innov=False), "null innov")
    # overlaps: an output on an input, and two outputs on each other
    refused(lambda: _overlap_jvp(nlp, p, guarded, fixed), "overlaps an input")
    refused(lambda: _overlap_vjp(nlp, p, guarded, r["dcot"]), "two outputs overlap")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _overlap_jvp(nlp, p, guarded, dirs):
    """Xhat_dot on top of Xhat, through the C entry"""
    from quadruped_landing_amd import _lib

    Hd = EF.dev(p["H"])
    ev = (_ptr(p["events_hat"]),) if guarded else ()
    fn = getattr(_lib.lib(), "qln_landing_filter_guarded_jvp" if guarded else "qln_landing_filter_jvp")
    _lib.check(fn(nlp._h, _ptr(p["Zref"]), _ptr(p["Zrec"]), _ptr(p["Lgain"]), _ptr(Hd), Hd.shape[0], _ptr(p["model"]), None,
                  _ptr(p["Xhat"]), None, *ev, _ptr(dirs["Y_dot"]), None, None, None, None, _ptr(p["Xhat"]), None, None, None,
                  *((None,) if guarded else ())))


def _overlap_vjp(nlp, p, guarded, cot):
    """xhat0_bar inside Y_bar, through the C entry"""
    import torch

    from quadruped_landing_amd import _lib

    Hd = EF.dev(p["H"])
    ev = (_ptr(p["events_hat"]),) if guarded else ()
    yb = torch.zeros(p["innov"].numel() + 15 * nlp.B, dtype=torch.float64, device="cuda")
    fn = getattr(_lib.lib(), "qln_landing_filter_guarded_vjp" if guarded else "qln_landing_filter_vjp")
    _lib.check(fn(nlp._h, _ptr(p["Zref"]), _ptr(p["Zrec"]), _ptr(p["Lgain"]), _ptr(Hd), Hd.shape[0], _ptr(p["model"]), None,
                  _ptr(p["Xhat"]), None, *ev, _ptr(cot["Xhat_bar"]), None, None, None, _ptr(yb), None, None, _ptr(yb), None))
