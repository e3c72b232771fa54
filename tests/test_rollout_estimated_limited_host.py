"""The yardstick of the estimate-feedback roll-out within force limits (tests/rollout_estimated_limited_ref.py), held on the CPU
independently of the kernels: in float64 against longdouble, against the unlimited yardstick with infinite limits, against
rollout_limited_ref where the estimate does not reach the plant, its forward sweep against longdouble central differences of
its own roll-out, its reverse sweep as the adjoint of the forward one -- and, of the six entry points, what needs no device: the
ctypes table and the argument checks.  It also runs every case of tests/test_gpu_tracking_estimated_limited.py on the yardstick
alone, so that what the GPU assertions rely on (nothing left out, a bounded loop, clamps active) is established here first."""
import ctypes as C

import numpy as np
import pytest

from tests import rollout_estimated_limited_ref as XR
from tests import rollout_estimated_ref as ER
from tests import rollout_estimated_sweep_ref as ES
from tests import rollout_limited_ref as LR
from tests import rollout_ref as RR
from tests import tracking_cases as TC

LIM = XR.TEST_LIMITS
# (N, init_mode, k_trans, B, ny): tests/test_rollout_estimated_sweep_host.py's family
CASES = [(5, 1, 2, 16, 3), (5, 2, 4, 16, 8), (5, 1, 5, 16, 1), (40, 2, 14, 9, 8)]
LEFT_OUT = 0.10   # the share of a case's problems that change a touchdown knot or a saturation code over the difference's step
FD_BAR = 1e-9     # the quotient's own error, as worked out in tests/test_rollout_estimated_sweep_host.py
DIST_BAR = 1e-10  # the family's bar for a roll-out (tests/test_gpu_tracking_estimated.py), which the yardstick itself must meet


def _all_cases():
    return [(False,) + c for c in XR.SCHEDULED] + [(True,) + c for c in XR.GUARDED]


def _build(guarded, *c):
    batch, Zref, x0, th, seed = XR.guarded_case(*c) if guarded else XR.scheduled_case(*c)
    return batch, Zref, x0, th, seed


# ---- 1. every case the GPU module runs, on the yardstick alone -------------------------------------------------------------
@pytest.mark.parametrize("case", _all_cases(), ids=str)
def test_gpu_cases_on_the_yardstick_alone(case):
    """Every case, ny and combination of K, model, wnoise and xhat0 of the GPU module under TEST_LIMITS: no problem is within
    MARGIN of a guard or of a limit (the GPU module may leave out LEFT_OUT of a case; the yardstick needs none), the loop stays
    bounded, float64 is within the family's bar of longdouble with the same record and knots, and every single call has channels
    that are free, on a lower and on an upper limit (the shares over the case are printed): the GPU module's clamp assertions
    are never vacuous."""
    guarded = case[0]
    batch, Zref, x0, th, seed = _build(*case)
    B, N = batch.B, batch.N
    worst, left, fmin, big, every = 0.0, 0, np.inf, 0.0, []
    for ny in XR.NYS:
        for flags in XR.FLAGS:
            inp = XR.call_inputs(seed + ny, B, N, ny, Zref, flags, th)
            r = XR.call_rollout(batch, Zref, inp, x0, LIM, guarded)
            out = XR.left_out(r, XR.MARGIN)
            left, fmin = max(left, int(out.sum())), min(fmin, float(r["fmargin"].min()))
            assert out.mean() <= XR.LEFT_OUT, (ny, flags, int(out.sum()))
            big = max(big, float(np.abs(r["Zout"]).max()), float(np.abs(r["Xhat"]).max()))
            every.append(r["sat"])
            assert min(XR.digit_shares(r["sat"])) > 0, (ny, flags)
            if flags in (XR.FLAGS[0], XR.FLAGS[-1]):  # the extended-precision restatement, on two of the sixteen
                e = XR.call_rollout(batch, Zref, inp, x0, LIM, guarded, np.longdouble)
                keep = ~out
                assert np.array_equal(r["sat"][keep], e["sat"][keep])
                for n in ("Zout", "Xhat", "innov") + (("events", "events_hat") if guarded else ()):
                    worst = max(worst, RR.rel(r[n][keep], e[n][keep].astype(np.float64)))
    free, lower, upper = XR.digit_shares(np.concatenate(every))
    print(f"{case}: free {free:.3f}, on the lower limit {lower:.3f}, on the upper {upper:.3f}; left out at most {left}; smallest force "
          f"margin {fmin:.1e}; max |x| {big:.1e}; float64 to longdouble {worst:.2e}")
    assert np.isfinite(big) and big < 1e4
    assert worst <= DIST_BAR


# ---- 2. exact statements of the yardstick ------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_without_limits_the_yardstick_is_the_estimated_yardstick(N, im, kt, B, ny, guarded):
    batch, inp = ES.case(N, im, kt, B, ny, guarded)
    for dt in (np.float64, np.longdouble):
        a, b = XR.case_rollout(batch, inp, XR.NO_LIMITS, guarded, dt), ES.rollout(batch, inp, guarded, dt)
        for n in b:
            assert np.array_equal(a[n], b[n]), n
        assert not a["sat"].any() and np.isinf(a["fmargin"]).all()


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_reduction_3_without_gains_and_process_noise_the_plant_is_the_limited_roll_out(N, im, kt, B, ny, guarded):
    """K None and wnoise None: Zout, the plant's record and sat are rollout_limited_ref's, whatever the filter does."""
    batch, inp = ES.case(N, im, kt, B, ny, guarded)
    inp = dict(inp, K=None, wnoise=None)
    a = XR.case_rollout(batch, inp, LIM, guarded)
    if guarded:
        zo, ev, sat, _, _ = LR.rollout(N, np.asarray(batch.init_mode), inp["Zref"], None, inp["x0"], inp["model"], LIM)
        assert np.array_equal(a["events"], ev)
    else:
        zo, sat, _ = LR.rollout_scheduled(N, np.asarray(batch.k_trans), np.asarray(batch.init_mode), inp["Zref"], None, inp["x0"],
                                          inp["model"], LIM)
    assert np.array_equal(a["Zout"], zo) and np.array_equal(a["sat"], sat) and sat.any()
    assert not np.array_equal(a["Xhat"][:, 1], a["Zout"][:, 20:35])  # the estimate is somewhere else


@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_reduction_4_without_filter_gains_the_scheduled_estimate_stays_on_the_limited_nominal(N, im, kt, B, ny):
    """Lgain = 0, xhat0 None, wnoise None and Zref the limited open-loop roll-out under the handle's model: whatever K is,
    Zout and sat are rollout_limited_ref's without gains."""
    batch, inp = ES.case(N, im, kt, B, ny, False)
    sched = (N, np.asarray(batch.k_trans), np.asarray(batch.init_mode))
    nominal, _, _ = LR.rollout_scheduled(*sched, inp["Zref"], None, inp["Zref"][:, :15], TC.SECOND, LIM)
    inp = dict(inp, Zref=nominal, Lgain=np.zeros_like(inp["Lgain"]), xhat0=None, wnoise=None)
    a = XR.case_rollout(batch, inp, LIM, False)
    zo, sat, _ = LR.rollout_scheduled(*sched, nominal, None, inp["x0"], inp["model"], LIM)
    assert np.array_equal(a["Zout"], zo) and np.array_equal(a["sat"], sat)
    zr = np.concatenate([nominal, np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15]
    assert np.array_equal(a["Xhat"], zr) and np.abs(inp["K"]).min() > 0


# ---- 3. the sweeps at fixed active set -----------------------------------------------------------------------------------------
def _trajectory(N, im, kt, B, ny, guarded, with_xhat0=True, ctype=np.complex128):
    batch, inp = ES.case(N, im, kt, B, ny, guarded)
    if not with_xhat0:
        inp = dict(inp, xhat0=None)
    out = XR.case_rollout(batch, inp, LIM, guarded)
    blk = ES.chain_blocks(N, np.asarray(batch.init_mode), np.asarray(batch.k_trans), out["Zout"], out["Xhat"], inp["model"],
                          TC.SECOND, guarded, out.get("events"), out.get("events_hat"), ctype=ctype)
    return batch, inp, out, blk


def _jvp(blk, inp, out, dirs):
    if inp["xhat0"] is not None and "xhat0_dot" not in dirs:
        dirs = dict(dirs, xhat0_dot=np.zeros_like(inp["xhat0"]))  # a given xhat0 held fixed: None would follow Zref_dot
    return XR.sweep_jvp(blk, out["sat"], inp["Zref"], inp["K"], inp["Lgain"], inp["H"], out["Zout"], out["Xhat"], out["innov"],
                        events=out.get("events"), events_hat=out.get("events_hat"), **dirs)


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_forward_sweep_matches_longdouble_central_differences_of_the_limited_roll_out(N, im, kt, B, ny, guarded):
    """All tangents together and each alone, and all but xhat0_dot on a roll-out with xhat0 = None, on the problems whose two
    touchdown knots and every saturation code are the same at +t, 0 and -t."""
    worst, left = 0.0, 0
    for with_xhat0 in (True, False):
        batch, inp, out, blk = _trajectory(N, im, kt, B, ny, guarded, with_xhat0)
        assert {0, 1, 2} <= set(np.unique(LR.unpack(out["sat"])))
        full, _ = ES.directions(N + ny, B, N, ny)
        if not with_xhat0:
            full = {k: v for k, v in full.items() if k != "xhat0_dot"}
        sets = [full] + ([{k: full[k]} for k in full] if with_xhat0 else [])
        for dirs in sets:
            fd, same, centre = XR.central_difference(batch, inp, LIM, guarded, dirs)
            assert np.array_equal(centre["sat"], out["sat"])
            assert (~same).mean() <= LEFT_OUT, f"{(~same).sum()} of {B} problems change a knot or a code over the step"
            left = max(left, int((~same).sum()))
            ref = _jvp(blk, inp, out, dirs)
            for name, q in fd.items():
                w = ES.worst(ref[name][same], q[same])
                worst = max(worst, w)
                assert w <= FD_BAR, (name, sorted(dirs), w)
    print(f"N={N} mode={im} k_trans={kt} B={B} ny={ny} guarded={guarded}: limited forward sweep against the longdouble quotient "
          f"{worst:.2e} of max(1, |ref|); bar {FD_BAR:.0e}; at most {left} of {B} problems left out")


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("with_xhat0", [True, False])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_reverse_sweep_is_the_adjoint_and_saturated_channels_get_exact_zeros(N, im, kt, B, ny, guarded, with_xhat0):
    batch, inp, out, blk = _trajectory(N, im, kt, B, ny, guarded, with_xhat0)
    dirs, cot = ES.directions(N + ny + 1, B, N, ny)
    if not with_xhat0:
        dirs = {k: v for k, v in dirs.items() if k != "xhat0_dot"}
    fwd = _jvp(blk, inp, out, dirs)
    rev = XR.sweep_vjp(blk, out["sat"], inp["Zref"], inp["K"], inp["Lgain"], inp["H"], out["Zout"], out["Xhat"], out["innov"],
                       cot["Zbar"], cot["Xhat_bar"], cot["innov_bar"], with_xhat0)
    lhs = sum(float(np.sum(cot[c] * fwd[o])) for c, o in (("Zbar", "Zout_dot"), ("Xhat_bar", "Xhat_dot"), ("innov_bar", "innov_dot")))
    rhs = sum(float(np.sum(rev[k[:-4] + "_bar"] * v)) for k, v in dirs.items())
    print(f"N={N} guarded={guarded} xhat0={with_xhat0}: <bar, J d> {lhs:.15e}, <J' bar, d> {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs))
    held = ~LR.free_channels(out["sat"])
    assert held.any() and not rev["K_bar"][held].any()
    zb = np.concatenate([rev["Zref_bar"], np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :-1, 15:19]
    assert not zb[held].any() and zb[~held].all()
    fz = np.concatenate([fwd["Zout_dot"], np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :-1, 15:19]
    assert not fz[held].any()


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_distance_of_the_float64_sweeps_from_their_longdouble_restatement(N, im, kt, B, ny, guarded):
    """Printed, and small against the GPU tests' bar of 1e-12: what that bar is widened by where it is not."""
    batch, inp, out, blk = _trajectory(N, im, kt, B, ny, guarded)
    _, _, _, blkl = _trajectory(N, im, kt, B, ny, guarded, ctype=np.clongdouble)
    dirs, cot = ES.directions(N + ny + 2, B, N, ny)
    args = (out["sat"], inp["Zref"], inp["K"], inp["Lgain"], inp["H"], out["Zout"], out["Xhat"], out["innov"])
    ev = dict(events=out.get("events"), events_hat=out.get("events_hat"))
    f, fl = XR.sweep_jvp(blk, *args, **dirs, **ev), XR.sweep_jvp(blkl, *args, **dirs, **ev)
    r, rl = XR.sweep_vjp(blk, *args, **cot), XR.sweep_vjp(blkl, *args, **cot)
    dist = max([ES.worst(f[k], fl[k]) for k in f] + [ES.worst(r[k], rl[k]) for k in r])
    print(f"N={N} mode={im} k_trans={kt} B={B} ny={ny} guarded={guarded}: float64 limited sweeps to longdouble {dist:.2e}")
    assert dist <= 1e-12


def test_sweeps_at_an_empty_active_set_are_the_estimated_yardsticks():
    N, im, kt, B, ny = CASES[0]
    batch, inp, out, blk = _trajectory(N, im, kt, B, ny, True)
    dirs, cot = ES.directions(3, B, N, ny)
    args = (inp["Zref"], inp["K"], inp["Lgain"], inp["H"], out["Zout"], out["Xhat"], out["innov"])
    ev = dict(events=out["events"], events_hat=out["events_hat"])
    zero = np.zeros_like(out["sat"])
    a, b = XR.sweep_jvp(blk, zero, *args, **dirs, **ev), ES.sweep_jvp(blk, *args, **dirs, **ev)
    assert all(np.array_equal(a[k], b[k]) for k in b)
    a, b = XR.sweep_vjp(blk, zero, *args, **cot), ES.sweep_vjp(blk, *args, **cot)
    assert all(np.array_equal(a[k], b[k]) for k in b)


# ---- 4. what of the entry points needs no device -------------------------------------------------------------------------------
NAMES = {"qln_tracking_rollout_estimated_limited": 19, "qln_tracking_rollout_estimated_limited_jvp": 24,
         "qln_tracking_rollout_estimated_limited_vjp": 22}


def test_ctypes_table():
    from quadruped_landing_amd import _lib

    for base, n in NAMES.items():
        for name in (base, base + "_host"):
            res, args = _lib.SIGNATURES[name]
            assert res is C.c_int and len(args) == n
            assert [i for i, a in enumerate(args) if a is C.c_int32] == ([5, 12] if n == 19 else [5])
            assert getattr(_lib.lib(), name).argtypes == args


def test_roll_out_rejects_bad_arguments_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    bad = _lib.QLN_ERR_INVALID_ARGUMENT
    a = np.zeros(2000)
    p = a.ctypes.data
    ok_lim = np.array(LIM)
    for name in ("qln_tracking_rollout_estimated_limited", "qln_tracking_rollout_estimated_limited_host"):
        fn = getattr(L, name)

        def call(lim=ok_lim, guarded=0, ev=None, eh=None, Lg=p, H=p, ny=8, Zref=p, Zout=p):
            return fn(None, Zref, None, Lg, H, ny, None, None, None, None, None, None if lim is None else lim.ctypes.data, guarded,
                      Zout, None, None, ev, eh, None)

        assert call() == bad and b"null handle" in L.qln_last_error()
        assert call(lim=None) == bad and b"null lim" in L.qln_last_error()
        for i, v in ((0, np.nan), (3, np.nan), (6, 99.0), (1, -1.0)):
            lim = ok_lim.copy()
            lim[i] = v
            assert call(lim=lim) == bad and b"not a {lo, hi} pair" in L.qln_last_error(), (i, v)
        inf = np.array([-np.inf, np.inf] * 4)
        assert call(lim=inf) == bad and b"null handle" in L.qln_last_error()
        assert call(ev=p) == bad and b"with guarded == 0" in L.qln_last_error()
        assert call(eh=p) == bad and b"with guarded == 0" in L.qln_last_error()
        assert call(ev=p, eh=p, guarded=1) == bad and b"null handle" in L.qln_last_error()
        for ny in (0, 9):
            assert call(ny=ny) == bad and b"ny must be" in L.qln_last_error()
        assert call(Lg=None) == bad and b"null Lgain or H" in L.qln_last_error()
        assert call(H=None) == bad and b"null Lgain or H" in L.qln_last_error()


def test_sweeps_reject_bad_arguments_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    bad = _lib.QLN_ERR_INVALID_ARGUMENT
    a = np.zeros(2000)
    p = a.ctypes.data
    for base in ("qln_tracking_rollout_estimated_limited_jvp", "qln_tracking_rollout_estimated_limited_vjp"):
        for name in (base, base + "_host"):
            fn = getattr(L, name)
            fwd = "jvp" in name

            def call(K=None, Lg=p, H=p, ny=8, Zout=p, Xhat=p, innov=None, ev=(None, None), sat=p, first=p, k_=None, l_=None, main=p,
                     dots=(None, None)):
                head = (None, p, K, Lg, H, ny, None, Zout, Xhat, innov) + ev + (sat,)
                if fwd:  # Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, Zout_dot, Xhat_dot, innov_dot, the event dots
                    return fn(*head, None, k_, l_, first, None, None, main, None, None, *dots)
                return fn(*head, main, None, None, None, k_, l_, first, None, None)  # Zbar, ..., K_bar, Lgain_bar, x0_bar, ...

            assert call() == bad and b"null handle" in L.qln_last_error()
            assert call(ev=(p, p)) == bad and b"null handle" in L.qln_last_error()
            assert call(sat=None) == bad and b"null sat" in L.qln_last_error()
            assert call(ev=(p, None)) == bad and b"exactly one of event and event_hat" in L.qln_last_error()
            assert call(ev=(None, p)) == bad and b"exactly one of event and event_hat" in L.qln_last_error()
            for ny in (0, 9, -1):
                assert call(ny=ny) == bad and b"ny must be" in L.qln_last_error()
            assert call(Lg=None) == bad and b"null Lgain or H" in L.qln_last_error()
            assert call(Zout=None) == bad and b"null Zref, Zout or Xhat" in L.qln_last_error()
            assert call(Xhat=None) == bad and b"null Zref, Zout or Xhat" in L.qln_last_error()
            assert call(l_=p) == bad and b"null innov" in L.qln_last_error()
            assert call(k_=p) == bad and b"needs K" in L.qln_last_error()
            assert call(main=None) == bad and (b"null Zout_dot" if fwd else b"null Zbar") in L.qln_last_error()
            if fwd:
                assert call(first=None) == bad and b"every tangent is NULL" in L.qln_last_error()
                assert call(dots=(p, None)) == bad and b"without event and event_hat" in L.qln_last_error()
                assert call(dots=(None, p)) == bad and b"without event and event_hat" in L.qln_last_error()
                assert call(ev=(p, p), dots=(p, p)) == bad and b"null handle" in L.qln_last_error()
