"""CPU checks of the forward sweep through the Kalman design (qln_kalman_design_jvp): the numpy yardstick
tests/tracking_kalman_sweep_ref.py against longdouble central differences of the design recursion itself
(tests/tracking_kalman_ref.py), in each tangent alone and in all together; the yardstick's float64 against its longdouble;
and the composition of HybridNLP.landing_loglik_jvp, restated in numpy, against longdouble central differences of the filter's
log-likelihood under redesign, down to V = 1e-6.

No bar is fixed in advance: a quotient is formed at t and at t/2 in longdouble, the distance of the two is the quotient's own
error, and ten times that is allowed.  Measured values: profiles/tracking_kalman_jvp_tests.txt."""
import functools

import numpy as np
import pytest

from tests import landing_filter_sweep_ref as FS
from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_ref as GR
from tests import rollout_guarded_sweep_ref as SR
from tests import rollout_ref as RR
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR
from tests import tracking_guarded_ref as TG
from tests import tracking_kalman_sweep_ref as KS
from tests.estimation_cases import measurement

LD = np.longdouble
T_STEP = 2.0 ** -20
# (N, k_trans, init_mode) on the knot schedule; (N, init_mode, B) through the guarded touchdown
SCHEDULED = [(5, 3, 2), (17, 6, 1)]
GUARDED = [(5, 2, 6), (17, 1, 3)]
NYS = (1, 3, 8)
ALONE = ("Sigma0", "W", "V", "all")


@functools.lru_cache(maxsize=None)
def _blocks(form, N, a, b):
    """The open-loop blocks A of one case, (B, N-1, 15, 15): complex-step blocks of the knot schedule at a reference, or of the
    guarded roll-out of rollout_guarded_cases.case (the touchdown knot's composite block included).  Shared, never changed."""
    if form == "scheduled":
        Zref, _, _, _ = TC.problem(N, a, b, 11 * N + a)
        return RR.complex_step_blocks(N, a, b, Zref)[None, :, :, :15], None
    _, Zref, K, x0, th = GC.case(N, a, b, False, True)
    Zout, ev, _, _ = GR.rollout(N, a, Zref, K, x0, th)
    F, _ = SR.blocks(N, a, Zout, th, ev)
    A, _ = TG.split(F)
    return A, ev


def _case(form, N, a, b, ny):
    A, ev = _blocks(form, N, a, b)
    rng = np.random.default_rng(1000 * N + 10 * ny + (form == "guarded"))
    H, V = measurement(rng, ny)
    B = len(A)
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    S0d, Wd, Vd = KS.directions(N + ny, ny, (B,))
    return A, H, V, S0, W, dict(Sigma0=(S0d, None, None), W=(None, Wd, None), V=(None, None, Vd), all=(S0d, Wd, Vd)), ev


CASES = [("scheduled",) + c for c in SCHEDULED] + [("guarded",) + c for c in GUARDED]


@pytest.mark.parametrize("ny", NYS)
@pytest.mark.parametrize("form,N,a,b", CASES)
def test_yardstick_against_longdouble_central_differences_of_the_design(form, N, a, b, ny):
    """Ld, Pd^+ (knot_rel) and logdet_dot (entry_rel) of the longdouble yardstick, at the gains of the longdouble design,
    against the design's central differences at t / 2; the bar is ten times the distance of the quotients at t and t / 2, in
    the same measure.  Every problem and every knot takes part."""
    A, H, V, S0, W, dirs, ev = _case(form, N, a, b, ny)
    if form == "guarded":
        assert (ev[:, 0] >= 0).any()
    base = KS.design(A, H, V, S0, W, LD)
    for which in ALONE:
        S0d, Wd, Vd = dirs[which]
        cast = lambda x: None if x is None else x.astype(LD)  # noqa: E731
        yard = KS.sweep(A.astype(LD), H.astype(LD), V.astype(LD), base["L"], cast(S0d), cast(Wd), cast(Vd))
        q1 = KS.design_quotient(A, H, V, S0, W, S0d, Wd, Vd, T_STEP)
        q2 = KS.design_quotient(A, H, V, S0, W, S0d, Wd, Vd, T_STEP / 2)
        own = KS.errors(q1, q2)
        err = KS.errors(yard, q2)
        print(f"design sweep {form} N={N} ny={ny} along {which}: yardstick to the quotient Ld {err[0]:.2e} Pd {err[1]:.2e} "
              f"logdet {err[2]:.2e}; the quotient's own error {own[0]:.2e} {own[1]:.2e} {own[2]:.2e}")
        for e, o in zip(err, own):
            assert e <= 10 * o, (which, err, own)
        assert np.array_equal(yard["Pd"], np.swapaxes(yard["Pd"], -1, -2))
        if which == "W":  # knot 0 sees no process noise
            assert not yard["Ld"][:, 0].any() and not yard["Pd"][:, 0].any() and not yard["logdet"][:, 0].any()


@pytest.mark.parametrize("ny", NYS)
@pytest.mark.parametrize("form,N,a,b", CASES)
def test_float64_yardstick_against_its_longdouble(form, N, a, b, ny):
    """The yardstick's own rounding at the float64 design's gains, to be set against the GPU test's 1e-10.  With V in [0.5, 2]
    against priors of order one, I - H L loses about a digit; 1e-11 leaves the GPU comparison a factor of ten."""
    A, H, V, S0, W, dirs, _ = _case(form, N, a, b, ny)
    L = KS.design(A, H, V, S0, W, np.float64)["L"]
    S0d, Wd, Vd = dirs["all"]
    lo = KS.sweep(A, H, V, L, S0d, Wd, Vd)
    hi = KS.sweep(A.astype(LD), H.astype(LD), V.astype(LD), L.astype(LD), S0d.astype(LD), Wd.astype(LD), Vd.astype(LD))
    e = KS.errors(lo, hi)
    print(f"design sweep {form} N={N} ny={ny}: float64 yardstick to longdouble Ld {e[0]:.2e} Pd {e[1]:.2e} logdet {e[2]:.2e}")
    assert max(e) <= 1e-11, e


def test_the_library_and_the_binding_have_the_sweep():
    """What this yardstick is the yardstick of: the four entries in the library (it loads without a device) and the binding's
    methods, whose composition composite() restates."""
    import inspect

    from quadruped_landing_amd import HybridNLP, _lib

    L = _lib.lib()
    for name in ("qln_kalman_design_jvp", "qln_kalman_design_jvp_host", "qln_kalman_design_guarded_jvp",
                 "qln_kalman_design_guarded_jvp_host"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    for method in ("tracking_kalman_jvp", "tracking_kalman_jvp_host"):
        p = inspect.signature(getattr(HybridNLP, method)).parameters
        assert list(p)[1:] == ["Zout", "Lgain", "H", "V", "Sigma0_dot", "W_dot", "V_dot", "events", "model", "guarded", "want"]
    assert HybridNLP.KALMAN_JVP_OUT == ("Lgain", "Pest", "logdet")
    assert {"Sigma0_dot", "W_dot", "V_dot", "events_hat", "guarded"} <= set(inspect.signature(HybridNLP.landing_loglik_jvp).parameters)


# ---- the composition of landing_loglik_jvp --------------------------------------------------------------------------------
def _loglik_under_redesign(batch, rec, guarded, A, S0, W, V, dtype):
    """(design in dtype at (S0, W, V), the replay of the record under its gains and V)"""
    d = KS.design(A, rec["H"], V, S0, W, dtype)
    return d, FS.replay(batch, rec, guarded, dtype, Lgain=d["L"], V=V)


@pytest.mark.parametrize("vscale", [1e-2, 1e-4, 1e-6])
@pytest.mark.parametrize("N,guarded", [(5, False), (17, False), (5, True), (17, True)])
def test_composite_against_central_differences_of_loglik_under_redesign(N, guarded, vscale):
    """The design runs along the record's reference (knot-schedule blocks, per record); the filter replays the flown record
    under the design's gains.  loglik_dot of the composition -- the yardstick's Ld and logdet_dot, landing_filter_sweep_ref's
    innov_dot under that Ld, the three einsums -- against the longdouble central difference of loglik with the gains designed
    again at both offsets.  V from 1e-2 down to 1e-6 against priors of 1e-6 .. 1e-4 puts the digit loss of I - H L on record."""
    ny, B = 3, 3
    batch, rec = FS.record(N, 1, max(2, N // 3), B, ny, guarded, seed=40 + N)
    rec = dict(rec)
    V = vscale * (1.0 + 0.25 * np.arange(ny))
    im, kt = np.asarray(batch.init_mode), np.asarray(batch.k_trans)
    A = np.stack([RR.complex_step_blocks(N, int(kt[b]), int(im[b]), rec["Zref"][b])[:, :, :15] for b in range(B)])
    rng = np.random.default_rng(N)
    S0, W = 1e-4 * CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-6, size=15)
    S0d, Wd, Vd = KS.directions(7 + N, ny, (B,))
    S0d, Wd, Vd = 1e-4 * S0d, 1e-4 * Wd, vscale * Vd

    def at(s):
        _, r = _loglik_under_redesign(batch, rec, guarded, A, S0.astype(LD) + LD(s) * S0d, W.astype(LD) + LD(s) * Wd,
                                      V.astype(LD) + LD(s) * Vd, LD)
        return r

    t = T_STEP
    c = at(0.0)
    quot = []
    for step in (t, t / 2):
        p, m = at(step), at(-step)
        if guarded:
            assert np.array_equal(p["events_hat"][:, 0], c["events_hat"][:, 0])
            assert np.array_equal(m["events_hat"][:, 0], c["events_hat"][:, 0])
        quot.append((p["loglik"] - m["loglik"]) / (2 * LD(step)))
    own = CR.entry_rel(quot[0], quot[1])
    worst = {}
    for dt in (LD, np.float64):
        d, r = _loglik_under_redesign(batch, rec, guarded, A, S0.astype(dt), W.astype(dt), V.astype(dt), dt)
        ctype = np.clongdouble if dt is LD else np.complex128
        F, T = FS.blocks(N, im, kt, rec["Zrec"], r["Xhat"], rec["model"], guarded, r.get("events_hat"), ctype=ctype)
        s = KS.sweep(A.astype(dt), rec["H"].astype(dt), V.astype(dt), d["L"], S0d.astype(dt), Wd.astype(dt), Vd.astype(dt))
        f = FS.sweep_jvp(F.real.astype(dt), T.real.astype(dt), d["L"], rec["H"], r["innov"], None, r.get("events_hat"),
                         Lgain_dot=s["Ld"])
        ll, _ = KS.composite(r["innov"], f["innov_dot"], d["L"], s["Ld"], rec["H"], V.astype(dt), Vd.astype(dt), s["logdet"])
        worst[dt] = CR.entry_rel(ll, quot[1])
    print(f"loglik under redesign N={N} guarded={guarded} V~{vscale:.0e}: composition to the quotient {worst[LD]:.2e} in "
          f"longdouble, {worst[np.float64]:.2e} in float64; the quotient's own error {own:.2e}")
    assert worst[LD] <= 10 * own, (worst, own)
