"""CPU checks of the estimate-feedback roll-out (qln_tracking_rollout_estimated / _guarded): the numpy yardstick
tests/rollout_estimated_ref.py against the roll-out yardsticks it reduces to, against the linear joint recursion of
tests/tracking_kalman_ref.py to second order, and -- sampled 4 096 times -- against the covariances the Kalman layer predicts;
argument validation that needs no device; the ctypes table."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import rollout_estimated_cases as EC
from tests import rollout_estimated_ref as ER
from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_ref as GR
from tests import rollout_guarded_sweep_ref as SR
from tests import rollout_ref as RR
from tests import tracking_cases as TC
from tests import tracking_guarded_ref as TG
from tests import tracking_kalman_ref as KR
from tests import tracking_ref as TR


# ---- 1. no gain: the roll-outs it is built from, exactly --------------------------------------------------------------------
@pytest.mark.parametrize("N,k_trans,init_mode", TC.CASES)
@pytest.mark.parametrize("ny", [1, 8])
def test_without_filter_gains_the_knot_scheduled_form_is_the_model_roll_out(N, k_trans, init_mode, ny):
    B = 6
    batch = TC.batch(B, N, k_trans, init_mode, seed=N + k_trans)
    rng = np.random.default_rng(N)
    Zref = np.ascontiguousarray(batch.Z, dtype=np.float64)
    x0 = Zref[:, :15] + 1e-2 * rng.normal(size=(B, 15))
    th = RR.draw_models(B, N, TC.SECOND)
    d = EC.draws(N, B, N, ny)
    out = ER.rollout(N, init_mode, Zref, None, np.zeros_like(d["Lgain"]), d["H"], x0, th, TC.SECOND, d["vnoise"], None, None, k_trans)
    assert np.array_equal(out["Zout"], RR.rollout(N, k_trans, init_mode, Zref, None, x0, th))
    hat = RR.rollout(N, k_trans, init_mode, Zref, None, Zref[:, :15], np.tile(TC.SECOND, (B, 1)))
    assert np.array_equal(out["Xhat"], np.concatenate([hat, np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15])
    # the innovation is what the measurement says of the distance between the two
    z = np.concatenate([out["Zout"], np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15]
    np.testing.assert_allclose(out["innov"], (z - out["Xhat"]) @ d["H"].T + d["vnoise"], rtol=0, atol=1e-13)


@pytest.mark.parametrize("N,init_mode,B", GC.SHAPES)
def test_without_filter_gains_the_guarded_form_is_the_guarded_roll_out(N, init_mode, B):
    batch, Zref, _, x0, th = GC.case(N, init_mode, B, False, True)
    d = EC.draws(N, B, N, 3)
    out = ER.rollout(N, init_mode, Zref, None, np.zeros_like(d["Lgain"]), d["H"], x0, th, TC.SECOND, d["vnoise"], guarded=True)
    Zo, ev, mg, _ = GR.rollout(N, init_mode, Zref, None, x0, th)
    assert np.array_equal(out["Zout"], Zo) and np.array_equal(out["events"], ev) and np.array_equal(out["margin"], mg)
    Zh, evh, mgh, _ = GR.rollout(N, init_mode, Zref, None, Zref[:, :15], TC.SECOND)
    assert np.array_equal(out["Xhat"], np.concatenate([Zh, np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15])
    assert np.array_equal(out["events_hat"][:, :6], evh[:, :6]) and np.array_equal(out["margin_hat"], mgh)
    assert (ev[:, 0] >= 0).any() and ev[B - 1, 0] == -1


def test_the_yardstick_is_dtype_generic():
    N, init_mode, B = 8, 1, 48
    batch, Zref, K, x0, th = GC.case(N, init_mode, B, True, True)
    d = EC.draws(5, B, N, 3)
    args = (N, init_mode, Zref, K, d["Lgain"], d["H"], x0, th, TC.SECOND, d["vnoise"], d["wnoise"], Zref[:, :15] + d["dxhat0"])
    lo, hi = ER.rollout(*args, guarded=True), ER.rollout(*args, guarded=True, dtype=np.longdouble)
    assert hi["Zout"].dtype == np.longdouble and hi["events_hat"].dtype == np.longdouble
    ok = np.minimum(lo["margin"], lo["margin_hat"]) >= GC.MARGIN
    assert ok.mean() >= 1 - GC.LEFT_OUT
    for name in ("Zout", "Xhat", "innov", "events", "events_hat"):
        assert RR.rel(lo[name][ok], hi[name][ok].astype(np.float64)) <= 1e-12, name


# ---- 2. second order against the linear joint recursion -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nominal(guarded):
    """The notebook problem at tests/golden/data_6.csv, the nominal re-rolled open loop from the file's controls (guarded: the
    free foot dropped 2 cm higher than planned), its step blocks and the numpy Riccati gains along it."""
    nb = EC.notebook()
    N, kt, im = nb.N, int(nb.k_trans[0]), int(nb.init_mode[0])
    th = np.array(nb.model.plant_parameters())
    x0 = nb.x0[0].copy()
    if guarded:
        x0[6] += EC.MC_HEIGHT
        zn, ev, _, _ = GR.rollout(N, im, nb.Z, None, x0[None], th)
        F, T = SR.blocks(N, im, zn, th[None], ev)
        A, Bm = TG.split(F[0])
        zn = zn[0]
    else:
        zn = RR.rollout(N, kt, im, nb.Z[0], None, x0, th)
        F = RR.complex_step_blocks(N, kt, im, zn, th)
        A, Bm, ev, T = F[:, :, :15], F[:, :, 15:19], None, None
    K, _ = TR.riccati(A, Bm, EC.Q, EC.R, EC.Q)
    return dict(N=N, kt=kt, im=im, th=th, x0=x0, zn=zn, A=A, Bm=Bm, K=K, ev=ev, F=F, T=T)


@pytest.mark.parametrize("guarded", [False, True])
def test_deviations_agree_with_the_linear_joint_recursion_to_second_order(guarded):
    """Perturbations of size eps in x0, xhat0 and both noises: the yardstick's deviation from the nominal minus the linear
    recursion of (dx, xhat^-) driven by the same samples is a remainder c eps^2 (1 + O(eps)); halving eps quarters it.  At
    eps = 1e-3 and 5e-4 the cubic term moves the quotient by a few eps times the trajectory's scale, and rounding (1e-16 of
    states of size 1 against remainders of 1e-5) does not reach it: the quotient is asserted within 10 % of 1/4."""
    nom = _nominal(guarded)
    N, H = nom["N"], EC.sensors()
    B = 16
    S0, _, _, _, _, _ = EC.mc_draws(1, N, 1e-3, EC.MC_W, S=1)
    L = KR.recursion(nom["A"], nom["Bm"], nom["K"], H, np.full(8, 1e-6), S0, EC.MC_W)["L"]
    rng = np.random.default_rng(7)
    # directions in the proportions the filter is designed for: drop state and estimate 0.1, sensors 1, process 0.01
    d0, dh, v, w = (c * rng.normal(size=s) for c, s in ((0.1, (B, 15)), (0.1, (B, 15)), (1.0, (B, N, 8)), (0.01, (B, N - 1, 15))))
    rep = lambda a: np.broadcast_to(a, (B,) + a.shape)  # noqa: E731
    zn = np.concatenate([nom["zn"], np.zeros(5)]).reshape(N, 20)[:, :15]

    def remainder(eps):
        out = ER.rollout(N, nom["im"], rep(nom["zn"]), rep(nom["K"]), rep(L), H, nom["x0"] + eps * d0, nom["th"], nom["th"],
                         eps * v, eps * w, nom["zn"][:15] + eps * dh, nom["kt"], guarded)
        if guarded:
            assert (out["events"][:, 0] == nom["ev"][0, 0]).all() and (out["events_hat"][:, 0] == nom["ev"][0, 0]).all()
        dx, xh, iv = ER.linear_joint(nom["A"], nom["Bm"], nom["K"], L, H, eps * d0, eps * v, eps * w, eps * dh)
        z = np.concatenate([out["Zout"], np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15]
        return max(np.abs(z - zn - dx).max(), np.abs(out["Xhat"] - zn - xh).max()), np.abs(out["innov"] - iv).max(), np.abs(dx).max()

    (r1, i1, size), (r2, i2, _) = remainder(1e-3), remainder(5e-4)
    print(f"guarded={guarded}: deviations up to {size:.2e}; remainder {r1:.3e} -> {r2:.3e} (quotient {r2 / r1:.4f}), of the "
          f"innovations {i1:.3e} -> {i2:.3e} (quotient {i2 / i1:.4f})")
    assert r1 < 1e-2 * size
    assert abs(r2 / r1 - 0.25) <= 0.025 and abs(i2 / i1 - 0.25) <= 0.025


# ---- 3. the sampled closed loop against the Kalman layer's predictions -----------------------------------------------------
@pytest.mark.parametrize("guarded,setting", [(False, 0), (True, 0), (False, 1), (True, 2)])
def test_monte_carlo_of_4096_noisy_landings_on_the_yardstick(guarded, setting):
    """S = 4 096 landings of the notebook problem with drop states ~ N(x0, Sigma_0), sensor and process noise, flown by the
    yardstick under the numpy Riccati gains and the filter gains of tracking_kalman_ref.  At every knot and along 32 fixed
    directions each, the sample variance of the true state's deviation, of the estimation error and of the innovation over the
    predicted X_k, P^+_k and S_k lies within 1 +- 5 sqrt(2 / (S - 1)) = 1 +- 0.1105.  The guarded experiment lands in knot 19
    at tau / h = 0.50, plant and estimator in the same knot in every sample."""
    nom = _nominal(guarded)
    N, H, S = nom["N"], EC.sensors(), EC.MC_S
    sd, W, seed = EC.MC_SETTINGS[setting]
    S0, dx0, v, w, Wx, Wy = EC.mc_draws(seed, N, sd, W)
    V = np.full(8, sd * sd)
    r = KR.recursion(nom["A"], nom["Bm"], nom["K"], H, V, S0, W)
    rep = lambda a: np.broadcast_to(a, (S,) + a.shape)  # noqa: E731
    out = ER.rollout(N, nom["im"], rep(nom["zn"]), rep(nom["K"]), rep(r["L"]), H, nom["x0"] + dx0, nom["th"], nom["th"], v, w, None,
                     nom["kt"], guarded)
    worst = EC.mc_worst(out["Zout"], out["Xhat"], out["innov"], nom["zn"], r["X"], r["Pp"], EC.innovation_covariances(r["Pm"], H, V),
                        Wx, Wy)
    print(f"guarded={guarded} sensor sd {sd:.0e} W {'1e-10' if W is not None else '0'} seed {seed}: worst |ratio - 1| X "
          f"{worst['X']:.4f}, P+ {worst['P+']:.4f}, S {worst['S']:.4f}; band {EC.band():.4f}")
    assert max(worst.values()) <= EC.band(), worst
    if guarded:
        ks = nom["ev"][0, 0]
        tau_h = nom["ev"][0, 1] / nom["zn"][20 * int(ks) + 19]
        differing = float(np.mean(out["events"][:, 0] != out["events_hat"][:, 0]))
        g = KR.guarded(nom["F"], nom["T"], nom["ev"], nom["K"][None], H, V, S0, W, nom["zn"][None, 2::20], nom["th"][None, 3])
        clock = float(np.var(out["events"][:, 2], ddof=1) / g["event_var"][0, 1])
        print(f"  touchdown in knot {ks:.0f} at tau / h = {tau_h:.2f}; plant and estimator land in different knots in "
              f"{differing:.4f} of the samples; touchdown-clock variance over event_var[1]: {clock:.4f}")
        assert ks == 19 and abs(tau_h - 0.5) < 0.01
        assert (out["events"][:, 0] == ks).all() and differing == 0.0
        assert abs(clock - 1.0) <= EC.band()


# ---- 4. argument validation that needs no device -----------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    bad = _lib.QLN_ERR_INVALID_ARGUMENT
    z, k, lg, Hm, out = np.zeros(100), np.zeros(60), np.zeros(1000), np.zeros((8, 15)), np.zeros(1000)
    p = lambda a: a.ctypes.data  # noqa: E731
    for name in ("qln_tracking_rollout_estimated", "qln_tracking_rollout_estimated_host", "qln_tracking_rollout_estimated_guarded",
                 "qln_tracking_rollout_estimated_guarded_host"):
        fn = getattr(L, name)
        tail = (None, None) if "guarded" in name else ()
        call = lambda Lg, H, ny: fn(None, p(z), p(k), Lg, H, ny, None, None, None, None, None, p(out), None, None, *tail)  # noqa: E731
        assert call(p(lg), p(Hm), 8) == bad and b"null handle" in L.qln_last_error()
        assert call(p(lg), p(Hm), 1) == bad and b"null handle" in L.qln_last_error()
        for ny in (0, 9, -1):
            assert call(p(lg), p(Hm), ny) == bad and b"ny must be" in L.qln_last_error()
        assert call(None, p(Hm), 8) == bad and b"null Lgain or H" in L.qln_last_error()
        assert call(p(lg), None, 8) == bad and b"null Lgain or H" in L.qln_last_error()


# ---- 5. the ctypes table ---------------------------------------------------------------------------------------------------
def test_ctypes_table():
    from quadruped_landing_amd import _lib

    for name, n in (("qln_tracking_rollout_estimated", 14), ("qln_tracking_rollout_estimated_host", 14),
                    ("qln_tracking_rollout_estimated_guarded", 16), ("qln_tracking_rollout_estimated_guarded_host", 16)):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n
        assert [i for i, a in enumerate(args) if a is C.c_int32] == [5]
        assert getattr(_lib.lib(), name).argtypes == args
