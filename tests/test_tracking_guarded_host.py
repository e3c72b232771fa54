"""The numpy yardstick of the gains and covariances through the guard-triggered touchdown (tests/tracking_guarded_ref.py),
held on the CPU without the library: the guarded Riccati to the LQ cost of the tangent sweep it is meant to minimise, the
guarded covariance to the sum of tangent sweeps over a factor of Sigma0, both through the yardstick of the sweeps
(tests/rollout_guarded_sweep_ref.py), which is itself held to differences of the guarded roll-out
(tests/test_rollout_guarded_sweeps_host.py).  The cases are tests/rollout_guarded_cases.py's, the ones the GPU runs
(tests/test_gpu_tracking_guarded.py); trajectory and events come from rollout_guarded_ref.rollout."""
import functools

import numpy as np
import pytest

from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_ref as GR
from tests import rollout_guarded_sweep_ref as SR
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR
from tests import tracking_guarded_ref as TG

# with gains: feedback and per-problem models; without: open loop at one model, as the GPU's cases
CASES = [("shape", N, im, B, wg) for (N, im, B) in GC.SHAPES for wg in (False, True)] + [("ragged", 12, 0, 70, True)]
# Both identities hold exactly in exact arithmetic; 1e-10 is the project's bar for these recursions against numpy
# (tests/test_gpu_tracking.py, tests/test_gpu_tracking_cov.py).  The GPU's oracle-free forms of the two comparisons take ten
# times the worst value measured here (tests/test_gpu_tracking_guarded.py).
IDENTITY_BAR = 1e-10
# A Riccati sweep without the saltation term must be told from the right one by the GPU's 1e-10 comparison: the gains of the
# blocks at frozen tau have to differ by orders more than that bar.
FROZEN_MISS = 1e-6


@functools.lru_cache(maxsize=None)
def _case(kind, N, im, B, wg):
    """One case: the guarded roll-out, its blocks, the guarded gains.  Shared by the tests of the case; nothing here is
    changed afterwards."""
    if kind == "shape":
        _, Zref, K, x0, th = GC.case(N, im, B, wg, wg)
        ims = im
    else:
        batch, Zref, K, x0, th = GC.ragged_case()
        ims = np.asarray(batch.init_mode)
    Zout, ev, _, _ = GR.rollout(N, ims, Zref, K, x0, th)
    F, T = SR.blocks(N, ims, Zout, th, ev)
    Kg, Pg = TG.riccati(F, TC.QW, TC.R, TC.QFW)
    return (Zref, K, x0, th, ims), (Zout, ev), (F, T), (Kg, Pg)


@pytest.mark.parametrize("kind,N,im,B,wg", CASES)
def test_cost_to_go_is_the_lq_cost_of_the_tangent_sweep_under_the_returned_gains(kind, N, im, B, wg):
    """x' P_0 x = sum_k dx_k'Q dx_k + dF_k'R dF_k + dx_N'Qf dx_N along sweep_jvp(x0_dot = x) with dF = -K dx.  Measured worst
    8.15e-15 of the cost."""
    (Zref, _, _, _, _), (Zout, ev), (F, T), (Kg, Pg) = _case(kind, N, im, B, wg)
    x = np.random.default_rng(N + B).normal(size=(B, 15))
    zd, _ = SR.sweep_jvp(F, T, ev, Zout, Kg, Zout, None, None, x, None)
    cost = TG.lq_cost(zd, N, TC.QW, TC.R, TC.QFW)
    quad = np.einsum("bi,bij,bj->b", x, Pg[:, 0], x)
    w = float(np.max(np.abs(cost - quad) / np.abs(cost)))
    print(f"{kind} N={N} mode={im} B={B} K={wg}: x'P_0 x against the sweep's LQ cost {w:.2e}")
    assert w <= IDENTITY_BAR and (ev[:, 0] >= 0).any()
    assert np.array_equal(Pg, np.swapaxes(Pg, -1, -2))


@pytest.mark.parametrize("kind,N,im,B,wg,closed", [c + (closed,) for c in CASES for closed in ((True, False) if c[4] else (False,))])
def test_covariance_without_noise_is_the_sum_of_tangent_sweeps_over_a_factor_of_sigma0(kind, N, im, B, wg, closed):
    """Sigma_k = sum_i z_i,k z_i,k' for dx_0 = column i of G, Sigma0 = G G'; event_var the same sums over event_dot's d tau and
    clock tangent.  Measured worst 2.7e-15 (knot_rel of Sigma), 6.5e-16 (event_var)."""
    (Zref, K, _, th, _), (Zout, ev), (F, T), _ = _case(kind, N, im, B, wg)
    Kc = K if closed else None
    G = np.random.default_rng(7 * N + B).normal(size=(15, 15)) / 4
    S, mg, var = TG.covariance(F, T, ev, Kc, G @ G.T, None, Zout[:, 2::20], th[:, 3])
    acc, vacc = np.zeros_like(S), np.zeros_like(var)
    for i in range(15):
        zd, ed = SR.sweep_jvp(F, T, ev, Zout, Kc, Zout, None, None, np.tile(G[:, i], (B, 1)), None)
        z = np.concatenate([zd, np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15]
        acc += np.einsum("bki,bkj->bkij", z, z)
        vacc += ed[:, 1:3] ** 2
    ws, wv = CR.knot_rel(S, acc), SR.worst(var, vacc)
    print(f"{kind} N={N} mode={im} B={B} K={wg} closed={closed}: Sigma {ws:.2e}, event_var {wv:.2e}")
    assert ws <= IDENTITY_BAR and wv <= IDENTITY_BAR
    land = ev[:, 0] >= 0
    assert land.any() and (var[land, 1] > 0).all() and not var[~land].any()
    assert np.array_equal(S, np.swapaxes(S, -1, -2))


@pytest.mark.parametrize("kind,N,im,B,wg", CASES)
def test_a_knots_quadratic_form_is_the_reverse_sweeps_x0_bar_in_sigma0(kind, N, im, B, wg):
    """Without noise, zbar' Sigma_k zbar = x0_bar' Sigma0 x0_bar for the reverse sweep of a cotangent zbar on x_k alone: the
    comparison the GPU makes between its own two kernels.  Measured worst 1.46e-14 of the quadratic form (N = 61, open loop)."""
    (Zref, K, _, th, _), (Zout, ev), (F, T), _ = _case(kind, N, im, B, wg)
    rng = np.random.default_rng(3 * N + B)
    S0 = CR.random_psd(rng, shape=(B,))
    S, _, _ = TG.covariance(F, T, ev, K, S0, None, Zout[:, 2::20], th[:, 3])
    worst = 0.0
    for k in sorted({N - 1, N // 2 + 1} & set(range(1, N))):
        Zbar = np.zeros_like(Zout)
        Zbar[:, 20 * k: 20 * k + 15] = rng.normal(size=(B, 15))
        _, _, xb, _ = SR.sweep_vjp(F, Zref, K, Zout, Zbar)
        lhs = np.einsum("bi,bij,bj->b", Zbar[:, 20 * k: 20 * k + 15], S[:, k], Zbar[:, 20 * k: 20 * k + 15])
        rhs = np.einsum("bi,bij,bj->b", xb, S0, xb)
        worst = max(worst, float(np.max(np.abs(lhs - rhs) / np.abs(rhs))))
    print(f"{kind} N={N} mode={im} B={B} K={wg}: zbar'Sigma_k zbar against x0_bar'Sigma0 x0_bar {worst:.2e}")
    assert worst <= IDENTITY_BAR


@pytest.mark.parametrize("kind,N,im,B,wg", CASES)
def test_gains_on_blocks_with_tau_frozen_differ_visibly(kind, N, im, B, wg):
    """What the saltation term is worth: the gains of the same recursion on blocks without it.  Measured knot_rel of K:
    3.1e-3 (N = 2) .. 3.8e-2 (N = 61) over the shapes, 2.5e-2 ragged."""
    (_, _, _, th, ims), (Zout, ev), _, (Kg, _) = _case(kind, N, im, B, wg)
    Ff, _ = SR.blocks(N, ims, Zout, th, ev, freeze_tau=True)
    Kf, _ = TG.riccati(Ff, TC.QW, TC.R, TC.QFW)
    land = ev[:, 0] >= 0
    w = CR.knot_rel(Kf[land], Kg[land])
    print(f"{kind} N={N} mode={im} B={B} K={wg}: gains at frozen tau differ by {w:.2e} (knot_rel)")
    assert w > FROZEN_MISS
    assert np.array_equal(Kf[~land], Kg[~land])


@pytest.mark.parametrize("kind,N,im,B,wg", CASES)
def test_the_float64_yardstick_is_close_to_its_longdouble_restatement(kind, N, im, B, wg):
    """Recorded per shape; the GPU tests take 100 times these as their bar where that exceeds 1e-10.  Measured worst: K 2.3e-13
    (N = 61), P 1.6e-14, Sigma 3.9e-15, marg 1.4e-13, event_var 2.0e-15: no bar moves."""
    (_, K, _, th, ims), (Zout, ev), _, _ = _case(kind, N, im, B, wg)
    rng = np.random.default_rng(N)
    d = TG.distances(N, ims, Zout, th, ev, K, TC.QW, TC.R, TC.QFW, CR.random_psd(rng, shape=(B,)), rng.uniform(0, 1e-2, 15))
    print(f"{kind} N={N} mode={im} B={B} K={wg}: float64 to longdouble K {d[0]:.2e}, P {d[1]:.2e}, Sigma {d[2]:.2e}, marg {d[3]:.2e}, "
          f"event_var {d[4]:.2e}")
    assert max(d) <= 1e-9
