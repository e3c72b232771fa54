"""CPU checks of the roll-out with a per-problem plant model: the numpy restatement with explicit (g, mb, mf, lb) equals the
oracle's roll-out under np_oracle.model(...) exactly; its complex-step blocks [A B G] against central differences on single
steps of every mode; both sweeps against a complex step of the whole roll-out in a model direction; the adjoint identity of
the two numpy sweeps; G's structural pattern; argument validation that needs no device and the ctypes table.  The models are
drawn around the second model (tests/tracking_cases.py), never the default: there 1/mb == mf and lb*lb == lb/2 hold bit for
bit, and a confused parameter passes."""
import numpy as np
import pytest

from tests import rollout_ref as RR
from tests import tracking_cases as TC
from tests.tracking_cases import CASES

# G's pattern from the derivation: (row, parameter) pairs that can be non-zero in some mode
PATTERN = ({(r, 0) for r in (1, 2, 4, 6, 8, 9, 11, 13)} | {(r, 1) for r in (0, 1, 2, 7, 8, 9)}
           | {(r, 2) for r in (3, 4, 5, 6, 10, 11, 12, 13)} | {(2, 3), (9, 3)})


def _model(seed):
    return RR.draw_models(1, seed, TC.SECOND)[0]


@pytest.mark.parametrize("N,k_trans,init_mode", CASES)
@pytest.mark.parametrize("with_gains", [False, True])
def test_restatement_equals_the_oracle_rollout_under_the_model_exactly(N, k_trans, init_mode, with_gains):
    from oracle import np_oracle as O

    Zref, K, x0, _ = TC.problem(N, k_trans, init_mode, seed=10 * N + k_trans)
    K = K if with_gains else None
    th = _model(N + k_trans)
    with O.model(*th):
        ref = RR.rollout(N, k_trans, init_mode, Zref, K, x0)
        F_ref = RR.complex_step_blocks(N, k_trans, init_mode, ref)
    got = RR.rollout(N, k_trans, init_mode, Zref, K, x0, th)
    assert np.array_equal(got, ref)
    assert not np.array_equal(got, RR.rollout(N, k_trans, init_mode, Zref, K, x0))  # and the model is read
    # the [A B] part of the blocks is the oracle's (to rounding: a complex model makes tau / Ib a complex division), with
    # the same zeros, and a batch of blocks is the single ones stacked
    F = RR.complex_step_blocks(N, k_trans, init_mode, got, th)
    assert RR.rel(F[:, :, :20], F_ref) <= 1e-14 and np.array_equal(F[:, :, :20] == 0.0, F_ref == 0.0)
    Fb = RR.complex_step_blocks(N, k_trans, init_mode, np.stack([got, got]), np.stack([th, TC.SECOND]))
    assert np.array_equal(Fb[0], F)


# mode 3 has no jump knot: the jump follows the last knot of the initial mode
@pytest.mark.parametrize("mode,jump", [(1, False), (1, True), (2, False), (2, True), (3, False)])
def test_G_by_complex_step_against_central_differences_and_its_pattern(mode, jump):
    """Single steps at the second model: complex-step G_k against a 1e-5-relative central difference, as a fraction of the
    block's largest entry.  The bar is the quotient's own error.  Truncation: every entry is the derivative of a
    power law th^-q in its parameter, and a central difference with step rel |th| errs by (q + 1)(q + 2) / 6 rel^2 of the
    entry: nothing for g (linear), rel^2 for 1/mb and 1/mf, 2 rel^2 = 2e-10 for the lb column (1/Ib ~ lb^-2) -- which is the
    whole figure where the lb column holds the block's largest entry (at the jump and in mode 3, where no free foot's
    1/mf^2 entries lead).  Rounding: the two stepped states carry about an ulp each of the largest state
    entry, divided by the step: 2 u max|x+| / (2 rel min|th_p|), as a fraction of the largest entry of G.  Outside the
    derivation's pattern the complex step leaves rounding only (mf's and mb's acceleration paths into theta and omega cancel
    algebraically, not numerically); inside it every entry is alive in the mode that frees its foot."""
    # A landing's knots behind the touchdown, where both feet carry force, stepped under every mode's flags (the closed
    # loop's feedback puts force on a free foot too).  The 1/mf^2 entries then lead the block; where the lb column leads, its
    # own truncation error, 2 rel^2 of the entry for a 1/lb^2 law, is the whole of the bar.
    Zref, _, _, _ = TC.problem(8, 5, 1, seed=10 * mode + jump)
    worst = bar = 0.0
    for k in (4, 5, 6):
        x, u = Zref[20 * k: 20 * k + 15], Zref[20 * k + 15: 20 * k + 20]
        th = TC.SECOND
        z = np.concatenate([x, u])
        # one knot as a two-knot trajectory: k_trans = 2 puts the jump at knot 0, a later k_trans none
        kt, im = (2, mode) if jump else ((3, mode) if mode != 3 else (1, 1))
        Zo = np.concatenate([z, np.zeros(15)])
        G = RR.complex_step_blocks(2, kt, im, Zo, th)[0][:, 20:]
        fd = RR.central_difference_G(mode, jump, x, u, th, rel=1e-5)
        scale = np.abs(G).max()
        worst = max(worst, float(np.abs(G - fd).max() / scale))
        xn = RR.model_step(mode, jump, x, u, th)
        bar = max(bar, 2.0 * 1e-5**2 + 2.0 * np.finfo(float).eps * np.abs(xn).max() / (2 * 1e-5 * np.abs(th).min()) / scale)
        for r in range(15):
            for p in range(4):
                if (r, p) not in PATTERN:
                    assert abs(G[r, p]) <= 1e-13 * scale, (r, p, G[r, p])
        assert np.all(G[14] == 0.0)
        if jump:
            assert np.all(G[[4, 6, 10, 11, 12, 13]] == 0.0)
        free = {1: (5, 6, 12, 13), 2: (3, 4, 10, 11), 3: ()}[mode]
        alive = {(r, p) for (r, p) in PATTERN if (p != 2 or r in free) and (p != 0 or r in (1, 2, 8, 9) or r in free)}
        if jump:
            alive = {(r, p) for (r, p) in alive if r not in (4, 6, 10, 11, 12, 13)}
        for (r, p) in alive:
            assert G[r, p] != 0.0, (r, p)
    # The bar stands above the 2e-10 this comparison was first reported to reach: that figure is the lb column's truncation
    # alone, and the rounding term comes on top of it (the worst case measured here is 2.3e-10, at the jump of mode 1).
    print(f"mode {mode} jump {jump}: complex-step G against central differences {worst:.2e} of the largest entry, bar {bar:.2e}")
    assert worst <= bar, (worst, bar)


@pytest.mark.parametrize("N,k_trans,init_mode", CASES)
@pytest.mark.parametrize("with_gains", [False, True])
def test_sweeps_match_complex_step_of_the_whole_rollout_in_a_model_direction(N, k_trans, init_mode, with_gains):
    Zref, K, x0, Zbar = TC.problem(N, k_trans, init_mode, seed=10 * N + k_trans)
    K = K if with_gains else None
    th = _model(3 * N + k_trans)
    rng = np.random.default_rng(7 * N + k_trans)
    zd = rng.normal(size=20 * N - 5)
    kd = rng.normal(size=(N - 1, 4, 15)) if with_gains else None
    xd = rng.normal(size=15)
    md = th * rng.normal(size=4)
    Zout = RR.rollout(N, k_trans, init_mode, Zref, K, x0, th)
    F = RR.complex_step_blocks(N, k_trans, init_mode, Zout, th)
    for dots in ((zd, kd, xd, md), (None, None, None, md), (zd, kd, xd, None)):
        got = RR.sweep_jvp(F, Zref, K, Zout, *dots)
        ref = RR.jvp_complex_step(N, k_trans, init_mode, Zref, K, x0, th, *dots)
        assert RR.rel(got, ref) <= 1e-8, RR.rel(got, ref)
    # the reverse sweep: model_bar by one complex roll-out per parameter, the other three as without a model
    zb, kb, xb, mb = RR.sweep_vjp(F, Zref, K, Zout, Zbar)
    mc = np.array([RR.jvp_complex_step(N, k_trans, init_mode, Zref, K, x0, th, model_dot=e) @ Zbar for e in np.eye(4)])
    assert RR.rel(mb, mc) <= 1e-8, RR.rel(mb, mc)
    z0, k0, x0b, _ = RR.sweep_vjp(F[:, :, :20], Zref, K, Zout, Zbar)
    assert np.array_equal(zb, z0) and np.array_equal(xb, x0b) and (kb is None or np.array_equal(kb, k0))
    # and the two sweeps are adjoint
    out = RR.sweep_jvp(F, Zref, K, Zout, zd, kd, xd, md)
    lhs = float(Zbar @ out)
    rhs = float(zb @ zd + xb @ xd + mb @ md + (0.0 if kb is None else kb.reshape(-1) @ kd.reshape(-1)))
    assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs)), (lhs, rhs)


@pytest.mark.parametrize("N,k_trans,init_mode", CASES)
@pytest.mark.parametrize("with_gains", [False, True])
def test_sweeps_on_blocks_with_G_reduce_to_the_sweeps_without_it_exactly(N, k_trans, init_mode, with_gains):
    """One statement of each sweep serves blocks with and without G: on [A B G] whose [A B] is a set of 20-column blocks,
    the reverse sweep's first three outputs, and the forward sweep with model_dot None or all zeros, are the 20-column
    sweeps' bit for bit."""
    Zref, K, x0, Zbar = TC.problem(N, k_trans, init_mode, seed=10 * N + k_trans)
    K = K if with_gains else None
    th = _model(3 * N + k_trans)
    rng = np.random.default_rng(7 * N + k_trans)
    zd = rng.normal(size=20 * N - 5)
    kd = rng.normal(size=(N - 1, 4, 15)) if with_gains else None
    xd = rng.normal(size=15)
    Zout = RR.rollout(N, k_trans, init_mode, Zref, K, x0, th)
    F20 = RR.complex_step_blocks(N, k_trans, init_mode, Zout)
    F24 = np.concatenate([F20, RR.complex_step_blocks(N, k_trans, init_mode, Zout, th)[:, :, 20:]], axis=2)
    assert F24.shape == (N - 1, 15, 24) and np.array_equal(F24[:, :, :20], F20) and F24[:, :, 20:].any()
    zb, kb, xb, mb = RR.sweep_vjp(F24, Zref, K, Zout, Zbar)
    z0, k0, x0b, m0 = RR.sweep_vjp(F20, Zref, K, Zout, Zbar)
    assert m0 is None and mb.any()
    assert np.array_equal(zb, z0) and np.array_equal(xb, x0b) and ((kb is None and k0 is None) or np.array_equal(kb, k0))
    ref = RR.sweep_jvp(F20, Zref, K, Zout, zd, kd, xd)
    assert np.array_equal(RR.sweep_jvp(F24, Zref, K, Zout, zd, kd, xd, None), ref)
    assert np.array_equal(RR.sweep_jvp(F24, Zref, K, Zout, zd, kd, xd, np.zeros(4)), ref)
    assert not np.array_equal(RR.sweep_jvp(F24, Zref, K, Zout, zd, kd, xd, th), ref)  # and G is read


def test_entry_points_reject_bad_arguments_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    z, o = np.zeros(100), np.zeros(100)
    k, kd = np.zeros(60), np.zeros(60)
    x, m = np.zeros(15), np.ones(4)
    p = lambda a: a.ctypes.data  # noqa: E731
    for fn in (L.qln_tracking_rollout_model_jvp, L.qln_tracking_rollout_model_jvp_host):
        # all four tangents NULL; K_dot without K; a NULL Zout_dot; a NULL handle
        assert fn(None, p(z), p(k), p(z), p(m), None, None, None, None, p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert fn(None, p(z), None, p(z), p(m), None, p(kd), None, p(m), p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert fn(None, p(z), p(k), p(z), p(m), None, None, None, p(m), None) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert fn(None, p(z), p(k), p(z), p(m), p(z), p(kd), p(x), p(m), p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
    for fn in (L.qln_tracking_rollout_model_vjp, L.qln_tracking_rollout_model_vjp_host):
        assert fn(None, p(z), None, p(z), p(m), p(z), None, p(k), None, p(m)) == _lib.QLN_ERR_INVALID_ARGUMENT
    for fn in (L.qln_tracking_rollout_model, L.qln_tracking_rollout_model_host):
        assert fn(None, p(z), None, None, p(m), p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
    # the forms without a model: the same refusals, with no model arguments to give
    for fn in (L.qln_tracking_rollout_jvp, L.qln_tracking_rollout_jvp_host):
        # all three tangents NULL; K_dot without K; a NULL Zout_dot; a NULL handle
        assert fn(None, p(z), p(k), p(z), None, None, None, p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert fn(None, p(z), None, p(z), None, p(kd), None, p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert fn(None, p(z), p(k), p(z), None, None, p(x), None) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert fn(None, p(z), p(k), p(z), p(z), p(kd), p(x), p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
    for fn in (L.qln_tracking_rollout_vjp, L.qln_tracking_rollout_vjp_host):
        assert fn(None, p(z), None, p(z), p(z), None, p(k), None) == _lib.QLN_ERR_INVALID_ARGUMENT
    for fn in (L.qln_tracking_rollout, L.qln_tracking_rollout_host):
        assert fn(None, p(z), p(k), p(x), p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT


def test_ctypes_table_and_helper():
    import ctypes as C
    import os
    import re

    from quadruped_landing_amd import PlanarQuadruped, _lib
    from quadruped_landing_amd.planar_quadruped import plant_models

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qln_evaluator.h")).read()
    assert re.search(r"#define\s+QLN_MODEL_NP\s+4\b", header) and _lib.MODEL_NP == 4
    for stem, n in (("qln_tracking_rollout_model", 6), ("qln_tracking_rollout_model_jvp", 10), ("qln_tracking_rollout_model_vjp", 10)):
        for name in (stem, stem + "_host"):
            res, args = _lib.SIGNATURES[name]
            assert res is C.c_int and len(args) == n
            assert getattr(_lib.lib(), name).argtypes == args
            proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
            assert proto, name
            params = [q.strip() for q in proto.group(1).split(",")]
            assert len(params) == n and params[0].startswith("qln_handle*")
    second = PlanarQuadruped(g=-9.1, mb=8.7, mf=0.13, lb=0.46)
    assert np.array_equal(plant_models(second, 3), np.tile(TC.SECOND, (3, 1)))
    assert np.array_equal(plant_models([second, PlanarQuadruped()], 2), np.array([TC.SECOND, [-9.81, 10.0, 0.1, 0.5]]))
    with pytest.raises(ValueError):
        plant_models([second], 2)
