"""The numpy yardstick of the contact-aware force limits (tests/rollout_limited_ref.py), held on the CPU: to itself in
longdouble (same saturation codes, same touchdown knots), to the existing yardsticks exactly with infinite limits, its
masked-block sweeps to each other (adjoint) and to longdouble central differences of the limited roll-out; and the entry
points' argument checks, which need no GPU.  The cases are tests/rollout_guarded_cases.py's with gains and per-problem models,
the ones the GPU runs (tests/test_gpu_rollout_limited.py), under the limits LR.TEST_LIMITS."""
import functools

import numpy as np
import pytest

from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_ref as GR
from tests import rollout_guarded_sweep_ref as SR
from tests import rollout_limited_ref as LR
from tests import rollout_ref as RR

FD_STEP = 1e-7
DIRECTION_SCALE = 1e-2  # tests/test_rollout_guarded_sweeps_host.py
FD_BAR = 1e-9           # that file's: longdouble rounding over the step, 1e-19 x |Zout| / 1e-7
ADJOINT_BAR = 1e-12


@functools.lru_cache(maxsize=None)
def _case(N, im, B):
    """One case: the limited roll-out, its blocks, one direction and the differences along it.  Shared by the tests of the
    case; nothing here is changed afterwards."""
    _, Zref, K, x0, th = GC.case(N, im, B, True, True)
    Zout, ev, sat, mg, fm = LR.rollout(N, im, Zref, K, x0, th, LR.TEST_LIMITS)
    F, T = SR.blocks(N, im, Zout, th, ev)
    dirs = SR.directions(GC.seed_of(N, im, True, True) + 31, B, N, True, DIRECTION_SCALE)
    return (Zref, K, x0, th), (Zout, ev, sat, mg, fm), (F, T), dirs


@pytest.mark.parametrize("N,im,B", GC.SHAPES)
def test_float64_and_longdouble_take_the_same_decisions(N, im, B):
    (Zref, K, x0, th), (Zout, ev, sat, mg, fm), _, _ = _case(N, im, B)
    Zl, evl, satl, _, _ = LR.rollout(N, im, Zref, K, x0, th, LR.TEST_LIMITS, dtype=np.longdouble)
    keep = (mg >= GC.MARGIN) & (fm >= GC.MARGIN)
    assert (~keep).sum() <= GC.LEFT_OUT * B
    assert np.array_equal(sat[keep], satl[keep]) and np.array_equal(ev[keep, 0], evl[keep, 0].astype(np.float64))
    w = SR.worst(Zout[keep], Zl[keep].astype(np.float64))
    print(f"N={N} mode={im} B={B}: float64 to longdouble {w:.2e}; guard margin {mg.min():.2e}, force margin {fm.min():.2e}")
    assert w <= 1e-12
    # the limits bite: both sides of some channel, free knots too, and every applied force is inside its limits
    s = LR.unpack(sat)
    assert (s == 1).any() and (s == 2).any() and (sat == 0).any()
    assert ev[:, 6].min() >= LR.TEST_LIMITS[6]


@pytest.mark.parametrize("N,im,B", GC.SHAPES)
@pytest.mark.parametrize("wg", [False, True])
def test_infinite_limits_are_the_existing_yardsticks_exactly(N, im, B, wg):
    batch, Zref, K, x0, th = GC.case(N, im, B, wg, True)
    Zout, ev, sat, mg, fm = LR.rollout(N, im, Zref, K, x0, th, LR.NO_LIMITS)
    Zg, evg, mgg, _ = GR.rollout(N, im, Zref, K, x0, th)
    assert np.array_equal(Zout, Zg) and np.array_equal(ev, evg) and np.array_equal(mg, mgg) and not sat.any()
    kt = int(batch.k_trans[0])
    Zs, sats, _ = LR.rollout_scheduled(N, kt, im, Zref, K, x0, th, LR.NO_LIMITS)
    assert np.array_equal(Zs, RR.rollout(N, kt, im, Zref, K, x0, th)) and not sats.any()


@pytest.mark.parametrize("N,im,B", GC.SHAPES)
def test_masked_block_sweeps_are_adjoint(N, im, B):
    (Zref, K, _, _), (Zout, ev, sat, _, _), (F, T), dirs = _case(N, im, B)
    zd, _ = LR.sweep_jvp(F, T, ev, sat, Zref, K, Zout, *dirs)
    Zbar = np.random.default_rng(5).normal(size=Zout.shape)
    zb, kb, xb, mb = LR.sweep_vjp(F, sat, Zref, K, Zout, Zbar)
    lhs = np.sum(Zbar * zd, axis=1)
    rhs = (np.sum(zb * dirs[0], axis=1) + np.sum(xb * dirs[2], axis=1) + np.sum(mb * dirs[3], axis=1) +
           np.sum(kb * dirs[1], axis=(1, 2, 3)))
    w = float(np.max(np.abs(lhs - rhs) / np.maximum(1.0, np.abs(lhs))))
    print(f"N={N} mode={im} B={B}: adjoint identity {w:.2e}")
    assert w <= ADJOINT_BAR
    # a saturated channel's F_ref_bar and row of K_bar are exact zeros, its tangent too
    held = ~LR.free_channels(sat)
    assert held.any() and not kb[held].any()
    n1 = N - 1
    assert not zb[:, : 20 * n1].reshape(B, n1, 20)[:, :, 15:19][held].any()
    assert not zd[:, : 20 * n1].reshape(B, n1, 20)[:, :, 15:19][held].any()


@pytest.mark.parametrize("N,im,B", GC.SHAPES)
def test_forward_sweep_matches_longdouble_central_differences_of_the_limited_rollout(N, im, B):
    (Zref, K, x0, th), (Zout, ev, sat, _, _), (F, T), dirs = _case(N, im, B)
    fd, fd_ev, same = LR.central_difference(N, im, Zref, K, x0, th, LR.TEST_LIMITS, dirs, FD_STEP)
    assert (~same).sum() <= GC.LEFT_OUT * B, f"{(~same).sum()} of {B} problems change a decision over the step"
    zd, ed = LR.sweep_jvp(F, T, ev, sat, Zref, K, Zout, *dirs)
    wz, we = SR.worst(zd[same], fd[same]), SR.worst(ed[same, 1:3], fd_ev[same, 1:3])
    print(f"N={N} mode={im} B={B}: Zout_dot {wz:.2e}, event_dot {we:.2e} of max(1, |ref|); left out {(~same).sum()}")
    assert wz <= FD_BAR and we <= FD_BAR
    # the comparison discriminates: the unmasked sweep misses the same differences
    zu, _ = SR.sweep_jvp(F, T, ev, Zref, K, Zout, *dirs)
    assert SR.worst(zu[same], fd[same]) > 1e3 * FD_BAR


def test_scheduled_rollout_clamps_by_the_knot_schedule():
    """Knot-scheduled: the free foot's limits up to and including the jump knot, the standing pair from the next knot on."""
    batch, Zref, K, x0, th = GC.case(8, 1, 48, True, True)
    kt = int(batch.k_trans[0])
    Zs, sat, fm = LR.rollout_scheduled(8, kt, 1, Zref, K, x0, th, LR.TEST_LIMITS)
    u = np.concatenate([Zs, np.zeros((48, 5))], axis=1).reshape(48, 8, 20)[:, :7, 15:19]
    lim = LR.TEST_LIMITS
    for k in range(7):
        free2 = k + 1 <= kt - 1  # foot 2 is free while the knot is at or before the jump knot
        lo, hi = (lim[2], lim[3]) if free2 else (lim[6], lim[7])
        assert (u[:, k, 3] >= lo).all() and (u[:, k, 3] <= hi).all()
        assert (u[:, k, 1] >= lim[6]).all() and (u[:, k, 1] <= lim[7]).all()
    assert sat.any() and (sat == 0).any()


def test_entry_points_reject_bad_arguments_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    INV = _lib.QLN_ERR_INVALID_ARGUMENT
    z, o, k, s, e, m = np.zeros(100), np.zeros(100), np.zeros(60), np.zeros(4), np.zeros(8), np.ones(4)
    p = lambda a: a.ctypes.data  # noqa: E731
    lim = np.array(LR.TEST_LIMITS)
    err = lambda: L.qln_last_error().decode()  # noqa: E731
    for fn in (L.qln_tracking_rollout_limited, L.qln_tracking_rollout_limited_host):
        bad = lim.copy()
        bad[3] = np.nan
        assert fn(None, p(z), None, None, None, p(bad), 1, p(o), None, p(s)) == INV and "NaN" in err()
        bad = lim.copy()
        bad[4], bad[5] = 0.5, 0.4
        assert fn(None, p(z), None, None, None, p(bad), 1, p(o), None, p(s)) == INV and "lo > hi" in err()
        assert fn(None, p(z), None, None, None, None, 1, p(o), None, p(s)) == INV and "null lim" in err()
        assert fn(None, p(z), None, None, None, p(lim), 0, p(o), p(e), p(s)) == INV and "guarded == 0" in err()
        assert fn(None, p(z), None, None, None, p(lim), 1, p(o), p(e), p(s)) == INV and "null handle" in err()
    for fn in (L.qln_tracking_rollout_limited_jvp, L.qln_tracking_rollout_limited_jvp_host):
        assert fn(None, p(z), None, p(z), None, p(e), None, None, None, p(m), None, p(o), None) == INV and "null sat" in err()
        assert fn(None, p(z), None, p(z), None, None, p(s), None, None, p(m), None, p(o), p(e)) == INV and "event_dot" in err()
    for fn in (L.qln_tracking_rollout_limited_vjp, L.qln_tracking_rollout_limited_vjp_host):
        assert fn(None, p(z), None, p(z), None, p(e), None, p(z), None, None, p(m), None) == INV and "null sat" in err()
    for fn in (L.qln_tracking_lqr_limited, L.qln_tracking_lqr_limited_host):
        q, r = np.ones(15), np.ones(4)
        assert fn(None, p(z), None, p(e), None, p(q), p(r), p(q), p(k), None) == INV and "null sat" in err()
        assert fn(None, p(z), p(m), None, p(s), p(q), p(r), p(q), p(k), None) == INV and "model without event" in err()


def test_python_helpers():
    from quadruped_landing_amd import nlp as NL

    sat = np.array([[0.0, 1 + 2 * 4 + 0 * 16 + 1 * 64, 170.0]])
    s = NL.unpack_saturation(sat)
    assert s.dtype == np.int8 and s.shape == (1, 3, 4)
    assert s.tolist() == [[[0, 0, 0, 0], [1, 2, 0, 1], [2, 2, 2, 2]]] and np.array_equal(s, LR.unpack(sat))
    K = np.ones((1, 3, 4, 15))
    Km = NL.mask_gains(K, sat)
    assert np.array_equal(Km, LR.mask_gains(K, sat)) and Km[0, 0].all() and not Km[0, 2].any()
    assert not Km[0, 1, [0, 1, 3]].any() and Km[0, 1, 2].all()
    assert np.array_equal(NL.force_limits(LR.TEST_LIMITS), LR.TEST_LIMITS)
    for bad in ([0.0] * 7, [np.nan] + [0.0] * 7, [1.0, 0.0] + [0.0] * 6):
        with pytest.raises(ValueError):
            NL.force_limits(bad)
