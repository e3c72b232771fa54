"""The numpy yardstick of the sweeps through the guard-triggered touchdown (tests/rollout_guarded_sweep_ref.py), held on the
CPU: its composite step to the guarded roll-out's yardstick exactly, its forward sweep to longdouble central differences of
that roll-out, its reverse sweep to the forward one, and -- so that the comparison is known to discriminate -- the blocks
with tau frozen shown to MISS the same differences.  The cases are tests/rollout_guarded_cases.py's, the ones the GPU runs
(tests/test_gpu_rollout_guarded_sweeps.py)."""
import functools

import numpy as np
import pytest

from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_ref as GR
from tests import rollout_guarded_sweep_ref as SR

ALL = [(N, im, B, wg) for (N, im, B) in GC.SHAPES for wg in (False, True)]
FD_STEP = 1e-7
# The directions are normal draws of the size of the cases' own perturbations (x0 lies 1e-2 from the reference): the maps are
# linear in them, and with tangents of order ten an inner product of a few hundred terms is held to max(1, |lhs|) and not to an
# lhs that cancelled to nothing (with unit draws one problem's lhs is 0.43 out of terms summing to 6.5e3).
DIRECTION_SCALE = 1e-2
FD_BAR = 1e-9        # measured worst 1.4e-10 of max(1, |ref|): longdouble rounding over the step, 1e-19 x |Zout| / 1e-7
ADJOINT_BAR = 1e-12  # measured worst 2.3e-14 of max(1, |lhs|)
FROZEN_MISS = 1e-2   # what blocks without the tau term miss the differences by, at least, at N = 40 and 61


@functools.lru_cache(maxsize=None)
def _case(N, im, B, wg):
    """One case, with per-problem models: the roll-out, its blocks, one direction and the differences along it.  Shared by
    the tests of the case; nothing here is changed afterwards."""
    _, Zref, K, x0, th = GC.case(N, im, B, wg, True)
    Zout, ev, mg, pre = GR.rollout(N, im, Zref, K, x0, th)
    F, T = SR.blocks(N, im, Zout, th, ev)
    dirs = SR.directions(GC.seed_of(N, im, wg, True) + 31, B, N, wg, DIRECTION_SCALE)
    fd, fd_ev, same = SR.central_difference(N, im, Zref, K, x0, th, dirs, FD_STEP)
    return (Zref, K, x0, th), (Zout, ev, pre), (F, T), dirs, (fd, fd_ev, same)


@pytest.mark.parametrize("N,im,B,wg", ALL)
def test_composite_step_reproduces_the_guarded_yardsticks_touchdown_step_exactly(N, im, B, wg):
    (_, _, _, th), (Zout, ev, _), _, _, _ = _case(N, im, B, wg)
    seen = 0
    for b in np.flatnonzero(ev[:, 0] >= 0):
        k = int(ev[b, 0])
        xn, tau = SR.composite_step(im, Zout[b, 20 * k: 20 * k + 15], Zout[b, 20 * k + 15: 20 * k + 20], th[b])
        assert tau == ev[b, 1] and np.array_equal(xn, Zout[b, 20 * k + 20: 20 * k + 35]), b
        seen += 1
    assert seen and (ev[:, 0] < 0).any()


@pytest.mark.parametrize("N,im,B,wg", ALL)
def test_forward_sweep_matches_longdouble_central_differences_of_the_guarded_rollout(N, im, B, wg):
    (Zref, K, _, _), (Zout, ev, _), (F, T), dirs, (fd, fd_ev, same) = _case(N, im, B, wg)
    assert (~same).sum() <= GC.LEFT_OUT * B, f"{(~same).sum()} of {B} problems change their touchdown knot over the step"
    zd, ed = SR.sweep_jvp(F, T, ev, Zref, K, Zout, *dirs)
    wz, we = SR.worst(zd[same], fd[same]), SR.worst(ed[same, 1:3], fd_ev[same, 1:3])
    print(f"N={N} mode={im} B={B} K={wg}: Zout_dot {wz:.2e}, event_dot {we:.2e} of max(1, |ref|); left out {(~same).sum()}")
    assert wz <= FD_BAR and we <= FD_BAR
    land = same & (ev[:, 0] >= 0)
    assert land.any() and np.abs(ed[land, 1]).min() > 0 and not ed[ev[:, 0] < 0].any()
    assert not ed[:, [0, 3, 4, 5, 6, 7]].any()


@pytest.mark.parametrize("N,im,B,wg", ALL)
def test_reverse_sweep_is_the_adjoint_of_the_forward_sweep(N, im, B, wg):
    (Zref, K, _, _), (Zout, ev, _), (F, T), dirs, _ = _case(N, im, B, wg)
    zd, _ = SR.sweep_jvp(F, T, ev, Zref, K, Zout, *dirs)
    Zbar = np.random.default_rng(5).normal(size=Zout.shape)
    zb, kb, xb, mb = SR.sweep_vjp(F, Zref, K, Zout, Zbar)
    lhs = np.sum(Zbar * zd, axis=1)
    rhs = np.sum(zb * dirs[0], axis=1) + np.sum(xb * dirs[2], axis=1) + np.sum(mb * dirs[3], axis=1)
    if wg:
        rhs = rhs + np.sum(kb * dirs[1], axis=(1, 2, 3))
    w = float(np.max(np.abs(lhs - rhs) / np.maximum(1.0, np.abs(lhs))))
    print(f"N={N} mode={im} B={B} K={wg}: adjoint identity {w:.2e}")
    assert w <= ADJOINT_BAR


@pytest.mark.parametrize("N,im,B,wg", [c for c in ALL if c[0] >= 40])
def test_blocks_with_tau_frozen_miss_the_same_differences(N, im, B, wg):
    """The comparison discriminates: a sweep that forgets the saltation term is off by more than FROZEN_MISS."""
    (Zref, K, _, th), (Zout, ev, _), _, dirs, (fd, _, same) = _case(N, im, B, wg)
    Ff, Tf = SR.blocks(N, im, Zout, th, ev, freeze_tau=True)
    zd, _ = SR.sweep_jvp(Ff, Tf, ev, Zref, K, Zout, *dirs)
    w = SR.worst(zd[same], fd[same])
    print(f"N={N} mode={im} B={B} K={wg}: tau frozen misses by {w:.2e}")
    assert w > FROZEN_MISS


@pytest.mark.parametrize("im", [1, 2])
def test_a_touchdown_at_tau_zero_has_no_tau_term(im):
    """GC.tau_zero_case: the guard's first branch, d tau = 0, and the sweep agrees with longdouble differences of the
    roll-out whose touchdown step is the composite step at the frozen tau = 0 (at y = +-0 the guarded roll-out itself has no
    two-sided difference: one side leaves the branch)."""
    N = 5
    _, Zref, x0, th = GC.tau_zero_case(N, im)
    Zout, ev, _, _ = GR.rollout(N, im, Zref, None, x0, th)
    assert np.array_equal(ev[:, 0], np.zeros(3)) and not ev[:, 1].any()
    F, T = SR.blocks(N, im, Zout, th, ev)
    assert not T.any()
    Ff, _ = SR.blocks(N, im, Zout, th, ev, freeze_tau=True)
    assert np.array_equal(F, Ff)
    zd_, _, xd, md = SR.directions(17 + im, 3, N, False, DIRECTION_SCALE)
    zd, ed = SR.sweep_jvp(F, T, ev, Zref, None, Zout, zd_, None, xd, md)
    assert not ed[:, 1].any() and np.array_equal(ed[:, 2], xd[:, 14])
    # differences at the frozen tau = 0: the roll-out with the touchdown step taken as the composite step at tau = 0
    L, t = np.longdouble, FD_STEP

    def frozen(s, L=L):
        zr, x, m = Zref.astype(L) + L(s) * zd_, x0.astype(L) + L(s) * xd, th.astype(L) + L(s) * md
        out = np.zeros((3, 20 * N - 5), dtype=L)
        out[:, :15] = x
        for k in range(N - 1):
            u = zr[:, 20 * k + 15: 20 * k + 20]
            out[:, 20 * k + 15: 20 * k + 20] = u
            x = SR.composite_step(im, x, u, m, tau=L(0))[0] if k == 0 else SR.RR.model_step(3, False, x, u, m)
            out[:, 20 * (k + 1): 20 * (k + 1) + 15] = x
        return out

    assert np.array_equal(frozen(0, np.float64), Zout)
    fd = ((frozen(t) - frozen(-t)) / (2 * L(t))).astype(np.float64)
    w = SR.worst(zd, fd)
    print(f"tau = 0, mode {im}: {w:.2e}")
    assert w <= FD_BAR
