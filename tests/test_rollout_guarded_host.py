"""The numpy yardstick of the guarded roll-out (tests/rollout_guarded_ref.py), held on the CPU to what needs no second
implementation: the event is located where the foot is on the ground, the decision does not depend on the precision, the
steps before the touchdown are the knot-scheduled roll-out's, and open loop the map is continuous across a change of the
touchdown knot.  The seeds of tests/rollout_guarded_cases.py are the ones the GPU tests run: this module also checks that
none of their problems lies near a boundary of the guard."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_ref as GR
from tests import rollout_ref as RR

EPS = np.finfo(np.float64).eps
ALL = [(N, im, B, wg, wm) for (N, im, B) in GC.SHAPES for wg in (False, True) for wm in (False, True)]


@functools.lru_cache(maxsize=None)
def _run(N, im, B, wg, wm):
    _, Zref, K, x0, th = GC.case(N, im, B, wg, wm)
    return Zref, K, x0, th, GR.rollout(N, im, Zref, K, x0, th)


@pytest.mark.parametrize("N,im,B,wg,wm", ALL)
def test_the_foot_is_on_the_ground_before_the_jump_map(N, im, B, wg, wm):
    """The height over the step is y + v t + a t^2 / 2 exactly and RK4 integrates it exactly, so what is left at t = tau is
    rounding: tau carries a few ulp (a square root, a division, a sum), which moves the height by |v| tau times that, and
    the RK4 sum adds about eight roundings of terms no larger than |y| + |v| tau + |a| tau^2 / 2.  Sixteen ulp of that sum
    bound both."""
    Zref, K, x0, th, (Zo, ev, mg, pre) = _run(N, im, B, wg, wm)
    iy, iv = GC.free_foot(im)
    iF = 3 if im == 1 else 1
    worst, n = 0.0, 0
    for b in np.flatnonzero(ev[:, 0] >= 0):
        k, tau = int(ev[b, 0]), ev[b, 1]
        xk, uk = Zo[b, 20 * k: 20 * k + 15], Zo[b, 20 * k + 15: 20 * k + 20]
        a = -uk[iF] / th[b, 2] + th[b, 0]
        scale = abs(xk[iy]) + abs(xk[iv]) * tau + abs(a) * tau * tau / 2
        if scale > 0:
            worst = max(worst, abs(pre[b, iy]) / (EPS * scale))
        assert abs(pre[b, iy]) <= 16 * EPS * scale
        assert 0 <= tau <= uk[4]
        n += 1
    print(f"N={N} mode={im} K={wg} models={wm}: {n} touchdowns, pre-jump height <= {worst:.2f} ulp of the step's terms")
    assert 0 < n < B


@pytest.mark.parametrize("N,im,B,wg,wm", ALL)
def test_float64_and_longdouble_take_the_same_knots_and_no_problem_is_near_a_boundary(N, im, B, wg, wm):
    Zref, K, x0, th, (Zo, ev, mg, _) = _run(N, im, B, wg, wm)
    Zl, el, ml, _ = GR.rollout(N, im, Zref, K, x0, th, dtype=np.longdouble)
    assert np.array_equal(ev[:, 0], el[:, 0].astype(np.float64))
    assert mg.min() >= GC.MARGIN and ml.min() >= GC.MARGIN, (mg.min(), ml.min())
    worst = max(RR.rel(Zo[b], Zl[b].astype(np.float64)) for b in range(B))
    print(f"N={N} mode={im} K={wg} models={wm}: smallest margin {mg.min():.1e}, float64 against longdouble {worst:.1e}")
    assert worst <= 1e-12  # the roll-out's bar (tests/test_gpu_model.py), which the yardstick itself has to meet


@pytest.mark.parametrize("N,im,B,wg,wm", ALL)
def test_before_the_touchdown_it_is_the_knot_scheduled_rollout_without_a_transition(N, im, B, wg, wm):
    Zref, K, x0, th, (Zo, ev, _, _) = _run(N, im, B, wg, wm)
    ref = RR.rollout(N, N + 1, im, Zref, K, x0, th)
    for b in range(B):
        k = int(ev[b, 0])
        upto = 20 * N - 5 if k < 0 else 20 * k + 20  # x_k and u_k of the touchdown knot included
        assert np.array_equal(Zo[b, :upto], ref[b, :upto])
        if k >= 0:
            assert not np.array_equal(Zo[b, upto: upto + 15], ref[b, upto: upto + 15])
            for j in range(k + 1, N):  # both feet on the ground and at rest from then on
                assert not Zo[b, 20 * j: 20 * j + 15][GR.JUMP].any()
        else:
            assert not ev[b, 1:6].any()


@pytest.mark.parametrize("N,kt", GC.CONTINUITY)
def test_open_loop_the_map_is_continuous_across_a_change_of_the_touchdown_knot(N, kt):
    """A roll-out that dropped the rest of the touchdown step, or applied the jump at the knot, would jump by about h v at a
    change of the knot, two orders more than the neighbour differences elsewhere."""
    _, Zref, x0, th = GC.continuity_case(N, kt)
    Zo, ev, _, _ = GR.rollout(N, 1, Zref, None, x0, th)
    changes, ratio = GC.continuity_ratio(ev[:, 0], Zo[:, -15:])
    print(f"N={N}: {changes} changes of the knot, neighbour difference at a change / elsewhere = {ratio:.2f}")
    assert changes >= 2 and ratio <= 2.0


def test_tau_zero_starts_from_the_jump_map_of_x0():
    for im in (1, 2):
        _, Zref, x0, th = GC.tau_zero_case(5, im)
        Zo, ev, _, _ = GR.rollout(5, im, Zref, None, x0, th)
        xj = x0.copy()
        xj[:, GR.JUMP] = 0.0
        ref = RR.rollout(5, 1, im, Zref, None, xj, th)  # k_trans = 1: mode 3 from the first knot on
        assert np.array_equal(Zo[:, 15:], ref[:, 15:])
        assert np.array_equal(ev[:, 0], np.zeros(3)) and np.array_equal(ev[:, 1], np.zeros(3))
        assert np.array_equal(ev[:, 2], x0[:, 14])


def test_a_null_handle_is_refused_without_a_gpu():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    z = np.zeros(64)
    for fn in (L.qln_tracking_rollout_guarded, L.qln_tracking_rollout_guarded_host):
        assert fn(None, z.ctypes.data, None, None, None, z.ctypes.data, None) == _lib.QLN_ERR_INVALID_ARGUMENT
    assert C.sizeof(C.c_double) * _lib.TOUCHDOWN_INFO_STRIDE == 64
