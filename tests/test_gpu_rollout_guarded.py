"""qln_tracking_rollout_guarded on the GPU: the closed-loop roll-out in which touchdown happens when the free foot reaches
the ground (include/qln_evaluator.h).  The kernel is held without trusting the yardstick by the bitwise prefix (the
knot-scheduled roll-out of a handle that never switches), the exact zeros after the touchdown, the tau = 0 case and the
open-loop continuity; the yardstick (tests/rollout_guarded_ref.py) holds the semantics to the header.  The cases and their
seeds are tests/rollout_guarded_cases.py's, checked on the CPU by tests/test_rollout_guarded_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_ref as GR
from tests import rollout_ref as RR
from tests import tracking_cases as TC

pytestmark = pytest.mark.gpu

ROLLOUT_BAR = 1e-12  # tests/test_gpu_model.py's bar for a roll-out against numpy, and its derivation
ALL = [(N, im, B, wg, wm) for (N, im, B) in GC.SHAPES for wg in (False, True) for wm in (False, True)]
JUMP = GR.JUMP


def _dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _run(N, im, B, wg, wm):
    """One case on the GPU and in numpy, shared by the tests of the case: nothing here is changed afterwards."""
    batch, Zref, K, x0, th = GC.case(N, im, B, wg, wm)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    dZ, dK, dx, dm = nlp.upload_Z(Zref), _dev(K), _dev(x0), _dev(th) if wm else None
    Zout, ev = nlp.tracking_rollout_guarded(dZ, dK, dx, dm)
    # the knot-scheduled roll-out of a handle that never switches mode
    never = TC.nlp(GC.with_k_trans(batch, N + 1), TC.SECOND_MODEL)
    plain = never.tracking_rollout_model(never.upload_Z(Zref), dK, dx, dm)
    ref = GR.rollout(N, im, Zref, K, x0, th)
    return TC.rows(nlp, Zout), ev.cpu().numpy(), TC.rows(never, plain), ref, (Zref, K, x0, th)


def _compare(got_Z, got_ev, ref, what):
    """Test 1's comparison of one batch against the yardstick; every figure is printed before it is asserted."""
    Zr, er, mg, _ = ref
    B, N = got_Z.shape[0], (got_Z.shape[1] + 5) // 20
    keep = mg >= GC.MARGIN
    assert (~keep).sum() <= GC.LEFT_OUT * B, f"{(~keep).sum()} of {B} problems near a boundary of the guard"
    assert (er[keep, 0] >= 0).any() and (er[keep, 0] < 0).any(), "the batch needs a touchdown and a problem without one"
    wz = wt = we = wf = 0.0
    for b in np.flatnonzero(keep):
        wz = max(wz, RR.rel(got_Z[b], Zr[b]))
        assert got_ev[b, 0] == er[b, 0], (what, b, got_ev[b, 0], er[b, 0])
        assert got_ev[b, 7] == 0.0
        fmax = np.abs(np.append(Zr[b], np.zeros(5)).reshape(N, 20)[: N - 1, 15:19]).max()  # the largest applied force
        wf = max(wf, abs(got_ev[b, 6] - er[b, 6]) / fmax)
        k = int(er[b, 0])
        if k < 0:
            assert not got_ev[b, 1:6].any()
            continue
        nx = np.linalg.norm(Zr[b, 20 * k: 20 * k + 15])
        wt = max(wt, np.abs(got_ev[b, 1:3] - er[b, 1:3]).max() * abs(er[b, 5]) / nx)
        we = max(we, np.abs(got_ev[b, 3:6] - er[b, 3:6]).max() / nx)
    print(f"{what}: Zout {wz:.2e}, tau and clock {wt:.2e} (x |v_y| / |x_k|), foot x and velocity {we:.2e}, "
          f"smallest force {wf:.2e}; smallest margin {mg.min():.1e}, left out {(~keep).sum()}")
    assert wz <= ROLLOUT_BAR and wt <= ROLLOUT_BAR and we <= ROLLOUT_BAR and wf <= ROLLOUT_BAR, (wz, wt, we, wf)


# ---- 1. against the yardstick -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,im,B,wg,wm", ALL)
def test_against_the_numpy_yardstick(N, im, B, wg, wm):
    """Zout per problem within ROLLOUT_BAR (tests/test_gpu_model.py: 65 steps x a growth below ten x 1e-15; the composite
    step is one step more, 66 x 10 x 1e-15 = 6.6e-13), the knot exactly, tau and the clock within the state's bar carried
    through the root to first order (d tau = d y / |v_y|), the foot's x and velocity and the smallest force within the bar
    relative to |x_k| and to the largest applied force."""
    got_Z, got_ev, _, ref, _ = _run(N, im, B, wg, wm)
    _compare(got_Z, got_ev, ref, f"N={N} mode={im} B={B} K={wg} models={wm}")


# ---- 2. bitwise prefix, 3. exact zeros ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,im,B,wg,wm", ALL)
def test_prefix_is_bitwise_the_rollout_of_a_handle_that_never_switches(N, im, B, wg, wm):
    got_Z, got_ev, plain, _, _ = _run(N, im, B, wg, wm)
    knots = got_ev[:, 0].astype(int)
    assert (knots >= 0).any() and (knots < 0).any()
    for b in range(B):
        upto = 20 * N - 5 if knots[b] < 0 else 20 * knots[b] + 20  # x_k and u_k of the touchdown knot included
        assert np.array_equal(got_Z[b, :upto], plain[b, :upto]), b
        if knots[b] >= 0:
            assert not np.array_equal(got_Z[b, upto: upto + 15], plain[b, upto: upto + 15]), b


@pytest.mark.parametrize("N,im,B,wg,wm", ALL)
def test_feet_are_exactly_on_the_ground_and_at_rest_after_the_touchdown(N, im, B, wg, wm):
    got_Z, got_ev, _, _, _ = _run(N, im, B, wg, wm)
    knots = got_ev[:, 0].astype(int)
    X = np.concatenate([got_Z, np.zeros((B, 5))], axis=1).reshape(B, N, 20)[:, :, :15]
    seen = 0
    for b in np.flatnonzero(knots >= 0):
        after = X[b, knots[b] + 1:, :][:, JUMP]
        assert after.size and not after.any(), b  # 0.0 == -0.0: any() is False for either
        assert not np.signbit(after).any(), b
        seen += 1
    assert seen


# ---- 4. tau = 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("im", [1, 2])
def test_a_foot_that_starts_on_or_below_the_ground_lands_at_tau_zero(im):
    N = 5
    batch, Zref, x0, th = GC.tau_zero_case(N, im)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Zout, ev = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), None, _dev(x0))
    xj = x0.copy()
    xj[:, JUMP] = 0.0
    stance = TC.nlp(GC.with_k_trans(batch, 1), TC.SECOND_MODEL)  # mode 3 from the first knot on
    ref = TC.rows(stance, stance.tracking_rollout(stance.upload_Z(Zref), None, _dev(xj)))
    got, e = TC.rows(nlp, Zout), ev.cpu().numpy()
    assert np.array_equal(got[:, :15], x0) and np.array_equal(got[:, 15:], ref[:, 15:])
    iy, iv = GC.free_foot(im)
    want = np.zeros((3, 8))
    want[:, 2], want[:, 3], want[:, 4], want[:, 5] = x0[:, 14], x0[:, iy - 1], x0[:, iv - 1], x0[:, iv]
    # knot 0 starts in single stance: only the standing foot's force counts there, both feet's from knot 1 on
    stand0 = got[:, 16 if im == 1 else 18]
    later = np.min(got[:, np.add.outer(20 * np.arange(1, N - 1), [16, 18]).reshape(-1)], axis=1)
    want[:, 6] = np.minimum(stand0, later)
    assert np.array_equal(e, want), (e, want)


# ---- 5. continuity, open loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,kt", GC.CONTINUITY)
def test_open_loop_the_map_is_continuous_across_a_change_of_the_touchdown_knot(N, kt):
    """2 001 drops whose free foot starts between 0.02 and 0.12 m: where the touchdown knot changes, x_N moves no more than
    twice what it moves between other neighbours (the yardstick: 0.99 and 0.62).  A roll-out that dropped the rest of the
    touchdown step, or applied the jump at the knot, would jump by about h v there, two orders more."""
    batch, Zref, x0, _ = GC.continuity_case(N, kt)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    Zout, ev = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), None, _dev(x0))
    got = TC.rows(nlp, Zout)
    changes, ratio = GC.continuity_ratio(ev.cpu().numpy()[:, 0], got[:, -15:])
    print(f"N={N}: {changes} changes of the knot, neighbour difference at a change / elsewhere = {ratio:.2f}")
    assert changes >= 2 and ratio <= 2.0


# ---- 6. model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,im,B", [(8, 1, 48), (40, 2, 9)])
def test_models_are_bitwise_the_handles_created_with_them(N, im, B):
    import torch

    from quadruped_landing_amd import PlanarQuadruped

    batch, Zref, K, x0, _ = GC.case(N, im, B, True, False)
    other = PlanarQuadruped(g=-9.6, mb=9.3, mf=0.117, lb=0.43)
    nlp, nlp_a, nlp_b = TC.nlp(batch, PlanarQuadruped()), TC.nlp(batch, TC.SECOND_MODEL), TC.nlp(batch, other)
    dZ, dK, dx = nlp.upload_Z(Zref), _dev(K), _dev(x0)
    model = nlp.plant_models([TC.SECOND_MODEL if b % 2 == 0 else other for b in range(B)])
    got, gev = nlp.tracking_rollout_guarded(dZ, dK, dx, model)
    (za, ea), (zb, eb) = nlp_a.tracking_rollout_guarded(dZ, dK, dx), nlp_b.tracking_rollout_guarded(dZ, dK, dx)
    got, za, zb = got.view(B, -1), za.view(B, -1), zb.view(B, -1)
    assert torch.equal(got[0::2], za[0::2]) and torch.equal(got[1::2], zb[1::2])
    assert torch.equal(gev[0::2], ea[0::2]) and torch.equal(gev[1::2], eb[1::2])
    assert not torch.equal(za, zb)
    # model = NULL and the handle's own four values are the same call
    z2, e2 = nlp_a.tracking_rollout_guarded(dZ, dK, dx, nlp_a.plant_models())
    assert torch.equal(z2.view(B, -1), za) and torch.equal(e2, ea)


# ---- 7. forms and arguments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"z_stride": 20 * 12 + 3, "align": 7}])
def test_ragged_batch_padded_layout_host_form_and_null_event(kw):
    """70 problems (two blocks of lanes) with per-problem init_mode, k_trans and step lengths: against the yardstick, the
    host form and the form without an event record bit for bit, and a sentinel past n_nlp that survives."""
    import torch

    batch, Zref, K, x0, th = GC.ragged_case()
    B, N = batch.B, batch.N
    nlp = TC.nlp(batch, TC.SECOND_MODEL, **kw)
    n, zs = nlp.n_nlp, nlp.z_stride
    dZ, dK, dx, dm = nlp.upload_Z(Zref), _dev(K), _dev(x0), _dev(th)
    sentinel = torch.full((B * zs,), -7.25, dtype=torch.float64, device="cuda")
    Zout, ev = nlp.tracking_rollout_guarded(dZ, dK, dx, dm, out=sentinel)
    assert Zout is sentinel and bool((Zout.view(B, zs)[:, n:] == -7.25).all())
    _compare(TC.rows(nlp, Zout), ev.cpu().numpy(), GR.rollout(N, batch.init_mode, Zref, K, x0, th), f"ragged {kw}")
    z2, e2 = nlp.tracking_rollout_guarded(dZ, dK, dx, dm, with_events=False)
    assert e2 is None and torch.equal(z2.view(B, zs)[:, :n], Zout.view(B, zs)[:, :n])
    Zh = np.zeros((B, zs))
    Zh[:, :n] = Zref
    zh, eh = nlp.tracking_rollout_guarded_host(Zh.reshape(-1), K, x0, th)
    assert np.array_equal(zh.reshape(B, zs)[:, :n], TC.rows(nlp, Zout)) and np.array_equal(eh, ev.cpu().numpy())
    assert not zh.reshape(B, zs)[:, n:].any()
    zh2, eh2 = nlp.tracking_rollout_guarded_host(Zh.reshape(-1), K, x0, th, with_events=False)
    assert eh2 is None and np.array_equal(zh2, zh)


def test_invalid_arguments_are_refused():
    import torch

    from quadruped_landing_amd import _lib

    batch, Zref, K, x0, th = GC.case(5, 2, 32, True, True)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    L, h, INV = _lib.lib(), nlp._h, _lib.QLN_ERR_INVALID_ARGUMENT
    dZ, out = nlp.upload_Z(Zref), nlp.new_Z()
    ev = torch.zeros((nlp.B, 8), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.qln_tracking_rollout_guarded(None, p(dZ), None, None, None, p(out), p(ev)) == INV
    assert L.qln_tracking_rollout_guarded(h, None, None, None, None, p(out), p(ev)) == INV
    assert L.qln_tracking_rollout_guarded(h, p(dZ), None, None, None, None, p(ev)) == INV
    assert L.qln_tracking_rollout_guarded(h, p(dZ), None, None, None, p(dZ), p(ev)) == INV  # Zout overlaps Zref
    assert b"overlaps" in L.qln_last_error()
    assert L.qln_tracking_rollout_guarded(h, p(dZ), None, None, None, p(out), p(dZ)) == INV  # event overlaps Zref
    assert L.qln_tracking_rollout_guarded(h, p(dZ), None, None, None, p(out), p(ev)) == _lib.QLN_OK
    # host form: the same, and the model's values
    Zh, oh, eh = np.ascontiguousarray(TC.rows(nlp, dZ)).reshape(-1), np.zeros(nlp.dims.z_total), np.zeros((nlp.B, 8))
    a = lambda v: v.ctypes.data  # noqa: E731
    host = L.qln_tracking_rollout_guarded_host
    assert host(None, a(Zh), None, None, None, a(oh), a(eh)) == INV
    assert host(h, None, None, None, None, a(oh), a(eh)) == INV
    assert host(h, a(Zh), None, None, None, None, a(eh)) == INV
    assert host(h, a(Zh), None, None, None, a(Zh), a(eh)) == INV
    for entry, value in ((0, np.nan), (1, 0.0), (2, -0.1), (3, np.inf)):
        bad = np.array(th)
        bad[nlp.B - 1, entry] = value
        before = oh.copy()
        assert host(h, a(Zh), None, None, a(bad), a(oh), a(eh)) == INV, (entry, value)
        assert np.array_equal(oh, before)
    assert host(h, a(Zh), None, None, a(np.ascontiguousarray(th)), a(oh), a(eh)) == _lib.QLN_OK
