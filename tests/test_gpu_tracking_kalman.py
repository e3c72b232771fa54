"""qln_tracking_kalman / qln_tracking_kalman_guarded on the GPU: Kalman filter gains and the LQG covariance along tracked
landings (include/qln_evaluator.h).  The yardstick is tests/tracking_kalman_ref.py, held on the CPU by
tests/test_tracking_kalman_host.py; it runs on the evaluator's dense blocks, and for the guarded call on the complex-step
blocks of tests/rollout_guarded_sweep_ref.py.  Besides it the kernel is held without an oracle: with H = 0 it is bit for bit
the open-loop covariance sweep, ny rows are bit for bit eight rows with zero rows written out, every subset of outputs has
the bits of the full call, and the host forms have the bits of the device forms."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import estimation_cases as EF
from tests import rollout_guarded_cases as GC
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR
from tests import tracking_kalman_ref as KR

pytestmark = pytest.mark.gpu
_time_limit = EF.time_limit(600)

BAR = 1e-10  # the family's bar (tests/test_gpu_tracking_cov.py, tests/test_gpu_tracking_guarded.py)
# A problem's inputs are well conditioned in the compared measures when the float64 yardstick is itself within BAR / 100 of its
# longdouble restatement in every one of them.  The measure that needs this is entry_rel on the applied-force variances
# diag(K M K'): M_k has rank min(15, (k + 1) ny), so with ny = 1 the first knots' variances are single squares (K_m . l)^2 S that
# come out of terms 1e6 times their size when a random gain row is nearly orthogonal to the filter gain, and no float64
# evaluation of them, the yardstick's included, is good to 1e-10 (measured: the yardstick 1.1e-10 from longdouble, the kernel
# 4.7e-10 from the yardstick, on an entry of 1.3e-8 where trace M is 0.83; L, P^+ and X of the same problem agree to 4e-15).
# Such a problem's gains are drawn again, by the yardstick alone and before the GPU is asked; the bar stays.
COND = BAR / 100
REDRAWS = 200

# EF.design_shapes() with sigma0_batch taking turns; the guarded shapes without and with gains
CASES = [c + (i % 4 < 2,) for i, c in enumerate(EF.design_shapes())] + [EF.RAGGED[0] + (True,), EF.RAGGED[1] + (False,)]
GUARDED = [s + (wg,) for s in EF.GUARDED_SHAPES for wg in (False, True)] + [EF.GUARDED_RAGGED + (True,)]


def _host(t):
    from quadruped_landing_amd import nlp as NL

    L, Pe, S, mg = t[:4]
    out = dict(L=TC.to_np(L), Pp=None if Pe is None else NL.unpack_covariance(Pe), X=None if S is None else NL.unpack_covariance(S),
               marg=TC.to_np(mg))
    if len(t) > 4:
        out["var"] = TC.to_np(t[4])
    return out


def _conditioned_gains(K, seed, yardsticks):
    """K (B, N-1, 4, 15) with the gains of every ill-conditioned problem drawn again (0.05 * normal, as tracking_cases.gains)
    until the problem is well conditioned.  yardsticks(b, K_b) -> (float64 dict, longdouble dict) with the compared arrays
    under 'L', 'Pp', 'X' (knot_rel) and 'marg', 'event_var' (entry_rel) where present.  Returns (K, the float64 dicts, the worst
    distance, how many problems were redrawn)."""
    K = np.array(K)
    refs, worst, redrawn = [], 0.0, 0
    for b in range(len(K)):
        rng = np.random.default_rng([seed, b])
        for attempt in range(REDRAWS):
            if attempt:
                K[b] = 0.05 * rng.normal(size=K[b].shape)
            lo, hi = yardsticks(b, K[b])
            d = max([CR.knot_rel(lo[n], hi[n]) for n in ("L", "Pp", "X")] +
                    [CR.entry_rel(lo[n], hi[n]) for n in ("marg", "event_var") if n in lo])
            if d <= COND:
                break
        else:
            raise AssertionError(f"problem {b}: no well-conditioned gains in {REDRAWS} draws")
        redrawn += attempt > 0
        worst = max(worst, d)
        refs.append(lo)
    return K, refs, worst, redrawn


def _design(A, Bm, K, H, V, S0, W, theta, lb):
    """The yardstick of one knot-scheduled problem in the dtype of its arrays: the recursion, and the marginals of its X and M"""
    r = KR.recursion(A, Bm, K, H, V, S0, W)
    r["marg"] = KR.marginals(r["X"], r["M"], K, theta, A.dtype.type(lb))
    return r


@functools.lru_cache(maxsize=None)
def _run(kind, B, N, k_trans, im, ny, per_problem):
    """One knot-scheduled case: the handle, the inputs, the GPU's outputs and the yardstick's on the evaluator's dense blocks
    at the same Zout, with the yardstick's own float64-to-longdouble distance.  Shared by the case's tests, never changed."""
    d = EF.scheduled_design(kind, B, N, k_trans, im, ny, 5)
    nlp, Zout, H, V, W = d.nlp, d.Zout, d.H, d.V, d.W
    S0 = d.S0 if per_problem else d.S0[0]

    def yardsticks(b, Kb):
        F = d.blocks(b, d.zo[b])
        return EF.in_both_precisions(_design, F[:, :, :15], F[:, :, 15:19], Kb, H, V, S0[b] if per_problem else S0, W,
                                     d.zo[b][2 + 20 * np.arange(N)], lb=nlp.model.lb)

    Kh, refs, dist, redrawn = _conditioned_gains(TC.to_np(d.K), d.seed, yardsticks)
    K = EF.dev(Kh)
    ref = {n: np.stack([r[n] for r in refs]) for n in ("L", "Pm", "Pp", "X", "marg")}
    got = nlp.tracking_kalman(Zout, H, V, K, S0, W)
    inp = dict(Zout=Zout, K=K, H=H, V=V, S0=S0, W=W, redrawn=redrawn)
    return nlp, inp, got, _host(got), ref, dist


def _errors(g, r):
    return (CR.knot_rel(g["L"], r["L"]), CR.knot_rel(g["Pp"], r["Pp"]), CR.knot_rel(g["X"], r["X"]), CR.entry_rel(g["marg"], r["marg"]))


def _check_structure(g, r):
    """One stored value per pair, non-negative variances, and an update that does not add uncertainty: trace P^+_k against the
    yardstick's prior P^-_k (within the bar on the comparison of the two)."""
    assert np.array_equal(g["Pp"], np.swapaxes(g["Pp"], -1, -2))
    assert (np.diagonal(g["Pp"], axis1=-2, axis2=-1) >= 0).all()
    tp, tm = np.trace(g["Pp"], axis1=-2, axis2=-1), np.trace(r["Pm"], axis1=-2, axis2=-1)
    assert (tp <= tm * (1 + BAR)).all()
    if g["X"] is not None:
        assert np.array_equal(g["X"], np.swapaxes(g["X"], -1, -2))
        assert not g["marg"][:, -1, 1:5].any()


# ---- 1. against the yardstick --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem", CASES)
def test_gains_and_covariances_match_the_yardstick(kind, B, N, k_trans, im, ny, per_problem):
    """L, P^+ and X in knot_rel, marg in entry_rel, against the numpy recursion on the evaluator's dense blocks: within 1e-10.
    Measured worst cases and the yardstick's own distance to longdouble: profiles/tracking_kalman_tests.txt."""
    nlp, inp, _, g, r, dist = _run(kind, B, N, k_trans, im, ny, per_problem)
    errs = _errors(g, r)
    print(f"kalman {kind} B={B} N={N} k_trans={k_trans} mode={im} ny={ny} sigma0_batch={B if per_problem else 1}: L {errs[0]:.2e}, "
          f"Pest {errs[1]:.2e}, Sigma {errs[2]:.2e}, marg {errs[3]:.2e}; yardstick to longdouble {dist:.2e}; gains drawn again for "
          f"{inp['redrawn']} of {B} problems")
    assert g["L"].shape == (B, N, 15, ny)
    assert all(e <= BAR for e in errs), errs
    _check_structure(g, r)


# ---- 2. no measurement: the open-loop covariance sweep, bit for bit ------------------------------------------------------
@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem", [CASES[0], CASES[9], CASES[20], CASES[31], CASES[32]])
def test_without_measurements_the_call_is_the_open_loop_covariance_sweep(kind, B, N, k_trans, im, ny, per_problem):
    import torch

    nlp, inp, _, _, _, _ = _run(kind, B, N, k_trans, im, ny, per_problem)
    L, Pe, S, mg = nlp.tracking_kalman(inp["Zout"], np.zeros((ny, 15)), np.ones(ny), inp["K"], inp["S0"], inp["W"])
    Sr, mr = nlp.tracking_covariance(inp["Zout"], None, inp["S0"], inp["W"])
    assert not bool(L.any())
    assert torch.equal(Pe, Sr) and torch.equal(S, Sr)
    assert not bool(mg[:, :, 1:5].any())
    assert torch.equal(mg[:, :, 0], mr[:, :, 0]) and torch.equal(mg[:, :, 5:], mr[:, :, 5:])


# ---- 3. ny rows are eight rows with the zero rows written out -------------------------------------------------------------
@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem", [c for c in CASES if c[5] == 3][::3])
def test_three_rows_are_eight_rows_with_five_zero_rows_of_unit_variance(kind, B, N, k_trans, im, ny, per_problem):
    import torch

    nlp, inp, got, _, _, _ = _run(kind, B, N, k_trans, im, ny, per_problem)
    H8, V8 = np.zeros((8, 15)), np.ones(8)
    H8[:3], V8[:3] = inp["H"], inp["V"]
    L8, Pe8, S8, mg8 = nlp.tracking_kalman(inp["Zout"], H8, V8, inp["K"], inp["S0"], inp["W"])
    L, Pe, S, mg = got
    assert torch.equal(Pe8, Pe) and torch.equal(S8, S) and torch.equal(mg8, mg)
    assert torch.equal(L8[..., :3], L) and not bool(L8[..., 3:].any())


# ---- 4. which outputs are asked for ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,N,k_trans,im,ny,per_problem", [CASES[2], CASES[21], CASES[32]])
def test_every_subset_of_outputs_has_the_bits_of_the_full_call(kind, B, N, k_trans, im, ny, per_problem):
    import torch

    nlp, inp, got, _, _, _ = _run(kind, B, N, k_trans, im, ny, per_problem)
    for flags in itertools.product((False, True), repeat=4):
        if not any(flags):
            continue
        part = nlp.tracking_kalman(inp["Zout"], inp["H"], inp["V"], inp["K"], inp["S0"], inp["W"], *flags)
        for p, ref, asked in zip(part, got, flags):
            assert (p is None and not asked) or torch.equal(p, ref)
    for flags in ((True, True), (True, False), (False, True)):  # the filter alone
        L, Pe, S, mg = nlp.tracking_kalman(inp["Zout"], inp["H"], inp["V"], None, inp["S0"], inp["W"], *flags)
        assert S is None and mg is None
        assert (L is None and not flags[0]) or torch.equal(L, got[0])
        assert (Pe is None and not flags[1]) or torch.equal(Pe, got[1])


# ---- 6. through the guarded touchdown -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run_guarded(kind, N, im, B, wg):
    d = EF.guarded_design(kind, N, im, B, wg, wg)
    nlp, Zout, ev, evh, H, V, S0, W, K, dK = d.nlp, d.Zout, d.ev, d.evh, d.H, d.V, d.S0, d.W, d.K, d.dK

    def yardsticks(b, Kb):
        s = slice(b, b + 1)
        return EF.in_both_precisions(lambda F, T, *rest: KR.guarded(F, T, evh[s], *rest), d.F[s], d.T[s],
                                     None if Kb is None else Kb[None], H, V, S0[s], W, d.zo[s, 2::20], d.th[s, 3])

    redrawn = 0
    if K is None:  # the filter alone: nothing of it depends on gains
        pairs = [yardsticks(b, None) for b in range(B)]
        refs = [lo for lo, _ in pairs]
        dist = max(CR.knot_rel(lo[n], hi[n]) for lo, hi in pairs for n in ("L", "Pp"))
    else:
        # the roll-out keeps the gains it ran under; the call takes Zout and K independently, as the header says
        K, refs, dist, redrawn = _conditioned_gains(K, d.seed, yardsticks)
        dK = EF.dev(K)
    ref = {n: np.concatenate([r[n] for r in refs]) for n in refs[0]}
    got = nlp.tracking_kalman_guarded(Zout, ev, H, V, dK, S0, W, d.model)
    inp = dict(Zout=Zout, ev=ev, K=dK, model=d.model, H=H, V=V, S0=S0, W=W, evh=evh, redrawn=redrawn)
    return nlp, inp, got, _host(got), ref, dist


@pytest.mark.parametrize("kind,N,im,B,wg", GUARDED)
def test_guarded_call_matches_the_yardstick(kind, N, im, B, wg):
    """On the complex-step blocks of the composite step, every problem included: L, P^+, X in knot_rel, marg and event_var in
    entry_rel, within 1e-10.  Without gains the call is the filter alone."""
    nlp, inp, _, g, r, dist = _run_guarded(kind, N, im, B, wg)
    land = inp["evh"][:, 0] >= 0
    assert land.any()
    if inp["K"] is None:
        errs = (CR.knot_rel(g["L"], r["L"]), CR.knot_rel(g["Pp"], r["Pp"]))
        assert g["X"] is None and g["marg"] is None and g["var"] is None
    else:
        errs = _errors(g, r) + (CR.entry_rel(g["var"], r["event_var"]),)
        assert not g["var"][~land].any() and (g["var"][land, 1] > 0).all()
    print(f"kalman guarded {kind} N={N} mode={im} B={B} K={wg} ny={inp['H'].shape[0]}: " + ", ".join(f"{e:.2e}" for e in errs) +
          f" (L, Pest" + (", Sigma, marg, event_var" if inp["K"] is not None else "") + f"); yardstick to longdouble {dist:.2e}; gains drawn again for {inp['redrawn']} of {B} problems")
    assert all(e <= BAR for e in errs), errs
    _check_structure(g, r)


@pytest.mark.parametrize("kind,N,im,B,wg", [("shape", 8, 1, 48, True), ("shape", 40, 2, 9, True), ("ragged", 12, 0, 70, True)])
def test_guarded_call_without_measurements_is_the_open_loop_guarded_covariance_sweep(kind, N, im, B, wg):
    import torch

    nlp, inp, _, _, _, _ = _run_guarded(kind, N, im, B, wg)
    L, Pe, S, mg, var = nlp.tracking_kalman_guarded(inp["Zout"], inp["ev"], np.zeros((8, 15)), np.ones(8), inp["K"], inp["S0"],
                                                    inp["W"], inp["model"])
    Sr, mr, _ = nlp.tracking_covariance_guarded(inp["Zout"], inp["ev"], None, inp["S0"], inp["W"], inp["model"])
    assert not bool(L.any()) and torch.equal(Pe, Sr) and torch.equal(S, Sr)
    assert not bool(mg[:, :, 1:5].any()) and torch.equal(mg[:, :, 0], mr[:, :, 0]) and torch.equal(mg[:, :, 5:], mr[:, :, 5:])


def test_guarded_subsets_of_outputs_have_the_bits_of_the_full_call():
    import torch

    nlp, inp, got, _, _, _ = _run_guarded("shape", 40, 1, 9, True)
    for flags in itertools.product((False, True), repeat=5):
        if not any(flags):
            continue
        part = nlp.tracking_kalman_guarded(inp["Zout"], inp["ev"], inp["H"], inp["V"], inp["K"], inp["S0"], inp["W"], inp["model"],
                                           *flags)
        for p, ref, asked in zip(part, got, flags):
            assert (p is None and not asked) or torch.equal(p, ref)
    L, Pe, S, mg, var = nlp.tracking_kalman_guarded(inp["Zout"], inp["ev"], inp["H"], inp["V"], None, inp["S0"], inp["W"],
                                                    inp["model"])
    assert S is None and mg is None and var is None and torch.equal(L, got[0]) and torch.equal(Pe, got[1])


@pytest.mark.parametrize("N,im,B", [(8, 1, 48), (40, 2, 9), (5, 2, 32)])
def test_a_batch_that_never_lands_is_bitwise_the_knot_scheduled_call_of_a_handle_that_never_switches(N, im, B):
    """model == NULL and the handle's model passed explicitly, against qln_tracking_kalman of a handle with k_trans = N + 1."""
    import torch

    batch, Zref, K, x0, th = GC.case(N, im, B, True, False)
    iy, iv = GC.free_foot(im)
    Zref[:, 15 + (3 if im == 1 else 1)::20] = -2.0  # every problem gets the last problem's pulling reference
    x0[:, iy], x0[:, iv] = 0.3, 0.0
    nlp, never = TC.nlp(batch, TC.SECOND_MODEL), TC.nlp(GC.with_k_trans(batch, N + 1), TC.SECOND_MODEL)
    dK = EF.dev(K)
    Zout, ev = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), dK, EF.dev(x0))
    assert bool((ev[:, 0] == -1).all())
    rng = np.random.default_rng(N)
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    H, V = EF.measurement(rng, 3)
    for k_ in (dK, None):
        ref = never.tracking_kalman(Zout, H, V, k_, S0, W)
        for model in (None, EF.dev(np.tile(TC.SECOND, (B, 1)))):
            got = nlp.tracking_kalman_guarded(Zout, ev, H, V, k_, S0, W, model)
            for g, r in zip(got[:4], ref):
                assert (g is None and r is None) or torch.equal(g, r)
            assert got[4] is None or not bool(got[4].any())


# ---- 7. host forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 1024])
def test_host_forms_equal_device_forms_after_other_host_calls_left_nans_behind(B):
    """The staging buffers are shared by role: other host forms first leave NaNs in the roles this call reads and writes."""
    N = 12
    batch, Zref, K, x0, th = GC.ragged_case(B=B, N=N)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    dK, dm = EF.dev(K), EF.dev(th)
    Zout, ev = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), dK, EF.dev(x0), dm)
    rng = np.random.default_rng(B)
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    H, V = EF.measurement(rng, 3)
    zh, evh = Zout.cpu().numpy(), ev.cpu().numpy()
    nan = lambda *s: np.full(s, np.nan)  # noqa: E731
    with np.errstate(all="ignore"):
        nlp.tracking_covariance_host(nan(*zh.shape), nan(*K.shape), nan(B, 120), None)
        nlp.tracking_covariance_guarded_host(nan(*zh.shape), evh, nan(*K.shape), nan(B, 120), None, th)
        nlp.tracking_kalman_host(nan(*zh.shape), np.ones((8, 15)), 1.0, nan(*K.shape), nan(B, 120), None)
    for k_ in (K, None):
        dev = nlp.tracking_kalman(Zout, H, V, EF.dev(k_), S0, W)
        host = nlp.tracking_kalman_host(zh, H, V, k_, S0, W)
        for d, h in zip(dev, host):
            assert (d is None and h is None) or np.array_equal(h, d.cpu().numpy())
        dev = nlp.tracking_kalman_guarded(Zout, ev, H, V, EF.dev(k_), S0[0], W, dm)
        host = nlp.tracking_kalman_guarded_host(zh, evh, H, V, k_, S0[0], W, th)
        for d, h in zip(dev, host):
            assert (d is None and h is None) or np.array_equal(h, d.cpu().numpy())
    assert host[0].shape == (B, N, 15, 3) and np.isfinite(host[0]).all() and np.isfinite(host[1]).all()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused():
    import torch

    from quadruped_landing_amd import _lib

    batch, Zref, K, x0, th = GC.case(5, 2, 32, True, True)
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    L, h, INV, OK = _lib.lib(), nlp._h, _lib.QLN_ERR_INVALID_ARGUMENT, _lib.QLN_OK
    B, N = nlp.B, nlp.N
    dK, dm = EF.dev(K), EF.dev(th)
    Zout, ev = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), dK, EF.dev(x0), dm)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    Lo, Po, So, mo, vo, S0, Hd = f64(B, N, 15, 8), f64(B, N, 120), f64(B, N, 120), f64(B, N, 8), f64(B, 2), f64(120), f64(8, 15)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    a = lambda v: v.ctypes.data  # noqa: E731
    V, W = np.ones(8), np.zeros(15)
    kal, gkal = L.qln_tracking_kalman, L.qln_tracking_kalman_guarded
    for ny in (0, 9):
        assert kal(h, p(Zout), p(dK), p(Hd), ny, a(V), p(S0), 1, a(W), p(Lo), None, None, None) == INV
    assert kal(h, p(Zout), p(dK), None, 8, a(V), p(S0), 1, a(W), p(Lo), None, None, None) == INV  # H == NULL
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(np.array([1.0] * 7 + [0.0])), p(S0), 1, a(W), p(Lo), None, None, None) == INV
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 1, a(np.array([0.0] * 14 + [-1.0])), p(Lo), None, None, None) == INV
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 2, a(W), p(Lo), None, None, None) == INV  # sigma0_batch
    assert b"sigma0_batch" in L.qln_last_error()
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 1, a(W), None, None, None, None) == INV  # no output
    assert kal(h, p(Zout), None, p(Hd), 8, a(V), p(S0), 1, a(W), p(Lo), None, p(So), None) == INV  # Sigma without K
    assert kal(h, p(Zout), None, p(Hd), 8, a(V), p(S0), 1, a(W), p(Lo), None, None, p(mo)) == INV  # marg without K
    assert gkal(h, p(Zout), None, None, p(ev), p(Hd), 8, a(V), p(S0), 1, a(W), p(Lo), None, None, None, p(vo)) == INV
    assert gkal(h, p(Zout), p(dK), None, None, p(Hd), 8, a(V), p(S0), 1, a(W), p(Lo), None, None, None, None) == INV  # NULL event
    assert b"event" in L.qln_last_error()
    # overlaps: the new roles H, Lgain and Pest take part
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 1, a(W), p(Hd), None, None, None) == INV  # Lgain over H
    assert b"overlaps" in L.qln_last_error()
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 1, a(W), None, p(Hd), None, None) == INV  # Pest over H
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 1, a(W), p(Lo), p(Lo), None, None) == INV  # Pest over Lgain
    assert b"two outputs" in L.qln_last_error()
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 1, a(W), None, p(Po), p(Po), None) == INV  # Sigma over Pest
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 1, a(W), p(Zout), None, None, None) == INV  # Lgain over Zout
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 1, a(W), None, p(dK), None, None) == INV  # Pest over K
    assert gkal(h, p(Zout), p(dK), p(dm), p(ev), p(Hd), 8, a(V), p(S0), 1, a(W), p(Lo), None, None, None, p(ev)) == INV
    assert gkal(h, p(Zout), p(dK), p(dm), p(ev), p(Hd), 8, a(V), p(S0), 1, a(W), p(dm), None, None, None, None) == INV
    assert kal(h, p(Zout), p(dK), p(Hd), 8, a(V), p(S0), 1, a(W), p(Lo), p(Po), p(So), p(mo)) == OK
    assert kal(h, p(Zout), None, p(Hd), 1, a(V), p(S0), 1, None, None, p(Po), None, None) == OK  # the filter alone, Pest alone
    assert gkal(h, p(Zout), p(dK), p(dm), p(ev), p(Hd), 8, a(V), p(S0), 1, a(W), None, None, None, None, p(vo)) == OK
    torch.cuda.synchronize()
    # host forms: the same, and the values of H, of the record and of the models
    zo, evh, S0h, Hh = Zout.cpu().numpy(), ev.cpu().numpy(), np.zeros(120), np.zeros((8, 15))
    Lh = np.zeros((B, N, 15, 8))
    hk, hg = L.qln_tracking_kalman_host, L.qln_tracking_kalman_guarded_host
    assert hk(h, a(zo), a(K), a(Hh), 9, a(V), a(S0h), 1, a(W), a(Lh), None, None, None) == INV
    assert hk(h, a(zo), a(K), a(Hh), 8, a(V), a(S0h), 1, a(W), None, None, None, None) == INV
    assert hg(h, a(zo), a(K), None, None, a(Hh), 8, a(V), a(S0h), 1, a(W), a(Lh), None, None, None, None) == INV
    for value in (np.nan, np.inf):
        bad = Hh.copy()
        bad[7, 14] = value
        assert hk(h, a(zo), a(K), a(bad), 8, a(V), a(S0h), 1, a(W), a(Lh), None, None, None) == INV
        assert b"H is not finite" in L.qln_last_error()
        assert hk(h, a(zo), a(K), a(bad), 7, a(V), a(S0h), 1, a(W), a(Lh), None, None, None) == OK  # behind ny: not read
        assert hg(h, a(zo), a(K), a(th), a(evh), a(bad), 8, a(V), a(S0h), 1, a(W), a(Lh), None, None, None, None) == INV
    for entry, value in ((0, 0.5), (0, float(N - 1)), (1, -1e-3), (1, np.nan)):
        bad = np.array(evh)
        bad[B - 2, entry] = value
        assert hg(h, a(zo), a(K), None, a(bad), a(Hh), 8, a(V), a(S0h), 1, a(W), a(Lh), None, None, None, None) == INV, (entry, value)
    for entry, value in ((0, np.nan), (1, 0.0), (3, np.inf)):
        bad = np.array(th)
        bad[3, entry] = value
        assert hg(h, a(zo), a(K), a(bad), a(evh), a(Hh), 8, a(V), a(S0h), 1, a(W), a(Lh), None, None, None, None) == INV, (entry, value)
    assert hg(h, a(zo), a(K), a(th), a(evh), a(Hh), 8, a(V), a(S0h), 1, a(W), a(Lh), None, None, None, None) == OK
    # the Python layer refuses what measurement_model refuses before any call
    with pytest.raises(ValueError):
        nlp.tracking_kalman(Zout, np.ones((9, 15)), 1.0, dK, np.ones(15))
    with pytest.raises(ValueError):
        nlp.tracking_kalman(Zout, np.ones((2, 15)), [1.0, 0.0], dK, np.ones(15))
