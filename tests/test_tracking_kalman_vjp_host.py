"""CPU checks of the reverse sweep through the Kalman design (qln_noise_design_vjp): the numpy yardstick
tests/tracking_kalman_vjp_ref.py against the transpose of the forward yardstick's dense matrix (tests/tracking_kalman_sweep_ref.py,
built column by column in longdouble), the duality identity over the stored arrays in float64 and in longdouble, the yardstick's
float64 against its longdouble, and the composition of HybridNLP.landing_loglik_grad, restated in numpy, against longdouble
central differences of the filter's log-likelihood under redesign, entry by entry in W and V.

Where a bar is not the quotient's own error it is a multiple of the format's epsilon, stated where it is used.  Measured values:
profiles/tracking_kalman_vjp_tests.txt."""
import inspect

import numpy as np
import pytest

from tests import landing_filter_sweep_ref as FS
from tests import rollout_ref as RR
from tests import tracking_cov_ref as CR
from tests import tracking_kalman_sweep_ref as KS
from tests import tracking_kalman_vjp_ref as KV
from tests.test_tracking_kalman_sweep_host import CASES, NYS, T_STEP, _case, _loglik_under_redesign

LD = np.longdouble
EPS = {np.float64: float(np.finfo(np.float64).eps), LD: float(np.finfo(LD).eps)}
# A sweep is N knots of sums of a few hundred products, and I - H L loses about a digit at these V (tests/
# test_tracking_kalman_sweep_host.py): 1e4 epsilons of the format, relative to the largest entry or to the sum of the magnitudes.
ROUNDING = 1e4


def _cast(dt, *a):
    return tuple(None if x is None else np.asarray(x).astype(dt) for x in a)


def _setup(form, N, a, b, ny, dt):
    """(A, H, V, gains of the design in dt, a direction, cotangents, B), all in dt"""
    A, H, V, S0, W, dirs, _ = _case(form, N, a, b, ny)
    L = KS.design(A, H, V, S0, W, dt)["L"]
    cot = KV.cotangents(7 * N + ny, N, ny, (len(A),))
    return _cast(dt, A, H, V) + (L,) + (_cast(dt, *dirs["all"]), _cast(dt, *cot), len(A))


@pytest.mark.parametrize("ny", NYS)
@pytest.mark.parametrize("form,N,a,b", [c for c in CASES if c[1] == 5])
def test_yardstick_is_the_transpose_of_the_forward_yardsticks_matrix(form, N, a, b, ny):
    """The dense matrix of tracking_kalman_sweep_ref.sweep between the stored arrays, column by column in longdouble, transposed
    and applied to the cotangents, against the yardstick: to longdouble rounding, relative to each output's largest entry."""
    A, H, V, L, _, (Lb, Pb, lb), B = _setup(form, N, a, b, ny, LD)
    got = KV.sweep(A, H, V, L, Lb, Pb, lb)
    worst = 0.0
    for p in range(B):
        D = KV.dense_forward(A[p], H, V, L[p])
        assert D.shape == (N * 15 * ny + N * 120 + N, 120 + 15 + ny)
        ref = D.T @ np.concatenate([Lb[p].reshape(-1), Pb[p].reshape(-1), lb[p].reshape(-1)])
        for name, r in (("Sigma0", ref[:120]), ("W", ref[120:135]), ("V", ref[135:])):
            e, _ = KV.out_rel(got[name][p], r)
            worst = max(worst, e)
            assert e <= ROUNDING * EPS[LD], (name, p, e)
    print(f"design vjp {form} N={N} ny={ny}: yardstick to the transposed matrix {worst:.2e} (longdouble)")


@pytest.mark.parametrize("dt", [np.float64, LD], ids=["float64", "longdouble"])
@pytest.mark.parametrize("ny", NYS)
@pytest.mark.parametrize("form,N,a,b", CASES)
def test_duality_over_the_stored_arrays(form, N, a, b, ny, dt):
    """<Lb, Ld> + <Pb, Pd> + <lb, ld> = <S0b, S0d> + <Wb, wd> + <Vb, vd> per problem with no weights, relative to the sum of the
    products' magnitudes on the left."""
    A, H, V, L, (S0d, Wd, Vd), cot, _ = _setup(form, N, a, b, ny, dt)
    fwd = KS.sweep(A, H, V, L, S0d, Wd, Vd)
    rev = KV.sweep(A, H, V, L, *cot)
    lhs, rhs = KV.inner(cot, fwd, rev, (S0d, Wd, Vd))
    mag, _ = KV.inner(tuple(np.abs(c) for c in cot), {k: np.abs(v) for k, v in fwd.items()}, rev, (S0d, Wd, Vd))
    gap = float(np.max(np.abs(lhs - rhs) / mag))
    print(f"design vjp {form} N={N} ny={ny} {np.dtype(dt).name}: duality gap {gap:.2e} of the magnitudes")
    assert gap <= ROUNDING * EPS[dt], gap


@pytest.mark.parametrize("ny", NYS)
@pytest.mark.parametrize("form,N,a,b", CASES)
def test_float64_yardstick_against_its_longdouble(form, N, a, b, ny):
    """The yardstick's own rounding at the float64 design's gains, which the GPU test measures the kernel with."""
    A, H, V, L, _, cot, _ = _setup(form, N, a, b, ny, np.float64)
    lo = KV.sweep(A, H, V, L, *cot)
    hi = KV.sweep(*_cast(LD, A, H, V, L), *_cast(LD, *cot))
    e = {k: KV.out_rel(lo[k], hi[k])[0] for k in KV.OUT}
    print(f"design vjp {form} N={N} ny={ny}: float64 yardstick to longdouble " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= ROUNDING * EPS[np.float64], e


def test_a_cotangent_of_knot_0s_covariance_alone_leaves_no_process_noise_gradient():
    form, N, a, b = CASES[0]
    A, H, V, L, _, (_, Pb, _), _ = _setup(form, N, a, b, 3, np.float64)
    Pb[:, 1:] = 0.0
    out = KV.sweep(A, H, V, L, None, Pb, None)
    assert not out["W"].any() and out["Sigma0"].any() and out["V"].any()


def test_the_library_and_the_binding_have_the_sweep():
    """What this yardstick is the yardstick of: the four entries in the library (it loads without a device) and the binding's
    methods, whose composition loglik_grad() restates."""
    from quadruped_landing_amd import HybridNLP, _lib

    L = _lib.lib()
    for name in ("qln_noise_design_vjp", "qln_noise_design_vjp_host", "qln_noise_design_guarded_vjp",
                 "qln_noise_design_guarded_vjp_host"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    for method in ("tracking_kalman_vjp", "tracking_kalman_vjp_host"):
        p = inspect.signature(getattr(HybridNLP, method)).parameters
        assert list(p)[1:] == ["Zout", "Lgain", "H", "V", "Lgain_bar", "Pest_bar", "logdet_bar", "events", "model", "guarded", "want",
                               "reduce"]
    assert HybridNLP.KALMAN_VJP_OUT == ("Sigma0", "W", "V")
    jvp = [p for p in inspect.signature(HybridNLP.landing_loglik_jvp).parameters if not p.endswith("_dot")]
    assert list(inspect.signature(HybridNLP.landing_loglik_grad).parameters) == jvp


# ---- the composition of landing_loglik_grad -------------------------------------------------------------------------------
def _grad(batch, rec, guarded, A, S0, W, V, dt):
    """loglik_grad() at the design and the replay in dt: dict(Sigma0, W, V) per record"""
    d, r = _loglik_under_redesign(batch, rec, guarded, A, S0.astype(dt), W.astype(dt), V.astype(dt), dt)
    im, kt = np.asarray(batch.init_mode), np.asarray(batch.k_trans)
    ctype = np.clongdouble if dt is LD else np.complex128
    F, _ = FS.blocks(batch.N, im, kt, rec["Zrec"], r["Xhat"], rec["model"], guarded, r.get("events_hat"), ctype=ctype)
    F = F.real.astype(dt)
    vjp = lambda ib: FS.sweep_vjp(F, d["L"], rec["H"], r["innov"], None, innov_bar=ib)["Lgain_bar"]  # noqa: E731
    return KV.loglik_grad(A.astype(dt), F, d["L"], rec["H"], V.astype(dt), r["innov"], vjp)


@pytest.mark.parametrize("N,guarded", [(5, False), (17, False), (5, True), (17, True)])
def test_loglik_grad_against_central_differences_of_loglik_under_redesign(N, guarded):
    """One central difference per entry of W and of V, in longdouble, along that entry's relative change, the gains designed
    again at both offsets; the gradient's entry times the entry's own size is set against it.  The bar is ten times the distance
    of the quotients at t and t / 2.  The distance is taken over a record's whole gradient, the worst entry relative to the
    record's largest: loglik is several hundred, so its longdouble rounding over 2 t puts the same absolute noise of 1e-11 on
    every quotient, whatever the entry's size, and the distance of two quotients of one entry is one draw of that noise (it can
    be an exact zero).  The float64 composition's distance is recorded."""
    ny, B = 3, 3
    batch, rec = FS.record(N, 1, max(2, N // 3), B, ny, guarded, seed=40 + N)
    rec = dict(rec)
    V = 1e-2 * (1.0 + 0.25 * np.arange(ny))
    im, kt = np.asarray(batch.init_mode), np.asarray(batch.k_trans)
    A = np.stack([RR.complex_step_blocks(N, int(kt[b]), int(im[b]), rec["Zref"][b])[:, :, :15] for b in range(B)])
    rng = np.random.default_rng(N)
    S0, W = 1e-4 * CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-6, size=15)

    def loglik(Wv, Vv):
        return _loglik_under_redesign(batch, rec, guarded, A, S0.astype(LD), Wv, Vv, LD)[1]

    c = loglik(W.astype(LD), V.astype(LD))
    g = {dt: _grad(batch, rec, guarded, A, S0, W, V, dt) for dt in (LD, np.float64)}
    q1, q2, got = [], [], {LD: [], np.float64: []}
    for which, size in (("W", 15), ("V", ny)):
        for p in range(size):
            quot = []
            for step in (T_STEP, T_STEP / 2):
                side = []
                for s in (step, -step):
                    Wv, Vv = W.astype(LD), V.astype(LD)
                    (Wv if which == "W" else Vv)[p] *= 1 + LD(s)
                    r = loglik(Wv, Vv)
                    if guarded:
                        assert np.array_equal(r["events_hat"][:, 0], c["events_hat"][:, 0])
                    side.append(r["loglik"])
                quot.append((side[0] - side[1]) / (2 * LD(step)))
            q1.append(quot[0])
            q2.append(quot[1])
            for dt in got:
                got[dt].append(g[dt][which][:, p].astype(LD) * LD((W if which == "W" else V)[p]))
    q1, q2 = np.stack(q1), np.stack(q2)  # (15 + ny, B)
    scale = np.abs(q2).max(axis=0)
    dist = lambda x: float(np.max(np.abs(x - q2) / scale))  # noqa: E731
    own, err = dist(q1), {dt: dist(np.stack(got[dt])) for dt in got}
    print(f"loglik gradient under redesign N={N} guarded={guarded}: composition to the quotients {err[LD]:.2e} in longdouble, "
          f"{err[np.float64]:.2e} in float64, of the record's largest entry; the quotients' own error {own:.2e}")
    assert err[LD] <= 10 * own, (err, own)
