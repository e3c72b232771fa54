"""The numpy yardstick of qln_landing_filter_jvp / _vjp (tests/landing_filter_sweep_ref.py), held on the CPU before the GPU tests
rely on it: against longdouble central differences of landing_filter_ref.replay in every tangent, one at a time and all
together, the score included; the adjoint identity between its two sweeps; its own distance from a longdouble restatement.
The seeds are those of landing_filter_sweep_ref.record, which the GPU tests run: no problem changes its estimator's touchdown
knot over the step, which is asserted, and no problem is left out."""
import functools

import numpy as np
import pytest

from tests import landing_filter_sweep_ref as FS

# (N, init_mode, k_trans, B, ny): N = 5 and 17, ny over 1, 3, 8; each scheduled and guarded
CASES = [(5, 1, 2, 6, 1), (5, 2, 4, 6, 3), (5, 1, 3, 6, 8), (17, 1, 6, 6, 3), (17, 2, 9, 6, 8), (17, 2, 12, 6, 1)]
# The quotient's own error at t = 1e-6 in longdouble: truncation t^2 |f'''| / 6, below 1e-11 for tangents of size 1e-2 on the
# states; nis divides by V = 1e-2 .. 2.75e-2 and is quadratic in the innovations, which costs two more digits; rounding
# 1e-19 |x| / t is below 1e-12.  A sweep that is right agrees to 1e-9 of max(1, |ref|), one that misses a term (the saltation
# term, the model's column, e's dependence on dinnov) misses by the term's size, 1e-4 and more.
FD_BAR = 1e-9
STEP = 1e-6


@functools.lru_cache(maxsize=None)
def _point(N, im, kt, B, ny, guarded):
    batch, rec = FS.record(N, im, kt, B, ny, guarded)
    out = FS.replay(batch, rec, guarded)
    ev = out.get("events_hat")
    mk = lambda ct: FS.blocks(N, np.asarray(batch.init_mode), np.asarray(batch.k_trans), rec["Zrec"], out["Xhat"], rec["model"],  # noqa: E731
                              guarded, ev, ctype=ct)
    return batch, rec, out, mk(np.complex128), mk


def _jvp(F, T, rec, out, dirs, score):
    return FS.sweep_jvp(F, T, rec["Lgain"], rec["H"], out["innov"], rec["V"] if score else None, out.get("events_hat"), **dirs)


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_forward_sweep_matches_longdouble_central_differences_in_every_tangent(N, im, kt, B, ny, guarded):
    """Each tangent alone; the four that go with the score together, nis and loglik included; all five together, where the
    score is not differentiated (the gains move)."""
    batch, rec, out, (F, T), _ = _point(N, im, kt, B, ny, guarded)
    full, _ = FS.directions(N + ny, B, N, ny)
    fixed = {k: v for k, v in full.items() if k != "Lgain_dot"}
    worst = 0.0
    for dirs in [full, fixed] + [{k: full[k]} for k in full]:
        score = "Lgain_dot" not in dirs
        fd, same, centre = FS.central_difference(batch, rec, guarded, dirs, STEP)
        assert same.all(), f"{(~same).sum()} of {B} problems change the estimator's touchdown knot over the step"
        ref = _jvp(F, T, rec, out, dirs, score)
        for name, q in fd.items():
            if name in ref:
                w = FS.worst(ref[name], q)
                worst = max(worst, w)
                assert w <= FD_BAR, (name, sorted(dirs), w)
        assert not score or {"nis_dot", "loglik_dot"} <= set(ref)
    if guarded:
        assert (out["events_hat"][:, 0] >= 0).any()
    print(f"N={N} mode={im} k_trans={kt} B={B} ny={ny} guarded={guarded}: yardstick's forward sweep against the longdouble quotient "
          f"{worst:.2e} of max(1, |ref|); bar {FD_BAR:.0e}; no problem left out")


@pytest.mark.parametrize("score", [False, True])
@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_reverse_sweep_is_the_adjoint_of_the_forward_sweep(N, im, kt, B, ny, guarded, score):
    batch, rec, out, (F, T), _ = _point(N, im, kt, B, ny, guarded)
    dirs, cot = FS.directions(N + ny + 1, B, N, ny)
    if score:
        dirs = {k: v for k, v in dirs.items() if k != "Lgain_dot"}
    else:
        cot = {k: v for k, v in cot.items() if k in ("Xhat_bar", "innov_bar")}
    fwd = _jvp(F, T, rec, out, dirs, score)
    rev = FS.sweep_vjp(F, rec["Lgain"], rec["H"], out["innov"], rec["V"] if score else None, **cot)
    assert (rev["Lgain_bar"] is None) == score
    lhs, rhs = FS.inner(cot, fwd, rev, dirs)
    print(f"N={N} guarded={guarded} score={score}: <bar, J d> {lhs:.15e}, <J' bar, d> {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs)) and lhs != 0.0


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_distance_of_the_float64_yardstick_from_its_longdouble_restatement(N, im, kt, B, ny, guarded):
    """Printed, and small against the GPU tests' bar of 1e-12: what that bar is widened by where it is not."""
    batch, rec, out, (F, T), mk = _point(N, im, kt, B, ny, guarded)
    Fl, Tl = mk(np.clongdouble)
    dirs, cot = FS.directions(N + ny + 2, B, N, ny)
    dirs = {k: v for k, v in dirs.items() if k != "Lgain_dot"}
    f, fl = _jvp(F, T, rec, out, dirs, True), _jvp(Fl, Tl, rec, out, dirs, True)
    args = (rec["Lgain"], rec["H"], out["innov"], rec["V"])
    r, rl = FS.sweep_vjp(F, *args, **cot), FS.sweep_vjp(Fl, *args, **cot)
    dist = max([FS.worst(f[k], fl[k]) for k in f] + [FS.worst(r[k], rl[k]) for k in r if r[k] is not None])
    print(f"N={N} mode={im} k_trans={kt} B={B} ny={ny} guarded={guarded}: float64 yardstick to longdouble {dist:.2e}")
    assert dist <= 1e-12
