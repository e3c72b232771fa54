"""The yardstick of the sweeps through the estimate-feedback roll-out (tests/rollout_estimated_sweep_ref.py), held on the CPU
independently of the kernels: its forward sweep against longdouble central differences of tests/rollout_estimated_ref.rollout in
every tangent, its reverse sweep as the adjoint of the forward one, its own float64-to-longdouble distance -- and what of the
eight entry points needs no device: the ctypes table and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from tests import rollout_estimated_sweep_ref as ES

# (N, init_mode, k_trans, B, ny): the GPU tests' small family and one full-length case
CASES = [(5, 1, 2, 16, 3), (5, 2, 4, 16, 8), (5, 1, 5, 16, 1), (40, 2, 14, 9, 8)]
LEFT_OUT = 0.10  # the share of a case's problems whose plant or estimator changes its touchdown knot over the difference's step
# The quotient's own error: truncation t^2 |f'''| / 6 at t = 1e-6 is below 1e-11 for the tangents' size of 1e-2, and the
# longdouble roll-out's rounding 1e-19 |x| / t below 1e-12: a sweep that is right agrees to 1e-9 of max(1, |ref|); one that
# misses a term (the saltation term, a gain's tangent) misses by the term's size, 1e-4 and more (measured with freeze_tau).
FD_BAR = 1e-9


def _trajectory(N, im, kt, B, ny, guarded, with_xhat0=True):
    batch, inp = ES.case(N, im, kt, B, ny, guarded)
    if not with_xhat0:
        inp = dict(inp, xhat0=None)
    out = ES.rollout(batch, inp, guarded)
    blk = ES.chain_blocks(N, np.asarray(batch.init_mode), np.asarray(batch.k_trans), out["Zout"], out["Xhat"], inp["model"],
                          ES.TC.SECOND, guarded, out.get("events"), out.get("events_hat"))
    return batch, inp, out, blk


def _jvp(blk, inp, out, dirs):
    if inp["xhat0"] is not None and "xhat0_dot" not in dirs:
        dirs = dict(dirs, xhat0_dot=np.zeros_like(inp["xhat0"]))  # a given xhat0 held fixed: None would follow Zref_dot
    return ES.sweep_jvp(blk, inp["Zref"], inp["K"], inp["Lgain"], inp["H"], out["Zout"], out["Xhat"], out["innov"],
                        events=out.get("events"), events_hat=out.get("events_hat"), **dirs)


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_forward_sweep_matches_longdouble_central_differences_in_every_tangent(N, im, kt, B, ny, guarded):
    """Each tangent alone, all together, and all but xhat0_dot on a roll-out with xhat0 = None (the estimate follows Zref), on
    the problems whose plant and estimator keep their touchdown knots at both offsets."""
    worst, left = 0.0, 0
    for with_xhat0 in (True, False):
        batch, inp, out, blk = _trajectory(N, im, kt, B, ny, guarded, with_xhat0)
        full, _ = ES.directions(N + ny, B, N, ny)
        if not with_xhat0:
            full = {k: v for k, v in full.items() if k != "xhat0_dot"}
        sets = [full] + ([{k: full[k]} for k in full] if with_xhat0 else [])
        for dirs in sets:
            fd, same = ES.central_difference(batch, inp, guarded, dirs)
            assert (~same).mean() <= LEFT_OUT, f"{(~same).sum()} of {B} problems change a touchdown knot over the step"
            left = max(left, int((~same).sum()))
            ref = _jvp(blk, inp, out, dirs)
            for name, q in fd.items():
                w = ES.worst(ref[name][same], q[same])
                worst = max(worst, w)
                assert w <= FD_BAR, (name, sorted(dirs), w)
        if guarded:
            assert (out["events"][:, 0] >= 0).any() and (out["events_hat"][:, 0] >= 0).any()
    print(f"N={N} mode={im} k_trans={kt} B={B} ny={ny} guarded={guarded}: yardstick's forward sweep against the longdouble quotient "
          f"{worst:.2e} of max(1, |ref|); bar {FD_BAR:.0e}; at most {left} of {B} problems left out")


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("with_xhat0", [True, False])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_reverse_sweep_is_the_adjoint_of_the_forward_sweep(N, im, kt, B, ny, guarded, with_xhat0):
    batch, inp, out, blk = _trajectory(N, im, kt, B, ny, guarded, with_xhat0)
    dirs, cot = ES.directions(N + ny + 1, B, N, ny)
    if not with_xhat0:
        dirs = {k: v for k, v in dirs.items() if k != "xhat0_dot"}
    fwd = _jvp(blk, inp, out, dirs)
    rev = ES.sweep_vjp(blk, inp["Zref"], inp["K"], inp["Lgain"], inp["H"], out["Zout"], out["Xhat"], out["innov"], cot["Zbar"],
                       cot["Xhat_bar"], cot["innov_bar"], with_xhat0)
    lhs = sum(float(np.sum(cot[c] * fwd[o])) for c, o in (("Zbar", "Zout_dot"), ("Xhat_bar", "Xhat_dot"), ("innov_bar", "innov_dot")))
    rhs = sum(float(np.sum(rev[k[:-4] + "_bar"] * v)) for k, v in dirs.items())
    print(f"N={N} guarded={guarded} xhat0={with_xhat0}: <bar, J d> {lhs:.15e}, <J' bar, d> {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs))
    assert (rev["xhat0_bar"] is None) == (not with_xhat0)


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("N,im,kt,B,ny", CASES)
def test_distance_of_the_float64_yardstick_from_its_longdouble_restatement(N, im, kt, B, ny, guarded):
    """Printed, and small against the GPU tests' bar of 1e-12: what that bar is widened by where it is not."""
    batch, inp, out, blk = _trajectory(N, im, kt, B, ny, guarded)
    blkl = ES.chain_blocks(N, np.asarray(batch.init_mode), np.asarray(batch.k_trans), out["Zout"], out["Xhat"], inp["model"],
                           ES.TC.SECOND, guarded, out.get("events"), out.get("events_hat"), ctype=np.clongdouble)
    dirs, cot = ES.directions(N + ny + 2, B, N, ny)
    args = (inp["Zref"], inp["K"], inp["Lgain"], inp["H"], out["Zout"], out["Xhat"], out["innov"])
    ev = dict(events=out.get("events"), events_hat=out.get("events_hat"))
    f, fl = ES.sweep_jvp(blk, *args, **dirs, **ev), ES.sweep_jvp(blkl, *args, **dirs, **ev)
    r, rl = ES.sweep_vjp(blk, *args, **cot), ES.sweep_vjp(blkl, *args, **cot)
    dist = max([ES.worst(f[k], fl[k]) for k in f] + [ES.worst(r[k], rl[k]) for k in r])
    print(f"N={N} mode={im} k_trans={kt} B={B} ny={ny} guarded={guarded}: float64 yardstick to longdouble {dist:.2e}")
    assert dist <= 1e-12


# ---- what of the entry points needs no device --------------------------------------------------------------------------------
NAMES = {"qln_tracking_rollout_estimated_jvp": 19, "qln_tracking_rollout_estimated_vjp": 19,
         "qln_tracking_rollout_estimated_guarded_jvp": 23, "qln_tracking_rollout_estimated_guarded_vjp": 21}


def test_ctypes_table():
    from quadruped_landing_amd import _lib

    for base, n in NAMES.items():
        for name in (base, base + "_host"):
            res, args = _lib.SIGNATURES[name]
            assert res is C.c_int and len(args) == n
            assert [i for i, a in enumerate(args) if a is C.c_int32] == [5]
            assert getattr(_lib.lib(), name).argtypes == args


def test_entry_points_reject_bad_arguments_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    bad = _lib.QLN_ERR_INVALID_ARGUMENT
    a = np.zeros(2000)
    p = a.ctypes.data
    for base in NAMES:
        for name in (base, base + "_host"):
            fn = getattr(L, name)
            guarded, fwd = "guarded" in name, "jvp" in name

            def call(K=None, Lg=p, H=p, ny=8, Zout=p, Xhat=p, innov=None, ev=(p, p), first=p, k_=None, l_=None, main=p):
                head = (None, p, K, Lg, H, ny, None, Zout, Xhat, innov) + (ev if guarded else ())
                if fwd:  # Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, Zout_dot, Xhat_dot, innov_dot[, event dots]
                    return fn(*head, None, k_, l_, first, None, None, main, None, None, *((None, None) if guarded else ()))
                return fn(*head, main, None, None, None, k_, l_, first, None, None)  # Zbar, ..., K_bar, Lgain_bar, x0_bar, ...

            assert call() == bad and b"null handle" in L.qln_last_error()
            for ny in (0, 9, -1):
                assert call(ny=ny) == bad and b"ny must be" in L.qln_last_error()
            assert call(Lg=None) == bad and b"null Lgain or H" in L.qln_last_error()
            assert call(H=None) == bad and b"null Lgain or H" in L.qln_last_error()
            assert call(Zout=None) == bad and b"null Zref, Zout or Xhat" in L.qln_last_error()
            assert call(Xhat=None) == bad and b"null Zref, Zout or Xhat" in L.qln_last_error()
            assert call(l_=p) == bad and b"null innov" in L.qln_last_error()
            assert call(l_=p, innov=p) == bad and b"null handle" in L.qln_last_error()
            assert call(k_=p) == bad and b"needs K" in L.qln_last_error()
            assert call(main=None) == bad and (b"null Zout_dot" if fwd else b"null Zbar") in L.qln_last_error()
            if fwd:
                assert call(first=None) == bad and b"every tangent is NULL" in L.qln_last_error()
            if guarded:
                assert call(ev=(None, p)) == bad and b"null event or event_hat" in L.qln_last_error()
                assert call(ev=(p, None)) == bad and b"null event or event_hat" in L.qln_last_error()
