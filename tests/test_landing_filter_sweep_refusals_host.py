"""The refusals of qln_landing_filter_model*, qln_landing_filter_jvp* and qln_landing_filter_vjp* that need no device: each is
called with a null handle, so the latest refusal a call can reach is "null handle" and nothing touches a device.  Every refusal
gives QLN_ERR_INVALID_ARGUMENT and its text, and the checks that need no handle come before the null handle, in the family's
order: ny, the tangents (cotangents), the outputs, Lgain's tangent together with a score term, Vdiag missing with a score term,
V's entries, innov where it is required, event_hat (guarded), then H and Lgain."""
import ctypes as C

import pytest

from quadruped_landing_amd import _lib

POINT = ("Zref", "Zrec", "Lgain", "H", "ny", "model", "Vdiag", "Xhat", "innov")
TAN = ("Y_dot", "Zrec_dot", "Lgain_dot", "xhat0_dot", "model_dot")
JOUT = ("Xhat_dot", "innov_dot", "nis_dot", "loglik_dot")
COT = ("Xhat_bar", "innov_bar", "nis_bar", "loglik_bar")
VOUT = ("Y_bar", "Zrec_bar", "Lgain_bar", "xhat0_bar", "model_bar")
FILTER = ("Zref", "Zrec", "Lgain", "H", "ny", "model", "Vdiag", "Y", "xhat0", "Xhat", "innov", "score", "loglik")
PARAMS = {
    "qln_landing_filter_model": FILTER,
    "qln_landing_filter_guarded_model": FILTER + ("event_hat",),
    "qln_landing_filter_jvp": POINT + TAN + JOUT,
    "qln_landing_filter_guarded_jvp": POINT + ("event_hat",) + TAN + JOUT + ("event_hat_dot",),
    "qln_landing_filter_vjp": POINT + COT + VOUT,
    "qln_landing_filter_guarded_vjp": POINT + ("event_hat",) + COT + VOUT,
}
PARAMS.update({k + "_host": v for k, v in list(PARAMS.items())})
NAMES = sorted(PARAMS)
SWEEPS = [n for n in NAMES if "jvp" in n or "vjp" in n]
INV = _lib.QLN_ERR_INVALID_ARGUMENT
NH = (INV, "null handle")


def _call(name, **change):
    """The symbol with a null handle, every pointer at its own buffer of ones and ny = 2; change: None, an int, or (index, value)"""
    types = _lib.SIGNATURES[name][1][1:]
    assert len(types) == len(PARAMS[name])
    keep, args = [], [None]
    for p, t in zip(PARAMS[name], types):
        if t is C.c_int32:
            args.append(change.get(p, 2))
            continue
        buf = (C.c_double * 64)(*([1.0] * 64))
        keep.append(buf)
        if p in change and change[p] is None:
            args.append(None)
            continue
        if p in change:
            buf[change[p][0]] = change[p][1]
        args.append(C.cast(buf, C.POINTER(C.c_double)))
    L = _lib.lib()
    code = getattr(L, name)(*args)
    return int(code), L.qln_last_error().decode()


def _none(name, *params):
    return {p: None for p in params if p in PARAMS[name]}


def _roles(name):
    """(the tangents or cotangents, the outputs, Lgain's, the score's terms) of a sweep"""
    if "jvp" in name:
        return TAN, JOUT + ("event_hat_dot",), "Lgain_dot", ("nis_dot", "loglik_dot")
    return COT, VOUT, "Lgain_bar", ("nis_bar", "loglik_bar")


def test_the_symbols_are_declared_with_ny_in_the_familys_place():
    for n in NAMES:
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and len(args) == len(PARAMS[n]) + 1
        assert [i for i, a in enumerate(args) if a is C.c_int32] == [5]
        assert PARAMS[n][5] == "model"  # behind ny, in the family's order


@pytest.mark.parametrize("name", [n for n in NAMES if n not in SWEEPS])
def test_the_model_forms_of_the_filter_refuse_what_the_filter_refuses(name):
    assert _call(name) == NH and _call(name, model=None) == NH
    assert _call(name, ny=9) == (INV, name + ": ny must be in [1, 8]")
    outs = _none(name, "Xhat", "innov", "score", "loglik", "event_hat")
    assert _call(name, **outs) == (INV, name + ": every output is NULL (nothing to compute)")
    assert _call(name, Vdiag=None) == (INV, name + ": null Vdiag with score or loglik")
    assert _call(name, Vdiag=(1, 0.0)) == (INV, name + ": Vdiag must be finite and > 0 (entry 1)")
    for p in ("H", "Lgain", "Y"):
        assert _call(name, **{p: None}) == (INV, name + ": null H, Lgain or Y")


@pytest.mark.parametrize("name", SWEEPS)
def test_a_valid_sweep_reaches_the_null_handle(name):
    given, outs, gain, score = _roles(name)
    assert _call(name, **{gain: None}) == NH  # with the score, at fixed gains
    assert _call(name, **_none(name, *score)) == NH  # with the gains, without the score
    for keep in given:  # one tangent or cotangent is enough, whichever goes with the rest
        drop = _none(name, *(g for g in given if g != keep))
        drop.update({gain: None} if keep in score or keep != gain else _none(name, *score))
        assert _call(name, **drop) == NH, keep
    for keep in outs:
        if keep in PARAMS[name]:
            drop = _none(name, *(o for o in outs if o != keep))
            drop.update({gain: None} if keep != gain else _none(name, *score))
            assert _call(name, **drop) == NH, keep
    # innov and Vdiag are required, and Vdiag looked at, only where they are read
    assert _call(name, innov=None, Vdiag=None, **{gain: None}, **_none(name, *score)) == NH
    assert _call(name, Vdiag=(0, -1.0), **_none(name, *score)) == NH
    assert _call(name, model=None, **{gain: None}) == NH
    for p in ("Zref", "Zrec", "Xhat"):  # looked at behind the handle
        assert _call(name, **{p: None, gain: None}) == NH


@pytest.mark.parametrize("name", SWEEPS)
def test_each_refusal_of_a_sweep_gives_its_code_and_text(name):
    given, outs, gain, score = _roles(name)
    fwd = "jvp" in name
    ok = {gain: None}
    for ny in (0, 9, -1):
        assert _call(name, ny=ny, **ok) == (INV, name + ": ny must be in [1, 8]")
    text = ": every tangent is NULL (no direction)" if fwd else ": every cotangent is NULL (nothing to pull back)"
    assert _call(name, **_none(name, *given), **({} if fwd else ok)) == (INV, name + text)
    assert _call(name, **_none(name, *outs), **({} if not fwd else ok)) == (INV, name + ": every output is NULL (nothing to compute)")
    for term in score:
        other = [s for s in score if s != term][0]
        code, msg = _call(name, **{other: None})
        assert code == INV and "the score is differentiated at fixed gains" in msg and msg.startswith(name + ": " + gain)
        assert _call(name, Vdiag=None, **{other: None}, **ok) == (INV, name + ": null Vdiag with a score term")
        for value in (0.0, -1.0, float("nan"), float("inf")):
            assert _call(name, Vdiag=(1, value), **{other: None}, **ok) == (INV, name + ": Vdiag must be finite and > 0 (entry 1)")
        assert _call(name, innov=None, **{other: None}, **ok)[1].startswith(name + ": null innov")
    assert _call(name, Vdiag=(2, 0.0), **ok) == NH  # behind ny: not read
    assert _call(name, innov=None, **_none(name, *score))[1].startswith(name + ": null innov")
    if "guarded" in name:
        assert _call(name, event_hat=None, **ok) == (INV, name + ": null event_hat (the guarded filter's record)")
    for p in ("H", "Lgain"):
        assert _call(name, **{p: None}, **ok) == (INV, name + ": null H or Lgain")


@pytest.mark.parametrize("name", SWEEPS)
def test_the_refusals_of_a_sweep_keep_the_familys_order(name):
    given, outs, gain, score = _roles(name)
    fwd = "jvp" in name
    first, second = given, outs
    ladder = [({"ny": 9}, "ny must be"), (_none(name, *first), "every tangent is NULL" if fwd else "every cotangent is NULL"),
              (_none(name, *second), "every output is NULL"),
              ({}, "at fixed gains"), ({"Vdiag": None}, "null Vdiag"), ({"Vdiag": (0, 0.0)}, "Vdiag must be"),
              ({"innov": None}, "null innov")]
    if "guarded" in name:
        ladder.append(({"event_hat": None}, "null event_hat"))
    ladder += [({"H": None}, "null H or Lgain"), ({"Zrec": None}, "null handle")]
    for i in range(len(ladder)):
        change = {}
        for c, _ in reversed(ladder[i:]):
            change.update(c)
        # the later rungs need a tangent (cotangent) and an output; behind rung 3 the gains' own are left out
        for p in (first if i >= 2 else ()) + (second if i >= 3 else ()):
            change.pop(p, None)
        if i >= 4:
            change[gain] = None
        code, text = _call(name, **change)
        assert code == INV and ladder[i][1] in text, (i, text)
