"""The refusals of qln_landing_filter and its three siblings that need no device: each is called with a null handle, so the
latest refusal a call can reach is "null handle" and nothing touches a device.  Every refusal gives QLN_ERR_INVALID_ARGUMENT and
its text, and the checks that need no handle come before the null handle, in the family's order: ny, the outputs, Vdiag missing
when a score is asked for, V's entries, then H, Lgain and Y."""
import ctypes as C

import pytest

from quadruped_landing_amd import _lib

PARAMS = {
    "qln_landing_filter": ("Zref", "Zrec", "Lgain", "H", "ny", "Vdiag", "Y", "xhat0", "Xhat", "innov", "score", "loglik"),
    "qln_landing_filter_guarded": ("Zref", "Zrec", "Lgain", "H", "ny", "Vdiag", "Y", "xhat0", "Xhat", "innov", "score", "loglik",
                                   "event_hat"),
}
PARAMS.update({k + "_host": v for k, v in list(PARAMS.items())})
NAMES = sorted(PARAMS)
OUTPUTS = ("Xhat", "innov", "score", "loglik", "event_hat")


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


def test_the_symbols_are_declared_and_outside_the_tracking_prefix():
    assert all(n in _lib.SIGNATURES and not n.startswith("qln_tracking_") for n in NAMES)
    for n in NAMES:
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and len(args) == len(PARAMS[n]) + 1
        assert [i for i, a in enumerate(args) if a is C.c_int32] == [5]


@pytest.mark.parametrize("name", NAMES)
def test_a_valid_call_reaches_the_null_handle(name):
    NH = (_lib.QLN_ERR_INVALID_ARGUMENT, "null handle")
    assert _call(name) == NH
    for keep in OUTPUTS:  # one output is enough, whichever
        if keep in PARAMS[name]:
            assert _call(name, **_none(name, *(o for o in OUTPUTS if o != keep))) == NH
    assert _call(name, xhat0=None) == NH  # optional
    # Vdiag is required, and looked at, only with score or loglik
    assert _call(name, Vdiag=None, score=None, loglik=None) == NH
    assert _call(name, Vdiag=(0, -1.0), score=None, loglik=None) == NH
    assert _call(name, Zref=None) == NH and _call(name, Zrec=None) == NH  # looked at behind the handle


@pytest.mark.parametrize("name", NAMES)
def test_each_refusal_gives_its_code_and_text(name):
    INV = _lib.QLN_ERR_INVALID_ARGUMENT
    for ny in (0, 9, -1):
        assert _call(name, ny=ny) == (INV, name + ": ny must be in [1, 8]")
    assert _call(name, **_none(name, *OUTPUTS)) == (INV, name + ": every output is NULL (nothing to compute)")
    for asked in ("score", "loglik"):
        other = "loglik" if asked == "score" else "score"
        assert _call(name, Vdiag=None, **{other: None}) == (INV, name + ": null Vdiag with score or loglik")
        for value in (0.0, -1.0, float("nan"), float("inf")):
            assert _call(name, Vdiag=(1, value), **{other: None}) == (INV, name + ": Vdiag must be finite and > 0 (entry 1)")
    assert _call(name, Vdiag=(2, 0.0)) == (INV, "null handle")  # behind ny: not read
    for p in ("H", "Lgain", "Y"):
        assert _call(name, **{p: None}) == (INV, name + ": null H, Lgain or Y")


@pytest.mark.parametrize("name", NAMES)
def test_the_refusals_keep_the_familys_order(name):
    """ny, then the outputs, then a missing Vdiag, then V's entries, then H, Lgain and Y, then the handle"""
    INV = _lib.QLN_ERR_INVALID_ARGUMENT
    ladder = [({"ny": 9}, "ny must be"), (_none(name, *OUTPUTS), "every output is NULL"), ({"Vdiag": None}, "null Vdiag"),
              ({"Vdiag": (0, 0.0)}, "Vdiag must be"), ({"Y": None}, "null H, Lgain or Y"), ({"Zrec": None}, "null handle")]
    for i in range(len(ladder)):
        change = {}
        for c, _ in reversed(ladder[i:]):
            change.update(c)
        if i >= 2:  # the ladder's later rungs need an output, and the score's rungs need the score
            for o in OUTPUTS:
                change.pop(o, None)
        code, text = _call(name, **change)
        assert code == INV and ladder[i][1] in text, (i, text)
