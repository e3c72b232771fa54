"""The refusals of qln_landing_smoother and its three siblings that need no device: each is called with a null handle, so the
latest refusal a call can reach is "null handle" and nothing touches a device.  Every refusal gives QLN_ERR_INVALID_ARGUMENT and
its text, and the checks that need no handle come before the null handle, in the family's order: ny, the outputs, the guarded
form's event, H and Vdiag, V's entries, the other inputs."""
import ctypes as C

import pytest

from quadruped_landing_amd import _lib

PARAMS = {
    "qln_landing_smoother": ("Ztraj", "Lgain", "Pest", "H", "ny", "Vdiag", "Xhat", "innov", "Xs", "Ps"),
    "qln_landing_smoother_guarded": ("Ztraj", "model", "event", "Lgain", "Pest", "H", "ny", "Vdiag", "Xhat", "innov", "Xs", "Ps"),
}
PARAMS.update({k + "_host": v for k, v in list(PARAMS.items())})
NAMES = sorted(PARAMS)


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


def test_the_symbols_are_declared_and_outside_the_tracking_prefix():
    assert all(n in _lib.SIGNATURES and not n.startswith("qln_tracking_") for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_a_valid_call_reaches_the_null_handle(name):
    assert _call(name) == (_lib.QLN_ERR_INVALID_ARGUMENT, "null handle")
    assert _call(name, Xs=None) == (_lib.QLN_ERR_INVALID_ARGUMENT, "null handle")  # one output is enough
    assert _call(name, Ps=None) == (_lib.QLN_ERR_INVALID_ARGUMENT, "null handle")
    if "model" in PARAMS[name]:
        assert _call(name, model=None) == (_lib.QLN_ERR_INVALID_ARGUMENT, "null handle")  # optional
    assert _call(name, Ztraj=None) == (_lib.QLN_ERR_INVALID_ARGUMENT, "null handle")  # looked at behind the handle


@pytest.mark.parametrize("name", NAMES)
def test_each_refusal_gives_its_code_and_text(name):
    INV = _lib.QLN_ERR_INVALID_ARGUMENT
    for ny in (0, 9, -1):
        assert _call(name, ny=ny) == (INV, name + ": ny must be in [1, 8]")
    assert _call(name, Xs=None, Ps=None) == (INV, name + ": Xs and Ps are both NULL (nothing to compute)")
    for p in ("H", "Vdiag"):
        assert _call(name, **{p: None}) == (INV, name + ": null H or Vdiag")
    for value in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(name, Vdiag=(1, value)) == (INV, name + ": Vdiag must be finite and > 0 (entry 1)")
    assert _call(name, Vdiag=(2, 0.0)) == (INV, "null handle")  # behind ny: not read
    for p in ("Lgain", "Pest"):
        assert _call(name, **{p: None}) == (INV, name + ": null Lgain or Pest")
    for p in ("Xhat", "innov"):
        assert _call(name, **{p: None}) == (INV, name + ": null Xhat or innov")
    if "event" in PARAMS[name]:
        assert _call(name, event=None) == (INV, name + ": null event (the guarded roll-out's records)")


@pytest.mark.parametrize("name", NAMES)
def test_the_refusals_keep_the_familys_order(name):
    """ny, then the outputs, then event, then H and Vdiag, then V's entries, then the other inputs, then the handle"""
    INV = _lib.QLN_ERR_INVALID_ARGUMENT
    guarded = "event" in PARAMS[name]
    ladder = [({"ny": 9}, "ny must be"), ({"Xs": None, "Ps": None}, "both NULL")]
    if guarded:
        ladder.append(({"event": None}, "null event"))
    ladder += [({"H": None}, "null H or Vdiag"), ({"Vdiag": (0, 0.0)}, "Vdiag must be"), ({"Lgain": None}, "null Lgain or Pest"),
               ({"innov": None}, "null Xhat or innov"), ({"Ztraj": None}, "null handle")]
    for i in range(len(ladder)):
        change = {}
        for c, _ in ladder[i:]:
            change.update(c)
        code, text = _call(name, **change)
        assert code == INV and ladder[i][1] in text, (i, text)
