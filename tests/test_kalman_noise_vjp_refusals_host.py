"""The refusals of qln_noise_design_vjp and its three siblings that need no device: each is called with a null handle, so the
latest refusal a call can reach is "null handle" and nothing touches a device.  Every refusal gives QLN_ERR_INVALID_ARGUMENT and
its text, and the checks that need no handle come before the null handle, in qln_kalman_design_jvp's order: ny, the outputs, the
guarded form's event, H and Vdiag, V's entries, the cotangents, Lgain.  What needs the handle -- a NULL Zout, overlaps, and the
host forms' look at H, model and event -- is tests/test_gpu_tracking_kalman_vjp.py's."""
import ctypes as C

import pytest

from quadruped_landing_amd import _lib
from tests.tracking_abi import FAMILIES, parameter_names

PLAIN = ("Zout", "Lgain", "H", "ny", "Vdiag", "Lgain_bar", "Pest_bar", "logdet_bar", "Sigma0_bar", "Wdiag_bar", "Vdiag_bar")
PARAMS = {"qln_noise_design_vjp": PLAIN, "qln_noise_design_guarded_vjp": PLAIN[:1] + ("model", "event") + PLAIN[1:]}
PARAMS.update({k + "_host": v for k, v in list(PARAMS.items())})
NAMES = sorted(PARAMS)
COT = ("Lgain_bar", "Pest_bar", "logdet_bar")
OUT = ("Sigma0_bar", "Wdiag_bar", "Vdiag_bar")
INV = _lib.QLN_ERR_INVALID_ARGUMENT
NULL_HANDLE = (INV, "null handle")


def _call(name, **change):
    """The symbol with a null handle, every pointer at its own buffer of ones and ny = 2; change: None, an int, or
    (index, value)"""
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


def test_the_symbols_are_declared_with_the_headers_parameters_and_outside_the_pinned_prefixes():
    declared = parameter_names(("noise_design",))
    assert sorted(declared) == NAMES
    for n in NAMES:
        assert n in _lib.SIGNATURES and not n.startswith(tuple("qln_%s_" % f for f in FAMILIES + ("kalman",)))
        assert tuple(declared[n]) == PARAMS[n]
        ints = [i for i, t in enumerate(_lib.SIGNATURES[n][1][1:]) if t is C.c_int32]
        assert [PARAMS[n][i] for i in ints] == ["ny"]
        assert getattr(_lib.lib(), n).argtypes == _lib.SIGNATURES[n][1]


@pytest.mark.parametrize("name", NAMES)
def test_a_valid_call_reaches_the_null_handle(name):
    assert _call(name) == NULL_HANDLE
    for keep in OUT:  # one output is enough
        assert _call(name, **{o: None for o in OUT if o != keep}) == NULL_HANDLE
    for keep in COT:  # one cotangent is enough
        assert _call(name, **{o: None for o in COT if o != keep}) == NULL_HANDLE
    if "model" in PARAMS[name]:
        assert _call(name, model=None) == NULL_HANDLE  # optional
    assert _call(name, Zout=None) == NULL_HANDLE  # looked at behind the handle
    for value in (-3.0, 0.0, float("nan")):  # the cotangents are device data in the device forms: not looked at
        assert _call(name, logdet_bar=(1, value), Pest_bar=(3, value)) == NULL_HANDLE


@pytest.mark.parametrize("name", NAMES)
def test_each_refusal_gives_its_code_and_text(name):
    for ny in (0, 9, -1):
        assert _call(name, ny=ny) == (INV, name + ": ny must be in [1, 8]")
    assert _call(name, **{o: None for o in OUT}) == (INV, name + ": every output is NULL (nothing to compute)")
    for p in ("H", "Vdiag"):
        assert _call(name, **{p: None}) == (INV, name + ": null H or Vdiag")
    for value in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(name, Vdiag=(1, value)) == (INV, name + ": Vdiag must be finite and > 0 (entry 1)")
    assert _call(name, Vdiag=(2, 0.0)) == NULL_HANDLE  # behind ny: not read
    assert _call(name, **{c: None for c in COT}) == (INV, name + ": Lgain_bar, Pest_bar and logdet_bar are all NULL (no cotangent)")
    assert _call(name, Lgain=None) == (INV, name + ": null Lgain")
    if "event" in PARAMS[name]:
        assert _call(name, event=None) == (INV, name + ": null event (the guarded roll-out's records)")


@pytest.mark.parametrize("name", NAMES)
def test_the_refusals_keep_the_forward_sweeps_order(name):
    guarded = "event" in PARAMS[name]
    ladder = [({"ny": 9}, "ny must be"), ({o: None for o in OUT}, "every output is NULL")]
    if guarded:
        ladder.append(({"event": None}, "null event"))
    ladder += [({"H": None}, "null H or Vdiag"), ({"Vdiag": (0, 0.0)}, "Vdiag must be"), ({c: None for c in COT}, "no cotangent"),
               ({"Lgain": None}, "null Lgain"), ({"Zout": None}, "null handle")]
    for i in range(len(ladder)):
        change = {}
        for c, _ in ladder[i:]:
            change.update(c)
        code, text = _call(name, **change)
        assert code == INV and ladder[i][1] in text, (i, text)
