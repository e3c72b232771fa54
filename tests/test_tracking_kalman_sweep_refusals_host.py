"""The refusals of qln_kalman_design_jvp and its three siblings that need no device: each is called with a null handle, so the
latest refusal a call can reach is "null handle" and nothing touches a device.  Every refusal gives QLN_ERR_INVALID_ARGUMENT and
its text, and the checks that need no handle come before the null handle, in the family's order: ny, the outputs, the guarded
form's event, H and Vdiag, V's entries, the direction, its entries, Lgain, sigma0_batch.  What needs the handle -- sigma0_batch
against B, a NULL Zout, overlaps, and the host forms' look at H, model and event -- is tests/test_gpu_tracking_kalman_sweep.py's."""
import ctypes as C

import pytest

from quadruped_landing_amd import _lib
from tests.tracking_abi import parameter_names

PLAIN = ("Zout", "Lgain", "H", "ny", "Vdiag", "Sigma0_dot", "sigma0_batch", "Wdiag_dot", "Vdiag_dot", "Lgain_dot", "Pest_dot",
         "logdet_dot")
PARAMS = {"qln_kalman_design_jvp": PLAIN, "qln_kalman_design_guarded_jvp": PLAIN[:1] + ("model", "event") + PLAIN[1:]}
PARAMS.update({k + "_host": v for k, v in list(PARAMS.items())})
NAMES = sorted(PARAMS)
INTS = {"ny": 2, "sigma0_batch": 1}
INV = _lib.QLN_ERR_INVALID_ARGUMENT
NULL_HANDLE = (INV, "null handle")


def _call(name, **change):
    """The symbol with a null handle, every pointer at its own buffer of ones, ny = 2 and sigma0_batch = 1; change: None, an
    int, or (index, value)"""
    types = _lib.SIGNATURES[name][1][1:]
    assert len(types) == len(PARAMS[name])
    keep, args = [], [None]
    for p, t in zip(PARAMS[name], types):
        if t is C.c_int32:
            args.append(change.get(p, INTS[p]))
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


def test_the_symbols_are_declared_with_the_headers_parameters_and_outside_the_tracking_prefix():
    declared = parameter_names(("kalman",))
    assert sorted(declared) == NAMES
    for n in NAMES:
        assert n in _lib.SIGNATURES and not n.startswith("qln_tracking_")
        assert tuple(declared[n]) == PARAMS[n]
        ints = [i for i, t in enumerate(_lib.SIGNATURES[n][1][1:]) if t is C.c_int32]
        assert [PARAMS[n][i] for i in ints] == ["ny", "sigma0_batch"]
        assert getattr(_lib.lib(), n).argtypes == _lib.SIGNATURES[n][1]


@pytest.mark.parametrize("name", NAMES)
def test_a_valid_call_reaches_the_null_handle(name):
    assert _call(name) == NULL_HANDLE
    for keep in ("Lgain_dot", "Pest_dot", "logdet_dot"):  # one output is enough
        assert _call(name, **{o: None for o in ("Lgain_dot", "Pest_dot", "logdet_dot") if o != keep}) == NULL_HANDLE
    for keep in ("Sigma0_dot", "Wdiag_dot", "Vdiag_dot"):  # one tangent is enough
        assert _call(name, **{o: None for o in ("Sigma0_dot", "Wdiag_dot", "Vdiag_dot") if o != keep}) == NULL_HANDLE
    if "model" in PARAMS[name]:
        assert _call(name, model=None) == NULL_HANDLE  # optional
    assert _call(name, Zout=None) == NULL_HANDLE  # looked at behind the handle
    assert _call(name, sigma0_batch=7) == NULL_HANDLE  # against B: behind the handle
    assert _call(name, Sigma0_dot=None, sigma0_batch=0) == NULL_HANDLE  # not read without Sigma0_dot
    for value in (-3.0, 0.0):  # the tangents are signed
        assert _call(name, Wdiag_dot=(3, value), Vdiag_dot=(1, value)) == NULL_HANDLE


@pytest.mark.parametrize("name", NAMES)
def test_each_refusal_gives_its_code_and_text(name):
    for ny in (0, 9, -1):
        assert _call(name, ny=ny) == (INV, name + ": ny must be in [1, 8]")
    assert _call(name, Lgain_dot=None, Pest_dot=None, logdet_dot=None) == (INV, name + ": every output is NULL (nothing to compute)")
    for p in ("H", "Vdiag"):
        assert _call(name, **{p: None}) == (INV, name + ": null H or Vdiag")
    for value in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(name, Vdiag=(1, value)) == (INV, name + ": Vdiag must be finite and > 0 (entry 1)")
    assert _call(name, Vdiag=(2, 0.0)) == NULL_HANDLE  # behind ny: not read
    assert _call(name, Sigma0_dot=None, Wdiag_dot=None, Vdiag_dot=None) == (
        INV, name + ": Sigma0_dot, Wdiag_dot and Vdiag_dot are all NULL (no direction)")
    for value in (float("nan"), float("inf"), -float("inf")):
        assert _call(name, Wdiag_dot=(14, value)) == (INV, name + ": Wdiag_dot must be finite (entry 14)")
        assert _call(name, Vdiag_dot=(1, value)) == (INV, name + ": Vdiag_dot must be finite (entry 1)")
        assert _call(name, Vdiag_dot=(2, value)) == NULL_HANDLE  # behind ny: not read, and cannot be expressed
    assert _call(name, Lgain=None) == (INV, name + ": null Lgain")
    for nb in (0, -1):
        assert _call(name, sigma0_batch=nb) == (INV, name + ": sigma0_batch must be 1 or B")
    if "event" in PARAMS[name]:
        assert _call(name, event=None) == (INV, name + ": null event (the guarded roll-out's records)")


@pytest.mark.parametrize("name", NAMES)
def test_the_refusals_keep_the_familys_order(name):
    guarded = "event" in PARAMS[name]
    ladder = [({"ny": 9}, "ny must be"), ({"Lgain_dot": None, "Pest_dot": None, "logdet_dot": None}, "every output is NULL")]
    if guarded:
        ladder.append(({"event": None}, "null event"))
    ladder += [({"H": None}, "null H or Vdiag"), ({"Vdiag": (0, 0.0)}, "Vdiag must be"),
               ({"Wdiag_dot": (0, float("nan"))}, "Wdiag_dot must be"), ({"Vdiag_dot": (0, float("nan"))}, "Vdiag_dot must be"),
               ({"Lgain": None}, "null Lgain"), ({"sigma0_batch": 0}, "sigma0_batch"), ({"Zout": None}, "null handle")]
    for i in range(len(ladder)):
        change = {}
        for c, _ in ladder[i:]:
            change.update(c)
        code, text = _call(name, **change)
        assert code == INV and ladder[i][1] in text, (i, text)
