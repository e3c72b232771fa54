"""Every qln_tracking_*, qln_landing_* and qln_kalman_design_* entry point keeps the code, the text and the precedence of its
refusals that need no device.

Each of the 80 symbols of _lib.SIGNATURES is called with a null handle: the latest refusal such a call can reach is
"null handle", so nothing touches a device.  The base call points every pointer argument at its own buffer of ones (valid
weights, {lo, hi} pairs, Vdiag and H) with ny = 2, sigma0_batch = 1 and guarded = 1; the variations break one thing at a
time.  The landing and Kalman-design symbols are also called with every output left out, with every tangent or cotangent
left out, and once more through every variation without each group of optional arguments that switches a check off (the
gains' tangent, the score terms, Sigma0_dot): with all of them given, the filter sweeps are refused at their first check.
The expected (code, qln_last_error()) of every call is tests/golden/tracking_refusals.json, recorded by

    python -m tests.test_tracking_refusals_host --record <commit>

against a build of that commit; the file names the commit it was recorded at."""
import ctypes as C
import json
import os
import sys

import pytest

from quadruped_landing_amd import _lib
from tests.tracking_abi import OUTPUTS, PARAMS, ROOT, SYMBOLS

GOLDEN = os.path.join(ROOT, "tests", "golden", "tracking_refusals.json")
ONES = 64  # doubles per buffer: more than any check reads before it asks for the handle (15 weights, 8 limits, 8 Vdiag)
INTS = {"ny": 2, "sigma0_batch": 1, "guarded": 1}
NEGATIVE = ("Qdiag", "Qfdiag", "Wdiag")  # must be >= 0
ZERO = ("Rdiag", "Vdiag")  # must be > 0
FINITE = ("Wdiag_dot", "Vdiag_dot")  # must be finite
# optional arguments of the landing and Kalman-design symbols that, given together, switch a check on
GROUPS = (("Lgain_dot",), ("Lgain_bar",), ("score", "loglik"), ("nis_dot", "loglik_dot"), ("nis_bar", "loglik_bar"),
          ("Lgain_dot", "nis_dot", "loglik_dot"), ("Lgain_bar", "nis_bar", "loglik_bar"), ("Sigma0_dot",))


def _one_at_a_time(name):
    """(label, {parameter: replacement}) of every call of one symbol; a replacement is None, an int, or (index, value)"""
    types = _lib.SIGNATURES[name][1][1:]
    names = PARAMS[name]
    assert len(names) == len(types), name
    yield "base", {}
    for p, t in zip(names, types):
        if t is not C.c_int32:
            yield "null " + p, {p: None}
    if "ny" in names:
        yield "ny = 0", {"ny": 0}
        yield "ny = 9", {"ny": 9}
    if "sigma0_batch" in names:
        yield "sigma0_batch = 0", {"sigma0_batch": 0}
    if "guarded" in names:
        yield "guarded = 0 with event", {"guarded": 0}
    if "lim" in names:
        yield "NaN in lim", {"lim": (2, float("nan"))}
        yield "lo > hi in lim", {"lim": (2, 2.0)}
    for p in NEGATIVE:
        if p in names:
            yield "negative " + p, {p: (1, -1.0)}
    for p in ZERO:
        if p in names:
            yield "zero " + p, {p: (1, 0.0)}
    for p in FINITE:
        if p in names:
            yield "NaN in " + p, {p: (1, float("nan"))}


def _variations(name):
    """the calls of one symbol; the qln_tracking_* ones are called as they always were"""
    yield from _one_at_a_time(name)
    if name.startswith("qln_tracking_"):
        return
    names = PARAMS[name]
    yield "every output null", {p: None for p in OUTPUTS[name]}
    given = [p for p in names if p.endswith(("_dot", "_bar")) and p not in OUTPUTS[name]]
    if given:
        yield "every tangent or cotangent null", {p: None for p in given}
    for group in GROUPS:
        if all(p in names for p in group):
            for label, change in _one_at_a_time(name):
                yield "without %s: %s" % (", ".join(group), label), {**change, **{p: None for p in group}}


def _call(L, name, change):
    types = _lib.SIGNATURES[name][1][1:]
    keep, args = [], [None]  # the null handle
    for p, t in zip(PARAMS[name], types):
        if t is C.c_int32:
            args.append(change.get(p, INTS[p]))
            continue
        buf = (C.c_double * ONES)(*([1.0] * ONES))
        keep.append(buf)
        if p in change and change[p] is None:
            args.append(None)
            continue
        if p in change:
            buf[change[p][0]] = change[p][1]
        args.append(C.cast(buf, C.POINTER(C.c_double)))
    code = getattr(L, name)(*args)
    return [int(code), L.qln_last_error().decode()]


def _observe(L, name):
    return {label: _call(L, name, change) for label, change in _variations(name)}


def test_every_tracking_symbol_is_covered():
    assert len(SYMBOLS) == 80
    assert sorted(PARAMS) == SYMBOLS
    assert sorted(json.load(open(GOLDEN))["refusals"]) == SYMBOLS


@pytest.mark.parametrize("name", SYMBOLS)
def test_refusals_without_a_device(name):
    want = json.load(open(GOLDEN))["refusals"][name]
    got = _observe(_lib.lib(), name)
    assert sorted(got) == sorted(want)
    for label in want:
        assert got[label][0] != _lib.QLN_OK, (name, label)
        assert got[label] == want[label], (name, label)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    L = _lib.lib()
    doc = {"recorded_at": sys.argv[2], "refusals": {name: _observe(L, name) for name in SYMBOLS}}
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(SYMBOLS), "symbols,", sum(len(v) for v in doc["refusals"].values()), "calls ->", GOLDEN)
