"""What the tests that call the qln_tracking_*, qln_landing_* and qln_kalman_design_* entry points through ctypes share: the
parameter names of every prototype of include/qln_evaluator.h, which of them are outputs, which are host arrays in both
memory forms, and the size of every buffer by its parameter's name.  Not a test module."""
import ctypes as C
import os
import re

import numpy as np

from quadruped_landing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("tracking", "landing", "kalman_design")
SYMBOLS = sorted(n for n in _lib.SIGNATURES if n.startswith(tuple("qln_%s_" % f for f in FAMILIES)))
# host arrays in the device forms too
HOST_ONLY = {"Qdiag": 15, "Qfdiag": 15, "Rdiag": 4, "Wdiag": 15, "Vdiag": 8, "lim": 8, "Wdiag_dot": 15, "Vdiag_dot": 8}


def _prototypes(families):
    """(name, its parameter declarations with the handle left out) of every prototype of the families in the header"""
    src = open(os.path.join(ROOT, "include", "qln_evaluator.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, params in re.findall(r"\bint\s+(qln_(?:%s)_[a-z_]+)\s*\(([^)]*)\)\s*;" % "|".join(families), src):
        yield name, [p.strip() for p in params.split(",")][1:]


def parameter_names(families=("tracking",)):
    """name -> the parameter names of its prototype in the header, the handle left out; families: of qln_tracking_*,
    qln_landing_* and qln_kalman_design_*, the ones to read"""
    return {name: [re.search(r"(\w+)\s*$", p).group(1) for p in params] for name, params in _prototypes(families)}


def output_names(families=FAMILIES):
    """name -> the parameters its prototype declares double* without const: the outputs and the in-outs"""
    return {name: [re.search(r"(\w+)\s*$", p).group(1) for p in params if re.match(r"double\s*\*", p)]
            for name, params in _prototypes(families)}


PARAMS = parameter_names(FAMILIES)
OUTPUTS = output_names()


def is_int(name, p):
    return _lib.SIGNATURES[name][1][1 + PARAMS[name].index(p)] is C.c_int32


def size(p, B, N, z_total):
    """doubles behind the parameter p of a handle with B problems of N knots, at the largest ny"""
    if p in HOST_ONLY:
        return HOST_ONLY[p]
    if p.startswith("Z"):  # Zref, Zout, Ztraj, Zrec and their tangents and cotangents
        return z_total
    if p in ("K", "K_bar", "K_dot"):
        return B * (N - 1) * 60
    if p.startswith(("x0", "xhat0")):
        return B * 15
    if p.startswith("model"):
        return B * 4
    if p == "event_var":
        return B * 2
    if p.startswith("event"):
        return B * 8
    if p == "sat":
        return B * (N - 1)
    if p in ("P", "Pest", "Pest_dot", "Ps", "Sigma"):
        return B * N * 120
    if p in ("Sigma0", "Sigma0_dot"):
        return B * 120
    if p == "H":
        return 8 * 15
    if p.startswith("Lgain"):
        return B * N * 15 * 8
    if p == "wnoise":
        return B * (N - 1) * 15
    if p == "Xs" or p.startswith("Xhat"):
        return B * N * 15
    if p in ("marg", "vnoise") or p.startswith(("innov", "Y")):
        return B * N * 8
    if p == "score":
        return B * N * 2
    if p == "logdet_dot" or p.startswith("nis"):
        return B * N
    if p.startswith("loglik"):
        return B
    raise KeyError(p)


def address(a):
    """The raw address of a numpy array or a torch tensor (None stays None)."""
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def call(h, name, values):
    """Calls the entry point with values[p] for every parameter p: an int, None, a numpy array or a torch tensor."""
    args = [values[p] if is_int(name, p) else address(values[p]) for p in PARAMS[name]]
    return getattr(_lib.lib(), name)(h, *args)
