"""Records ilqr_ref_bits.npz: the controls, multipliers and report of tests/ilqr_ref.py for the ONE and TWELVE cases of
N12-kt5 and N17-ragged in float64 and in 80-bit longdouble.  The committed file was written by the restatement as it stood
BEFORE the rescue phase was added to it; tests/test_ilqr_ref_host.py holds the restatement with rescue_outer = 0 to these
bits.  A longdouble is stored as two float64 (hi = the value rounded to double, lo = the rest, exact: 64 bits of mantissa
fit 53 + 53).  Run from the repository root:  python -m tests.golden.make_ilqr_ref_bits"""
import os

import numpy as np

from tests import ilqr_cases as IC
from tests import ilqr_ref as IR

CASES = [("N12-kt5", "ONE"), ("N12-kt5", "TWELVE"), ("N17-ragged", "ONE"), ("N17-ragged", "TWELVE")]


def split(a):
    """longdouble array -> (hi, lo) float64 arrays with hi + lo == a exactly"""
    a = np.asarray(a, dtype=np.longdouble)
    hi = a.astype(np.float64)
    lo = (a - hi.astype(np.longdouble)).astype(np.float64)
    assert np.array_equal(hi.astype(np.longdouble) + lo.astype(np.longdouble), a)
    return np.stack([hi, lo])


def record(name, which):
    """{key: array} of one case"""
    batch = IC.shape(name)
    o = getattr(IC, which)
    P, U0 = IC.problems(batch)
    out = {}
    for b in range(batch.B):
        r64, r80 = IC.reference_pair(P[b], U0[b], o, keep_trials=False)
        key = f"{name}/{which}/{b}"
        out[key + "/U64"], out[key + "/lam64"], out[key + "/leq64"] = r64.U, r64.lam, r64.leq
        out[key + "/U80"], out[key + "/lam80"], out[key + "/leq80"] = split(r80.U), split(r80.lam), split(r80.leq)
        out[key + "/info64"], out[key + "/info80"] = r64.info(), r80.info()
        out[key + "/viol"] = np.array([r64.viol, r80.viol])
    return out


if __name__ == "__main__":
    IR.require_extended_precision()
    arrays = {}
    for name, which in CASES:
        arrays.update(record(name, which))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ilqr_ref_bits.npz"), **arrays)
    print(len(arrays), "arrays")
