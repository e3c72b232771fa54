"""Time per CGLS iteration of qln_estimate_multipliers against qln_gauss_newton_step's, in one run on the same point:
100 forced iterations of each (rel_tol = 0, so no problem stops early) at N = 40, B = 1 024 and B = 65 536, HIP events,
median of 5 launches after 2 warm-ups.  Both kernels run one wave per problem with everything in LDS and apply the same
two products once per iteration; the estimate also scales by 1/w twice per iteration (m-vectors) and keeps four n-vectors
in LDS where the step keeps five.  The per-iteration figure is the launch time over 100 and so includes the prologue (the
loads, the row norms) and, for the estimate, the epilogue (one more transposed product, the second read of g).
Also reports the second figure that separates the two: the same launches with 200 iterations, so that
(t200 - t100) / 100 is the cost of an iteration alone.  Prints one JSON line.
N = 40 keeps every knot's step block in registers; --N above 64 (the tests use 80) times the variants that re-derive it.
   python bench/multiplier_timing.py [--N N] [B ...]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, _lib, problem_gen as PG  # noqa: E402


def t_ms(fn, iters=5, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def run(B, N=40, k_trans=14):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Z = nlp.upload_Z(batch.Z)
    c, g = nlp.eval_c(Z), nlp.grad_f(Z)
    lam, lag, dZ = nlp.new_c(), nlp.new_Z(), nlp.new_Z()
    minfo = torch.zeros(B * _lib.MULT_INFO_STRIDE, dtype=torch.float64, device="cuda")
    ginfo = torch.zeros(B * _lib.GN_INFO_STRIDE, dtype=torch.float64, device="cuda")
    out = {"B": B, "N": N, "k_trans": k_trans}
    for iters in (100, 200):
        for scaled in (True, False):
            ms = t_ms(lambda: nlp.estimate_multipliers(Z, c, g, max_iters=iters, rel_tol=0.0, row_scaling=scaled, lam=lam, lag=lag,
                                                       info=minfo))
            done = minfo.view(B, -1)[:, 0]
            assert bool((done == iters).all()), "a problem stopped early: the per-iteration figure would be wrong"
            out[f"multipliers_{'scaled' if scaled else 'plain'}_{iters}_ms"] = round(ms, 4)
        ms = t_ms(lambda: nlp.gauss_newton_step(Z, c, out=dZ, max_iters=iters, rel_tol=0.0, info=ginfo))
        assert bool((ginfo.view(B, -1)[:, 0] == iters).all())
        out[f"gauss_newton_{iters}_ms"] = round(ms, 4)
    for k in ("multipliers_scaled", "multipliers_plain", "gauss_newton"):
        out[f"{k}_us_per_iteration"] = round(10.0 * out[f"{k}_100_ms"], 3)
        out[f"{k}_us_per_iteration_marginal"] = round(10.0 * (out[f"{k}_200_ms"] - out[f"{k}_100_ms"]), 3)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--N", type=int, default=40, help="knots per problem (above 64: the variants that re-derive the step blocks)")
    ap.add_argument("B", type=int, nargs="*", default=[1024, 65536], help="batch sizes")
    args = ap.parse_args()
    print(json.dumps({"kernel": "qln_estimate_multipliers vs qln_gauss_newton_step", "launches": 5, "warmup": 2,
                      "results": [run(B, args.N) for B in args.B]}))
