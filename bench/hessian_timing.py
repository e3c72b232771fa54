"""Launch time of qln_eval_hessian_lagrangian (HIP events, median of 20 launches after 3 warm-ups) at BASELINE.json
configs[2] (B = 65 536, N = 40, shared cost table) and at N = 61 (the notebook's horizon), against the kernel's own
compulsory bytes: Z, the dynamics and clearance multipliers, sigma, the cost table (once if shared) and the values.
Prints one JSON line.
   python bench/hessian_timing.py [B]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

PEAK = 8.0e12  # B/s, MI355X HBM spec


def t_ms(fn, iters=20, warmup=3):
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


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf, exact_hessian=True)
    Z = nlp.upload_Z(batch.Z)
    sigma = torch.rand(B, dtype=torch.float64, device="cuda")
    mu = torch.randn(nlp.dims.c_total, dtype=torch.float64, device="cuda")
    out = nlp.new_hvals()
    ms = t_ms(lambda: nlp.hess_lag(Z, sigma, mu, out))
    per_problem = 8 * (nlp.n_nlp + 15 * (N - 1) + N + 1 + nlp.h_nnz)
    byts = B * per_problem + 8 * 41 * N * (B if nlp.cost_batch > 1 else 1)
    del out, Z, mu, nlp
    torch.cuda.empty_cache()
    return {"B": B, "N": N, "k_trans": k_trans, "ms": round(ms, 4), "compulsory_bytes": byts,
            "bytes_per_problem": per_problem, "GBps": round(byts / ms / 1e6, 1), "frac_of_8TBps": round(byts / ms / 1e-3 / PEAK, 4)}


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    res = [run(B, 40, 14), run(B, 61, 21)]
    print(json.dumps({"kernel": "qln_eval_hessian_lagrangian", "iters": 20, "warmup": 3, "results": res}))
