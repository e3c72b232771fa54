"""Launch time of qln_eval_hessian_lagrangian_product (HIP events, median of 20 launches after 3 warm-ups) at
BASELINE.json configs[2] (B = 65 536, N = 40, shared cost table) and at N = 61 (the notebook's horizon), against the
kernel's own compulsory bytes: Z, v and y (n_nlp doubles each), the dynamics and clearance multipliers, sigma and the
cost table (once if shared).  qln_eval_hessian_lagrangian is timed in the same run on the same inputs, and the host
(MOI) form's per-call latency is taken for the notebook's single problem (B = 1, N = 61).  Prints one JSON line.
   python bench/hessian_product_timing.py [B]"""
import json
import os
import sys
import time

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


def host_ms(fn, iters=20, warmup=3):
    """per-call wall time of a synchronous host call"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e3)


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf,
                    exact_hessian=True, matrix_free=True)
    Z = nlp.upload_Z(batch.Z)
    sigma = torch.rand(B, dtype=torch.float64, device="cuda")
    mu = torch.randn(nlp.dims.c_total, dtype=torch.float64, device="cuda")
    v = torch.randn(nlp.dims.z_total, dtype=torch.float64, device="cuda")
    y = nlp.new_Z()
    ms = t_ms(lambda: nlp.hess_lag_vec(Z, sigma, mu, v, y))
    hv = nlp.new_hvals()
    ms_hess = t_ms(lambda: nlp.hess_lag(Z, sigma, mu, hv))
    per_problem = 8 * (3 * nlp.n_nlp + 15 * (N - 1) + N + 1)
    byts = B * per_problem + 8 * 41 * N * (B if nlp.cost_batch > 1 else 1)
    del y, hv, v, Z, mu, nlp
    torch.cuda.empty_cache()
    return {"B": B, "N": N, "k_trans": k_trans, "ms": round(ms, 4), "compulsory_bytes": byts,
            "bytes_per_problem": per_problem, "GBps": round(byts / ms / 1e6, 1),
            "frac_of_8TBps": round(byts / ms / 1e-3 / PEAK, 4), "hessian_lagrangian_ms": round(ms_hess, 4)}


def run_host():
    nb = PG.notebook_problem()
    one = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, nb.N, nb.x0, nb.xf, exact_hessian=True, matrix_free=True)
    rng = np.random.default_rng(0)
    x = np.ascontiguousarray(nb.Z.reshape(-1))
    v = rng.normal(size=one.n_nlp)
    mu = rng.normal(size=one.dims.c_total)
    return {"B": 1, "N": nb.N, "hess_lag_vec_host_ms": round(host_ms(lambda: one.hess_lag_vec_host(x, 1.0, mu, v)), 4),
            "jac_vec_host_ms": round(host_ms(lambda: one.jac_vec_host(x, v)), 4),
            "jac_t_vec_host_ms": round(host_ms(lambda: one.jac_t_vec_host(x, mu)), 4),
            "hess_lag_host_ms": round(host_ms(lambda: one.hess_lag_host(x, 1.0, mu)), 4)}


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    res = [run(B, 40, 14), run(B, 61, 21)]
    print(json.dumps({"kernel": "qln_eval_hessian_lagrangian_product", "iters": 20, "warmup": 3, "results": res,
                      "host": run_host()}))
