"""Launch time of qln_tracking_rollout_vjp (HIP events, median of 20 launches after 3 warm-ups) at B = 65 536, N = 40 and
N = 61, with TVLQR gains and all three outputs, and with K == NULL (the shooting gradient, Zref_bar and x0_bar), against
the compulsory bytes over 8 TB/s: with K, Zout and Zbar read (20 doubles per knot each), Zref's states (15) and K (60)
read, Zref_bar (20) and K_bar (60) written; without K, Zout and Zbar read and Zref_bar written.  Prints one JSON line.
   python bench/rollout_vjp_timing.py [B]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

PEAK = 8.0e12  # B/s, MI355X HBM spec
Q = np.array([10.0] * 14 + [0.0])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])


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


def entry(name, ms, byts, target):
    t_bw = byts / PEAK * 1e3
    return {"call": name, "ms": round(ms, 4), "bytes": int(byts), "hbm_floor_ms": round(t_bw, 4),
            "frac_of_peak": round(t_bw / ms, 4), "target_ms": target, "met": ms <= target}


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Zref = nlp.upload_Z(batch.Z)
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    Zout = nlp.tracking_rollout(Zref, K)
    Zbar = torch.randn_like(Zout)
    zb, kb, xb = nlp.tracking_rollout_vjp(Zref, Zout, Zbar, K)
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    knots = B * (N - 1)
    with_k = knots * 8 * (20 + 20 + 15 + 60 + 20 + 60)
    no_k = knots * 8 * (20 + 20 + 20)
    call = lambda kp, kbp: _lib.check(L.qln_tracking_rollout_vjp(  # noqa: E731
        nlp._h, Zref.data_ptr(), kp, Zout.data_ptr(), Zbar.data_ptr(), zb.data_ptr(), kbp, xb.data_ptr()))
    res = [entry("qln_tracking_rollout_vjp (K, all outputs)", t_ms(lambda: call(K.data_ptr(), kb.data_ptr())), with_k, 1.0),
           entry("qln_tracking_rollout_vjp (K == NULL)", t_ms(lambda: call(None, None)), no_k, 0.45),
           entry("qln_tracking_rollout (forward, K)", t_ms(lambda: nlp.tracking_rollout(Zref, K, None, Zout)),
                 knots * 8 * (20 + 20 + 60), float("nan"))]
    del K, Zout, Zbar, zb, kb, xb, Zref, nlp
    torch.cuda.empty_cache()
    return {"B": B, "N": N, "k_trans": k_trans, "results": res}


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    print(json.dumps({"iters": 20, "warmup": 3, "configs": [run(B, 40, 14), run(B, 61, 21)]}))
