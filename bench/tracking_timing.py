"""Launch time of qln_tracking_lqr (with and without the cost-to-go P) and of qln_tracking_rollout (HIP events, median of 20
launches after 3 warm-ups) at B = 65 536, N = 40 and N = 61, against two floors: the compulsory bytes over 8 TB/s (Zref read
once; K, and P when asked for, written once; the roll-out reads Zref and K and writes Zout) and the FP64 FMAs of the sparse
sweep (~3.5 k per knot and problem) over the chip's vector FP64 rate (profiles/r01_fp64_rate.txt: 16 FMA/clk/SIMD, 1024
SIMDs, 2.4 GHz).  The share of peak is taken against the larger of the two.  Prints one JSON line.
   python bench/tracking_timing.py [B]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

PEAK = 8.0e12  # B/s, MI355X HBM spec
FMA_RATE = 16 * 1024 * 2.4e9  # FP64 FMA/s
FMA_PER_KNOT = 3500
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


def entry(name, ms, byts, fmas):
    t_bw, t_fma = byts / PEAK * 1e3, fmas / FMA_RATE * 1e3
    floor = max(t_bw, t_fma)
    return {"call": name, "ms": round(ms, 4), "bytes": int(byts), "hbm_floor_ms": round(t_bw, 4),
            "fp64_floor_ms": round(t_fma, 4), "bound": "hbm" if t_bw >= t_fma else "fp64",
            "frac_of_peak": round(floor / ms, 4)}


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Z = nlp.upload_Z(batch.Z)
    K, P = nlp.tracking_lqr(Z, Q, R, Q)
    out = nlp.new_Z()
    zb, kb, pb = 8 * B * nlp.n_nlp, 8 * K.numel(), 8 * P.numel()
    fm = B * (N - 1) * FMA_PER_KNOT
    res = [entry("qln_tracking_lqr (K and P)", t_ms(lambda: nlp.tracking_lqr(Z, Q, R, Q, K, P)), zb + kb + pb, fm),
           entry("qln_tracking_lqr (K only)", t_ms(lambda: nlp.tracking_lqr(Z, Q, R, Q, K, with_cost_to_go=False)), zb + kb, fm),
           entry("qln_tracking_rollout", t_ms(lambda: nlp.tracking_rollout(Z, K, None, out)), 2 * zb + kb, B * (N - 1) * 60)]
    del K, P, out, Z, nlp
    torch.cuda.empty_cache()
    return {"B": B, "N": N, "k_trans": k_trans, "results": res}


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    print(json.dumps({"iters": 20, "warmup": 3, "lib": os.path.basename(os.environ.get("QLN_LIB_PATH", "libqln_hip.so")),
                      "configs": [run(B, 40, 14), run(B, 61, 21)]}))
