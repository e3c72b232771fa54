"""Launch time of qln_tracking_covariance (Sigma and marg, marg only, open loop) and, in the same run on the same box, of
qln_tracking_lqr with P, by bench/tracking_timing.py's method: HIP events, median of 20 launches after 3 warm-ups, at
B = 65 536, N = 40 and N = 61.  The floor beside each time is the compulsory bytes over 8 TB/s: Zout read once (795
doubles per problem at N = 40), K read once (2 340), Sigma (4 800) and marg
(320) written once -- 66 040 B per problem, 4.33 GB per launch, 0.54 ms for the full call at N = 40.  Prints one JSON line
(kept as profiles/tracking_covariance_timing.json).
   python bench/tracking_covariance_timing.py [B]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402
from tracking_timing import PEAK, Q, R, t_ms  # noqa: E402


def entry(name, ms, byts):
    floor = byts / PEAK * 1e3
    return {"call": name, "ms": round(ms, 4), "bytes": int(byts), "hbm_floor_ms": round(floor, 4),
            "frac_of_peak": round(floor / ms, 4)}


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Z = nlp.upload_Z(batch.Z)
    K, P = nlp.tracking_lqr(Z, Q, R, Q)
    rng = np.random.default_rng(0)
    G = rng.normal(size=(15, 15))
    s0 = torch.from_numpy(np.ascontiguousarray((G @ G.T / 15)[np.tril_indices(15)])).cuda()
    W = rng.uniform(0.0, 1e-3, size=15)
    S, mg = nlp.tracking_covariance(Z, K, s0, W)
    zb = 8 * B * nlp.n_nlp
    kb, sb, mb = 8 * K.numel(), 8 * S.numel(), 8 * mg.numel()
    res = [entry("qln_tracking_covariance (Sigma and marg)", t_ms(lambda: nlp.tracking_covariance(Z, K, s0, W, Sigma=S, marg=mg)),
                 zb + kb + sb + mb),
           entry("qln_tracking_covariance (marg only)",
                 t_ms(lambda: nlp.tracking_covariance(Z, K, s0, W, with_sigma=False, marg=mg)), zb + kb + mb),
           entry("qln_tracking_covariance (open loop, Sigma and marg)",
                 t_ms(lambda: nlp.tracking_covariance(Z, None, s0, W, Sigma=S, marg=mg)), zb + sb + mb),
           entry("qln_tracking_lqr (K and P)", t_ms(lambda: nlp.tracking_lqr(Z, Q, R, Q, K, P)), 8 * B * nlp.n_nlp + kb + 8 * P.numel())]
    del K, P, S, mg, Z, nlp
    torch.cuda.empty_cache()
    return {"B": B, "N": N, "k_trans": k_trans, "results": res,
            "covariance_over_lqr": round(res[0]["ms"] / res[3]["ms"], 4)}


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    print(json.dumps({"iters": 20, "warmup": 3, "configs": [run(B, 40, 14), run(B, 61, 21)]}))
