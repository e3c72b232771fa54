"""Launch time of qln_tracking_kalman (every output, TVLQR gains, ny = 8) beside the calls whose work it contains, interleaved in
the same run on the same box: qln_tracking_covariance open loop (the prediction of P) and closed loop (the prediction of M),
and qln_tracking_lqr.  HIP events; per call the median of three rounds, each the median of 20 launches after 3 warm-ups, and
the rounds' spread; B = 65 536, N = 40 and N = 61.  The floor beside each time is the compulsory bytes over 8 TB/s: Zout and K
read once, every output written once (the Kalman call at N = 40: 795 + 2 340 doubles in, 4 800 of L, 4 800 of P+, 4 800 of X
and 320 of marg out: 142 840 B per problem).  Prints one JSON line (kept as profiles/tracking_kalman_timing.json).
   python bench/tracking_kalman_timing.py [B]
   QLN_LIB_PATH=<another build of libqln_hip.so> python bench/tracking_kalman_timing.py --siblings [B]
The second form times only the three sibling calls, for a library that may not have the new entry points (the parent's): run
in the same session, its times say whether this commit changed the siblings."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import _lib  # noqa: E402

SIBLINGS_ONLY = "--siblings" in sys.argv
if SIBLINGS_ONLY:  # the other library is asked for the symbols it has
    for name in [s for s in _lib.SIGNATURES if s.startswith("qln_tracking_kalman")]:
        del _lib.SIGNATURES[name]

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402
from tracking_timing import PEAK, Q, R, t_ms  # noqa: E402

ROUNDS = 3
NY = 8


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Z = nlp.upload_Z(batch.Z)
    K, P = nlp.tracking_lqr(Z, Q, R, Q)
    rng = np.random.default_rng(0)
    G = rng.normal(size=(15, 15))
    s0 = torch.from_numpy(np.ascontiguousarray((G @ G.T / 15)[np.tril_indices(15)])).cuda()
    W = rng.uniform(0.0, 1e-3, size=15)
    H, V = rng.normal(size=(NY, 15)) / np.sqrt(15.0), rng.uniform(0.5, 2.0, size=NY)
    S, mg = nlp.tracking_covariance(Z, K, s0, W)
    zb, kb, sb, mb = 8 * B * nlp.n_nlp, 8 * K.numel(), 8 * S.numel(), 8 * mg.numel()
    calls = [("qln_tracking_covariance (open loop)", lambda: nlp.tracking_covariance(Z, None, s0, W, Sigma=S, marg=mg), zb + sb + mb),
             ("qln_tracking_covariance (closed loop)", lambda: nlp.tracking_covariance(Z, K, s0, W, Sigma=S, marg=mg), zb + kb + sb + mb),
             ("qln_tracking_lqr (K and P)", lambda: nlp.tracking_lqr(Z, Q, R, Q, K, P), zb + kb + 8 * P.numel())]
    if not SIBLINGS_ONLY:
        lb = 8 * B * N * 15 * NY
        calls.append(("qln_tracking_kalman (L, Pest, Sigma, marg)", lambda: nlp.tracking_kalman(Z, H, V, K, s0, W), zb + kb + lb + 2 * sb + mb))
        calls.append(("qln_tracking_kalman (filter alone: L, Pest)", lambda: nlp.tracking_kalman(Z, H, V, None, s0, W), zb + lb + sb))
    ms = {name: [] for name, _, _ in calls}
    for _ in range(ROUNDS):  # interleaved: every round times every call
        for name, fn, _ in calls:
            ms[name].append(t_ms(fn))
    res = []
    for name, _, byts in calls:
        med, floor = float(np.median(ms[name])), byts / PEAK * 1e3
        res.append({"call": name, "ms": round(med, 4), "rounds_ms": [round(v, 4) for v in ms[name]], "bytes": int(byts),
                    "bytes_per_problem": int(byts // B), "hbm_floor_ms": round(floor, 4), "frac_of_peak": round(floor / med, 4)})
    out = {"B": B, "N": N, "k_trans": k_trans, "ny": NY, "results": res}
    if not SIBLINGS_ONLY:
        out["kalman_over_covariance_siblings_sum"] = round(res[3]["ms"] / (res[0]["ms"] + res[1]["ms"]), 4)
        out["kalman_over_lqr"] = round(res[3]["ms"] / res[2]["ms"], 4)
    del K, P, S, mg, Z, nlp
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 65536
    print(json.dumps({"library": os.path.basename(_lib.LIB_PATH), "siblings_only": SIBLINGS_ONLY, "iters": 20, "warmup": 3,
                      "rounds": ROUNDS, "configs": [run(B, 40, 14), run(B, 61, 21)]}))
