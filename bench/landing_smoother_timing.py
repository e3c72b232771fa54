"""Launch time of qln_landing_smoother and qln_landing_smoother_guarded (ny = 8; both outputs, Xs alone, Ps alone) beside the two
siblings whose work it resembles, interleaved in the same run on the same box: qln_tracking_kalman as the filter alone (the
forward pass the smoother reads) and qln_tracking_lqr (the other backward sweep).  HIP events; per call the median of three
rounds, each the median of 20 launches after 3 warm-ups, and the rounds' spread; B = 65 536, N = 40 and N = 61.  The floor
beside each time is the compulsory bytes over 8 TB/s: Ztraj, Lgain, Pest, Xhat and innov read once (the vector recursion alone
does not need Pest's second use, but reads it), every output written once.  Prints one JSON line (kept as
profiles/landing_smoother_timing.json).
   python bench/landing_smoother_timing.py [B]
   QLN_LIB_PATH=<another build of libqln_hip.so> python bench/landing_smoother_timing.py --siblings [B]
The second form times only the two sibling calls, for a library that does not have the new entry points (the parent's): run in
the same session, its times say whether this commit changed the siblings."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import _lib  # noqa: E402

SIBLINGS_ONLY = "--siblings" in sys.argv
if SIBLINGS_ONLY:  # the other library is asked for the symbols it has
    for name in [s for s in _lib.SIGNATURES if s.startswith("qln_landing_smoother")]:
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
    L, Pe, _, _ = nlp.tracking_kalman(Z, H, V, None, s0, W)
    zb, kb, lb, pb = 8 * B * nlp.n_nlp, 8 * K.numel(), 8 * L.numel(), 8 * Pe.numel()
    calls = [("qln_tracking_kalman (filter alone: L, Pest)", lambda: nlp.tracking_kalman(Z, H, V, None, s0, W), zb + lb + pb),
             ("qln_tracking_lqr (K and P)", lambda: nlp.tracking_lqr(Z, Q, R, Q, K, P), zb + kb + 8 * P.numel())]
    if not SIBLINGS_ONLY:
        gen = torch.Generator(device="cuda").manual_seed(0)
        Xhat = torch.randn(B, N, 15, dtype=torch.float64, device="cuda", generator=gen)
        innov = torch.randn(B, N, NY, dtype=torch.float64, device="cuda", generator=gen)
        # a guarded record: every problem lands in the knot its schedule switches in, a quarter of the step into it
        ev = torch.zeros(B, 8, dtype=torch.float64, device="cuda")
        ev[:, 0] = k_trans - 2
        ev[:, 1] = 0.25 * Z.view(B, -1)[:, 20 * (k_trans - 2) + 19]
        xb, ib = 8 * Xhat.numel(), 8 * innov.numel()
        rd = zb + lb + pb + xb + ib
        a = (Z, L, Pe, H, V, Xhat, innov)
        g = (Z, ev, L, Pe, H, V, Xhat, innov)
        calls += [("qln_landing_smoother (Xs and Ps)", lambda: nlp.landing_smoother(*a), rd + xb + pb),
                  ("qln_landing_smoother (Xs alone)", lambda: nlp.landing_smoother(*a, with_cov=False), rd + xb),
                  ("qln_landing_smoother (Ps alone)", lambda: nlp.landing_smoother(*a, with_states=False), rd - xb - ib + pb),
                  ("qln_landing_smoother_guarded (Xs and Ps)", lambda: nlp.landing_smoother_guarded(*g), rd + xb + pb),
                  ("qln_landing_smoother_guarded (Xs alone)", lambda: nlp.landing_smoother_guarded(*g, with_cov=False), rd + xb),
                  ("qln_landing_smoother_guarded (Ps alone)", lambda: nlp.landing_smoother_guarded(*g, with_states=False),
                   rd - xb - ib + pb)]
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
        out["smoother_over_filter_alone"] = round(res[2]["ms"] / res[0]["ms"], 4)
        out["smoother_over_lqr"] = round(res[2]["ms"] / res[1]["ms"], 4)
    del K, P, L, Pe, Z, nlp
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 65536
    print(json.dumps({"library": os.path.basename(_lib.LIB_PATH), "siblings_only": SIBLINGS_ONLY, "iters": 20, "warmup": 3,
                      "rounds": ROUNDS, "configs": [run(B, 40, 14), run(B, 61, 21)]}))
