"""Launch time of qln_tracking_rollout_estimated / _guarded (every input and output, ny = 8) beside the roll-outs whose step it
takes twice, interleaved in the same run on the same box: qln_tracking_rollout_model and qln_tracking_rollout_guarded (gains,
models, event record).  HIP events; per call the median of three rounds, each the median of 20 launches after 3 warm-ups, and
the rounds' spread; B = 65 536, N = 40 and N = 61.  The floor beside each time is the compulsory bytes over 8 TB/s: Zref, K and
every other input read once, every output written once (the estimated call at N = 40, ny = 8: 795 of Zref, 2 340 of K, 4 800 of
L, 320 of v, 585 of w, 34 of x0, xhat0 and model in; 795 of Zout, 600 of Xhat, 320 of innov out: 84 712 B per problem, the
guarded form 16 doubles of records more).  Prints one JSON line (kept as profiles/tracking_estimated_timing.json).
   python bench/tracking_estimated_timing.py [B]
   QLN_LIB_PATH=<another build of libqln_hip.so> python bench/tracking_estimated_timing.py --siblings [B]
The second form times only the two sibling calls, for a library that may not have the new entry points (the parent's): run in
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
    for name in [s for s in _lib.SIGNATURES if s.startswith("qln_tracking_rollout_estimated")]:
        del _lib.SIGNATURES[name]

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402
from tracking_timing import PEAK, Q, R, t_ms  # noqa: E402

ROUNDS = 3
NY = 8


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Z = nlp.upload_Z(batch.Z)
    K, _ = nlp.tracking_lqr(Z, Q, R, Q, with_cost_to_go=False)
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    x0 = dev(batch.Z[:, :15] + 1e-3 * rng.normal(size=(B, 15)))
    model = nlp.plant_models()
    out, ev = nlp.new_Z(), torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    zb, kb, small = 8 * B * nlp.n_nlp, 8 * K.numel(), 8 * B * (15 + 4)
    calls = [("qln_tracking_rollout_model", lambda: nlp.tracking_rollout_model(Z, K, x0, model, out=out), 2 * zb + kb + small),
             ("qln_tracking_rollout_guarded", lambda: nlp.tracking_rollout_guarded(Z, K, x0, model, out=out), 2 * zb + kb + small + 64 * B)]
    if not SIBLINGS_ONLY:
        H = rng.normal(size=(NY, 15)) / np.sqrt(15.0)
        L = torch.from_numpy(1e-2 * rng.normal(size=(B, N, 15, NY))).cuda()
        v, w = dev(1e-3 * rng.normal(size=(B, N, NY))), dev(1e-4 * rng.normal(size=(B, N - 1, 15)))
        xh = dev(batch.Z[:, :15] + 1e-3 * rng.normal(size=(B, 15)))
        byts = 2 * zb + kb + small + 8 * (L.numel() + 2 * v.numel() + w.numel() + 2 * xh.numel() + B * N * 15)
        # the C entry points on preallocated outputs: the wrapper's fresh Xhat / innov tensors are not part of the launch
        Hd, Xh, iv = dev(H), torch.zeros((B, N, 15), dtype=torch.float64, device="cuda"), torch.zeros_like(v)
        eh = torch.zeros_like(ev)
        lib, p = _lib.lib(), lambda t: t.data_ptr()  # noqa: E731
        head = (nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(v), p(w), p(x0), p(xh), p(model), p(out), p(Xh), p(iv))
        calls.append(("qln_tracking_rollout_estimated", lambda: _lib.check(lib.qln_tracking_rollout_estimated(*head)), byts))
        calls.append(("qln_tracking_rollout_estimated_guarded",
                      lambda: _lib.check(lib.qln_tracking_rollout_estimated_guarded(*head, p(ev), p(eh))), byts + 128 * B))
    ms = {name: [] for name, _, _ in calls}
    for _ in range(ROUNDS):  # interleaved: every round times every call
        for name, fn, _ in calls:
            ms[name].append(t_ms(fn))
    res = []
    for name, _, byts in calls:
        med, floor = float(np.median(ms[name])), byts / PEAK * 1e3
        res.append({"call": name, "ms": round(med, 4), "rounds_ms": [round(v, 4) for v in ms[name]], "bytes": int(byts),
                    "bytes_per_problem": int(byts // B), "hbm_floor_ms": round(floor, 4), "frac_of_peak": round(floor / med, 4)})
    cfg = {"B": B, "N": N, "k_trans": k_trans, "ny": NY, "results": res}
    if not SIBLINGS_ONLY:
        cfg["estimated_over_twice_rollout_model"] = round(res[2]["ms"] / (2 * res[0]["ms"]), 4)
        cfg["estimated_guarded_over_twice_rollout_guarded"] = round(res[3]["ms"] / (2 * res[1]["ms"]), 4)
    del K, Z, nlp
    torch.cuda.empty_cache()
    return cfg


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 65536
    print(json.dumps({"library": os.path.basename(_lib.LIB_PATH), "siblings_only": SIBLINGS_ONLY, "iters": 20, "warmup": 3,
                      "rounds": ROUNDS, "configs": [run(B, 40, 14), run(B, 61, 21)]}))
