"""Launch time of the roll-out with guard-triggered touchdown (qln_tracking_rollout_guarded) next to the knot-scheduled
roll-out (qln_tracking_rollout) on the same inputs: HIP events, median of 20 launches after 3 warm-ups, three rounds per pair
with the order swapped from round to round, at B = 65 536, N = 40 and N = 61, with TVLQR gains and the handle's drop states.
Both calls move the same 800 B per knot; the guarded one adds 64 B of event record per problem and, on one knot per problem,
two more RK4 evaluations.  Prints one JSON line and writes it to the file named by --out.
   python bench/rollout_guarded_timing.py [B] [--out profiles/rollout_guarded_timing.json]
   python bench/rollout_guarded_timing.py [B] --plain-only [--label NAME] [--out FILE]
--plain-only times qln_tracking_rollout alone, and also loads a library built before the guarded entry points existed
(QLN_LIB_PATH): the kernel body the two share was touched when the guarded one was added, and this is how the roll-out of
the commit before and of this one are timed in one session."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import _lib  # noqa: E402

PLAIN_ONLY = "--plain-only" in sys.argv
if PLAIN_ONLY:
    for _name in [s for s in _lib.SIGNATURES if "guarded" in s]:
        del _lib.SIGNATURES[_name]  # a library from before this entry point has no such symbol to bind

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

from rollout_model_timing import Q, R, entry, pair_ms  # noqa: E402


def run(B, N, k_trans):
    torch.manual_seed(0)
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Zref = nlp.upload_Z(batch.Z)
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    out = nlp.new_Z()
    L = _lib.lib()
    d = lambda t: t.data_ptr()  # noqa: E731
    plain = lambda: _lib.check(L.qln_tracking_rollout(nlp._h, d(Zref), d(K), None, d(out)))  # noqa: E731
    knots = B * (N - 1)
    res = {"B": B, "N": N, "k_trans": k_trans}
    if PLAIN_ONLY:
        ms, _, per, _ = pair_ms(plain, plain)
        res["results"] = [entry("qln_tracking_rollout (K)", ms, per, knots * 800)]
    else:
        ev = torch.zeros((B, _lib.TOUCHDOWN_INFO_STRIDE), dtype=torch.float64, device=Zref.device)
        guarded = lambda: _lib.check(L.qln_tracking_rollout_guarded(nlp._h, d(Zref), d(K), None, None, d(out), d(ev)))  # noqa: E731
        ms_g, ms, per_g, per = pair_ms(guarded, plain)
        torch.cuda.synchronize()
        knot = ev[:, 0].cpu().numpy()
        res["results"] = [entry("qln_tracking_rollout_guarded (K, events)", ms_g, per_g, knots * 800 + B * 64),
                          entry("qln_tracking_rollout (K)", ms, per, knots * 800)]
        res["guarded_over_rollout"] = round(ms_g / ms, 4)
        res["touchdowns"] = {"share": round(float((knot >= 0).mean()), 4),
                             "knot_median": float(np.median(knot[knot >= 0])) if (knot >= 0).any() else None,
                             "planned_knot": k_trans - 2}
        del ev
    del K, out, Zref, nlp
    torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--plain-only"]
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    label = "this commit"
    if "--label" in args:
        i = args.index("--label")
        label = args[i + 1]
        del args[i:i + 2]
    B = int(args[0]) if args else 65536
    line = json.dumps({"iters": 20, "warmup": 3, "rounds": 3, "library": label,
                       "configs": [run(B, 40, 14), run(B, 61, 21)]})
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
