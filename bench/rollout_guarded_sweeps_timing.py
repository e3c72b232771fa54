"""Launch time of the sweeps through the guard-triggered touchdown (qln_tracking_rollout_guarded_jvp / _vjp) next to the
_model_ sweeps (qln_tracking_rollout_model_jvp / _vjp) on the same buffers in the same run: HIP events, median of 20 launches
after 3 warm-ups, three rounds per pair with the order swapped from round to round, at B = 65 536, N = 40 and N = 61, with
TVLQR gains, per-problem models and every tangent / output.  Every problem lands: the free foot starts between 2 and 12 cm
above the ground at 1 m/s downwards, which spreads the touchdown over a dozen knots, so that the four problems of a wave
take their composite knot at different iterations of the loop.  All four calls move 1 560 B per knot; the guarded ones add
64 B of event record per problem (and 64 B of event_dot).  Prints one JSON line and writes it to the file named by --out.
   python bench/rollout_guarded_sweeps_timing.py [B] [--out profiles/rollout_guarded_sweeps_timing.json]
   python bench/rollout_guarded_sweeps_timing.py [B] --plain-only [--label NAME] [--out FILE]
--plain-only times qln_tracking_rollout_jvp / _vjp alone, and also loads a library built before the guarded sweeps existed
(QLN_LIB_PATH): the two kernels gained a template flag and kernel arguments, and this is how the sweeps of the commit before
and of this one are timed in one session, loaded in turn."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import _lib  # noqa: E402

PLAIN_ONLY = "--plain-only" in sys.argv
if PLAIN_ONLY:
    for _name in [s for s in _lib.SIGNATURES if "guarded_jvp" in s or "guarded_vjp" in s]:
        del _lib.SIGNATURES[_name]  # a library from before these entry points has no such symbols to bind

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

from rollout_model_timing import Q, R, entry, pair_ms  # noqa: E402


def run(B, N, k_trans):
    torch.manual_seed(0)
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Zref = nlp.upload_Z(batch.Z)
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    rng = np.random.default_rng(0)
    model = nlp.plant_models() * torch.from_numpy(1.0 + 0.1 * rng.uniform(-1.0, 1.0, size=(B, 4))).cuda()
    x0 = np.ascontiguousarray(batch.Z[:, :15], dtype=np.float64)
    x0[:, 6], x0[:, 13] = rng.uniform(0.02, 0.12, size=B), -1.0  # init_mode 1: foot 2 is the free one
    x0 = torch.from_numpy(x0).cuda()
    zd, kd = torch.randn_like(Zref), torch.randn_like(K)
    xd = torch.randn(B, 15, dtype=torch.float64, device=Zref.device)
    md = model * torch.randn(B, 4, dtype=torch.float64, device=Zref.device)
    out = nlp.new_Z()
    L = _lib.lib()
    d = lambda t: t.data_ptr()  # noqa: E731
    knots = B * (N - 1)
    res = {"B": B, "N": N, "k_trans": k_trans}
    if PLAIN_ONLY:
        Zout = nlp.tracking_rollout(Zref, K, x0)
        Zbar = torch.randn_like(Zout)
        zb, kb, xb = nlp.tracking_rollout_vjp(Zref, Zout, Zbar, K)
        jvp = lambda: _lib.check(L.qln_tracking_rollout_jvp(nlp._h, d(Zref), d(K), d(Zout), d(zd), d(kd), d(xd), d(out)))  # noqa: E731
        vjp = lambda: _lib.check(L.qln_tracking_rollout_vjp(nlp._h, d(Zref), d(K), d(Zout), d(Zbar), d(zb), d(kb), d(xb)))  # noqa: E731
        ms_j, ms_v, per_j, per_v = pair_ms(jvp, vjp)
        res["results"] = [entry("qln_tracking_rollout_jvp (K, all three tangents)", ms_j, per_j, knots * 8 * 195),
                          entry("qln_tracking_rollout_vjp (K, all three outputs)", ms_v, per_v, knots * 8 * 195)]
    else:
        Zout, ev = nlp.tracking_rollout_guarded(Zref, K, x0, model)
        Zbar = torch.randn_like(Zout)
        zb, kb, xb, mb = nlp.tracking_rollout_guarded_vjp(Zref, Zout, ev, Zbar, K, model)
        ed = torch.zeros_like(ev)
        jvp_g = lambda: _lib.check(L.qln_tracking_rollout_guarded_jvp(  # noqa: E731
            nlp._h, d(Zref), d(K), d(Zout), d(model), d(ev), d(zd), d(kd), d(xd), d(md), d(out), d(ed)))
        jvp_m = lambda: _lib.check(L.qln_tracking_rollout_model_jvp(  # noqa: E731
            nlp._h, d(Zref), d(K), d(Zout), d(model), d(zd), d(kd), d(xd), d(md), d(out)))
        vjp_g = lambda: _lib.check(L.qln_tracking_rollout_guarded_vjp(  # noqa: E731
            nlp._h, d(Zref), d(K), d(Zout), d(model), d(ev), d(Zbar), d(zb), d(kb), d(xb), d(mb)))
        vjp_m = lambda: _lib.check(L.qln_tracking_rollout_model_vjp(  # noqa: E731
            nlp._h, d(Zref), d(K), d(Zout), d(model), d(Zbar), d(zb), d(kb), d(xb), d(mb)))
        ms_jg, ms_jm, per_jg, per_jm = pair_ms(jvp_g, jvp_m)
        ms_vg, ms_vm, per_vg, per_vm = pair_ms(vjp_g, vjp_m)
        torch.cuda.synchronize()
        knot = ev[:, 0].cpu().numpy()
        res["results"] = [entry("qln_tracking_rollout_guarded_jvp (K, all four tangents, event_dot)", ms_jg, per_jg,
                                knots * 8 * 195 + B * 192),
                          entry("qln_tracking_rollout_model_jvp (K, all four tangents)", ms_jm, per_jm, knots * 8 * 195 + B * 64),
                          entry("qln_tracking_rollout_guarded_vjp (K, all four outputs)", ms_vg, per_vg, knots * 8 * 195 + B * 128),
                          entry("qln_tracking_rollout_model_vjp (K, all four outputs)", ms_vm, per_vm, knots * 8 * 195 + B * 64)]
        res["jvp_guarded_over_model"] = round(ms_jg / ms_jm, 4)
        res["vjp_guarded_over_model"] = round(ms_vg / ms_vm, 4)
        res["one_extra_knot_per_divergent_problem"] = round((N + 3) / (N - 1), 4)
        res["touchdowns"] = {"share": round(float((knot >= 0).mean()), 4), "knot_min": float(knot.min()),
                             "knot_median": float(np.median(knot)), "knot_max": float(knot.max()),
                             "distinct_knots": int(len(np.unique(knot)))}
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
