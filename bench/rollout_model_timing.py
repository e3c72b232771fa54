"""Launch time of the roll-out with a per-problem plant model and of its two sweeps (HIP events, median of 20 launches after
3 warm-ups, three rounds per pair with the order swapped from round to round) at B = 65 536, N = 40 and N = 61, each next to
the call without a model on the same inputs:
qln_tracking_rollout_model_jvp with gains and all four tangents against qln_tracking_rollout_jvp with all three,
qln_tracking_rollout_model_vjp with gains and all four outputs against qln_tracking_rollout_vjp with all three, and the
forward roll-out both ways.  The model forms move the same bytes per knot (1 560 B for the sweeps, 800 B forward) plus, per
problem, 32 B of model and 32 B of model_dot / model_bar.  Prints one JSON line and writes it to the file named by --out.
   python bench/rollout_model_timing.py [B] [--out profiles/rollout_model_timing.json]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, _lib, problem_gen as PG  # noqa: E402

PEAK = 8.0e12  # B/s, MI355X HBM spec
Q = np.array([10.0] * 14 + [0.0])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])


def pair_ms(with_model, without, reps=3, iters=20, warmup=3):
    """Launch times of two calls, interleaved: `reps` rounds, each timing `iters` launches of one and then of the other after
    `warmup` launches, the order swapped from round to round, so that neither call always runs first or on other clocks.
    Returns the two medians over all rounds and the per-round medians."""
    def one(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    m, w = [], []
    for r in range(reps):
        if r % 2 == 0:
            m.append(one(with_model))
            w.append(one(without))
        else:
            w.append(one(without))
            m.append(one(with_model))
    med = lambda rounds: float(np.median(np.concatenate(rounds)))  # noqa: E731
    per = lambda rounds: [round(float(np.median(x)), 4) for x in rounds]  # noqa: E731
    return med(m), med(w), per(m), per(w)


def entry(name, ms, rounds, byts):
    t_bw = byts / PEAK * 1e3
    return {"call": name, "ms": round(ms, 4), "ms_per_round": rounds, "bytes": int(byts), "hbm_floor_ms": round(t_bw, 4),
            "frac_of_peak": round(t_bw / ms, 4)}


def run(B, N, k_trans):
    torch.manual_seed(0)
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Zref = nlp.upload_Z(batch.Z)
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    rng = np.random.default_rng(0)
    model = nlp.plant_models() * torch.from_numpy(1.0 + 0.1 * rng.uniform(-1.0, 1.0, size=(B, 4))).cuda()
    Zout = nlp.tracking_rollout_model(Zref, K, None, model)
    Zbar = torch.randn_like(Zout)
    zd, kd = torch.randn_like(Zref), torch.randn_like(K)
    xd = torch.randn(B, 15, dtype=torch.float64, device=Zref.device)
    md = model * torch.randn(B, 4, dtype=torch.float64, device=Zref.device)
    zb, kb, xb, mb = nlp.tracking_rollout_model_vjp(Zref, Zout, Zbar, K, model)
    out = nlp.new_Z()
    L = _lib.lib()
    d = lambda t: t.data_ptr()  # noqa: E731
    jvp = lambda: _lib.check(L.qln_tracking_rollout_jvp(nlp._h, d(Zref), d(K), d(Zout), d(zd), d(kd), d(xd), d(out)))  # noqa: E731
    jvp_m = lambda: _lib.check(L.qln_tracking_rollout_model_jvp(  # noqa: E731
        nlp._h, d(Zref), d(K), d(Zout), d(model), d(zd), d(kd), d(xd), d(md), d(out)))
    vjp = lambda: _lib.check(L.qln_tracking_rollout_vjp(nlp._h, d(Zref), d(K), d(Zout), d(Zbar), d(zb), d(kb), d(xb)))  # noqa: E731
    vjp_m = lambda: _lib.check(L.qln_tracking_rollout_model_vjp(  # noqa: E731
        nlp._h, d(Zref), d(K), d(Zout), d(model), d(Zbar), d(zb), d(kb), d(xb), d(mb)))
    fwd = lambda: _lib.check(L.qln_tracking_rollout(nlp._h, d(Zref), d(K), None, d(out)))  # noqa: E731
    fwd_m = lambda: _lib.check(L.qln_tracking_rollout_model(nlp._h, d(Zref), d(K), None, d(model), d(out)))  # noqa: E731
    knots = B * (N - 1)
    res = []
    for (name_m, fn_m, bytes_m), (name, fn, byts) in (
            (("qln_tracking_rollout_model_jvp (K, all four tangents)", jvp_m, knots * 8 * 195 + B * 64),
             ("qln_tracking_rollout_jvp (K, all three tangents)", jvp, knots * 8 * 195)),
            (("qln_tracking_rollout_model_vjp (K, all four outputs)", vjp_m, knots * 8 * 195 + B * 64),
             ("qln_tracking_rollout_vjp (K, all three outputs)", vjp, knots * 8 * 195)),
            (("qln_tracking_rollout_model (forward, K)", fwd_m, knots * 8 * 100 + B * 32),
             ("qln_tracking_rollout (forward, K)", fwd, knots * 8 * 100))):
        ms_m, ms, per_m, per = pair_ms(fn_m, fn)
        res += [entry(name_m, ms_m, per_m, bytes_m), entry(name, ms, per, byts)]
    ratios = {"jvp_model_over_jvp": round(res[0]["ms"] / res[1]["ms"], 4),
              "vjp_model_over_vjp": round(res[2]["ms"] / res[3]["ms"], 4),
              "rollout_model_over_rollout": round(res[4]["ms"] / res[5]["ms"], 4)}
    del K, Zout, Zbar, zd, kd, xd, md, zb, kb, xb, mb, out, Zref, model, nlp
    torch.cuda.empty_cache()
    return {"B": B, "N": N, "k_trans": k_trans, "results": res, **ratios}


if __name__ == "__main__":
    args = sys.argv[1:]
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    B = int(args[0]) if args else 65536
    line = json.dumps({"iters": 20, "warmup": 3, "rounds": 3, "configs": [run(B, 40, 14), run(B, 61, 21)]})
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
