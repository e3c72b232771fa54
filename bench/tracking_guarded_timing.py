"""Launch time of the Riccati and covariance sweeps through the guard-triggered touchdown (qln_tracking_lqr_guarded,
qln_tracking_covariance_guarded) next to qln_tracking_lqr / qln_tracking_covariance on the same buffers in the same run, in
the protocol of bench/rollout_guarded_sweeps_timing.py: HIP events, median of 20 launches after 3 warm-ups, three rounds per
pair with the order swapped from round to round, at B = 65 536, N = 40 and N = 61.  Every problem lands: the free foot starts
between 2 and 12 cm above the ground at 1 m/s downwards, which spreads the touchdown over a dozen knots, so that the four
problems of a wave take their composite knot at different iterations of the loop.  The guarded calls run with per-problem
models, K and P (the Riccati sweep) and K, Sigma, marg and event_var (the covariance sweep).  Prints one JSON line and writes
it to the file named by --out.
   python bench/tracking_guarded_timing.py [B] [--out profiles/tracking_guarded_timing.json]
   python bench/tracking_guarded_timing.py [B] --plain-only [--label NAME] [--out FILE]
--plain-only times qln_tracking_lqr / qln_tracking_covariance alone, and also loads a library built before the guarded calls
existed (QLN_LIB_PATH): the two kernels gained template flags and kernel arguments, and this is how the sweeps of the commit
before and of this one are timed in one session, loaded in turn."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import _lib  # noqa: E402

PLAIN_ONLY = "--plain-only" in sys.argv
if PLAIN_ONLY:
    for _name in [s for s in _lib.SIGNATURES if "lqr_guarded" in s or "covariance_guarded" in s]:
        del _lib.SIGNATURES[_name]  # a library from before these entry points has no such symbols to bind

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

from rollout_model_timing import Q, R, entry, pair_ms  # noqa: E402

# operator applications the composite knot costs a lane (each two blocks deep, and the wave's other three rows wait for them):
# the Riccati sweep's (T, S) row, T's column and S's four columns; the covariance sweep's two
C_LQR, C_COV = 6, 2


def run(B, N, k_trans):
    torch.manual_seed(0)
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Zref = nlp.upload_Z(batch.Z)
    Kp, Pp = nlp.tracking_lqr(Zref, Q, R, Q)
    rng = np.random.default_rng(0)
    x0 = np.ascontiguousarray(batch.Z[:, :15], dtype=np.float64)
    x0[:, 6], x0[:, 13] = rng.uniform(0.02, 0.12, size=B), -1.0  # init_mode 1: foot 2 is the free one
    x0 = torch.from_numpy(x0).cuda()
    S0 = torch.from_numpy(np.ascontiguousarray(np.diag(np.full(15, 1e-4))[np.tril_indices(15)])).cuda()
    W = np.full(15, 1e-6)
    L = _lib.lib()
    d = lambda t: t.data_ptr()  # noqa: E731
    w = [np.ascontiguousarray(a, dtype=np.float64) for a in (Q, R, Q, W)]
    knots = B * (N - 1)
    byts_lqr = knots * 8 * (20 + 60) + B * N * 8 * 120
    byts_cov = knots * 8 * (20 + 60) + B * N * 8 * (120 + 8)
    res = {"B": B, "N": N, "k_trans": k_trans}
    Sp, mp = nlp.tracking_covariance(Zref, Kp, S0, W)
    lqr_p = lambda: _lib.check(L.qln_tracking_lqr(nlp._h, d(Zref), w[0].ctypes.data, w[1].ctypes.data, w[2].ctypes.data,  # noqa: E731
                                                  d(Kp), d(Pp)))
    cov_p = lambda: _lib.check(L.qln_tracking_covariance(nlp._h, d(Zref), d(Kp), d(S0), 1, w[3].ctypes.data, d(Sp), d(mp)))  # noqa: E731
    if PLAIN_ONLY:
        ms_l, ms_c, per_l, per_c = pair_ms(lqr_p, cov_p)
        res["results"] = [entry("qln_tracking_lqr (K, P)", ms_l, per_l, byts_lqr),
                          entry("qln_tracking_covariance (K, Sigma, marg)", ms_c, per_c, byts_cov)]
    else:
        model = nlp.plant_models() * torch.from_numpy(1.0 + 0.1 * rng.uniform(-1.0, 1.0, size=(B, 4))).cuda()
        Zg, ev = nlp.tracking_rollout_guarded(Zref, Kp, x0, model)
        Kg, Pg = nlp.tracking_lqr_guarded(Zg, ev, Q, R, Q, model)
        Sg, mg, vg = nlp.tracking_covariance_guarded(Zg, ev, Kg, S0, W, model)
        lqr_g = lambda: _lib.check(L.qln_tracking_lqr_guarded(nlp._h, d(Zg), d(model), d(ev), w[0].ctypes.data,  # noqa: E731
                                                              w[1].ctypes.data, w[2].ctypes.data, d(Kg), d(Pg)))
        cov_g = lambda: _lib.check(L.qln_tracking_covariance_guarded(nlp._h, d(Zg), d(Kg), d(model), d(ev), d(S0), 1,  # noqa: E731
                                                                     w[3].ctypes.data, d(Sg), d(mg), d(vg)))
        ms_lg, ms_lp, per_lg, per_lp = pair_ms(lqr_g, lqr_p)
        ms_cg, ms_cp, per_cg, per_cp = pair_ms(cov_g, cov_p)
        torch.cuda.synchronize()
        knot = ev[:, 0].cpu().numpy()
        res["results"] = [entry("qln_tracking_lqr_guarded (models, K, P)", ms_lg, per_lg, byts_lqr + B * 96),
                          entry("qln_tracking_lqr (K, P)", ms_lp, per_lp, byts_lqr),
                          entry("qln_tracking_covariance_guarded (models, K, Sigma, marg, event_var)", ms_cg, per_cg,
                                byts_cov + B * 112),
                          entry("qln_tracking_covariance (K, Sigma, marg)", ms_cp, per_cp, byts_cov)]
        res["lqr_guarded_over_plain"] = round(ms_lg / ms_lp, 4)
        res["covariance_guarded_over_plain"] = round(ms_cg / ms_cp, 4)
        res["lqr_extra_applications_per_divergent_problem"] = round((N + C_LQR) / (N - 1), 4)
        res["covariance_extra_applications_per_divergent_problem"] = round((N + C_COV) / (N - 1), 4)
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
