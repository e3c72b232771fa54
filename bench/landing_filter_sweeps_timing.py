"""Launch time of qln_landing_filter_jvp and qln_landing_filter_vjp (ny = 8; without the score's terms, with them) beside the
kernels whose estimator half they are, interleaved in the same run on the same box: qln_tracking_rollout_estimated_jvp and
_vjp with K, a per-problem model and every tangent / cotangent but Lgain's.  The filter's sweeps read a subset of the siblings'
bytes and apply one block per knot where the siblings apply two, so the expectation is that each takes less than its sibling;
the figure is reported, not asserted.  The protocol is bench/landing_filter_timing.py's: HIP events; per call the median of
three rounds, each the median of 20 launches after 3 warm-ups, and the rounds' spread; B = 65 536, N = 40 and N = 61.  The floor
beside each time is the compulsory bytes over 8 TB/s: every input the call reads once, every output written once.  Prints one
JSON line (kept as profiles/landing_filter_sweeps_timing.json).
   python bench/landing_filter_sweeps_timing.py [B]
   QLN_LIB_PATH=<another build of libqln_hip.so> python bench/landing_filter_sweeps_timing.py --siblings [B]
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
NEW = ("qln_landing_filter_model", "qln_landing_filter_guarded_model", "qln_landing_filter_jvp", "qln_landing_filter_vjp",
       "qln_landing_filter_guarded_jvp", "qln_landing_filter_guarded_vjp")
if SIBLINGS_ONLY:  # the other library is asked for the symbols it has
    for name in [s for s in _lib.SIGNATURES if s.startswith(NEW)]:
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
    zeros = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    rand = lambda *s: 1e-2 * torch.randn(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    torch.manual_seed(0)
    x0 = dev(batch.Z[:, :15] + 1e-3 * rng.normal(size=(B, 15)))
    xh = dev(batch.Z[:, :15] + 1e-3 * rng.normal(size=(B, 15)))
    model = nlp.plant_models()
    H = rng.normal(size=(NY, 15)) / np.sqrt(15.0)
    L = torch.from_numpy(1e-2 * rng.normal(size=(B, N, 15, NY))).cuda()
    v, w = dev(1e-3 * rng.normal(size=(B, N, NY))), dev(1e-4 * rng.normal(size=(B, N - 1, 15)))
    Hd = dev(H)
    lib, p = _lib.lib(), lambda t: t.data_ptr()  # noqa: E731
    # one flight: the point of the siblings' sweeps, and the record of the filter's
    Zout, Xhat, innov = nlp.new_Z(), zeros(B, N, 15), zeros(B, N, NY)
    _lib.check(lib.qln_tracking_rollout_estimated(nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(v), p(w), p(x0), p(xh), p(model), p(Zout),
                                                  p(Xhat), p(innov)))
    zd, xd, hd, md = rand(Z.numel()), rand(B, 15), rand(B, 15), rand(B, 4) * model
    Zbar, Xb, Ib = rand(Z.numel()), rand(B, N, 15), rand(B, N, NY)
    zo_d, xh_d, iv_d = nlp.new_Z(), zeros(B, N, 15), zeros(B, N, NY)
    zr_b, x0_b, xh_b, m_b = nlp.new_Z(), zeros(B, 15), zeros(B, 15), zeros(B, 4)
    zb, kb, gb = 8 * B * nlp.n_nlp, 8 * K.numel(), 8 * L.numel()
    xb, ib, small = 8 * B * N * 15, 8 * B * N * NY, 8 * B * (15 + 15 + 4 + 4)
    point = (nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(model), p(Zout), p(Xhat), p(innov))
    # the sweeps do not read Zref without K_dot / K_bar, nor innov without Lgain's tangent / cotangent
    sib_j = zb + kb + gb + xb + zb + small + zb + xb + ib
    sib_v = zb + kb + gb + xb + zb + xb + ib + zb + small
    calls = [("qln_tracking_rollout_estimated_jvp",
              lambda: _lib.check(lib.qln_tracking_rollout_estimated_jvp(*point, p(zd), None, None, p(xd), p(hd), p(md), p(zo_d), p(xh_d),
                                                                        p(iv_d))), sib_j),
             ("qln_tracking_rollout_estimated_vjp",
              lambda: _lib.check(lib.qln_tracking_rollout_estimated_vjp(*point, p(Zbar), p(Xb), p(Ib), p(zr_b), None, None, p(x0_b),
                                                                        p(xh_b), p(m_b))), sib_v)]
    if not SIBLINGS_ONLY:
        Y = nlp.landing_measurements(Zout, Z, H, v)
        Vd = np.full(NY, 1e-6)
        yd, nd, ld = rand(B, N, NY), zeros(B, N), zeros(B)
        nb, lb = rand(B, N), rand(B)
        y_b = zeros(B, N, NY)
        rec = (nlp._h, p(Z), p(Zout), p(L), p(Hd), NY, p(model))
        ctrl = 8 * B * 5 * (N - 1)  # the control slots of Zrec, of Zrec_dot, of Zrec_bar
        fj = ctrl + gb + xb + ib + ctrl + small + xb + ib
        fv = ctrl + gb + xb + xb + ib + ib + zb + small
        score = ib + 8 * B * N + 8 * B
        calls += [("qln_landing_filter_jvp (Xhat_dot, innov_dot)",
                   lambda: _lib.check(lib.qln_landing_filter_jvp(*rec, None, p(Xhat), None, p(yd), p(zd), None, p(hd), p(md), p(xh_d),
                                                                 p(iv_d), None, None)), fj),
                  ("qln_landing_filter_jvp (and nis_dot, loglik_dot)",
                   lambda: _lib.check(lib.qln_landing_filter_jvp(*rec, Vd.ctypes.data, p(Xhat), p(innov), p(yd), p(zd), None, p(hd),
                                                                 p(md), p(xh_d), p(iv_d), p(nd), p(ld))), fj + score),
                  ("qln_landing_filter_vjp (Xhat_bar, innov_bar)",
                   lambda: _lib.check(lib.qln_landing_filter_vjp(*rec, None, p(Xhat), None, p(Xb), p(Ib), None, None, p(y_b), p(zr_b),
                                                                 None, p(xh_b), p(m_b))), fv),
                  ("qln_landing_filter_vjp (and nis_bar, loglik_bar)",
                   lambda: _lib.check(lib.qln_landing_filter_vjp(*rec, Vd.ctypes.data, p(Xhat), p(innov), p(Xb), p(Ib), p(nb), p(lb),
                                                                 p(y_b), p(zr_b), None, p(xh_b), p(m_b))), fv + score)]
    ms = {name: [] for name, _, _ in calls}
    for _ in range(ROUNDS):  # interleaved: every round times every call
        for name, fn, _ in calls:
            ms[name].append(t_ms(fn))
    res = []
    for name, _, byts in calls:
        med, floor = float(np.median(ms[name])), byts / PEAK * 1e3
        res.append({"call": name, "ms": round(med, 4), "rounds_ms": [round(t, 4) for t in ms[name]], "bytes": int(byts),
                    "bytes_per_problem": int(byts // B), "hbm_floor_ms": round(floor, 4), "frac_of_peak": round(floor / med, 4)})
    cfg = {"B": B, "N": N, "k_trans": k_trans, "ny": NY, "results": res}
    if not SIBLINGS_ONLY:
        cfg["filter_jvp_over_estimated_jvp"] = round(res[2]["ms"] / res[0]["ms"], 4)
        cfg["filter_vjp_over_estimated_vjp"] = round(res[4]["ms"] / res[1]["ms"], 4)
        cfg["score_over_filter_jvp"] = round(res[3]["ms"] / res[2]["ms"], 4)
        cfg["score_over_filter_vjp"] = round(res[5]["ms"] / res[4]["ms"], 4)
    del K, Z, L, nlp
    torch.cuda.empty_cache()
    return cfg


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 65536
    print(json.dumps({"library": os.path.basename(_lib.LIB_PATH), "siblings_only": SIBLINGS_ONLY, "iters": 20, "warmup": 3,
                      "rounds": ROUNDS, "configs": [run(B, 40, 14), run(B, 61, 21)]}))
