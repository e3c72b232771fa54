"""Launch time of qln_landing_filter and qln_landing_filter_guarded (ny = 8; without the score, with it) beside the kernel whose
estimator half it is, interleaved in the same run on the same box: qln_tracking_rollout_estimated and its guarded form (every
input and output).  The filter without the score does one of that kernel's two steps and a subset of its loads, so it must not be
slower; the score's extra cost is reported.  HIP events; per call the median of three rounds, each the median of 20 launches
after 3 warm-ups, and the rounds' spread; B = 65 536, N = 40 and N = 61.  The floor beside each time is the compulsory bytes over
8 TB/s: the state slots of Zref, the control slots of Zrec, Lgain, Y and xhat0 read once, every output written once.  Prints one
JSON line (kept as profiles/landing_filter_timing.json).
   python bench/landing_filter_timing.py [B]
   QLN_LIB_PATH=<another build of libqln_hip.so> python bench/landing_filter_timing.py --siblings [B]
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
    for name in [s for s in _lib.SIGNATURES if s.startswith("qln_landing_filter")]:
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
    xh = dev(batch.Z[:, :15] + 1e-3 * rng.normal(size=(B, 15)))
    model = nlp.plant_models()
    H = rng.normal(size=(NY, 15)) / np.sqrt(15.0)
    L = torch.from_numpy(1e-2 * rng.normal(size=(B, N, 15, NY))).cuda()
    v, w = dev(1e-3 * rng.normal(size=(B, N, NY))), dev(1e-4 * rng.normal(size=(B, N - 1, 15)))
    out, ev, eh = nlp.new_Z(), torch.zeros((B, 8), dtype=torch.float64, device="cuda"), torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    Hd, Xh, iv = dev(H), torch.zeros((B, N, 15), dtype=torch.float64, device="cuda"), torch.zeros_like(v)
    zb, kb, small = 8 * B * nlp.n_nlp, 8 * K.numel(), 8 * B * (15 + 4)
    lib, p = _lib.lib(), lambda t: t.data_ptr()  # noqa: E731
    # the C entry points on preallocated outputs: a wrapper's fresh tensors are not part of the launch
    head = (nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(v), p(w), p(x0), p(xh), p(model), p(out), p(Xh), p(iv))
    eb = 2 * zb + kb + small + 8 * (L.numel() + 2 * v.numel() + w.numel() + 2 * xh.numel() + B * N * 15)
    calls = [("qln_tracking_rollout_estimated", lambda: _lib.check(lib.qln_tracking_rollout_estimated(*head)), eb),
             ("qln_tracking_rollout_estimated_guarded",
              lambda: _lib.check(lib.qln_tracking_rollout_estimated_guarded(*head, p(ev), p(eh))), eb + 128 * B)]
    if not SIBLINGS_ONLY:
        # the record of one flight: its Zout's controls and its measurements
        _lib.check(lib.qln_tracking_rollout_estimated(*head))
        Zrec = out.clone()
        Y = nlp.landing_measurements(Zrec, Z, H, v)
        Vd = np.full(NY, 1e-6)
        Xo, io = torch.zeros_like(Xh), torch.zeros_like(iv)
        sc, ll = torch.zeros((B, N, 2), dtype=torch.float64, device="cuda"), torch.zeros((B,), dtype=torch.float64, device="cuda")
        fh = (nlp._h, p(Z), p(Zrec), p(L), p(Hd), NY)
        rd = 8 * B * (15 * N + 5 * (N - 1)) + 8 * (L.numel() + Y.numel() + xh.numel())
        plain, scored = rd + 8 * (Xo.numel() + io.numel()), rd + 8 * (Xo.numel() + io.numel() + sc.numel() + ll.numel())
        calls += [("qln_landing_filter (Xhat, innov)",
                   lambda: _lib.check(lib.qln_landing_filter(*fh, None, p(Y), p(xh), p(Xo), p(io), None, None)), plain),
                  ("qln_landing_filter (and score, loglik)",
                   lambda: _lib.check(lib.qln_landing_filter(*fh, Vd.ctypes.data, p(Y), p(xh), p(Xo), p(io), p(sc), p(ll))), scored),
                  ("qln_landing_filter_guarded (Xhat, innov, event_hat)",
                   lambda: _lib.check(lib.qln_landing_filter_guarded(*fh, None, p(Y), p(xh), p(Xo), p(io), None, None, p(eh))), plain + 64 * B),
                  ("qln_landing_filter_guarded (and score, loglik)",
                   lambda: _lib.check(lib.qln_landing_filter_guarded(*fh, Vd.ctypes.data, p(Y), p(xh), p(Xo), p(io), p(sc), p(ll), p(eh))),
                   scored + 64 * B)]
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
        cfg["filter_over_estimated"] = round(res[2]["ms"] / res[0]["ms"], 4)
        cfg["filter_guarded_over_estimated_guarded"] = round(res[4]["ms"] / res[1]["ms"], 4)
        cfg["score_over_filter"] = round(res[3]["ms"] / res[2]["ms"], 4)
        cfg["score_guarded_over_filter_guarded"] = round(res[5]["ms"] / res[4]["ms"], 4)
    del K, Z, L, nlp
    torch.cuda.empty_cache()
    return cfg


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 65536
    print(json.dumps({"library": os.path.basename(_lib.LIB_PATH), "siblings_only": SIBLINGS_ONLY, "iters": 20, "warmup": 3,
                      "rounds": ROUNDS, "configs": [run(B, 40, 14), run(B, 61, 21)]}))
