"""Launch time of the calls with contact-aware force limits, each next to its unlimited sibling on the same inputs, by the
method of bench/rollout_guarded_timing.py: HIP events, median of 20 launches after 3 warm-ups, three rounds per pair with the
order swapped from round to round, at B = 65 536, N = 40 and N = 61, with TVLQR gains and the handle's drop states.
   qln_tracking_rollout_limited (guarded)      | qln_tracking_rollout_guarded
   qln_tracking_rollout_limited (knot schedule)| qln_tracking_rollout_model
   qln_tracking_rollout_limited_jvp / _vjp     | qln_tracking_rollout_guarded_jvp / _vjp   (gains, every tangent / output)
   qln_tracking_lqr_limited (event, P)         | qln_tracking_lqr_guarded
   qln_tracking_lqr_limited (knot schedule, P) | qln_tracking_lqr
A limited call moves its sibling's bytes plus 8 B of saturation code per knot.  The limits come from the plan's own forces: no
pull under a standing foot, and caps at the 99th percentile of the forces of the kind in the references, so that a realistic
share of (knot, channel) pairs rides a limit (reported).  The sweeps and the designs of a pair run at the same trajectory, the
limited roll-out's (Zout, event) -- a guarded sweep does not ask where its trajectory came from -- so that a pair differs in
the flag's code and the saturation record alone.
   python bench/rollout_limited_timing.py [B] [--out FILE]
   python bench/rollout_limited_timing.py [B] --unchanged-only [--label NAME] [--out FILE]
   python bench/rollout_limited_timing.py --combine FILE FILE ... --out profiles/rollout_limited_timing.json
--unchanged-only times the unlimited calls alone (each against itself, six rounds), and also loads a library built before the
limited entry points existed (QLN_LIB_PATH): their kernels' bodies gained a compile-time flag, and this is how the calls of
the commit before and of this one are timed in one session.  --combine files the runs' lines as one JSON document."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import _lib  # noqa: E402

UNCHANGED_ONLY = "--unchanged-only" in sys.argv
if UNCHANGED_ONLY:
    for _name in [s for s in _lib.SIGNATURES if "limited" in s]:
        del _lib.SIGNATURES[_name]  # a library from before this entry point has no such symbol to bind

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

from rollout_model_timing import Q, R, entry, pair_ms  # noqa: E402


def limits_from(Zref, k_trans, B, N):
    """No pull under a standing foot; caps at the 99th percentile of the plan's forces of the kind (init_mode 1: foot 1 stands,
    foot 2 is free up to and including the jump knot)."""
    z = torch.cat([Zref.view(B, -1)[:, : 20 * N - 5], torch.zeros(B, 5, dtype=Zref.dtype, device=Zref.device)], dim=1)
    F = z.view(B, N, 20)[:, : N - 1, 15:19].cpu().numpy()
    landed = np.broadcast_to(np.arange(N - 1)[None, :] > k_trans - 2, (B, N - 1))
    stand_y = np.concatenate([F[:, :, 1].ravel(), F[:, :, 3][landed]])
    stand_x = np.concatenate([F[:, :, 0].ravel(), F[:, :, 2][landed]])
    free_y, free_x = F[:, :, 3][~landed], F[:, :, 2][~landed]
    q = lambda a: float(np.percentile(np.abs(a[np.isfinite(a)]), 99.0))  # noqa: E731  (a diverged drop says nothing)
    return np.array([-q(free_x), q(free_x), -q(free_y), q(free_y), -q(stand_x), q(stand_x), 0.0, q(stand_y)])


def run(B, N, k_trans):
    torch.manual_seed(0)
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Zref = nlp.upload_Z(batch.Z)
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    model = nlp.plant_models()
    Zg, ev = nlp.tracking_rollout_guarded(Zref, K, None, model)
    Zm = nlp.tracking_rollout_model(Zref, K, None, model)
    dev = Zref.device
    zd, kd, Zbar = torch.randn_like(Zref), torch.randn_like(K), torch.randn_like(Zref)
    xd = torch.randn(B, 15, dtype=torch.float64, device=dev)
    md = model * torch.randn(B, 4, dtype=torch.float64, device=dev)
    zb, kb, xb, mb = nlp.tracking_rollout_guarded_vjp(Zref, Zg, ev, Zbar, K, model)
    out, ed, ev2 = nlp.new_Z(), torch.zeros_like(ev), torch.zeros_like(ev)
    Kout = torch.empty_like(K)
    Pout = torch.empty((B, N, _lib.TRACK_P_NNZ), dtype=torch.float64, device=dev)
    L = _lib.lib()
    d = lambda t: t.data_ptr()  # noqa: E731
    w = [a.ctypes.data for a in (Q, R, Q)]
    knots = B * (N - 1)
    h = nlp._h
    # the trajectory the sweeps and the designs run at: the unlimited roll-outs', or (below) the limited ones' for both of a pair
    Zt, evt, Zts = Zg, ev, Zm
    plain = {
        "rollout_guarded": (lambda: _lib.check(L.qln_tracking_rollout_guarded(h, d(Zref), d(K), None, d(model), d(out), d(ev2))),
                            "qln_tracking_rollout_guarded (K, model, events)", knots * 800 + B * 96),
        "rollout_model": (lambda: _lib.check(L.qln_tracking_rollout_model(h, d(Zref), d(K), None, d(model), d(out))),
                          "qln_tracking_rollout_model (K)", knots * 800 + B * 32),
        "jvp": (lambda: _lib.check(L.qln_tracking_rollout_guarded_jvp(h, d(Zref), d(K), d(Zt), d(model), d(evt), d(zd), d(kd), d(xd),
                                                                      d(md), d(out), d(ed))),
                "qln_tracking_rollout_guarded_jvp (K, all four tangents)", knots * 8 * 195 + B * 192),
        "vjp": (lambda: _lib.check(L.qln_tracking_rollout_guarded_vjp(h, d(Zref), d(K), d(Zt), d(model), d(evt), d(Zbar), d(zb),
                                                                      d(kb), d(xb), d(mb))),
                "qln_tracking_rollout_guarded_vjp (K, all four outputs)", knots * 8 * 195 + B * 128),
        "lqr_guarded": (lambda: _lib.check(L.qln_tracking_lqr_guarded(h, d(Zt), d(model), d(evt), *w, d(Kout), d(Pout))),
                        "qln_tracking_lqr_guarded (P)", knots * 8 * 200 + B * (960 + 96)),
        "lqr": (lambda: _lib.check(L.qln_tracking_lqr(h, d(Zts), *w, d(Kout), d(Pout))),
                "qln_tracking_lqr (P)", knots * 8 * 200 + B * 960),
    }
    res = {"B": B, "N": N, "k_trans": k_trans, "results": []}
    if UNCHANGED_ONLY:
        for key, (fn, name, byts) in plain.items():
            _, _, per_a, per_b = pair_ms(fn, fn)
            rounds = per_a + per_b
            res["results"].append(entry(name, float(np.median(rounds)), rounds, byts))
    else:
        lim = limits_from(Zref, k_trans, B, N)
        lp = lim.ctypes.data
        sat, sat_s, sat2 = (torch.zeros((B, N - 1), dtype=torch.float64, device=dev) for _ in range(3))
        Zl, Zs, evl = nlp.new_Z(), nlp.new_Z(), torch.zeros_like(ev)
        _lib.check(L.qln_tracking_rollout_limited(h, d(Zref), d(K), None, d(model), lp, 1, d(Zl), d(evl), d(sat)))
        _lib.check(L.qln_tracking_rollout_limited(h, d(Zref), d(K), None, d(model), lp, 0, d(Zs), None, d(sat_s)))
        torch.cuda.synchronize()
        Zt, evt, Zts = Zl, evl, Zs
        limited = {
            "rollout_guarded": (lambda: _lib.check(L.qln_tracking_rollout_limited(h, d(Zref), d(K), None, d(model), lp, 1, d(out),
                                                                                 d(ev2), d(sat2))),
                                "qln_tracking_rollout_limited (guarded, K, model, events, sat)"),
            "rollout_model": (lambda: _lib.check(L.qln_tracking_rollout_limited(h, d(Zref), d(K), None, d(model), lp, 0, d(out), None,
                                                                               d(sat2))),
                              "qln_tracking_rollout_limited (knot schedule, K, sat)"),
            "jvp": (lambda: _lib.check(L.qln_tracking_rollout_limited_jvp(h, d(Zref), d(K), d(Zl), d(model), d(evl), d(sat), d(zd),
                                                                          d(kd), d(xd), d(md), d(out), d(ed))),
                    "qln_tracking_rollout_limited_jvp (event, K, all four tangents)"),
            "vjp": (lambda: _lib.check(L.qln_tracking_rollout_limited_vjp(h, d(Zref), d(K), d(Zl), d(model), d(evl), d(sat), d(Zbar),
                                                                          d(zb), d(kb), d(xb), d(mb))),
                    "qln_tracking_rollout_limited_vjp (event, K, all four outputs)"),
            "lqr_guarded": (lambda: _lib.check(L.qln_tracking_lqr_limited(h, d(Zl), d(model), d(evl), d(sat), *w, d(Kout), d(Pout))),
                            "qln_tracking_lqr_limited (event, P)"),
            "lqr": (lambda: _lib.check(L.qln_tracking_lqr_limited(h, d(Zs), None, None, d(sat_s), *w, d(Kout), d(Pout))),
                    "qln_tracking_lqr_limited (knot schedule, P)"),
        }
        res["limited_over_sibling"] = {}
        for key, (fn, name, byts) in plain.items():
            fn_l, name_l = limited[key]
            ms_l, ms, per_l, per = pair_ms(fn_l, fn)
            res["results"] += [entry(name_l, ms_l, per_l, byts + knots * 8), entry(name, ms, per, byts)]
            res["limited_over_sibling"][key] = round(ms_l / ms, 4)
        codes = sat.cpu().numpy().astype(np.int64)
        digits = (codes[..., None] >> np.array([0, 2, 4, 6])) & 3
        res["limits"] = [round(float(x), 4) for x in lim]
        res["saturated_share"] = {"guarded": round(float((digits != 0).mean()), 4),
                                  "knot_schedule": round(float((sat_s != 0).double().mean()), 4),
                                  "touchdown_knot_moved": round(float((evl[:, 0] != ev[:, 0]).double().mean()), 4)}
    torch.cuda.synchronize()
    del nlp
    torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--unchanged-only"]
    out_path, label = None, "this commit"
    for flag in ("--out", "--label"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                out_path = args[i + 1]
            else:
                label = args[i + 1]
            del args[i:i + 2]
    if args and args[0] == "--combine":
        line = json.dumps({"runs": [json.loads(open(f).read()) for f in args[1:]]})
    else:
        B = int(args[0]) if args else 65536
        line = json.dumps({"iters": 20, "warmup": 3, "rounds": 3, "library": label, "unchanged_only": UNCHANGED_ONLY,
                           "configs": [run(B, 40, 14), run(B, 61, 21)]})
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
