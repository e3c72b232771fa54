"""Launch time of qln_tracking_rollout_estimated_limited and its two sweeps, knot-scheduled and guarded (every input, tangent,
cotangent and output, ny = 8), beside their unlimited siblings -- qln_tracking_rollout_estimated / _guarded and their _jvp /
_vjp -- interleaved in the same run from the same library.  The protocol of bench/tracking_estimated_timing.py: HIP events; per
call the median of three rounds, each the median of 20 launches after 3 warm-ups, and the rounds' spread; B = 65 536, N = 40
and N = 61.  The limits are the tests' (tests/rollout_limited_ref.TEST_LIMITS); the share of (knot, channel) pairs they hold is
printed with the times.  The limited calls move what their siblings move, plus the saturation record: B (N - 1) doubles written
by the roll-out and read by a sweep.  Prints one JSON line (kept as profiles/tracking_estimated_limited_timing.json).
   python bench/tracking_estimated_limited_timing.py [B]
   QLN_LIB_PATH=<another build of libqln_hip.so> python bench/tracking_estimated_limited_timing.py --siblings [B]
The second form times only the six unlimited calls, for a library that does not have the new entry points (the parent's): run
in the same session, its times say whether the flag cost the existing paths anything."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import _lib  # noqa: E402

SIBLINGS_ONLY = "--siblings" in sys.argv
if SIBLINGS_ONLY:  # the other library is asked for the symbols it has
    for name in [s for s in _lib.SIGNATURES if s.startswith("qln_tracking_rollout_estimated_limited")]:
        del _lib.SIGNATURES[name]

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402
from tracking_timing import PEAK, Q, R, t_ms  # noqa: E402

ROUNDS = 3
NY = 8
LIMITS = np.array([-0.3, 0.3, -0.05, 49.5, -0.4, 0.4, 48.6, 98.15])


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Z = nlp.upload_Z(batch.Z)
    K, _ = nlp.tracking_lqr(Z, Q, R, Q, with_cost_to_go=False)
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rnd = lambda t, s: s * torch.randn(t.shape, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    x0 = dev(batch.Z[:, :15] + 1e-3 * rng.normal(size=(B, 15)))
    xh0 = dev(batch.Z[:, :15] + 1e-3 * rng.normal(size=(B, 15)))
    model = nlp.plant_models()
    H = rng.normal(size=(NY, 15)) / np.sqrt(15.0)
    L = 1e-2 * torch.randn((B, N, 15, NY), dtype=torch.float64, device="cuda", generator=gen)
    v = 1e-3 * torch.randn((B, N, NY), dtype=torch.float64, device="cuda", generator=gen)
    w = 1e-4 * torch.randn((B, N - 1, 15), dtype=torch.float64, device="cuda", generator=gen)
    # the trajectories the sweeps run along
    Zo, Xh, iv = nlp.tracking_rollout_estimated(Z, K, L, H, v, w, x0, xh0, model, with_innovations=True)
    Zog, Xhg, ivg, ev, eh = nlp.tracking_rollout_estimated(Z, K, L, H, v, w, x0, xh0, model, guarded=True, with_innovations=True)
    zd, kd, Ld = rnd(Z, 1e-2), rnd(K, 1e-2), rnd(L, 1e-2)
    xd, hd, md = rnd(x0, 1e-2), rnd(x0, 1e-2), rnd(model, 1e-3)
    zbar, xbar, ibar = rnd(Z, 1e-2), rnd(Xh, 1e-2), rnd(iv, 1e-2)
    out, oX, oi = nlp.new_Z(), torch.zeros_like(Xh), torch.zeros_like(iv)
    oK, oL, ox, oh, om = torch.zeros_like(K), torch.zeros_like(L), torch.zeros_like(x0), torch.zeros_like(x0), torch.zeros_like(model)
    oe, oeh, osat = torch.zeros_like(ev), torch.zeros_like(ev), torch.zeros((B, N - 1), dtype=torch.float64, device="cuda")
    Hd = dev(H)
    lib, p, ck = _lib.lib(), (lambda t: t.data_ptr()), _lib.check
    nz, nk, nl, nx, ni = 8 * B * nlp.n_nlp, 8 * K.numel(), 8 * L.numel(), 8 * Xh.numel(), 8 * iv.numel()
    small, rec, ns = 8 * B * 15, 64 * B, 8 * B * (N - 1)
    roll = 2 * nz + nk + nl + 2 * ni + 8 * w.numel() + nx + 2 * small + 32 * B
    sweep = 4 * nz + 2 * nk + 2 * nl + 2 * nx + 2 * ni + 2 * small + 64 * B
    head = (nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(v), p(w), p(x0), p(xh0), p(model))
    traj = (nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(model), p(Zo), p(Xh), p(iv))
    trajg = (nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(model), p(Zog), p(Xhg), p(ivg), p(ev), p(eh))
    tang = (p(zd), p(kd), p(Ld), p(xd), p(hd), p(md), p(out), p(oX), p(oi))
    cot = (p(zbar), p(xbar), p(ibar), p(out), p(oK), p(oL), p(ox), p(oh), p(om))
    calls = [
        ("qln_tracking_rollout_estimated", lambda: ck(lib.qln_tracking_rollout_estimated(*head, p(out), p(oX), p(oi))), roll),
        ("qln_tracking_rollout_estimated_guarded",
         lambda: ck(lib.qln_tracking_rollout_estimated_guarded(*head, p(out), p(oX), p(oi), p(oe), p(oeh))), roll + 2 * rec),
        ("qln_tracking_rollout_estimated_jvp", lambda: ck(lib.qln_tracking_rollout_estimated_jvp(*traj, *tang)), sweep),
        ("qln_tracking_rollout_estimated_guarded_jvp",
         lambda: ck(lib.qln_tracking_rollout_estimated_guarded_jvp(*trajg, *tang, p(oe), p(oeh))), sweep + 4 * rec),
        ("qln_tracking_rollout_estimated_vjp", lambda: ck(lib.qln_tracking_rollout_estimated_vjp(*traj, *cot)), sweep),
        ("qln_tracking_rollout_estimated_guarded_vjp", lambda: ck(lib.qln_tracking_rollout_estimated_guarded_vjp(*trajg, *cot)),
         sweep + 2 * rec),
    ]
    shares = None
    if not SIBLINGS_ONLY:
        from quadruped_landing_amd.nlp import unpack_saturation

        # the limited trajectories, and their records
        Zl, Xl, il, _, _, sat = nlp.tracking_rollout_estimated_limited(Z, LIMITS, K, L, H, v, w, x0, xh0, model, with_innovations=True)
        Zlg, Xlg, ilg, evl, ehl, satg = nlp.tracking_rollout_estimated_limited(Z, LIMITS, K, L, H, v, w, x0, xh0, model, guarded=True,
                                                                              with_innovations=True)
        shares = [float((unpack_saturation(s) != 0).mean()) for s in (sat, satg)]
        lim = LIMITS.ctypes.data
        trl = (nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(model), p(Zl), p(Xl), p(il), None, None, p(sat))
        trlg = (nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(model), p(Zlg), p(Xlg), p(ilg), p(evl), p(ehl), p(satg))
        calls += [
            ("qln_tracking_rollout_estimated_limited",
             lambda: ck(lib.qln_tracking_rollout_estimated_limited(*head, lim, 0, p(out), p(oX), p(oi), None, None, p(osat))), roll + ns),
            ("qln_tracking_rollout_estimated_limited guarded",
             lambda: ck(lib.qln_tracking_rollout_estimated_limited(*head, lim, 1, p(out), p(oX), p(oi), p(oe), p(oeh), p(osat))),
             roll + 2 * rec + ns),
            ("qln_tracking_rollout_estimated_limited_jvp",
             lambda: ck(lib.qln_tracking_rollout_estimated_limited_jvp(*trl, *tang, None, None)), sweep + ns),
            ("qln_tracking_rollout_estimated_limited_jvp guarded",
             lambda: ck(lib.qln_tracking_rollout_estimated_limited_jvp(*trlg, *tang, p(oe), p(oeh))), sweep + 4 * rec + ns),
            ("qln_tracking_rollout_estimated_limited_vjp", lambda: ck(lib.qln_tracking_rollout_estimated_limited_vjp(*trl, *cot)),
             sweep + ns),
            ("qln_tracking_rollout_estimated_limited_vjp guarded",
             lambda: ck(lib.qln_tracking_rollout_estimated_limited_vjp(*trlg, *cot)), sweep + 2 * rec + ns),
        ]
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
        cfg["on_a_limit_scheduled_guarded"] = [round(s, 4) for s in shares]
        t = {r["call"]: r["ms"] for r in res}
        for i in range(6):
            cfg["limited_over_sibling: " + calls[6 + i][0]] = round(t[calls[6 + i][0]] / t[calls[i][0]], 4)
    del K, Z, L, Ld, oL, nlp
    torch.cuda.empty_cache()
    return cfg


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 65536
    print(json.dumps({"library": os.path.basename(_lib.LIB_PATH), "siblings_only": SIBLINGS_ONLY, "iters": 20, "warmup": 3,
                      "rounds": ROUNDS, "limits": LIMITS.tolist(), "configs": [run(B, 40, 14), run(B, 61, 21)]}))
