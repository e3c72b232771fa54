"""Launch time of qln_tracking_rollout_estimated_jvp / _vjp and their _guarded forms (every tangent, cotangent and output,
ny = 8) beside the sweeps whose knot they apply twice, interleaved in the same run from the same library:
qln_tracking_rollout_model_jvp / _vjp and qln_tracking_rollout_guarded_jvp / _vjp (gains, models, every tangent and output).
The protocol of bench/tracking_estimated_timing.py: HIP events; per call the median of three rounds, each the median of 20
launches after 3 warm-ups, and the rounds' spread; B = 65 536, N = 40 and N = 61.  The floor beside each time is the compulsory
bytes over 8 TB/s: every input read once, every output written once.  Per problem at N = 40, ny = 8 the forward sweep reads
Zref, Zout and Zref_dot (795 doubles each), K and K_dot (2 340 each), L and L_dot (4 800 each), Xhat (600), innov (320), x0_dot,
xhat0_dot, the model and its tangent (38) and writes Zout_dot (795), Xhat_dot (600) and innov_dot (320): 154 704 B, of which
76 800 are the filter gains and their tangent; the reverse sweep moves the same arrays the other way round, and the guarded
forms 16 doubles of records (and 16 of their tangents) more.  The yardstick is twice the sibling sweep plus the filter-gain
traffic at 8 TB/s.  Prints one JSON line (kept as profiles/tracking_estimated_sweeps_timing.json).
   python bench/tracking_estimated_sweeps_timing.py [B]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, _lib, problem_gen as PG  # noqa: E402
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
    rnd = lambda t, s: s * torch.randn(t.shape, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    gen = torch.Generator(device="cuda").manual_seed(0)
    x0 = dev(batch.Z[:, :15] + 1e-3 * rng.normal(size=(B, 15)))
    xh0 = dev(batch.Z[:, :15] + 1e-3 * rng.normal(size=(B, 15)))
    model = nlp.plant_models()
    H = rng.normal(size=(NY, 15)) / np.sqrt(15.0)
    L = 1e-2 * torch.randn((B, N, 15, NY), dtype=torch.float64, device="cuda", generator=gen)
    v = 1e-3 * torch.randn((B, N, NY), dtype=torch.float64, device="cuda", generator=gen)
    w = 1e-4 * torch.randn((B, N - 1, 15), dtype=torch.float64, device="cuda", generator=gen)
    # the trajectories the sweeps run along: the siblings' roll-outs and the estimate-feedback ones
    Zm = nlp.tracking_rollout_model(Z, K, x0, model)
    Zg, evg = nlp.tracking_rollout_guarded(Z, K, x0, model)
    Zo, Xh, iv = nlp.tracking_rollout_estimated(Z, K, L, H, v, w, x0, xh0, model, with_innovations=True)
    Zog, Xhg, ivg, ev, eh = nlp.tracking_rollout_estimated(Z, K, L, H, v, w, x0, xh0, model, guarded=True, with_innovations=True)
    landed = (float((ev[:, 0] >= 0).double().mean()), float((eh[:, 0] >= 0).double().mean()))
    # tangents, cotangents and preallocated outputs: the C entry points, so that no wrapper's allocation is timed
    zd, kd, Ld = rnd(Z, 1e-2), rnd(K, 1e-2), rnd(L, 1e-2)
    xd, hd, md = rnd(x0, 1e-2), rnd(x0, 1e-2), rnd(model, 1e-3)
    zbar, xbar, ibar = rnd(Z, 1e-2), rnd(Xh, 1e-2), rnd(iv, 1e-2)
    oz, oX, oi = nlp.new_Z(), torch.zeros_like(Xh), torch.zeros_like(iv)
    oK, oL, ox, oh, om = torch.zeros_like(K), torch.zeros_like(L), torch.zeros_like(x0), torch.zeros_like(x0), torch.zeros_like(model)
    oe, oeh = torch.zeros_like(ev), torch.zeros_like(ev)
    Hd = dev(H)
    lib, p = _lib.lib(), lambda t: t.data_ptr()  # noqa: E731
    nz, nk, nl, nx, ni = 8 * B * nlp.n_nlp, 8 * K.numel(), 8 * L.numel(), 8 * Xh.numel(), 8 * iv.numel()
    small, rec = 8 * B * 15, 64 * B
    sib_j = 4 * nz + 2 * nk + small + 64 * B      # Zref, Zout, Zref_dot, Zout_dot; K, K_dot; x0_dot; model and model_dot
    sib_v = 4 * nz + 2 * nk + small + 64 * B      # Zref, Zout, Zbar, Zref_bar; K, K_bar; x0_bar; model and model_bar
    est = 4 * nz + 2 * nk + 2 * nl + 2 * nx + 2 * ni + 2 * small + 64 * B
    ck = _lib.check
    calls = [
        ("qln_tracking_rollout_model_jvp",
         lambda: ck(lib.qln_tracking_rollout_model_jvp(nlp._h, p(Z), p(K), p(Zm), p(model), p(zd), p(kd), p(xd), p(md), p(oz))), sib_j),
        ("qln_tracking_rollout_model_vjp",
         lambda: ck(lib.qln_tracking_rollout_model_vjp(nlp._h, p(Z), p(K), p(Zm), p(model), p(zbar), p(oz), p(oK), p(ox), p(om))), sib_v),
        ("qln_tracking_rollout_guarded_jvp",
         lambda: ck(lib.qln_tracking_rollout_guarded_jvp(nlp._h, p(Z), p(K), p(Zg), p(model), p(evg), p(zd), p(kd), p(xd), p(md), p(oz),
                                                         p(oe))), sib_j + 2 * rec),
        ("qln_tracking_rollout_guarded_vjp",
         lambda: ck(lib.qln_tracking_rollout_guarded_vjp(nlp._h, p(Z), p(K), p(Zg), p(model), p(evg), p(zbar), p(oz), p(oK), p(ox),
                                                         p(om))), sib_v + rec),
        ("qln_tracking_rollout_estimated_jvp",
         lambda: ck(lib.qln_tracking_rollout_estimated_jvp(nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(model), p(Zo), p(Xh), p(iv), p(zd), p(kd),
                                                           p(Ld), p(xd), p(hd), p(md), p(oz), p(oX), p(oi))), est),
        ("qln_tracking_rollout_estimated_vjp",
         lambda: ck(lib.qln_tracking_rollout_estimated_vjp(nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(model), p(Zo), p(Xh), p(iv), p(zbar),
                                                           p(xbar), p(ibar), p(oz), p(oK), p(oL), p(ox), p(oh), p(om))), est),
        ("qln_tracking_rollout_estimated_guarded_jvp",
         lambda: ck(lib.qln_tracking_rollout_estimated_guarded_jvp(nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(model), p(Zog), p(Xhg), p(ivg),
                                                                   p(ev), p(eh), p(zd), p(kd), p(Ld), p(xd), p(hd), p(md), p(oz), p(oX),
                                                                   p(oi), p(oe), p(oeh))), est + 4 * rec),
        ("qln_tracking_rollout_estimated_guarded_vjp",
         lambda: ck(lib.qln_tracking_rollout_estimated_guarded_vjp(nlp._h, p(Z), p(K), p(L), p(Hd), NY, p(model), p(Zog), p(Xhg), p(ivg),
                                                                   p(ev), p(eh), p(zbar), p(xbar), p(ibar), p(oz), p(oK), p(oL), p(ox),
                                                                   p(oh), p(om))), est + 2 * rec),
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
    t = {r["call"]: r["ms"] for r in res}
    gain_ms = 2 * nl / PEAK * 1e3  # the filter gains and their tangent or cotangent at peak bandwidth
    cfg = {"B": B, "N": N, "k_trans": k_trans, "ny": NY, "landed_plant_estimator": landed,
           "filter_gain_bytes_per_problem": int(2 * nl // B), "filter_gain_floor_ms": round(gain_ms, 4), "results": res}
    for g in ("", "guarded_"):
        sib = "guarded" if g else "model"
        for s in ("jvp", "vjp"):
            yard = 2 * t[f"qln_tracking_rollout_{sib}_{s}"] + gain_ms
            cfg[f"estimated_{g}{s}_over_yardstick"] = round(t[f"qln_tracking_rollout_estimated_{g}{s}"] / yard, 4)
    del K, Z, L, Ld, oL, nlp
    torch.cuda.empty_cache()
    return cfg


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 65536
    print(json.dumps({"library": os.path.basename(_lib.LIB_PATH), "iters": 20, "warmup": 3, "rounds": ROUNDS,
                      "yardstick": "2 x the sibling sweep + the filter gains' bytes at peak",
                      "configs": [run(B, 40, 14), run(B, 61, 21)]}))
