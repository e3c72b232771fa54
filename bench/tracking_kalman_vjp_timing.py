"""Launch time of qln_noise_design_vjp (every cotangent and output, ny = 8), scheduled and guarded, beside the calls whose work it
shares, interleaved in the same run on the same box: qln_kalman_design_jvp (the forward sweep: the same gain traffic),
qln_tracking_kalman, the filter alone, and qln_landing_smoother with both outputs (the same transposed two-sided applications).
HIP events; per call the median of three rounds, each the median of 20 launches after 3 warm-ups, and the rounds' spread;
B = 65 536, N = 40 and N = 61.  The floor beside each time is the compulsory bytes over 8 TB/s: every input read once, every output
written once.  Prints one JSON line (kept as profiles/tracking_kalman_vjp_timing.json).
   python bench/tracking_kalman_vjp_timing.py [B] [--parent <a build of the parent commit's libqln_hip.so>]
   QLN_LIB_PATH=<another build of libqln_hip.so> python bench/tracking_kalman_vjp_timing.py --siblings [B]
The second form times only the three sibling calls, for a library that may not have the new entry points.  --parent runs it in a
fresh process on that library between this build's rounds' end and the report, in the same session, and keeps its result beside
this build's: the two builds' siblings must agree within the rounds' spread."""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import _lib  # noqa: E402

SIBLINGS_ONLY = "--siblings" in sys.argv
if SIBLINGS_ONLY:  # the other library is asked for the symbols it has
    for name in [s for s in _lib.SIGNATURES if s.startswith("qln_noise_design")]:
        del _lib.SIGNATURES[name]

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402
from tracking_timing import PEAK, Q, R, t_ms  # noqa: E402

ROUNDS = 3
NY = 8


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Z = nlp.upload_Z(batch.Z)
    rng = np.random.default_rng(0)
    G = rng.normal(size=(15, 15))
    s0 = torch.from_numpy(np.ascontiguousarray((G @ G.T / 15)[np.tril_indices(15)])).cuda()
    W = rng.uniform(0.0, 1e-3, size=15)
    H, V = rng.normal(size=(NY, 15)) / np.sqrt(15.0), rng.uniform(0.5, 2.0, size=NY)
    Hs = rng.normal(size=(15, 15)) / np.sqrt(15.0)
    s0d = torch.from_numpy(np.ascontiguousarray((Hs + Hs.T)[np.tril_indices(15)])).cuda()
    Wd, Vd = 1e-3 * rng.normal(size=15), rng.normal(size=NY)
    L, Pe = nlp.tracking_kalman(Z, H, V, None, s0, W)[:2]
    gen = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    Xhat, innov = rand(B, N, 15), rand(B, N, NY)
    zb, lb, pb, xb, ib, nb = 8 * B * nlp.n_nlp, 8 * L.numel(), 8 * Pe.numel(), 8 * Xhat.numel(), 8 * innov.numel(), 8 * B * N
    calls = [("qln_kalman_design_jvp (Lgain_dot, Pest_dot, logdet_dot)", lambda: nlp.tracking_kalman_jvp(Z, L, H, V, s0d, Wd, Vd),
              zb + 2 * lb + pb + nb),
             ("qln_tracking_kalman (filter alone: L, Pest)", lambda: nlp.tracking_kalman(Z, H, V, None, s0, W), zb + lb + pb),
             ("qln_landing_smoother (Xs and Ps)", lambda: nlp.landing_smoother(Z, L, Pe, H, V, Xhat, innov),
              zb + lb + 2 * pb + 2 * xb + ib)]
    if not SIBLINGS_ONLY:
        Lb, Pb, lgb = rand(B, N, 15, NY), rand(B, N, 120), rand(B, N)
        K, _ = nlp.tracking_lqr(Z, Q, R, Q, with_cost_to_go=False)
        Zg, ev = nlp.tracking_rollout_guarded(Z, K, None, None)
        Lg = nlp.tracking_kalman_guarded(Zg, ev, H, V, None, s0, W, None)[0]
        del K
        byts = zb + 2 * lb + pb + nb + 8 * B * (120 + 15 + NY)
        calls.append(("qln_noise_design_vjp (Sigma0_bar, Wdiag_bar, Vdiag_bar)",
                      lambda: nlp.tracking_kalman_vjp(Z, L, H, V, Lb, Pb, lgb), byts))
        calls.append(("qln_noise_design_guarded_vjp (Sigma0_bar, Wdiag_bar, Vdiag_bar)",
                      lambda: nlp.tracking_kalman_vjp(Zg, Lg, H, V, Lb, Pb, lgb, events=ev, guarded=True), byts))
    ms = {name: [] for name, _, _ in calls}
    for _ in range(ROUNDS):  # interleaved: every round times every call
        for name, fn, _ in calls:
            ms[name].append(t_ms(fn))
    res = []
    for name, _, byts in calls:
        med, floor = float(np.median(ms[name])), byts / PEAK * 1e3
        res.append({"call": name, "ms": round(med, 4), "rounds_ms": [round(v, 4) for v in ms[name]], "bytes": int(byts),
                    "bytes_per_problem": int(byts // B), "hbm_floor_ms": round(floor, 4), "frac_of_peak": round(floor / med, 4)})
    out = {"B": B, "N": N, "k_trans": k_trans, "ny": NY, "results": res}
    if not SIBLINGS_ONLY:
        out["vjp_over_forward_sweep"] = round(res[3]["ms"] / res[0]["ms"], 4)
        out["vjp_over_filter_alone"] = round(res[3]["ms"] / res[1]["ms"], 4)
        out["vjp_over_smoother"] = round(res[3]["ms"] / res[2]["ms"], 4)
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    parent = argv[argv.index("--parent") + 1] if "--parent" in argv else None
    args = [a for a in argv if not a.startswith("--") and a != parent]
    B = int(args[0]) if args else 65536
    doc = {"library": os.path.basename(_lib.LIB_PATH), "siblings_only": SIBLINGS_ONLY, "iters": 20, "warmup": 3, "rounds": ROUNDS,
           "configs": [run(B, 40, 14), run(B, 61, 21)]}
    if parent and not SIBLINGS_ONLY:
        torch.cuda.synchronize()
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--siblings", str(B)], capture_output=True, text=True,
                               env=dict(os.environ, QLN_LIB_PATH=os.path.abspath(parent)), timeout=600, check=True)
        doc["parent_build"] = json.loads(child.stdout.strip().splitlines()[-1])
    print(json.dumps(doc))
