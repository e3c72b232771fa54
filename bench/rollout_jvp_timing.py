"""Launch time of qln_tracking_rollout_jvp (HIP events, median of 20 launches after 3 warm-ups) at B = 65 536, N = 40 and
N = 61: with TVLQR gains and all three tangents, with gains and x0_dot alone, and with K == NULL and Zref_dot; in the same
run, qln_tracking_rollout_vjp with gains and all outputs (the yardstick: the all-tangents call may take at most 1.10 x its
time) and qln_tracking_rollout.  Bytes per knot over 8 TB/s: all tangents read Zout (20 doubles), Zref's states (15), K and
K_dot (60 each) and Zref_dot (20) and write Zout_dot (20), 1 560 B as the reverse sweep with all outputs; x0_dot alone reads
Zout and K and writes Zout_dot, 800 B; K == NULL reads Zout and Zref_dot and writes Zout_dot, 480 B.  Prints one JSON line
and writes it to the file named by --out.
   python bench/rollout_jvp_timing.py [B] [--out profiles/rollout_jvp_timing.json]"""
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
BAR = 1.10     # all tangents against the reverse sweep with K and all outputs, same run


def t_ms(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def entry(name, ms, byts):
    t_bw = byts / PEAK * 1e3
    return {"call": name, "ms": round(ms, 4), "bytes": int(byts), "hbm_floor_ms": round(t_bw, 4),
            "frac_of_peak": round(t_bw / ms, 4)}


def run(B, N, k_trans):
    batch = PG.make_batch(B, N, k_trans, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Zref = nlp.upload_Z(batch.Z)
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    Zout = nlp.tracking_rollout(Zref, K)
    Zbar = torch.randn_like(Zout)
    zd, kd = torch.randn_like(Zref), torch.randn_like(K)
    xd = torch.randn(B, 15, dtype=torch.float64, device=Zref.device)
    zb, kb, xb = nlp.tracking_rollout_vjp(Zref, Zout, Zbar, K)
    out = nlp.new_Z()
    L = _lib.lib()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    jvp = lambda k, z, kk, x: _lib.check(L.qln_tracking_rollout_jvp(  # noqa: E731
        nlp._h, Zref.data_ptr(), p(k), Zout.data_ptr(), p(z), p(kk), p(x), out.data_ptr()))
    vjp = lambda: _lib.check(L.qln_tracking_rollout_vjp(  # noqa: E731
        nlp._h, Zref.data_ptr(), K.data_ptr(), Zout.data_ptr(), Zbar.data_ptr(), zb.data_ptr(), kb.data_ptr(), xb.data_ptr()))
    knots = B * (N - 1)
    res = [entry("qln_tracking_rollout_jvp (K, all tangents)", t_ms(lambda: jvp(K, zd, kd, xd)), knots * 8 * 195),
           entry("qln_tracking_rollout_jvp (K, x0_dot only)", t_ms(lambda: jvp(K, None, None, xd)), knots * 8 * 100),
           entry("qln_tracking_rollout_jvp (K == NULL, Zref_dot)", t_ms(lambda: jvp(None, zd, None, None)), knots * 8 * 60),
           entry("qln_tracking_rollout_vjp (K, all outputs)", t_ms(vjp), knots * 8 * 195),
           entry("qln_tracking_rollout (forward, K)", t_ms(lambda: nlp.tracking_rollout(Zref, K, None, Zout)),
                 knots * 8 * 100)]
    ratio = res[0]["ms"] / res[3]["ms"]
    del K, Zout, Zbar, zd, kd, xd, zb, kb, xb, out, Zref, nlp
    torch.cuda.empty_cache()
    return {"B": B, "N": N, "k_trans": k_trans, "results": res, "jvp_over_vjp": round(ratio, 4), "bar": BAR,
            "met": ratio <= BAR}


if __name__ == "__main__":
    args = sys.argv[1:]
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    B = int(args[0]) if args else 65536
    line = json.dumps({"iters": 20, "warmup": 3, "configs": [run(B, 40, 14), run(B, 61, 21)]})
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
