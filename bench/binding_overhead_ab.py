"""What the Python binding costs per call of the tracking and landing section, A/B between two checkouts.

    python bench/binding_overhead_ab.py --parent PATH [--rounds 6] [--out profiles/binding_overhead_ab.txt]
        alternates the checkout at PATH and this tree in fresh child processes, one at a time and each under its own timeout,
        `rounds` times each, and writes per method the median and the spread (max - min) over the rounds, in us per call, and
        the bar: this tree's median no higher than the other's median plus the other's own round-to-round spread.  Both
        children load this tree's libqln_hip.so (QLN_LIB_PATH), so only the Python between the caller and the C ABI differs.
    python bench/binding_overhead_ab.py --child --tree PATH
        one child: 2 000 back-to-back calls followed by one synchronize() of each method, at B = 64, N = 40, where the kernels
        are short and a call is host-bound (but for tracking_rollout, whose kernel's 150 us bound it); prints one JSON line
        {method: us per call}.  Public methods only, so that it runs on any checkout.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, NY, CALLS, WARM = 64, 40, 3, 2000, 200
METHODS = ("tracking_rollout", "tracking_rollout_guarded_vjp", "landing_filter_vjp", "tracking_rollout_host")


def child(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch

    from quadruped_landing_amd import HybridNLP, problem_gen as PG

    b = PG.make_batch(B, N, 14, 1, seed=B)
    nlp = HybridNLP(b.model, b.obj, b.init_mode, b.k_trans, b.N, b.x0, b.xf)
    rng = np.random.default_rng(B)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    Kh = 0.05 * rng.normal(size=(B, N - 1, 4, 15))
    x0h = b.Z[:, :15] + 1e-2 * rng.normal(size=(B, 15))
    Zref, K, x0 = nlp.upload_Z(b.Z), dev(Kh), dev(x0h)
    Zbar = nlp.upload_Z(rng.normal(size=(B, nlp.n_nlp)))
    Zout = nlp.tracking_rollout(Zref, K, x0)
    Zg, ev = nlp.tracking_rollout_guarded(Zref, K, x0)
    H, V = rng.normal(size=(NY, 15)) / np.sqrt(15.0), np.full(NY, 1e-5)
    Lg = nlp.tracking_kalman(Zout, H, V, K, Sigma0=np.full(15, 1e-6), with_sigma=False, with_marginals=False)[0]
    Xf = nlp.landing_filter(Zref, Zout, Lg, H, nlp.landing_measurements(Zout, Zref, H))[0]
    Xbar = dev(rng.normal(size=(B, N, 15)))
    Zh = np.ascontiguousarray(b.Z, dtype=np.float64)
    calls = {
        "tracking_rollout": lambda: nlp.tracking_rollout(Zref, K, x0),
        "tracking_rollout_guarded_vjp": lambda: nlp.tracking_rollout_guarded_vjp(Zref, Zg, ev, Zbar, K),
        "landing_filter_vjp": lambda: nlp.landing_filter_vjp(Zref, Zout, Lg, H, Xf, Xhat_bar=Xbar),
        "tracking_rollout_host": lambda: nlp.tracking_rollout_host(Zh, Kh, x0h),
    }
    out = {}
    for name in METHODS:
        fn = calls[name]
        for _ in range(WARM):
            fn()
        nlp.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        nlp.synchronize()
        out[name] = 1e6 * (time.perf_counter() - t0) / CALLS
    torch.cuda.synchronize()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binding_overhead_ab.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a.tree)
    trees = {"parent": os.path.abspath(a.parent), "new": ROOT}
    env = dict(os.environ, QLN_LIB_PATH=os.path.join(ROOT, "quadruped_landing_amd", "csrc", "libqln_hip.so"))
    runs = {k: [] for k in trees}
    for rnd in range(a.rounds):
        for k, tree in trees.items():  # a child that fails ends the run: nothing more is started on the device
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree], env=env, cwd=tree,
                                 check=True, capture_output=True, text=True, timeout=240)
            runs[k].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(rnd, k, runs[k][-1], flush=True)
    lines = [f"us per call, {CALLS} back-to-back calls and one synchronize(), B = {B}, N = {N}; {a.rounds} alternating rounds",
             f"{'method':32s} {'parent median':>14s} {'spread':>8s} {'new median':>11s} {'spread':>8s} {'bar':>8s}  within"]
    ok = True
    for m in METHODS:
        p, q = [r[m] for r in runs["parent"]], [r[m] for r in runs["new"]]
        bar = statistics.median(p) + (max(p) - min(p))
        within = statistics.median(q) <= bar
        ok &= within
        lines.append(f"{m:32s} {statistics.median(p):14.2f} {max(p) - min(p):8.2f} {statistics.median(q):11.2f} "
                     f"{max(q) - min(q):8.2f} {bar:8.2f}  {'yes' if within else 'NO'}")
    lines.append("tracking_rollout's kernel takes 150 us at this size (profiles/tracking_host_layer_ab.txt), more than the host's "
                 "share of a call: its row shows the kernel, not the binding.  The two sweeps and the host form are host-bound.")
    lines.append("rounds: " + json.dumps(runs))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
