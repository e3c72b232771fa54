"""The host-side cost of the qln_tracking_* entry points, A/B between two builds of the library, and the copies their host
forms make.

    python bench/tracking_host_layer_ab.py --other PATH/libqln_hip_other.so [--rounds 5]
        alternates the other build and this tree's build in fresh child processes, `rounds` times each, and prints per figure
        the median and the spread (max - min) of each build over its rounds:
          enqueue_us   wall time per call of 1 000 back-to-back qln_tracking_rollout device-form calls (B = 64, N = 40), ending in
                       one synchronisation (the kernel's 150 us per call bound it when this was written)
          issue_us     the same loop up to its last call's return, before the synchronisation: the host's share
          mapped_us    wall time per call of qln_tracking_rollout_estimated_limited_jvp_host, the entry point with the most
                       arguments, at B = 5, N = 40 (mapped host memory)
          staged_us    the same at B = 64, N = 40 on the padded layout that is staged through device memory
    python bench/tracking_host_layer_ab.py --child time      one child: the three figures of the build QLN_LIB_PATH selects
    python bench/tracking_host_layer_ab.py --child copies    calls every tracking host form once on the staged layout; run it under
        rocprofv3 --memory-copy-trace --output-format json -d DIR -- python bench/tracking_host_layer_ab.py --child copies
    python bench/tracking_host_layer_ab.py --summarise DIR   the copies of such a trace in start order, "direction bytes" per line
"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, NY = 40, 3
Z_STRIDE = 3000  # 64 problems of 40 knots are 7.4 MB and mapped; padded to this they are 8.5 MB, past the switch at 8 MiB
LIMITS = np.array([-0.3, 0.3, -0.05, 49.5, -0.4, 0.4, 48.6, 98.15])


class Session:
    """A handle on B problems and host inputs for every tracking entry point, by the header's parameter names."""

    def __init__(self, B, z_stride=0):
        from quadruped_landing_amd import HybridNLP, problem_gen as PG
        from tests import tracking_abi as TA

        self.TA, self.B = TA, B
        b = PG.make_batch(B, N, 14, 1, seed=B)
        self.nlp = HybridNLP(b.model, b.obj, b.init_mode, b.k_trans, b.N, b.x0, b.xf, z_stride=z_stride)
        rng = np.random.default_rng(B)
        n, zs = self.nlp.n_nlp, self.nlp.z_stride

        def like_Z(rows):
            z = np.zeros((B, zs))
            z[:, :n] = rows
            return z.reshape(-1)

        x0 = b.Z[:, :15] + 1e-2 * rng.normal(size=(B, 15))
        th = np.tile(np.array(b.model.plant_parameters()), (B, 1))
        eye = np.tile(1e-6 * np.eye(15)[np.tril_indices(15)], (B, 1))
        self.v = dict(
            Zref=like_Z(b.Z), K=0.05 * rng.normal(size=(B, N - 1, 4, 15)), x0=x0, model=th, lim=LIMITS, guarded=1, ny=NY,
            sigma0_batch=B, Qdiag=np.array([10.0] * 14 + [0.7]), Rdiag=np.array([1e-3, 1e-2, 1e-3, 1e-2]),
            Qfdiag=np.array([30.0] * 14 + [2.0]), Wdiag=np.full(15, 1e-3), Vdiag=np.full(8, 1e-5), Sigma0=eye,
            Lgain=0.01 * rng.normal(size=(B, N, 15, NY)), H=rng.normal(size=(NY, 15)) / np.sqrt(15.0),
            vnoise=1e-3 * rng.normal(size=(B, N, NY)), wnoise=1e-4 * rng.normal(size=(B, N - 1, 15)),
            xhat0=x0 + 1e-2 * rng.normal(size=(B, 15)), Zref_dot=like_Z(rng.normal(size=(B, n))),
            K_dot=rng.normal(size=(B, N - 1, 4, 15)), x0_dot=rng.normal(size=(B, 15)), model_dot=th * rng.normal(size=(B, 4)),
            Lgain_dot=rng.normal(size=(B, N, 15, NY)), xhat0_dot=rng.normal(size=(B, 15)), Zbar=like_Z(rng.normal(size=(B, n))),
            Xhat_bar=rng.normal(size=(B, N, 15)), innov_bar=rng.normal(size=(B, N, NY)))

    def arguments(self, name, outs, device=False, **more):
        """parameter -> value of one call: host arrays (device tensors with device=True), fresh zeros for the outputs"""
        import torch

        TA, vals = self.TA, {}
        for p in TA.PARAMS[name]:
            if p in outs:
                vals[p] = np.zeros(TA.size(p, self.B, N, self.nlp.dims.z_total))
            else:
                v = more[p] if p in more else self.v[p]
                vals[p] = v if TA.is_int(name, p) else np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
            if device and isinstance(vals[p], np.ndarray) and p not in TA.HOST_ONLY:
                vals[p] = torch.from_numpy(vals[p]).cuda()
        return vals

    def call(self, name, vals):
        from quadruped_landing_amd import _lib

        _lib.check(self.TA.call(self.nlp._h, name, vals))

    def bound(self, name, vals):
        """The call as a closure over its ctypes arguments, so that a timing loop pays for nothing else."""
        TA, fn = self.TA, getattr(self.TA._lib.lib(), name)
        args = [self.nlp._h] + [vals[p] if TA.is_int(name, p) else TA.address(vals[p]) for p in TA.PARAMS[name]]
        return lambda: fn(*args)

    def host(self, name, outs, **more):
        vals = self.arguments(name + "_host", outs, **more)
        self.call(name + "_host", vals)
        return {p: vals[p] for p in outs}


def every_host_form(s):
    """Calls each of the 28 tracking host forms once."""
    r = "qln_tracking_rollout"
    sweeps = lambda stem, events, **t: (  # noqa: E731
        s.host(stem + "_jvp", ("Zout_dot",) + events, **t), s.host(stem + "_vjp", ("Zref_bar", "K_bar", "x0_bar", "model_bar"), **t))
    plain, model = s.host(r, ("Zout",)), s.host(r + "_model", ("Zout",))
    g, lim = s.host(r + "_guarded", ("Zout", "event")), s.host(r + "_limited", ("Zout", "event", "sat"))
    s.host(r + "_jvp", ("Zout_dot",), **plain), s.host(r + "_vjp", ("Zref_bar", "K_bar", "x0_bar"), **plain)
    sweeps(r + "_model", (), **model), sweeps(r + "_guarded", ("event_dot",), **g), sweeps(r + "_limited", ("event_dot",), **lim)
    s.host("qln_tracking_lqr", ("K", "P"))
    s.host("qln_tracking_lqr_guarded", ("K", "P"), Ztraj=g["Zout"], event=g["event"])
    s.host("qln_tracking_lqr_limited", ("K", "P"), Ztraj=lim["Zout"], event=lim["event"], sat=lim["sat"])
    s.host("qln_tracking_covariance", ("Sigma", "marg"), **plain)
    s.host("qln_tracking_covariance_guarded", ("Sigma", "marg", "event_var"), **g)
    s.host("qln_tracking_kalman", ("Lgain", "Pest", "Sigma", "marg"), **plain)
    s.host("qln_tracking_kalman_guarded", ("Lgain", "Pest", "Sigma", "marg", "event_var"), **g)
    e = r + "_estimated"
    for stem, outs, events in ((e, (), ()), (e + "_guarded", ("event", "event_hat"), ("event_dot", "event_hat_dot")),
                               (e + "_limited", ("event", "event_hat", "sat"), ("event_dot", "event_hat_dot"))):
        t = s.host(stem, ("Zout", "Xhat", "innov") + outs)
        s.host(stem + "_jvp", ("Zout_dot", "Xhat_dot", "innov_dot") + events, **t)
        s.host(stem + "_vjp", ("Zref_bar", "K_bar", "Lgain_bar", "x0_bar", "xhat0_bar", "model_bar"), **t)


def per_call_us(fn, calls, finish=lambda: None):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    finish()
    return 1e6 * (time.perf_counter() - t0) / calls


def child_time():
    import torch

    out = {}
    s = Session(64)
    vals = s.arguments("qln_tracking_rollout", ("Zout",), device=True)
    enqueue = s.bound("qln_tracking_rollout", vals)
    assert enqueue() == 0
    per_call_us(enqueue, 200, torch.cuda.synchronize)  # warm
    t0 = time.perf_counter()
    for _ in range(1000):
        enqueue()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    out["issue_us"], out["enqueue_us"] = 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t0)
    name = "qln_tracking_rollout_estimated_limited"
    for key, sess in (("mapped_us", Session(5)), ("staged_us", Session(64, Z_STRIDE))):
        t = sess.host(name, ("Zout", "Xhat", "innov", "event", "event_hat", "sat"))
        vals = sess.arguments(name + "_jvp_host", ("Zout_dot", "Xhat_dot", "innov_dot", "event_dot", "event_hat_dot"), **t)
        jvp = sess.bound(name + "_jvp_host", vals)
        assert jvp() == 0
        per_call_us(jvp, 20)  # warm: the buffers of every role exist
        out[key] = per_call_us(jvp, 200)
    print(json.dumps(out))


def summarise(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*results.json"), recursive=True))
    assert files, "no *results.json under " + directory
    rows = []

    def walk(node):  # the records are the dicts with a byte count under a "memory_copy" key, wherever the tool puts it
        if isinstance(node, dict):
            for k, v in node.items():
                if k == "memory_copy" and isinstance(v, list):
                    rows.extend(r for r in v if isinstance(r, dict) and "bytes" in r)
                else:
                    walk(v)
        elif isinstance(node, list):
            for v in node:
                walk(v)

    for f in files:
        walk(json.load(open(f)))
    rows.sort(key=lambda r: r["start_timestamp"])
    for r in rows:
        print(r.get("operation", r.get("kind")), r["bytes"])
    print("copies", len(rows), "bytes", sum(r["bytes"] for r in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", choices=["time", "copies"])
    ap.add_argument("--summarise")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    if a.child == "time":
        return child_time()
    if a.child == "copies":
        return every_host_form(Session(64, Z_STRIDE))
    builds = {"other": os.path.abspath(a.other), "this": os.path.join(ROOT, "quadruped_landing_amd", "csrc", "libqln_hip.so")}
    runs = {k: [] for k in builds}
    for rnd in range(a.rounds):
        for k, path in builds.items():
            env = dict(os.environ, QLN_LIB_PATH=path)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "time"], env=env, check=True,
                                 capture_output=True, text=True, timeout=120)
            runs[k].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(rnd, k, runs[k][-1], flush=True)
    report = {}
    for key in runs["this"][0]:
        for k in builds:
            xs = [r[key] for r in runs[k]]
            report[f"{key}.{k}"] = {"median": statistics.median(xs), "spread": max(xs) - min(xs)}
        o, t = report[f"{key}.other"], report[f"{key}.this"]
        report[f"{key}.within_spread"] = abs(t["median"] - o["median"]) <= o["spread"]
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
