"""The JSON line `bench.py --full` prints (the committed line of the round's final run, profiles/r03_bench.json) carries
every field of the driver's contract, and its numbers are consistent with each other and with SURVEY.md 8d's byte counts;
a plain run reports the headline alone and dumps what its last timed launch computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_bench_line_has_the_contract_fields_and_consistent_numbers():
    d = json.load(open(os.path.join(ROOT, "profiles", "r03_bench.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"].startswith("knot-point constraint+Jacobian evals/sec") and d["unit"] == "knot-evals/s"
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    B, N = d["config"]["problems_per_gpu"], d["config"]["knots"]
    # value = units of all ranks / wall time per step
    assert abs(d["value"] - B * N / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    alg = float(np.sum(bench.algorithmic_bytes(N, np.full(B, 14))))
    assert abs(r["algorithmic_bytes_per_launch"] - alg) <= 1.0 and abs(alg / (B * N) - 2651.4) < 1e-9
    assert abs(r["achieved"] - alg / (r["launch_ms_avg"] * 1e-3) / 1e9) <= 1e-6 * r["achieved"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) <= 1e-12
    assert 0.99 * alg <= r["traffic"] <= 1.05 * alg          # PMC traffic: no wasted re-reads
    assert r["launch_ms_avg"] <= d["ms_per_step"]            # the kernel inside the wall-clock step
    s = r["strict_nnz"]
    assert abs(s["bytes_per_knot_eval"] - float(bench.strict_bytes(N, 14)) / N) < 1e-9
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0
    # north star: >= 1e7 knot-evals/s at >= 40 % of the HBM roofline
    assert d["value"] >= 1e7 and r["frac"] >= 0.40
    # the measured traffic is quoted for the build it was taken on, and says where it comes from
    assert "traffic_source" in r and "rocprofv3" in r["traffic_source"]
    # the caller side on BASELINE.json configs[1]: every problem solved, judged by the evaluator, a CPU figure beside it
    sv = d["other"]["solve_config2_B1024_N40"]
    assert sv["problems"] == 1024 and sv["solved_to_1e-6"] == 1024 and sv["violation_max"] <= 1e-6 * 1.0001
    assert sv["solved_problems_per_s"] > 1e3
    cs = sv["cpu_baseline"]
    assert cs["cores"] == 1 and cs["kind"] == "port" and cs["solved_to_1e-6"] == cs["problems"] >= 1 and "not Ipopt" in cs["sample"]
    # one measurement for every N: the timed region holds the K launches only, the end-of-job tail is reported beside it
    assert "K-launch region only" in d["config"]["timing"] and d["gather_ms"] > 0 and d["gather_c_ms"] > 0
    assert d["config"]["multi_gpu_status"] == "single GPU" and "generated on the device" in d["config"]["workload_data"]
    # the tracked rocprofv3 average of the newest profile round stands beside the live one (and a note when they differ by > 5 %)
    assert r["profile_launch_ms_avg"] > 0
    if abs(r["profile_launch_ms_avg"] - r["launch_ms_avg"]) > 0.05 * r["profile_launch_ms_avg"]:
        assert "profile_vs_live" in r


def test_kernel_build_id_is_stable_and_traffic_lookup_refuses_other_builds(tmp_path, monkeypatch):
    """bench.measured_traffic quotes profiles/traffic.json only for the kernel build it was measured on."""
    import json as J

    bid = bench.kernel_build_id()
    assert len(bid) == 16 and bid == bench.kernel_build_id()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    os.makedirs(tmp_path / "profiles")
    os.makedirs(tmp_path / "quadruped_landing_amd" / "csrc")
    for f in ("qln_kernels.hip", "qln_kernel_common.h", "qln_device.h"):
        (tmp_path / "quadruped_landing_amd" / "csrc" / f).write_text("x" + f)
    here = bench.kernel_build_id()
    J.dump({"config3": {"hbm_bytes_per_launch": 7.0e9, "build_id": here, "profile": "p"},
            "config4": {"hbm_bytes_per_launch": 1.4e10, "build_id": "somethingelse"}}, open(tmp_path / "profiles" / "traffic.json", "w"))
    assert bench.measured_traffic("config3")[0] == 7.0e9
    t, why = bench.measured_traffic("config4")
    assert t is None and "not quoted" in why
    t, why = bench.measured_traffic("config2")
    assert t is None and "no PMC profile" in why


@pytest.mark.gpu
def test_plain_run_times_the_steps_only_and_dumps_the_same_outputs_every_run(tmp_path):
    """Without --full the line holds the headline of exactly --steps launches and nothing measured beside it; --dump-outputs
    writes c and the Jacobian values of the last launch for a fixed sample of problems, the same bits in a second run."""
    B, N, kt, S = 1024, 40, 14, bench.DUMP_PROBLEMS
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload",
               "config2", "--placement-trials", "1", "--dump-outputs", str(out)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f64" and d["unit"] == "knot-evals/s"
        assert d["config"]["problems_per_gpu"] == B and d["config"]["knots"] == N
        assert abs(d["value"] - B * N / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
        for k in ("other", "cpu_baseline", "cpu_baseline_all_cores", "gather_ms", "gather_c_ms"):
            assert k not in d, k
        assert sorted(os.listdir(out)) == ["c.npy", "jac_vals.npy"]
        a = {k: np.load(out / (k + ".npy")) for k in ("c", "jac_vals")}
        assert all(v.dtype == np.float64 and v.ndim == 1 for v in a.values())
        assert sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
        # whole segments of S problems: m_nlp = 18 N - k_trans + 16 constraints, the dense-block value count of each
        assert a["c"].size == S * (18 * N - kt + 16)
        assert a["jac_vals"].size == S * (300 * (N - 1) + N + 435 + 15 * (N - 1) + 3 * N - kt + 3)
        assert np.count_nonzero(a["c"]) > 0 and np.count_nonzero(a["jac_vals"]) > 0
        runs.append(a)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k], equal_nan=True), k
