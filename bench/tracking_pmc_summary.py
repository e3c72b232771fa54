"""Summarise rocprofv3 --pmc output dirs of bench/tracking_timing.py: per counter, the mean over the dispatches of each
k_tracking_lqr instantiation and configuration (the first half of an instantiation's dispatches run at N = 40, the second
at N = 61).
   python bench/tracking_pmc_summary.py DIR [DIR ...]"""
import collections
import csv
import glob
import sys

for d in sys.argv[1:]:
    rows = []
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "k_tracking_lqr" in r["Kernel_Name"]]
    disp = collections.OrderedDict()  # (kernel, dispatch id) -> {counter: value}, start time
    for r in rows:
        key = (r["Kernel_Name"], int(r["Dispatch_Id"]))
        e = disp.setdefault(key, {"_t": int(r["Start_Timestamp"]), "_dur_us": (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3})
        e[r["Counter_Name"]] = e.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    by_kernel = collections.defaultdict(list)
    for (k, _), e in sorted(disp.items(), key=lambda kv: kv[1]["_t"]):
        by_kernel["k_tracking_lqr<true>  (K and P)" if "<true" in k else "k_tracking_lqr<false> (K only) "].append(e)
    for k, es in by_kernel.items():
        h = len(es) // 2
        for N, part in ((40, es[:h]), (61, es[h:])):
            for c in sorted(x for x in part[0] if x != "_t"):
                v = [e[c] for e in part]
                print(f"{d.rstrip('/').split('/')[-1]:14s} {k} N={N} n={len(v):3d} {c:24s} mean={sum(v) / len(v):.4g}")
