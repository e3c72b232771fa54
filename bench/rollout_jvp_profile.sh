#!/bin/bash
# Timing and kernel statistics of qln_tracking_rollout_jvp, each GPU step under its own time limit, the steps chained:
#   1. bench/rollout_jvp_timing.py (HIP events)                       -> $OUT/rollout_jvp_timing.json
#   2. the same under rocprofv3 --kernel-trace --stats (a run of its own) -> $OUT/rollout_jvp_kernel_stats.csv
# usage: bench/rollout_jvp_profile.sh [OUT, default profiles]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/profiles}
mkdir -p "$OUT"
TMP=$(mktemp -d)
timeout -k 10 300 python3 "$R/bench/rollout_jvp_timing.py" --out "$OUT/rollout_jvp_timing.json" &&
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$TMP" -- python3 "$R/bench/rollout_jvp_timing.py" > "$TMP/under_rocprof.json" 2> "$TMP/stats.log" &&
cp "$(find "$TMP" -name '*kernel_stats.csv' | head -1)" "$OUT/rollout_jvp_kernel_stats.csv" &&
cat "$TMP/under_rocprof.json"
rc=$?
[ $rc -ne 0 ] && tail -5 "$TMP/stats.log"
rm -rf "$TMP"
exit $rc
