#!/bin/bash
# rocprofv3 kernel statistics of tools/bench_spec.py (one series, D = 7 unless a second argument names another, both weight formats)
# -> <out dir, default profiles>/spec_kernel_stats.csv (D = 7) or spec_kernel_stats_d<D>.csv.  A run of its own: its times are not the
# benchmark's headline figures.  The GPU step runs under a time limit of its own.
set -o pipefail
REPO="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-$REPO/profiles}"
D="${2:-7}"
TMP="$(mktemp -d)"
NAME="spec_kernel_stats.csv"
[ "$D" = 7 ] || NAME="spec_kernel_stats_d$D.csv"
timeout -k 10 "${VZ_PROF_TIMEOUT:-540}" rocprofv3 --kernel-trace --stats -d "$TMP" -o spec --output-format csv -- python3 "$REPO/tools/bench_spec.py" --D "$D" --series 1 --steps 100 > "$TMP/bench.log" 2>&1 || { tail -20 "$TMP/bench.log"; exit 1; }
grep '^{' "$TMP/bench.log"
mkdir -p "$OUT"
cp "$(find "$TMP" -name 'spec_kernel_stats.csv' | head -1)" "$OUT/$NAME"
head -16 "$OUT/$NAME"
