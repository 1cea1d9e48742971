#!/bin/bash
# dev: tests subset + bench + kernel trace on one GPU box; outputs under $OUT (default out/)
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-out}; mkdir -p "$OUT"
export TMPDIR=/tmp
T="${TESTS:-tests/test_fused_step_gpu.py tests/test_deepconn_gpu.py tests/test_graph_step_gpu.py tests/test_optim_gpu.py}"
if [ "$T" != "none" ]; then
  timeout -k 10 900 python -m pytest $T -m gpu -q --maxfail=8 > $OUT/tests.log 2>&1
  rc=$?; grep -E "^(FAILED|ERROR)|passed|failed" $OUT/tests.log | tail -15; echo "tests rc=$rc"
  [ $rc -eq 124 ] && exit $rc
fi
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-variants ${BENCH_ARGS} > $OUT/bench.log 2>&1; rc=$?
tail -3 $OUT/bench.log | cut -c1-1500; echo "bench rc=$rc"
[ $rc -ne 0 ] && exit $rc
rm -rf $OUT/prof
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o r -- python3 bench.py --no-cpu-baseline --no-variants ${BENCH_ARGS} > $OUT/prof.log 2>&1; rc=$?
echo "prof rc=$rc"
f=$(find $OUT/prof -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && cp "$f" $OUT/kernel_stats.csv && python tools/kstats.py $OUT/kernel_stats.csv 2>/dev/null | head -40
exit 0
