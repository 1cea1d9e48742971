#!/bin/bash
# dev: A/B bench runs on ONE box: each line of $AB_CONFIGS is "name ENV=.. ENV=.." ; bench + rocprof kernel trace per config
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-out}; mkdir -p "$OUT"
export TMPDIR=/tmp
if [ -n "$TESTS" ] && [ "$TESTS" != "none" ]; then
  timeout -k 10 900 python -m pytest $TESTS -m gpu -q --maxfail=10 > $OUT/tests.log 2>&1
  rc=$?; grep -E "^(FAILED|ERROR)|passed|failed" $OUT/tests.log | tail -15; echo "tests rc=$rc"
  [ $rc -eq 124 ] && exit $rc
fi
while IFS= read -r line; do
  [ -z "$line" ] && continue
  name=$(echo "$line" | cut -d' ' -f1); envs=$(echo "$line" | cut -s -d' ' -f2-)
  echo "=== $name [$envs]"
  env $envs timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-variants ${BENCH_ARGS} > $OUT/bench_$name.log 2>&1; rc=$?
  python - "$name" "$OUT" <<'PY'
import json,sys
name, out = sys.argv[1], sys.argv[2]
try:
    l=[x for x in open(f"{out}/bench_{name}.log") if x.startswith("{")][-1]; d=json.loads(l)
    print(name, "ms_per_step", d["ms_per_step"], "min", d["median_block"]["ms_per_step_min"], "pairs/s", d["value"], "kernels_ms", d.get("kernels_ms"))
except Exception as e:
    print(name, "no bench line:", e); print(open(f"{out}/bench_{name}.log").read()[-1500:])
PY
  [ $rc -eq 124 ] && exit $rc
  if [ "${PROF:-1}" = "1" ]; then
    rm -rf $OUT/prof_$name
    # (the program itself after --: no env / bash hop under the profiler)
    export $envs 2>/dev/null
    timeout -k 10 200 rocprofv3 --kernel-trace -d $OUT/prof_$name -o r -- python3 bench.py --no-cpu-baseline --no-variants --steps 20 ${BENCH_ARGS} > $OUT/prof_$name.log 2>&1; rc=$?
    for e in $envs; do unset "${e%%=*}"; done
    python tools/prof_db.py $OUT/prof_$name --timeline 20 > $OUT/prof_$name.txt 2>&1; head -50 $OUT/prof_$name.txt
    rm -rf $OUT/prof_$name
    [ $rc -eq 124 ] && exit $rc
  fi
done <<< "$AB_CONFIGS"
exit 0
