#!/bin/bash
# full parity suite + bench + rocprof kernel stats + traffic counters
cd "$GRAFT_REPO_ROOT" || exit 1
: "${OUT:?set OUT to the output directory}"; mkdir -p "$OUT"
export TMPDIR=/tmp
run() {
  local t=$1 log=$2; shift 2
  timeout -k 10 "$t" "$@" > "$OUT/$log" 2>&1; local rc=$?
  echo "[$log] rc=$rc"; tail -n ${TAILN:-6} "$OUT/$log"
  if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then echo "TIMEOUT in $log: stopping"; exit 99; fi
  return 0
}
run 1100 gpu_tests.log python -m pytest tests -x -q -m gpu
run 600 probe_sg.log python tools/perf_sg.py
run 900 bench.log python bench.py --full
rm -rf $OUT/prof_stats
run 900 prof.log rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_stats -- python bench.py --full --steps 3 --warmup 1 --no-cpu
f=$(find $OUT/prof_stats -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -12 "$f"
find $OUT/prof_stats -name "*kernel_trace.csv" -size +8M -delete
run 600 perf_host.log python tools/perf_host.py
