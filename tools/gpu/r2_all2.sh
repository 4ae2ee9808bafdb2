#!/bin/bash
# full suite, bench (with cpu legs), producer timings
cd "$GRAFT_REPO_ROOT" || exit 1
: "${OUT:?set OUT to the output directory}"; mkdir -p "$OUT"; export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -x -q --durations=5 > $OUT/pytest_gpu.log 2>&1; rc=$?
tail -n 10 $OUT/pytest_gpu.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python tools/perf_prep.py > $OUT/perf_prep.log 2>&1; rc=$?
grep -v amdgpu.ids $OUT/perf_prep.log | tail -n 8
[ $rc -ne 0 ] && exit $rc
timeout -k 10 700 python bench.py --full > $OUT/bench_full.log 2> $OUT/bench_full.err; rc=$?
tail -c 1500 $OUT/bench_full.log
exit $rc
