#!/bin/bash
cd "$GRAFT_REPO_ROOT" || exit 1
: "${OUT:?set OUT to the output directory}"; mkdir -p "$OUT"; export TMPDIR=/tmp
timeout -k 10 ${1:-900} python bench.py --full ${2:-} > $OUT/bench.log 2> $OUT/bench.err; rc=$?
tail -c 6000 $OUT/bench.log; tail -n 5 $OUT/bench.err
exit $rc
