#!/bin/bash
cd "$GRAFT_REPO_ROOT" || exit 1
: "${OUT:?set OUT to the output directory}"; mkdir -p "$OUT"
for flags in "--no-aggregate" ""; do
  LOCREC_DEBUG_TIMING=1 timeout -k 10 400 python bench.py --full --no-cpu --no-sg $flags > $OUT/bisect.log 2> $OUT/bisect.err || { echo "failed"; tail -5 $OUT/bisect.err; exit 1; }
  grep "locrec recommend" $OUT/bisect.err | tail -3
  tail -n 1 $OUT/bisect.log | python -c "
import sys, json
d = json.loads(sys.stdin.read()); print('$flags', d['value'] / 1e9, d['knn_request'])"
done
