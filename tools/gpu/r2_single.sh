#!/bin/bash
cd "$GRAFT_REPO_ROOT" || exit 1
: "${OUT:?set OUT to the output directory}"; mkdir -p "$OUT"; export TMPDIR=/tmp
timeout -k 10 500 python -m pytest tests/test_gpu_knn.py tests/test_gpu_fuzz.py -m gpu -x -q -k "single or random_index or sharded_request or cfg2_full_size or large_k" > $OUT/pytest_single.log 2>&1; rc=$?
tail -n 4 $OUT/pytest_single.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 500 python bench.py --full --no-sg --no-formats --no-cpu --steps 2 > $OUT/bench_single.log 2> $OUT/bench_single.err
python - <<'PY'
import json, os
for line in open(os.environ["OUT"] + "/bench_single.log"):
    if line.startswith("{"):
        d = json.loads(line); r = d["knn_request"]
        print("step ms", d["ms_per_step"], "| recommend ms", r["ms_per_request"], "query ms", r["find_similar_persons_ms"], "scan kernel ms", r["scan_roofline"]["avg_launch_ms"], "frac", r["scan_roofline"]["frac"], "| large_k", r["large_k"]["recommend_ms"], r["large_k"]["find_similar_persons_ms"])
PY
