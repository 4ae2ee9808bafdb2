#!/usr/bin/env python3
"""One pool call (locrec_sg_pool_recommend_batch) against one locrec_sg_recommend_batch call per graph in sequence, for
the same requests in the same process (both warmed first, alternated, repeated; medians of wall clock):

  workloads   64 graphs of ~36 k edges (synth.sg_dataset(2000, 200, 20), the shape DESIGN.md section 4 quotes for groups)
              and 8 graphs of cfg3 size (synth.sg_dataset()), with 1, 4 and 16 person requests per graph
  parameters  shipped (epsilon 0.01, max_iterations 20) and fixed work (epsilon 0, max_iterations 100)

The rows go to --out (default profiles/sg_pool_perf.txt) and to the standard output.  --small-only / --large-only run
one of the two workloads (each needs a few minutes of host time to generate its graphs)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
from locations_recommender_amd import synth  # noqa: E402

ALPHA = 0.15
WORKLOADS = (("64 graphs of ~36 k edges", 2_000, 200, 64), ("8 graphs of cfg3 size", 280_000, 10_000, 8))
PARAMS = (("shipped (epsilon 0.01, max 20)", 0.01, 20), ("fixed (epsilon 0, max 100)", 0.0, 100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sg_pool_perf.txt"))
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--large-only", action="store_true")
    args = ap.parse_args()
    lines = ["# tools/perf_sg_pool.py: per-graph = one locrec_sg_recommend_batch call per graph in sequence, pool = one "
             "locrec_sg_pool_recommend_batch call;",
             f"# medians of wall clock over {args.repeats} alternated repeats, ratio = per-graph / pool (above 1: the pool is faster)"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for name, persons, places, n in WORKLOADS:
        if (args.small_only and n != 64) or (args.large_only and n != 8):
            continue
        specs = [synth.sg_dataset(n_persons=persons, n_places=places, n_categories=20, seed=0x700 + i) for i in range(n)]
        graphs = [pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"]) for g in specs]
        pool = pkg.SgPool(graphs)
        edges = graphs[0].info()["edges"]
        rng = np.random.default_rng(64)
        drawn = [int(g["first_person"]) + rng.choice(persons, 16, replace=False) for g in specs]
        for per_graph in (1, 4, 16):
            gi = np.repeat(np.arange(n, dtype=np.int32), per_graph)
            v = np.concatenate([d[:per_graph] for d in drawn]).astype(np.int64)
            for label, eps, max_it in PARAMS:
                def per_graph_calls():
                    t0 = time.perf_counter()
                    r = [g.recommend_batch(d[:per_graph], ALPHA, eps, max_it) for g, d in zip(graphs, drawn)]
                    return time.perf_counter() - t0, r

                def pool_call():
                    t0 = time.perf_counter()
                    r = pool.recommend_batch(gi, v, ALPHA, eps, max_it)
                    return time.perf_counter() - t0, r

                for _ in range(2):  # warm both (batch buffers, staging)
                    _, rb = per_graph_calls()
                    _, rp = pool_call()
                assert np.array_equal(np.concatenate([r[1] for r in rb]), rp[1])
                assert np.concatenate([r[2] for r in rb]).tobytes() == rp[2].tobytes()
                tb, tp = [], []
                for _ in range(args.repeats):
                    tb.append(per_graph_calls()[0])
                    tp.append(pool_call()[0])
                st = pool.stats()
                mb, mp = float(np.median(tb)), float(np.median(tp))
                emit(f"{name} ({edges} edges each), {per_graph:2d} requests per graph, {label}: per-graph {mb * 1e3:9.3f} ms, "
                     f"pool {mp * 1e3:9.3f} ms, ratio {mb / mp:5.2f}  [pool: {st['tile_waves']} tile waves, {st['rounds']} rounds, "
                     f"{st['sweep_launches']} + {st['finalize_launches']} launches, {st['polls']} polls]")
        pool.close()
        for g in graphs:
            g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
