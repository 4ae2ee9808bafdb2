#!/usr/bin/env python3
"""One pool call (locrec_knn_pool_recommend_ranked_batch) against one locrec_knn_recommend_ranked_batch call per distinct
member in sequence - how a queue over many region-set indexes was served before the pool - for the same requests in the
same process, at the shipped K = 2,000,000 (both warmed first, alternated, repeated; medians of wall clock, every call
synchronous):

  workloads   12 and 64 members of ~3,000 persons (synth.knn_dataset(3000, 300), the size of the walk-through's region
              sets) and 8 members of ~200,000 persons (synth.knn_dataset(200000, 10000)), with 1, 4 and 16 requests per
              member, every person rating the places of its place vector

The rows go to --out (default profiles/knn_pool_perf.txt) and to the standard output.  --small-only / --large-only run
one of the two sizes."""
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

PW, CW, K, TOP = 0.5, 0.5, 2_000_000, 10
WORKLOADS = (("12 members of ~3 k persons", 3_000, 300, 12), ("64 members of ~3 k persons", 3_000, 300, 64),
             ("8 members of ~200 k persons", 200_000, 10_000, 8))


def member(persons, places, seed):
    d = synth.knn_dataset(persons, places, seed)
    rating = np.random.default_rng(seed).integers(1, 6, size=len(d["p_idx"])).astype(np.int64)
    return d, pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"],
                           d["c_val"], d["c_dim"], d["p_rowptr"].copy(), d["p_idx"].astype(np.int64), rating)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_pool_perf.txt"))
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--large-only", action="store_true")
    args = ap.parse_args()
    lines = ["# tools/perf_knn_pool.py: per-member = one locrec_knn_recommend_ranked_batch call per distinct member in sequence, "
             "pool = one locrec_knn_pool_recommend_ranked_batch call;",
             f"# K = {K}, top {TOP}; medians of wall clock over {args.repeats} alternated repeats, ratio = per-member / pool "
             "(above 1: the pool is faster)"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for name, persons, places, n in WORKLOADS:
        if (args.small_only and persons > 10_000) or (args.large_only and persons <= 10_000):
            continue
        made = [member(persons, places, 0x900 + i) for i in range(n)]
        ds, ixs = [m[0] for m in made], [m[1] for m in made]
        pool = pkg.KnnPool(ixs)
        place_ids = np.arange(40, 40 + places, dtype=np.int64)
        regions = place_ids % 3
        rng = np.random.default_rng(64)
        drawn = [d["person_ids"][rng.choice(persons, 16, replace=False)] for d in ds]
        for per_member in (1, 4, 16):
            gi = np.repeat(np.arange(n, dtype=np.int32), per_member)
            pid = np.concatenate([d[:per_member] for d in drawn]).astype(np.int64)
            tgt = rng.integers(0, 3, len(gi)).astype(np.int64)

            def per_member_calls():
                t0 = time.perf_counter()
                r = [ix.recommend_ranked_batch(d[:per_member], PW, CW, K, place_ids, regions,
                                               tgt[m * per_member:(m + 1) * per_member], TOP)
                     for m, (ix, d) in enumerate(zip(ixs, drawn))]
                return time.perf_counter() - t0, r

            def pool_call():
                t0 = time.perf_counter()
                r = pool.recommend_ranked_batch(gi, pid, PW, CW, K, place_ids, regions, tgt, TOP)
                return time.perf_counter() - t0, r

            for _ in range(2):  # warm both (workspaces, row buffers)
                _, rb = per_member_calls()
                _, rp = pool_call()
            assert np.array_equal(np.concatenate([r[0] for r in rb]), rp[0])
            assert np.concatenate([r[1] for r in rb]).tobytes() == rp[1].tobytes()
            assert np.array_equal(np.concatenate([r[2] for r in rb]), rp[2])
            tb, tp = [], []
            for _ in range(args.repeats):
                tb.append(per_member_calls()[0])
                tp.append(pool_call()[0])
            st = pool.stats()
            mb, mp = float(np.median(tb)), float(np.median(tp))
            emit(f"{name}, {per_member:2d} requests per member: per-member {mb * 1e3:9.3f} ms, pool {mp * 1e3:9.3f} ms, "
                 f"ratio {mb / mp:5.2f}  [pool: {st['waves']} waves, {st['member_tiles']} member tiles, "
                 f"{st['fill_launches'] + st['scan_launches'] + st['aggregate_launches'] + st['finish_launches']} launches, "
                 f"{st['host_syncs']} waits, {st['readback_bytes']} bytes back]")
        pool.close()
        for ix in ixs:
            ix.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    append = args.large_only and os.path.exists(args.out)  # (the two sizes measured in two runs: one table)
    with open(args.out, "a" if append else "w") as f:
        f.write("\n".join(lines[2:] if append else lines) + "\n")


if __name__ == "__main__":
    main()
