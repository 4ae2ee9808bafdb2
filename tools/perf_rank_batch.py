#!/usr/bin/env python3
"""Ranked KNN batches against the row fetch plus the single ranker, on one GPU.

Shapes: cfg2 (1 M persons x 100 k places), N = 10:
  range   the 16,384-row range step at K = 50
  large   16 persons at K = 2,000,000
Compared in one process, alternating, after a warm-up, as the median of --reps steps timed with a host clock around
calls that end in a stream synchronisation:
  (a) recommend_range_async + fetch_recommend, then prep.rank_recommendations per person (the parent's code only; the
      places and the fetched rows are uploaded once per step and sliced, which favours (a))
  (b) recommend_range_async + fetch_ranked
The scan and aggregation are common to both, so the step after the range step is timed on its own too.  Also counts the
hipMalloc calls of five steady-state fetch_ranked steps.  Writes the report to --out and prints it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--persons", type=int, default=1_000_000)
    ap.add_argument("--places", type=int, default=100_000)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_batch_perf.txt"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("perf_rank_batch.py measures on a GPU: none is visible (there is no CPU fallback)")
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from locations_recommender_amd import _lib as L, prep, synth

    t0 = time.perf_counter()
    d = synth.knn_dataset_parallel(args.persons, args.places, 0x5EED0002, workers=8)
    d["r_rowptr"], d["r_place"] = d["p_rowptr"], d["p_idx"].astype(np.int64)
    d["r_rating"] = 1 + d["r_place"] % 5
    ix = pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"],
                      d["c_val"], d["c_dim"], d["r_rowptr"], d["r_place"], d["r_rating"])
    print(f"data and index: {time.perf_counter() - t0:.1f} s", flush=True)
    place_ids = np.arange(40, 40 + args.places, dtype=np.int64)
    regions = place_ids % 3
    dev_places, dev_regions = torch.as_tensor(place_ids).cuda(), torch.as_tensor(regions).cuda()
    lines = [f"ranked KNN batches, {args.persons} persons x {args.places} places, N = {args.limit}, "
             f"median of {args.reps} after one warm-up, host clock around synchronised calls",
             f"device: {torch.cuda.get_device_name(0)}"]

    def step_a(first, nq, k, targets):
        t0 = time.perf_counter()
        ix.recommend_range_async(first, nq, 0.5, 0.5, k)
        ix.synchronize()
        t1 = time.perf_counter()
        off, places, est = ix.fetch_recommend(nq)
        dp, de = torch.as_tensor(places).cuda(), torch.as_tensor(est).cuda()
        out = [prep.rank_recommendations(dp[off[q]:off[q + 1]], de[off[q]:off[q + 1]], dev_places, dev_regions,
                                         int(targets[q]), args.limit) for q in range(nq)]
        out = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in out]
        t2 = time.perf_counter()
        return t2 - t0, t2 - t1, int(off[-1]) * 16 + (nq + 1) * 8, out

    def step_b(first, nq, k, targets):
        t0 = time.perf_counter()
        ix.recommend_range_async(first, nq, 0.5, 0.5, k)
        ix.synchronize()
        t1 = time.perf_counter()
        out = ix.fetch_ranked(nq, place_ids, regions, targets, args.limit)
        t2 = time.perf_counter()
        return t2 - t0, t2 - t1, nq * args.limit * 16 + nq * 8, out

    ok = True
    for name, nq, k in (("range", 16384, 50), ("large", 16, 2_000_000)):
        nq = min(nq, args.persons)
        first = 4096 % max(1, args.persons - nq)
        targets = (np.arange(nq) % 3).astype(np.int64)
        res = {"a": [], "b": []}
        for rep in range(args.reps + 1):      # rep 0 warms up both
            for which, fn in (("a", step_a), ("b", step_b)):
                total, stage, nbytes, out = fn(first, nq, k, targets)
                if rep:
                    res[which].append((total, stage))
                res[which + "_bytes"], res[which + "_out"] = nbytes, out
            print(f"{name} rep {rep}: a {res['a'][-1] if rep else '-'} b {res['b'][-1] if rep else '-'}", flush=True)
        oi, osc, cnt = res["b_out"]
        same = all(np.array_equal(oi[q, :cnt[q]], a) and np.array_equal(osc[q, :cnt[q]].view(np.uint64), b.view(np.uint64))
                   for q, (a, b) in enumerate(res["a_out"]))
        st = prep.rank_recommendations_batch_stats()
        lines.append(f"\n{name}: {nq} persons at K = {k} (results of (a) and (b) identical: {same}; stats of (b): {st})")
        for which, label in (("a", "(a) fetch_recommend + single ranker per person"), ("b", "(b) fetch_ranked")):
            tot = sorted(t for t, _ in res[which])
            stg = sorted(s for _, s in res[which])
            lines.append(f"  {label}: step median {statistics.median(tot) * 1e3:.2f} ms (min {tot[0] * 1e3:.2f}, max "
                         f"{tot[-1] * 1e3:.2f}); after the range step alone: median {statistics.median(stg) * 1e3:.2f} ms "
                         f"(min {stg[0] * 1e3:.2f}, max {stg[-1] * 1e3:.2f}); {res[which + '_bytes']} bytes to the host")
        ma, mb = (statistics.median(t for t, _ in res[w]) for w in ("a", "b"))
        lines.append(f"  median (b) < median (a): {mb < ma} (ratio a / b = {ma / mb:.2f})")
        ok = ok and same and mb < ma
        # hipMalloc calls of steady-state fetch_ranked steps
        before = L.device_allocations()
        for _ in range(5):
            ix.recommend_range_async(first, nq, 0.5, 0.5, k)
            ix.fetch_ranked(nq, place_ids, regions, targets, args.limit)
        per = (L.device_allocations() - before) / 5
        lines.append(f"  hipMalloc calls per steady-state range + fetch_ranked step: {per:g} (the call-local buffers of the "
                     f"ranker: places, targets, segments, outputs, the region table's sort buffers and the plan)")
    ix.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
