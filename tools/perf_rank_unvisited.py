#!/usr/bin/env python3
"""The ranked stage of a KNN range step with and without the exclusion lists, on one GPU.

Shape: cfg2 (1 M persons x 100 k places), one batch of 16,384 requests at K = 50, N = 10.  The range step runs once per
repetition and is waited for; then the ranked stage alone - fetch_ranked, or fetch_ranked(unvisited=True) - is timed with
events on the index's stream around the call (and with a host clock, for comparison).  Both forms in one process,
alternating, median of --reps after a warm-up.  The plain call is unchanged code: the yardstick.  Writes the report to
--out and prints it."""
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
    ap.add_argument("--nq", type=int, default=16_384)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_unvisited_perf.txt"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("perf_rank_unvisited.py measures on a GPU: none is visible (there is no CPU fallback)")
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from locations_recommender_amd import prep, synth

    t0 = time.perf_counter()
    d = synth.knn_dataset_parallel(args.persons, args.places, 0x5EED0002, workers=8)
    d["r_rowptr"], d["r_place"] = d["p_rowptr"], d["p_idx"].astype(np.int64)
    d["r_rating"] = 1 + d["r_place"] % 5
    ix = pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"],
                      d["c_val"], d["c_dim"], d["r_rowptr"], d["r_place"], d["r_rating"])
    print(f"data and index: {time.perf_counter() - t0:.1f} s", flush=True)
    stream = torch.cuda.Stream()
    ix.set_stream(stream.cuda_stream)
    place_ids = np.arange(40, 40 + args.places, dtype=np.int64)
    regions = place_ids % 3
    nq = min(args.nq, args.persons)
    first = 4096 % max(1, args.persons - nq)
    targets = (np.arange(nq) % 3).astype(np.int64)
    # the lists' entries: the rating rows of the persons at the range's internal rows
    order = np.argsort(d["person_ids"], kind="stable")
    at = order[np.searchsorted(d["person_ids"][order], ix.row_person_ids(first, nq))]
    pairs = int((d["r_rowptr"][at + 1] - d["r_rowptr"][at]).sum())

    def stage(unvisited):
        ix.recommend_range_async(first, nq, 0.5, 0.5, args.k)
        ix.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t = time.perf_counter()
        out = ix.fetch_ranked(nq, place_ids, regions, targets, args.limit, unvisited=unvisited)
        host_ms = (time.perf_counter() - t) * 1e3
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), host_ms, out

    res = {False: [], True: []}
    outs, stats = {}, {}
    for rep in range(args.reps + 1):      # rep 0 warms up both
        for unvisited in (False, True):
            ev, host_ms, outs[unvisited] = stage(unvisited)
            stats[unvisited] = prep.rank_recommendations_batch_stats()
            if rep:
                res[unvisited].append((ev, host_ms))
        print(f"rep {rep}: plain {res[False][-1] if rep else '-'} unvisited {res[True][-1] if rep else '-'}", flush=True)
    changed = int((outs[False][0] != outs[True][0]).any(axis=1).sum())
    med = {u: (statistics.median(e for e, _ in res[u]), statistics.median(h for _, h in res[u])) for u in res}
    ratio = med[True][0] / med[False][0]
    lines = [f"ranked stage of a KNN range step, {args.persons} persons x {args.places} places, {nq} requests, K = {args.k}, "
             f"N = {args.limit}; median of {args.reps} after one warm-up, events on the index's stream around the call",
             f"device: {torch.cuda.get_device_name(0)}",
             f"exclusion lists: {pairs} entries in all ({pairs / nq:.1f} a request); {changed} of {nq} rankings differ"]
    for u, label in ((False, "fetch_ranked"), (True, "fetch_ranked(unvisited=True)")):
        ev = sorted(e for e, _ in res[u])
        lines.append(f"  {label}: median {med[u][0]:.2f} ms (min {ev[0]:.2f}, max {ev[-1]:.2f}); host clock median "
                     f"{med[u][1]:.2f} ms; stats {stats[u]}")
    lines.append(f"  unvisited / plain = {ratio:.3f} (expected within 1.5)")
    ix.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
