#!/usr/bin/env python3
"""Batched KNN at K beyond the per-query LDS lists (the tiled top-K of knn_large.hip) against sequential single
requests, on bench.py's KNN input (synth.knn_dataset, placeRatings from the place index, rating 1 + place % 5):

  cfg1   configs[1] (1 M persons x 100 k places, seed 0x5EED0002), 64 persons drawn with a fixed seed:
         query_batch against 64 sequential locrec_knn_query calls, and recommend_batch against 64 sequential
         locrec_knn_recommend calls (the one-by-one service a mid-K batch used to get), at K = 5,000 and 100,000
  cfg3   configs[3] on one GPU (10 M persons x 1 M places, seed 0x5EED0004), 16 persons: recommend_batch at the
         shipped K = 2,000,000 against 16 sequential requests (recorded, no target)

Both forms are warmed first, checked equal, then alternated; queries/s as min / median / max over --repeats.
recommend_batch is called through the C ABI with output arrays kept from the previous call - one call per batch, as
KnnIndex.recommend keeps its buffers for the sequential form (KnnIndex.recommend_batch sizes its arrays with a first
call and fills them with a second, which computes the batch twice).

--profile-only: one warm batch of each kind at cfg1 and nothing else (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys
import time

import ctypes as C

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
from locations_recommender_amd import _lib as L, synth  # noqa: E402

PW = CW = 0.5


def knn_input(n, places, seed):
    d = synth.knn_dataset(n, places, seed) if n <= 2_000_000 else synth.knn_dataset_parallel(n, places, seed, workers=16)
    d["r_rowptr"] = d["p_rowptr"]
    d["r_place"] = d["p_idx"].astype(np.int64)
    d["r_rating"] = 1 + d["r_place"] % 5
    return d


def make_index(d):
    return pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"],
                        d["c_val"], d["c_dim"], d["r_rowptr"], d["r_place"], d["r_rating"])


def compare(ix, kind, pids, k, repeats):
    """queries/s of the sequential and the batched form, alternated; returns the record"""
    if kind == "query":
        def sequential():
            return [ix.query(int(p), PW, CW, k) for p in pids]

        def batched():
            return ix.query_batch(pids, PW, CW, k)

        def same(s, b):
            ids, sims, cnt = b
            return all(np.array_equal(a, ids[j, :cnt[j]]) and np.array_equal(x, sims[j, :cnt[j]])
                       for j, (a, x) in enumerate(s))
    else:
        def sequential():
            return [ix.recommend(int(p), PW, CW, k) for p in pids]

        buf = [np.empty(0, np.int64), np.empty(0, np.float64)]

        def batched():
            off = np.zeros(len(pids) + 1, np.int64)
            while True:
                cap = C.c_int64(len(buf[0]))
                L.check(L.lib().locrec_knn_recommend_batch(ix._h, len(pids), L.ptr(pids, C.c_int64), PW, CW, k,
                                                           L.ptr(off, C.c_int64), L.ptr(buf[0], C.c_int64),
                                                           L.ptr(buf[1], C.c_double), C.byref(cap)))
                if cap.value <= len(buf[0]):
                    return off, buf[0][:off[-1]], buf[1][:off[-1]]
                buf[:] = [np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)]

        def same(s, b):
            off, places, est = b
            return all(np.array_equal(a, places[off[j]:off[j + 1]]) and np.array_equal(e, est[off[j]:off[j + 1]])
                       for j, (a, e) in enumerate(s))

    for _ in range(2):  # warm both (workspaces grown, staging buffers allocated)
        s, b = sequential(), batched()
    assert same(s, b), f"{kind} K={k}: the batch differs from the single requests"
    seq, bat = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        sequential()
        t1 = time.perf_counter()
        batched()
        t2 = time.perf_counter()
        seq.append(len(pids) / (t1 - t0))
        bat.append(len(pids) / (t2 - t1))
    seq, bat = np.array(seq), np.array(bat)
    ratio = bat / seq
    print(f"{kind}_batch K={k:,} of {len(pids)}: sequential {seq.min():,.1f} / {np.median(seq):,.1f} / {seq.max():,.1f} "
          f"queries/s, batch {bat.min():,.1f} / {np.median(bat):,.1f} / {bat.max():,.1f} queries/s (min / median / max "
          f"over {repeats}), batch / sequential {ratio.min():.2f} / {np.median(ratio):.2f} / {ratio.max():.2f}x", flush=True)
    return {"kind": kind, "k": k, "queries": len(pids), "sequential_queries_per_s": sorted(seq.round(2).tolist()),
            "batch_queries_per_s": sorted(bat.round(2).tolist()),
            "ratio": [round(float(ratio.min()), 3), round(float(np.median(ratio)), 3), round(float(ratio.max()), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--config", choices=["1", "3", "all"], default="all")
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    recs = []
    if args.config in ("1", "all") or args.profile_only:
        n = 1_000_000
        d = knn_input(n, 100_000, 0x5EED0002)
        ix = make_index(d)
        pids = d["person_ids"][np.random.default_rng(64).choice(n, 64, replace=False)].astype(np.int64)
        if args.profile_only:
            for k in (5_000, 100_000):
                ix.query_batch(pids, PW, CW, k)
                ix.recommend_batch(pids, PW, CW, k)
            ix.synchronize()
            ix.close()
            return
        for kind in ("query", "recommend"):
            for k in (5_000, 100_000):
                recs.append(dict(compare(ix, kind, pids, k, args.repeats), config=1))
        ix.close()
    if args.config in ("3", "all"):
        n = 10_000_000
        d = knn_input(n, 1_000_000, 0x5EED0004)
        ix = make_index(d)
        pids = d["person_ids"][np.random.default_rng(16).choice(n, 16, replace=False)].astype(np.int64)
        recs.append(dict(compare(ix, "recommend", pids, 2_000_000, args.repeats), config=3))
        ix.close()
    print(json.dumps({"metric": "knn_any_k_batch", "results": recs}), flush=True)


if __name__ == "__main__":
    main()
