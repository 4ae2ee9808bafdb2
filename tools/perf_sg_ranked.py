#!/usr/bin/env python3
"""The ranked SG batch on the device against its host-ranked form at cfg3 (synth.sg_dataset(seed=0x5EED0003): 280 k
persons, 10 k places), person targets drawn with a fixed seed, places in three regions, epsilon 0.01, 20 iterations at
the most, N = 10:

  device   SgGraph.recommend_ranked_batch(on_device=True): locrec_sg_recommend_ranked_batch, x stays on the device
  host     on_device=False: locrec_sg_recommend_batch's host rows, uploaded again for locrec_rank_recommendations_batch
           (the path before the device form existed: the baseline)

for 16, 256 and 1,024 targets.  Both are warmed, then alternated `--repeats` times; per form the median (min - max) of
the wall clock around the call (it ends in a stream synchronise) and of a HIP event pair recorded on the handle's
stream around it.  The results are compared once per size (ids, counts, probability bits).  readback_bytes: the device
form's own count (locrec_sg_recommend_ranked_batch_stats); the host form's is computed from the shapes - per tile the
packed state, block sums and x ((T + 1) x 16 fp64), then the ranker's rows.

--profile-only: one warm call of each form at 256 targets and nothing else (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
from locations_recommender_amd import synth  # noqa: E402

ALPHA, EPSILON, MAX_ITERATIONS, LIMIT = 0.15, 0.01, 20, 10
SIZES = (16, 256, 1024)
TILE, PARTS = 16, 64  # kBatchB, kParts


def host_form_readback(n_targets, live, width):
    tiles = -(-n_targets // TILE)
    per_tile = 256 + 2 * PARTS * TILE * 8 + (live + 1) * TILE * 8
    return tiles * per_tile + n_targets * (16 * width + 8) + 32


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) and x.shape == y.shape
               for x, y in zip(a, b))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")

    g = synth.sg_dataset(seed=0x5EED0003)
    person0 = int(g["first_person"])
    n_persons = int(g["source_id"].max()) - person0 + 1
    n_places = person0 - 40
    rng = np.random.default_rng(1024)
    place_ids = np.arange(40, 40 + n_places, dtype=np.int64)
    regions = rng.integers(0, 3, n_places).astype(np.int64)
    sg = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"])
    live = sg.live_count()
    stream = torch.cuda.Stream()
    sg.set_stream(stream.cuda_stream)

    def call(v, t, on_device):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        r = sg.recommend_ranked_batch(v, ALPHA, EPSILON, MAX_ITERATIONS, place_ids, regions, t, LIMIT, on_device=on_device)
        wall = time.perf_counter() - t0
        b.record(stream)
        b.synchronize()
        return r, wall * 1e3, a.elapsed_time(b)

    if args.profile_only:
        v = (person0 + rng.choice(n_persons, 256, replace=False)).astype(np.int64)
        t = rng.integers(0, 3, 256).astype(np.int64)
        call(v, t, True)
        call(v, t, False)
        sg.close()
        return

    print(f"cfg3: {sg.info()['vertices']} vertices, T = {live} live, {n_places} places in 3 regions; epsilon {EPSILON}, "
          f"max {MAX_ITERATIONS} iterations, N = {LIMIT}; median (min - max) of {args.repeats} alternated calls, ms", flush=True)
    rec = {"metric": "sg_ranked_batch", "repeats": args.repeats, "sizes": {}}
    for n in SIZES:
        v = (person0 + rng.choice(n_persons, n, replace=False)).astype(np.int64)
        t = rng.integers(0, 3, n).astype(np.int64)
        for _ in range(2):  # warm both forms at this size
            dev = call(v, t, True)[0]
            host = call(v, t, False)[0]
        assert same(dev, host), "the two forms disagree"
        st = None
        times = {True: ([], []), False: ([], [])}
        for _ in range(args.repeats):
            for form in (True, False):
                _, wall, ev = call(v, t, form)
                times[form][0].append(wall)
                times[form][1].append(ev)
                if form:
                    st = pkg.SgGraph.ranked_batch_stats()
        width = dev[0].shape[1]
        host_bytes = host_form_readback(n, live, width)

        def fmt(x):
            return f"{np.median(x):8.3f} ({np.min(x):.3f} - {np.max(x):.3f})"

        dw, de = times[True]
        hw, he = times[False]
        print(f"{n:5d} targets  device: wall {fmt(dw)}  events {fmt(de)}  readback {st['readback_bytes']:>10,d} B "
              f"({st['tiles']} tiles, {st['groups']} group(s), {st['emitted_rows']:,d} rows emitted, {st['host_syncs']} waits)", flush=True)
        print(f"{n:5d} targets  host:   wall {fmt(hw)}  events {fmt(he)}  readback {host_bytes:>10,d} B (from the shapes)", flush=True)
        print(f"{n:5d} targets  host / device: wall {np.median(hw) / np.median(dw):.2f}x, events "
              f"{np.median(he) / np.median(de):.2f}x", flush=True)
        rec["sizes"][str(n)] = {"device_wall_ms": sorted(np.round(dw, 3).tolist()), "host_wall_ms": sorted(np.round(hw, 3).tolist()),
                                "device_event_ms": sorted(np.round(de, 3).tolist()), "host_event_ms": sorted(np.round(he, 3).tolist()),
                                "device_readback_bytes": st["readback_bytes"], "host_readback_bytes": host_bytes,
                                "device_stats": st}
    print(json.dumps(rec), flush=True)
    sg.close()


if __name__ == "__main__":
    main()
