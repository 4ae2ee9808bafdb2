#!/usr/bin/env python3
"""Batched SG requests against sequential single requests at cfg3 (synth.sg_dataset(seed=0x5EED0003)), 64 person
targets drawn with a fixed seed:

  shipped   epsilon 0.01, max_iterations 20: targets/s of 64 sequential locrec_sg_recommend calls against one
            locrec_sg_recommend_batch of the same 64 (both warmed first, alternated, repeated; min / median / max)
  fixed     epsilon 0, max_iterations 100: target-iterations/s of one tile of w targets (w = 1, 2, 4, 8, 16: every
            tile width the build runs) next to a single request's iterations/s; executed sweeps are counted per
            target (an exact fp64 fixed point can stop a target before 100)

--profile-only: one warm batch of each kind and nothing else (for a rocprofv3 --kernel-trace --stats run)."""
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

ALPHA = 0.15
TILE = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()

    g = synth.sg_dataset(seed=0x5EED0003)
    rng = np.random.default_rng(64)
    person0 = int(g["first_person"])
    n_persons = int(g["source_id"].max()) - person0 + 1
    targets = (person0 + rng.choice(n_persons, 64, replace=False)).astype(np.int64)
    sg = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"])

    if args.profile_only:
        sg.recommend_batch(targets, ALPHA, 0.01, 20)
        sg.recommend_batch(targets[:TILE], ALPHA, 0.0, 100)
        sg.synchronize()
        sg.close()
        return

    # ---- shipped parameters: 64 sequential requests vs one batch of the same 64
    def sequential():
        t0 = time.perf_counter()
        its = [sg.recommend(int(v), ALPHA, 0.01, 20)[2] for v in targets]
        return time.perf_counter() - t0, its

    def batched():
        t0 = time.perf_counter()
        r = sg.recommend_batch(targets, ALPHA, 0.01, 20)
        return time.perf_counter() - t0, r[3]

    for _ in range(2):  # warm both (graphs captured, staging and batch buffers allocated)
        sequential()
        batched()
    seq, bat = [], []
    for _ in range(args.repeats):
        ts, its_s = sequential()
        tb, its_b = batched()
        assert list(its_s) == list(its_b)
        seq.append(len(targets) / ts)
        bat.append(len(targets) / tb)
    seq, bat = np.array(seq), np.array(bat)
    ratio = bat / seq
    print(f"shipped (epsilon 0.01, max 20), 64 persons, iterations {np.min(its_b)}-{np.max(its_b)}: "
          f"sequential {seq.min():,.0f} / {np.median(seq):,.0f} / {seq.max():,.0f} targets/s, "
          f"batch {bat.min():,.0f} / {np.median(bat):,.0f} / {bat.max():,.0f} targets/s (min / median / max over "
          f"{args.repeats}), batch / sequential {ratio.min():.2f}-{ratio.max():.2f}x", flush=True)
    rec = {"metric": "sg_batch_shipped", "targets": 64, "sequential_targets_per_s": sorted(seq.round(1).tolist()),
           "batch_targets_per_s": sorted(bat.round(1).tolist()), "ratio": [round(ratio.min(), 3), round(float(np.median(ratio)), 3),
                                                                          round(ratio.max(), 3)]}

    # ---- fixed work: one tile of w targets, 100 sweeps each, vs one single request
    def single_rate():
        v = int(targets[0])
        sg.recommend(v, ALPHA, 0.0, 100)
        rates = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            _, _, it, conv = sg.recommend(v, ALPHA, 0.0, 100)
            rates.append((it + conv) / (time.perf_counter() - t0))
        return np.array(rates)

    single = single_rate()
    print(f"fixed (epsilon 0, max 100): single request {single.min():,.0f} / {np.median(single):,.0f} / "
          f"{single.max():,.0f} iterations/s", flush=True)
    rec["fixed_single_iterations_per_s"] = sorted(single.round(1).tolist())
    rec["fixed_batch_target_iterations_per_s"] = {}
    for w in (1, 2, 4, 8, 16):
        tw = targets[:w]
        sg.recommend_batch(tw, ALPHA, 0.0, 100)
        rates = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            _, _, _, its, conv = sg.recommend_batch(tw, ALPHA, 0.0, 100)
            rates.append(float(np.sum(its + conv)) / (time.perf_counter() - t0))
        rates = np.array(rates)
        print(f"fixed (epsilon 0, max 100): batch of {w:2d} {rates.min():,.0f} / {np.median(rates):,.0f} / "
              f"{rates.max():,.0f} target-iterations/s ({np.median(rates) / np.median(single):.1f}x the single request)",
              flush=True)
        rec["fixed_batch_target_iterations_per_s"][str(w)] = sorted(rates.round(1).tolist())
    print(json.dumps(rec), flush=True)
    sg.close()


if __name__ == "__main__":
    main()
