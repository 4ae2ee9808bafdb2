#!/usr/bin/env python3
"""SG for visitors at cfg3 (synth.sg_dataset(seed=0x5EED0003)): 16 persons drawn with a fixed seed leave the edge list (G)
and come back as one full visitors tile.

  persons   the same 16 asked through locrec_sg_recommend_batch on the plus-visitors graph (the full edge list): one tile
            there too, the same sweeps.  Calls are alternated and repeated; a call's time and its time per round (the
            most sweeps a column of the tile executed) are given as min / median / max, and the visitors round is
            compared with the persons round against the persons round's own run-to-run spread (max - min).
  rebuilds  what serves a newcomer without the visitors path: for each of the 16, SgGraph(G + v), one request, close.

Parameters: the shipped (epsilon 0.01, max_iterations 20) and the fixed-work (epsilon 0, max_iterations 100).
--out FILE: the lines are written there too."""
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
TILE = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    g = synth.sg_dataset(seed=0x5EED0003)
    src, dst, w = g["source_id"], g["target_id"], g["balanced_weight"]
    rng = np.random.default_rng(64)
    person0 = int(g["first_person"])
    persons = (person0 + rng.choice(int(src.max()) - person0 + 1, TILE, replace=False)).astype(np.int64)
    out = np.isin(src, persons)
    rest = (src[~out], dst[~out], w[~out])
    live = np.unique(rest[1])
    visitors = [(dst[src == p], w[src == p]) for p in persons]
    assert all(np.isin(t, live).all() for t, _ in visitors), "a target lost its last inbound edge"
    off = np.zeros(TILE + 1, np.int64)
    np.cumsum([len(t) for t, _ in visitors], out=off[1:])
    vt, vw = np.concatenate([t for t, _ in visitors]), np.concatenate([x for _, x in visitors])
    sg, sg_plus = pkg.SgGraph(*rest), pkg.SgGraph(src, dst, w)
    say(f"cfg3: {sg_plus.info()['vertices']:,} vertices, {len(src):,} edges; a tile of {TILE} visitors with {len(vt)} edges")

    for eps, max_it in ((0.01, 20), (0.0, 100)):
        def as_visitors():
            t0 = time.perf_counter()
            r = sg.visitors_recommend_batch(off, vt, vw, ALPHA, eps, max_it)
            return time.perf_counter() - t0, int(np.max(r[3] + r[4]))

        def as_persons():
            t0 = time.perf_counter()
            r = sg_plus.recommend_batch(persons, ALPHA, eps, max_it)
            return time.perf_counter() - t0, int(np.max(r[3] + r[4]))

        for _ in range(2):
            as_visitors()
            as_persons()
        tv, tp, rv, rp = [], [], [], []
        for _ in range(args.repeats):
            a, ra = as_visitors()
            b, rb = as_persons()
            tv.append(a * 1e3), tp.append(b * 1e3), rv.append(a * 1e6 / max(1, ra)), rp.append(b * 1e6 / max(1, rb))
        tv, tp, rv, rp = (np.array(x) for x in (tv, tp, rv, rp))
        three = lambda x: f"{x.min():.2f} / {np.median(x):.2f} / {x.max():.2f}"
        say(f"epsilon {eps}, max {max_it}, {ra} rounds: visitors tile {three(tv)} ms a call, {three(rv)} us a round; the same "
            f"{TILE} persons on the plus-visitors graph {three(tp)} ms a call, {three(rp)} us a round (min / median / max over "
            f"{args.repeats}); visitors - persons {np.median(rv) - np.median(rp):+.2f} us a round, the persons round's spread "
            f"{rp.max() - rp.min():.2f} us")
        st = pkg.SgGraph.visitors_stats()
        say(f"    visitors call: {st}")

    # what a newcomer costs without the visitors path: the graph rebuilt around each
    for name in ("first pass", "second pass"):
        t0 = time.perf_counter()
        for p, (t, x) in zip(persons, visitors):
            one = pkg.SgGraph(np.r_[rest[0], np.full(len(t), p)], np.r_[rest[1], t], np.r_[rest[2], x])
            one.recommend(int(p), ALPHA, 0.01, 20)
            one.close()
        dt = time.perf_counter() - t0
        say(f"{TILE} rebuilds of G + v with one request each (epsilon 0.01, max 20), {name}: {dt:.3f} s, {dt / TILE * 1e3:.1f} ms a visitor")
    sg.close()
    sg_plus.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
