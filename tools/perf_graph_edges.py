#!/usr/bin/env python3
"""Times of the stochastic graph's edge-family producers (csrc/prep.hip), device-memory inputs, one warm-up, then
min / median / max over --repeats; host clock around calls that return synchronised, phase split from HIP events.

  (a) locrec_calc_count_edges beside locrec_calc_ratings on the same visit rows (default 25 M rows, 625 k persons,
      50 entities, top_n = 100), alternated - the existing function is the yardstick; they share every sort.
  (b) locrec_calc_similar_place_edges on a synthetic week-dense case (default 4 M rows, 20 k persons = 200 visits
      each, 5 k places, timestamps uniform over 14 days in ms, interval 7 days, top_n = 50): candidate pairs, chunks,
      pairs/s and the sort / emit / merge split (locrec_similar_place_edges_stats).
  (c) CPU context only: the numpy restatement of the co-visit join (tests/edge_cases.py) on a 1/100-size case
      (1/100 of the persons, the same visits per person), and the device on that same small case."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
prep = pkg.prep
DAY_MS = 86_400_000


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def mmm(xs):
    xs = np.asarray(xs, np.float64)
    return f"{xs.min():.4f} / {np.median(xs):.4f} / {xs.max():.4f}"


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def count_edges_beside_ratings(n, repeats):
    rng = np.random.default_rng(0x5EED0E01)
    persons = max(2, n // 40)
    p = dev(2040 + rng.integers(0, persons, n))
    e = dev(40 + np.minimum(rng.geometric(0.15, n) - 1, 49))
    r = prep.calc_ratings(p, e, 100)
    c = prep.calc_count_edges(p, e, 100)                      # (the warm-up of both)
    assert torch.equal(r[0], c[0]) and torch.equal(r[1], c[1])
    rows = len(r[0])
    del r, c
    t_r, t_c = [], []
    for _ in range(repeats):
        t_r.append(timed(lambda: prep.calc_ratings(p, e, 100))[0])
        t_c.append(timed(lambda: prep.calc_count_edges(p, e, 100))[0])
    ratio = np.array(t_c) / np.array(t_r)
    print(f"(a) {n:,} visit rows, {persons:,} persons, 50 entities, top_n 100 -> {rows:,} rows; seconds, min / median / max over {repeats}")
    print(f"    calc_ratings      {mmm(t_r)}")
    print(f"    calc_count_edges  {mmm(t_c)}")
    print(f"    calc_count_edges / calc_ratings  {mmm(ratio)}", flush=True)


def week_dense(persons, per_person, places, seed):
    rng = np.random.default_rng(seed)
    n = persons * per_person
    return (rng.integers(0, persons, n).astype(np.int64), (40 + rng.integers(0, places, n)).astype(np.int64),
            (1_600_000_000_000 + rng.integers(0, 14 * DAY_MS, n)).astype(np.int64))


def similar_place_edges(persons, per_person, places, repeats):
    cols = week_dense(persons, per_person, places, 0x5EED0E02)
    d = [dev(c) for c in cols]
    out = prep.calc_similar_place_edges(*d, 7 * DAY_MS, 50)   # warm-up
    torch.cuda.synchronize()
    st = prep.similar_place_edges_stats()
    rows = len(out[0])
    del out
    secs, phases = [], []
    for _ in range(repeats):
        t, _ = timed(lambda: prep.calc_similar_place_edges(*d, 7 * DAY_MS, 50))
        s = prep.similar_place_edges_stats()
        secs.append(t)
        phases.append((s["sort_ms"], s["emit_ms"], s["merge_ms"]))
    ph = np.array(phases)
    print(f"(b) {len(cols[0]):,} visit rows, {persons:,} persons, {places:,} places, 14 days, interval 7 days, top_n 50: "
          f"{st['pairs']:,} candidate pairs in {st['chunks']} chunks -> {rows:,} edges")
    print(f"    calc_similar_place_edges seconds  {mmm(secs)}   (min / median / max over {repeats})")
    print(f"    every repeat, seconds             {' '.join(f'{t:.4f}' for t in secs)}")
    print(f"    candidate pairs/s                 {mmm(st['pairs'] / np.array(secs) / 1e9)} G")
    for k, name in enumerate(("sort (rows, pair keys, run lengths)", "emit (windows, pair keys)", "merge (chunks, rank, weights)")):
        print(f"    HIP-event ms, {name:<36} {mmm(ph[:, k])}")
    sys.stdout.flush()


def cpu_context(persons, per_person, places):
    import edge_cases
    cols = week_dense(persons, per_person, places, 0x5EED0E03)
    t0 = time.perf_counter()
    want = edge_cases.similar_place_edges(*cols, 7 * DAY_MS, 50)
    t_cpu = time.perf_counter() - t0
    d = [dev(c) for c in cols]
    prep.calc_similar_place_edges(*d, 7 * DAY_MS, 50)
    t_gpu, got = timed(lambda: prep.calc_similar_place_edges(*d, 7 * DAY_MS, 50))
    same = all(np.array_equal(g.cpu().numpy().view(np.int64), w.view(np.int64)) for g, w in zip(got, want))
    print(f"(c) CPU context only: {len(cols[0]):,} rows, {persons:,} persons, {places:,} places: numpy restatement "
          f"{t_cpu:.3f} s, device {t_gpu:.4f} s (one run each), results identical: {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--visit-rows", type=int, default=25_000_000)
    ap.add_argument("--persons", type=int, default=20_000)
    ap.add_argument("--per-person", type=int, default=200)
    ap.add_argument("--places", type=int, default=5_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    print(f"{torch.cuda.get_device_name(0)}; LOCREC_PREP_PAIR_BUDGET={os.environ.get('LOCREC_PREP_PAIR_BUDGET', 'default (2^28)')}")
    count_edges_beside_ratings(args.visit_rows, args.repeats)
    similar_place_edges(args.persons, args.per_person, args.places, args.repeats)
    cpu_context(max(1, args.persons // 100), args.per_person, args.places)


if __name__ == "__main__":
    main()
