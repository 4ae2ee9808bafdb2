#!/usr/bin/env python3
"""By category, measured on one GPU ("By category"): the ranked stage alone on the rows of a
cfg2-shaped KNN batch (1 M persons x 100 k places, K = 50, 16,384 persons a batch, N = 10, about 20 categories over the
places) as device arrays, whole calls timed with a host clock (every call ends in a device synchronise), all routes in one
process, alternated with the order reversed every other round, median of --reps after a warm-up of every route.

  (a)  the plain ranker                  prep.rank_recommendations_batch
  (a') the identity dispatch             ..._by_category with every cap 2^63 - 1: must equal (a) within the spread
  (b1) a one-category allow-list         ..._by_category, allowed = one category per segment
  (b2) cap 2, no list                    ..._by_category, max_per_category = 2
  (b3) both, with a 1 % circle           ..._by_category, allowed, cap 2, circles
  (c)  what a caller has today           the rows to the host, the numpy restatement of (b2) - vectorised over the batch:
                                         a python loop per segment takes minutes at this shape -, N rows back

(b2) and (c) must agree on ids and score bits, (a') and (a) likewise; the tool stops when they do not.  The whole KNN
call (recommend_ranked_batch_by_category, cap 2) is recorded once beside them, for orientation.  Writes the log to --out
and prints it."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from near_rank_probe import LIMIT, centres, coordinates, measure, one_percent_radius  # noqa: E402

NO_CAP = 2 ** 63 - 1


def host_route(off_dev, ids_dev, scores_dev, place_ids, regions, cats, targets, cap):
    """(c): ids and scores to the host; membership, the order (score desc, id, row) per segment, a running count per
    (segment, category), the first N rows under the cap.  place_ids is ascending and lists every place once."""
    off, ids, scores = off_dev.cpu().numpy(), ids_dev.cpu().numpy(), scores_dev.cpu().numpy()
    nseg = len(targets)
    seg = np.repeat(np.arange(nseg), np.diff(off))
    at = np.searchsorted(place_ids, ids)
    at[at >= len(place_ids)] = 0
    keep = (place_ids[at] == ids) & (regions[at] == targets[seg])
    row = np.flatnonzero(keep)
    seg, at = seg[row], at[row]
    order = np.lexsort((row, ids[row], -scores[row], seg))              # (finite scores: no NaN, no zero of either sign)
    seg, at, row = seg[order], at[order], row[order]
    key = seg * (int(cats.max()) + 1) + cats[at]
    by_cat = np.argsort(key, kind="stable")
    k = key[by_cat]
    head = np.r_[True, k[1:] != k[:-1]]
    start = np.maximum.accumulate(np.where(head, np.arange(len(k)), 0))
    ok = np.zeros(len(k), bool)
    ok[by_cat] = np.arange(len(k)) - start < cap
    seg, row = seg[ok], row[ok]
    first = np.searchsorted(seg, np.arange(nseg))
    j = np.arange(len(seg)) - first[seg]
    take = j < LIMIT
    out_ids, out_scores = np.full((nseg, LIMIT), -1, np.int64), np.zeros((nseg, LIMIT))
    out_ids[seg[take], j[take]] = ids[row[take]]
    out_scores[seg[take], j[take]] = scores[row[take]]
    return out_ids, out_scores, np.bincount(seg[take], minlength=nseg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--persons", type=int, default=1_000_000)
    ap.add_argument("--places", type=int, default=100_000)
    ap.add_argument("--nq", type=int, default=16_384)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--categories", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_category.log"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("rank_category_probe.py measures on a GPU: none is visible (there is no CPU fallback)")
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from locations_recommender_amd import prep, synth

    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say(f"device: {torch.cuda.get_device_name(0)}; N = {LIMIT}; {args.categories} categories")
    t0 = time.perf_counter()
    d = synth.knn_dataset_parallel(args.persons, args.places, 0x5EED0002, workers=8)
    ix = pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"],
                      d["c_val"], d["c_dim"], d["p_rowptr"], d["p_idx"].astype(np.int64), 1 + d["p_idx"].astype(np.int64) % 5)
    say(f"KNN: {args.persons} persons x {args.places} places, K = {args.k}, {args.nq} persons a batch "
        f"(data and index {time.perf_counter() - t0:.0f} s)")
    place_ids = np.arange(args.places, dtype=np.int64)
    regions = place_ids % 3
    rng = np.random.default_rng(12)
    cats = rng.integers(0, args.categories, args.places).astype(np.int64)
    plat, plon = coordinates(regions, 11)
    persons = d["person_ids"][rng.choice(len(d["person_ids"]), min(args.nq, args.persons), replace=False)]
    nseg = len(persons)
    targets = rng.integers(0, 3, nseg).astype(np.int64)
    clat, clon = centres(targets, 13)
    r1 = np.array([one_percent_radius(t) for t in targets])
    one = rng.integers(0, args.categories, nseg).astype(np.int64)
    pw, cw = 0.5, 0.5
    off, ids, scores = ix.recommend_batch(persons, pw, cw, args.k)
    say(f"  rows of the batch: {off[-1]} ({off[-1] / nseg:.0f} a person)")
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    D = {n: dev(v) for n, v in dict(off=off, ids=ids, sc=scores, pl=place_ids, reg=regions, cat=cats, plat=plat, plon=plon, t=targets,
                                    clat=clat, clon=clon, r1=r1, aoff=np.arange(nseg + 1, dtype=np.int64), aid=one,
                                    cap2=np.full(nseg, 2, np.int64), nocap=np.full(nseg, NO_CAP, np.int64)).items()}
    by = lambda **kw: prep.rank_recommendations_batch_by_category(D["off"], D["ids"], D["sc"], D["pl"], D["reg"], D["t"], LIMIT,
                                                                  D["cat"], **kw)
    circles = (D["plat"], D["plon"], D["clat"], D["clon"], D["r1"])
    host = lambda x: tuple(None if a is None else a.cpu().numpy() for a in x)
    routes = {"(a)  plain ranker": lambda: prep.rank_recommendations_batch(D["off"], D["ids"], D["sc"], D["pl"], D["reg"], D["t"], LIMIT),
              "(a') identity dispatch": lambda: by(max_per_category=D["nocap"]),
              "(b1) one-category allow-list": lambda: by(allowed=(D["aoff"], D["aid"])),
              "(b2) cap 2": lambda: by(max_per_category=D["cap2"]),
              "(b3) list, cap 2, 1 % circle": lambda: by(allowed=(D["aoff"], D["aid"]), max_per_category=D["cap2"], circles=circles),
              "(c)  rows to the host, numpy": lambda: host_route(D["off"], D["ids"], D["sc"], place_ids, regions, cats, targets, 2)}

    def check(outs):
        a, ai, b1, b2, b3, c = (outs[k] for k in routes)
        a, ai, b1, b2, b3 = host(a), host(ai), host(b1), host(b2), host(b3)
        assert np.array_equal(a[0], ai[0]) and a[1].tobytes() == ai[1].tobytes(), "(a') differs from (a)"
        assert np.array_equal(b2[0], c[0]) and b2[1].tobytes() == c[1].tobytes() and np.array_equal(b2[3], c[2]), "(b2) differs from (c)"
        say(f"  rows returned: (a) {int(a[2].sum())}, (b1) {int(b1[3].sum())}, (b2) {int(b2[3].sum())}, (b3) {int(b3[3].sum())}; "
            f"rows (b2) changes against (a): {int((a[0] != b2[0]).any(axis=1).sum())} of {nseg} segments")
    med, _ = measure(say, "KNN rows, the segmented ranker alone (device arrays)", routes, args.reps, check)
    k = list(routes)
    say(f"  (a') / (a) = {med[k[1]] / med[k[0]]:.3f}; (b1) / (a) = {med[k[2]] / med[k[0]]:.3f}; (b2) / (a) = {med[k[3]] / med[k[0]]:.3f}; "
        f"(b3) / (a) = {med[k[4]] / med[k[0]]:.3f}")
    say(f"  (c) / (b1) = {med[k[5]] / med[k[2]]:.1f}; (c) / (b2) = {med[k[5]] / med[k[3]]:.1f}; (c) / (b3) = {med[k[5]] / med[k[4]]:.1f}")
    whole = {"whole KNN call, plain ranked batch": lambda: ix.recommend_ranked_batch(persons, pw, cw, args.k, place_ids, regions, targets, LIMIT),
             "whole KNN call, by category, cap 2": lambda: ix.recommend_ranked_batch_by_category(
                 persons, pw, cw, args.k, place_ids, regions, targets, LIMIT, cats, max_per_category=np.full(nseg, 2, np.int64))}

    def check_whole(outs):
        got, b2 = outs["whole KNN call, by category, cap 2"], host(routes["(b2) cap 2"]())
        assert np.array_equal(got[0], b2[0]) and np.array_equal(got[3], b2[3]), "the KNN call differs from the ranker on its rows"
    measure(say, "KNN, the whole call (host arrays in and out)", whole, args.reps, check_whole)
    ix.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
