#!/usr/bin/env python3
"""Within reach, measured on one GPU ("Within reach"): three routes to a ranked batch, whole calls
timed with a host clock (every call ends in a device synchronise), alternated in one process (the order of the routes
reversed every other round, so that no route always follows the same one), median of --reps after a
warm-up of every route.

  (a) the plain ranked batch                      recommend_ranked_batch
  (b) the near ranked batch                       recommend_ranked_batch_near, every radius +inf, and a radius that keeps
                                                  about 1 % of a region's places
  (c) what a caller had before the near calls     recommend_batch's rows to the host, prep.distance_meters of every row's
                                                  place from its request's centre, a host filter,
                                                  prep.rank_recommendations_batch

Workloads: a cfg2-shaped KNN batch (1 M persons x 100 k places, K = 50, 16,384 persons a batch) and a cfg3 SG batch of
256 requests.  Places lie uniformly (seeded) in a box of 0.03 degrees per region; a request's centre lies inside its
region's box, far enough from the edge for the 1 % circle.  (b) at the 1 % radius and (c) must agree on ids and score bits;
the tool stops when they do not.  Writes the log to --out and prints it."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOX = 0.03
CORNERS = ((48.85, 2.30), (40.40, -3.72), (-33.90, 151.19))     # region -> the box's south-west corner
METERS_PER_DEGREE = 6371000.0 * math.pi / 180.0
LIMIT = 10


def coordinates(regions, seed):
    rng = np.random.default_rng(seed)
    lat0 = np.array([CORNERS[r][0] for r in regions])
    lon0 = np.array([CORNERS[r][1] for r in regions])
    return lat0 + BOX * rng.random(len(regions)), lon0 + BOX * rng.random(len(regions))


def one_percent_radius(region):
    """The radius of a circle whose area is 1 % of the region's box."""
    lat = CORNERS[region][0] + BOX / 2
    area = (BOX * METERS_PER_DEGREE) * (BOX * METERS_PER_DEGREE * math.cos(math.radians(lat)))
    return math.sqrt(0.01 * area / math.pi)


def centres(targets, seed):
    """A centre per request inside its region's box, a 1 % radius (about 0.002 degrees of latitude) away from the edge."""
    rng = np.random.default_rng(seed)
    m = 0.2 * BOX
    lat0 = np.array([CORNERS[t][0] for t in targets])
    lon0 = np.array([CORNERS[t][1] for t in targets])
    return lat0 + m + (BOX - 2 * m) * rng.random(len(targets)), lon0 + m + (BOX - 2 * m) * rng.random(len(targets))


def host_route(prep, rows, place_ids, regions, plat, plon, targets, clat, clon, radius):
    """(c): the rows are on the host; one distance per row, a filter, the plain segmented ranker."""
    off, ids, scores = rows
    seg = np.repeat(np.arange(len(targets)), np.diff(off))
    at = np.searchsorted(place_ids, ids)
    at[at >= len(place_ids)] = 0
    known = place_ids[at] == ids                                    # (a row that is no place has no coordinates)
    d = np.full(len(ids), np.inf)
    d[known] = prep.distance_meters(clat[seg[known]], clon[seg[known]], plat[at[known]], plon[at[known]])
    keep = d <= radius[seg]
    new_off = np.zeros(len(off), np.int64)
    np.cumsum(np.bincount(seg[keep], minlength=len(targets)), out=new_off[1:])
    return prep.rank_recommendations_batch(new_off, ids[keep], scores[keep], place_ids, regions, targets, LIMIT)


def timed(f):
    t = time.perf_counter()
    out = f()
    return (time.perf_counter() - t) * 1e3, out


def measure(say, name, routes, reps, check):
    """routes: label -> callable.  One warm-up of every route, then `reps` alternated rounds."""
    outs = {k: f() for k, f in routes.items()}
    check(outs)
    ms = {k: [] for k in routes}
    order = list(routes)
    for rep in range(reps):                       # forwards and backwards in turn: no route always follows the same one
        for k in (order if rep % 2 == 0 else order[::-1]):
            ms[k].append(timed(routes[k])[0])
    med = {k: statistics.median(v) for k, v in ms.items()}
    say(f"{name}: median (min - max) of {reps} alternated calls after a warm-up, ms, host clock around the whole call")
    for k, v in ms.items():
        say(f"  {k:34s} {med[k]:10.2f} ({min(v):.2f} - {max(v):.2f})")
    return med, outs


def pad(a, width, fill):
    out = np.full((a.shape[0], width), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def same_rows(near, host):
    """ids and score bits of (b) against (c), whatever the two forms' widths."""
    w = max(near[0].shape[1], host[0].shape[1])
    return (np.array_equal(pad(near[0], w, -1), pad(np.asarray(host[0]), w, -1)) and
            pad(near[1], w, 0.0).tobytes() == pad(np.asarray(host[1]), w, 0.0).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--persons", type=int, default=1_000_000)
    ap.add_argument("--places", type=int, default=100_000)
    ap.add_argument("--nq", type=int, default=16_384)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--sg-requests", type=int, default=256)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip-knn", action="store_true")
    ap.add_argument("--skip-sg", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "near_rank.log"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("near_rank_probe.py measures on a GPU: none is visible (there is no CPU fallback)")
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from locations_recommender_amd import prep, synth

    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say(f"device: {torch.cuda.get_device_name(0)}; N = {LIMIT}")
    if not args.skip_knn:
        t0 = time.perf_counter()
        d = synth.knn_dataset_parallel(args.persons, args.places, 0x5EED0002, workers=8)
        ix = pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"],
                          d["c_val"], d["c_dim"], d["p_rowptr"], d["p_idx"].astype(np.int64), 1 + d["p_idx"].astype(np.int64) % 5)
        say(f"KNN: {args.persons} persons x {args.places} places, K = {args.k}, {args.nq} persons a batch "
            f"(data and index {time.perf_counter() - t0:.0f} s)")
        place_ids = np.arange(args.places, dtype=np.int64)           # the index's place dimensions
        regions = place_ids % 3
        plat, plon = coordinates(regions, 11)
        rng = np.random.default_rng(12)
        persons = d["person_ids"][rng.choice(len(d["person_ids"]), min(args.nq, args.persons), replace=False)]
        targets = rng.integers(0, 3, len(persons)).astype(np.int64)
        clat, clon = centres(targets, 13)
        inf = np.full(len(persons), np.inf)
        r1 = np.array([one_percent_radius(t) for t in targets])
        pw, cw = 0.5, 0.5
        near = lambda rad: ix.recommend_ranked_batch_near(persons, pw, cw, args.k, place_ids, regions, plat, plon, targets, clat,
                                                          clon, rad, LIMIT)
        routes = {"(a) recommend_ranked_batch": lambda: ix.recommend_ranked_batch(persons, pw, cw, args.k, place_ids, regions,
                                                                                    targets, LIMIT),
                  "(b) near, every radius +inf": lambda: near(inf),
                  "(b) near, 1 % of the region": lambda: near(r1),
                  "(c) rows to the host, filter, rank": lambda: host_route(prep, ix.recommend_batch(persons, pw, cw, args.k), place_ids,
                                                                           regions, plat, plon, targets, clat, clon, r1)}

        def check(outs):
            a, bi, b1, c = (outs[k] for k in routes)
            assert np.array_equal(a[0], bi[0]) and a[1].tobytes() == bi[1].tobytes(), "(b) at +inf differs from (a)"
            assert same_rows(b1, c), "(b) at the 1 % radius differs from (c)"
            rows = ix.recommend_batch(persons, pw, cw, args.k)[0][-1]
            say(f"  rows of the batch: {rows} ({rows / len(persons):.0f} a person); rows returned: (a) {int(a[2].sum())}, "
                f"(b, 1 %) {int(b1[3].sum())}; mean distance of a returned row {b1[2][b1[0] >= 0].mean():.1f} m, "
                f"radius {r1.mean():.1f} m")
        med, _ = measure(say, "KNN", routes, args.reps, check)
        k = list(routes)
        say(f"  (b, +inf) / (a) = {med[k[1]] / med[k[0]]:.3f}; (b, 1 %) / (a) = {med[k[2]] / med[k[0]]:.3f}; "
            f"(c) / (b, 1 %) = {med[k[3]] / med[k[2]]:.2f}")
        # the ranked stage alone: the ranker on the same rows, device arrays, events around the call
        off, ids, scores = ix.recommend_batch(persons, pw, cw, args.k)
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
        D = {n: dev(v) for n, v in dict(off=off, ids=ids, sc=scores, pl=place_ids, reg=regions, plat=plat, plon=plon, t=targets,
                                        clat=clat, clon=clon, inf=inf, r1=r1).items()}
        stage = {"ranker alone, plain": lambda: prep.rank_recommendations_batch(D["off"], D["ids"], D["sc"], D["pl"], D["reg"], D["t"], LIMIT),
                 "ranker alone, near +inf": lambda: prep.rank_recommendations_batch_near(
                     D["off"], D["ids"], D["sc"], D["pl"], D["reg"], D["plat"], D["plon"], D["t"], D["clat"], D["clon"], D["inf"], LIMIT),
                 "ranker alone, near 1 %": lambda: prep.rank_recommendations_batch_near(
                     D["off"], D["ids"], D["sc"], D["pl"], D["reg"], D["plat"], D["plon"], D["t"], D["clat"], D["clon"], D["r1"], LIMIT)}
        smed, _ = measure(say, "KNN rows, the segmented ranker alone (device arrays)", stage, args.reps, lambda outs: None)
        k = list(stage)
        say(f"  near +inf / plain = {smed[k[1]] / smed[k[0]]:.3f}; near 1 % / plain = {smed[k[2]] / smed[k[0]]:.3f}")
        ix.close()
        del d

    if not args.skip_sg:
        g = synth.sg_dataset(seed=0x5EED0003)
        person0 = int(g["first_person"])
        n_persons = int(g["source_id"].max()) - person0 + 1
        n_places = person0 - 40
        sg = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"])
        say(f"SG: cfg3, {sg.info()['vertices']} vertices, {n_places} places, {args.sg_requests} requests, epsilon 0.01, 20 iterations")
        rng = np.random.default_rng(1024)
        place_ids = np.arange(40, 40 + n_places, dtype=np.int64)
        regions = rng.integers(0, 3, n_places).astype(np.int64)
        plat, plon = coordinates(regions, 21)
        v = (person0 + rng.choice(n_persons, args.sg_requests, replace=False)).astype(np.int64)
        targets = rng.integers(0, 3, len(v)).astype(np.int64)
        clat, clon = centres(targets, 23)
        inf = np.full(len(v), np.inf)
        r1 = np.array([one_percent_radius(t) for t in targets])
        near = lambda rad: sg.recommend_ranked_batch_near(v, 0.15, 0.01, 20, place_ids, regions, plat, plon, targets, clat, clon,
                                                          rad, LIMIT)
        routes = {"(a) recommend_ranked_batch": lambda: sg.recommend_ranked_batch(v, 0.15, 0.01, 20, place_ids, regions, targets, LIMIT),
                  "(b) near, every radius +inf": lambda: near(inf),
                  "(b) near, 1 % of the region": lambda: near(r1),
                  "(c) rows to the host, filter, rank": lambda: host_route(prep, sg.recommend_batch(v, 0.15, 0.01, 20)[:3], place_ids,
                                                                           regions, plat, plon, targets, clat, clon, r1)}

        def check(outs):
            a, bi, b1, c = (outs[k] for k in routes)
            assert np.array_equal(a[0], bi[0]) and a[1].tobytes() == bi[1].tobytes(), "(b) at +inf differs from (a)"
            assert same_rows(b1, c), "(b) at the 1 % radius differs from (c)"
            rows = sg.recommend_batch(v, 0.15, 0.01, 20)[0][-1]
            say(f"  rows of the batch: {rows} ({rows / len(v):.0f} a request); rows returned: (a) {int(a[2].sum())}, "
                f"(b, 1 %) {int(b1[3].sum())}")
        med, _ = measure(say, "SG", routes, args.reps, check)
        k = list(routes)
        say(f"  (b, +inf) / (a) = {med[k[1]] / med[k[0]]:.3f}; (b, 1 %) / (a) = {med[k[2]] / med[k[0]]:.3f}; "
            f"(c) / (b, 1 %) = {med[k[3]] / med[k[2]]:.2f}")
        sg.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
