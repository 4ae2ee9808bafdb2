#!/usr/bin/env python3
"""Offline evaluation, measured on one GPU ("Offline evaluation"): three routes from a ranked batch
to its metrics, whole calls timed with a host clock (every call ends in a device synchronise), alternated in one process
(the order reversed every other round), median of --reps after a warm-up of every route.

  (a) prep.evaluate_ranked on device arrays        rows, counts and lists already resident
  (b) prep.evaluate_ranked on host arrays          what the ranked KNN / SG calls return today
  (c) what a caller had before                     the ranked rows on the host, a Python loop per person over sets

Workload: a cfg2-shaped KNN batch (1 M persons x 100 k places, K = 50, 16,384 persons a batch), ranked at widths 10 and
100; a person's relevant list is a seeded draw of places of its target region plus every third recommended place, so
there are hits at every depth.  (a), (b) and (c) must agree (integers exactly, means to 1e-12); the tool stops when
they do not.  Then the hold-out split of a visit table made of the index's rating rows (a seeded timestamp per row, the
cut at the median) against a numpy lexsort / unique version, which must return the same rows and triples.
Every step runs under a watchdog (--step-seconds): a step that does not come back ends the process.  Writes the log to
--out and prints it."""
import argparse
import faulthandler
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUTOFFS = [1, 5, 10, 100]


class step:
    """A step of the run under the watchdog: the traceback of every thread and exit when it takes too long."""
    seconds = 300

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        faulthandler.dump_traceback_later(step.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def host_route(ids, counts, offsets, rel, cutoffs):
    """(c): per person, sets and sums in Python - the definitions of include/locrec.h."""
    nc = len(cutoffs)
    sums, evaluated = np.zeros((nc, 6)), 0
    seen = [set() for _ in cutoffs]
    relevant = np.zeros(len(counts), np.int64)
    for s in range(len(counts)):
        wanted = set(rel[offsets[s]:offsets[s + 1]].tolist())
        row = ids[s, :counts[s]].tolist()
        for j, k in enumerate(cutoffs):
            seen[j].update(row[:k])
        relevant[s] = len(wanted)
        if not wanted:
            continue
        evaluated += 1
        first, hit_at = set(), []
        for r, x in enumerate(row):
            if x in wanted and x not in first:
                hit_at.append(r)
            first.add(x)
        for j, k in enumerate(cutoffs):
            at = [r for r in hit_at if r < k]
            ideal = min(len(wanted), k)
            sums[j] += (len(at) / k, len(at) / len(wanted), 1.0 / (at[0] + 1) if at else 0.0,
                        sum((i + 1) / (r + 1) for i, r in enumerate(at)) / ideal,
                        sum(1.0 / math.log2(r + 2) for r in at) / sum(1.0 / math.log2(r + 2) for r in range(ideal)),
                        1.0 if at else 0.0)
    return {"means": sums / max(evaluated, 1), "coverage": np.array([len(x) for x in seen], np.int64), "evaluated": evaluated,
            "relevant": relevant}


def numpy_split(person, ts, place, region, cut, new_only):
    """The hold-out split with numpy: lexsort / unique and searchsorted over packed (person, place) keys."""
    train = np.flatnonzero(ts < cut)
    rest = np.flatnonzero(ts >= cut)
    span = int(place.max()) - int(place.min()) + 1
    pack = lambda p, q: (p - person.min()) * span + (q - place.min())
    persons = np.unique(person[train])
    keep = np.isin(person[rest], persons)
    if new_only:
        been = np.unique(pack(person[train], place[train]))
        keep &= ~np.isin(pack(person[rest], place[rest]), been)
    rest = rest[keep]
    order = np.lexsort((place[rest], region[rest], person[rest]))
    p, r, q = person[rest][order], region[rest][order], place[rest][order]
    head = np.ones(len(p), bool)
    head[1:] = (p[1:] != p[:-1]) | (r[1:] != r[:-1]) | (q[1:] != q[:-1])
    return train, p[head], r[head], q[head]


def timed(f):
    t = time.perf_counter()
    out = f()
    return (time.perf_counter() - t) * 1e3, out


def measure(say, name, routes, reps, check):
    with step(name + ": warm-up"):
        outs = {k: f() for k, f in routes.items()}
        check(outs)
    ms = {k: [] for k in routes}
    order = list(routes)
    for rep in range(reps):
        for k in (order if rep % 2 == 0 else order[::-1]):
            with step(f"{name}: {k}"):
                ms[k].append(timed(routes[k])[0])
    med = {k: statistics.median(v) for k, v in ms.items()}
    say(f"{name}: median (min - max) of {reps} alternated calls after a warm-up, ms, host clock around the whole call")
    for k, v in ms.items():
        say(f"  {k:44s} {med[k]:10.2f} ({min(v):.2f} - {max(v):.2f})")
    return med, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--persons", type=int, default=1_000_000)
    ap.add_argument("--places", type=int, default=100_000)
    ap.add_argument("--nq", type=int, default=16_384)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--split-rows", type=int, default=10_000_000)
    ap.add_argument("--step-seconds", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval.log"))
    args = ap.parse_args()
    step.seconds = args.step_seconds

    import torch
    if not torch.cuda.is_available():
        sys.exit("eval_probe.py measures on a GPU: none is visible (there is no CPU fallback)")
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from locations_recommender_amd import prep, synth

    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    say(f"device: {torch.cuda.get_device_name(0)}; cutoffs {CUTOFFS}")
    with step("data and index"):
        t0 = time.perf_counter()
        d = synth.knn_dataset_parallel(args.persons, args.places, 0x5EED0002, workers=8)
        ix = pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"],
                          d["c_val"], d["c_dim"], d["p_rowptr"], d["p_idx"].astype(np.int64), 1 + d["p_idx"].astype(np.int64) % 5)
        say(f"KNN: {args.persons} persons x {args.places} places, K = {args.k}, {args.nq} persons a batch "
            f"(data and index {time.perf_counter() - t0:.0f} s)")
    place_ids = np.arange(args.places, dtype=np.int64)
    regions = place_ids % 3
    rng = np.random.default_rng(12)
    persons = d["person_ids"][rng.choice(len(d["person_ids"]), min(args.nq, args.persons), replace=False)]
    targets = rng.integers(0, 3, len(persons)).astype(np.int64)
    for width in (10, 100):
        with step(f"ranked batch, width {width}"):
            ms, (ids, _, counts) = timed(lambda: ix.recommend_ranked_batch(persons, 0.5, 0.5, args.k, place_ids, regions, targets,
                                                                           width, unvisited=True))
        # the lists: eight places of the target region, and every third recommended place
        drawn = 3 * rng.integers(0, args.places // 3, (len(persons), 8)) + targets[:, None]
        taken = [ids[s, :counts[s]:3] for s in range(len(persons))]
        lists = [np.concatenate([drawn[s], taken[s]]) for s in range(len(persons))]
        offsets = np.zeros(len(persons) + 1, np.int64)
        np.cumsum([len(x) for x in lists], out=offsets[1:])
        rel = np.concatenate(lists).astype(np.int64)
        cut = [k for k in CUTOFFS if k <= width]
        say(f"width {width}: the ranked batch itself {ms:.1f} ms; {int(counts.sum())} rows, {len(rel)} relevant ids, cutoffs {cut}")
        D = [dev(ids), dev(counts), dev(offsets), dev(rel)]
        routes = {"(a) evaluate_ranked, device arrays": lambda: prep.evaluate_ranked(*D, cut),
                  "(b) evaluate_ranked, host arrays": lambda: prep.evaluate_ranked(ids, counts, offsets, rel, cut),
                  "(c) rows on the host, Python sets per person": lambda: host_route(ids, counts, offsets, rel, cut)}

        def check(outs):
            a, b, c = (outs[k] for k in routes)
            assert a["means"].tobytes() == b["means"].tobytes() and np.array_equal(a["coverage"], b["coverage"]), "(a) differs from (b)"
            assert a["evaluated"] == b["evaluated"] == c["evaluated"] and np.array_equal(b["coverage"], c["coverage"])
            assert np.array_equal(b["relevant"], c["relevant"]) and np.allclose(b["means"], c["means"], rtol=1e-12, atol=0)
            say(f"  evaluated {b['evaluated']}; at the last cutoff: precision {b['means'][-1, 0]:.4f} recall {b['means'][-1, 1]:.4f} "
                f"ndcg {b['means'][-1, 4]:.4f} hit rate {b['means'][-1, 5]:.4f} coverage {int(b['coverage'][-1])}; "
                f"stats {prep.evaluate_ranked_stats()}")
        med, _ = measure(say, f"width {width}", routes, args.reps, check)
        k = list(routes)
        say(f"  (c) / (a) = {med[k[2]] / med[k[0]]:.1f}; (c) / (b) = {med[k[2]] / med[k[1]]:.1f}; (b) / (a) = {med[k[1]] / med[k[0]]:.2f}")
    ix.close()

    # the hold-out split: the index's rating rows as a visit table
    n = min(args.split_rows, len(d["p_idx"]))
    rowptr = np.asarray(d["p_rowptr"], np.int64)
    last = int(np.searchsorted(rowptr, n, "right")) - 1
    n = int(rowptr[last])
    visits = {"person_id": np.repeat(np.asarray(d["person_ids"][:last], np.int64), np.diff(rowptr[:last + 1])),
              "place_id": np.asarray(d["p_idx"][:n], np.int64)}
    visits["timestamp"] = np.random.default_rng(14).integers(0, 365 * 86_400_000, n).astype(np.int64)
    visits["region_id"] = visits["place_id"] % 3
    visits["category_id"] = visits["place_id"] % 40
    cut_ts = int(np.median(visits["timestamp"]))
    DV = {k: dev(v) for k, v in visits.items()}
    say(f"hold-out split: {n} visits of {last} persons, the cut at the median timestamp, new places only")
    def on_device():
        out = prep.holdout_split(DV, cut_ts, True)
        torch.cuda.synchronize()                     # (the train columns are gathered by torch, on its own stream)
        return out
    routes = {"prep.holdout_split, device arrays": on_device,
              "prep.holdout_split, host arrays": lambda: prep.holdout_split(visits, cut_ts, True),
              "numpy lexsort / unique": lambda: numpy_split(visits["person_id"], visits["timestamp"], visits["place_id"],
                                                            visits["region_id"], cut_ts, True)}

    def check_split(outs):
        a, b, c = (outs[k] for k in routes)
        for (train, held), name in ((a, "device"), (b, "host")):
            h = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in held.items()}
            t = train["person_id"].cpu().numpy() if torch.is_tensor(train["person_id"]) else train["person_id"]
            assert np.array_equal(t, visits["person_id"][c[0]]), name
            assert (np.array_equal(h["person_id"], c[1]) and np.array_equal(h["region_id"], c[2]) and
                    np.array_equal(h["place_id"], c[3])), name
        say(f"  train rows {len(c[0])}, held-out triples {len(c[1])}")
    med, _ = measure(say, "hold-out split", routes, max(3, args.reps // 2), check_split)
    k = list(routes)
    say(f"  numpy / device = {med[k[2]] / med[k[0]]:.1f}; numpy / host = {med[k[2]] / med[k[1]]:.1f}")

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
