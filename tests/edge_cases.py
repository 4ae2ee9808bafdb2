"""The stochastic graph's four edge families restated on the CPU from the Scala text (plain dicts and loops, no use
of the package), and the seeded inputs the CPU and GPU tests of those families share.

    count_edges          PersonLikesPlace / PersonLikesCategory / CategorySelectedPlace   stochastic/PersonLikesPlace.scala:12-37
    similar_place_edges  PlaceSimilarPlace.calcPlaceSimilarPlaceEdges                      stochastic/PlaceSimilarPlace.scala:18-63
    stochastic_graph     StochasticGraphBuilderMain.generateStochasticGraph                stochastic/StochasticGraphBuilderMain.scala:47-66
"""
import numpy as np

DAY_MS = 86_400_000
INTERVAL_MS = 7 * DAY_MS          # PlaceSimilarPlace.scala:13-14
TOP_N = {"place_place": 50, "category_place": 100, "person_place": 100, "person_category": 100}


def rank_and_normalise(counts, top_n):
    """counts: {(source, target): count}.  Window.partitionBy(source).orderBy(count.desc), rank() <= top_n, then
    count / sum of the KEPT counts of the source (PersonLikesPlace.scala:17-31).  Rows by (source, target)."""
    by_source = {}
    for (s, t), c in counts.items():
        by_source.setdefault(s, []).append((t, c))
    src, dst, w = [], [], []
    for s in sorted(by_source):
        items = by_source[s]
        desc = sorted((c for _, c in items), reverse=True)
        kept = [(t, c) for t, c in items if 1 + desc.index(c) <= top_n]     # rank = 1 + number of strictly larger counts
        total = sum(c for _, c in kept)
        for t, c in sorted(kept):
            src.append(s)
            dst.append(t)
            w.append(float(c) / float(total))
    return np.array(src, np.int64), np.array(dst, np.int64), np.array(w, np.float64)


def count_edges(source_ids, target_ids, top_n):
    """groupBy(source, target).agg(count("*")), then rank_and_normalise."""
    counts = {}
    for key in zip(np.asarray(source_ids).tolist(), np.asarray(target_ids).tolist()):
        counts[key] = counts.get(key, 0) + 1
    return rank_and_normalise(counts, top_n)


def covisit_counts_loops(person_ids, place_ids, timestamps, interval):
    """The self-join of PlaceSimilarPlace.scala:29-36 as the literal double loop over each person's rows."""
    rows = {}
    for p, pl, ts in zip(np.asarray(person_ids).tolist(), np.asarray(place_ids).tolist(), np.asarray(timestamps).tolist()):
        rows.setdefault(p, []).append((pl, ts))
    counts = {}
    for visits in rows.values():
        for place, ts in visits:
            for that_place, that_ts in visits:
                if place != that_place and abs(ts - that_ts) <= interval:
                    counts[(place, that_place)] = counts.get((place, that_place), 0) + 1
    return counts


def covisit_counts(person_ids, place_ids, timestamps, interval):
    """The same self-join with one outer comparison per person (for persons of thousands of rows)."""
    person, place, ts = (np.asarray(a, np.int64) for a in (person_ids, place_ids, timestamps))
    counts = {}
    for p in np.unique(person):
        sel = person == p
        pl, t = place[sel], ts[sel]
        ids, local = np.unique(pl, return_inverse=True)
        joined = (pl[:, None] != pl[None, :]) & (np.abs(t[:, None] - t[None, :]) <= interval)
        a, b = np.nonzero(joined)
        per_pair = np.bincount(local[a] * len(ids) + local[b], minlength=len(ids) ** 2)
        for k in np.flatnonzero(per_pair):
            key = (int(ids[k // len(ids)]), int(ids[k % len(ids)]))
            counts[key] = counts.get(key, 0) + int(per_pair[k])
    return counts


def similar_place_edges(person_ids, place_ids, timestamps, interval, top_n, loops=False):
    fn = covisit_counts_loops if loops else covisit_counts
    return rank_and_normalise(fn(person_ids, place_ids, timestamps, interval), top_n)


def stochastic_graph_families(pv, interval=INTERVAL_MS):
    """The four families in generateStochasticGraph's order (:48-57), each as (source, target, weight)."""
    return [similar_place_edges(pv["person_id"], pv["place_id"], pv["timestamp"], interval, TOP_N["place_place"]),
            count_edges(pv["category_id"], pv["place_id"], TOP_N["category_place"]),
            count_edges(pv["person_id"], pv["place_id"], TOP_N["person_place"]),
            count_edges(pv["person_id"], pv["category_id"], TOP_N["person_category"])]


# ---- inputs ---------------------------------------------------------------------------------------------------------

# days as the timestamp unit, interval = 7: person 1 visits A@0, B@1, B@2, C@8; person 2 visits A@0, B@3
A, B, C_ = 10, 20, 30
HAND = dict(person=np.array([1, 1, 1, 1, 2, 2], np.int64), place=np.array([A, B, B, C_, A, B], np.int64),
            ts=np.array([0, 1, 2, 8, 0, 3], np.int64), interval=7)
HAND_TOP_50 = [(A, B, 1.0), (B, A, 0.6), (B, C_, 0.4), (C_, B, 1.0)]
HAND_TOP_1 = [(A, B, 1.0), (B, A, 1.0), (C_, B, 1.0)]


def covisit_case(seed, n, persons=50, places=40, days=90, equal_timestamps=False, negative_ids=False):
    """(person, place, timestamp in ms) rows: ~n / persons visits per person over `days` days, so windows of 7 days are
    partial; equal_timestamps draws the timestamps from a few dozen values."""
    rng = np.random.default_rng(seed)
    person = 2040 + rng.integers(0, persons, n)
    place = 40 + np.minimum(rng.geometric(0.08, n) - 1, places - 1)
    if equal_timestamps:
        ts = 1_600_000_000_000 + rng.integers(0, 3 * days, n) * (DAY_MS // 3)
    else:
        ts = 1_600_000_000_000 + rng.integers(0, days * DAY_MS, n)
    if negative_ids:
        person, place = person - 2040 - persons // 2, place - 40 - places // 2
    return person.astype(np.int64), place.astype(np.int64), ts.astype(np.int64)


def long_window_person(seed, rows=3000, places=40, person=777):
    """One person with `rows` visits inside one interval: every row's window is the whole person (~rows^2 pairs)."""
    rng = np.random.default_rng(seed)
    return (np.full(rows, person, np.int64), (40 + rng.integers(0, places, rows)).astype(np.int64),
            (1_600_000_000_000 + rng.integers(0, 6 * DAY_MS, rows)).astype(np.int64))


def budget_case():
    """20 000 rows that contain the 3 000-row person (~9 M of its own candidate pairs), shuffled."""
    a = covisit_case(31, 17_000)
    b = long_window_person(32)
    cols = [np.concatenate([x, y]) for x, y in zip(a, b)]
    order = np.random.default_rng(33).permutation(len(cols[0]))
    return tuple(c[order] for c in cols)


def run_budget_case(pkg, out_path):
    """Runs budget_case() in THIS process (whose LOCREC_PREP_PAIR_BUDGET the caller chose) and stores the result."""
    s, t, w = pkg.prep.calc_similar_place_edges(*budget_case(), INTERVAL_MS, 50)
    stats = pkg.prep.similar_place_edges_stats()
    np.savez(out_path, source=s, target=t, weight=w, chunks=stats["chunks"], pairs=stats["pairs"])
