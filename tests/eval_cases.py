"""Cases and models of the offline evaluation (locrec_eval_ranked_batch, locrec_holdout_split).  The models are written
with Python sets, lists and math.fsum and share no code with the library; tests/test_eval_cases.py checks them against
answers worked by hand.  The generators are seeded: a case is the same on every machine."""
import math

import numpy as np

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
U = 2.0 ** -53


# ---- the model of the evaluator ----------------------------------------------------------------------------------------

def model_segment(row, count, relevant, cutoffs):
    """-> (R, [(hits, precision, recall, rr, ap, ndcg) per cutoff]) of one segment, by the definitions of the header."""
    wanted = set(int(x) for x in relevant)
    R = len(wanted)
    out = []
    for k in cutoffs:
        if R == 0:
            out.append((0, 0.0, 0.0, 0.0, 0.0, 0.0))
            continue
        L = min(int(k), int(count))
        seen, hit_at = set(), []
        for r in range(L):
            x = int(row[r])
            if x in wanted and x not in seen:
                hit_at.append(r)
            seen.add(x)
        hits = len(hit_at)
        ideal = min(R, int(k))
        ap = math.fsum((i + 1) / (r + 1) for i, r in enumerate(hit_at)) / ideal
        ndcg = math.fsum(1.0 / math.log2(r + 2) for r in hit_at) / math.fsum(1.0 / math.log2(r + 2) for r in range(ideal))
        out.append((hits, hits / int(k), hits / R, 1.0 / (hit_at[0] + 1) if hit_at else 0.0, ap, ndcg))
    return R, out


def model_eval(rec_ids, rec_counts, rel_offsets, rel_ids, cutoffs):
    """The whole call: relevant[S], hits[S, C], metrics[S, C, 5], means[C, 6], coverage[C], evaluated."""
    S, C = len(rec_counts), len(cutoffs)
    relevant, hits, metrics = np.zeros(S, np.int64), np.zeros((S, C), np.int64), np.zeros((S, C, 5))
    for s in range(S):
        R, per = model_segment(rec_ids[s], rec_counts[s], rel_ids[rel_offsets[s]:rel_offsets[s + 1]], cutoffs)
        relevant[s] = R
        for j, m in enumerate(per):
            hits[s, j], metrics[s, j] = m[0], m[1:]
    live = [s for s in range(S) if relevant[s] > 0]
    means = np.zeros((C, 6))
    for j in range(C):
        if live:
            for m in range(5):
                means[j, m] = math.fsum(metrics[s, j, m] for s in live) / len(live)
            means[j, 5] = sum(1 for s in live if hits[s, j] > 0) / len(live)
    coverage = np.array([len({int(rec_ids[s][r]) for s in range(S) for r in range(min(int(k), int(rec_counts[s])))})
                         for k in cutoffs], np.int64)
    return {"relevant": relevant, "hits": hits, "metrics": metrics, "means": means, "coverage": coverage, "evaluated": len(live)}


def assert_matches_model(got, want, cutoffs, n_segments, per_segment=True):
    """The tolerances of the evaluator's contract: integers and the one-division metrics exact; ap and ndcg within
    4 (k + 2) 2^-53 relative (at most k positive terms, each within 2 ulp, summed in any fixed order, one division); the
    means within (n_segments + 4 (k + 2)) 2^-53 relative of the model's fsum."""
    assert np.array_equal(np.asarray(got["relevant"]), want["relevant"])
    assert np.array_equal(np.asarray(got["coverage"]), want["coverage"])
    assert int(got["evaluated"]) == want["evaluated"]
    if per_segment:
        assert np.array_equal(np.asarray(got["hits"]), want["hits"])
        gm, wm = np.asarray(got["metrics"]), want["metrics"]
        assert gm.shape == wm.shape
        assert np.array_equal(gm[:, :, :3], wm[:, :, :3]), "precision, recall and rr are one division of exact integers"
        for j, k in enumerate(cutoffs):
            tol = 4 * (int(k) + 2) * U
            assert (np.abs(gm[:, j, 3:] - wm[:, j, 3:]) <= tol * np.abs(wm[:, j, 3:])).all(), (j, k)
    for j, k in enumerate(cutoffs):
        tol = (n_segments + 4 * (int(k) + 2)) * U
        g, w = np.asarray(got["means"])[j], want["means"][j]
        assert (np.abs(g - w) <= tol * np.abs(w)).all(), (j, k, g, w)


# ---- cases of the evaluator ------------------------------------------------------------------------------------------

def eval_case(seed, n_segments, width):
    """n_segments rows of `width`: the counts cycle through width, width - 1, 1 and 0, the lists through a mix of the
    row's ids and strangers, duplicates, the extreme ids, one id, ids no row has (and -1), and the empty list.  Every
    fourth row repeats its first id; the padding is -1 in even rows and a RELEVANT id in odd ones (it is never read).
    -> (rec_ids[S, W], rec_counts[S], rel_offsets[S + 1], rel_ids)."""
    rng = np.random.default_rng(seed)
    specials = [I64_MIN, I64_MAX, -5, -4242, -1]
    pool = np.array(list(range(-width - 3, 2 * width + 12)) + specials[:-1], np.int64)   # (-1 is already in the range)
    rec = np.empty((n_segments, width), np.int64)
    counts = np.zeros(n_segments, np.int64)
    lists = []
    for s in range(n_segments):
        c = max(0, min(width, (width, width - 1, 1, 0)[s % 4]))
        row = rng.permutation(pool)[:width].copy()
        kind = (5, 2, 4, 1, 3, 0)[s % 6]
        if kind == 4 and c >= 3:
            row[:3] = (I64_MAX, -5, I64_MIN)
        if s % 4 == 0 and c >= 3:
            row[2] = row[0]                                                   # a repeated id, relevant in kinds 5, 2 and 1
        strangers = rng.integers(10 ** 6, 2 * 10 ** 6, 5)
        if kind == 5:
            rel = list(row[:c:2]) + list(strangers[:2])
        elif kind == 2:
            rel = list(row[:max(c, 1)][:3]) * 3 + [int(strangers[0])] * 2
        elif kind == 4:
            rel = [I64_MIN, I64_MAX, -5, -4242]
        elif kind == 1:
            rel = [int(row[0])]
        elif kind == 3:
            rel = list(strangers) + [-1]
        else:
            rel = []
        rel = [int(x) for x in rng.permutation(np.array(rel, np.int64))] if rel else []
        pad = -1 if s % 2 == 0 or not rel else rel[0]
        row[c:] = pad
        rec[s], counts[s] = row, c
        lists.append(rel)
    offsets = np.zeros(n_segments + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=offsets[1:])
    rel_ids = np.array([x for l in lists for x in l], np.int64)
    return rec, counts, offsets, rel_ids


def corner_case():
    """Hand-made: id 50 is relevant in segments 0 and 1 but recommended only in 1; segment 2 repeats the relevant 7
    (a hit at its first position only) and its list repeats it too; segment 3's list holds -1 and its row is all
    padding behind one id; segment 4 has the extreme ids; segment 5 has no list.  rel_offsets starts above 0."""
    rec = np.array([[1, 2, 3, 4], [50, 2, 3, 4], [7, 9, 7, 8], [6, -1, -1, -1], [I64_MAX, I64_MIN, -3, 0], [1, 2, 3, 4]], np.int64)
    counts = np.array([4, 4, 4, 1, 4, 4], np.int64)
    lists = [[50, 3], [50], [7, 7, 8, 7], [-1, 6], [I64_MIN, -3, I64_MAX, 12345], []]
    offsets = np.zeros(7, np.int64)
    np.cumsum([len(x) for x in lists], out=offsets[1:])
    offsets += 2                                              # two ids in front that belong to no segment
    rel_ids = np.array([50, 1] + [x for l in lists for x in l] + [2], np.int64)
    return rec, counts, offsets, rel_ids


def wide_case():
    """Two rows of 3000 ids against lists of 5000: hits up to the last position, far beyond any LDS-sized buffer."""
    rng = np.random.default_rng(77)
    rec = np.stack([rng.permutation(3000) + 10, rng.permutation(3000) + 10]).astype(np.int64)
    counts = np.array([3000, 2999], np.int64)
    lists = []
    for s in range(2):
        mine = np.concatenate([rec[s, 2040:3000:3], rec[s, :40:7], rng.integers(10 ** 6, 2 * 10 ** 6, 5000)])[:5000]
        lists.append(rng.permutation(mine))
    offsets = np.array([0, 5000, 10000], np.int64)
    return rec, counts, offsets, np.concatenate(lists).astype(np.int64)


# ---- the hold-out split ------------------------------------------------------------------------------------------------

def model_holdout(person, timestamp, place, region, cut, new_places_only):
    """-> (train rows, sorted distinct held-out (person, region, place) triples)."""
    n = len(person)
    train = [i for i in range(n) if timestamp[i] < cut]
    persons = {int(person[i]) for i in train}
    been = {(int(person[i]), int(place[i])) for i in train}
    held = {(int(person[i]), int(region[i]), int(place[i])) for i in range(n)
            if timestamp[i] >= cut and int(person[i]) in persons
            and not (new_places_only and (int(person[i]), int(place[i])) in been)}
    return train, sorted(held)


def holdout_case(seed, n, cut=1000, before=True, after=True):
    """n visits of 40 persons (negative ids among them) at 30 places of 3 regions, timestamps around `cut` - many equal
    to it - so that persons appear only behind the cut, (person, place) pairs on both sides and triples many times."""
    rng = np.random.default_rng(seed)
    person = rng.integers(-20, 20, n).astype(np.int64) * 1_000_003
    place = rng.integers(-5, 25, n).astype(np.int64)
    region = place % 3 - 1                                    # a place lies in one region (-1, 0 or 1)
    lo, hi = (cut - 50 if before else cut), (cut + 50 if after else cut)
    ts = rng.integers(lo, max(hi, lo + 1), n).astype(np.int64)
    ts[rng.random(n) < 0.1] = cut if after else cut - 1
    late = person == person.min()                             # one person is seen only behind the cut
    if after:
        ts[late] = np.maximum(ts[late], cut)
    return {"person_id": person, "timestamp": ts, "place_id": place, "region_id": region.astype(np.int64),
            "category_id": (place % 7).astype(np.int64)}
