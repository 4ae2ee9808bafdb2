"""GPU: the unvisited forms of the ranked KNN batches (locrec_knn_recommend_ranked_batch_unvisited,
locrec_knn_fetch_ranked_unvisited): only new places.  Expected: the unchanged row calls' rows, without the places the
person has a rating row for, ranked per person by oracle.rank_recommendations.  Equality of ids, score bits and counts."""
import numpy as np
import pytest

import rank_batch_cases as rb
import rank_exclude_cases as rx
from test_gpu_knn_ranked import AGG_CAP, CW, LIMITS, PW, make_index, places_of, with_ratings, without_place_vector

pytestmark = pytest.mark.gpu
# The share of 120 requests (40 persons x 3 regions, limit 10) whose ranking must differ from the plain call's; None: at
# least one.  On the CPU the oracle finds 84 / 48 / 3 / 11 such requests for the persons this test draws at K = 5 / 50 /
# 1500 / 2,000,000 (82 / 63 / 13 for another draw of 40 persons from the same fixture).
MIN_CHANGED = {5: 0.25, 50: 0.25, 1500: 0.0, 2_000_000: None}


def rated_places(d, person):
    row = int(np.flatnonzero(d["person_ids"] == person)[0])
    return d["r_place"][d["r_rowptr"][row]:d["r_rowptr"][row + 1]]


def expect(oracle, d, persons, off, ids, scores, places, regions, targets, limit):
    lists = [rated_places(d, int(p)) for p in persons]
    case = rx.with_lists(dict(offsets=off, ids=ids, scores=scores, place_ids=places, regions=regions, targets=targets), lists)
    width = max(0, min(limit, len(places)))                  # the KNN forms' width does not depend on the rows
    return rx.widened(rb.expected(oracle.rank_recommendations, rx.filtered(case), limit), width), lists


def no_rated_place(got, lists):
    return all(not np.isin(got[0][i, :got[2][i]], lists[i]).any() for i in range(len(lists)))


def changed_rows(a, b):
    return sum(1 for i in range(len(a[2])) if a[2][i] != b[2][i] or not np.array_equal(a[0][i], b[0][i]))


@pytest.fixture(scope="module")
def small(pkg):
    from locations_recommender_amd import synth
    d = with_ratings(without_place_vector(synth.small_knn_dataset(n=3000, p_dim=600, seed=11), 1203))
    ix = make_index(pkg, d)
    yield d, ix
    ix.close()


@pytest.mark.parametrize("k", [5, 50, 1500, 2_000_000])
def test_unvisited_batch_and_range(pkg, oracle, small, k):
    d, ix = small
    places, regions = places_of(d)
    rng = np.random.default_rng(k)
    valid = np.flatnonzero(np.diff(d["p_rowptr"]) > 0)
    rows = np.r_[rng.choice(valid, 40, replace=False), [valid[-1], valid[5], valid[5]]]       # unsorted, with a repeat
    persons = d["person_ids"][rows]
    targets = rng.choice([0, 1, 2, 99], len(rows)).astype(np.int64)
    targets[-1], targets[-2] = 0, 1                                                           # the repeat, two targets
    off, rp, re = ix.recommend_batch(persons, PW, CW, k)
    for limit in LIMITS:
        plain = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, limit)
        got = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, limit, unvisited=True)
        st = pkg.prep.rank_recommendations_batch_stats()
        want, lists = expect(oracle, d, persons, off, rp, re, places, regions, targets, limit)
        assert rb.same(got, want), limit
        assert no_rated_place(got, lists) and got[2].sum() > 0
        assert st["host_assembled"] == 0 and (st["sorted"] > 0) == (limit > 256) and st["host_syncs"] <= 3
        # the plain call on the same handle returns what it did before
        assert rb.same(ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, limit), plain)
    same_target = np.full(len(rows), 2, np.int64)
    got = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, same_target, 10, unvisited=True)
    assert np.array_equal(got[0][-1], got[0][-2]) and np.array_equal(got[1][-1].view(np.uint64), got[1][-2].view(np.uint64))
    # how often the exclusion bites: 40 persons x 3 regions at limit 10
    p40, t3 = np.repeat(persons[:40], 3), np.tile(np.arange(3, dtype=np.int64), 40)
    plain = ix.recommend_ranked_batch(p40, PW, CW, k, places, regions, t3, 10)
    got = ix.recommend_ranked_batch(p40, PW, CW, k, places, regions, t3, 10, unvisited=True)
    changed = changed_rows(plain, got)
    print(f"K = {k}: {changed} of 120 requests differ from the plain ranked call")
    if MIN_CHANGED[k] is None:
        assert changed >= 1
    else:
        assert changed >= MIN_CHANGED[k] * 120
    assert got[2].min() > 0                                  # every request still has rows
    # the range form, over the person with the empty place vector
    at = int(np.flatnonzero(ix.row_person_ids(0, len(d["person_ids"])) == d["person_ids"][1203])[0])   # its internal row
    nq = 48
    first = min(max(0, at - 20), len(d["person_ids"]) - nq)
    ix.recommend_range_async(first, nq, PW, CW, k)
    roff, rrp, rre = ix.fetch_recommend(nq)
    range_persons = ix.row_person_ids(first, nq)
    empty = np.flatnonzero(range_persons == d["person_ids"][1203])
    rt = rng.choice([0, 1, 2], nq).astype(np.int64)
    for limit in LIMITS:
        ix.recommend_range_async(first, nq, PW, CW, k)
        got = ix.fetch_ranked(nq, places, regions, rt, limit, unvisited=True)
        st = pkg.prep.rank_recommendations_batch_stats()
        want, lists = expect(oracle, d, range_persons, roff, rrp, rre, places, regions, rt, limit)
        assert rb.same(got, want), limit
        assert no_rated_place(got, lists) and got[2][empty[0]] == 0 and st["host_assembled"] == 0
        plain = ix.fetch_ranked(nq, places, regions, rt, limit)
        assert rb.same(plain, rx.widened(rb.expected(oracle.rank_recommendations, dict(
            offsets=roff, ids=rrp, scores=rre, place_ids=places, regions=regions, targets=rt), limit), got[0].shape[1]))


def test_aggregation_overflow_is_host_assembled(pkg, oracle):
    """The overflow case of test_gpu_knn_ranked: the host-assembled segments of the second ranker call get their persons'
    lists as well."""
    from locations_recommender_amd import synth
    d = with_ratings(synth.knn_dataset(3_000, 400, seed=42, mean_places=110, max_places=160))
    rows = np.array([0, 1500, 2999, 77, 1500])
    persons = d["person_ids"][rows]
    k = 1000
    nnz = np.diff(d["r_rowptr"])
    pos = {int(p): i for i, p in enumerate(d["person_ids"])}
    neighbours, _ = oracle.knn_similar(d, int(persons[0]), PW, CW, k)
    assert sum(int(nnz[pos[int(p)]]) for p in neighbours) > AGG_CAP          # sized on the CPU: this query overflows
    ix = make_index(pkg, d)
    places, regions = places_of(d)
    targets = np.array([0, 1, 2, 0, 2], np.int64)
    off, rp, re = ix.recommend_batch(persons, PW, CW, k)
    for limit in LIMITS:
        got = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, limit, unvisited=True)
        st = pkg.prep.rank_recommendations_batch_stats()
        want, lists = expect(oracle, d, persons, off, rp, re, places, regions, targets, limit)
        assert rb.same(got, want), limit
        assert st["host_assembled"] > 0 and no_rated_place(got, lists) and got[2].min() > 0
    ix.close()


def test_index_without_ratings_uses_the_place_vectors(pkg, oracle):
    from locations_recommender_amd import synth
    d = synth.small_knn_dataset(n=400, p_dim=300, seed=5)
    ix = pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"],
                      d["c_rowptr"], d["c_idx"], d["c_val"], d["c_dim"])
    d = dict(d, r_rowptr=d["p_rowptr"], r_place=d["p_idx"].astype(np.int64))
    places, regions = places_of(d)
    persons = d["person_ids"][[7, 399, 0, 7]]
    targets = np.array([0, 1, 2, 1], np.int64)
    for k in (20, 2_000_000):
        off, rp, re = ix.recommend_batch(persons, PW, CW, k)
        got = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, 10, unvisited=True)
        want, lists = expect(oracle, d, persons, off, rp, re, places, regions, targets, 10)
        assert rb.same(got, want) and no_rated_place(got, lists) and got[2].sum() > 0 and all(len(x) for x in lists)
    ix.close()


def test_ratings_not_ascending_by_place(pkg, oracle):
    """The rating rows of every person in descending place order, then shuffled: the lists are read as they lie."""
    from locations_recommender_amd import synth
    d = with_ratings(synth.small_knn_dataset(n=400, p_dim=300, seed=6))
    rng = np.random.default_rng(1)
    place, rating = d["r_place"].copy(), d["r_rating"].copy()
    for r in range(len(d["person_ids"])):
        a, b = d["r_rowptr"][r], d["r_rowptr"][r + 1]
        order = rng.permutation(b - a) if r % 2 else np.arange(b - a)[::-1]
        place[a:b], rating[a:b] = place[a:b][order], rating[a:b][order]
    d = dict(d, r_place=place, r_rating=rating)
    assert any(np.any(np.diff(place[d["r_rowptr"][r]:d["r_rowptr"][r + 1]]) < 0) for r in range(10))
    ix = make_index(pkg, d)
    places, regions = places_of(d)
    persons = d["person_ids"][[3, 4, 250, 399]]
    targets = np.array([0, 1, 2, 0], np.int64)
    off, rp, re = ix.recommend_batch(persons, PW, CW, 30)
    for limit in LIMITS:
        got = ix.recommend_ranked_batch(persons, PW, CW, 30, places, regions, targets, limit, unvisited=True)
        want, lists = expect(oracle, d, persons, off, rp, re, places, regions, targets, limit)
        assert rb.same(got, want) and no_rated_place(got, lists) and got[2].sum() > 0
    ix.close()


def test_errors_are_the_plain_calls(pkg):
    from locations_recommender_amd import synth
    d = with_ratings(synth.small_knn_dataset(n=300, p_dim=200, seed=12))
    ix = make_index(pkg, d)                                # a fresh index: nothing is resident
    places, regions = places_of(d)
    ok = d["person_ids"][:2]
    with pytest.raises(pkg.IllegalArgumentException, match="no matching batched recommendation"):
        ix.fetch_ranked(2, places, regions, [0, 1], 10, unvisited=True)
    with pytest.raises(pkg.IllegalArgumentException, match="No such person"):
        ix.recommend_ranked_batch([10 ** 9], PW, CW, 50, places, regions, [0], 10, unvisited=True)
    for pw, cw, k in [(0.0, 1.0, 3), (1.0, 0.0, 3), (0.5, 0.4, 3), (0.5, 0.5, 0), (0.5, 0.5, -1)]:
        with pytest.raises(pkg.IllegalArgumentException):
            ix.recommend_ranked_batch(ok, pw, cw, k, places, regions, [0, 1], 10, unvisited=True)
    assert ix.recommend_ranked_batch(ok, PW, CW, 50, places, regions, [0, 1], 10, unvisited=True)[2].shape == (2,)
    assert ix.fetch_ranked(2, places, regions, [0, 1], 10, unvisited=True)[2].shape == (2,)
    ix.recommend_range_async(0, 8, PW, CW, 50)
    with pytest.raises(pkg.IllegalArgumentException):      # another nq than the resident range's
        ix.fetch_ranked(9, places, regions, [0] * 9, 10, unvisited=True)
    ix.close()
