"""GPU: the ranked KNN batches (locrec_knn_recommend_ranked_batch, locrec_knn_fetch_ranked) and
SgGraph.recommend_ranked_batch against the unchanged row calls followed by oracle.rank_recommendations per person.
Equality of ids, score bits and counts: the ranked forms move rows, they compute nothing."""
import json
import os

import numpy as np
import pytest

import rank_batch_cases as rb

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PW, CW = 0.4, 0.6
LIMITS = (10, 257)            # the LDS lists; beyond LOCREC_RANK_BATCH_MAX_N
AGG_CAP = 4096                # kAggCap of csrc/knn.hip: rating rows one aggregation block sorts


def with_ratings(d, seed=3):
    rng = np.random.default_rng(seed)
    d = dict(d)
    d["r_rowptr"], d["r_place"] = d["p_rowptr"].copy(), d["p_idx"].astype(np.int64)
    d["r_rating"] = rng.integers(1, 6, size=len(d["p_idx"])).astype(np.int64)
    return d


def without_place_vector(d, row):
    """The person at `row` keeps its ratings' rows out: an empty place vector (no valid query)."""
    d = dict(d)
    a, b = d["p_rowptr"][row], d["p_rowptr"][row + 1]
    d["p_idx"], d["p_val"] = np.delete(d["p_idx"], np.s_[a:b]), np.delete(d["p_val"], np.s_[a:b])
    ptr = d["p_rowptr"].copy()
    ptr[row + 1:] -= b - a
    d["p_rowptr"] = ptr
    return d


def make_index(pkg, d):
    return pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"],
                        d["c_rowptr"], d["c_idx"], d["c_val"], d["c_dim"], d["r_rowptr"], d["r_place"], d["r_rating"])


def places_of(d):
    ids = np.arange(-5, d["p_dim"] + 5, dtype=np.int64)      # every place of the index and a few that nobody rated
    return ids, ids % 3


def csr_case(off, ids, scores, places, regions, targets):
    return dict(offsets=off, ids=ids, scores=scores, place_ids=places, regions=regions, targets=targets)


def expect(oracle, off, ids, scores, places, regions, targets, limit):
    ei, es, ec = rb.expected(oracle.rank_recommendations, csr_case(off, ids, scores, places, regions, targets), limit)
    width = max(0, min(limit, len(places)))                  # the KNN forms' width does not depend on the rows
    oi, osc = np.full((len(targets), width), -1, np.int64), np.zeros((len(targets), width))
    oi[:, :ei.shape[1]], osc[:, :es.shape[1]] = ei, es
    return oi, osc, ec


@pytest.fixture(scope="module")
def small(pkg):
    from locations_recommender_amd import synth
    d = with_ratings(without_place_vector(synth.small_knn_dataset(n=3000, p_dim=600, seed=11), 1203))
    ix = make_index(pkg, d)
    yield d, ix
    ix.close()


@pytest.mark.parametrize("k", [5, 50, 1500, 2_000_000])
def test_ranked_batch_and_range(pkg, oracle, small, k):
    d, ix = small
    places, regions = places_of(d)
    rng = np.random.default_rng(k)
    valid = np.flatnonzero(np.diff(d["p_rowptr"]) > 0)
    rows = np.r_[rng.choice(valid, 40, replace=False), [valid[-1], valid[5], valid[5]]]       # unsorted, with a repeat
    persons = d["person_ids"][rows]
    targets = rng.choice([0, 1, 2, 99], len(rows)).astype(np.int64)
    targets[-1], targets[-2] = 0, 1                                                           # the repeat, two targets
    off, rp, re = ix.recommend_batch(persons, PW, CW, k)
    assert off[-1] > 0
    for limit in LIMITS:
        got = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, limit)
        st = pkg.prep.rank_recommendations_batch_stats()
        assert rb.same(got, expect(oracle, off, rp, re, places, regions, targets, limit)), limit
        assert st["host_assembled"] == 0 and (st["sorted"] > 0) == (limit > 256)
    same_target = np.full(len(rows), 2, np.int64)
    got = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, same_target, 10)
    assert np.array_equal(got[0][-1], got[0][-2]) and np.array_equal(got[1][-1].view(np.uint64), got[1][-2].view(np.uint64))
    # the range form, over the person with the empty place vector
    at = int(np.flatnonzero(ix.row_person_ids(0, len(d["person_ids"])) == d["person_ids"][1203])[0])   # its internal row
    nq = 48
    first = min(max(0, at - 20), len(d["person_ids"]) - nq)
    ix.recommend_range_async(first, nq, PW, CW, k)
    roff, rrp, rre = ix.fetch_recommend(nq)
    empty = np.flatnonzero(ix.row_person_ids(first, nq) == d["person_ids"][1203])
    assert len(empty) == 1 and roff[empty[0]] == roff[empty[0] + 1]
    rt = rng.choice([0, 1, 2], nq).astype(np.int64)
    for limit in LIMITS:
        ix.recommend_range_async(first, nq, PW, CW, k)
        got = ix.fetch_ranked(nq, places, regions, rt, limit)
        st = pkg.prep.rank_recommendations_batch_stats()
        assert rb.same(got, expect(oracle, roff, rrp, rre, places, regions, rt, limit)), limit
        assert got[2][empty[0]] == 0 and st["host_assembled"] == 0


def test_aggregation_overflow_is_host_assembled(pkg, oracle):
    """K = 1000 neighbours with about 110 rating rows each are far more than the AGG_CAP rows one aggregation block
    sorts (enqueue_aggregate: M = pow2ceil(min(K * max_r_nnz, kAggCap))), so the queries overflow and their rows are
    assembled on the host; the ranked result is the same."""
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
        got = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, limit)
        st = pkg.prep.rank_recommendations_batch_stats()
        assert rb.same(got, expect(oracle, off, rp, re, places, regions, targets, limit)), limit
        assert st["host_assembled"] > 0
    ix.close()


def test_errors(pkg):
    from locations_recommender_amd import synth
    d = with_ratings(synth.small_knn_dataset(n=300, p_dim=200, seed=12))
    ix = make_index(pkg, d)                                # a fresh index: nothing is resident
    places, regions = places_of(d)
    ok = d["person_ids"][:2]
    with pytest.raises(pkg.IllegalArgumentException, match="no matching batched recommendation"):
        ix.fetch_ranked(2, places, regions, [0, 1], 10)
    with pytest.raises(pkg.IllegalArgumentException, match="No such person"):
        ix.recommend_ranked_batch([10 ** 9], PW, CW, 50, places, regions, [0], 10)
    for pw, cw, k in [(0.0, 1.0, 3), (1.0, 0.0, 3), (0.5, 0.4, 3), (0.5, 0.5, 0), (0.5, 0.5, -1)]:
        with pytest.raises(pkg.IllegalArgumentException):
            ix.recommend_ranked_batch(ok, pw, cw, k, places, regions, [0, 1], 10)
    # a batch of two was resident, then a call of two failed its requires: the same nq, but nothing resident any more
    assert ix.recommend_ranked_batch(ok, PW, CW, 50, places, regions, [0, 1], 10)[2].shape == (2,)
    assert ix.fetch_ranked(2, places, regions, [0, 1], 10)[2].shape == (2,)
    with pytest.raises(pkg.IllegalArgumentException):
        ix.recommend_ranked_batch(ok, 0.5, 0.4, 3, places, regions, [0, 1], 10)
    with pytest.raises(pkg.IllegalArgumentException, match="no matching batched recommendation"):
        ix.fetch_ranked(2, places, regions, [0, 1], 10)
    ix.recommend_range_async(0, 8, PW, CW, 50)
    with pytest.raises(pkg.IllegalArgumentException):      # another nq than the resident range's
        ix.fetch_ranked(9, places, regions, [0] * 9, 10)
    ix.close()


def test_sg_ranked_batch(pkg, oracle):
    with open(os.path.join(GOLD, "sg_kats.json")) as f:
        g = json.load(f)
    e = np.array(g["edges"], dtype=np.float64)
    sg = pkg.SgGraph(e[:, 0].astype(np.int64), e[:, 1].astype(np.int64), e[:, 2])
    cases = [c for c in g["cases"] if "expected_error" not in c]
    vertices = np.array([c["vertex_id"] for c in cases] + [cases[0]["vertex_id"]], np.int64)
    places = np.unique(e[:, :2].astype(np.int64))
    regions = places % 2
    targets = (np.arange(len(vertices)) % 3).astype(np.int64)      # 2: no such region
    c0 = cases[0]
    off, ids, probs, its, conv = sg.recommend_batch(vertices, g["alpha"], c0["epsilon"], c0["max_iterations"])
    assert off[-1] > 0
    for limit in (1, 2, 10):
        oi, op, cnt, its2, conv2 = sg.recommend_ranked_batch(vertices, g["alpha"], c0["epsilon"], c0["max_iterations"], places,
                                                             regions, targets, limit)
        want = rb.expected(oracle.rank_recommendations, csr_case(off, ids, probs, places, regions, targets), limit)
        assert rb.same((oi, op, cnt), want) and np.array_equal(its, its2) and np.array_equal(conv, conv2)
    sg.close()
