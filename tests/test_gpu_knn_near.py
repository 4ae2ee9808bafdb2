"""GPU: KnnIndex.recommend_ranked_batch_near (locrec_knn_recommend_ranked_batch_near) against the unchanged row call
followed by the composition of rank_near_cases: prep.distance_meters(centre, place) <= radius cuts the place table,
oracle.rank_recommendations ranks each person's rows against the cut table (without the person's rated places where
unvisited), and the distances are those of the first kept listing.  Equality of ids, score bits, distance bits and
counts, for both resident row forms and for host-assembled overflow queries."""
import numpy as np
import pytest

import rank_batch_cases as rb
import rank_near_cases as rn
from test_gpu_knn_ranked import AGG_CAP, CW, LIMITS, PW, csr_case, make_index, places_of, with_ratings, without_place_vector

pytestmark = pytest.mark.gpu


def near_case(d, rows, off, rp, re, targets, seed, unvisited):
    """The batch's rows as a rank_near_cases case: coordinates for places_of(d) by that module's scheme, a circle per
    position, and - unvisited - the rated places of each position's person as its list."""
    places, regions = places_of(d)
    case = rn.with_circles(csr_case(off, rp, re, places, regions, targets), seed)
    if unvisited:
        lists = [d["r_place"][d["r_rowptr"][r]:d["r_rowptr"][r + 1]] for r in rows]
        xoff = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(x) for x in lists], out=xoff[1:])
        case.update(ex_offsets=xoff, ex_ids=np.concatenate(lists).astype(np.int64))
    return case


def expect(pkg, oracle, case, kept, limit):
    """rank_near_cases.expected in the KNN forms' width, which does not depend on the rows."""
    ei, es, em, ec = rn.expected(oracle.rank_recommendations, None, case, limit, kept)
    n, width = len(ec), max(0, min(limit, len(case["place_ids"])))
    oi, osc, om = np.full((n, width), -1, np.int64), np.zeros((n, width)), np.zeros((n, width))
    oi[:, :ei.shape[1]], osc[:, :es.shape[1]], om[:, :em.shape[1]] = ei, es, em
    return oi, osc, om, ec


def call(ix, persons, k, case, limit, unvisited):
    return ix.recommend_ranked_batch_near(persons, PW, CW, k, case["place_ids"], case["regions"], case["lat"], case["lon"],
                                          case["targets"], case["clat"], case["clon"], case["radius"], limit, unvisited=unvisited)


@pytest.fixture(scope="module")
def small(pkg):
    from locations_recommender_amd import synth
    d = with_ratings(without_place_vector(synth.small_knn_dataset(n=3000, p_dim=600, seed=11), 1203))
    ix = make_index(pkg, d)
    yield d, ix
    ix.close()


@pytest.mark.parametrize("unvisited", [False, True], ids=["all", "unvisited"])
@pytest.mark.parametrize("k", [5, 1500, 2_000_000])
def test_near_batch(pkg, oracle, small, k, unvisited):
    d, ix = small
    places, regions = places_of(d)
    rng = np.random.default_rng(k)
    valid = np.flatnonzero(np.diff(d["p_rowptr"]) > 0)
    rows = np.r_[rng.choice(valid, 40, replace=False), [valid[-1], valid[5], valid[5]]]       # unsorted, with a repeat
    persons = d["person_ids"][rows]
    targets = rng.choice([0, 1, 2, 99], len(rows)).astype(np.int64)
    targets[-1], targets[-2] = 0, 0                                # the repeat: one region, two circles
    off, rp, re = ix.recommend_batch(persons, PW, CW, k)
    assert off[-1] > 0
    case = near_case(d, rows, off, rp, re, targets, k % 7, unvisited)
    case["clat"][-1], case["clon"][-1], case["radius"][-1] = case["clat"][-2], case["clon"][-2], np.inf
    case["radius"][-2] = 400.0
    kept = rn.all_kept(pkg.prep.distance_meters, case)
    before = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, 10)
    filtered = 0
    for limit in LIMITS:
        got = call(ix, persons, k, case, limit, unvisited)
        st = pkg.prep.rank_recommendations_batch_stats()
        want = expect(pkg, oracle, case, kept, limit)
        assert rn.same(got, want), limit
        assert st["host_assembled"] == 0 and (st["sorted"] > 0) == (limit > 256)
        filtered += int((want[3] < before[2]).sum()) if limit == 10 else 0
    assert filtered > 0                                            # the circles (and lists) bite
    assert got[3][-2] < got[3][-1] or got[3][-1] == 0              # the repeated person, ranked per position
    # the plain call afterwards returns what it did before
    after = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, 10)
    assert rb.same(after, before)


@pytest.mark.parametrize("unvisited", [False, True], ids=["all", "unvisited"])
def test_aggregation_overflow_goes_through_the_near_ranker(pkg, oracle, unvisited):
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
    targets = np.array([0, 1, 2, 0, 2], np.int64)
    off, rp, re = ix.recommend_batch(persons, PW, CW, k)
    case = near_case(d, rows, off, rp, re, targets, 5, unvisited)
    case["radius"][:] = (1500.0, 400.0, np.inf, 60.0, 1500.0)
    kept = rn.all_kept(pkg.prep.distance_meters, case)
    for limit in LIMITS:
        got = call(ix, persons, k, case, limit, unvisited)
        st = pkg.prep.rank_recommendations_batch_stats()
        assert rn.same(got, expect(pkg, oracle, case, kept, limit)), limit
        assert st["host_assembled"] > 0
    assert got[3].sum() > 0 and got[3][1] < got[3][2]
    ix.close()


def test_refusals_leave_the_index_usable(pkg, small):
    d, ix = small
    places, regions = places_of(d)
    persons = d["person_ids"][:2]
    lat, lon = rn.coordinates(0, regions)
    ok = (persons, PW, CW, 5, places, regions, lat, lon, [0, 1], [48.86, 89.98], [2.31, -29.98])
    with pytest.raises(pkg.IllegalArgumentException, match="radius_meters"):
        ix.recommend_ranked_batch_near(*ok, [10.0, -1.0], 10)
    with pytest.raises(pkg.IllegalArgumentException, match="No such person"):
        ix.recommend_ranked_batch_near([10 ** 9, 5], *ok[1:], [10.0, 10.0], 10)
    oi, osc, om, cnt = ix.recommend_ranked_batch_near(*ok, [np.inf, 0.0], 10)
    assert cnt[1] == 0 and (om[oi == -1] == 0).all()
