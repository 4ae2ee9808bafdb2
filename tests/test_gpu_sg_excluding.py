"""GPU: the ranked SG batch with caller-given exclusion lists (locrec_sg_recommend_ranked_batch_excluding,
SgGraph.recommend_ranked_batch(excluded=...)) in the world of test_gpu_sg_ranked.  Expected: recommend_batch's host rows
(locrec_sg_recommend's rows), without the listed ids, ranked per request by oracle.rank_recommendations.  Every
comparison is exact - ids, counts, probability bits."""
import numpy as np
import pytest

import rank_batch_cases as rb
import rank_exclude_cases as rx
from test_gpu_sg_ranked import ALPHA, NOBODYS_REGION, PERSON0, PLACE0, handmade, main_requests, pkg_stats, places_table

pytestmark = pytest.mark.gpu
LIMITS = (1, 10, 256, 257, 2 ** 40)


@pytest.fixture(scope="module")
def world(pkg):
    from locations_recommender_amd import stochastic, synth
    g = synth.sg_dataset(n_persons=1_200, n_places=300, n_categories=20, seed=8)
    sg = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"])
    place_ids, regions = places_table()
    v, t, own = main_requests(place_ids, regions)
    yield dict(g=g, sg=sg, place_ids=place_ids, regions=regions, v=v, t=t, own=own,
               lists=stochastic.out_neighbours(g["source_id"], g["target_id"], v))
    sg.close()


def expected(oracle, sg, v, eps, max_it, place_ids, regions, targets, lists, limit):
    """-> ((ids, probabilities, counts) with W = the limit cut to the longest row count, iterations, converged)"""
    off, ids, probs, its, conv = sg.recommend_batch(v, ALPHA, eps, max_it)
    case = dict(offsets=off, ids=ids, scores=probs, place_ids=place_ids, regions=regions, targets=targets, ex_offsets=lists[0],
                ex_ids=lists[1])
    return rx.expected(oracle.rank_recommendations, case, limit), its, conv


def same_all(got, want):
    ranked, its, conv = want
    return rb.same(got[:3], ranked) and np.array_equal(got[3], its) and np.array_equal(got[4], conv)


@pytest.mark.parametrize("eps,max_it", ((0.01, 20), (0.0, 3), (0.01, 0)))
def test_lists_from_out_neighbours(oracle, world, eps, max_it):
    w = world
    sg, v, t, lists = w["sg"], w["v"], w["t"], w["lists"]
    assert np.diff(lists[0]).max() > 0
    for limit in LIMITS:
        want = expected(oracle, sg, v, eps, max_it, w["place_ids"], w["regions"], t, lists, limit)
        got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, w["place_ids"], w["regions"], t, limit, excluded=lists)
        assert same_all(got, want), (eps, max_it, limit)
        host = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, w["place_ids"], w["regions"], t, limit, on_device=False,
                                         excluded=lists)
        assert rb.same(got[:3], tuple(np.asarray(x) for x in host[:3])) and np.array_equal(got[3], host[3])
        for i in range(len(v)):
            assert not np.isin(got[0][i, :got[2][i]], rx.list_of(dict(ex_offsets=lists[0], ex_ids=lists[1]), i)).any()
    # the lists bite: a person's walk lands on its own places first
    plain = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, w["place_ids"], w["regions"], t, 10)
    got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, w["place_ids"], w["regions"], t, 10, excluded=lists)
    persons = np.flatnonzero((v >= PERSON0) & (t != NOBODYS_REGION))
    changed = sum(1 for i in persons if not np.array_equal(plain[0][i], got[0][i]))
    if max_it > 0:
        assert changed >= len(persons) // 2, changed


def test_empty_lists_are_the_plain_call(world):
    from locations_recommender_amd import _lib as L
    import ctypes as C
    w = world
    sg, v, t, pl, reg = w["sg"], w["v"], w["t"], w["place_ids"], w["regions"]
    none = (np.zeros(len(v) + 1, np.int64), np.empty(0, np.int64))
    for max_it in (20, 0):
        plain = sg.recommend_ranked_batch(v, ALPHA, 0.01, max_it, pl, reg, t, 10)
        pst = pkg_stats(sg)
        got = sg.recommend_ranked_batch(v, ALPHA, 0.01, max_it, pl, reg, t, 10, excluded=none)
        st = pkg_stats(sg)
        assert rb.same(got[:3], plain[:3]) and np.array_equal(got[3], plain[3]) and np.array_equal(got[4], plain[4])
        assert [st[k] for k in ("tiles", "groups", "emitted_rows", "host_syncs")] == \
            [pst[k] for k in ("tiles", "groups", "emitted_rows", "host_syncs")]
        # out_row_counts through the C entry
        n, stride = len(v), 7
        off = sg.recommend_batch(v, ALPHA, 0.01, max_it)[0]
        oi, op = np.full((n, stride), -5, np.int64), np.full((n, stride), -5.0)
        cnt, rows = np.full(n, -5, np.int64), np.full(n, -5, np.int64)
        L.check(L.lib().locrec_sg_recommend_ranked_batch_excluding(
            sg._h, n, L.ptr(v, C.c_int64), ALPHA, 0.01, max_it, len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64),
            L.ptr(t, C.c_int64), stride, L.ptr(none[0], C.c_int64), 0, None, L.ptr(oi, C.c_int64), L.ptr(op, C.c_double),
            L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64), None, None))
        assert np.array_equal(rows, np.diff(off)) and rows.min() > 0 and cnt.max() == stride


def test_row_counts_do_not_see_the_lists(world):
    """out_row_counts is makeRecommendations' own row count, with lists too."""
    from locations_recommender_amd import _lib as L
    import ctypes as C
    w = world
    sg, v, t, pl, reg, lists = w["sg"], w["v"], w["t"], w["place_ids"], w["regions"], w["lists"]
    n, stride = len(v), 7
    off = sg.recommend_batch(v, ALPHA, 0.01, 20)[0]
    oi, op = np.full((n, stride), -5, np.int64), np.full((n, stride), -5.0)
    cnt, rows = np.full(n, -5, np.int64), np.full(n, -5, np.int64)
    L.check(L.lib().locrec_sg_recommend_ranked_batch_excluding(
        sg._h, n, L.ptr(v, C.c_int64), ALPHA, 0.01, 20, len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64),
        L.ptr(t, C.c_int64), stride, L.ptr(lists[0], C.c_int64), len(lists[1]), L.ptr(lists[1], C.c_int64), L.ptr(oi, C.c_int64),
        L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64), None, None))
    assert np.array_equal(rows, np.diff(off))


def test_a_repeated_vertex_with_two_lists_and_more_requests_than_a_tile_has_columns(oracle, world):
    """40 requests of one person (and 3 of a place): one column, 43 segments, a list of its own for every position."""
    w = world
    sg = w["sg"]
    v = np.r_[np.full(40, PERSON0 + 77), np.full(3, PLACE0 + 9)].astype(np.int64)
    t = np.r_[np.arange(40) % 4, [0, 1, 2]].astype(np.int64)
    t[t == 3] = NOBODYS_REGION
    visited = w["g"]["target_id"][w["g"]["source_id"] == PERSON0 + 77].astype(np.int64)
    assert len(visited) > 4
    lists = [visited[:i % 5] if i % 2 else visited[::-1][:i % 7] for i in range(40)] + [np.array([PLACE0 + 10], np.int64)] * 3
    lists[0], lists[4] = visited, np.empty(0, np.int64)               # the same vertex and region: everything, nothing
    x = rx.with_lists({}, lists)
    x = (x["ex_offsets"], x["ex_ids"])
    for max_it in (20, 0):
        want = expected(oracle, sg, v, 0.01, max_it, w["place_ids"], w["regions"], t, x, 10)
        got = sg.recommend_ranked_batch(v, ALPHA, 0.01, max_it, w["place_ids"], w["regions"], t, 10, excluded=x)
        assert same_all(got, want) and pkg_stats(sg)["tiles"] == 1
        assert not np.array_equal(got[0][0], got[0][4]) and not np.isin(got[0][0], visited).any()


@pytest.mark.parametrize("budget", [1, 97])
def test_row_budget_does_not_change_the_result(world, monkeypatch, budget):
    w = world
    sg, lists = w["sg"], w["lists"]
    for limit in (10, 300):
        base = sg.recommend_ranked_batch(w["v"], ALPHA, 0.01, 20, w["place_ids"], w["regions"], w["t"], limit, excluded=lists)
        assert pkg_stats(sg)["groups"] == 1 and base[2].max() > 0
        monkeypatch.setenv("LOCREC_SG_RANKED_ROW_BUDGET", str(budget))
        got = sg.recommend_ranked_batch(w["v"], ALPHA, 0.01, 20, w["place_ids"], w["regions"], w["t"], limit, excluded=lists)
        st = pkg_stats(sg)
        monkeypatch.delenv("LOCREC_SG_RANKED_ROW_BUDGET")
        assert rb.same(got[:3], base[:3]) and np.array_equal(got[3], base[3]) and np.array_equal(got[4], base[4])
        assert st["groups"] > 1 and st["tiles"] == 3
        if budget == 1:     # a group per request
            assert st["groups"] == len(w["v"])


def test_handmade_tie_group_with_one_member_excluded(pkg, oracle):
    src, dst, wgt, place_ids, regions = handmade()
    sg = pkg.SgGraph(src, dst, wgt)
    v, t = np.array([100, 50, 9], np.int64), np.full(3, 5, np.int64)
    x = (np.array([0, 1, 3, 3], np.int64), np.array([3, 1, 8], np.int64))     # 100 without 3; 50 without 1 and 8; 9 as it is
    for limit in (3, 8):
        want = expected(oracle, sg, v, 0.0, 5, place_ids, regions, t, x, limit)
        got = sg.recommend_ranked_batch(v, ALPHA, 0.0, 5, place_ids, regions, t, limit, excluded=x)
        assert same_all(got, want)
        kept = ([1, 2, 4, 5, 6, 7, 8], [2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8])
        for i in range(3):   # one tie group: id ascending, the excluded member missing
            assert got[0][i, :got[2][i]].tolist() == kept[i][:limit]
            assert len(set(got[1][i, :got[2][i]].tolist())) == 1
    sg.close()


def test_errors(pkg, world):
    w = world
    sg, pl, reg = w["sg"], w["place_ids"], w["regions"]
    v, t = w["v"][:4], np.zeros(4, np.int64)
    ids = np.arange(6, dtype=np.int64)
    for bad in ([0, 4, 2, 5, 6], [-1, 1, 2, 3, 6], [0, 1, 2, 3, 7]):
        with pytest.raises(pkg.IllegalArgumentException, match="excluded_offsets"):
            sg.recommend_ranked_batch(v, ALPHA, 0.01, 20, pl, reg, t, 10, excluded=(np.array(bad, np.int64), ids))
    with pytest.raises(pkg.IllegalArgumentException):            # one list too few
        sg.recommend_ranked_batch(v, ALPHA, 0.01, 20, pl, reg, t, 10, excluded=(np.array([0, 1, 2, 3], np.int64), ids))
    with pytest.raises(pkg.IllegalArgumentException, match="No such vertex in the graph"):
        sg.recommend_ranked_batch(np.r_[v[:3], 10 ** 9], ALPHA, 0.01, 20, pl, reg, t, 10, excluded=(np.zeros(5, np.int64), ids[:0]))
    # the handle serves the plain call as before
    a = sg.recommend_ranked_batch(w["v"], ALPHA, 0.01, 20, pl, reg, w["t"], 10)
    sg.recommend_ranked_batch(w["v"], ALPHA, 0.01, 20, pl, reg, w["t"], 10, excluded=w["lists"])
    b = sg.recommend_ranked_batch(w["v"], ALPHA, 0.01, 20, pl, reg, w["t"], 10)
    assert rb.same(a[:3], b[:3])
