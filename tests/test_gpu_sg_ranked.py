"""GPU: the ranked SG batch (locrec_sg_recommend_ranked_batch, SgGraph.recommend_ranked_batch(on_device=True)): the rows
of a batched makeRecommendations are emitted into per-request segments and ranked on the device.

The expected value everywhere is recommend_batch's host rows put through mains.rank_recommendations_batch (numpy).
Every comparison is exact - ids, counts, probability bits: nothing is computed after the iteration, only moved."""
import ctypes as C

import numpy as np
import pytest

import rank_batch_cases as rb

pytestmark = pytest.mark.gpu
ALPHA = 0.15
N_PERSONS, N_PLACES, N_CATEGORIES = 1_200, 300, 20
PLACE0, PERSON0 = 40, 40 + N_PLACES
NOBODYS_REGION = 99
LIMITS = (-1, 0, 1, 10, 256, 257, 2 ** 40)
PARAMS = ((0.01, 20), (0.0, 3), (0.5, 1))


def places_table(n_places=N_PLACES, seed=3):
    """rank_batch_cases.places' kind of table over the graph's places: regions 0..2, 20 rows listed twice in their region,
    15 ids listed in a second region as well, 20 ids no vertex has, and a category and a person listed as places."""
    rng = np.random.default_rng(seed)
    ids = np.arange(PLACE0, PLACE0 + n_places, dtype=np.int64)
    reg = rng.integers(0, 3, len(ids)).astype(np.int64)
    twice = rng.choice(len(ids), 20, replace=False)
    other = rng.choice(len(ids), 15, replace=False)
    ids2 = np.concatenate([ids, ids[twice], ids[other], np.arange(900_000, 900_020), [3, PLACE0 + n_places + 5]])
    reg2 = np.concatenate([reg, reg[twice], (reg[other] + 1) % 3, rng.integers(0, 3, 20), [1, 0]])
    order = rng.permutation(len(ids2))
    return ids2[order].astype(np.int64), reg2[order].astype(np.int64)


def main_requests(place_ids, regions):
    """35 requests over 33 distinct vertices (two full tiles and a part): persons (source-only), places and categories
    (live); one person three times with three regions; a place that is its own target inside its target region; a
    region nobody has."""
    persons = PERSON0 + np.array([3, 700, 11, 12, 13, 50, 51, 999, 1199, 0, 1, 2, 600, 601, 602, 603, 604, 605, 606, 607])
    places = PLACE0 + np.array([5, 6, 7, 100, 150, 299, 0, 42, 43, 44])
    cats = np.array([2, 7, 19])
    v = np.concatenate([persons, places, cats]).astype(np.int64)
    t = (np.arange(len(v)) % 3).astype(np.int64)
    own = PLACE0 + 5
    t[20] = regions[np.flatnonzero(place_ids == own)[0]]      # the place's own region: it must not recommend itself
    t[4] = NOBODYS_REGION
    v = np.concatenate([v[:9], [v[0]], v[9:30], [v[0]], v[30:]])   # v[0] three times ...
    t = np.concatenate([t[:9], [1], t[9:30], [2], t[30:]])         # ... with regions 0, 1, 2
    assert len(v) == 35 and len(np.unique(v)) == 33
    return v, t, own


def expected(mains, sg, v, eps, max_it, place_ids, regions, targets, limit):
    off, ids, probs, its, conv = sg.recommend_batch(v, ALPHA, eps, max_it)
    return mains.rank_recommendations_batch(off, ids, probs, place_ids, regions, targets, limit), its, conv, np.diff(off)


def same_all(got, want):
    (wi, ws, wc), wits, wconv, _ = want
    return (rb.same(got[:3], (wi, ws, wc)) and np.array_equal(got[3], wits) and np.array_equal(got[4], wconv)
            and got[4].dtype == np.bool_)


@pytest.fixture(scope="module")
def world(pkg):
    from locations_recommender_amd import mains, synth
    g = synth.sg_dataset(n_persons=N_PERSONS, n_places=N_PLACES, n_categories=N_CATEGORIES, seed=8)
    sg = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"])
    place_ids, regions = places_table()
    v, t, own = main_requests(place_ids, regions)
    yield dict(g=g, sg=sg, mains=mains, place_ids=place_ids, regions=regions, v=v, t=t, own=own)
    sg.close()


@pytest.mark.parametrize("eps,max_it", PARAMS)
def test_main_case(world, eps, max_it):
    w = world
    sg, v, t = w["sg"], w["v"], w["t"]
    off, ids, probs, its, conv = sg.recommend_batch(v, ALPHA, eps, max_it)
    for limit in LIMITS:
        want = w["mains"].rank_recommendations_batch(off, ids, probs, w["place_ids"], w["regions"], t, limit)
        got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, w["place_ids"], w["regions"], t, limit)
        assert rb.same(got[:3], want), (eps, max_it, limit)
        assert np.array_equal(got[3], its) and np.array_equal(got[4], conv)
        cnt = got[2]
        if limit > 0:
            assert cnt[t != NOBODYS_REGION].min() > 0 and cnt[t == NOBODYS_REGION].tolist() == [0]
            assert got[0].shape[1] == min(limit, int(np.diff(off).max()))
            if limit >= 256:   # every place of the region the vertex reaches: more than one block's worth of rows is in play
                assert cnt.max() > 64
        else:
            assert got[0].shape == (35, 0) and not cnt.any()
    # the place that is its own target, inside its own region: absent (and its region's other places present)
    got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, w["place_ids"], w["regions"], t, 2 ** 40)
    i = int(np.flatnonzero(v == w["own"])[0])
    assert got[2][i] > 0 and w["own"] not in got[0][i, :got[2][i]].tolist()
    # the three positions of the repeated person: its own region each
    rep = np.flatnonzero(v == v[0])
    assert len(rep) == 3 and len({tuple(got[0][i, :5].tolist()) for i in rep}) == 3


def test_row_counts_and_null_counters(world):
    """out_row_counts is makeRecommendations' own row count (before the region join); the counters may be NULL."""
    from locations_recommender_amd import _lib as L
    w = world
    sg, v, t, pl, reg = w["sg"], w["v"], w["t"], w["place_ids"], w["regions"]
    n, stride = len(v), 7
    for max_it in (0, 20):
        off = sg.recommend_batch(v, ALPHA, 0.01, max_it)[0]
        oi, op = np.full((n, stride), -5, np.int64), np.full((n, stride), -5.0)
        cnt, rows = np.full(n, -5, np.int64), np.full(n, -5, np.int64)
        L.check(L.lib().locrec_sg_recommend_ranked_batch(
            sg._h, n, L.ptr(v, C.c_int64), ALPHA, 0.01, max_it, len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64),
            L.ptr(t, C.c_int64), stride, L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64),
            L.ptr(rows, C.c_int64), None, None))
        assert np.array_equal(rows, np.diff(off)) and rows.min() > 0
        want = w["mains"].rank_recommendations_batch(off, *sg.recommend_batch(v, ALPHA, 0.01, max_it)[1:3], pl, reg, t, stride)
        assert rb.same((oi, op, cnt), want) and cnt.max() == stride
        # without the row counts too
        L.check(L.lib().locrec_sg_recommend_ranked_batch(
            sg._h, n, L.ptr(v, C.c_int64), ALPHA, 0.01, max_it, len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64),
            L.ptr(t, C.c_int64), stride, L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64), None, None, None))
        assert rb.same((oi, op, cnt), want)


def test_empty_cases(world):
    w = world
    sg, v, t = w["sg"], w["v"][:5], w["t"][:5]
    _, _, _, its, conv = sg.recommend_batch(v, ALPHA, 0.01, 20)
    none = np.empty(0, np.int64)
    oi, op, cnt, gits, gconv = sg.recommend_ranked_batch(v, ALPHA, 0.01, 20, none, none, t, 10)   # no places at all
    assert not cnt.any() and (oi == -1).all() and np.array_equal(gits, its) and np.array_equal(gconv, conv) and its.max() > 0
    oi, op, cnt, gits, gconv = sg.recommend_ranked_batch(none, ALPHA, 0.01, 20, w["place_ids"], w["regions"], none, 10)
    assert oi.shape == (0, 0) and len(cnt) == len(gits) == len(gconv) == 0


def test_one_vertex_with_more_requests_than_a_tile_has_columns(world):
    """40 requests of one vertex (and 3 of another): one column, 40 segments."""
    w = world
    sg = w["sg"]
    v = np.r_[np.full(40, PERSON0 + 77), np.full(3, PLACE0 + 9)].astype(np.int64)
    t = np.r_[np.arange(40) % 4, [0, 1, 2]].astype(np.int64)
    t[t == 3] = NOBODYS_REGION
    for max_it in (20, 0):
        want = expected(w["mains"], sg, v, 0.01, max_it, w["place_ids"], w["regions"], t, 10)
        got = sg.recommend_ranked_batch(v, ALPHA, 0.01, max_it, w["place_ids"], w["regions"], t, 10)
        assert same_all(got, want) and got[2][t != NOBODYS_REGION].min() == 10 and not got[2][t == NOBODYS_REGION].any()
        assert pkg_stats(sg)["tiles"] == 1


def pkg_stats(sg):
    return type(sg).ranked_batch_stats()


# ---- the hand-made graph --------------------------------------------------------------------------------------------

def handmade():
    """Person 100 -> places 1..8 (1/8 each); each place -> category 50 (1.0); the category -> the 8 places (1/8 each);
    place 9 has an out-edge only (to the category)."""
    p = np.arange(1, 9, dtype=np.int64)
    src = np.concatenate([np.full(8, 100), p, np.full(8, 50), [9]]).astype(np.int64)
    dst = np.concatenate([p, np.full(8, 50), p, [50]]).astype(np.int64)
    wgt = np.concatenate([np.full(8, 0.125), np.ones(8), np.full(8, 0.125), [1.0]])
    place_ids = np.arange(1, 10, dtype=np.int64)
    return src, dst, wgt, place_ids, np.full(9, 5, np.int64)


def test_handmade_tie_group_and_source_only_place(pkg, world):
    mains = world["mains"]
    src, dst, wgt, place_ids, regions = handmade()
    sg = pkg.SgGraph(src, dst, wgt)
    v, t = np.array([100, 50, 9], np.int64), np.full(3, 5, np.int64)
    for limit in (3, 8):
        want = expected(mains, sg, v, 0.0, 5, place_ids, regions, t, limit)
        got = sg.recommend_ranked_batch(v, ALPHA, 0.0, 5, place_ids, regions, t, limit)
        assert same_all(got, want)
        for i in range(3):   # one tie group: id ascending
            assert got[2][i] == limit and got[0][i].tolist() == list(range(1, limit + 1))
            assert len(set(got[1][i].tolist())) == 1 and got[1][i][0] > 0
    # no sweep: every vertex ties at 1 / V; the source-only place appears, a target never does
    want = expected(mains, sg, v, 0.0, 0, place_ids, regions, t, 20)
    got = sg.recommend_ranked_batch(v, ALPHA, 0.0, 0, place_ids, regions, t, 20)
    assert same_all(got, want)
    assert got[0][0, :got[2][0]].tolist() == list(range(1, 10)) and got[0][2, :got[2][2]].tolist() == list(range(1, 9))
    assert (got[1][0, :9] == 1.0 / 11).all()
    # one sweep: the source-only place is gone
    want = expected(mains, sg, v, 0.0, 1, place_ids, regions, t, 20)
    got = sg.recommend_ranked_batch(v, ALPHA, 0.0, 1, place_ids, regions, t, 20)
    assert same_all(got, want) and got[0][0, :got[2][0]].tolist() == list(range(1, 9))
    sg.close()


# ---- switches, row budget, handle state, errors, stats ---------------------------------------------------------------

@pytest.mark.parametrize("env", ["LOCREC_SG_NO_COL16", "LOCREC_SG_NO_DICT", "LOCREC_SG_NO_PACK"])
def test_switches_set_before_create(pkg, world, monkeypatch, env):
    w = world
    monkeypatch.setenv(env, "1")
    sg = pkg.SgGraph(w["g"]["source_id"], w["g"]["target_id"], w["g"]["balanced_weight"])
    monkeypatch.delenv(env)
    for eps, max_it in ((0.01, 20), (0.01, 0)):
        base = w["sg"].recommend_ranked_batch(w["v"], ALPHA, eps, max_it, w["place_ids"], w["regions"], w["t"], 10)
        want = expected(w["mains"], sg, w["v"], eps, max_it, w["place_ids"], w["regions"], w["t"], 10)
        got = sg.recommend_ranked_batch(w["v"], ALPHA, eps, max_it, w["place_ids"], w["regions"], w["t"], 10)
        assert same_all(got, want) and got[2].max() == 10
        assert rb.same(got[:3], base[:3]) and np.array_equal(got[3], base[3]) and np.array_equal(got[4], base[4])
    sg.close()


@pytest.mark.parametrize("budget", [1, 97, 1000])
def test_row_budget_does_not_change_the_result(world, monkeypatch, budget):
    w = world
    sg = w["sg"]
    for limit in (10, 300):
        base = sg.recommend_ranked_batch(w["v"], ALPHA, 0.01, 20, w["place_ids"], w["regions"], w["t"], limit)
        assert pkg_stats(sg)["groups"] == 1 and base[2].max() == min(limit, int(base[2].max())) > 0
        monkeypatch.setenv("LOCREC_SG_RANKED_ROW_BUDGET", str(budget))
        got = sg.recommend_ranked_batch(w["v"], ALPHA, 0.01, 20, w["place_ids"], w["regions"], w["t"], limit)
        st = pkg_stats(sg)
        monkeypatch.delenv("LOCREC_SG_RANKED_ROW_BUDGET")
        assert rb.same(got[:3], base[:3]) and np.array_equal(got[3], base[3]) and np.array_equal(got[4], base[4])
        assert st["groups"] > 1 and st["tiles"] == 3
        if budget == 1:     # a group per request
            assert st["groups"] == len(w["v"])


def test_handle_state_after_a_ranked_batch(pkg, world):
    w = world
    src, dst, wgt = w["g"]["source_id"], w["g"]["target_id"], w["g"]["balanced_weight"]
    fresh = pkg.SgGraph(src, dst, wgt)
    used = pkg.SgGraph(src, dst, wgt)
    used.recommend_ranked_batch(w["v"], ALPHA, 0.01, 20, w["place_ids"], w["regions"], w["t"], 10)
    for vertex in (int(w["v"][0]), PLACE0 + 5, 2, int(w["v"][-1])):
        a, b = used.recommend(vertex, ALPHA, 0.01, 20), fresh.recommend(vertex, ALPHA, 0.01, 20)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:] and len(a[0]) > 0
    used.recommend_ranked_batch(w["v"], ALPHA, 0.01, 20, w["place_ids"], w["regions"], w["t"], 10)
    a, b = used.recommend_batch(w["v"], ALPHA, 0.01, 20), fresh.recommend_batch(w["v"], ALPHA, 0.01, 20)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[2].tobytes() == b[2].tobytes() and len(a[1]) > 0
    fresh.close()
    used.close()


def test_errors(pkg, world):
    from locations_recommender_amd import _lib as L
    w = world
    sg, pl, reg = w["sg"], w["place_ids"], w["regions"]
    v = np.r_[w["v"][:4], 10 ** 9].astype(np.int64)
    t = np.zeros(5, np.int64)
    oi, op = np.full(50, -7, np.int64), np.full(50, -7.0)
    cnt, rows, its, conv = np.full(5, -7, np.int64), np.full(5, -7, np.int64), np.full(5, -7, np.int64), np.full(5, -7, np.int32)
    status = L.lib().locrec_sg_recommend_ranked_batch(
        sg._h, 5, L.ptr(v, C.c_int64), ALPHA, 0.01, 20, len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64), L.ptr(t, C.c_int64),
        10, L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64), L.ptr(its, C.c_int64),
        L.ptr(conv, C.c_int32))
    assert status == L.E_NOT_FOUND and b"No such vertex in the graph: 1000000000" in L.lib().locrec_last_error()
    for o in (oi, op, cnt, rows, its, conv):
        assert (o == -7).all()
    with pytest.raises(pkg.IllegalArgumentException, match="epsilon must be non-negative"):
        sg.recommend_ranked_batch(v[:4], ALPHA, -1.0, 20, pl, reg, t[:4], 10)
    with pytest.raises(pkg.IllegalArgumentException, match="max iterations number must be non-negative"):
        sg.recommend_ranked_batch(v[:4], ALPHA, 0.01, -1, pl, reg, t[:4], 10)
    g = w["g"]
    for by_target in (False, True):
        sh = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"], shard_index=0, shard_count=2, by_target=by_target)
        with pytest.raises(pkg.IllegalArgumentException, match="sharded"):
            sh.recommend_ranked_batch(v[:4], ALPHA, 0.01, 20, pl, reg, t[:4], 10)
        sh.close()


def region_popcounts(g, place_ids, regions, targets):
    """Per request: the distinct ids of its region's places that are vertices of the graph."""
    vertices = np.unique(np.concatenate([g["source_id"], g["target_id"]]))
    return np.array([len(np.intersect1d(np.unique(place_ids[regions == r]), vertices)) for r in targets], np.int64)


@pytest.mark.parametrize("n_places", [N_PLACES, 10 * N_PLACES])
def test_stats_bound_the_read_back(pkg, world, n_places):
    """readback_bytes <= tiles * 8192 + n_targets * (16 * stride + 64), whatever T is: x stayed on the device."""
    from locations_recommender_amd import synth
    w = world
    if n_places == N_PLACES:
        g, sg, pl, reg, v, t = w["g"], w["sg"], w["place_ids"], w["regions"], w["v"], w["t"]
    else:
        g = synth.sg_dataset(n_persons=N_PERSONS, n_places=n_places, n_categories=N_CATEGORIES, seed=8)
        sg = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"])
        pl, reg = places_table(n_places)
        person0 = int(g["first_person"])
        v = np.r_[person0 + np.arange(0, 1200, 40), PLACE0 + np.arange(0, 3000, 500)].astype(np.int64)
        t = (np.arange(len(v)) % 3).astype(np.int64)
    assert sg.live_count() > 0.9 * n_places
    stride = 10
    for eps, max_it in ((0.01, 20), (1e-9, 200), (0.01, 0)):
        want = expected(w["mains"], sg, v, eps, max_it, pl, reg, t, stride)
        got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, pl, reg, t, stride)
        st = pkg_stats(sg)
        assert same_all(got, want) and got[2].max() == stride
        tiles = -(-len(np.unique(v)) // 16)
        assert st["tiles"] == tiles and st["groups"] == 1 and st["host_syncs"] > 0
        assert 0 < st["emitted_rows"] <= region_popcounts(g, pl, reg, t).sum()
        assert 0 < st["readback_bytes"] <= tiles * 8192 + len(v) * (16 * stride + 64), st
    if n_places != N_PLACES:
        sg.close()
