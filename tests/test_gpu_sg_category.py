"""GPU: the ranked SG batch by category (locrec_sg_recommend_ranked_batch_by_category,
SgGraph.recommend_ranked_batch_by_category) in the world of test_gpu_sg_near.  Expected: recommend_batch's host rows
through the composition of rank_category_cases - the place table cut to the listings that pass (target region,
allow-list, circle), the listed ids leave, oracle.rank_recommendations ranks per request, then the greedy walk with a
counter per category.  Ids, counts, probability bits and distance bits are equal; the host route (on_device=False) agrees
within the 1e-6 bar of the ranked SG tests."""
import numpy as np
import pytest

import rank_batch_cases as rb
import rank_category_cases as rc
import rank_near_cases as rn
from test_gpu_sg_ranked import ALPHA, main_requests, pkg_stats, places_table

pytestmark = pytest.mark.gpu
LIMITS = (1, 2, 10, 256, 257, 2 ** 40)


@pytest.fixture(scope="module")
def world(pkg):
    from locations_recommender_amd import stochastic, synth
    g = synth.sg_dataset(n_persons=1_200, n_places=300, n_categories=20, seed=8)
    sg = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"])
    place_ids, regions = places_table()
    v, t, _ = main_requests(place_ids, regions)
    assert len(v) > 16 and v[9] == v[0]
    t[9] = t[0]                                    # the repeated vertex: one region, two lists and caps
    circ = rn.with_circles(dict(place_ids=place_ids, regions=regions, targets=t), 4)
    circ["radius"] = np.array([rc.RADII[(s + 1) % 3] for s in range(len(t))])
    circ["radius"][0] = circ["radius"][9] = np.inf
    base = dict(circ, cats=rc.categories(3, len(place_ids)))
    lists = rc.allow_lists(3, base)
    lists[0] = lists[9] = np.empty(0, np.int64)    # ... and no list for either
    base = rc.with_allow(base, lists)
    yield dict(g=g, sg=sg, v=v, t=t, base=base, lists=stochastic.out_neighbours(g["source_id"], g["target_id"], v))
    sg.close()


def call(w, case, eps, max_it, limit, lists, circles, on_device=True):
    c = tuple(case[k] for k in ("lat", "lon", "clat", "clon", "radius")) if circles else None
    return w["sg"].recommend_ranked_batch_by_category(w["v"], ALPHA, eps, max_it, case["place_ids"], case["regions"], w["t"], limit,
                                                      case["cats"], allowed=(case["al_offsets"], case["al_ids"]),
                                                      max_per_category=case.get("caps"), circles=c, excluded=lists,
                                                      on_device=on_device)


def expected(oracle, w, case, eps, max_it, lists, limit, kept, circles):
    off, ids, probs, its, conv = w["sg"].recommend_batch(w["v"], ALPHA, eps, max_it)
    case = dict(case, offsets=off, ids=ids, scores=probs)
    if not circles:
        case = {k: v for k, v in case.items() if k not in ("lat", "lon", "clat", "clon", "radius")}
    if lists is not None:
        case.update(ex_offsets=lists[0], ex_ids=lists[1])
    return rc.expected(oracle.rank_recommendations, case, limit, kept if circles else None), its, conv


@pytest.mark.parametrize("with_lists,circles", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["all", "new", "near", "new-near"])
@pytest.mark.parametrize("eps,max_it", ((0.01, 20), (0.0, 3)))
def test_category_batch(pkg, oracle, world, eps, max_it, with_lists, circles):
    w = world
    lists = w["lists"] if with_lists else None
    kept = rn.all_kept(pkg.prep.distance_meters, w["base"])
    changed = 0
    for limit in LIMITS:
        case = rc.with_caps(w["base"], limit, 1)
        case["caps"][0], case["caps"][9] = rc.NO_CAP, 1
        ranked, its, conv = expected(oracle, w, case, eps, max_it, lists, limit, kept, circles)
        got = call(w, case, eps, max_it, limit, lists, circles)
        assert rc.same(got[:4], ranked, meters=circles), (eps, max_it, limit)
        assert (got[2] is None) == (not circles)
        assert np.array_equal(got[4], its) and np.array_equal(got[5], conv)
        host = call(w, case, eps, max_it, limit, lists, circles, on_device=False)
        assert np.array_equal(got[0], np.asarray(host[0])) and np.array_equal(got[3], np.asarray(host[3]))
        np.testing.assert_allclose(got[1], np.asarray(host[1]), rtol=1e-6, atol=0)
        free, _, _ = expected(oracle, w, {k: v for k, v in case.items() if k != "caps"}, eps, max_it, lists, limit, kept, circles)
        changed += int(not np.array_equal(free[0], ranked[0]))
    assert pkg_stats(w["sg"])["tiles"] == 3
    assert changed > 0                                               # the caps bite
    # the repeated vertex is ranked per position with its own cap: at most one row per category against no cap
    assert got[3][9] <= min(len(rc.FEW), got[3][0]) and (got[3][9] > 0) == (got[3][0] > 0)


@pytest.mark.parametrize("budget", [1, 97])
def test_row_budget_does_not_change_the_result(world, monkeypatch, budget):
    w = world
    for limit in (10, 300):
        case = rc.with_caps(w["base"], limit, 2)
        base = call(w, case, 0.01, 20, limit, w["lists"], True)
        assert pkg_stats(w["sg"])["groups"] == 1 and base[3].max() > 0
        monkeypatch.setenv("LOCREC_SG_RANKED_ROW_BUDGET", str(budget))
        got = call(w, case, 0.01, 20, limit, w["lists"], True)
        st = pkg_stats(w["sg"])
        monkeypatch.delenv("LOCREC_SG_RANKED_ROW_BUDGET")
        assert rc.same(got[:4], base[:4]) and np.array_equal(got[4], base[4]) and np.array_equal(got[5], base[5])
        assert st["groups"] > 1 and st["tiles"] == 3
        if budget == 1:     # a group per request
            assert st["groups"] == len(w["v"])


def test_identity_and_errors(pkg, world):
    w = world
    sg, v, c = w["sg"], w["v"], w["base"]
    plain = sg.recommend_ranked_batch(v, ALPHA, 0.01, 20, c["place_ids"], c["regions"], w["t"], 10, excluded=w["lists"])
    for caps in (None, np.full(len(v), 10, np.int64)):
        got = sg.recommend_ranked_batch_by_category(v, ALPHA, 0.01, 20, c["place_ids"], c["regions"], w["t"], 10, c["cats"],
                                                    max_per_category=caps, excluded=w["lists"])
        assert rb.same((got[0], got[1], got[3]), plain[:3]) and np.array_equal(got[4], plain[3]) and got[2] is None
    with pytest.raises(pkg.IllegalArgumentException, match="max_per_category"):
        sg.recommend_ranked_batch_by_category(v, ALPHA, 0.01, 20, c["place_ids"], c["regions"], w["t"], 10, c["cats"],
                                              max_per_category=np.zeros(len(v), np.int64))
    with pytest.raises(pkg.IllegalArgumentException, match="No such vertex in the graph"):
        sg.recommend_ranked_batch_by_category(np.r_[v[:-1], 10 ** 9], ALPHA, 0.01, 20, c["place_ids"], c["regions"], w["t"], 10,
                                              c["cats"], max_per_category=np.ones(len(v), np.int64))
    again = sg.recommend_ranked_batch(v, ALPHA, 0.01, 20, c["place_ids"], c["regions"], w["t"], 10, excluded=w["lists"])
    assert rb.same(again[:3], plain[:3])
