"""End to end: sample_generator_main at its smallest useful size -> calc_place_visits -> mains.knn_holdout_evaluation and
mains.sg_holdout_evaluation, against the same protocol done the old way - the set model's split, the existing ranked
calls, the rows on the host and the set-and-fsum model of tests/eval_cases.py.  Integers are exact; the means are within
eval_cases' tolerance, (requests + 4 (k + 2)) 2^-53 relative, whatever the batch."""
import numpy as np
import pytest
import torch

import eval_cases as ec
import sample_cases as sc

pytestmark = pytest.mark.gpu
N_PLACES = N_PERSONS = 200
CUTOFFS = [1, 5, 10]
KNN = (0.5, 0.5, 10)                  # place weight, category weight, k nearest
SG = (0.15, 0.01, 20, 0.5, 0.5)       # alpha, epsilon, max iterations, the two betas


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


@pytest.fixture(scope="module")
def world(pkg, oracle, tmp_path_factory):
    """The sample's place visits on the device and on the host, the places, and the cut at the median timestamp.  That
    the sample is large enough is settled on the CPU first: the restatement joined by the oracle, split by the model,
    holds out places on either setting of new_places, and more with visited places allowed."""
    from locations_recommender_amd import mains
    D = sc.defaults()
    regions = D["regions"][:2]
    want = sc.generate(N_PLACES, N_PERSONS, regions, D["categories"])
    v, p = want["location_visits"], want["places"]
    vr, pr = oracle.place_visits(v, p, int(v["timestamp"].min()))
    cols = (v["person_id"][vr], v["timestamp"][vr], p["id"][pr], v["region_id"][vr])
    cut = int(np.median(cols[1]))
    every, new = (ec.model_holdout(*cols, cut, flag)[1] for flag in (False, True))
    assert 0 < len(new) < len(every) and {r for _, r, _ in new} == {regions[0][0], regions[1][0]}

    t = mains.sample_generator_main(str(tmp_path_factory.mktemp("eval")), N_PLACES, N_PERSONS, regions, D["categories"])
    pv = pkg.prep.calc_place_visits(t["location_visits"], t["places"], int(v["timestamp"].min()))
    pv_host = {k: host(a) for k, a in pv.items()}
    assert np.array_equal(np.sort(pv_host["timestamp"]), np.sort(cols[1]))
    places = {"id": host(t["places"]["id"]), "region_id": host(t["places"]["region_id"])}
    return {"pv": pv, "pv_host": pv_host, "places": places, "cut": cut}


def old_way(pkg, world, new_places, build, rank):
    """The model's split, a recommender built from the train rows (host arrays), one ranked call for all requests, the
    model's evaluation of the host rows."""
    pv = world["pv_host"]
    train_rows, held = ec.model_holdout(pv["person_id"], pv["timestamp"], pv["place_id"], pv["region_id"], world["cut"], new_places)
    train = {k: a[train_rows] for k, a in pv.items()}
    requests = sorted({(p, r) for p, r, _ in held})
    persons, regions = np.array([p for p, _ in requests], np.int64), np.array([r for _, r in requests], np.int64)
    lists = {q: [] for q in requests}
    for p, r, place in held:
        lists[(p, r)].append(place)
    offsets = np.zeros(len(requests) + 1, np.int64)
    np.cumsum([len(lists[q]) for q in requests], out=offsets[1:])
    rel = np.array([x for q in requests for x in lists[q]], np.int64)
    handle = build(train)
    try:
        ids, counts = rank(handle, train, persons, regions)
    finally:
        handle.close()
    return ec.model_eval(ids, counts, offsets, rel, CUTOFFS), persons, regions


def assert_same_evaluation(got, want, persons, regions):
    assert np.array_equal(got["person_ids"], persons) and np.array_equal(got["region_ids"], regions)
    assert got["evaluated"] == want["evaluated"] > 0
    assert np.array_equal(got["relevant"], want["relevant"]) and np.array_equal(got["coverage"], want["coverage"])
    for j, k in enumerate(CUTOFFS):
        tol = (len(persons) + 4 * (k + 2)) * ec.U
        assert (np.abs(got["means"][j] - want["means"][j]) <= tol * np.abs(want["means"][j])).all(), (k, got["means"][j], want["means"][j])


def test_knn_holdout_evaluation(pkg, world):
    from locations_recommender_amd import mains
    prep, places = pkg.prep, world["places"]
    totals = []
    for new_places in (True, False):
        def rank(ix, train, persons, regions):
            ids, _, counts = ix.recommend_ranked_batch(persons, *KNN, places["id"], places["region_id"], regions, max(CUTOFFS),
                                                       unvisited=new_places)
            return ids, counts
        want, persons, regions = old_way(pkg, world, new_places,
                                         lambda tr: prep.knn_index_from_visits(tr["person_id"], tr["place_id"], tr["category_id"]), rank)
        got = mains.knn_holdout_evaluation(world["pv"], places, world["cut"], *KNN, CUTOFFS, new_places=new_places)
        assert_same_evaluation(got, want, persons, regions)
        small = mains.knn_holdout_evaluation(world["pv"], places, world["cut"], *KNN, CUTOFFS, new_places=new_places, batch=7)
        assert_same_evaluation(small, want, persons, regions)
        totals.append(int(got["relevant"].sum()))
    assert totals[0] < totals[1], "new_places must change what is relevant on this data"


def test_sg_holdout_evaluation(pkg, world):
    from locations_recommender_amd import mains
    from locations_recommender_amd.stochastic import out_neighbours
    prep, places = pkg.prep, world["places"]
    alpha, epsilon, max_iterations, beta_place, beta_category = SG
    totals = []
    for new_places in (True, False):
        def rank(g, train, persons, regions):
            s, t, _ = prep.generate_stochastic_graph(train, beta_place, beta_category)
            excluded = out_neighbours(s, t, persons) if new_places else None
            ids, _, counts, _, _ = g.recommend_ranked_batch(persons, alpha, epsilon, max_iterations, places["id"], places["region_id"],
                                                            regions, max(CUTOFFS), excluded=excluded)
            return ids, counts
        want, persons, regions = old_way(pkg, world, new_places, lambda tr: prep.sg_graph_from_visits(tr, beta_place, beta_category),
                                         rank)
        got = mains.sg_holdout_evaluation(world["pv"], places, world["cut"], *SG, CUTOFFS, new_places=new_places)
        assert_same_evaluation(got, want, persons, regions)
        small = mains.sg_holdout_evaluation(world["pv"], places, world["cut"], *SG, CUTOFFS, new_places=new_places, batch=7)
        assert_same_evaluation(small, want, persons, regions)
        totals.append(int(got["relevant"].sum()))
    assert totals[0] < totals[1], "new_places must change what is relevant on this data"
