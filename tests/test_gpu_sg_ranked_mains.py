"""GPU: the host layers above the ranked SG batch.  StochasticRecommender.makeRecommendationsRankedBatch against the
per-vertex makeRecommendations followed by mains.rank_recommendations, and mains.sg_recommend_places_batch on the device
against its host-ranked form (on_device=False) on a Parquet set written like the reference's builders write it."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import rank_batch_cases as rb

pytestmark = pytest.mark.gpu


def places_frame():
    ids = np.r_[np.arange(40, 340), [45, 46, 47], [50, 51], [777_777]].astype(np.int64)     # listed twice; a second region
    regions = np.r_[np.where(np.arange(40, 340) % 2 == 0, 0, 2), [2, 0, 2], [1, 1], [0]].astype(np.int64)
    return ids, regions


def test_make_recommendations_ranked_batch(pkg, capsys):
    from locations_recommender_amd import mains, synth
    g = synth.sg_dataset(n_persons=1_200, n_places=300, seed=8)
    edges = pd.DataFrame({"source_id": g["source_id"], "target_id": g["target_id"], "balanced_weight": g["balanced_weight"]})
    ids, regions = places_frame()
    places = pd.DataFrame({"id": ids, "region_id": regions.astype(np.int32)})
    p0 = int(g["first_person"])
    vertices = [p0 + 3, 45, p0 + 3, 2, p0 + 900] + [p0 + 100 + i for i in range(14)]     # 17 distinct: two tiles
    targets = [0, 0, 2, 1, 7] + [i % 3 for i in range(14)]
    rec = pkg.StochasticRecommender(edges, epsilon=0.01, maxIterations=20)
    capsys.readouterr()
    singles = [rec.makeRecommendations(vertexId=v) for v in vertices]
    single_out = capsys.readouterr().out
    for limit in (10, 1000):
        df = rec.makeRecommendationsRankedBatch(vertices, places, targets, limit)
        assert capsys.readouterr().out == single_out
        assert list(df.columns) == ["vertex_id", "id", "probability"]
        at = 0
        for v, t, s in zip(vertices, targets, singles):
            wi, wp = mains.rank_recommendations(s["id"].to_numpy(), s["probability"].to_numpy(), ids, regions, t, limit)
            part = df.iloc[at:at + len(wi)]
            at += len(wi)
            assert (part["vertex_id"] == v).all() and part["id"].tolist() == wi.tolist()
            assert part["probability"].to_numpy().tobytes() == wp.tobytes()
            assert (len(wi) > 0) == (t != 7) and 45 not in (wi.tolist() if v == 45 else [])
        assert at == len(df) > 0
    with pytest.raises(pkg.IllegalArgumentException, match="No such vertex in the graph: 10000000"):
        rec.makeRecommendationsRankedBatch([p0, 10_000_000], places, [0, 0], 10)
    quiet = pkg.StochasticRecommender(edges, epsilon=0.01, maxIterations=20, quiet=True)
    capsys.readouterr()
    quiet.makeRecommendationsRankedBatch(vertices, places, targets, 10)
    assert capsys.readouterr().out == ""
    rec.close()
    quiet.close()
    pkg.lib().locrec_cache_clear()


def test_sg_recommend_places_batch_on_device_against_host_ranked(pkg, tmp_path):
    from locations_recommender_amd import mains, synth
    g = synth.sg_dataset(n_persons=1_200, n_places=300, seed=8)
    pq.write_table(pa.table({"source_id": g["source_id"], "target_id": g["target_id"],
                             "balanced_weight": g["balanced_weight"]}), tmp_path / "stochastic_graph_region0_region2")
    ids, regions = places_frame()
    pq.write_table(pa.table({"id": ids, "latitude": np.zeros(len(ids)), "longitude": np.zeros(len(ids)),
                             "region_id": pa.array(regions, pa.int32())}), tmp_path / "places_sample")
    v0 = int(g["first_person"])
    requests = [(v0 + 3, 0), (v0 + 700, 2), (v0 + 3, 2), (v0 + 11, 7), (46, 0), (3, 1)] + [(v0 + 20 + i, i % 3) for i in range(30)]
    for eps, max_it, limit in ((0.01, 20, 10), (0.01, 0, 400), (0.0, 2, 1)):
        dev = mains.sg_recommend_places_batch(str(tmp_path), [0, 2], requests, eps, max_it, max_recommendations=limit)
        host = mains.sg_recommend_places_batch(str(tmp_path), [0, 2], requests, eps, max_it, max_recommendations=limit,
                                               on_device=False)
        assert rb.same(dev[:3], tuple(np.asarray(x) for x in host[:3])) and dev[2][3] == 0 and dev[2][:3].min() > 0
        assert np.array_equal(dev[3], host[3]) and np.array_equal(dev[4], host[4])
        assert 46 not in dev[0][4].tolist() and dev[2][4] > 0
    pkg.lib().locrec_cache_clear()
