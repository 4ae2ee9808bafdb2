"""GPU: the mains' batched callers (mains.knn_recommend_places_batch, mains.sg_recommend_places_batch) on Parquet sets
written like the reference's builders write them: requests of one region pair, each with its own target region,
against the single-request callers followed by the oracle's ranker."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import rank_batch_cases as rb
from test_mains import knn_files

pytestmark = pytest.mark.gpu


@pytest.fixture
def mains(pkg):
    from locations_recommender_amd import mains
    return mains


def write_places(tmp_path, ids, regions):
    pq.write_table(pa.table({"id": ids, "latitude": np.zeros(len(ids)), "longitude": np.zeros(len(ids)),
                             "region_id": pa.array(regions, pa.int32())}), tmp_path / "places_sample")


def want_rows(oracle, rows, place_ids, regions, targets, limit):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r[0]) for r in rows], out=off[1:])
    case = dict(offsets=off, ids=np.concatenate([r[0] for r in rows]), scores=np.concatenate([r[1] for r in rows]),
                place_ids=place_ids, regions=regions, targets=np.asarray(targets, np.int64))
    return rb.expected(oracle.rank_recommendations, case, limit)


def test_knn_recommend_places_batch(mains, tmp_path, pkg, oracle):
    from locations_recommender_amd import synth
    d = synth.knn_dataset(1_500, 300, seed=9)
    knn_files(tmp_path, d)
    place_ids = np.arange(40, 340, dtype=np.int64)
    regions = np.where(place_ids % 2 == 0, 0, 2)
    write_places(tmp_path, place_ids, regions)
    requests = [(int(d["person_ids"][r]), t) for r, t in [(3, 0), (900, 2), (3, 2), (1499, 0), (77, 5)]]
    oi, osc, cnt = mains.knn_recommend_places_batch(str(tmp_path), [2, 0], requests, 0.5, 0.5, 50, 10)
    rows = [mains.knn_make_recommendations(str(tmp_path), [0, 2], p, 0.5, 0.5, 50) for p, _ in requests]
    wi, ws, wc = want_rows(oracle, rows, place_ids, regions, [t for _, t in requests], 10)
    assert oi.shape == (5, 10) and cnt.tolist() == wc.tolist() and cnt[-1] == 0 and cnt[:4].min() > 0
    for q in range(5):
        assert oi[q, :cnt[q]].tolist() == wi[q, :wc[q]].tolist() and (oi[q, cnt[q]:] == -1).all()
        np.testing.assert_allclose(osc[q, :cnt[q]], ws[q, :wc[q]], rtol=1e-12, atol=0)   # batched against single aggregation
    with pytest.raises(pkg.IllegalArgumentException, match="No such person"):
        mains.knn_recommend_places_batch(str(tmp_path), [0, 2], [(10 ** 9, 0)], 0.5, 0.5, 50)
    pkg.lib().locrec_cache_clear()


def test_sg_recommend_places_batch(mains, tmp_path, pkg, oracle):
    from locations_recommender_amd import synth
    g = synth.sg_dataset(n_persons=1_200, n_places=300, seed=8)
    pq.write_table(pa.table({"source_id": g["source_id"], "target_id": g["target_id"],
                             "balanced_weight": g["balanced_weight"]}), tmp_path / "stochastic_graph_region0_region2")
    place_ids = np.arange(40, 340, dtype=np.int64)
    regions = np.where(place_ids % 2 == 0, 0, 2)
    write_places(tmp_path, place_ids, regions)
    v0 = int(g["first_person"])
    requests = [(v0 + 3, 0), (v0 + 700, 2), (v0 + 3, 2), (v0 + 11, 7)]
    oi, op, cnt, its, conv = mains.sg_recommend_places_batch(str(tmp_path), [0, 2], requests, 0.01, 20, max_recommendations=10)
    rows = [mains.sg_make_recommendations(str(tmp_path), [0, 2], v, 0.01, 20) for v, _ in requests]
    want = want_rows(oracle, [(r[0], r[1]) for r in rows], place_ids, regions, [t for _, t in requests], 10)
    assert rb.same((oi, op, cnt), want) and cnt[-1] == 0 and cnt[:3].min() > 0
    assert its.tolist() == [r[2] for r in rows] and conv.tolist() == [r[3] for r in rows]
    pkg.lib().locrec_cache_clear()
