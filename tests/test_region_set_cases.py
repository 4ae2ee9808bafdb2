"""CPU checks of the region sets of the builder mains: the numpy restatement (tests/region_set_cases.py) on a
hand-written case, the order of the sets, the day arithmetic of visitsFrom, and the Parquet writers of mains.py against
the readers (mains.load_* and, where it is built, liblocrec_parquet.so)."""
import os
from datetime import timedelta, timezone

import numpy as np
import pytest

import region_set_cases as rsc


@pytest.fixture
def mains(pkg):
    from locations_recommender_amd import mains
    return mains


def test_restatement_on_the_hand_written_case():
    regions = rsc.HAND_REGIONS
    assert len(regions) == 12
    assert rsc.extract_region_ids(regions[regions != 42]).tolist() == [3, 5, 7]
    for rs, rows in rsc.HAND_SET_ROWS.items():
        assert rsc.set_rows(regions, rs).tolist() == rows, rs
        assert rsc.set_rows(regions, rs[::-1]).tolist() == rows, rs
    rows, offsets = rsc.partition(regions, [3, 5, 7])
    assert rows.tolist() == rsc.HAND_PARTITION[0] and offsets.tolist() == rsc.HAND_PARTITION[1] and rows.dtype == np.int32
    # a pair's rows are the stable merge of its two groups
    for (a, b) in [(0, 1), (0, 2), (1, 2)]:
        merged = np.sort(np.concatenate([rows[offsets[a]:offsets[a + 1]], rows[offsets[b]:offsets[b + 1]]]))
        assert merged.tolist() == rsc.HAND_SET_ROWS[((3, 5, 7)[a], (3, 5, 7)[b])]
    table = rsc.table_for(regions)
    pv = rsc.place_visits_of_set(table, (3, 7))
    assert pv["person_id"].tolist() == [2040 + 7 * r for r in rsc.HAND_SET_ROWS[(3, 7)]]
    assert set(pv["region_id"].tolist()) == {3, 7} and sorted(pv) == sorted(rsc.PLACE_VISIT_COLUMNS)
    assert rsc.max_timestamp([5, -3, 9, 9, 1]) == 9
    with pytest.raises(ValueError):
        rsc.max_timestamp([])


def test_case_generators_have_the_lengths_and_limits_they_name():
    for la, lb in rsc.RUN_LENGTHS:
        for how in rsc.INTERLEAVINGS:
            regions, listed = rsc.run_case(la, lb, how, seed=la + lb)
            assert (regions == rsc.REGION_A).sum() == la and (regions == rsc.REGION_B).sum() == lb
            assert (regions == rsc.REGION_EMPTY).sum() == 0 and (regions == rsc.REGION_UNLISTED).sum() >= 2
            assert listed.tolist() == [rsc.REGION_A, rsc.REGION_EMPTY, rsc.REGION_B]
    regions, ids = rsc.many_regions_case(3)
    assert len(regions) == 70_000 and len(ids) == 7 and ids.min() < 0 and np.all(np.diff(ids) > 0)
    assert all((regions == r).sum() > 0 for r in ids) and (regions == 1000).sum() > 0
    assert len(rsc.region_sets(ids)) == 28


@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_set_order(pkg, r):
    """Seq.map(Seq(_)) ++ combinations(2): the single regions in the given order, then the pairs in combinations' order."""
    ids = [9, -5, 2, 30][:r]
    want = {1: [(9,)], 2: [(9,), (-5,), (9, -5)], 3: [(9,), (-5,), (2,), (9, -5), (9, 2), (-5, 2)],
            4: [(9,), (-5,), (2,), (30,), (9, -5), (9, 2), (9, 30), (-5, 2), (-5, 30), (2, 30)]}[r]
    assert pkg.prep.region_sets(ids) == want == rsc.region_sets(ids)
    assert pkg.prep.region_sets(np.asarray(ids, np.int64)) == want
    assert len(want) == r + r * (r - 1) // 2


def test_visits_from_timestamp_in_utc_and_at_a_fixed_offset(pkg):
    f = pkg.prep.visits_from_timestamp
    for max_ts in (1_600_000_000_123, 0, -86_400_001, 1_616_893_200_000):
        for days in (0, 1, 60, 365):
            want = rsc.visits_from_fixed_offset(max_ts, days)
            assert f(max_ts, days) == want
            assert f(max_ts, days, timezone.utc) == want
            assert f(max_ts, days, timezone(timedelta(hours=3))) == want
    assert isinstance(f(5, 1), int)


def test_visits_from_timestamp_across_a_march_switch(pkg):
    """Europe/Berlin, 2021-03-28 02:00 -> 03:00: two wall-clock days back from 29 March 12:00 CEST is 27 March 12:00 CET,
    one hour LESS than 48 hours (28 March has 23).  Runs where the zone's data loads."""
    zoneinfo = pytest.importorskip("zoneinfo")
    try:
        berlin = zoneinfo.ZoneInfo("Europe/Berlin")
    except Exception:
        pytest.skip("no time zone data for Europe/Berlin")
    from datetime import datetime
    at = int(datetime(2021, 3, 29, 12, 0, tzinfo=berlin).timestamp() * 1000)
    got = pkg.prep.visits_from_timestamp(at, 2, berlin)
    assert got == at - 2 * rsc.MS_PER_DAY + 3_600_000
    assert got == int(datetime(2021, 3, 27, 12, 0, tzinfo=berlin).timestamp() * 1000)


# ---- the writers against the readers -----------------------------------------------------------------------------------

def native():
    from locations_recommender_amd import parquet
    return parquet if os.path.exists(parquet.LIB_PATH) else None


def ratings_and_vectors(mains, seed, n=900):
    import prep_cases
    p, e = prep_cases.visits_case(seed, n, persons=30, entities=50)
    c = e % 7
    pr = mains.calc_ratings(p, e, 5)
    cr = mains.calc_ratings(p, c, 3)
    return pr, mains.calc_rating_vectors(*pr), mains.calc_rating_vectors(*cr)


def test_vector_and_rating_writers_round_trip(mains, tmp_path):
    pr, pv, cv = ratings_and_vectors(mains, 4)
    names = [str(tmp_path / f"{f}_region2_region9") for f in ("place_rating_vectors", "category_rating_vectors", "place_ratings")]
    mains.write_rating_vectors(names[0], *pv)
    mains.write_rating_vectors(names[1], *cv)
    mains.write_place_ratings(names[2], *pr)
    for name in names:
        assert sorted(os.listdir(name)) == ["_SUCCESS", "part-00000.parquet"]
    for name, want in ((names[0], pv), (names[1], cv)):
        got = mains.load_rating_vectors(name)
        assert got[4] == want[4] and got[2].dtype == np.int32
        for g, w in zip(got[:4], want[:4]):
            assert np.array_equal(g, w)
    for g, w in zip(mains.load_place_ratings(names[2]), pr):
        assert np.array_equal(g, w)
    # writing again replaces the part file
    mains.write_place_ratings(names[2], pr[0][:3], pr[1][:3], pr[2][:3])
    assert sorted(os.listdir(names[2])) == ["_SUCCESS", "part-00000.parquet"]
    assert len(mains.load_place_ratings(names[2])[0]) == 3
    mains.write_place_ratings(names[2], *pr)
    if native() is None:
        return
    got = native().read_knn(*names)
    ids = pv[0]
    assert np.array_equal(got["person_ids"], ids) and got["p_dim"] == pv[4] and got["c_dim"] == cv[4]
    assert np.array_equal(got["p_rowptr"], pv[1]) and np.array_equal(got["p_idx"], pv[2]) and np.array_equal(got["p_val"], pv[3])
    assert np.array_equal(got["c_rowptr"], cv[1]) and np.array_equal(got["c_idx"], cv[2]) and np.array_equal(got["c_val"], cv[3])
    assert np.array_equal(got["r_rowptr"], pv[1]) and np.array_equal(got["r_place"], pr[1]) and np.array_equal(got["r_rating"], pr[2])


def test_graph_and_place_visit_writers_round_trip(mains, tmp_path):
    rng = np.random.default_rng(5)
    s, t = rng.integers(-9, 400, 700), rng.integers(0, 2 ** 40, 700)
    w = rng.random(700) / 3.0
    name = mains.generate_file_name([9, 2], str(tmp_path), "stochastic_graph")
    mains.write_stochastic_graph(name, s, t, w)
    gs, gt, gw = mains.load_stochastic_graph(name)
    assert np.array_equal(gs, s) and np.array_equal(gt, t) and np.array_equal(gw.view(np.int64), w.view(np.int64))
    if native() is not None:
        ns, nt, nw = native().read_edges(name)
        assert np.array_equal(ns, s) and np.array_equal(nt, t) and np.array_equal(nw.view(np.int64), w.view(np.int64))
    table = rsc.table_for(rsc.HAND_REGIONS, seed=2)
    mains.write_place_visits(str(tmp_path / "place_visits"), table)
    got = mains.load_place_visits(str(tmp_path / "place_visits"))
    assert sorted(got) == sorted(rsc.PLACE_VISIT_COLUMNS)
    for k in rsc.PLACE_VISIT_COLUMNS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], table[k]), k
    import pyarrow as pa
    import pyarrow.parquet as pq
    assert pa.types.is_timestamp(pq.read_table(str(tmp_path / "place_visits")).schema.field("timestamp").type)


def test_empty_sets_write_empty_files_with_the_full_schema(mains, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    none = np.empty(0, np.int64)
    names = [str(tmp_path / f"{f}_region7") for f in ("place_rating_vectors", "category_rating_vectors", "place_ratings")]
    mains.write_rating_vectors(names[0], none, None, none, none, 0)
    mains.write_rating_vectors(names[1], none, np.zeros(1, np.int64), none, none, 0)
    mains.write_place_ratings(names[2], none, none, none)
    graph = str(tmp_path / "stochastic_graph_region7")
    mains.write_stochastic_graph(graph, none, none, np.empty(0, np.float64))
    schema = pq.read_table(names[0]).schema
    assert schema.names == ["person_id", "rating_vector"] and schema.field("person_id").type == pa.int64()
    vec = schema.field("rating_vector").type
    assert [(f.name, f.type) for f in vec] == [("type", pa.int8()), ("size", pa.int32()), ("indices", pa.list_(pa.int32())),
                                                ("values", pa.list_(pa.float64()))]
    assert pq.read_table(names[2]).schema.names == ["person_id", "place_id", "rating"]
    gschema = pq.read_table(graph).schema
    assert gschema.names == ["source_id", "target_id", "balanced_weight"] and gschema.field("balanced_weight").type == pa.float64()
    ids, rowptr, idx, val, dim = mains.load_rating_vectors(names[0])
    assert len(ids) == 0 and rowptr.tolist() == [0] and len(idx) == 0 and len(val) == 0 and dim == 0
    assert all(len(a) == 0 for a in mains.load_place_ratings(names[2]))
    assert all(len(a) == 0 for a in mains.load_stochastic_graph(graph))
    if native() is not None:
        got = native().read_knn(*names)
        assert len(got["person_ids"]) == 0 and got["p_rowptr"].tolist() == [0]
        assert all(len(a) == 0 for a in native().read_edges(graph))


def test_sample_table_loaders_widen_regions_and_reduce_timestamps(mains, tmp_path):
    """region_id as int32 and as a dictionary (a Hive partition column); timestamps of micro- and millisecond units,
    before 1970 too (floor)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    ts_ms = np.array([1_600_000_000_123, -1, 0, 86_400_000], np.int64)
    us = pa.array(ts_ms * 1000 + np.array([7, 999, 0, 1]), pa.int64()).cast(pa.timestamp("us"))
    visits = pa.table({"person_id": pa.array([1, 2, 3, 4], pa.int64()), "timestamp": us,
                       "latitude": [55.0, 55.1, 55.2, 55.3], "longitude": [37.0, 37.1, 37.2, 37.3],
                       "region_id": pa.array([2, 2, 9, -5], pa.int32())})
    pq.write_table(visits, tmp_path / "location_visits_sample")
    places = pa.table({"id": pa.array([40, 41], pa.int64()), "name": ["a", "b"], "latitude": [55.0, 55.1], "longitude": [37.0, 37.1],
                       "region_id": pa.array([9, 2], pa.int32()).dictionary_encode(), "category_id": pa.array([3, 4], pa.int64())})
    pq.write_table(places, tmp_path / "places_sample")
    v = mains.load_location_visits(str(tmp_path))
    assert v["timestamp"].tolist() == [1_600_000_000_123, -1, 0, 86_400_000] and v["timestamp"].dtype == np.int64
    assert v["region_id"].tolist() == [2, 2, 9, -5] and v["region_id"].dtype == np.int64 and v["latitude"].dtype == np.float64
    p = mains.load_places_full(str(tmp_path))
    assert p["region_id"].tolist() == [9, 2] and p["region_id"].dtype == np.int64 and p["category_id"].tolist() == [3, 4]
    assert sorted(p) == ["category_id", "id", "latitude", "longitude", "region_id"]
    assert [a.tolist() for a in mains.load_places(str(tmp_path))] == [[40, 41], [9, 2]]
    pq.write_table(visits.set_column(1, "timestamp", pa.array(ts_ms, pa.int64()).cast(pa.timestamp("ms"))),
                   tmp_path / "location_visits_sample")
    assert mains.load_location_visits(str(tmp_path))["timestamp"].tolist() == ts_ms.tolist()
