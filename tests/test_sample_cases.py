"""CPU checks of the head and the tail of the reference's walk-through: the request line of the recommender mains
(RecommenderMainCommon.scala:16-56) and the numpy restatement of the sample generator (tests/sample_cases.py) that the
GPU tests compare the device against."""
import numpy as np
import pytest

import sample_cases as sc


@pytest.fixture(scope="module")
def mains(pkg):
    from locations_recommender_amd import mains
    return mains


# ---- parse_input / calc_recommender_target ----------------------------------------------------------------------------

@pytest.mark.parametrize("line, want", [("123", (123, None)), ("123 4", (123, 4)), ("123  4", (123, 4)), ("123\t4", (123, 4)),
                                        ("12 ", (12, None)), ("9223372036854775807", (2 ** 63 - 1, None)), ("007 08", (7, 8)),
                                        ("1234", (1234, None))])
def test_parse_input(mains, line, want):
    assert mains.parse_input(line) == want


@pytest.mark.parametrize("line", [" 12", "12 x", "", "-1", "１２", "9223372036854775808", "1 9223372036854775808", "1 2 3",
                                  "1.5", "12 ٣"])
def test_parse_input_errors(pkg, mains, line):
    with pytest.raises(pkg.IllegalArgumentException, match="Failed to parse input: "):
        mains.parse_input(line)


def test_calc_recommender_target(mains):
    persons = {"id": np.array([60_040, 60_041, 60_050]), "home_region_id": np.array([0, 0, 2], np.int32)}
    assert mains.calc_recommender_target(persons, (60_041, 1)) == (60_041, 0, 1)
    assert mains.calc_recommender_target(persons, (60_050, None)) == (60_050, 2, 2)
    assert mains.calc_recommender_target(persons, mains.parse_input("60040 2")) == (60_040, 0, 2)
    with pytest.raises(mains.NoSuchElementException, match="^Person not found: 7$"):
        mains.calc_recommender_target(persons, (7, 1))
    assert isinstance(mains.NoSuchElementException("x"), LookupError)


def test_load_persons_reads_what_the_generator_writes(mains, tmp_path):
    import pyarrow as pa
    table = pa.table([pa.array([60_040, 60_041], pa.int64()), pa.array([0, 2], pa.int32())], names=["id", "home_region_id"])
    mains._write_dir(str(tmp_path / "persons_sample"), table)
    got = mains.load_persons(str(tmp_path))
    assert got["id"].tolist() == [60_040, 60_041] and got["home_region_id"].tolist() == [0, 2]
    assert got["home_region_id"].dtype == np.int64


# ---- the restatement ----------------------------------------------------------------------------------------------------

def test_id_scheme_on_the_shipped_numbers(pkg):
    d = sc.defaults()
    assert len(d["categories"]) == 20 and d["place_count"] == 30_000 and d["person_count"] == 3_000_000
    assert sc.id_scheme(len(d["categories"]), d["place_count"]) == (0, 40, 60_040)
    assert pkg.sample.id_scheme(len(d["categories"]), d["place_count"]) == (0, 40, 60_040)
    for year in (1969, 2018, 2020, 2100):
        assert pkg.sample.year_interval(year) == sc.year_interval(year)
    assert sc.year_interval(2018) == (1_514_764_800_000, 8736, 365)


def test_persons_drop_the_remainder_and_use_the_region_id(pkg):
    regions = sc.defaults()["regions"]
    p = sc.persons(regions, 10, 60_040)
    assert len(p["id"]) == 9 and p["id"].tolist() == list(range(60_040, 60_049)) and p["home_region_id"].tolist() == [0] * 3 + [1] * 3 + [2] * 3
    gaps = [(0, "a", 0, 1, 0, 1), (5, "b", 0, 1, 0, 1), (2, "c", 0, 1, 0, 1)]
    q = sc.persons(gaps, 7, 100)
    assert q["id"].tolist() == [100, 101, 110, 111, 104, 105] and q["home_region_id"].tolist() == [0, 0, 5, 5, 2, 2]
    assert len(sc.persons(regions, 2, 60_040)["id"]) == 0


def test_grid_side():
    assert sc.grid_side(30_000, 3) == 100 and sc.grid_side(29_997, 3) == 99
    assert sc.grid_side(3, 3) == 1 and sc.grid_side(2, 3) == 0 and sc.grid_side(300, 3) == 10


def test_places_grid(pkg):
    d = sc.defaults()
    pl = sc.places(d["regions"], 300, 40, 20)
    assert len(pl["id"]) == 300 and len(np.unique(pl["id"])) == 300 and pl["id"].min() == 40 and pl["id"].max() == 339
    assert pl["category_id"].min() >= 0 and pl["category_id"].max() < 20 and len(np.unique(pl["category_id"])) > 10
    for r in d["regions"]:
        m = pl["region_id"] == r[0]
        lat, lon = pl["latitude"][m], pl["longitude"][m]
        assert lat.min() > r[2] and lon.min() > r[4]                            # the indices run from 1: no place on the min edge
        assert abs(lat.max() - r[3]) < 1e-9 and abs(lon.max() - r[5]) < 1e-9
        assert np.all(np.diff(lat.reshape(10, 10), axis=1) == 0)                # the latitude index is the outer loop
    assert sc.place_names(pl["id"][:1], pl["category_id"][:1], d["categories"]) == [f"{d['categories'][pl['category_id'][0]]}-40"]
    assert len(sc.places(d["regions"], 2, 40, 20)["id"]) == 0


def test_counts_reach_both_ends():
    counts = sc.visit_counts(999, 365)
    assert counts.min() == 1 and counts.max() == 365 and int(counts.sum()) == 182_131


def test_every_timestamp_of_2018_lies_before_december_31st():
    d = sc.defaults()
    from_ms, hours, days = sc.year_interval(2018)
    p = sc.persons(d["regions"], 999, 60_040)
    for shared in (True, False):
        v = sc.location_visits(p, d["regions"], from_ms, hours, days, shared_factor=shared)
        assert len(v["timestamp"]) == 182_131
        first = np.datetime64("2018-01-01T00:00", "ms").astype(np.int64)
        last = np.datetime64("2018-12-30T23:00", "ms").astype(np.int64)
        assert v["timestamp"].min() >= first and v["timestamp"].max() <= last
        assert np.all(v["timestamp"] % sc.MS_PER_HOUR == 0)
        assert set(np.unique(v["year_month"]).tolist()) == set(range(201801, 201813))
        by_id = {r[0]: r for r in d["regions"]}
        for rid in (0, 1, 2):
            m = v["region_id"] == rid
            assert v["latitude"][m].min() >= by_id[rid][2] and v["latitude"][m].max() <= by_id[rid][3]
            assert v["longitude"][m].min() >= by_id[rid][4] and v["longitude"][m].max() <= by_id[rid][5]
    assert np.array_equal(np.repeat(p["id"], sc.visit_counts(999, 365)), v["person_id"])


@pytest.mark.parametrize("year", [1969, 2018, 2020, 2100])
def test_year_month_is_numpys_calendar(year):
    from_ms, hours, days = sc.year_interval(year)
    assert days == (366 if year == 2020 else 365)
    ts = from_ms + np.arange(0, hours + 1, dtype=np.int64) * sc.MS_PER_HOUR          # every hour the generator can draw
    months = ts.astype("datetime64[ms]").astype("datetime64[M]")
    want = np.array([int(str(m).replace("-", "")) for m in np.unique(months)])
    got = sc.year_month(ts)
    assert np.array_equal(np.unique(got), want) and want[0] == year * 100 + 1 and want[-1] == year * 100 + 12
    assert np.array_equal(got, np.array([int(str(m).replace("-", "")) for m in months.astype(str)], np.int32))
    if year == 2020:
        assert np.any(ts.astype("datetime64[ms]").astype("datetime64[D]") == np.datetime64("2020-02-29"))
    assert sc.year_month(np.array([-1, 0, -sc.MS_PER_DAY * 31 - 1])).tolist() == [196912, 197001, 196911]


def test_a_shard_reproduces_the_rows_of_the_whole():
    d = sc.defaults()
    from_ms, hours, days = sc.year_interval(2018)
    p = sc.persons(d["regions"], 300, 60_040)
    whole = sc.location_visits(p, d["regions"], from_ms, hours, days, seed=3, shared_factor=False)
    a = sc.location_visits({k: v[:120] for k, v in p.items()}, d["regions"], from_ms, hours, days, seed=3, shared_factor=False)
    b = sc.location_visits({k: v[120:] for k, v in p.items()}, d["regions"], from_ms, hours, days, seed=3, shared_factor=False,
                           person_index_base=120)
    for k in whole:
        assert sc.same_bits(whole[k], np.concatenate([a[k], b[k]])), k
