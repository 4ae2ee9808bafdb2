"""GPU checks of the sample generator (csrc/sample.hip, sample.py, mains.sample_generator_main) and of the request line
of the recommender mains, against the numpy restatement of tests/sample_cases.py.  Every comparison is exact: integers
with array_equal, doubles by their bit patterns (the arithmetic is integer draws plus single IEEE operations)."""
import functools
import os

import numpy as np
import pytest
import torch

import sample_cases as sc

pytestmark = pytest.mark.gpu
D = sc.defaults()
REGIONS, CATEGORIES = D["regions"], D["categories"]
MIN_PERSON_ID = sc.id_scheme(len(CATEGORIES), D["place_count"])[2]


@pytest.fixture(scope="module")
def sample(pkg):
    return pkg.sample


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def dev_table(table):
    return {k: dev(v) for k, v in table.items()}


def assert_same_table(got, want, columns, what=None):
    for k in columns:
        g = host(got[k])
        assert sc.same_bits(g, want[k]), (what, k, g.dtype, len(g), len(want[k]))


@functools.lru_cache(maxsize=None)
def want_persons(n):
    return sc.persons(REGIONS, n * len(REGIONS), MIN_PERSON_ID)     # n persons a region


@functools.lru_cache(maxsize=None)
def want_visits(n_persons, shared, seed=0, year=2018):
    """The restatement's visits of the first n_persons persons of the 999 (computed once per shape, never changed)."""
    p = {k: v[:n_persons] for k, v in persons_999().items()}
    return sc.location_visits(p, REGIONS, *sc.year_interval(year), seed=seed, shared_factor=shared)


def persons_999():
    return want_persons(333)


def first_persons(n, on_device):
    p = {k: v[:n] for k, v in persons_999().items()}
    return dev_table(p) if on_device else p


# ---- persons ------------------------------------------------------------------------------------------------------------

GAPS = [(0, "a", 10.0, 11.0, 20.0, 21.0), (5, "b", -11.0, -10.0, -21.0, -20.0), (2, "c", 0.0, 0.5, 0.0, 0.5)]


@pytest.mark.parametrize("regions", [REGIONS, GAPS], ids=["ids012", "ids052"])
@pytest.mark.parametrize("person_count", [0, 2, 10, 3000])
@pytest.mark.parametrize("on_device", [False, True])
def test_persons(sample, regions, person_count, on_device):
    got = sample.generate_persons(regions, person_count, MIN_PERSON_ID, device=on_device)
    want = sc.persons(regions, person_count, MIN_PERSON_ID)
    assert torch.is_tensor(got["id"]) == on_device
    assert len(want["id"]) == (person_count // 3) * 3
    assert_same_table(got, want, ("id", "home_region_id"))


# ---- location visits ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_persons", [1, 63, 64, 65, 255, 256, 257, 999])
@pytest.mark.parametrize("shared", [True, False])
def test_visits(sample, n_persons, shared):
    want = want_visits(n_persons, shared)
    on_device = n_persons % 2 == 1                          # both memory forms over the sizes
    got = sample.generate_location_visits(first_persons(n_persons, on_device), REGIONS, *sc.year_interval(2018), shared_factor=shared)
    assert torch.is_tensor(got["person_id"]) == on_device
    assert_same_table(got, want, sample.VISIT_COLUMNS, (n_persons, shared))
    assert host(got["year_month"]).dtype == np.int32
    st = sample.location_visits_stats()
    assert st["rows"] == len(want["person_id"]) and st["bytes"] == 44 * st["rows"] and st["fill_ms"] > 0 and st["count_ms"] > 0


def test_visits_of_999_persons_reach_both_counts(sample):
    counts = sc.visit_counts(999, 365)
    assert counts.min() == 1 and counts.max() == 365 and counts.sum() == 182_131
    got = sample.generate_location_visits(first_persons(999, True), REGIONS, *sc.year_interval(2018))
    per_person = torch.unique_consecutive(got["person_id"], return_counts=True)[1].cpu().numpy()
    assert np.array_equal(per_person, counts)


def test_shared_factor_is_one_draw(sample):
    """On the device columns: with the shared factor a row's latitude and longitude fractions are the same number (so
    is the time fraction: its hour is floor(8736 * the latitude's factor)); without it they differ."""
    p = first_persons(999, True)
    box = {r[0]: r[2:6] for r in REGIONS}
    from_ms, hours, days = sc.year_interval(2018)
    tables = {s: sample.generate_location_visits(p, REGIONS, from_ms, hours, days, shared_factor=s) for s in (True, False)}
    g = want_visits(999, True)
    # the factor itself, recovered from the restatement's keying; the device's coordinates are min + span * factor
    row = np.repeat(np.arange(999), sc.visit_counts(999, 365))
    k = np.arange(len(row)) - np.repeat(np.cumsum(sc.visit_counts(999, 365)) - sc.visit_counts(999, 365), sc.visit_counts(999, 365))
    f = sc.u01(0, sc.STREAM_VISIT, row, 3 * k)
    b = np.array([box[int(h)] for h in g["region_id"]])
    shared = {k_: host(v) for k_, v in tables[True].items()}
    assert sc.same_bits(shared["latitude"], b[:, 0] + (b[:, 1] - b[:, 0]) * f)
    assert sc.same_bits(shared["longitude"], b[:, 2] + (b[:, 3] - b[:, 2]) * f)
    assert np.array_equal(shared["timestamp"], from_ms + (hours * f).astype(np.int64) * sc.MS_PER_HOUR)
    free = {k_: host(v) for k_, v in tables[False].items()}
    assert sc.same_bits(free["latitude"], shared["latitude"])                   # slot 3k is the latitude's in both
    assert not np.array_equal(free["longitude"], shared["longitude"])
    assert not np.array_equal(free["timestamp"], shared["timestamp"])
    lat_frac = (free["latitude"] - b[:, 0]) / (b[:, 1] - b[:, 0])
    lon_frac = (free["longitude"] - b[:, 2]) / (b[:, 3] - b[:, 2])
    assert np.mean(np.abs(lat_frac - lon_frac) > 1e-6) > 0.99


@pytest.mark.parametrize("on_device", [False, True])
def test_person_index_base(sample, on_device):
    want = want_visits(999, False)
    p = first_persons(999, on_device)
    iv = sc.year_interval(2018)
    a = sample.generate_location_visits({k: v[:400] for k, v in p.items()}, REGIONS, *iv, shared_factor=False)
    b = sample.generate_location_visits({k: v[400:] for k, v in p.items()}, REGIONS, *iv, shared_factor=False, person_index_base=400)
    for k in sample.VISIT_COLUMNS:
        assert sc.same_bits(np.concatenate([host(a[k]), host(b[k])]), want[k]), k
    c = sample.generate_location_visits({k: v[400:] for k, v in p.items()}, REGIONS, *iv, shared_factor=False)   # base 0: other rows
    assert not sc.same_bits(host(c["latitude"]), host(b["latitude"]))


def test_seeds(sample):
    p = first_persons(257, True)
    iv = sc.year_interval(2018)
    a = sample.generate_location_visits(p, REGIONS, *iv, seed=0)
    b = sample.generate_location_visits(p, REGIONS, *iv, seed=0)
    c = sample.generate_location_visits(p, REGIONS, *iv, seed=2 ** 64 - 1)
    for k in sample.VISIT_COLUMNS:
        assert torch.equal(a[k], b[k]), k
    want = sc.location_visits({k: v[:257] for k, v in persons_999().items()}, REGIONS, *iv, seed=2 ** 64 - 1)
    assert_same_table(c, want, sample.VISIT_COLUMNS)
    assert len(c["person_id"]) != len(a["person_id"]) or not torch.equal(c["latitude"], a["latitude"])


@pytest.mark.parametrize("on_device", [False, True])
def test_visits_capacity_protocol(sample, on_device):
    want = want_visits(999, True)
    total = len(want["person_id"])
    p = first_persons(999, on_device)
    iv = sc.year_interval(2018)
    assert sample.location_visits_count(p, REGIONS, *iv) == total == 182_131          # capacity 0 sizes the buffers
    for cap in (total - 1, total, total + 5, 1, 365):
        got = sample.generate_location_visits(p, REGIONS, *iv, capacity=cap)
        m = min(cap, total)
        assert sample.location_visits_stats()["rows"] == m
        assert_same_table(got, {k: v[:m] for k, v in want.items()}, sample.VISIT_COLUMNS, cap)


def test_visits_capacity_writes_nothing_beyond_it(pkg, sample):
    """Through the C ABI: a capacity of total - 1 leaves the entry after it untouched, and reports the full count."""
    import ctypes as C
    from locations_recommender_amd import _lib as L
    want = want_visits(999, True)
    total = len(want["person_id"])
    p = first_persons(999, True)
    c = pkg.prep._Cols(p["id"], p["home_region_id"])
    args, keep = sample._visit_args(c, p, REGIONS, *sc.year_interval(2018), 0, True, 0)
    outs = [torch.full((total,), -7, dtype=getattr(torch, np.dtype(dt).name), device="cuda") for dt in sample._VISIT_DTYPES]
    torch.cuda.synchronize()
    cnt = C.c_int64(total - 1)
    L.check(pkg.lib().locrec_sample_location_visits(*args, *[C.c_void_p(o.data_ptr()) for o in outs], C.byref(cnt)))
    assert cnt.value == total
    for k, o in zip(sample.VISIT_COLUMNS, outs):
        assert sc.same_bits(host(o[:total - 1]), want[k][:total - 1]) and float(o[total - 1]) == -7.0, k


@pytest.mark.parametrize("year", [1969, 2020, 2100])
def test_years(sample, year):
    iv = sc.year_interval(year)
    want = want_visits(999, False, year=year)
    got = sample.generate_location_visits(first_persons(999, True), REGIONS, *iv, shared_factor=False)
    assert_same_table(got, want, sample.VISIT_COLUMNS, year)
    ym = host(got["year_month"])
    assert ym.min() == year * 100 + 1 and ym.max() == year * 100 + 12
    per_person = torch.unique_consecutive(got["person_id"], return_counts=True)[1]
    assert int(per_person.max()) == iv[2]
    if year == 2020:
        assert iv[2] == 366
        days = host(got["timestamp"]).astype("datetime64[ms]").astype("datetime64[D]")
        assert np.any(days == np.datetime64("2020-02-29")) and not np.any(days == np.datetime64("2020-12-31"))


@pytest.mark.parametrize("on_device", [False, True])
def test_home_region_that_is_not_listed(pkg, sample, on_device):
    p = {k: v[:300].copy() for k, v in persons_999().items()}
    p["home_region_id"][[77, 200]] = 9
    with pytest.raises(pkg.IllegalArgumentException, match="person row 77: home region 9 "):
        sample.generate_location_visits(dev_table(p) if on_device else p, REGIONS, *sc.year_interval(2018))
    with pytest.raises(pkg.IllegalArgumentException, match="person row 77"):
        sample.location_visits_count(dev_table(p) if on_device else p, REGIONS, *sc.year_interval(2018))


def test_count_beyond_2_to_the_31(sample):
    """12,000,000 persons: 2,195,981,371 rows (the restatement's sum, computed in chunks), counted without allocating
    them - the offsets are 64-bit."""
    n = 12_000_000
    want = sum(int(sc.visit_counts(2_000_000, 365, 0, base).sum()) for base in range(0, n, 2_000_000))
    assert want == 2_195_981_371 > 2 ** 31
    ids = torch.arange(MIN_PERSON_ID, MIN_PERSON_ID + n, dtype=torch.int64, device="cuda")
    home = torch.arange(n, dtype=torch.int64, device="cuda") % 3
    assert sample.location_visits_count({"id": ids, "home_region_id": home}, REGIONS, *sc.year_interval(2018)) == want


# ---- places ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("place_count, side", [(0, 0), (2, 0), (3, 1), (300, 10), (30_000, 100), (29_997, 99)])
@pytest.mark.parametrize("on_device", [False, True])
def test_places(sample, place_count, side, on_device):
    assert sc.grid_side(place_count, 3) == side
    want = sc.places(REGIONS, place_count, 40, len(CATEGORIES))
    got = sample.generate_places(REGIONS, place_count, 40, len(CATEGORIES), device=on_device)
    assert torch.is_tensor(got["id"]) == on_device and len(want["id"]) == 3 * side * side
    assert_same_table(got, want, sample.PLACE_COLUMNS, place_count)
    ids, cats = host(got["id"]), host(got["category_id"])
    assert len(np.unique(ids)) == len(ids)
    assert len(cats) == 0 or (cats.min() >= 0 and cats.max() < len(CATEGORIES))


def test_places_of_regions_with_gaps_and_other_ids(sample):
    want = sc.places(GAPS, 77, 1000, 7, min_category_id=50, seed=9)
    got = sample.generate_places(GAPS, 77, 1000, 7, min_category_id=50, seed=9, device=True)
    assert len(want["id"]) == 75 and want["category_id"].min() >= 50 and want["category_id"].max() < 57
    assert_same_table(got, want, sample.PLACE_COLUMNS)
    assert host(got["id"])[25] == 1000 + 5 * 25


# ---- names ----------------------------------------------------------------------------------------------------------------

NAME_CATEGORIES = ["cafe", "", "театр", "a\U00010400b", "gas_station"]


def name_case(min_place_id):
    ids = np.array([9, 10, 99, 100, 40, 0, 12345, 7], np.int64) + min_place_id
    cats = np.array([0, 1, 2, 3, 4, 2, 0, 3], np.int64)
    return ids, cats


@pytest.mark.parametrize("min_place_id", [0, 10 ** 18, 2 ** 63 - 1 - 12345], ids=["small", "19digits", "long_max"])
@pytest.mark.parametrize("on_device", [False, True])
def test_names(pkg, sample, min_place_id, on_device):
    ids, cats = name_case(min_place_id)
    strings = sc.place_names(ids, cats + 3, NAME_CATEGORIES, 3)
    assert strings[0] == f"cafe-{9 + min_place_id}" and strings[1] == f"-{10 + min_place_id}" and strings[2].startswith("театр-")
    if min_place_id == 10 ** 18:
        assert all(len(str(int(i))) == 19 for i in ids)
    want_off, want_units = pkg.deduplicator.encode_names(strings, lower=False)
    x = (dev(ids), dev(cats + 3)) if on_device else (ids, cats + 3)
    off, units = sample.place_names(*x, NAME_CATEGORIES, min_category_id=3)
    assert torch.is_tensor(off) == on_device
    assert np.array_equal(host(off), want_off) and host(off).dtype == np.int64
    assert np.array_equal(host(units).view(np.uint16), want_units)
    assert sample.decode_names(off, units) == strings
    total = len(want_units)                                     # the unit-capacity protocol
    for cap in (total - 1, 1, total + 3):
        off2, units2 = sample.place_names(*x, NAME_CATEGORIES, min_category_id=3, capacity=cap)
        assert np.array_equal(host(off2), want_off)
        assert np.array_equal(host(units2).view(np.uint16), want_units[:min(cap, total)])


def test_names_of_generated_places_and_of_none(pkg, sample):
    pl = sample.generate_places(REGIONS, 300, 40, len(CATEGORIES), device=True)
    off, units = sample.place_names(pl["id"], pl["category_id"], CATEGORIES)
    strings = sc.place_names(host(pl["id"]), host(pl["category_id"]), CATEGORIES)
    want_off, want_units = pkg.deduplicator.encode_names(strings, lower=False)
    assert np.array_equal(host(off), want_off) and np.array_equal(host(units).view(np.uint16), want_units)
    off0, units0 = sample.place_names(np.empty(0, np.int64), np.empty(0, np.int64), CATEGORIES)
    assert off0.tolist() == [0] and len(units0) == 0


def test_names_refuse_a_bad_row(pkg, sample):
    with pytest.raises(pkg.IllegalArgumentException, match="place row 2"):
        sample.place_names(np.array([1, 2, -3, -4]), np.array([0, 0, 0, 0]), CATEGORIES)
    with pytest.raises(pkg.IllegalArgumentException, match="place row 1"):
        sample.place_names(np.array([1, 2, 3]), np.array([0, 20, 0]), CATEGORIES)


# ---- through the chain ------------------------------------------------------------------------------------------------------

def test_the_whole_walk_through(pkg, sample, oracle, tmp_path):
    """sample_generator_main -> both builder mains -> one request line of both recommender mains, on 300 persons and 300
    places of the reference's regions (chosen on the CPU: the restatement joined by the oracle has place visits in every
    region, asserted below)."""
    import pyarrow.parquet as pq
    from locations_recommender_amd import mains
    prep = pkg.prep
    d = str(tmp_path)
    n_persons = n_places = 300
    want = sc.generate(n_places, n_persons, REGIONS, CATEGORIES)
    vrows, _ = oracle.place_visits(want["location_visits"], want["places"], int(want["location_visits"]["timestamp"].min()))
    per_region = np.bincount(want["location_visits"]["region_id"][vrows], minlength=3)
    assert len(per_region) == 3 and per_region.min() >= 1, per_region

    t = mains.sample_generator_main(d, n_places, n_persons, REGIONS, CATEGORIES)
    assert all(torch.is_tensor(t[k][c]) for k, c in (("persons", "id"), ("location_visits", "latitude"), ("places", "id")))
    assert_same_table(t["persons"], want["persons"], ("id", "home_region_id"))
    assert_same_table(t["location_visits"], want["location_visits"], sample.VISIT_COLUMNS)
    assert_same_table(t["places"], want["places"], sample.PLACE_COLUMNS)
    assert sample.decode_names(t["places"]["name_offsets"], t["places"]["name_units"]) == want["names"]

    # the files, read back through the builders' loaders, are the returned tables
    file_visits, file_places = mains.load_location_visits(d), mains.load_places_full(d)
    assert_same_table(file_visits, {k: host(v) for k, v in t["location_visits"].items()},
                      ("person_id", "timestamp", "latitude", "longitude", "region_id"))
    assert_same_table(file_places, {k: host(v) for k, v in t["places"].items()}, sample.PLACE_COLUMNS)
    raw = pq.read_table(os.path.join(d, "location_visits_sample")).to_pydict()
    assert raw["year_month"] == [f"{v:06d}" for v in want["location_visits"]["year_month"].tolist()]
    schema = pq.read_schema(os.path.join(d, "location_visits_sample", "part-00000.parquet"))
    assert str(schema.field("timestamp").type) == "timestamp[ms]" and str(schema.field("region_id").type) == "int32"
    raw_places = pq.read_table(os.path.join(d, "places_sample")).to_pydict()
    assert raw_places["name"] == want["names"] and raw_places["description"] == want["names"]
    cats = pq.read_table(os.path.join(d, "categories_sample")).to_pydict()
    assert cats == {"category": CATEGORIES, "category_id": list(range(len(CATEGORIES)))}
    persons = mains.load_persons(d)
    assert_same_table(persons, want["persons"], ("id", "home_region_id"))

    # the device tables feed the join as they are
    visits_from = prep.visits_from_timestamp(prep.max_timestamp(t["location_visits"]["timestamp"]), 400)
    pv_dev = prep.calc_place_visits(t["location_visits"], t["places"], visits_from)
    pv_file = prep.calc_place_visits(file_visits, file_places, visits_from)
    assert len(pv_file["person_id"]) == len(vrows)
    for k in prep.PLACE_VISIT_COLUMNS:
        assert np.array_equal(host(pv_dev[k]), pv_file[k]), k
    assert np.array_equal(pv_file["person_id"], want["location_visits"]["person_id"][vrows])

    sets = prep.region_sets([0, 1, 2])
    assert mains.rating_vectors_builder_main(d, 400, 100, 10) == sets
    assert mains.stochastic_graph_builder_main(d, 400, 0.5, 0.5) == sets

    home_visitors = pv_file["person_id"][pv_file["region_id"] == 0]
    pid = int(home_visitors[0])
    places_of = mains.load_places(d)
    some_rows = 0
    for line, target in ((f"{pid} 1", 1), (f"{pid}", 0)):
        got = mains.knn_recommender_request(d, persons, line, 0.5, 0.5, 20, max_recommendations=7)
        ids, scores = mains.knn_make_recommendations(d, [0, target], pid, 0.5, 0.5, 20)
        by_hand = mains.rank_recommendations(ids, scores, *places_of, target, 7)
        assert got[0] == (pid, 0, target)
        assert np.array_equal(got[1], by_hand[0]) and sc.same_bits(np.asarray(got[2]), by_hand[1]), line
        got = mains.sg_recommender_request(d, persons, line, 0.01, 20, max_recommendations=7)
        ids, scores, _, _ = mains.sg_make_recommendations(d, [0, target], pid, 0.01, 20)
        by_hand = mains.rank_recommendations(ids, scores, *places_of, target, 7)
        assert got[0] == (pid, 0, target)
        assert np.array_equal(got[1], by_hand[0]) and sc.same_bits(np.asarray(got[2]), by_hand[1]), line
        assert np.all(np.isin(got[1], places_of[0][places_of[1] == target]))
        if target == 0:
            some_rows = len(got[1])
    assert some_rows > 0                                       # the person's own places carry probability
    for fn, args in ((mains.knn_recommender_request, (0.5, 0.5, 20)), (mains.sg_recommender_request, (0.01, 20))):
        with pytest.raises(mains.NoSuchElementException, match="^Person not found: 5$"):
            fn(d, persons, "5 1", *args)
        with pytest.raises(pkg.IllegalArgumentException, match="Failed to parse input"):
            fn(d, persons, "x", *args)
