"""The place deduplicator on the device (csrc/dedup.hip, locations-recommender_amd/deduplicator.py) against the
reference's known answers and the CPU restatement of tests/dedup_cases.py.  Every comparison is exact."""
import contextlib
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import dedup_cases as dc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LEV_THRESHOLDS = (0, 1, 3, 4, 7, 8, 15, 16, 40)


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


@contextlib.contextmanager
def switch(name, value):
    """An environment switch of the library for the calls inside (the library reads both of its switches per call)."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def to_device(cols):
    return {k: torch.as_tensor(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for k, v in cols.items()}


def to_host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def abi_columns(side):
    """A case's side as the C ABI takes it: names lower-cased, as CSR of UTF-16 code units."""
    off, units = dc.csr([s.lower() for s in side["name"]])
    return dict(id=side["id"], region_id=side["region_id"], latitude=side["latitude"], longitude=side["longitude"],
                name_offsets=off, name_units=units)


def frames(side, extra=False):
    import pandas as pd
    f = pd.DataFrame({"region_id": side["region_id"], "id": side["id"], "name": side["name"], "latitude": side["latitude"],
                      "longitude": side["longitude"]})
    if extra:
        f["category"] = np.arange(len(f)) % 7
    return f


_CASES = {}


def case(spec):
    """(places, confirmed, oracle distances of the in-region pairs), built once per process"""
    if spec not in _CASES:
        places, confirmed = dc.generated_case(*spec)
        _CASES[spec] = (places, confirmed, dc.pair_distances(places, confirmed))
    return _CASES[spec]


def assert_equals_restatement(got, want):
    prow, crow, diff, not_same = (to_host(x) for x in got)
    same, want_not_same = want
    assert np.array_equal(prow, np.array([s[0] for s in same], np.int64))
    assert np.array_equal(crow, np.array([s[1] for s in same], np.int64))
    assert np.array_equal(diff, np.array([s[2] for s in same], np.int32))
    assert np.array_equal(not_same, want_not_same)


# ---- known answers ----------------------------------------------------------------------------------------------------

def test_levenshtein_known_answers(pkg):
    d = pkg.deduplicator
    cases = load("levenshtein_kats.json")["cases"]
    a, b = dc.csr([c["str1"] for c in cases]), dc.csr([c["str2"] for c in cases])
    want = np.array([c["expected"] for c in cases], np.int32)
    assert want.tolist() == [3, 6, 7, 0, 0]
    assert np.array_equal(d.lev_distances(a[0], a[1], b[0], b[1]), want)
    assert [pkg.lev(c["str1"], c["str2"]) for c in cases] == want.tolist()
    for bad in ((None, "sitting"), ("sitting", None)):                  # LevenshteinTest.scala:34-44
        with pytest.raises(TypeError):
            pkg.lev(*bad)


def test_deduplicator_known_answer(pkg):
    kat = load("place_deduplicator_kat.json")

    def cols(rows):
        r = list(zip(*rows))
        return dict(region_id=np.array(r[0], np.int64), id=np.array(r[1], np.int64), name=list(r[2]),
                    latitude=np.array(r[3], np.float64), longitude=np.array(r[4], np.float64))
    places, confirmed = cols(kat["places"]), cols(kat["confirmed_places"])
    radius, k = kat["max_place_distance_meters"], kat["max_name_difference"]
    prow, crow, diff, not_same = pkg.deduplicator.find_duplicate_places(abi_columns(places), abi_columns(confirmed), radius, k)
    assert (prow.tolist(), crow.tolist(), diff.tolist(), not_same.tolist()) == ([0, 1], [0, 0], [3, 0], [0, 0, 1])
    dd = pkg.PlaceDeduplicator(maxPlaceDistanceMeters=radius, maxNameDifference=k)
    out = dd.dropDuplicates(frames(places), frames(confirmed))
    assert list(out.columns) == kat["columns"] and len(out) == 1
    assert out.iloc[0]["id"] == 103 and out.iloc[0]["name"] == "Biryulyovo Tovarnaya"
    assert out.values.tolist() == kat["expected_rows"]
    found = dd.findDuplicates(frames(places), frames(confirmed))
    assert list(found.columns) == ["id", "that_id", "name_difference"]
    assert found.values.tolist() == [[101, 1, 3], [102, 1, 0]]
    assert dd.withoutDuplicates(frames(places), frames(confirmed)).values.tolist() == kat["expected_rows"]


# ---- locrec_lev_distances ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def adversarial():
    pairs = dc.adversarial_strings()
    a, b = dc.csr([p[0] for p in pairs]), dc.csr([p[1] for p in pairs])
    exact = np.array([dc.lev_any(x, y) for x, y in pairs], np.int32)
    return a, b, exact


@pytest.mark.parametrize("mem", ("host", "device"))
def test_lev_distances_equal_the_restatement(pkg, adversarial, mem):
    d = pkg.deduplicator
    a, b, exact = adversarial
    args = (a[0], a[1], b[0], b[1])
    if mem == "device":
        args = tuple(torch.as_tensor(x.view(np.int16) if x.dtype == np.uint16 else x).cuda() for x in args)
    assert np.array_equal(to_host(d.lev_distances(*args)), exact)
    for k in LEV_THRESHOLDS:
        want = np.minimum(exact, k + 1)
        got = to_host(d.lev_distances(*args, max_difference=k))
        assert np.array_equal(got, want), (k, np.flatnonzero(got != want)[:5])
    with switch("LOCREC_DEDUP_FULL_DP", "1"):                           # the A/B partner gives the same numbers
        assert np.array_equal(to_host(d.lev_distances(*args)), exact)
        for k in LEV_THRESHOLDS:
            assert np.array_equal(to_host(d.lev_distances(*args, max_difference=k)), np.minimum(exact, k + 1)), k


def test_lev_distances_reject_offsets_that_are_no_csr(pkg):
    d = pkg.deduplicator
    units = np.arange(97, 101, dtype=np.uint16)
    good = np.array([0, 2, 4], np.int64)
    for bad in (np.array([0, 3, 2], np.int64), np.array([-1, 2, 4], np.int64)):
        with pytest.raises(pkg.IllegalArgumentException, match="never decrease"):
            d.lev_distances(bad, units, good, units)
        with pytest.raises(pkg.IllegalArgumentException, match="never decrease"):
            d.lev_distances(good, units, bad, units)


# ---- locrec_find_duplicate_places ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", ("host", "device"))
@pytest.mark.parametrize("spec", dc.CASES, ids=lambda c: "seed%d" % c[0])
def test_find_duplicates_equal_the_restatement(pkg, spec, mem):
    d = pkg.deduplicator
    places, confirmed, dist = case(spec)
    p, c = abi_columns(places), abi_columns(confirmed)
    if mem == "device":
        p, c = to_device(p), to_device(c)
    some_same = 0
    for radius in dc.RADII:
        for k in dc.NAME_DIFFERENCES:
            want = dc.drop_duplicates(places, confirmed, radius, k, dist)
            got = d.find_duplicate_places(p, c, radius, k)
            assert_equals_restatement(got, want)
            if radius < 0 or k < 0:
                assert not want[0]
            some_same += len(want[0])
    if len(dist) > 1000:
        assert some_same > 100


def test_switches_do_not_change_the_result(pkg):
    """The full-matrix A/B partner and a chunk budget that forces many chunks give what the default gives: the budget
    on every case and threshold tier, the full matrix on every case at the reference's parameters and on the smallest
    case everywhere (it is slow by design on the 5,000-unit names), and the two together."""
    d = pkg.deduplicator
    for spec in dc.CASES:
        places, confirmed, dist = case(spec)
        p, c = abi_columns(places), abi_columns(confirmed)
        small = len(places["id"]) <= 100
        for radius, k in ((60.0, 5), (5000.0, 2), (60.0, 20), (60.0, 0)):
            want = dc.drop_duplicates(places, confirmed, radius, k, dist)
            budget = 7 if small else 257                      # (hundreds of chunks on the large cases)
            with switch("LOCREC_DEDUP_PAIR_BUDGET", str(budget)):
                assert_equals_restatement(d.find_duplicate_places(p, c, radius, k), want)
                st = d.find_duplicate_places_stats()
                assert st["candidates"] <= budget or st["chunks"] > 1
                if small:
                    with switch("LOCREC_DEDUP_FULL_DP", "1"):
                        assert_equals_restatement(d.find_duplicate_places(p, c, radius, k), want)
            if small or (radius, k) == (60.0, 5):
                with switch("LOCREC_DEDUP_FULL_DP", "1"):
                    assert_equals_restatement(d.find_duplicate_places(p, c, radius, k), want)


@pytest.mark.parametrize("mem", ("host", "device"))
def test_capacity_protocol(pkg, mem):
    from locations_recommender_amd import _lib as L
    places, confirmed, dist = case(dc.CASES[0])
    same, not_same = dc.drop_duplicates(places, confirmed, 60.0, 5, dist)
    total = len(same)
    assert total > 10
    p, c = abi_columns(places), abi_columns(confirmed)
    keys = ("id", "region_id", "latitude", "longitude", "name_offsets", "name_units")
    if mem == "device":
        p, c = to_device(p), to_device(c)
        ptr = lambda a: C.c_void_p(a.data_ptr())                                      # noqa: E731
        new = lambda n, dt: torch.full((max(n, 1),), -7, dtype=getattr(torch, np.dtype(dt).name), device="cuda")   # noqa: E731
        memk = L.MEM_DEVICE
        torch.cuda.synchronize()
    else:
        ptr = lambda a: C.c_void_p(a.ctypes.data)                                     # noqa: E731
        new = lambda n, dt: np.full(max(n, 1), -7, dt)                                # noqa: E731
        memk = L.MEM_HOST
    pa, ca = [ptr(p[k]) for k in keys], [ptr(c[k]) for k in keys]
    fn = pkg.lib().locrec_find_duplicate_places
    for cap in (0, 1, total // 2, total, total + 5):
        op, oc, od, ns = new(cap + 2, np.int64), new(cap + 2, np.int64), new(cap + 2, np.int32), new(len(places["id"]), np.int64)
        cnt = C.c_int64(cap)
        outs = (None, None, None) if cap == 0 else (ptr(op), ptr(oc), ptr(od))
        L.check(fn(len(places["id"]), *pa, len(confirmed["id"]), *ca, 60.0, 5, memk, *outs, C.byref(cnt), ptr(ns)))
        assert cnt.value == total                                                     # the total, whatever the capacity
        m = min(cap, total)
        op, oc, od, ns = (to_host(x) for x in (op, oc, od, ns))
        assert [tuple(int(v) for v in t) for t in zip(op[:m], oc[:m], od[:m])] == same[:m]   # a prefix of the full result
        assert (op[m:] == -7).all() and (oc[m:] == -7).all() and (od[m:] == -7).all()   # nothing beyond the capacity
        assert np.array_equal(ns, not_same)


def test_bad_coordinates_fail_as_location_does(pkg):
    from locations_recommender_amd import _lib as L
    d = pkg.deduplicator
    places, confirmed, _ = case(dc.CASES[2])
    joined = set(places["region_id"].tolist()) & set(confirmed["region_id"].tolist())
    prow = int(np.flatnonzero(np.isin(places["region_id"], list(joined)))[3])
    crow = int(np.flatnonzero(np.isin(confirmed["region_id"], list(joined)))[1])
    keys = ("id", "region_id", "latitude", "longitude", "name_offsets", "name_units")

    def status(p, c):
        p, c = abi_columns(p), abi_columns(c)
        cnt = C.c_int64(0)
        st = pkg.lib().locrec_find_duplicate_places(len(p["id"]), *[C.c_void_p(p[k].ctypes.data) for k in keys], len(c["id"]),
                                                    *[C.c_void_p(c[k].ctypes.data) for k in keys], 60.0, 5, L.MEM_HOST,
                                                    None, None, None, C.byref(cnt), None)
        return st, cnt.value, pkg.lib().locrec_last_error().decode()

    def changed(side, row, key, value):
        out = {k: (v.copy() if isinstance(v, np.ndarray) else list(v)) for k, v in side.items()}
        out[key][row] = value
        return out
    st, cnt, msg = status(changed(places, prow, "latitude", 90.5), confirmed)
    assert (st, cnt) == (L.E_INVALID_ARG, -(1 + prow))
    assert msg == f"requirement failed: Latitude 90.5 must be within range [-90.0, 90.0] (place {prow})"
    st, cnt, msg = status(places, changed(confirmed, crow, "longitude", -180.25))
    assert (st, cnt) == (L.E_INVALID_ARG, -(1 + len(places["id"]) + crow))
    assert msg == f"requirement failed: Longitude -180.25 must be within range [-180.0, 180.0] (confirmed place {crow})"
    st, cnt, msg = status(changed(places, prow, "longitude", float("nan")), confirmed)
    assert (st, cnt) == (L.E_INVALID_ARG, -(1 + prow)) and "Longitude nan" in msg
    # a row whose region the other side lacks is never joined: no Location is made of it
    lonely = changed(changed(places, prow, "latitude", 90.5), prow, "region_id", 777)
    st, cnt, _ = status(lonely, confirmed)
    assert st == L.OK and cnt >= 0
    with pytest.raises(pkg.IllegalArgumentException, match="Latitude 90.5"):
        d.find_duplicate_places(abi_columns(changed(places, prow, "latitude", 90.5)), abi_columns(confirmed), 60.0, 5)


def test_identical_coordinates_are_zero_metres_apart(pkg):
    """Outside the generated cases (their margin condition excludes a pair AT a radius): for identical coordinates every
    term of the haversine is exactly 0 on any IEEE machine, so a radius of 0 keeps exactly these pairs."""
    d = pkg.deduplicator
    lat, lon = np.array([55.75, -89.5, 0.0, 10.0]), np.array([37.6, 180.0, 0.0, -20.0])
    conf = dict(region_id=np.zeros(4, np.int64), id=np.arange(4), name=["a", "b", "c", "d"], latitude=lat, longitude=lon)
    places = dict(region_id=np.zeros(4, np.int64), id=10 + np.arange(4), name=["a", "bb", "c", "x"],
                  latitude=lat.copy(), longitude=np.array([37.6, 180.0, 1e-7, -20.0]))
    prow, crow, diff, not_same = d.find_duplicate_places(abi_columns(places), abi_columns(conf), 0.0, 1)
    assert (prow.tolist(), crow.tolist(), diff.tolist(), not_same.tolist()) == ([0, 1, 3], [0, 1, 3], [0, 1, 1], [3, 3, 4, 3])


# ---- the mirror -------------------------------------------------------------------------------------------------------------

def test_mirror_equals_the_restatement(pkg):
    for spec in dc.CASES[:3]:
        places, confirmed, dist = case(spec)
        pf, cf = frames(places, extra=True), frames(confirmed)
        for radius, k in ((60.0, 5), (5000.0, 2)):
            same, not_same = dc.drop_duplicates(places, confirmed, radius, k, dist)
            dd = pkg.PlaceDeduplicator(radius, k)
            got = dd.dropDuplicates(pf, cf)
            want = pf.iloc[np.repeat(np.arange(len(pf)), not_same)].reset_index(drop=True)
            assert list(got.columns) == list(pf.columns) and got.equals(want)
            anti = np.ones(len(pf), bool)
            anti[[s[0] for s in same]] = False
            assert dd.withoutDuplicates(pf, cf).equals(pf.iloc[np.flatnonzero(anti)].reset_index(drop=True))
            found = dd.findDuplicates(pf, cf)
            assert found["id"].tolist() == [int(places["id"][s[0]]) for s in same]
            assert found["that_id"].tolist() == [int(confirmed["id"][s[1]]) for s in same]
            assert found["name_difference"].tolist() == [s[2] for s in same]


def test_mirror_null_name(pkg):
    places, confirmed, _ = case(dc.CASES[2])
    pf, cf = frames(places).astype({"name": object}), frames(confirmed)
    joined = np.flatnonzero(np.isin(places["region_id"], confirmed["region_id"]))
    lonely = np.flatnonzero(~np.isin(places["region_id"], confirmed["region_id"]))
    dd = pkg.PlaceDeduplicator(60, 5)
    if len(lonely):
        ok = pf.copy()
        ok.loc[int(lonely[0]), "name"] = None                           # never joined: the UDF never sees it
        dd.dropDuplicates(ok, cf)
    bad = pf.copy()
    bad.loc[int(joined[2]), "name"] = None
    with pytest.raises(TypeError, match=f"places row {int(joined[2])}"):
        dd.dropDuplicates(bad, cf)


# ---- scale ------------------------------------------------------------------------------------------------------------------

def haversine_numpy(lat1, lon1, lat2, lon2):
    p1, p2 = np.radians(lat1), np.radians(lat2)
    h = np.sin((p2 - p1) / 2) ** 2 + np.cos(p1) * np.cos(p2) * np.sin(np.radians(lon2 - lon1) / 2) ** 2
    return 2 * dc.EARTH_RADIUS_METERS * np.arcsin(np.sqrt(h))


def names_of(cols, rows):
    off, units = cols["name_offsets"], cols["name_units"]
    return [units[off[r]:off[r + 1]].tobytes().decode("utf-16-le") for r in rows]


def test_quarter_size_perf_case(pkg):
    """tools/perf_dedup.py's case at a quarter of its size: every output of 500 sampled places against the restatement
    restricted to them, the totals' bookkeeping, and the device memory given back."""
    from locations_recommender_amd import _lib as L
    spec = importlib.util.spec_from_file_location("perf_dedup", os.path.join(ROOT, "tools", "perf_dedup.py"))
    perf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(perf)
    d = pkg.deduplicator
    places, confirmed = perf.perf_case(250_000, 50_000)
    radius, k = perf.RADIUS_METERS, perf.NAME_DIFFERENCE
    p, c = to_device(places), to_device(confirmed)
    torch.cuda.synchronize()
    before = L.device_bytes_in_use()
    prow, crow, diff, not_same = (to_host(x) for x in d.find_duplicate_places(p, c, radius, k))
    assert L.device_bytes_in_use() == before
    st = d.find_duplicate_places_stats()
    assert st["same"] == len(prow) and st["candidates"] >= len(prow) > 20_000
    assert (np.diff(prow) >= 0).all() and ((np.diff(prow) > 0) | (np.diff(crow) > 0)).all()      # (place row, confirmed row) order
    # partners of every place with numpy: confirmed rows of its region, minus those with its id
    regions, per_region = np.unique(confirmed["region_id"], return_counts=True)
    at = np.searchsorted(regions, places["region_id"])
    partners = np.where((at < len(regions)) & (regions[np.minimum(at, len(regions) - 1)] == places["region_id"]),
                        per_region[np.minimum(at, len(regions) - 1)], 0)
    assert not np.isin(places["id"], confirmed["id"]).any()                                         # (this case shares no id)
    assert (not_same >= 0).all() and partners.sum() - not_same.sum() == len(prow)
    assert np.array_equal(partners - not_same, np.bincount(prow, minlength=len(partners)))
    # 500 places against the restatement: the confirmed places a numpy haversine puts within radius + 1 m go to the
    # literal loop with the oracle's distance (numpy and libm agree far better than 1 m); the others are too far
    sample = np.sort(np.random.default_rng(5).choice(len(partners), 500, replace=False))
    want_rows = []
    closest = np.inf
    for i in sample:
        near = np.flatnonzero((confirmed["region_id"] == places["region_id"][i]) &
                              (haversine_numpy(places["latitude"][i], places["longitude"][i], confirmed["latitude"],
                                               confirmed["longitude"]) <= radius + 1.0))
        one = dict(region_id=places["region_id"][[i]], id=places["id"][[i]], name=names_of(places, [i]),
                   latitude=places["latitude"][[i]], longitude=places["longitude"][[i]])
        some = dict(region_id=confirmed["region_id"][near], id=confirmed["id"][near], name=names_of(confirmed, near),
                    latitude=confirmed["latitude"][near], longitude=confirmed["longitude"][near])
        dist = dc.pair_distances(one, some)
        closest = min(closest, dc.min_margin(dist, (radius,)))
        same, _ = dc.drop_duplicates(one, some, radius, k, dist)
        want_rows += [(int(i), int(near[j]), diff_) for _, j, diff_ in same]
    assert closest > dc.MARGIN_METERS, "a sampled pair lies at the radius: sample other places"
    pick = np.isin(prow, sample)
    got_rows = [tuple(int(v) for v in t) for t in zip(prow[pick], crow[pick], diff[pick])]
    assert got_rows == want_rows and len(want_rows) > 50
    want_same = np.bincount([r[0] for r in want_rows], minlength=len(partners))[sample]
    assert np.array_equal(not_same[sample], partners[sample] - want_same)


# ---- one grid walk, two consumers -----------------------------------------------------------------------------------------

WALK_RADIUS = 60.0
WALK_SEED = 13   # the first seed whose case meets check_grid_walk_case with five matches across the antimeridian


def grid_walk_case(seed=WALK_SEED):
    """About 200 points and 60 anchors with disjoint ids in three regions, every point 0 - 120 m from an anchor of its
    region.  The regions sit on the walk's edges (csrc/place_grid.h): anchors on both sides of the antimeridian, anchors
    in the single-cell band at the pole, and mid-latitude anchors on both sides of a band boundary of the 60 m grid."""
    rng = np.random.default_rng(seed)
    band_deg = WALK_RADIUS / dc.EARTH_RADIUS_METERS * (180.0 / np.pi) * (1.0 + 1e-9) + 1e-12   # make_grid(60).band_deg
    boundary = -90.0 + np.floor((55.75 + 90.0) / band_deg) * band_deg
    k = np.arange(20)
    a_lat = np.concatenate([-17.0 + (k // 2) * 0.0007, np.full(20, 89.9995), boundary + np.where(k % 2 == 0, 9e-5, -9e-5)])
    a_lon = np.concatenate([np.where(k % 2 == 0, 179.9995, -179.9995), -180.0 + 18.0 * k, 37.6 + (k // 2) * 0.0012])
    a_region = np.repeat(np.array([-7, 3, 2 ** 40], np.int64), 20)
    n = 201
    near = np.arange(n) % 60
    p_lat, p_lon = np.empty(n), np.empty(n)
    for i in range(n):
        p_lat[i], p_lon[i] = dc.destination(a_lat[near[i]], a_lon[near[i]], rng.uniform(0, 2 * np.pi), rng.uniform(0, 120.0))
    points = dict(id=1000 + np.arange(n, dtype=np.int64), region_id=a_region[near], latitude=p_lat, longitude=p_lon)
    anchors = dict(id=1 + np.arange(60, dtype=np.int64), region_id=a_region, latitude=a_lat, longitude=a_lon)
    return points, anchors, boundary


def grid_walk_brute_force(points, anchors):
    """-> (the (point id, anchor id) pairs within the radius in (point row, anchor row) order, the distances of all
    in-region pairs [n_points, n_anchors] with NaN elsewhere)"""
    d = haversine_numpy(points["latitude"][:, None], points["longitude"][:, None], anchors["latitude"][None, :],
                        anchors["longitude"][None, :])
    d = np.where(points["region_id"][:, None] == anchors["region_id"][None, :], d, np.nan)
    rows, cols = np.nonzero(d <= WALK_RADIUS)
    return list(zip(points["id"][rows].tolist(), anchors["id"][cols].tolist())), d


def check_grid_walk_case(points, anchors, boundary):
    """The input condition (no decision within 1e-3 m of the radius: DESIGN.md section 2 allows device and libm distances
    to differ in the last ulps only) and that the case does reach the walk's edges.  Needs no GPU."""
    want, d = grid_walk_brute_force(points, anchors)
    assert np.nanmin(np.abs(d - WALK_RADIUS)) > 1e-3
    assert len(points["id"]) >= 200 and len(anchors["id"]) == 60 and not set(points["id"]) & set(anchors["id"])
    assert np.nanmax(np.nanmin(d, axis=1)) <= 120.0 and len(want) > len(points["id"]) // 4
    row_of_point = {int(v): r for r, v in enumerate(points["id"])}
    row_of_anchor = {int(v): r for r, v in enumerate(anchors["id"])}
    pr = np.array([row_of_point[p] for p, _ in want])
    ar = np.array([row_of_anchor[a] for _, a in want])
    plat, plon, alat, alon = points["latitude"][pr], points["longitude"][pr], anchors["latitude"][ar], anchors["longitude"][ar]
    wrap = anchors["region_id"][ar] == -7
    assert (wrap & (plon * alon < 0)).sum() >= 3                                  # matches across the antimeridian (53 m from each anchor)
    pole = anchors["region_id"][ar] == 3
    assert (pole & (np.abs(plon - alon) > 90.0)).sum() >= 5                       # matches across the pole's one cell
    band = anchors["region_id"][ar] == 2 ** 40
    assert (band & ((plat < boundary) != (alat < boundary))).sum() >= 5           # matches across the band boundary
    return want


def test_grid_walk_serves_both_joins_alike(pkg):
    """calc_place_visits (points as visits, anchors as places) and find_duplicate_places (points as places, anchors as
    confirmed places, empty names, no name difference allowed) walk the grid with one function: their (point, anchor)
    pairs are the same list, and it is the brute force's, in host and in device memory."""
    points, anchors, boundary = grid_walk_case()
    want = check_grid_walk_case(points, anchors, boundary)
    n, m = len(points["id"]), len(anchors["id"])
    visits = dict(person_id=points["id"], timestamp=5000 + (np.arange(n, dtype=np.int64) * 37) % 101,
                  latitude=points["latitude"], longitude=points["longitude"], region_id=points["region_id"])
    places = dict(anchors, category_id=np.zeros(m, np.int64))
    nameless = lambda side, count: dict(side, name_offsets=np.zeros(count + 1, np.int64), name_units=np.zeros(0, np.uint16))
    dp, dcf = nameless(points, n), nameless(anchors, m)
    for device in (False, True):
        v, p, a, b = ((to_device(x) if device else x) for x in (visits, places, dp, dcf))
        joined = pkg.prep.calc_place_visits(v, p, int(visits["timestamp"].min()), WALK_RADIUS)
        got_join = list(zip(to_host(joined["person_id"]).tolist(), to_host(joined["place_id"]).tolist()))
        prow, crow, diff, _ = (to_host(x) for x in pkg.deduplicator.find_duplicate_places(a, b, WALK_RADIUS, 0))
        got_dedup = list(zip(points["id"][prow].tolist(), anchors["id"][crow].tolist()))
        assert not diff.any()
        assert got_join == got_dedup
        assert got_join == want
