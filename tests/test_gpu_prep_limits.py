"""The producers (csrc/prep.hip through the C ABI, host arrays and device arrays) on the limits of their grid, keys,
tiles, counts, capacity and score order: the cases of tests/prep_limit_cases.py (each proven to stand on its limit by
tests/test_prep_limit_cases.py) against the oracle or the restatement in tests/edge_cases.py.  Every comparison is
exact - ids and order with array_equal, weights and scores as bit patterns - because the cases keep every distance
1e-3 m away from the radius.  Each docstring names the one-character change in prep.hip the test is there to catch."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import edge_cases
import prep_limit_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ("person_id", "timestamp", "place_id", "region_id", "category_id")


@pytest.fixture(scope="module")
def prep(pkg):
    return pkg.prep


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


# ---- the spatial join ---------------------------------------------------------------------------------------------------

def wanted_rows(oracle, case):
    v, p = case["visits"], case["places"]
    wv, wp = oracle.place_visits(v, p, case["visits_from"], case["radius"])
    return {"person_id": v["person_id"][wv], "timestamp": v["timestamp"][wv], "place_id": p["id"][wp],
            "region_id": v["region_id"][wv], "category_id": p["category_id"][wp]}, list(zip(wv.tolist(), wp.tolist()))


def joined(prep, case, on_device):
    v, p = case["visits"], case["places"]
    if on_device:
        v, p = {k: dev(a) for k, a in v.items()}, {k: dev(a) for k, a in p.items()}
    return {k: host(a) for k, a in prep.calc_place_visits(v, p, case["visits_from"], case["radius"]).items()}


def explain(case, got, pairs):
    """The decisions that differ, with the grid's view of each: which pair, which bands and cells."""
    v, p = case["visits"], case["places"]
    grid = lc.Grid(case["radius"])
    vrow = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(v["person_id"], v["timestamp"]))}
    have = {}
    for a, b, c, d in zip(got["person_id"].tolist(), got["timestamp"].tolist(), got["place_id"].tolist(), got["category_id"].tolist()):
        have[(vrow.get((a, b)), c, d)] = have.get((vrow.get((a, b)), c, d), 0) + 1
    want = {}
    for i, j in pairs:
        k = (i, int(p["id"][j]), int(p["category_id"][j]))
        want[k] = want.get(k, 0) + 1
    out = []
    for k in sorted(set(have) | set(want), key=str):
        if have.get(k, 0) != want.get(k, 0):
            i = k[0]
            rows = np.flatnonzero((p["id"] == k[1]) & (p["category_id"] == k[2])).tolist()
            group = [g["name"] for g in case["groups"] if g["visit"] == i]
            where = None if i is None else (grid.cell_of(v["latitude"][i], v["longitude"][i]),
                                            [grid.cell_of(p["latitude"][j], p["longitude"][j]) for j in rows])
            out.append(dict(visit=i, place_rows=rows, device=have.get(k, 0), oracle=want.get(k, 0), group=group, cells=where))
    return out[:20]


def assert_join(prep, oracle, case):
    want, pairs = wanted_rows(oracle, case)
    for on_device in (False, True):
        got = joined(prep, case, on_device)
        same = all(got[k].dtype == np.int64 and np.array_equal(got[k], want[k]) for k in COLUMNS)
        assert same, (case["name"], "device arrays" if on_device else "host arrays", explain(case, got, pairs))
    return len(pairs)


@pytest.mark.parametrize("name", list(lc.STANDARD_RADII))
def test_join_on_band_edges_cell_edges_and_poles(prep, oracle, name):
    """Decisive pairs astride band edges (first two, middle and last two bands), cell edges, the antimeridian
    (179.99.. / -179.99.. and +-180.0 exactly), at and across both poles and in the two-cell bands next to them, at 100 m,
    1 km, 50 km and on both sides of the band clamp (19.09 m) and of the equator's cell clamp (38.2 m).  Catches:
    `b = max(bv - 1, 0)` -> `bv - 0` and `min(bv + 1, ..)` -> `bv + 0` (a neighbouring band is never looked at);
    `((c_lo + t) % nx + nx) % nx` -> `((c_lo + t) % nx + 0) % nx` (the cell west of -180 is never looked at);
    `lon - win + 180.0` -> `lon - 0 + 180.0` (the western neighbour cell); `2.0 * asin(ratio)` -> `1.0 * asin(ratio)` (the
    full-window pairs); `ang * (180.0 / kPi)` -> `ang * (18.0 / kPi)` (bands lower than the radius: the full-span pairs, which
    are radius - 2 mm apart, are then two bands apart); `<= max_meters` -> `< max_meters` is not among them (no distance
    equals a radius), but `<=` -> `>=` is."""
    case = lc.standard_case(name, lc.STANDARD_RADII[name])
    assert assert_join(prep, oracle, case) == len(case["groups"])


def test_join_at_radius_zero(prep, oracle):
    """Radius 0.0: coincident points match, also 0.0 against -0.0, at the poles and on +-180.0; 1 cm away does not.
    The band clamp is what keeps this grid finite: `180.0 / (double)((1 << kCellBits) - 2)` -> `(1 < kCellBits)` makes the
    clamp negative, the bands 1e-12 degrees high and their count overflow, and nothing is found.  Also catches
    `<= max_meters` -> `< max_meters`."""
    case = lc.radius_zero_case()
    assert assert_join(prep, oracle, case) == 9


def test_join_with_thousands_of_matches_per_visit(prep, oracle):
    """3,000 matches of one visit in one cell and 600 over all nine cells around another, place rows shuffled: the rows
    of a visit come out by place row.  Catches `mine[b - 1] > v` -> `mine[b - 1] < v` in the per-visit insertion sort."""
    assert assert_join(prep, oracle, lc.many_matches_case()) == 3600


def test_join_duplicates_time_filter_and_extreme_regions(prep, oracle):
    """The same visit row twice, one place id on two rows, a timestamp equal to visits_from and one below it, regions
    -2^63 and 2^63 - 1, a region without visits and one without places.  Catches `v_ts[i] >= visits_from` -> `>` and
    `regions[mid] < region` -> `<=` in rank_of_region."""
    case, expected = lc.misc_case()
    assert assert_join(prep, oracle, case) == expected


@pytest.mark.parametrize("radius", lc.SPHERE_RADII)
def test_join_over_the_whole_sphere(prep, oracle, radius):
    """1 km to the largest accepted radius (the double below 6,371,000 m: four bands, two cells each) with points over the
    whole sphere, the poles and +-180.0 among them.  A decision may differ from the oracle's only where its distance is
    within 1e-6 m of the radius, and no more decisions may differ than the oracle itself places that close: the inputs
    keep every distance 1e-3 m away (test_sphere_case), so that number is zero and the comparison exact.  Catches
    `min(c_hi - c_lo + 1, (int64_t)nx)` -> `min(c_hi - c_lo + 2, ..)` (a cell looked at twice where a band has few) and
    `if (ratio < 1.0)` -> `if (ratio > 1.0)` (a window of 180 degrees where it is narrow and the reverse)."""
    case = lc.sphere_case(radius)
    want, pairs = wanted_rows(oracle, case)
    v, p = case["visits"], case["places"]
    for on_device in (False, True):
        got = joined(prep, case, on_device)
        if all(np.array_equal(got[k], want[k]) for k in COLUMNS):
            continue
        close = sum(1 for i in range(len(v["person_id"])) for j in np.flatnonzero(p["region_id"] == v["region_id"][i])
                    if abs(oracle.distance_meters(v["latitude"][i], v["longitude"][i], p["latitude"][j], p["longitude"][j]) - radius) < 1e-6)
        differing = explain(case, got, pairs)
        assert len(differing) <= close, (radius, on_device, close, differing)
    assert len(pairs) >= 100


def test_join_capacity_cuts_through_a_visit(prep, oracle):
    """Every capacity from 0 to the total, host and device memory: the count is the whole result and the rows written are
    its first `capacity` rows, untouched memory behind them - also where the capacity ends inside the matches of a visit
    whose cells the scan meets in another order than their place rows (the rows kept used to be the first FOUND).
    Catches `if (WRITE && base < cap)` -> `base + found < cap` (the cut visit sorts only what it met first)."""
    from locations_recommender_amd import _lib as L
    case = lc.capacity_case()
    want, pairs = wanted_rows(oracle, case)
    total = len(pairs)
    assert total == 60
    v = [np.ascontiguousarray(case["visits"][k], t) for k, t in (("person_id", np.int64), ("timestamp", np.int64), ("latitude", np.float64),
                                                                 ("longitude", np.float64), ("region_id", np.int64))]
    p = [np.ascontiguousarray(case["places"][k], t) for k, t in (("id", np.int64), ("latitude", np.float64), ("longitude", np.float64),
                                                                 ("region_id", np.int64), ("category_id", np.int64))]
    dv, dp = [dev(a) for a in v], [dev(a) for a in p]
    wrong = []
    for cap in range(total + 1):
        for mem in (L.MEM_HOST, L.MEM_DEVICE):
            if mem == L.MEM_HOST:
                outs = [np.full(cap + 8, -7, np.int64) for _ in range(5)]
                ptr = lambda a: C.c_void_p(a.ctypes.data)
                ins = v, p
            else:
                outs = [torch.full((cap + 8,), -7, dtype=torch.int64, device="cuda") for _ in range(5)]
                ptr = lambda a: C.c_void_p(a.data_ptr())
                ins = dv, dp
                torch.cuda.synchronize()
            cnt = C.c_int64(cap)
            L.check(L.lib().locrec_calc_place_visits(len(v[0]), *[ptr(a) for a in ins[0]], len(p[0]), *[ptr(a) for a in ins[1]],
                                                     case["visits_from"], case["radius"], mem, *[ptr(a) for a in outs], C.byref(cnt)))
            assert cnt.value == total, (cap, mem)
            for got, k in zip(outs, COLUMNS):
                got = host(got)
                if not (np.array_equal(got[:cap], want[k][:cap]) and np.all(got[cap:] == -7)):
                    wrong.append((cap, mem, k, got[:cap].tolist()[-12:], want[k][:cap].tolist()[-12:]))
    assert not wrong, (len(wrong), wrong[:3])


def test_distances_at_the_edge_coordinates(prep, oracle):
    """locrec_distance_meters on the coordinates of the decisive pairs (band and cell edges, +-90, +-180, +-0.0), on
    coincident points and on pairs 1 km and 100 km from antipodal, against the oracle with the tolerance of
    test_location_kats_on_device.  (At the antipode itself one ulp of the haversine moves the distance by 0.19 m: no
    tolerance that comes from a few ulp holds there, so it is not asked.)  Coincident points give exactly 0.0."""
    quads = []
    for case in (lc.standard_case("100 m", 100.0), lc.standard_case("50 km", 50_000.0), lc.radius_zero_case()):
        v, p = case["visits"], case["places"]
        for g in case["groups"]:
            for j in [g["place"], *g["near"]]:
                quads.append((v["latitude"][g["visit"]], v["longitude"][g["visit"]], p["latitude"][j], p["longitude"][j]))
    n_case = len(quads)
    for lat, lon in ((0.0, 0.0), (-0.0, 180.0), (90.0, 13.0), (-90.0, -170.0), (55.75, 37.62), (12.0, -180.0)):
        quads.append((lat, lon, lat, lon))
    for lat, lon in ((0.0, 0.0), (55.75, 37.62), (-33.0, 151.0), (89.0, 10.0)):
        for off in (1000.0, 100_000.0):
            quads.append((lat, lon, -lat + off / lc.MPD, lon - 180.0 if lon > 0 else lon + 180.0))
    quads += [(90.0, 0.0, 0.0, 0.0), (0.0, -180.0, 0.0, 180.0), (0.0, 180.0, 0.0, 0.0), (90.0, 5.0, 90.0, -175.0), (45.0, 180.0, 45.0, -180.0)]
    a = np.array(quads, np.float64)
    want = np.array([oracle.distance_meters(*q) for q in quads])
    for on_device in (False, True):
        cols = [dev(a[:, k]) for k in range(4)] if on_device else [a[:, k].copy() for k in range(4)]
        got = host(prep.distance_meters(*cols))
        print("largest difference from the oracle, m:", float(np.abs(got - want).max()))
        assert np.allclose(got, want, rtol=1e-9, atol=1e-7), np.abs(got - want).max()
        assert (got[n_case:n_case + 6] == 0.0).all() and not np.signbit(got[n_case:n_case + 6]).any()


# ---- the co-visit join --------------------------------------------------------------------------------------------------

def assert_same_edges(got, want, what=None):
    gs, gt, gw = (host(x) for x in got)
    ws, wt, ww = want
    assert gs.dtype == np.int64 and gt.dtype == np.int64 and gw.dtype == np.float64, what
    assert np.array_equal(gs, ws) and np.array_equal(gt, wt), what
    assert np.array_equal(gw.view(np.int64), ww.view(np.int64)), what      # bit for bit


def similar(prep, cols, interval, top_n, on_device):
    if on_device:
        return prep.calc_similar_place_edges(*[dev(c) for c in cols], interval, top_n)
    return prep.calc_similar_place_edges(*cols, interval, top_n)


@pytest.mark.parametrize("n_places", lc.PLACE_COUNTS)
def test_pair_keys_at_place_counts_around_powers_of_two(prep, n_places):
    """2, 3, 4, 5, 2^8, 2^8 + 1, 2^16 and 2^16 + 1 places, the highest rank on both sides of a key `rank_a << nb | rank_b`.
    Catches `((int64_t)1 << nb) < np` -> `((int64_t)2 << nb) < np` (one bit too few at 3, 5 and 2^k + 1 places: two ranks
    share a key) and `(keys[i] >> nb) != (keys[i] & ((1ull << nb) - 1))` -> `- 0)` in pr_pair_flags."""
    cols = lc.place_count_case(n_places)
    counts = edge_cases.covisit_counts_loops(*cols, 0)
    for top_n in (1, 50):
        want = edge_cases.rank_and_normalise(counts, top_n)
        assert len(want[0]) >= n_places
        for on_device in (False, True):
            assert_same_edges(similar(prep, cols, 0, top_n, on_device), want, (n_places, top_n, on_device))


@pytest.mark.parametrize("name", list(lc.TILE_CASES))
def test_pair_tiles_that_end_on_before_and_after_a_row(prep, name):
    """Candidate pairs of 2,046 / 2,048 / 2,050 / 4,096 in all (a total is never odd: (a, b) comes with (b, a)), and the end
    of the first 2,048-pair tile on the first, the second, a middle and the last partner of a row, with rows without
    partner before, at and after it.  Catches `threadIdx.x == 0 ? t0 : t1 - 1` -> `t1 - 2` (the row of the tile's last pair
    is not searched) and `if (j >= a) ++j` -> `if (j > a) ++j` (a row is its own partner)."""
    cols = lc.tile_case(name)
    _, off = lc.windows(*cols, 0)
    counts = edge_cases.covisit_counts_loops(*cols, 0)
    for top_n in (1, 50):
        want = edge_cases.rank_and_normalise(counts, top_n)
        for on_device in (False, True):
            assert_same_edges(similar(prep, cols, 0, top_n, on_device), want, (name, top_n, on_device))
            stats = prep.similar_place_edges_stats()
            assert stats["pairs"] == off[-1] and stats["chunks"] == 1, (name, stats)
    assert all(x.size == 0 for x in similar(prep, cols, -1, 50, False))


@pytest.mark.parametrize("budget", lc.BUDGETS)
def test_chunks_that_end_on_the_pair_budget(prep, tmp_path, budget):
    """LOCREC_PREP_PAIR_BUDGET = 2,048 - the candidate pairs of the first rows exactly - one less and one more, each in a
    fresh process (the switch is read once): the chunk count says which side was hit, and the edges equal the default run
    and the restatement bit for bit.  Catches `off[mid] - base <= budget` -> `< budget` in pr_chunk_end (a chunk that fits
    exactly is cut a row early: 3 chunks where 2 are due)."""
    out = str(tmp_path / "budget.npz")
    env = dict(os.environ, LOCREC_PREP_PAIR_BUDGET=str(budget))
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import __graft_entry__ as g, prep_limit_cases; "
            "prep_limit_cases.run_budget_cases(g.load_package(), sys.argv[3])")
    r = subprocess.run([sys.executable, "-c", code, ROOT, os.path.dirname(os.path.abspath(__file__)), out], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    small = np.load(out)
    for name in lc.BUDGET_SIZES:
        cols = lc.budget_case(name)
        _, off = lc.windows(*cols, 0)
        chunks = lc.chunk_pairs(off, budget)
        assert int(small[name + "_chunks"]) == len(chunks) and int(small[name + "_pairs"]) == off[-1], (name, budget, chunks)
        got = prep.calc_similar_place_edges(*cols, 0, 50)
        assert prep.similar_place_edges_stats()["chunks"] == 1
        assert_same_edges((small[name + "_source"], small[name + "_target"], small[name + "_weight"]), got, (name, budget))
        assert_same_edges(got, edge_cases.rank_and_normalise(edge_cases.covisit_counts_loops(*cols, 0), 50), name)


@pytest.mark.parametrize("top_n", [1, 50])
@pytest.mark.parametrize("on_device", [False, True])
def test_counts_of_two_to_the_32(prep, top_n, on_device):
    """One person, 131,073 rows inside one interval at three places of 65,536, 65,536 and 1 rows: count(10, 20) = 2^32,
    whose low word is zero, against count(10, 30) = 65,536, summed over 65 chunks of the default budget
    (17,180,000,256 candidate pairs).  Expected edges from the closed form rows(a) * rows(b).  Catches
    `rank_keep(m, srank.p, R.counts.p, top_n, true, ..` -> `false` (the packed 32-bit rank key: the rank inverts),
    `out_counts[pos[i]] = counts[i]` summed in 32 bits, and a `uint32_t` total in kept_totals."""
    cols, counts = lc.wide_count_case()
    want = edge_cases.rank_and_normalise(counts, top_n)
    t0 = time.perf_counter()
    got = similar(prep, cols, edge_cases.INTERVAL_MS, top_n, on_device)
    if on_device:
        torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    stats = prep.similar_place_edges_stats()
    print(f"2^32 counts: {seconds:.2f} s, {stats}")
    assert_same_edges(got, want, (top_n, on_device))
    n = len(cols[0])
    assert stats["pairs"] == n * (n - 1) and stats["chunks"] == 65


# ---- the final ranking ----------------------------------------------------------------------------------------------------

def ranked_bits(r):
    return host(r[0]), host(r[1]).view(np.int64)


@pytest.mark.parametrize("on_device", [False, True])
def test_ranking_of_special_scores(prep, oracle, on_device):
    """NaN of both signs and with payloads (one value, above +inf), +-inf, +-0.0 (equal: id ascending decides), subnormals,
    equal scores on ids -2^63 .. 2^63 - 1, ids and places listed twice, limits 1, count - 1, count, count + 1: Spark SQL's
    order of doubles, ties by id and then by input row, against the oracle with scores as bit patterns.  Catches
    `if (s != s)` -> `if (s == s)` and `else if (s == 0.0) b = 0ull` -> `b = 1ull` in score_desc_key (a NaN with the sign
    set sorts below -inf; -0.0 sorts below 0.0), and `(b >> 63) ? ~b : b | 0x8000..` -> `(b >> 62)`."""
    case = lc.ranking_case()
    kept = case["kept"]
    cols = (case["ids"], case["scores"], case["place_ids"], case["place_regions"])
    a = tuple(dev(c) for c in cols) if on_device else cols
    for limit in (-1, 0, 1, kept - 1, kept, kept + 1, 10 ** 9):
        want = oracle.rank_recommendations(*cols, case["target"], limit)
        got = prep.rank_recommendations(*a, case["target"], limit)
        assert len(want[0]) == min(max(limit, 0), kept)
        gi, gs = ranked_bits(got)
        wi, ws = ranked_bits(want)
        assert np.array_equal(gi, wi) and np.array_equal(gs, ws), (limit, gi[:12], wi[:12])
    scores = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324, 0.0])
    ids = np.arange(8, dtype=np.int64)
    b = (dev(ids), dev(scores), dev(ids), dev(np.zeros(8, np.int64))) if on_device else (ids, scores, ids, np.zeros(8, np.int64))
    assert host(prep.rank_recommendations(*b, 0, 8)[0]).tolist() == [2, 3, 5, 0, 1, 7, 6, 4]
