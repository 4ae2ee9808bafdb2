"""The cases of tests/dedup_limit_cases.py hold what they promise: the closed forms are the restatement's distances,
every list stands on the limit it names, the chunk model is the literal loop, and every join case keeps its in-region
pairs clear of its own radii.  Needs no GPU."""
import numpy as np
import pytest

import dedup_cases as dc
import dedup_limit_cases as lim


def test_limits_are_the_literals_the_sources_are_read_for():
    assert (lim.LDS_MAX_LONG, lim.LDS_CELLS, lim.SCRATCH_BYTES) == (2 ** 16 - 1, 1280, 268435456)
    assert lim.LDS_CELLS * 64 * 2 == 160 * 1024                                        # the whole LDS of a CU
    assert (lim.LDS_ATTRIBUTE_SHORT - 1 + 1) * 64 * 2 == 64 * 1024 < (lim.LDS_ATTRIBUTE_SHORT + 1) * 64 * 2
    assert lim.BIG_THRESHOLDS == (2147483646, 2147483647)


def test_row_limit_closed_forms_equal_the_row_form():
    pairs = lim.row_limit_pairs()
    exact = lim.exact_distances(pairs)
    assert exact.tolist() == [p["closed"] for p in pairs]
    assert {lim.shorter_longer(p) for p in pairs} == {(s, n) for n in lim.ROW_LIMIT_LONG for s in lim.ROW_LIMIT_SHORT}
    assert {p["kind"] for p in pairs} == {"equal units / empty", "disjoint alphabet", "cut from the middle"}
    by_tier = {n: {lim.tier(p) for p in pairs if lim.shorter_longer(p)[1] == n} for n in lim.ROW_LIMIT_LONG}
    assert by_tier == {65534: {"lds"}, 65535: {"lds"}, 65536: {"global"}, 65537: {"global"}}
    assert 65535 in exact and 65536 in exact                                           # the largest u16, and the first to wrap
    assert max(lim.cells(p) for p in pairs) <= lim.FULL_DP_MAX_CELLS
    assert {len(dc.units(p["a"])) <= len(dc.units(p["b"])) for p in pairs} == {True, False}    # both orders of the swap


def test_row_form_equals_the_literal_matrix_on_shortened_row_limit_pairs():
    """The same generator at lengths the literal matrix can afford, in both argument orders of the row form."""
    pairs = lim.row_limit_pairs((254, 255, 256, 257))
    for p in pairs:
        want = dc.lev(p["a"], p["b"])
        assert want == p["closed"] == dc.lev_rows(p["a"], p["b"]) == dc.lev_rows(p["b"], p["a"]), p["kind"]
    for n, pairs in lim.lds_size_calls().items():
        for p in pairs[:6]:
            assert dc.lev(p["a"], p["b"]) == lim.exact_distances([p])[0]


def test_lds_size_calls_stand_on_their_sizes():
    calls = lim.lds_size_calls()
    assert tuple(calls) == (511, 512, 1279)
    for n, pairs in calls.items():
        shorter = [lim.shorter_longer(p)[0] for p in pairs]
        assert max(shorter) == n and shorter.count(n) >= 3
        assert all(lim.tier(p) == "lds" for p in pairs)                                  # no name above 65,535 units
        assert sum(s < 40 for s in shorter) >= 10                                        # ordinary short pairs
        diff = np.array([abs(np.subtract(*lim.lengths(p))) for p in pairs])
        wide = np.array([p["wide"] for p in pairs])
        assert diff.max() == 40 and (diff <= 40).all()                                   # none is cut at threshold 40,
        assert (diff[~wide] <= 16).all() and (diff[wide] > 16).all() and wide.sum() == 3     # none but the wide ones at 16
        assert any(s == n and not p["wide"] for s, p in zip(shorter, pairs))
        exact = lim.exact_distances(pairs)
        assert exact.min() == 0 and exact.max() >= 41                                    # 0 - 45 typos,
        for k in lim.BAND_THRESHOLDS:                                                    # on both sides of each threshold
            walked = exact[diff <= k]
            assert (walked <= k).sum() >= 5 and (walked > k).sum() >= 2
    # the row's bytes: cells x 64 lanes x u16
    assert [(n + 1) * 128 > 64 * 1024 for n in calls] == [False, True, True] and (1279 + 1) * 128 == 160 * 1024


def test_scratch_pairs_are_eight_rows_of_distinct_sizes():
    pairs = lim.scratch_pairs()
    tiers = [lim.tier(p) for p in pairs]
    long_rows = [lim.shorter_longer(p)[0] + 1 for p, t in zip(pairs, tiers) if t == "global"]
    assert len(long_rows) == 8 == len(set(long_rows)) and sorted(long_rows) == sorted(s + 1 for s in lim.SCRATCH_SHORTER)
    assert min(long_rows) == lim.LDS_CELLS + 1 and max(long_rows) <= 1401                # the first row the LDS cannot hold
    first_long = tiers.index("global")
    assert first_long > 0 and "lds" in tiers[first_long:]                                # no prefix of the pair list
    assert sum(lim.shorter_longer(p)[0] >= 300 for p, t in zip(pairs, tiers) if t == "lds") >= 3
    assert max(lim.cells(p) for p in pairs) <= lim.FULL_DP_MAX_CELLS
    row = max(long_rows) * 4
    got = [(label, size if size is None else divmod(size, row), per) for label, size, per in lim.scratch_sizes()]
    assert got == [("below one row", (0, row - 1), 1), ("one row", (1, 0), 1), ("three rows", (3, 0), 3),
                   ("eight rows", (8, 0), 8), ("default", None, 8)]
    for label, size, per in lim.scratch_sizes():                                         # max(1, min(pairs, bytes / row))
        assert per == max(1, min(8, (lim.SCRATCH_BYTES if size is None else size) // row)), label


def slow_chunks(counts, budget):
    """The literal loop: try every end from the far side."""
    n, begin, chunks = len(counts), 0, 0
    while begin < n:
        end = begin + 1
        for e in range(n, begin, -1):
            if sum(counts[begin:e]) <= budget:
                end = e
                break
        chunks += 1
        begin = end
    return chunks


def test_chunk_model_equals_the_literal_loop():
    lists = ([0, 0, 0, 0], [5], [0], [1, 1, 1, 1, 1], [0, 9, 0], [9, 0, 0, 9], [3, 0, 0, 0, 4, 0], [2, 2, 2, 7, 0, 1, 1],
             list(lim.CHUNK_COUNTS))
    for counts in lists:
        for budget in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 30, 31, 2 ** 30):
            assert lim.chunk_model(counts, budget) == slow_chunks(counts, budget), (counts, budget)
            bounds = lim.chunk_bounds(counts, budget)
            assert bounds[0][0] == 0 and bounds[-1][1] == len(counts)
            assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    assert lim.chunk_model([0, 0, 0, 0], 1) == 1 and lim.chunk_model([2, 2], 1) == 2      # chunks without a pair count;
    assert lim.chunk_model([0, 9, 0], 1) == 3                                             # [0], [9], [0]: one place at least
    # hand-counted on the case's own counts (0, 3, 2, 0, 0, 13, 4, 1, 0, 7, 0, 0)
    c = list(lim.CHUNK_COUNTS)
    assert [lim.chunk_model(c, b) for b in (1, 2, 3, 4, 5, 6, 7, 30, 31)] == [9, 8, 7, 7, 5, 5, 4, 1, 1]
    assert lim.chunk_bounds(c, lim.CAPACITY_BUDGET) == [(0, 5), (5, 6), (6, 9), (9, 10), (10, 12)]
    assert [lim.budget_of(t) for t in ("0", "-5", "7", "4294967296")] == [1, 1, 7, 2 ** 30]


def test_chunk_case_has_the_chosen_counts(oracle):
    places, confirmed = lim.chunk_case()
    dist = dc.pair_distances(places, confirmed)
    counts = lim.candidate_counts(places, confirmed, dist, lim.CHUNK_RADIUS)
    assert counts.tolist() == list(lim.CHUNK_COUNTS)
    c = list(lim.CHUNK_COUNTS)
    assert c[0] == 0 and c[-1] == 0 and 0 in c[3:5] and max(c) > 7                        # zeros everywhere, one count above
    budgets = {lim.budget_of(t) for t in lim.CHUNK_BUDGETS}                              # every small budget
    assert {1, 2, c[1], c[1] + c[2] - 1, c[1] + c[2], c[1] + c[2] + 1, sum(c), sum(c) + 1, 2 ** 30} <= budgets
    assert len(set(places["region_id"].tolist()) | set(confirmed["region_id"].tolist())) == 1
    assert len(dist) > sum(c) + len(c)                                                    # confirmed places beyond the radius too
    assert set(places["id"].tolist()) & set(confirmed["id"].tolist())                    # ... and equal ids within it
    same, not_same = dc.drop_duplicates(places, confirmed, lim.CHUNK_RADIUS, lim.CHUNK_NAME_DIFFERENCE, dist)
    assert sum(c) // 3 <= len(same) <= 2 * sum(c) // 3                                    # about half are name matches
    per_chunk = [sum(1 for s in same if a <= s[0] < b) for a, b in lim.chunk_bounds(c, lim.CAPACITY_BUDGET)]
    assert len(per_chunk) == 5 and all(per_chunk[:4]) and per_chunk[4] == 0               # four chunks write, the last is empty


def test_id_extremes_case_has_what_it_promises(oracle):
    places, confirmed = lim.id_extremes_case()
    five = {lim.INT64_MIN, lim.INT64_MAX, -1, 0, 1}
    assert set(confirmed["id"].tolist()) == five and five <= set(places["id"].tolist())
    assert sorted(set(confirmed["region_id"].tolist())) == [lim.INT64_MIN, 5, lim.INT64_MAX]
    assert set(places["region_id"].tolist()) - set(confirmed["region_id"].tolist()) == {77}
    order = np.lexsort((confirmed["id"], confirmed["region_id"]))                         # by (region, id)
    ids, regions = confirmed["id"][order], confirmed["region_id"][order]
    last = np.flatnonzero(np.diff(regions) != 0)
    assert len(last) == 2
    for at in last:                                                                       # ... MAX, MAX, MAX | MIN ...
        assert ids[at - 2:at + 1].tolist() == [lim.INT64_MAX] * 3 and ids[at + 1] == lim.INT64_MIN
    assert ids[-1] == lim.INT64_MAX
    dist = dc.pair_distances(places, confirmed)
    assert len(dist) == 300 and max(dist.values()) < 30.0 + 1e-3
    same, not_same = dc.drop_duplicates(places, confirmed, 60.0, 5, dist)
    hit = {int(places["id"][i]) for i, _, _ in same} | {int(confirmed["id"][j]) for _, j, _ in same}
    assert {lim.INT64_MIN, lim.INT64_MAX} <= hit and 20 < len(same) < 250 and not_same.sum() > 20
    _, partners = dc.drop_duplicates(places, confirmed, -1.0, -1, dist)                   # nobody is the same: all partners
    by_id = {int(i): set(partners[places["id"] == i].tolist()) for i in five}
    assert by_id[lim.INT64_MAX] == {7, 0} and by_id[lim.INT64_MIN] == {8} and by_id[-1] == {9}    # (0: the place in region 77)


def test_wide_radius_case_has_what_it_promises(oracle):
    places, confirmed = lim.wide_radius_case()
    assert 55 <= len(places["id"]) <= 65 and 55 <= len(confirmed["id"]) <= 65
    for side in (places, confirmed):
        lat, lon = side["latitude"], side["longitude"]
        assert lat.max() == 90.0 and lat.min() == -90.0 and lon.max() == 180.0 and lon.min() == -180.0
        assert (lat > 60).sum() >= 3 and (lat < -60).sum() >= 3 and (np.abs(lon) < 0.05).sum() >= 2
    dist = dc.pair_distances(places, confirmed)
    d = np.array(list(dist.values()))
    assert lim.WIDE_RADII == (1.0e6, 6370999.0) and all(r < dc.EARTH_RADIUS_METERS for r in lim.WIDE_RADII)
    assert lim.REFUSED_RADII[0] == dc.EARTH_RADIUS_METERS
    for radius in lim.WIDE_RADII:                                                         # some inside, some outside
        inside = (d <= radius).sum()
        assert 30 <= inside <= len(d) - 30, (radius, inside)
        same, _ = dc.drop_duplicates(places, confirmed, radius, lim.WIDE_NAME_DIFFERENCE, dist)
        assert len(same) >= 10
    assert d.max() > 1.9e7                                                                # nearly antipodal pairs


def test_crowded_place_case_has_what_it_promises(oracle):
    places, confirmed = lim.crowded_place_case()
    assert len(places["id"]) == 1
    dist = dc.pair_distances(places, confirmed)
    counts = lim.candidate_counts(places, confirmed, dist, lim.CROWD_RADIUS)
    assert counts.tolist() == [lim.CROWD] and len(dist) == lim.CROWD + 40
    same, _ = dc.drop_duplicates(places, confirmed, lim.CROWD_RADIUS, lim.CROWD_NAME_DIFFERENCE, dist)
    assert 200 <= len(same) <= 400
    lat, lon = confirmed["latitude"], confirmed["longitude"]
    assert (np.diff(lat) <= 0).all()                                                      # rows by descending latitude
    band_deg = np.degrees(lim.CROWD_RADIUS / dc.EARTH_RADIUS_METERS)                      # a band and (here) a cell
    inside = np.array([dist[(0, j)] <= lim.CROWD_RADIUS for j in range(len(lat))])
    assert np.ptp(lat[inside]) > 1.5 * band_deg and np.ptp(lon[inside]) > 1.5 * band_deg  # two bands x two cells at least


@pytest.mark.parametrize("name,make,radii", lim.JOIN_CASES, ids=[c[0].replace(" ", "_") for c in lim.JOIN_CASES])
def test_join_cases_keep_clear_of_their_radii(name, make, radii, oracle):
    """The margin condition of test_dedup_cases.py, for each case's own radii: a seed that fails is replaced."""
    places, confirmed = make()
    dist = dc.pair_distances(places, confirmed)
    margin = dc.min_margin(dist, radii)
    print(name, "in-region pairs", len(dist), "closest to a radius: %.3g m" % margin)
    assert margin > dc.MARGIN_METERS
