"""The CPU restatement of the place deduplicator (tests/dedup_cases.py) reproduces the reference's own known answers,
agrees with itself, and the generated cases the GPU tests use keep every in-region pair clear of every tested radius."""
import json
import os

import numpy as np
import pytest

import dedup_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def kat_frames():
    kat = load("place_deduplicator_kat.json")

    def cols(rows):
        r = list(zip(*rows))
        return dict(region_id=np.array(r[0], np.int64), id=np.array(r[1], np.int64), name=list(r[2]),
                    latitude=np.array(r[3], np.float64), longitude=np.array(r[4], np.float64))
    return kat, cols(kat["places"]), cols(kat["confirmed_places"])


def test_restatement_gives_the_levenshtein_known_answers():
    cases = load("levenshtein_kats.json")["cases"]
    assert [c["expected"] for c in cases] == [3, 6, 7, 0, 0]
    for c in cases:
        assert dc.lev(c["str1"], c["str2"]) == c["expected"], c["name"]
        assert dc.lev_rows(c["str1"], c["str2"]) == c["expected"], c["name"]


def test_restatement_gives_the_deduplicator_known_answer(oracle):
    kat, places, confirmed = kat_frames()
    dist = dc.pair_distances(places, confirmed)
    same, not_same = dc.drop_duplicates(places, confirmed, kat["max_place_distance_meters"], kat["max_name_difference"], dist)
    assert not_same.tolist() == [0, 0, 1]                     # exactly one row: id 103
    rows = [kat["places"][i] for i in np.repeat(np.arange(3), not_same)]
    assert rows == kat["expected_rows"] and rows[0][1] == 103 and rows[0][2] == "Biryulyovo Tovarnaya"
    assert same == [(0, 0, 3), (1, 0, 0)]
    lower = [s.lower() for s in places["name"]]
    assert [dc.lev(s, confirmed["name"][0].lower()) for s in lower] == kat["restated"]["name_differences"]
    got = [dist[(i, 0)] for i in range(3)]
    assert got[0] == 0.0 and abs(got[1] - 52.16) < 0.005 and int(got[2]) == 7925


def test_row_form_equals_the_literal_matrix():
    for a, b in dc.adversarial_strings():
        if len(a) * len(b) <= 20_000:
            assert dc.lev(a, b) == dc.lev_rows(a, b), (a, b)
    assert dc.lev("\U0001F600", "\U0001F601") == 1            # a surrogate pair is two units; only the low one differs
    assert dc.lev("\U0001F600", "a") == 2
    assert len(dc.units("\U00010400".lower())) == 2 and "\U00010400".lower() == "\U00010428"


def test_adversarial_strings_cover_every_tier_and_band_edge():
    pairs = dc.adversarial_strings()
    lens = {(len(dc.units(a)), len(dc.units(b))) for a, b in pairs}
    shorter = {min(x) for x in lens}
    assert 0 in shorter and any(512 < s < 1280 for s in shorter) and any(s >= 1280 for s in shorter)
    assert any(abs(x - y) in (3, 4, 7, 8, 15, 16) for x, y in lens)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: "seed%d" % c[0])
def test_generated_cases_keep_clear_of_every_radius(case, oracle):
    """A device and a libm haversine differ in the last ulps only, so a same / not same decision
    can differ only for a pair closer than that to the radius.  The fixed seeds keep 1e-6 m clear, a margin eight or
    more orders of magnitude above an ulp of these distances."""
    seed, n_places, n_confirmed, spread = case
    assert n_places <= 5000 and n_confirmed <= 5000
    places, confirmed = dc.generated_case(seed, n_places, n_confirmed, spread)
    dist = dc.pair_distances(places, confirmed)
    margin = dc.min_margin(dist)
    print("seed", seed, "in-region pairs", len(dist), "closest to a radius: %.3g m" % margin)
    assert margin > dc.MARGIN_METERS


def test_generated_cases_have_what_they_promise(oracle):
    places, confirmed = dc.generated_case(*dc.CASES[0])
    pr, cr = set(places["region_id"].tolist()), set(confirmed["region_id"].tolist())
    assert pr - cr and cr - pr and len(pr & cr) >= 3                      # regions on one side only
    assert set(places["id"].tolist()) & set(confirmed["id"].tolist())     # equal ids on both sides
    assert len(confirmed["id"]) > len(set(confirmed["id"].tolist()))      # a confirmed id that repeats
    lens = {len(dc.units(s)) for s in confirmed["name"]}
    assert set(dc.SPECIAL_LENGTHS) <= lens
    names = "".join(places["name"]) + "".join(confirmed["name"])
    assert any(ch.isupper() for ch in names) and any("а" <= ch <= "я" for ch in names) and any(ord(ch) > 0xFFFF for ch in names)
    assert np.abs(confirmed["longitude"]).max() > 179.99 and confirmed["latitude"].max() > 89.9 and confirmed["latitude"].min() < -89.9
    dist = dc.pair_distances(places, confirmed)
    counts = {}
    for k in (2, 5):
        same, not_same = dc.drop_duplicates(places, confirmed, 60.0, k, dist)
        counts[k] = len(same)
        assert len(same) > 20 and not_same.sum() > 0
    assert counts[2] < counts[5]                                          # typo counts straddle the thresholds
    diffs = {dc.lev_any(places["name"][i].lower(), confirmed["name"][j].lower()) for (i, j), d in dist.items() if d <= 60.0}
    assert {4, 5, 6, 7} & diffs and any(d > 5 for d in diffs) and any(d <= 5 for d in diffs)


def test_bad_location_is_reported_only_where_the_join_reaches_it(oracle):
    _, places, confirmed = kat_frames()
    places["latitude"][1] = 90.5
    with pytest.raises(dc.BadLocation) as e:
        dc.pair_distances(places, confirmed)
    assert (e.value.side, e.value.row) == ("place", 1)
    places["region_id"][1] = 77                                           # no confirmed place there: never constructed
    dc.pair_distances(places, confirmed)
