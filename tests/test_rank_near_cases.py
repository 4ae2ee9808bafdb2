"""CPU: the cases of rank_near_cases are fit for an equality test and do what they claim, measured with the oracle's
haversine: no (centre, place) pair lies on a radius' threshold, and every finite radius class really filters."""
import numpy as np
import pytest

import rank_batch_cases as rb
import rank_near_cases as rn

SEEDS = range(4)


@pytest.fixture(scope="module")
def meters(oracle):
    return rn.elementwise(oracle.distance_meters)


@pytest.mark.parametrize("lists", [False, True], ids=["plain", "lists"])
@pytest.mark.parametrize("seed", SEEDS)
def test_shape_of_a_case(seed, lists):
    case = rn.fuzz_case(seed, lists)
    nseg, npl = len(case["targets"]), len(case["place_ids"])
    assert len(case["lat"]) == len(case["lon"]) == npl and len(case["clat"]) == len(case["clon"]) == len(case["radius"]) == nseg
    assert (np.abs(case["lat"]) <= 90).all() and (np.abs(case["lon"]) <= 180).all()
    assert (np.abs(case["clat"]) <= 90).all() and (np.abs(case["clon"]) <= 180).all()
    assert np.array_equal(case["ids"], rb.fuzz_case(seed)["ids"])           # (the rows are fuzz_case's own)
    assert case["radius"][0] == rn.RADII[seed % 6] and set(case["radius"].tolist()) <= set(rn.RADII)
    for r, (lat0, lon0) in rn.CORNERS.items():
        at = case["regions"] == r
        assert at.any() and (case["lat"][at] >= lat0).all() and (case["lat"][at] <= lat0 + rn.BOX).all()
    at = case["regions"] == 2
    assert (case["lon"][at] > 179.9).any() and (case["lon"][at] < -179.9).any()      # both sides of the antimeridian
    assert (case["lat"][case["regions"] == 1] > 89.97).all()
    # a place listed twice in its region has two different points
    order = np.lexsort((case["place_ids"], case["regions"]))
    pid, reg = case["place_ids"][order], case["regions"][order]
    twin = np.flatnonzero((pid[1:] == pid[:-1]) & (reg[1:] == reg[:-1]))
    assert len(twin) > 0 and (case["lat"][order][twin] != case["lat"][order][twin + 1]).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_no_pair_on_a_threshold(meters, seed):
    """The device and the CPU haversine may differ by rounding, so the cases stay clear of every threshold: no
    (segment, place of its region) pair within CLEAR_METERS of the radius, apart from distance 0 at radius 0."""
    case = rn.fuzz_case(seed)
    closest = np.inf
    for s in range(len(case["targets"])):
        _, d = rn.distances(meters, case, s)
        r = case["radius"][s]
        if not np.isfinite(r) or not len(d):
            continue
        assert not np.isnan(d).any()
        gap = np.abs(d - r)
        if r == 0.0:
            gap = gap[d != 0.0]
        if len(gap):
            closest = min(closest, float(gap.min()))
    print(f"seed {seed}: closest pair to a threshold {closest:.3e} m")
    assert closest > rn.CLEAR_METERS


def test_every_finite_radius_filters(meters):
    """Over seeds 0-3, each of the radii 0, 60, 400 and 1500 has a segment whose circle removes some but not all of its
    member rows."""
    partly = {r: 0 for r in rn.RADII[:4]}
    emptied = dict(partly)
    for seed in SEEDS:
        case = rn.fuzz_case(seed)
        off = case["offsets"]
        for s in range(len(case["targets"])):
            r = float(case["radius"][s])
            if r not in partly:
                continue
            ids = case["ids"][off[s]:off[s + 1]]
            member = np.isin(ids, case["place_ids"][rn.region_rows(case, s)])
            inside = np.isin(ids, case["place_ids"][rn.kept_rows(meters, case, s)[0]])
            assert not (inside & ~member).any()
            if member.any():
                partly[r] += bool(inside.any() and (member & ~inside).any())
                emptied[r] += not inside.any()
    print("strictly filtered:", partly, "emptied:", emptied)
    assert all(v >= 1 for v in partly.values()), partly


def test_infinite_radius_is_the_plain_expectation(oracle, meters):
    case = rn.all_inf(rn.fuzz_case(1))
    want = rn.expected(oracle.rank_recommendations, meters, case, 10)
    plain = rb.expected(oracle.rank_recommendations, case, 10)
    assert rb.same((want[0], want[1], want[3]), plain)


def test_one_point_seam(meters):
    on = rn.one_point_seam(3)
    off = rn.one_point_seam(3, meters_off=1.0)
    assert len(rn.kept_rows(meters, on, 0)[0]) == len(on["place_ids"])
    rows, d = rn.distances(meters, off, 0)
    assert len(rn.kept_rows(meters, off, 0)[0]) == 0 and 0.5 < d.min() < 2.0
