"""The place deduplicator on the device (csrc/dedup.hip, csrc/place_grid.h) AT the limits of its Levenshtein tiers, its
chunks and launches, its ids and its grid: the cases of tests/dedup_limit_cases.py (checked on the CPU by
test_dedup_limit_cases.py) against the restatement of tests/dedup_cases.py.  Every comparison is exact.  Each test's
docstring names a one-line change of the sources that it catches ("Bites")."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dedup_cases as dc
import dedup_limit_cases as lim
from test_gpu_dedup import LEV_THRESHOLDS, abi_columns, assert_equals_restatement, case, switch, to_device, to_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMS = ("host", "device")
KEYS = ("id", "region_id", "latitude", "longitude", "name_offsets", "name_units")
SENTINEL = -7


def pair_lists():
    lists = {"row limit": lim.row_limit_pairs(), "scratch": lim.scratch_pairs()}
    lists.update({"lds %d" % n: pairs for n, pairs in lim.lds_size_calls().items()})
    return lists


PAIR_LISTS = ("row limit", "lds 511", "lds 512", "lds 1279", "scratch")
_LEV = {}


def lev_case(name, mem):
    """(the arguments of lev_distances in `mem`, the restatement's exact distances), the latter computed once"""
    if name not in _LEV:
        pairs = pair_lists()[name]
        assert max(lim.cells(p) for p in pairs) <= lim.FULL_DP_MAX_CELLS          # cheap enough for the full matrix
        _LEV[name] = (lim.pairs_csr(pairs), lim.exact_distances(pairs))
    args, exact = _LEV[name]
    if mem == "device":
        args = tuple(torch.as_tensor(x.view(np.int16) if x.dtype == np.uint16 else x).cuda() for x in args)
    return args, exact


_JOIN = {}


def join_case(make):
    """(places, confirmed, the oracle's distances of the in-region pairs), built once"""
    if make not in _JOIN:
        places, confirmed = make()
        _JOIN[make] = (places, confirmed, dc.pair_distances(places, confirmed))
    return _JOIN[make]


def sides(places, confirmed, mem):
    p, c = abi_columns(places), abi_columns(confirmed)
    return (to_device(p), to_device(c)) if mem == "device" else (p, c)


def raw_find(pkg, p, c, radius, k, mem, cap):
    """locrec_find_duplicate_places through ctypes with sentinel-filled outputs two elements larger than `cap`
    -> (status, count, place rows, confirmed rows, differences, not_same) on the host"""
    from locations_recommender_amd import _lib as L
    n_p, n_c = len(p["id"]), len(c["id"])
    if mem == "device":
        ptr = lambda a: C.c_void_p(a.data_ptr())                                      # noqa: E731
        new = lambda n, dt: torch.full((n,), SENTINEL, dtype=getattr(torch, np.dtype(dt).name), device="cuda")   # noqa: E731
        torch.cuda.synchronize()
    else:
        ptr = lambda a: C.c_void_p(a.ctypes.data)                                     # noqa: E731
        new = lambda n, dt: np.full(n, SENTINEL, dt)                                  # noqa: E731
    op, oc, od, ns = new(cap + 2, np.int64), new(cap + 2, np.int64), new(cap + 2, np.int32), new(n_p, np.int64)
    cnt = C.c_int64(cap)
    outs = (None, None, None) if cap == 0 else (ptr(op), ptr(oc), ptr(od))
    st = pkg.lib().locrec_find_duplicate_places(n_p, *[ptr(p[key]) for key in KEYS], n_c, *[ptr(c[key]) for key in KEYS],
                                                float(radius), int(k), L.MEM_DEVICE if mem == "device" else L.MEM_HOST,
                                                *outs, C.byref(cnt), ptr(ns))
    return (st, cnt.value) + tuple(to_host(x) for x in (op, oc, od, ns))


# ---- the Levenshtein tiers (limits 1 - 5) ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name", PAIR_LISTS)
def test_lev_distances_at_the_limits_of_the_tiers(pkg, name, mem):
    """Bites: `kLdsMaxLong = 65535` read as 65536 sends a 65,536-unit name to the u16 row, where the distance 65,536
    wraps to 0 (`row limit`); kLdsCells read as 1281 asks for 163,968 bytes of LDS for the 1,280-unit name of `scratch`,
    more than a CU has, and the call fails (read as 1279 the 1,279-unit names go to the global tier, which is still
    right); `cells = max_short + 1` without the 1 leaves the largest pair of each `lds` list unwritten."""
    d = pkg.deduplicator
    args, exact = lev_case(name, mem)
    assert np.array_equal(to_host(d.lev_distances(*args)), exact)
    for k in LEV_THRESHOLDS:
        got = to_host(d.lev_distances(*args, max_difference=k))
        assert np.array_equal(got, np.minimum(exact, k + 1)), (k, np.flatnonzero(got != np.minimum(exact, k + 1))[:5])
    with switch("LOCREC_DEDUP_FULL_DP", "1"):
        assert np.array_equal(to_host(d.lev_distances(*args)), exact)
        for k in LEV_THRESHOLDS:
            assert np.array_equal(to_host(d.lev_distances(*args, max_difference=k)), np.minimum(exact, k + 1)), k


def test_first_launch_of_a_process_above_64_kib(pkg):
    """Bites: `lds > 64 * 1024` read as `> 128 * 1024` (or the attribute call dropped): a row of 513 cells is 65,664
    bytes of dynamic LDS, which a launch gets only after hipFuncSetAttribute.  The attribute sticks to the process, so
    only a process whose FIRST stored-row call stands at 512 units can tell: a child process runs that call alone."""
    pairs = lim.lds_size_calls()[512]
    exact = lim.exact_distances(pairs)
    script = ("import sys; sys.path[:0] = [%r, %r]\n"
              "import __graft_entry__ as g, dedup_limit_cases as lim\n"
              "d = g.load_package().deduplicator\n"
              "print(d.lev_distances(*lim.pairs_csr(lim.lds_size_calls()[512]), max_difference=40).tolist())\n"
              % (ROOT, os.path.join(ROOT, "tests")))
    flags = ["-s"] if sys.flags.no_user_site else []                      # the child sees the packages this process sees
    out = subprocess.run([sys.executable, *flags, "-c", script], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == str(np.minimum(exact, 41).tolist())


@pytest.mark.parametrize("mem", MEMS)
def test_thresholds_at_the_end_of_int32(pkg, mem):
    """Bites: `clamp_threshold` dropped at either entry point: with k = 2^31 - 1 every stored-row kernel returns
    min(d, k + 1) with k + 1 overflowed in int32 (a negative "distance").  2^31 - 2 is the largest threshold whose k + 1
    is an int32."""
    d = pkg.deduplicator
    for name in PAIR_LISTS:
        args, exact = lev_case(name, mem)
        for k in lim.BIG_THRESHOLDS:
            got = to_host(d.lev_distances(*args, max_difference=k))
            print(name, mem, k, "differing pairs:", int((got != exact).sum()), "first values:", got[:4].tolist())
            assert np.array_equal(got, exact), (name, k, got[:8].tolist(), exact[:8].tolist())


def test_join_when_names_do_not_matter(pkg):
    """Bites: the clamp dropped in locrec_find_duplicate_places: with max_name_difference = 2^31 - 1 (Int.MaxValue in
    the reference) every pair inside the radius is the same place, with its exact difference - not with k + 1 overflowed."""
    d = pkg.deduplicator
    for make, radius in ((lim.chunk_case, lim.CHUNK_RADIUS), (lim.crowded_place_case, lim.CROWD_RADIUS),
                         (lim.id_extremes_case, 60.0)):
        places, confirmed, dist = join_case(make)
        p, c = sides(places, confirmed, "host")
        want = dc.drop_duplicates(places, confirmed, radius, lim.INT32_MAX, dist)
        candidates = int(lim.candidate_counts(places, confirmed, dist, radius).sum())
        assert len(want[0]) == candidates > 20                          # every candidate is reported
        for k in lim.BIG_THRESHOLDS:
            got = d.find_duplicate_places(p, c, radius, k)
            print(make.__name__, k, "differences min / max:", int(to_host(got[2]).min()), int(to_host(got[2]).max()))
            assert_equals_restatement(got, want)
            assert d.find_duplicate_places_stats()["same"] == candidates


# ---- the launches of the global tier (limit 4) ----------------------------------------------------------------------------

@pytest.mark.parametrize("label,size,per_launch", lim.scratch_sizes(), ids=[s[0].replace(" ", "_") for s in lim.scratch_sizes()])
def test_scratch_sizes_give_the_same_distances(pkg, label, size, per_launch):
    """Bites: `long_list[first + u]` read as `long_list[u]`: every launch after the first repeats the first's pairs and
    leaves its own unwritten (sizes of one and three rows: 8 and 3 launches; eight rows and the default are one launch
    and pass).  The switch itself: a size below one row must still serve one pair per launch.  Host memory only: the
    launches do not depend on where the names came from (the test above runs both at the default)."""
    d = pkg.deduplicator
    args, exact = lev_case("scratch", "host")
    with switch("LOCREC_DEDUP_SCRATCH_BYTES", str(size)) if size is not None else contextlib.nullcontext():
        for k in (-1, 16, 40):
            want = exact if k < 0 else np.minimum(exact, k + 1)
            got = d.lev_distances(*args, max_difference=k)
            assert np.array_equal(got, want), (label, k, np.flatnonzero(got != want).tolist())


def test_scratch_of_one_row_in_the_join(pkg):
    """Bites: the same changes as above, through the candidate pair lists (`pa` / `pb` are not null there): the 5,000-unit
    name of the first generated case and its copies reach the global tier at k = 20, a scratch of one 5,001-cell row
    gives one launch per pair, and a budget of 257 pairs puts the chunks' loop around it."""
    d = pkg.deduplicator
    places, confirmed, dist = case(dc.CASES[0])
    long_pairs = [(i, j) for (i, j), m in dist.items() if m <= 60.0 and places["id"][i] != confirmed["id"][j] and
                  lim.tier(dict(a=places["name"][i].lower(), b=confirmed["name"][j].lower())) == "global"]
    counts = lim.candidate_counts(places, confirmed, dist, 60.0)
    bounds = lim.chunk_bounds(counts, 257)
    assert len(bounds) >= 3 and sum(i < bounds[0][1] for i, _ in long_pairs) >= 2     # several chunks, two long pairs in the first
    want = dc.drop_duplicates(places, confirmed, 60.0, 20, dist)
    p, c = sides(places, confirmed, "host")
    with switch("LOCREC_DEDUP_SCRATCH_BYTES", str(5001 * 4)), switch("LOCREC_DEDUP_PAIR_BUDGET", "257"):
        assert_equals_restatement(d.find_duplicate_places(p, c, 60.0, 20), want)
        assert d.find_duplicate_places_stats()["chunks"] == len(bounds)
    with switch("LOCREC_DEDUP_SCRATCH_BYTES", "1"):                                   # clamped to 4 bytes: one pair per launch
        assert_equals_restatement(d.find_duplicate_places(p, c, 60.0, 20), want)


# ---- chunks of places (limits 6 and 7) ------------------------------------------------------------------------------------

def test_chunks_follow_the_model(pkg):
    """Bites: `end_off - base <= budget` read as `<` in dd_chunk_end (a run that fits exactly is cut short: budget 30,
    the total, gives more than one chunk); `++g_dedup_stats.chunks` moved inside `if (m > 0)` (chunks of places without
    candidates are not counted: budget 1); the lower clamp of the budget (`"0"` and `"-5"` must mean 1)."""
    d = pkg.deduplicator
    places, confirmed, dist = join_case(lim.chunk_case)
    counts = lim.candidate_counts(places, confirmed, dist, lim.CHUNK_RADIUS)
    want = dc.drop_duplicates(places, confirmed, lim.CHUNK_RADIUS, lim.CHUNK_NAME_DIFFERENCE, dist)
    for mem in MEMS:
        p, c = sides(places, confirmed, mem)
        for text in lim.CHUNK_BUDGETS:
            with switch("LOCREC_DEDUP_PAIR_BUDGET", text):
                assert_equals_restatement(d.find_duplicate_places(p, c, lim.CHUNK_RADIUS, lim.CHUNK_NAME_DIFFERENCE), want)
                st = d.find_duplicate_places_stats()
            print(mem, "budget", text, "chunks", st["chunks"], "candidates", st["candidates"])
            assert st["chunks"] == lim.chunk_model(counts, lim.budget_of(text)), text
            assert st["candidates"] == counts.sum() and st["same"] == len(want[0])


@pytest.mark.parametrize("mem", MEMS)
def test_capacity_across_chunks(pkg, mem):
    """Bites: `written + pos[t]` without `written` (a later chunk overwrites the first's rows); `total_same +=` without
    the last flag (a chunk that ends with a same pair makes the next land one row early); `w >= cap` read as `w > cap`
    (one row behind the capacity: the sentinels say so)."""
    from locations_recommender_amd import _lib as L
    places, confirmed, dist = join_case(lim.chunk_case)
    same, not_same = dc.drop_duplicates(places, confirmed, lim.CHUNK_RADIUS, lim.CHUNK_NAME_DIFFERENCE, dist)
    bounds = lim.chunk_bounds(lim.CHUNK_COUNTS, lim.CAPACITY_BUDGET)
    assert len(bounds) >= 4
    total = len(same)
    two_chunks = sum(1 for s in same if s[0] < bounds[1][1])                          # same pairs up to the second chunk's end
    assert 0 < two_chunks < total - 1
    p, c = sides(places, confirmed, mem)
    with switch("LOCREC_DEDUP_PAIR_BUDGET", str(lim.CAPACITY_BUDGET)):
        for cap in (0, 1, two_chunks, two_chunks + 1, total - 1, total, total + 1):
            st, cnt, op, oc, od, ns = raw_find(pkg, p, c, lim.CHUNK_RADIUS, lim.CHUNK_NAME_DIFFERENCE, mem, cap)
            assert st == L.OK and cnt == total, cap                                   # the total, whatever the capacity
            assert pkg.deduplicator.find_duplicate_places_stats()["chunks"] == len(bounds)
            m = min(cap, total)
            assert [tuple(int(v) for v in t) for t in zip(op[:m], oc[:m], od[:m])] == same[:m], cap    # a prefix of the full result
            assert (op[m:] == SENTINEL).all() and (oc[m:] == SENTINEL).all() and (od[m:] == SENTINEL).all(), cap
            assert np.array_equal(ns, not_same), cap                                  # the same for every capacity


# ---- ids, radii, one crowded place (limits 8 - 10) --------------------------------------------------------------------------

@pytest.mark.parametrize("mem", MEMS)
def test_ids_at_the_ends_of_int64(pkg, mem):
    """Bites: the `key != ~0ull` branch of dd_partners dropped (key + 1 wraps to 0: a place of id INT64_MAX subtracts no
    confirmed place of its own id and keeps 3 partners too many); `b = hi` read as `b = nc` (it subtracts the next
    regions' rows too); ordered_key without the sign flip (INT64_MIN sorts behind -1: the run of an id is not where the
    binary search looks); region ranks that treat INT64_MIN or INT64_MAX as "no region"."""
    d = pkg.deduplicator
    places, confirmed, dist = join_case(lim.id_extremes_case)
    p, c = sides(places, confirmed, mem)
    for radius in lim.ID_RADII:
        for k in lim.ID_NAME_DIFFERENCES:
            want = dc.drop_duplicates(places, confirmed, radius, k, dist)
            got = d.find_duplicate_places(p, c, radius, k, not_same_counts=True)
            assert_equals_restatement(got, want)
            assert (radius >= 0 and k >= 0) == bool(want[0])
    with switch("LOCREC_DEDUP_PAIR_BUDGET", "9"):
        assert_equals_restatement(d.find_duplicate_places(p, c, 60.0, 5), dc.drop_duplicates(places, confirmed, 60.0, 5, dist))


@pytest.mark.parametrize("mem", MEMS)
def test_radii_near_the_earth_radius(pkg, mem):
    """Bites: `ncell = min(c_hi - c_lo + 1, nx)` without the min (at 6,370,999 m a band has two cells of 180 degrees and
    the window spans three: one cell is walked twice and its pairs repeat); `((c_lo + t) % nx + nx) % nx` without the
    `+ nx` (west of Greenwich c_lo is -1: a negative cell that holds nobody)."""
    d = pkg.deduplicator
    places, confirmed, dist = join_case(lim.wide_radius_case)
    p, c = sides(places, confirmed, mem)
    for radius in lim.WIDE_RADII:
        for k in (lim.WIDE_NAME_DIFFERENCE, lim.INT32_MAX):
            want = dc.drop_duplicates(places, confirmed, radius, k, dist)
            assert len(want[0]) >= 10
            assert_equals_restatement(d.find_duplicate_places(p, c, radius, k), want)


@pytest.mark.parametrize("mem", MEMS)
def test_radii_from_the_earth_radius_on_are_refused(pkg, mem):
    """Bites: `!(max_meters < kEarthRadiusMeters)` read as `<=` (6,371,000.0 m gets a grid whose band is a radian plus a
    margin: accepted, though the limit says refused), as `max_meters >= ...` alone (NaN passes every comparison and
    reaches make_grid), or moved behind the first write to an output."""
    from locations_recommender_amd import _lib as L
    places, confirmed, _ = join_case(lim.wide_radius_case)
    p, c = sides(places, confirmed, mem)
    for radius in lim.REFUSED_RADII:
        st, cnt, op, oc, od, ns = raw_find(pkg, p, c, radius, 3, mem, 8)
        assert st == L.E_INVALID_ARG and cnt == 0, radius
        assert "below the earth radius" in pkg.lib().locrec_last_error().decode()
        assert all((x == SENTINEL).all() for x in (op, oc, od, ns)), radius             # nothing written
    st, cnt = raw_find(pkg, p, c, np.nextafter(6_371_000.0, 0.0), 3, mem, 0)[:2]        # the last radius below it
    assert st == L.OK and cnt > 0


@pytest.mark.parametrize("mem", MEMS)
def test_one_place_with_six_hundred_matches(pkg, mem):
    """Bites: `mine[b - 1] > v` read as `<` in sort_ascending (descending rows), `a = 1` read as `a = 2` (the first two
    stay as walked), `mine[b] = v` dropped.  The walk meets the rows in an order far from ascending (four cells or
    more, the last rows first), and the output must ascend within the place."""
    d = pkg.deduplicator
    places, confirmed, dist = join_case(lim.crowded_place_case)
    p, c = sides(places, confirmed, mem)
    want = dc.drop_duplicates(places, confirmed, lim.CROWD_RADIUS, lim.CROWD_NAME_DIFFERENCE, dist)
    got = d.find_duplicate_places(p, c, lim.CROWD_RADIUS, lim.CROWD_NAME_DIFFERENCE)
    assert_equals_restatement(got, want)
    crow = to_host(got[1])
    assert len(crow) >= 200 and (np.diff(crow) > 0).all() and not to_host(got[0]).any()
    assert d.find_duplicate_places_stats()["candidates"] == lim.CROWD
    everyone = d.find_duplicate_places(p, c, lim.CROWD_RADIUS, lim.INT32_MAX)          # all 600, ascending
    assert np.array_equal(to_host(everyone[1]),
                          np.array(sorted(j for (_, j), m in dist.items() if m <= lim.CROWD_RADIUS), np.int64))
