"""Inputs that stand exactly ON the limits of the place deduplicator (csrc/dedup.hip, csrc/place_grid.h; DESIGN.md
section 9a, "Limits that tests stand on"), shared by the CPU checks of the cases themselves
(test_dedup_limit_cases.py) and the GPU tests (test_gpu_dedup_limits.py).  Plain numpy and dedup_cases: nothing of
the package under test.

A pair list is a list of dicts {a, b, kind} of Python strings (used as given: no lower-casing on either side); a join
case is a pair of column dicts as dedup_cases makes them.

The limits are written here as literals on purpose: a test that asks the library where its limit lies cannot catch a
moved limit."""
import functools

import numpy as np

import dedup_cases as dc

LDS_MAX_LONG = 65535              # the LDS row's cells are u16: the longer name of a pair it serves has at most this many units
LDS_CELLS = 1280                  # cells of the largest LDS row (1280 x 64 lanes x 2 B = 160 KiB): the shorter name + 1
LDS_ATTRIBUTE_SHORT = 512         # (512 + 1) cells x 64 x 2 B is the first row above 64 KiB: the launch needs the attribute
SCRATCH_BYTES = 256 << 20         # global rows per launch of the third tier, by default
FULL_DP_MAX_CELLS = 3_000_000     # shorter x longer above which no test forces the full matrix on a pair
INT32_MAX = 2 ** 31 - 1
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
BIG_THRESHOLDS = (INT32_MAX - 1, INT32_MAX)      # "names do not matter": k + 1 must not be computed in int32
BAND_THRESHOLDS = (16, 40)                       # the two thresholds of test_gpu_dedup.LEV_THRESHOLDS that walk a stored row

LOWER = "abcdefghijklmnopqrstuvwxyz абвгдежзийклмнопрстуфхцчшщъыьэюя"    # one unit each; never '#' or '@'


def fast_name(rng, n, alphabet=LOWER):
    return "".join(np.array(list(alphabet))[rng.integers(len(alphabet), size=n)])


def edited(rng, name, subs=0, ins=0, dels=0):
    """Exactly that many deletions, then substitutions by '#' at distinct places, then insertions of '@': the length
    changes by ins - dels, and at most subs + ins + dels units differ."""
    chars = list(name)
    for _ in range(dels):
        del chars[int(rng.integers(len(chars)))]
    for at in rng.choice(len(chars), subs, replace=False) if subs else ():
        chars[int(at)] = "#"
    for _ in range(ins):
        chars.insert(int(rng.integers(len(chars) + 1)), "@")
    return "".join(chars)


def lengths(pair):
    return len(dc.units(pair["a"])), len(dc.units(pair["b"]))


def shorter_longer(pair):
    la, lb = lengths(pair)
    return min(la, lb), max(la, lb)


def cells(pair):
    s, g = shorter_longer(pair)
    return s * g


def tier(pair):
    """Which stored row serves the pair once the threshold is above 15 (or absent): dd_lev_lds or dd_lev_global."""
    s, g = shorter_longer(pair)
    return "lds" if s + 1 <= LDS_CELLS and g <= LDS_MAX_LONG else "global"


def pairs_csr(pairs):
    """-> (a_offsets, a_units, b_offsets, b_units) as locrec_lev_distances takes them"""
    a, b = dc.csr([p["a"] for p in pairs]), dc.csr([p["b"] for p in pairs])
    return a[0], a[1], b[0], b[1]


def exact_distances(pairs):
    """lev of every pair by the row form, the shorter name first (its loop runs over the first argument)."""
    out = []
    for p in pairs:
        la, lb = lengths(p)
        out.append(dc.lev_rows(p["a"], p["b"]) if la <= lb else dc.lev_rows(p["b"], p["a"]))
    return np.array(out, np.int32)


# ---- limit 1: the u16 cells of the LDS row -------------------------------------------------------------------------------

ROW_LIMIT_LONG = (65534, 65535, 65536, 65537)
ROW_LIMIT_SHORT = (0, 1, 40)


@functools.lru_cache(maxsize=None)
def row_limit_pairs(long_lengths=ROW_LIMIT_LONG):
    """Pairs whose longer name has 65,534 .. 65,537 units and whose shorter one has 0, 1 or 40, each with the distance
    in closed form (`closed`): all-equal units against the empty name (the length: 65,535 is the largest u16, 65,536
    wraps to 0 in one), a disjoint alphabet (the longer length), the shorter name cut from the middle of the longer
    (the length difference).  Every other pair has the shorter name first, so both orders of the row's swap run.
    `long_lengths` exists for the shortened variants that the literal matrix can afford."""
    rng = np.random.default_rng(65535)
    pairs = []
    for n in long_lengths:
        long_name = fast_name(rng, n)
        found = [dict(a="a" * n, b="", closed=n, kind="equal units / empty")]
        for s in ROW_LIMIT_SHORT[1:]:
            found.append(dict(a=long_name, b="#@"[s % 2] * s, closed=n, kind="disjoint alphabet"))
            at = (n - s) // 2
            found.append(dict(a=long_name, b=long_name[at:at + s], closed=n - s, kind="cut from the middle"))
        for p in found:
            if len(pairs) % 2:
                p["a"], p["b"] = p["b"], p["a"]
            pairs.append(p)
    return tuple(pairs)


# ---- limits 2 and 3: the size of the dynamic LDS -----------------------------------------------------------------------

LDS_SIZE_LARGEST_SHORTER = (511, 512, 1279)


@functools.lru_cache(maxsize=None)
def lds_size_calls():
    """{largest shorter name: pair list}, one list per call: 511 (a row of exactly 64 KiB, the last that needs no
    attribute), 512 (the first that does) and 1279 (1,280 cells: the whole LDS of a CU).  Every list also holds
    ordinary short pairs, every name has at most 65,535 units, so the LDS row serves every pair.  The partners differ
    by 0 - 45 typos and by 0 - 40 units in length: `wide` marks the pairs whose lengths differ by 17 - 40 (cut by the
    length pre-test at threshold 16, walked to the band's edge at 40); no other pair is cut at either threshold, the
    pair that holds the largest shorter name among them."""
    calls = {}
    for n in LDS_SIZE_LARGEST_SHORTER:
        rng = np.random.default_rng(n)
        pairs = []

        def add(base, wide=False, **edits):
            other = edited(rng, base, **edits)
            pair = dict(a=base, b=other, wide=wide) if len(pairs) % 2 == 0 else dict(a=other, b=base, wide=wide)
            pairs.append(pair)
        for j in range(6):                                                       # ordinary short pairs in front
            base = dc.random_name(rng)
            pairs.append(dict(a=base, b=dc.with_typos(rng, base, j), wide=False))
        add(fast_name(rng, n), subs=10, ins=16)                                  # shorter = n exactly, 26 typos
        add(fast_name(rng, n))                                                   # equal names of n units
        add(fast_name(rng, n + 9), subs=3, dels=9)                               # shorter = n after the deletions
        add(fast_name(rng, n - 7), subs=20, dels=16)
        add(fast_name(rng, n - 50), wide=True, subs=5, ins=40)                   # 45 typos, lengths differ by 40
        add(fast_name(rng, n - 3), wide=True, dels=17)
        add(fast_name(rng, n - 1), wide=True, subs=1, dels=39)
        for typos in (0, 1, 15, 16, 17, 39, 40, 41, 45):                         # straddling both thresholds
            length = int(rng.integers(64, n - 50))
            ins = min(typos, int(rng.integers(0, 9)))
            add(fast_name(rng, length), subs=typos - ins, ins=ins // 2, dels=ins - ins // 2)
        for j in range(6):
            base = dc.random_name(rng)
            pairs.append(dict(a=base, b=dc.with_typos(rng, base, 8 - j), wide=False))
        calls[n] = tuple(pairs)
    return calls


# ---- limit 4: the launches of the global tier ----------------------------------------------------------------------------

SCRATCH_SHORTER = (1280, 1297, 1311, 1400, 1333, 1350, 1289, 1376)     # distinct, 1,280 .. 1,400; the largest in the middle


@functools.lru_cache(maxsize=None)
def scratch_pairs():
    """Eight pairs of the global tier (shorter names of SCRATCH_SHORTER units, partners 0 - 45 typos away) interleaved
    with pairs of the LDS tier and short pairs, a short one first: the list of long pairs is no prefix of the pair list."""
    rng = np.random.default_rng(1280)
    pairs = []
    for j, n in enumerate(SCRATCH_SHORTER):
        base = dc.random_name(rng)
        pairs.append(dict(a=base, b=dc.with_typos(rng, base, j)))
        typos = (0, 6, 17, 45, 40, 16, 30, 41)[j]
        ins = min(typos, 2 * j)
        base = fast_name(rng, n)
        other = edited(rng, base, subs=typos - ins, ins=ins)                    # never shorter than the base
        pairs.append(dict(a=base, b=other) if j % 2 else dict(a=other, b=base))
        if j % 3 == 0:
            base = fast_name(rng, 300 + 100 * j)
            pairs.append(dict(a=base, b=edited(rng, base, subs=j, dels=j)))
    return tuple(pairs)


def scratch_sizes():
    """[(label, LOCREC_DEDUP_SCRATCH_BYTES or None for the default, pairs per launch)] in multiples of the largest row
    of scratch_pairs(), (largest shorter + 1) x 4 bytes: just below one row (the launch keeps one pair), one row, three
    rows (launches of 3, 3 and 2 pairs), eight rows and the default."""
    row = (max(SCRATCH_SHORTER) + 1) * 4
    return (("below one row", row - 1, 1), ("one row", row, 1), ("three rows", 3 * row, 3), ("eight rows", 8 * row, 8),
            ("default", None, 8))


# ---- limits 6 and 7: chunks of places ------------------------------------------------------------------------------------

CHUNK_COUNTS = (0, 3, 2, 0, 0, 13, 4, 1, 0, 7, 0, 0)       # candidates per place: zeros in front, in the middle, at the end
CHUNK_RADIUS = 60.0
CHUNK_NAME_DIFFERENCE = 5
# 1, 2; 4 and 7 are single counts, 3 too; 5 = 3 + 2 is a sum of neighbours, with 4 and 6 around it; the total and one
# more; 13 is above every small budget.  The strings are what the switch reads: "0" and "-5" mean 1, 2^32 is clamped.
CHUNK_BUDGETS = ("1", "2", "3", "4", "5", "6", "7", "30", "31", "0", "-5", "4294967296")
MAX_PAIR_BUDGET = 1 << 30
CAPACITY_BUDGET = 5                                        # chunks [0, 5), [5, 6), [6, 9), [9, 10), [10, 12)


def budget_of(text):
    """What LOCREC_DEDUP_PAIR_BUDGET=text means: at least 1, at most 2^30."""
    return min(max(int(text), 1), MAX_PAIR_BUDGET)


def chunk_bounds(counts, budget):
    """The chunks [(begin, end)] of places: from `begin`, a chunk ends at the largest end > begin whose candidates
    sum(counts[begin:end]) fit the budget, or at begin + 1 where there is none; until begin reaches the places' number.
    Chunks without a pair count.  (A call without ANY candidate never enters the device's loop and reports no chunk; the
    model is compared where there are candidates.)"""
    total = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])
    n, begin, out = len(counts), 0, []
    while begin < n:
        end = int(np.searchsorted(total, total[begin] + budget, side="right")) - 1      # the last end that fits
        end = max(end, begin + 1)
        out.append((begin, end))
        begin = end
    return out


def chunk_model(counts, budget):
    return len(chunk_bounds(counts, budget))


def _cols(d):
    return dict(region_id=np.array(d["region_id"], np.int64), id=np.array(d["id"], np.int64), name=list(d["name"]),
                latitude=np.array(d["latitude"], np.float64), longitude=np.array(d["longitude"], np.float64))


def _empty():
    return dict(region_id=[], id=[], name=[], latitude=[], longitude=[])


def _add(side, region, id_, name, lat, lon):
    for key, v in zip(("region_id", "id", "name", "latitude", "longitude"), (region, id_, name, lat, lon)):
        side[key].append(v)


def _shuffled(rng, side):
    order = rng.permutation(len(side["id"]))
    return {k: [v[i] for i in order] for k, v in side.items()}


@functools.lru_cache(maxsize=None)
def chunk_case():
    """One region, a dozen places 2 km apart; place i has CHUNK_COUNTS[i] candidates (confirmed places 1 - 50 m away with
    another id), two confirmed places 100 - 300 m away, and every third place one within the radius that carries its
    own id (a partner of nobody).  About half the candidates are name matches at CHUNK_NAME_DIFFERENCE."""
    rng = np.random.default_rng(12)
    places, conf = _empty(), _empty()
    next_id = 1
    for i, count in enumerate(CHUNK_COUNTS):
        lat, lon, name = 55.0 + 0.02 * i, 37.0, dc.random_name(rng, 14)
        _add(places, 9, 1000 + i, name, lat, lon)
        for c in range(count + 2 + (i % 3 == 0)):
            meters = rng.uniform(1.0, 50.0) if c < count or c == count + 2 else rng.uniform(100.0, 300.0)
            clat, clon = dc.destination(lat, lon, rng.uniform(0, 2 * np.pi), meters)
            cname = dc.with_typos(rng, name, int(rng.integers(0, 4))) if c % 2 == 0 else dc.random_name(rng, 14)
            _add(conf, 9, 1000 + i if c == count + 2 else next_id, cname, clat, clon)
            next_id += 1
    return _cols(places), _cols(_shuffled(rng, conf))


def candidate_counts(places, confirmed, distances, radius):
    """Candidates per place by the restatement's rules: in the region, another id, within the radius."""
    counts = np.zeros(len(places["id"]), np.int64)
    for (i, j), d in distances.items():
        if places["id"][i] != confirmed["id"][j] and d <= radius:
            counts[i] += 1
    return counts


# ---- limit 8: ids at the ends of int64 -----------------------------------------------------------------------------------

ID_RADII = (60.0, -1.0)
ID_NAME_DIFFERENCES = (5, -1)
ID_REGIONS = (INT64_MIN, 5, INT64_MAX)


@functools.lru_cache(maxsize=None)
def id_extremes_case():
    """Three regions (ids INT64_MIN, 5, INT64_MAX) of ten places and ten confirmed places each, all within 15 m of the
    region's centre, ids drawn from INT64_MIN, INT64_MAX, -1, 0, 1 with repeats on both sides.  Sorted by (region, id)
    every region's confirmed rows end with three of id INT64_MAX, and the next region begins with INT64_MIN.  A fourth
    region has places only."""
    rng = np.random.default_rng(8)
    centres = ((55.75, 37.6), (-17.0, 179.9999), (0.0001, -0.0002))
    conf_ids = (INT64_MAX, INT64_MIN, -1, 0, 1, INT64_MAX, INT64_MIN, 0, INT64_MAX, 1)
    place_ids = (INT64_MIN, INT64_MAX, -1, 0, 1, INT64_MAX, INT64_MIN, 2, INT64_MAX, -1)
    places, conf = _empty(), _empty()
    for region, (lat0, lon0) in zip(ID_REGIONS, centres):
        base = dc.random_name(rng, 16)
        for ids, side in ((conf_ids, conf), (place_ids, places)):
            for id_ in ids:
                lat, lon = dc.destination(lat0, lon0, rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 15.0))
                _add(side, region, id_, dc.with_typos(rng, base, int(rng.integers(0, 8))), lat, lon)
    _add(places, 77, INT64_MAX, "nobody is here", 10.0, 10.0)
    return _cols(_shuffled(rng, places)), _cols(_shuffled(rng, conf))


# ---- limit 9: radii near the earth radius --------------------------------------------------------------------------------

WIDE_RADII = (1.0e6, 6_370_999.0)          # 21 bands of 9 degrees; 4 bands of 57.3 degrees with two cells each
REFUSED_RADII = (6_371_000.0, float("inf"), float("nan"))
WIDE_NAME_DIFFERENCE = 3
WIDE_SEED = 9


@functools.lru_cache(maxsize=None)
def wide_radius_case(seed=WIDE_SEED):
    """About 60 places and 60 confirmed places in two regions, uniform over the sphere, with both poles, both sides of
    the antimeridian and the meridian of 0 degrees (the cell boundary where a band has two cells) planted on both sides;
    every other place lies 100 - 1,500 km from a confirmed place.  Names are three words with 0 - 2 typos."""
    rng = np.random.default_rng(seed)
    planted = ((90.0, 0.0), (-90.0, 50.0), (10.0, 180.0), (10.0, -180.0), (-33.0, 179.99), (-33.0, -179.99), (24.0, -0.01),
               (25.0, 0.01), (82.5, -170.0), (-82.5, 170.0), (70.0, 60.0), (-70.0, -60.0))
    words = [dc.random_name(rng, int(rng.integers(7, 10))) for _ in range(3)]
    sides = []
    for first_id in (1, 40):                                   # ids 40 .. 60 are on both sides
        side = _empty()
        spots = list(planted) + [(float(np.degrees(np.arcsin(rng.uniform(-1, 1)))), float(rng.uniform(-180, 180)))
                                 for _ in range(48)]
        if sides:                                              # every other place 100 - 1,500 km from a confirmed place
            there = sides[0]
            for j in range(len(planted), len(spots), 2):
                spots[j] = dc.destination(there["latitude"][j], there["longitude"][j], rng.uniform(0, 2 * np.pi),
                                          rng.uniform(1.0e5, 1.5e6))
        for j, (lat, lon) in enumerate(spots):
            name = dc.with_typos(rng, words[int(rng.integers(len(words)))], int(rng.integers(0, 3)))
            _add(side, (1, 2)[int(rng.integers(2))], first_id + j, name, lat, lon)
        sides.append(_cols(_shuffled(rng, side)))
    return sides[1], sides[0]


# ---- limit 10: one place with many matches -------------------------------------------------------------------------------

CROWD = 600
CROWD_RADIUS = 5000.0
CROWD_NAME_DIFFERENCE = 5


@functools.lru_cache(maxsize=None)
def crowded_place_case():
    """One place at (0, 0) and 600 confirmed places 100 - 4,900 m around it, plus 40 beyond the radius.  The rows are
    laid out by DESCENDING (latitude, longitude) while the grid walk goes through bands and cells ascending (within a
    cell the stable key sort keeps row order), so the walk meets the last rows first and the per-place sort has to move
    nearly every match.  Half the confirmed places inside are name matches."""
    rng = np.random.default_rng(600)
    name = dc.random_name(rng, 18)
    rows = []
    for j in range(CROWD + 40):
        meters = rng.uniform(100.0, 4900.0) if j < CROWD else rng.uniform(5100.0, 9000.0)
        lat, lon = dc.destination(0.0, 0.0, rng.uniform(0, 2 * np.pi), meters)
        cname = dc.with_typos(rng, name, int(rng.integers(0, 5))) if j % 2 == 0 else dc.random_name(rng, 18)
        rows.append((lat, lon, cname))
    rows.sort(key=lambda r: (-r[0], -r[1]))
    conf = _empty()
    for j, (lat, lon, cname) in enumerate(rows):
        _add(conf, 4, j + 1, cname, lat, lon)
    places = _empty()
    _add(places, 4, 5000, name, 0.0, 0.0)
    return _cols(places), _cols(conf)


JOIN_CASES = (("chunks", chunk_case, (CHUNK_RADIUS,)), ("id extremes", id_extremes_case, ID_RADII),
              ("wide radii", wide_radius_case, WIDE_RADII), ("crowded place", crowded_place_case, (CROWD_RADIUS,)))
