"""CPU restatement of the place deduplicator and the seeded cases the device is compared with.  Nothing here uses
the package under test.

    lev               the literal matrix of deduplicator/Levenshtein.scala:18-57, on UTF-16 code units (Java chars)
    lev_rows          the same recurrence one numpy row at a time, for names too long for the literal loops
                      (test_dedup_cases.py checks the two against each other)
    drop_duplicates   the literal double loop of deduplicator/PlaceDeduplicator.scala:25-50 over (place, confirmed
                      place), with the oracle's haversine (oracle_binding.distance_meters) for the distance

A case is a pair of column dicts (places, confirmed): region_id, id, name (Python strings, mixed case), latitude,
longitude."""
import numpy as np

import oracle_binding

EARTH_RADIUS_METERS = 6371.0 * 1000.0
RADII = (-1.0, 0.0, 60.0, 5000.0)            # what test_gpu_dedup.py joins with
NAME_DIFFERENCES = (-1, 0, 2, 5, 20)
MARGIN_METERS = 1e-6                         # no in-region pair may be this close to a radius (test_dedup_cases.py)
SPECIAL_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 5000)


def units(s):
    """UTF-16 code units of a string: what Java's String.charAt sees (a surrogate pair is two)."""
    return np.frombuffer(s.encode("utf-16-le"), dtype=np.uint16)


def csr(names):
    """offsets[n + 1], units[] of the names AS GIVEN (lower-case them first where the deduplicator would)."""
    parts = [units(s) for s in names]
    off = np.zeros(len(parts) + 1, np.int64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    return off, (np.concatenate(parts) if parts else np.zeros(0, np.uint16)).astype(np.uint16)


def lev(str1, str2):
    """Levenshtein.scala:18-57, line by line."""
    s1, s2 = units(str1).tolist(), units(str2).tolist()
    len1, len2 = len(s1), len(s2)
    d = [[0] * (len2 + 1) for _ in range(len1 + 1)]
    for i in range(1, len1 + 1):
        d[i][0] = i
    for j in range(1, len2 + 1):
        d[0][j] = j
    for i in range(1, len1 + 1):
        for j in range(1, len2 + 1):
            replace_cost = 0 if s1[i - 1] == s2[j - 1] else 1
            d_add = d[i - 1][j] + 1
            d_remove = d[i][j - 1] + 1
            d_replace = d[i - 1][j - 1] + replace_cost
            d[i][j] = min(d_add, min(d_remove, d_replace))
    return d[len1][len2]


def lev_rows(str1, str2):
    """The same matrix, row i from row i - 1 with numpy: v(j) = min(d(i-1, j-1) + cost, d(i-1, j) + 1), then the
    left neighbour's `+ 1` chain d(i, j) = min(v(j), d(i, j-1) + 1) is a running minimum of v(j) - j."""
    s1, s2 = units(str1).astype(np.int64), units(str2).astype(np.int64)
    len2 = len(s2)
    js = np.arange(len2 + 1, dtype=np.int64)
    row = js.copy()
    for i in range(1, len(s1) + 1):
        v = np.empty(len2 + 1, np.int64)
        v[0] = i
        v[1:] = np.minimum(row[:-1] + (s2 != s1[i - 1]), row[1:] + 1)
        row = np.minimum.accumulate(v - js) + js
    return int(row[len2])


_LEV_MEMO = {}


def lev_any(str1, str2):
    """lev for short names, lev_rows for long ones; remembered, since the same pairs recur across thresholds."""
    key = (str1, str2)
    if key not in _LEV_MEMO:
        _LEV_MEMO[key] = lev(str1, str2) if len(str1) * len(str2) <= 40_000 else lev_rows(str1, str2)
    return _LEV_MEMO[key]


def location_ok(lat, lon):
    return -90.0 <= lat <= 90.0 and -180.0 <= lon <= 180.0      # Location.scala:7-8 (NaN fails)


class BadLocation(ValueError):
    def __init__(self, side, row):
        super().__init__(f"{side} row {row}")
        self.side, self.row = side, row


def in_region_pairs(places, confirmed):
    """(place row, confirmed row) of equal region_id, place row ascending then confirmed row ascending (:39)."""
    by_region = {}
    for j, r in enumerate(np.asarray(confirmed["region_id"]).tolist()):
        by_region.setdefault(r, []).append(j)
    for i, r in enumerate(np.asarray(places["region_id"]).tolist()):
        for j in by_region.get(r, ()):
            yield i, j


def pair_distances(places, confirmed):
    """{(i, j): oracle distance} of every in-region pair; raises BadLocation as Location's require would."""
    plat, plon = np.asarray(places["latitude"], np.float64), np.asarray(places["longitude"], np.float64)
    clat, clon = np.asarray(confirmed["latitude"], np.float64), np.asarray(confirmed["longitude"], np.float64)
    pairs = list(in_region_pairs(places, confirmed))
    bad_p = [i for i, _ in pairs if not location_ok(plat[i], plon[i])]
    bad_c = [j for _, j in pairs if not location_ok(clat[j], clon[j])]
    if bad_p:
        raise BadLocation("place", min(bad_p))
    if bad_c:
        raise BadLocation("confirmed", min(bad_c))
    return {(i, j): oracle_binding.distance_meters(plat[i], plon[i], clat[j], clon[j]) for i, j in pairs}


def drop_duplicates(places, confirmed, max_meters, max_name_difference, distances=None):
    """-> (same pairs [(place row, confirmed row, name difference)] ordered by (place row, confirmed row),
    not_same_counts[n_places]): the latter is how often dropDuplicates' inner join returns each place."""
    if distances is None:
        distances = pair_distances(places, confirmed)
    pid, cid = np.asarray(places["id"]).tolist(), np.asarray(confirmed["id"]).tolist()
    pname = [s.lower() for s in places["name"]]
    cname = [s.lower() for s in confirmed["name"]]
    same, not_same = [], np.zeros(len(pid), np.int64)
    for (i, j), dist in distances.items():          # join(thatConfirmedPlaces, "region_id") (:39)
        if pid[i] == cid[j]:                        # where(id =!= that_id) (:40)
            continue
        is_not_same = dist > max_meters             # the UDF (:34-35): `||` evaluates lev only when close
        if not is_not_same:
            difference = lev_any(pname[i], cname[j])
            is_not_same = difference > max_name_difference
            if not is_not_same:
                same.append((i, j, difference))
        if is_not_same:
            not_same[i] += 1
    return same, not_same


def min_margin(distances, radii=RADII):
    """The smallest |distance - radius| over all in-region pairs and the radii >= 0 (metres)."""
    d = np.array(list(distances.values()), np.float64)
    if not len(d):
        return np.inf
    return min(float(np.abs(d - r).min()) for r in radii if r >= 0)


# ---- generators --------------------------------------------------------------------------------------------------------

ASCII = "abcdefghijklmnopqrstuvwxyz '-ABCDEFGHKMZ"
CYRILLIC = "абвгдежзийклмнопрстуфхцчшщъыьэюяАБВЖЯ "
ASTRAL = "\U0001F600\U0001F37A\U00010400\U00010428\U0001D11E"      # surrogate pairs; U+10400 lower-cases to U+10428
REGION_IDS = (-7, 0, 3, 2 ** 40, 11)
# (latitude, longitude) a region's places scatter around: a city, the antimeridian, both poles, the equator / prime meridian
CENTRES = ((55.75, 37.6), (-17.0, 179.9995), (90.0, 10.0), (-89.9996, -120.0), (0.0002, -0.0003))


def destination(lat, lon, bearing, meters):
    """The point `meters` away along `bearing` (radians) on the sphere; longitudes wrapped into [-180, 180]."""
    p1, l1, d = np.radians(lat), np.radians(lon), meters / EARTH_RADIUS_METERS
    sin_p2 = np.clip(np.sin(p1) * np.cos(d) + np.cos(p1) * np.sin(d) * np.cos(bearing), -1.0, 1.0)
    p2 = np.arcsin(sin_p2)
    l2 = l1 + np.arctan2(np.sin(bearing) * np.sin(d) * np.cos(p1), np.cos(d) - np.sin(p1) * sin_p2)
    lon2 = (np.degrees(l2) + 180.0) % 360.0 - 180.0
    return float(np.clip(np.degrees(p2), -90.0, 90.0)), float(lon2)


def random_name(rng, length=None):
    pool = (ASCII, ASCII, CYRILLIC, ASCII + ASTRAL)[int(rng.integers(4))]
    if length is None:
        length = int(rng.integers(3, 26))
    out, n = [], 0
    while n < length:
        ch = pool[int(rng.integers(len(pool)))]
        w = 2 if ord(ch) > 0xFFFF else 1
        if n + w > length:
            ch, w = "x", 1
        out.append(ch)
        n += w
    return "".join(out)


def with_typos(rng, name, edits):
    """`edits` random substitutions / insertions / deletions of whole characters (so at most that many differ)."""
    chars = list(name)
    for _ in range(edits):
        kind = int(rng.integers(3))
        at = int(rng.integers(len(chars) + 1))
        if kind == 0 and chars:
            chars[min(at, len(chars) - 1)] = "qZжŋ"[int(rng.integers(4))]
        elif kind == 1:
            chars.insert(at, "wЫ"[int(rng.integers(2))])
        elif chars:
            del chars[min(at, len(chars) - 1)]
    return "".join(chars)


def generated_case(seed, n_places, n_confirmed, spread_meters=3000.0, special_lengths=SPECIAL_LENGTHS):
    """Confirmed places in the first four regions, places in the last four (one region on either side only).  Half the
    places are perturbed copies of a confirmed place of their region: 0.01 - 120 m away, 0 - 8 typos (straddling
    every tested threshold), some in another letter case.  Ids: some places carry the id of the confirmed place they
    copy (never a pair), of a far confirmed place of their region, or of one elsewhere; some confirmed ids repeat."""
    rng = np.random.default_rng(seed)
    conf = dict(region_id=[], id=[], name=[], latitude=[], longitude=[])
    lengths = list(special_lengths)
    for j in range(n_confirmed):
        r = int(rng.integers(4))
        lat0, lon0 = CENTRES[r]
        lat, lon = destination(lat0, lon0, rng.uniform(0, 2 * np.pi), rng.uniform(0.0, spread_meters))
        conf["region_id"].append(REGION_IDS[r])
        conf["id"].append(j + 1 if rng.random() > 0.03 or j == 0 else int(rng.integers(1, j + 1)))
        conf["name"].append(random_name(rng, lengths.pop() if lengths and j % 3 == 0 else None))
        conf["latitude"].append(lat)
        conf["longitude"].append(lon)
    by_region = {}
    for j, r in enumerate(conf["region_id"]):
        by_region.setdefault(r, []).append(j)
    places = dict(region_id=[], id=[], name=[], latitude=[], longitude=[])
    long_rows = [j for j, s in enumerate(conf["name"]) if len(units(s)) > 200]
    for i in range(n_places):
        r = 1 + int(rng.integers(4))
        region = REGION_IDS[r]
        pool = by_region.get(region, [])
        pid = 1_000_000 + i
        if pool and (i % 2 == 0 or (long_rows and i < 8)):
            j = pool[int(rng.integers(len(pool)))]
            if long_rows and i < 8:        # the long names get a copy each while places remain
                cand = [x for x in long_rows if conf["region_id"][x] in REGION_IDS[1:]]
                if cand:
                    j = cand[i % len(cand)]
                    region = conf["region_id"][j]
            lat, lon = destination(conf["latitude"][j], conf["longitude"][j], rng.uniform(0, 2 * np.pi), rng.uniform(0.01, 120.0))
            name = with_typos(rng, conf["name"][j], int(rng.integers(0, 9)))
            if rng.random() < 0.3:
                name = name.upper() if rng.random() < 0.5 else name.swapcase()
            u = rng.random()
            if u < 0.08:
                pid = conf["id"][j]
            elif u < 0.16:
                pid = conf["id"][pool[int(rng.integers(len(pool)))]]
            elif u < 0.2:
                pid = conf["id"][int(rng.integers(n_confirmed))]
        else:
            lat0, lon0 = CENTRES[r]
            lat, lon = destination(lat0, lon0, rng.uniform(0, 2 * np.pi), rng.uniform(0.0, spread_meters))
            name = random_name(rng)
        places["region_id"].append(region)
        places["id"].append(pid)
        places["name"].append(name)
        places["latitude"].append(lat)
        places["longitude"].append(lon)

    def cols(d):
        return dict(region_id=np.array(d["region_id"], np.int64), id=np.array(d["id"], np.int64), name=list(d["name"]),
                    latitude=np.array(d["latitude"], np.float64), longitude=np.array(d["longitude"], np.float64))
    return cols(places), cols(conf)


# (seed, places, confirmed places, scatter radius of a region in metres): the cases test_gpu_dedup.py runs.  Every one
# of them passes test_dedup_cases.py's margin condition; a seed that does not is replaced, never waived.
CASES = ((1, 1200, 400, 3000.0), (2, 300, 900, 800.0), (3, 40, 12, 200.0), (6, 1, 1, 50.0), (5, 700, 60, 150.0))


def adversarial_strings():
    """Pairs for locrec_lev_distances: the band's edges (lengths 2k + 1 around k = 3 / 7 / 15), all-different and
    all-equal names, one-sided empties, shifts (the optimal path runs along the band's edge), long names on every
    tier (LDS row below 1,280 units, global row above), and surrogate pairs that differ in one unit only."""
    rng = np.random.default_rng(99)
    pairs = [("sitting", "kitten"), ("", "kitten"), ("sitting", ""), ("", ""), ("sitting", "sitting"),
             ("\U0001F600", "\U0001F601"), ("a\U00010428b", "a\U00010429b"), ("ёж", "еж")]
    for n in (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 41, 63, 64, 65, 127, 128, 129):
        base = random_name(rng, n)
        pairs.append((base, base))
        pairs.append((base, "#" * n))                                 # nothing in common
        pairs.append((base, base[1:] + "#"))                          # a shift by one
        for sh in (3, 4, 7, 8, 15, 16):
            if sh < n:
                pairs.append((base, base[sh:]))                       # exactly `sh` deletions at the front
                pairs.append((base[:-sh], "#" * sh + base[:-sh]))     # ... insertions
        for e in (1, 3, 4, 5, 8, 16, 17, 41):
            pairs.append((base, with_typos(rng, base, e)))
    for n in (700, 1279, 1280, 1281, 5000):
        base = random_name(rng, n)
        pairs.append((base, with_typos(rng, base, 6)))
        pairs.append((with_typos(rng, base, 30), base))
    pairs.append((random_name(rng, 5000), random_name(rng, 12)))
    pairs.append((random_name(rng, 900), random_name(rng, 1100)))
    return pairs
