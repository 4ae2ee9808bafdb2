"""Inputs of the near ranker's tests (locrec_rank_recommendations_batch_near): rank_batch_cases' and rank_exclude_cases'
cases with coordinates for the place table and a circle per segment.  Seeded generators, no GPU.  A case is their dict
plus lat, lon (one per row of the place table) and clat, clon, radius (one per segment).

The expected value is composed of existing code: a keep mask per (segment, place row) from a haversine that is NOT the
code under test (distance <= radius), the place table cut to the kept rows, and an existing single ranker applied per
segment - to the rows that survive the exclusion list where the case has lists."""
import numpy as np

import rank_batch_cases as rb
import rank_exclude_cases as rx

BOX = 0.03                                      # degrees, both ways
# region -> the box's south-west corner: Paris; against the pole; across the antimeridian (longitudes wrapped)
CORNERS = {0: (48.85, 2.30), 1: (89.97, -30.0), 2: (-33.90, 179.985)}
RADII = (0.0, 60.0, 400.0, 1500.0, 20000.0, np.inf)
NORTH = 0.002                                   # degrees: the third kind of centre lies this far north of a place
LIMITS = (1, 10, 256, 257, 2 ** 40)
CLEAR_METERS = 1e-3                             # no (centre, place) pair of a case lies this close to its radius


def wrap(lon):
    return np.where(lon > 180.0, lon - 360.0, lon)


def coordinates(seed, regions):
    """One point per row of the place table, uniform inside its region's box: a place listed twice gets two points."""
    rng = np.random.default_rng(3000 + seed)
    u, v = rng.random(len(regions)), rng.random(len(regions))
    lat0 = np.array([CORNERS[int(r)][0] for r in regions])
    lon0 = np.array([CORNERS[int(r)][1] for r in regions])
    return np.minimum(lat0 + BOX * u, 90.0), wrap(lon0 + BOX * v)


def circles(seed, case, lat, lon):
    """Per segment a centre - on a place of the target region, the box centre, NORTH degrees north of a place, in turn -
    and a radius, RADII in turn starting at the seed.  A target that is no region gets region 0's box."""
    rng = np.random.default_rng(5000 + seed)
    nseg = len(case["targets"])
    clat, clon, radius = np.zeros(nseg), np.zeros(nseg), np.zeros(nseg)
    for s in range(nseg):
        t = int(case["targets"][s])
        rows = np.flatnonzero(case["regions"] == t)
        corner = CORNERS.get(t, CORNERS[0])
        kind = s % 3 if len(rows) else 1
        if kind == 1:
            clat[s], clon[s] = corner[0] + BOX / 2, float(wrap(np.float64(corner[1] + BOX / 2)))
        else:
            j = rows[int(rng.integers(0, len(rows)))]
            clat[s], clon[s] = min(lat[j] + (NORTH if kind == 2 else 0.0), 90.0), lon[j]
        radius[s] = RADII[(seed + s) % len(RADII)]
    return clat, clon, radius


def with_circles(case, seed):
    lat, lon = coordinates(seed, case["regions"])
    clat, clon, radius = circles(seed, case, lat, lon)
    return dict(case, lat=lat, lon=lon, clat=clat, clon=clon, radius=radius)


def fuzz_case(seed, lists=False):
    """rank_batch_cases.fuzz_case(seed) - with lists: rank_exclude_cases.fuzz_case(seed) - plus coordinates and circles."""
    return with_circles(rx.fuzz_case(seed) if lists else rb.fuzz_case(seed), seed)


def elementwise(distance):
    """A haversine of four scalars (the oracle's) as one of four arrays."""
    return lambda lat1, lon1, lat2, lon2: np.array([distance(*x) for x in zip(lat1, lon1, lat2, lon2)], np.float64)


def region_rows(case, s):
    return np.flatnonzero(case["regions"] == case["targets"][s])


def distances(distance, case, s):
    """(rows of the place table in segment s's target region, their distance from the segment's centre)."""
    rows = region_rows(case, s)
    n = len(rows)
    d = distance(np.full(n, case["clat"][s]), np.full(n, case["clon"][s]), case["lat"][rows], case["lon"][rows]) if n else np.empty(0)
    return rows, np.asarray(d, np.float64)


def kept_rows(distance, case, s):
    """The rows of the place table inside segment s's circle, in input order, with their distances."""
    rows, d = distances(distance, case, s)
    keep = d <= case["radius"][s]
    return rows[keep], d[keep]


def all_kept(distance, case):
    """kept_rows of every segment, from ONE call of `distance` over all (segment, place of its region) pairs."""
    rows = [region_rows(case, s) for s in range(len(case["targets"]))]
    seg = np.concatenate([np.full(len(r), s) for s, r in enumerate(rows)] + [np.empty(0, np.int64)]).astype(np.int64)
    flat = np.concatenate(rows + [np.empty(0, np.int64)]).astype(np.int64)
    d = np.asarray(distance(case["clat"][seg], case["clon"][seg], case["lat"][flat], case["lon"][flat]), np.float64) if len(flat) \
        else np.empty(0)
    keep = d <= case["radius"][seg]
    return [(flat[keep & (seg == s)], d[keep & (seg == s)]) for s in range(len(rows))]


def expected(rank, distance, case, limit, kept=None):
    """-> (ids[S, W], scores[S, W], meters[S, W], counts[S]): per segment `rank` on the (surviving) rows against the place
    table cut to the rows inside the circle; meters from the FIRST kept listing of each output id.  W is the limit cut to
    the longest segment before any filter, as the call cuts it."""
    off, nseg = case["offsets"], len(case["targets"])
    width = rx.width_of(case, limit)
    out_ids, out_scores, out_meters = np.full((nseg, width), -1, np.int64), np.zeros((nseg, width)), np.zeros((nseg, width))
    counts = np.zeros(nseg, np.int64)
    for s in range(nseg):
        ids, scores = case["ids"][off[s]:off[s + 1]], case["scores"][off[s]:off[s + 1]]
        if "ex_ids" in case:
            keep = ~np.isin(ids, rx.list_of(case, s))
            ids, scores = ids[keep], scores[keep]
        rows, d = kept[s] if kept is not None else kept_rows(distance, case, s)
        ri, rs = rank(ids, scores, case["place_ids"][rows], case["regions"][rows], int(case["targets"][s]), width)
        counts[s] = len(ri)
        out_ids[s, :len(ri)], out_scores[s, :len(ri)] = ri, rs
        pid = case["place_ids"][rows]
        for j, i in enumerate(np.asarray(ri)):
            out_meters[s, j] = d[np.flatnonzero(pid == i)[0]]
    return out_ids, out_scores, out_meters, counts


def same(got, want):
    """Equal ids, counts, score bits and distance bits."""
    gi, gs, gm, gc = (np.asarray(x) for x in got)
    wi, ws, wm, wc = want
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    return rb.same((gi, gs, gc), (wi, ws, wc)) and gm.shape == wm.shape and np.array_equal(bits(gm), bits(wm))


def args(case, limit):
    """prep.rank_recommendations_batch_near's positional arguments (the lists, where the case has them, as keywords)."""
    a = [case[k] for k in ("offsets", "ids", "scores", "place_ids", "regions", "lat", "lon", "targets", "clat", "clon", "radius")]
    kw = dict(excluded_offsets=case["ex_offsets"], excluded_ids=case["ex_ids"]) if "ex_ids" in case else {}
    return a + [limit], kw


def all_inf(case):
    return dict(case, radius=np.full(len(case["targets"]), np.inf))


def one_point_seam(chunks=3, meters_off=0.0):
    """rank_batch_cases.seam_case with every place on one point and radius 0: the centre on that point keeps all rows,
    a centre about meters_off metres north of it none."""
    case = rb.seam_case(chunks)
    n = len(case["place_ids"])
    lat, lon = np.full(n, 48.86), np.full(n, 2.31)
    return dict(case, lat=lat, lon=lon, clat=np.array([48.86 + meters_off / 111_195.0]), clon=np.array([2.31]),
                radius=np.zeros(1))
