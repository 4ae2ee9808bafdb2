"""Inputs of the producers (csrc/prep.hip) that stand exactly ON the limits of the spatial join's grid, the co-visit
join's pair keys, tiles and counts, the capacity protocol and the final ranking's score order ("Limits of
the producers").  Shared by the CPU checks of the cases themselves (test_prep_limit_cases.py) and the GPU tests
(test_gpu_prep_limits.py).  No GPU and no package import: plain numpy and math.

The grid is restated here from the comments of prep.hip and DESIGN.md section 9, with its constants as literals: a
test that asks the library where its limit lies cannot catch a moved limit.

A join case is a dict

    name, radius, visits, places, visits_from      the arguments of calc_place_visits (columns as numpy arrays)
    groups   [{"name", "visit": row, "place": row, "near": [place rows], "claim": {...}}]
             (visit, place) is the DECISIVE pair: the oracle matches it, and it stands where `claim` says (bands and
             cells of the two points, checked from the grid arithmetic by the CPU test); `near` are near misses: places
             of the same region that the oracle rejects.  Every group has a region of its own, so groups do not meet.

Every visit-place distance inside a region is at least MARGIN_M = 1e-3 m away from the radius - a thousand times what
libm and the device's sin / cos / asin can differ by - so the GPU comparison is exact.  The one exception is radius
0.0, where a match has distance exactly 0.0 by arithmetic (equal coordinates: every difference is 0, sin(0) = 0,
sqrt(0) = 0, asin(0) = 0 in any math library)."""
import math

import numpy as np

EARTH_RADIUS_M = 6371000.0                 # Location.scala:28
PI = 3.14159265358979323846
CELL_BITS = 20                             # bands and cells per band: < 2^20 each
MPD = EARTH_RADIUS_M * PI / 180.0          # metres per degree of a great circle
MARGIN_M = 1e-3
PAIR_TILE = 2048                           # pair keys one block of pr_covisit_emit writes
DEFAULT_PAIR_BUDGET = 1 << 28              # candidate pairs per chunk
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
T0 = 1_600_000_000_000

BAND_CLAMP_DEG = 180.0 / (2 ** 20 - 2)     # the band height never falls below this
CELL_CLAMP_DEG = 360.0 / (2 ** 20 - 1)     # a cell is never narrower than this
LARGEST_RADIUS = float(np.nextafter(EARTH_RADIUS_M, 0.0))       # the ABI accepts [0, 6 371 000)


# ---- the grid, restated -----------------------------------------------------------------------------------------------

def radians(deg):
    return deg / 180.0 * PI


def distance(lat1, lon1, lat2, lon2):
    """Location.distanceMeters (Location.scala:30-43) in libm arithmetic (the oracle is the judge; this places points)."""
    la1, la2, lo1, lo2 = radians(lat1), radians(lat2), radians(lon1), radians(lon2)
    h = math.sin((la2 - la1) / 2) ** 2 + math.cos(la1) * math.cos(la2) * math.sin((lo2 - lo1) / 2) ** 2
    return 2 * EARTH_RADIUS_M * math.asin(math.sqrt(h))


class Grid:
    """Latitude bands of band_deg degrees, at least the radius as an angle and at least BAND_CLAMP_DEG; band b is cut
    into nx(b) cells of 360 / nx(b) degrees, each at least as wide as the largest longitude difference of a match whose
    place is in band b and whose visit is in bands b - 1 .. b + 1, and at most 2^20 - 1 of them."""

    def __init__(self, radius):
        ang = radius / EARTH_RADIUS_M
        self.unclamped_band_deg = ang * (180.0 / PI) * (1.0 + 1e-9) + 1e-12
        self.band_deg = max(self.unclamped_band_deg, 180.0 / ((1 << CELL_BITS) - 2))
        self.nbands = int(math.floor(180.0 / self.band_deg)) + 1
        self.sin_half = math.sin(ang / 2) * (1.0 + 1e-9)

    def band_of(self, lat):
        return min(max(int(math.floor((lat + 90.0) / self.band_deg)), 0), self.nbands - 1)

    def cells(self, b):
        """(longitude half-window in degrees, number of cells) of band b."""
        lo, hi = -90.0 + (b - 1) * self.band_deg, -90.0 + (b + 2) * self.band_deg
        latmax = min(max(abs(lo), abs(hi)), 90.0)
        c = math.cos(radians(latmax))
        win = 180.0
        if c > 0.0:
            ratio = self.sin_half / c
            if ratio < 1.0:
                win = min(180.0, 2.0 * math.asin(ratio) * (180.0 / PI) * (1.0 + 1e-9) + 1e-12)
        return win, int(min(max(math.floor(360.0 / win), 1.0), float((1 << CELL_BITS) - 1)))

    def unclamped_cells(self, b):
        win, _ = self.cells(b)
        return int(math.floor(360.0 / win))

    def cell_of(self, lat, lon):
        """(band, cell) a place is filed under."""
        b = self.band_of(lat)
        _, nx = self.cells(b)
        return b, min(max(int(math.floor((lon + 180.0) / (360.0 / nx))), 0), nx - 1)

    def scan(self, lat, lon):
        """The (band, cell) sequence a visit looks at, in the kernel's order."""
        out = []
        bv = self.band_of(lat)
        for b in range(max(bv - 1, 0), min(bv + 1, self.nbands - 1) + 1):
            win, nx = self.cells(b)
            w = 360.0 / nx
            c_lo, c_hi = int(math.floor((lon - win + 180.0) / w)), int(math.floor((lon + win + 180.0) / w))
            for t in range(min(c_hi - c_lo + 1, nx)):
                out.append((b, ((c_lo + t) % nx + nx) % nx))
        return out

    def band_mid(self, b):
        lo = -90.0 + b * self.band_deg
        return (lo + min(lo + self.band_deg, 90.0)) / 2


def band_clamp_radius():
    """The radius whose angle is the clamped band height: pi R / (2^20 - 2), about 19.09 m."""
    return BAND_CLAMP_DEG / (180.0 / PI) * EARTH_RADIUS_M


def cell_clamp_radius():
    """The radius below which the equator's bands would get more than 2^20 - 1 cells: 2 pi R / (2^20 - 1), about 38.2 m."""
    return CELL_CLAMP_DEG / (180.0 / PI) * EARTH_RADIUS_M


# ---- join cases ---------------------------------------------------------------------------------------------------------

class _Join:
    def __init__(self, name, radius):
        self.name, self.radius, self.grid = name, float(radius), Grid(float(radius))
        self.v, self.p, self.groups = [], [], []

    def region(self, k):
        return (5 + 3 * k) * (-1 if k % 2 else 1)

    def add(self, name, visit, place, near=(), claim=None, more_places=()):
        k = len(self.groups)
        reg = self.region(k)
        self.v.append((2040 + len(self.v), T0 + len(self.v), visit[0], visit[1], reg))
        rows = []
        for lat, lon in [place, *near, *more_places]:
            rows.append(len(self.p))
            self.p.append((40 + len(self.p), lat, lon, reg, len(self.p) % 20))
        self.groups.append({"name": name, "visit": len(self.v) - 1, "place": rows[0], "near": rows[1:1 + len(near)],
                            "claim": dict(claim or {})})

    def finish(self, seed=1):
        return finish_join(self.name, self.radius, self.v, self.p, self.groups, T0, seed)


def finish_join(name, radius, v, p, groups, visits_from, seed):
    """Columns from row tuples; the place rows are permuted, so place-row order is not grid order."""
    perm = np.random.default_rng(seed).permutation(len(p))
    inv = np.argsort(perm)
    p = [p[i] for i in perm]
    for g in groups:
        g["place"] = int(inv[g["place"]])
        g["near"] = [int(inv[r]) for r in g["near"]]
    visits = {"person_id": np.array([r[0] for r in v], np.int64), "timestamp": np.array([r[1] for r in v], np.int64),
              "latitude": np.array([r[2] for r in v], np.float64), "longitude": np.array([r[3] for r in v], np.float64),
              "region_id": np.array([r[4] for r in v], np.int64)}
    places = {"id": np.array([r[0] for r in p], np.int64), "latitude": np.array([r[1] for r in p], np.float64),
              "longitude": np.array([r[2] for r in p], np.float64), "region_id": np.array([r[3] for r in p], np.int64),
              "category_id": np.array([r[4] for r in p], np.int64)}
    return {"name": name, "radius": float(radius), "visits": visits, "places": places, "visits_from": int(visits_from),
            "groups": groups}


def _meridian_miss(lat, r, factor, towards):
    """A latitude `factor` radii from lat along the meridian, on the side `towards` (+1 / -1) if that stays on the chart."""
    out = lat + towards * factor * r / MPD
    return out if abs(out) <= 90.0 else lat - towards * factor * r / MPD


def band_edge_group(J, edge, visit_below, lon=37.62):
    """Decisive pair half a radius apart on one meridian, on opposite sides of the edge between bands edge - 1 and edge."""
    g, r = J.grid, J.radius
    e = -90.0 + edge * g.band_deg
    a = 0.25 * r / MPD
    lo_lat, hi_lat = e - a, e + min(a, (90.0 - e) / 2)
    v, p = (lo_lat, hi_lat) if visit_below else (hi_lat, lo_lat)
    side = 1 if p > v else -1
    near = [(_meridian_miss(v, r, 1.5, side), lon), (_meridian_miss(v, r, 3.5, -side), lon)]
    J.add(f"band edge {edge}, visit {'below' if visit_below else 'above'}", (v, lon), (p, lon), near,
          {"bands": (edge - 1, edge) if visit_below else (edge, edge - 1)})


def full_span_group(J, edge, upward, lon=-78.5):
    """Decisive pair radius - 2 mm apart on one meridian, the visit 0.1 mm from the edge: with bands at least one radius
    high they are in neighbouring bands; with bands 2 mm too low they would be two bands apart and never meet.  The near
    miss is radius + 2 mm away."""
    g, r = J.grid, J.radius
    e = -90.0 + edge * g.band_deg
    tiny, span, over = 1e-4 / MPD, (r - 2e-3) / MPD, (r + 2e-3) / MPD
    if upward:
        v = e - tiny
        J.add(f"full span up from edge {edge}", (v, lon), (v + span, lon), [(v + over, lon)], {"bands": (edge - 1, edge)})
    else:
        v = e + tiny
        J.add(f"full span down from edge {edge}", (v, lon), (v - span, lon), [(v - over, lon)], {"bands": (edge, edge - 1)})


def _wrap(lon):
    return lon + 360.0 if lon < -180.0 else lon - 360.0 if lon > 180.0 else lon


def cell_edge_group(J, b, c, visit_west):
    """Decisive pair half a radius apart on the mid latitude of band b, on opposite sides of the western edge of cell c
    (c = 0: the antimeridian, longitudes 179.99.. against -179.99..)."""
    g, r = J.grid, J.radius
    _, nx = g.cells(b)
    lat = g.band_mid(b)
    edge_lon = c * (360.0 / nx) - 180.0
    a = min(0.25 * r / (MPD * max(math.cos(radians(lat)), 1e-300)), 40.0)
    west, east = _wrap(edge_lon - a), edge_lon + a
    v, p = (west, east) if visit_west else (east, west)
    step = 1.5 * r / (MPD * max(math.cos(radians(lat)), 1e-300))
    if step < 60.0:
        near = [(lat, _wrap(v + (step if visit_west else -step)))]
    else:
        near = [(_meridian_miss(lat, r, 1.5, -1 if lat > 0 else 1), v)]
    cells = ((c - 1) % nx, c) if visit_west else (c, (c - 1) % nx)
    J.add(f"cell edge {c} of {nx} in band {b}, visit {'west' if visit_west else 'east'}", (lat, v), (lat, p), near,
          {"bands": (b, b), "cells": cells, "wrap": c == 0})


def exact_antimeridian_group(J, b, visit_at_plus):
    """Longitudes 180.0 and -180.0 exactly: one meridian, the last cell and the first."""
    g, r = J.grid, J.radius
    _, nx = g.cells(b)
    lat = g.band_mid(b)
    v, p = (180.0, -180.0) if visit_at_plus else (-180.0, 180.0)
    d = 0.2 * min(r / MPD, g.band_deg)
    J.add(f"longitude {v} against {p} in band {b}", (lat, v), (lat + d, p), [(_meridian_miss(lat, r, 1.5, -1 if lat > 0 else 1), p)],
          {"bands": (b, b), "cells": (nx - 1, 0) if visit_at_plus else (0, nx - 1), "wrap": True})


def window_group(J, b, c):
    """Decisive pair radius - 2 mm apart along the mid latitude of band b, astride the western edge of cell c with the
    visit half the difference inside cell c: a window of half the needed width ends inside the visit's own cell."""
    g, r = J.grid, J.radius
    _, nx = g.cells(b)
    lat = g.band_mid(b)
    edge_lon = c * (360.0 / nx) - 180.0
    cl = math.cos(radians(lat))
    dlon = 2 * math.asin(math.sin((r - 2e-3) / (2 * EARTH_RADIUS_M)) / cl) * (180.0 / PI)
    over = 2 * math.asin(math.sin((r + 2e-3) / (2 * EARTH_RADIUS_M)) / cl) * (180.0 / PI)
    v = edge_lon + dlon / 2
    J.add(f"full window across cell edge {c} in band {b}", (lat, v), (lat, _wrap(v - dlon)), [(lat, _wrap(v - over))],
          {"bands": (b, b), "cells": (c, (c - 1) % nx)})


def pole_groups(J, s):
    """s = +1 / -1: latitude exactly +-90 with unrelated longitudes on both sides, and a pair across the pole."""
    r = J.radius
    pole, name = s * 90.0, "north" if s > 0 else "south"
    J.add(f"both at the {name} pole, unrelated longitudes", (pole, 13.0), (pole, -100.0), [(s * (90.0 - 1.5 * r / MPD), 77.0)],
          {"pole": s})
    J.add(f"place at the {name} pole", (s * (90.0 - 0.5 * r / MPD), 140.0), (pole, -100.0), [(s * (90.0 - 1.6 * r / MPD), -40.0)],
          {"pole": s})
    J.add(f"visit at the {name} pole", (pole, -179.0), (s * (90.0 - 0.5 * r / MPD), 55.0), [(s * (90.0 - 1.2 * r / MPD), 55.0)],
          {"pole": s})
    J.add(f"across the {name} pole", (s * (90.0 - 0.3 * r / MPD), 20.0), (s * (90.0 - 0.3 * r / MPD), -160.0),
          [(s * (90.0 - 0.8 * r / MPD), -160.0)], {"pole": s, "opposite": True})


def first_band_with_more_cells(grid):
    """The highest band that has more than the two cells of the bands next to the pole."""
    b = grid.nbands - 1
    while grid.cells(b)[1] <= 2:
        b -= 1
    return b


def standard_case(name, radius):
    """Band edges (first two, middle, last two bands; both directions), cell edges (interior and the antimeridian, both
    directions, +-180.0 exactly), full-span pairs, both poles and the highest bands, at one radius up to 50 km."""
    J = _Join(name, radius)
    g = J.grid
    for edge in (1, 2, g.nbands // 2, g.nbands - 2, g.nbands - 1):
        for visit_below in (True, False):
            band_edge_group(J, edge, visit_below)
    full_span_group(J, 1, True)
    full_span_group(J, g.nbands // 2 + 3, True)
    full_span_group(J, g.nbands // 2 - 3, False)
    full_span_group(J, g.nbands - 2, False)
    for b in (g.band_of(0.0), g.band_of(55.75), g.band_of(-60.0)):
        nx = g.cells(b)[1]
        for c in (nx // 3, 0):
            for visit_west in (True, False):
                cell_edge_group(J, b, c, visit_west)
        for visit_at_plus in (True, False):
            exact_antimeridian_group(J, b, visit_at_plus)
        window_group(J, b, nx // 5)
        window_group(J, b, 0)
    for s in (1, -1):
        pole_groups(J, s)
    top = first_band_with_more_cells(g)
    for b in (g.nbands - 1, top + 1, top, 0):
        for c in (1, 0):
            for visit_west in (True, False):
                cell_edge_group(J, b, c, visit_west)
    return J.finish()


STANDARD_RADII = {
    "100 m": 100.0,
    "below the band clamp": band_clamp_radius() * (1 - 1e-4),
    "above the band clamp": band_clamp_radius() * (1 + 1e-4),
    "below the cell clamp": cell_clamp_radius() * (1 - 1e-4),
    "above the cell clamp": cell_clamp_radius() * (1 + 1e-4),
    "1 km": 1000.0,
    "50 km": 50_000.0,
}


def radius_zero_case():
    """Radius 0.0: only coincident points match (distance exactly 0.0), also where one side writes its zeros as -0.0;
    the near misses are 1 cm away."""
    J = _Join("radius 0", 0.0)
    cm = 0.01 / MPD
    for lat, lon in ((55.75, 37.62), (0.0, 0.0), (90.0, 13.0), (-90.0, -170.0), (12.0, 180.0), (-33.0, -180.0), (0.0, -78.5)):
        J.add(f"coincident at {lat}, {lon}", (lat, lon), (lat, lon), [(lat - cm if lat > 0 else lat + cm, lon)], {"same": True})
    J.add("-0.0 against 0.0", (-0.0, -0.0), (0.0, 0.0), [(cm, 0.0)], {"same": True})
    J.add("0.0 against -0.0", (0.0, 12.5), (-0.0, 12.5), [(-cm, 12.5)], {"same": True})
    return J.finish()


def _destination(lat, lon, metres, bearing):
    la, d = math.radians(lat), metres / EARTH_RADIUS_M
    la2 = math.asin(min(1.0, max(-1.0, math.sin(la) * math.cos(d) + math.cos(la) * math.sin(d) * math.cos(bearing))))
    lo2 = math.radians(lon) + math.atan2(math.sin(bearing) * math.sin(d) * math.cos(la), math.cos(d) - math.sin(la) * math.sin(la2))
    return math.degrees(la2), (math.degrees(lo2) + 180.0) % 360.0 - 180.0


SPHERE_RADII = (1000.0, 50_000.0, 1_000_000.0, 3_000_000.0, 6_000_000.0, LARGEST_RADIUS)


def sphere_case(radius, seed=3, n=300):
    """n visits uniform over the whole sphere plus the poles and the antimeridian exactly; one place 0 .. 2.5 radii from
    every visit (both outcomes frequent at any radius) and as many uniform ones, two regions.  Places within MARGIN_M
    of the radius of any visit of their region are left out, so no decision is near the threshold."""
    rng = np.random.default_rng(seed)
    vlat = np.degrees(np.arcsin(rng.uniform(-1, 1, n))).tolist() + [90.0, -90.0, 0.0, 0.0, 45.0, -45.0]
    vlon = rng.uniform(-180, 180, n).tolist() + [13.0, -170.0, 180.0, -180.0, 180.0, -180.0]
    vreg = rng.integers(0, 2, len(vlat)).tolist()
    cand = [_destination(la, lo, rng.random() * 2.5 * radius, rng.random() * 2 * math.pi) for la, lo in zip(vlat, vlon)]
    cand += list(zip(np.degrees(np.arcsin(rng.uniform(-1, 1, n))).tolist(), rng.uniform(-180, 180, n).tolist()))
    cand += [(90.0, -100.0), (-90.0, 20.0), (0.0, -180.0), (0.0, 180.0), (-45.0, 180.0)]
    preg = vreg + rng.integers(0, 2, len(cand) - len(vreg)).tolist()       # the near place shares its visit's region
    v = [(2040 + i, T0 + i, la, lo, reg) for i, (la, lo, reg) in enumerate(zip(vlat, vlon, vreg))]
    p = []
    for (la, lo), reg in zip(cand, preg):
        la = min(max(la, -90.0), 90.0)
        if all(abs(distance(a, b, la, lo) - radius) >= 10 * MARGIN_M for a, b, r2 in zip(vlat, vlon, vreg) if r2 == reg):
            p.append((40 + len(p), la, lo, reg, len(p) % 20))
    return finish_join(f"sphere {radius:g} m", radius, v, p, [], T0, seed)


def _disc(rng, lat, lon, n, r_lo, r_hi, radius):
    out = []
    while len(out) < n:
        d, a = math.sqrt(rng.uniform(r_lo ** 2, r_hi ** 2)), rng.uniform(0, 2 * math.pi)
        q = (lat + d * math.cos(a) / MPD, lon + d * math.sin(a) / (MPD * math.cos(radians(lat))))
        if abs(distance(lat, lon, *q) - radius) >= 10 * MARGIN_M:
            out.append(q)
    return out


def _cell_centre(grid, lat, lon):
    b, c = grid.cell_of(lat, lon)
    return grid.band_mid(b), (c + 0.5) * (360.0 / grid.cells(b)[1]) - 180.0


def many_matches_case():
    """One visit with 3,000 matches in its own cell, one with 600 spread over all nine cells around it (and 200 near
    misses each), at 100 m: the per-visit insertion sort and the output order."""
    J = _Join("many matches", 100.0)
    rng = np.random.default_rng(5)
    lat, lon = _cell_centre(J.grid, 0.3, 101.7)
    pts = _disc(rng, lat, lon, 3000, 0.0, 40.0, 100.0)
    J.add("3000 matches in one cell", (lat, lon), pts[0], _disc(rng, lat, lon, 200, 101.0, 150.0, 100.0), {"one_cell": True},
          more_places=pts[1:])
    lat, lon = _cell_centre(J.grid, -0.2, -64.1)
    pts = _disc(rng, lat, lon, 600, 0.0, 99.0, 100.0)
    J.add("600 matches in nine cells", (lat, lon), pts[0], _disc(rng, lat, lon, 200, 101.0, 150.0, 100.0), {"nine_cells": True},
          more_places=pts[1:])
    return J.finish(seed=6)


def capacity_case():
    """Five visits at the centres of their cells with 12 places each within 99 m (and three near misses): every visit's
    matches lie in three or more cells, and their scan order (band, then cell) is not their place-row order.  The GPU
    test asks for every capacity from 0 to the total."""
    J = _Join("capacity", 100.0)
    rng = np.random.default_rng(8)
    for k, (la, lo) in enumerate(((0.3, 10.0), (-0.4, 10.0), (0.3, -120.0), (20.0, 77.0), (-35.0, -3.0))):
        lat, lon = _cell_centre(J.grid, la, lo)
        pts = _disc(rng, lat, lon, 12, 30.0, 99.0, 100.0)
        J.add(f"visit {k}", (lat, lon), pts[0], _disc(rng, lat, lon, 3, 101.0, 150.0, 100.0), {"cells_at_least": 3}, more_places=pts[1:])
    return J.finish(seed=9)


def misc_case():
    """Duplicate visit rows, duplicate place ids, a timestamp equal to visits_from and one below it, regions -2^63 and
    2^63 - 1, a region with places and no visits and one with visits and no places.  -> (case, expected match count)"""
    lat, lon, step = 55.75, 37.62, 30.0 / MPD
    visits_from = T0 + 100
    v = [(1, visits_from, lat, lon, I64_MIN),               # timestamp == visits_from: kept
         (2, visits_from - 1, lat, lon, I64_MIN),           # one below: dropped
         (3, visits_from + 5, lat, lon, I64_MAX),
         (3, visits_from + 5, lat, lon, I64_MAX),           # the same row twice: both joined
         (4, I64_MAX, lat + step, lon, I64_MAX),
         (5, I64_MIN, lat, lon, I64_MAX),                   # the smallest timestamp: dropped
         (6, visits_from + 7, lat, lon, 8)]                 # a region without places
    p = [(40, lat + step, lon, I64_MIN, 1), (40, lat - step, lon, I64_MIN, 2),      # one id twice, two spots: two rows out
         (41, lat + 5 * step, lon, I64_MIN, 3),                                     # 150 m: rejected
         (I64_MAX, lat, lon + step, I64_MAX, I64_MIN), (I64_MIN, lat, lon - step, I64_MAX, I64_MAX),
         (42, lat + 6 * step, lon, I64_MAX, 4),
         (43, lat, lon, 7, 5), (44, lat, lon, 7, 6)]                                # a region nobody visits
    groups = [{"name": "timestamp == visits_from", "visit": 0, "place": 0, "near": [2], "claim": {}},
              {"name": "region 2^63 - 1", "visit": 2, "place": 3, "near": [5], "claim": {}}]
    return finish_join("misc", 100.0, v, p, groups, visits_from, 4), 2 + 2 + 2 + 2


def join_cases():
    """name -> builder, for the parametrised tests."""
    out = {f"standard, {k}": (lambda k=k: standard_case(k, STANDARD_RADII[k])) for k in STANDARD_RADII}
    out["radius 0"] = radius_zero_case
    out["many matches"] = many_matches_case
    out["misc"] = lambda: misc_case()[0]
    return out


# ---- co-visit cases ---------------------------------------------------------------------------------------------------

def clusters(sizes, n_places, seed=0, first_person=100):
    """Person k has sizes[k] rows at one timestamp (an interval of 0 pairs them all): sorted by (person, timestamp), each
    of its rows has sizes[k] - 1 partners.  Places cycle through n_places ids (negative ones too), so a person of more
    rows than places pairs a place with itself; rows shuffled.  -> (person, place, timestamp)"""
    person = np.repeat(first_person + np.arange(len(sizes), dtype=np.int64), sizes)
    n = len(person)
    place = (np.arange(n, dtype=np.int64) % n_places) * 3 - n_places
    ts = T0 + person * 10
    order = np.random.default_rng(seed).permutation(n)
    return person[order], place[order], ts[order]


def windows(person, place, ts, interval):
    """The window arithmetic of the co-visit join: rows in (person, timestamp) order; width[i] = the rows of the same
    person within `interval` of row i, itself excluded; off = exclusive sum, off[n] = all candidate pairs."""
    order = np.lexsort((ts, person))
    p, t = np.asarray(person)[order], np.asarray(ts)[order]
    width = np.zeros(len(p), np.int64)
    for i in range(len(p)):
        same = p == p[i]
        width[i] = int(np.count_nonzero(same & (np.abs(t - t[i]) <= interval))) - 1
    return width, np.concatenate([[0], np.cumsum(width)])


def chunk_pairs(off, budget):
    """The chunks' candidate-pair counts: each chunk takes the rows from r0 up to the largest r1 with off[r1] - off[r0] <=
    budget, at least one row; chunks without pairs are not counted."""
    n, r0, out = len(off) - 1, 0, []
    while r0 < n:
        r1 = r0 + 1
        while r1 < n and off[r1 + 1] - off[r0] <= budget:
            r1 += 1
        if off[r1] - off[r0] > 0:
            out.append(int(off[r1] - off[r0]))
        r0 = r1
    return out


def place_count_case(n_places):
    """Exactly n_places distinct places, every one in a pair: persons of 2 and 3 rows.  The pair key is rank_a << nb |
    rank_b with nb = ceil(log2(places)), at least 1: 2^k places fill nb = k bits, 2^k + 1 need one more."""
    n, sizes = max(2 * n_places, 6), []
    while sum(sizes) < n:
        sizes.append(3 if len(sizes) % 4 == 0 else 2)
    return clusters(sizes, n_places, seed=n_places)


PLACE_COUNTS = (2, 3, 4, 5, 256, 257, 65536, 65537)

# Person sizes whose candidate pairs (size * (size - 1) each; a size of 1 is a row without partner) put the ends of the
# 2,048-pair tiles where the names say.  The total of a whole input is always even: a pair (a, b) comes with (b, a).
TILE_CASES = {
    # 46 * 45 = 2070: pair 2047 is the 23rd of the 45 partners of the 46th row, the tile ends in the middle of a row
    "tile ends inside a row": [46, 3],
    # 45 * 44 + 8 * 7 + 4 * 3 = 2048 exactly: one full tile, which ends on the last partner of a row
    "total 2048": [45, 8, 4],
    "total 2046": [2, 2, 3, 8, 45],
    "total 2050": [2, 45, 8, 4],
    "total 4096": [45, 8, 4, 45, 8, 4],
    # the second tile starts on the first partner of a row, after a run of rows without partner AT the tile end
    "rows without partner at the tile end": [45, 8, 4, 1, 1, 1, 1, 1, 30, 3],
    # 2046 pairs, rows without partner, then a row whose partners are pairs 2046, 2047 (the tile end), 2048 ..
    "tile ends on the second partner of a row": [45, 8, 3, 2, 2, 1, 1, 1, 40, 3],
    # 2036 pairs, then a person of 12: its second row's FIRST partner is pair 2047, the tile's last
    "tile ends on the first partner of a row": [45, 8, 12, 1, 1, 3],
    # rows without partner before the tile end (inside the tile) and after it
    "rows without partner before and after": [1, 1, 1, 45, 1, 1, 8, 4, 5, 1, 1, 1, 1, 3],
}


def tile_case(name, n_places=9):
    return clusters(TILE_CASES[name], n_places, seed=len(name))


# the fresh-process budget cases: rows whose candidate pairs reach 2,048 exactly at a row's end, twice ("even"), and
# the same with a person of two rows (one partner each) behind the first 2,048 ("step"); budgets 2047 / 2048 / 2049
BUDGET_SIZES = {"even": [45, 8, 4, 45, 8, 4], "step": [45, 8, 4, 2, 45, 8, 4]}
BUDGETS = (2047, 2048, 2049)


def budget_case(name):
    return clusters(BUDGET_SIZES[name], 9, seed=77)


def run_budget_cases(pkg, out_path):
    """Runs the budget cases in THIS process (whose LOCREC_PREP_PAIR_BUDGET the caller chose) and stores the results."""
    out = {}
    for name in BUDGET_SIZES:
        s, t, w = pkg.prep.calc_similar_place_edges(*budget_case(name), 0, 50)
        stats = pkg.prep.similar_place_edges_stats()
        out.update({name + "_source": s, name + "_target": t, name + "_weight": w, name + "_chunks": stats["chunks"],
                    name + "_pairs": stats["pairs"]})
    np.savez(out_path, **out)


WIDE_ROWS = {10: 65536, 20: 65536, 30: 1}        # place -> rows of the one person, all inside one interval


def wide_count_case():
    """One person, 131,073 rows inside one interval: count(10, 20) = 65536 * 65536 = 2^32, whose low 32 bits are zero,
    against count(10, 30) = 65536.  -> (person, place, timestamp), {(a, b): count} by the closed form rows(a) * rows(b)."""
    place = np.repeat(np.array(list(WIDE_ROWS), np.int64), list(WIDE_ROWS.values()))
    n = len(place)
    order = np.random.default_rng(12).permutation(n)
    ts = T0 + (np.arange(n, dtype=np.int64) * 37) % 1000
    counts = {(a, b): WIDE_ROWS[a] * WIDE_ROWS[b] for a in WIDE_ROWS for b in WIDE_ROWS if a != b}
    return (np.full(n, 777, np.int64), place[order], ts[order]), counts


# ---- ranking cases ------------------------------------------------------------------------------------------------------

def _bits(x):
    return np.array([x], np.uint64).view(np.float64)[0]


NANS = (_bits(0x7FF8000000000000), _bits(0xFFF8000000000000), _bits(0x7FF80000000ABCDE), _bits(0xFFF8000000000123))
SPECIAL_SCORES = NANS + (np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.225073858507201e-308, -2.225073858507201e-308,
                         2.2250738585072014e-308, 1.0, -1.0, 1.7976931348623157e308, -1.7976931348623157e308)


def ranking_case():
    """Scores with NaN of both signs and with payloads, +-inf, +-0.0, subnormals; every special score on ids from -2^63
    to 2^63 - 1; recommendation ids listed twice (with equal and with different scores); place ids listed twice inside
    the target region, in and out of it, and only outside.  -> dict(ids, scores, place_ids, place_regions, target, kept)"""
    target = 3
    inside = [I64_MIN, I64_MIN + 1, -7, -1, 0, 1, 2, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, I64_MAX - 1, I64_MAX]
    outside = [60, 61, 62, -60, I64_MAX - 5]
    place_ids = inside + [40, 41, I64_MIN] + [42, 43] + outside
    place_regions = [target] * len(inside) + [target] * 3 + [4, 4] + [4, -1, 5, 4, 0]
    ids, scores = [], []
    for rot in (0, 5, 11):                                      # every id three times, with three different scores
        for k, i in enumerate(inside):
            ids.append(i)
            scores.append(SPECIAL_SCORES[(k + rot) % len(SPECIAL_SCORES)])
    for s in SPECIAL_SCORES:                                    # every special score on both extreme ids and a middle one
        for i in (I64_MAX, 44, I64_MIN):
            ids.append(i)
            scores.append(s)
    for i, s in ((44, -0.0), (44, 0.0), (44, NANS[3]), (44, NANS[0]), (I64_MIN, -0.0), (I64_MIN, 0.0)):
        ids.append(i)                                           # equal (score, id) with different bits: input order decides
        scores.append(s)
    for k, i in enumerate(outside + [1000, -1000]):             # rows the join drops, some with the best scores
        ids.append(i)
        scores.append(SPECIAL_SCORES[k % 6])
    order = np.random.default_rng(2).permutation(len(ids))
    ids, scores = np.array(ids, np.int64)[order], np.array(scores, np.float64)[order]
    kept = int(np.isin(ids, np.array(inside, np.int64)).sum())
    rng = np.random.default_rng(3).permutation(len(place_ids))
    return dict(ids=ids, scores=scores, place_ids=np.array(place_ids, np.int64)[rng],
                place_regions=np.array(place_regions, np.int64)[rng], target=target, kept=kept)
