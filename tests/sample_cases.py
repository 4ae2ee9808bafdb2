"""The sample generator restated on the CPU: numpy over synth.u01, computed from the rules of the reference's
generator (LocationVisitsSampleGenerator.scala, PlacesSampleGenerator.scala, SampleGeneratorMain.scala) and the keying
of DESIGN.md section 9b - never from the device.  Every floating-point step is one numpy operation, so the device's
columns must equal these bit for bit."""
import calendar
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MS_PER_HOUR, MS_PER_DAY = 3_600_000, 86_400_000
STREAM_VISIT_COUNT, STREAM_VISIT, STREAM_CATEGORY = 1, 2, 3


def defaults():
    """The reference's regions, categories and shipped counts (tests/golden/sample_generator_defaults.json)."""
    with open(os.path.join(HERE, "golden", "sample_generator_defaults.json")) as f:
        d = json.load(f)
    d["regions"] = [(r["id"], r["name"], r["min_latitude"], r["max_latitude"], r["min_longitude"], r["max_longitude"])
                    for r in d["regions"]]
    return d


def u01(seed, stream, row, slot):
    from locations_recommender_amd import synth
    return synth.u01(seed, stream, row, slot)


def id_scheme(n_categories, place_count):
    min_category_id = 0
    min_place_id = min_category_id + 2 * n_categories
    return min_category_id, min_place_id, min_place_id + 2 * place_count


def year_interval(year):
    days = 366 if calendar.isleap(year) else 365
    from_ms = int(np.datetime64(f"{year:04d}-01-01T00:00", "ms").astype(np.int64))
    return from_ms, (days - 1) * 24, days


def persons(regions, person_count, min_person_id):
    ppr = person_count // len(regions)
    ids = [min_person_id + r[0] * ppr + np.arange(ppr, dtype=np.int64) for r in regions]
    home = [np.full(ppr, r[0], np.int64) for r in regions]
    return {"id": np.concatenate(ids), "home_region_id": np.concatenate(home)}


def visit_counts(n_persons, max_visits, seed=0, person_index_base=0):
    index = person_index_base + np.arange(n_persons, dtype=np.int64)
    return (u01(seed, STREAM_VISIT_COUNT, index, 0) * float(max_visits)).astype(np.int64) + 1


def year_month(timestamp_ms):
    """year * 100 + month in UTC, through numpy's calendar (floor semantics, proleptic Gregorian)."""
    months = np.asarray(timestamp_ms, np.int64).astype("datetime64[ms]").astype("datetime64[M]").astype(np.int64)   # since 1970-01
    return ((1970 + months // 12) * 100 + months % 12 + 1).astype(np.int32)


def location_visits(table, regions, from_ms, interval_hours, max_visits, seed=0, shared_factor=True, person_index_base=0):
    pid, home = np.asarray(table["id"], np.int64), np.asarray(table["home_region_id"], np.int64)
    n = len(pid)
    counts = visit_counts(n, max_visits, seed, person_index_base)
    row = np.repeat(np.arange(n, dtype=np.int64), counts)
    k = np.arange(len(row), dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
    index = row + person_index_base
    g_lat = u01(seed, STREAM_VISIT, index, 3 * k)
    g_lon = g_lat if shared_factor else u01(seed, STREAM_VISIT, index, 3 * k + 1)
    g_t = g_lat if shared_factor else u01(seed, STREAM_VISIT, index, 3 * k + 2)
    by_id = {r[0]: r for r in regions}
    box = np.array([by_id[int(h)][2:6] for h in home], np.float64).reshape(-1, 4)[row]
    lat = box[:, 0] + (box[:, 1] - box[:, 0]) * g_lat
    lon = box[:, 2] + (box[:, 3] - box[:, 2]) * g_lon
    ts = from_ms + (float(interval_hours) * g_t).astype(np.int64) * MS_PER_HOUR
    return {"person_id": pid[row], "region_id": home[row], "latitude": lat, "longitude": lon, "timestamp": ts,
            "year_month": year_month(ts)}


def grid_side(place_count, n_regions):
    ppr = place_count // n_regions
    return int(np.floor(np.sqrt(float(ppr))))


def places(regions, place_count, min_place_id, n_categories, min_category_id=0, seed=0):
    c = grid_side(place_count, len(regions))
    cols = {k: [] for k in ("id", "latitude", "longitude", "region_id")}
    if c > 0:
        idx = np.arange(c * c, dtype=np.int64)
        lat_idx, lon_idx = (idx // c + 1).astype(np.float64), (idx % c + 1).astype(np.float64)
        for r in regions:
            lat_step, lon_step = (np.float64(r[3]) - np.float64(r[2])) / np.float64(c), (np.float64(r[5]) - np.float64(r[4])) / np.float64(c)
            cols["id"].append(min_place_id + r[0] * c * c + idx)
            cols["latitude"].append(np.float64(r[2]) + lat_step * lat_idx)
            cols["longitude"].append(np.float64(r[4]) + lon_step * lon_idx)
            cols["region_id"].append(np.full(c * c, r[0], np.int64))
    out = {k: (np.concatenate(v) if v else np.empty(0, np.float64 if k in ("latitude", "longitude") else np.int64)) for k, v in cols.items()}
    n = len(out["id"])
    f = u01(seed, STREAM_CATEGORY, np.arange(n, dtype=np.int64), 0)
    out["category_id"] = min_category_id + (f * float(n_categories)).astype(np.int64)
    return out


def place_names(place_ids, category_ids, categories, min_category_id=0):
    return [f"{categories[int(c) - min_category_id]}-{int(i)}" for i, c in zip(place_ids, category_ids)]


def generate(place_count, person_count, regions, categories, seed=0, shared_factor=True, year=2018):
    min_category_id, min_place_id, min_person_id = id_scheme(len(categories), place_count)
    from_ms, hours, days = year_interval(year)
    p = persons(regions, person_count, min_person_id)
    pl = places(regions, place_count, min_place_id, len(categories), min_category_id, seed)
    return {"persons": p, "location_visits": location_visits(p, regions, from_ms, hours, days, seed, shared_factor), "places": pl,
            "names": place_names(pl["id"], pl["category_id"], categories, min_category_id)}


def same_bits(a, b):
    """Equal shapes, dtypes and bit patterns (doubles compared as their 64 bits)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return bool(np.array_equal(a, b))
