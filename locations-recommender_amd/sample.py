"""The reference's sample generator (sample-generator: SampleGeneratorMain.scala, LocationVisitsSampleGenerator.scala,
PlacesSampleGenerator.scala), computed by liblocrec.so's kernels (csrc/sample.hip):

    generate_persons           LocationVisitsSampleGenerator.generatePersons          :55-68
    generate_location_visits   ... withVisits / withGeoLocations / withTimestamps     :78-133
    generate_places            PlacesSampleGenerator.withGeo / withCategories         PlacesSampleGenerator.scala:41-77
    place_names                PlacesSampleGenerator.withNames                        PlacesSampleGenerator.scala:79-90
    id_scheme                  SampleGeneratorMain's id ranges                        SampleGeneratorMain.scala:36-37,54
    generate                   SampleGeneratorMain.doMain, to tables instead of files

The regions and the category names are arguments: the reference's own are literals of its program and are not part of
this package.  Spark's rand(seed) cannot be reproduced (its values depend on the partition layout), so the factors are
synth.u01(seed, stream, row, slot) - parity unpinned, DESIGN.md section 9b - and a table depends on nothing but its
arguments: a shard of the persons with its own person_index_base reproduces the rows of the whole.

Tables are dicts of columns.  Columns come back as numpy arrays, or as torch CUDA tensors that feed
prep.calc_place_visits directly (device=True, or CUDA tensors in).  There is no CPU fallback."""
import calendar
import collections
import ctypes as C
import datetime

import numpy as np

from . import _lib as L
from .prep import _Cols

Region = collections.namedtuple("Region", "id name min_latitude max_latitude min_longitude max_longitude")

VISIT_COLUMNS = ("person_id", "region_id", "latitude", "longitude", "timestamp", "year_month")
_VISIT_DTYPES = (np.int64, np.int64, np.float64, np.float64, np.int64, np.int32)
PLACE_COLUMNS = ("id", "latitude", "longitude", "region_id", "category_id")
_PLACE_DTYPES = (np.int64, np.float64, np.float64, np.int64, np.int64)


def id_scheme(n_categories, place_count):
    """SampleGeneratorMain.scala:36-37,54 -> (min_category_id, min_place_id, min_person_id)."""
    min_category_id = 0
    min_place_id = min_category_id + 2 * int(n_categories)
    return min_category_id, min_place_id, min_place_id + 2 * int(place_count)


def year_interval(year):
    """The visits' interval of a sample year (LocationVisitsSampleGenerator.scala:23-31), on the host:
    -> (from_timestamp_ms of January 1st 00:00 UTC, interval_hours = (days - 1) * 24, max_visits = days), so the last
    day of the year never occurs."""
    days = 366 if calendar.isleap(int(year)) else 365
    from_ms = (datetime.date(int(year), 1, 1) - datetime.date(1970, 1, 1)).days * 86_400_000
    return from_ms, (days - 1) * 24, days


def _region_tables(regions):
    regions = [Region(*r) for r in regions]
    ids = np.array([r.id for r in regions], np.int64)
    boxes = np.array([[r.min_latitude, r.max_latitude, r.min_longitude, r.max_longitude] for r in regions], np.float64).reshape(-1, 4)
    return ids, np.ascontiguousarray(boxes)


def _cols(device, *arrays):
    """The columns of a call that may have no input column: device=True allocates the outputs on the current GPU."""
    if arrays or not device:
        return _Cols(*arrays)
    import torch
    if not torch.cuda.is_available():
        raise L.LocrecRuntimeError("no GPU is usable: the sample generator has no CPU path")
    return _Cols(torch.empty(0, dtype=torch.int64, device="cuda"))


def _units_out(c, n):
    """A uint16 output column (a tensor of 2-byte integers where torch has no uint16)."""
    if c.device and not hasattr(c.torch, "uint16"):
        a = c.torch.empty(max(int(n), 1), dtype=c.torch.int16, device=c.dev)
        return a, C.c_void_p(a.data_ptr())
    return c.out(n, np.uint16)


def generate_persons(regions, person_count, min_person_id, device=False):
    """generatePersons: person_count // len(regions) persons per region, regions in the given order, ids ascending
    inside a region from min_person_id + region.id * that number.  -> dict(id, home_region_id)."""
    ids, _ = _region_tables(regions)
    c = _cols(device)
    total = (int(person_count) // len(ids)) * len(ids) if len(ids) and person_count > 0 else 0
    (oid, oidp), (ohome, ohomep) = c.out(total, np.int64), c.out(total, np.int64)
    cnt = C.c_int64()
    L.check(L.lib().locrec_sample_persons(len(ids), L.ptr(ids, C.c_int64), int(person_count), int(min_person_id), c.mem,
                                          oidp, ohomep, C.byref(cnt)))
    return {"id": oid[:cnt.value], "home_region_id": ohome[:cnt.value]}


def _visit_args(c, persons, regions, from_timestamp_ms, interval_hours, max_visits_per_person, seed, shared_factor,
                person_index_base):
    ids, boxes = _region_tables(regions)
    n = len(persons["id"])
    assert len(persons["home_region_id"]) == n
    args = [n, c.col(persons["id"], np.int64), c.col(persons["home_region_id"], np.int64), int(person_index_base), len(ids),
            L.ptr(ids, C.c_int64), L.ptr(boxes, C.c_double), int(from_timestamp_ms), int(interval_hours),
            int(max_visits_per_person), int(seed), 1 if shared_factor else 0, c.mem]
    return args, (ids, boxes)


def location_visits_count(persons, regions, from_timestamp_ms, interval_hours, max_visits_per_person, seed=0,
                          shared_factor=True, person_index_base=0):
    """The number of rows generate_location_visits would return (the count-and-scan phase alone: nothing is allocated
    for the rows)."""
    c = _Cols(persons["id"], persons["home_region_id"])
    args, _keep = _visit_args(c, persons, regions, from_timestamp_ms, interval_hours, max_visits_per_person, seed, shared_factor,
                              person_index_base)
    cnt = C.c_int64(0)
    L.check(L.lib().locrec_sample_location_visits(*args, None, None, None, None, None, None, C.byref(cnt)))
    return cnt.value


def generate_location_visits(persons, regions, from_timestamp_ms, interval_hours, max_visits_per_person, seed=0,
                             shared_factor=True, person_index_base=0, capacity=None):
    """The visits of the persons table (dict(id, home_region_id), numpy or CUDA tensors): per person 1 to
    max_visits_per_person rows inside its home region's box and inside [from_timestamp_ms, + interval_hours].
    shared_factor: one factor for latitude, longitude and time of a row, as the reference's three rand(0) columns are
    (False: three independent factors).  person_index_base: the index of the table's first person in the key of the
    random numbers.  capacity: write no more than that many rows (the first rows of the full result).
    -> dict(person_id, region_id, latitude, longitude, timestamp (epoch ms), year_month (int32, e.g. 201803)),
    ordered by (person row, visit number)."""
    c = _Cols(persons["id"], persons["home_region_id"])
    args, _keep = _visit_args(c, persons, regions, from_timestamp_ms, interval_hours, max_visits_per_person, seed, shared_factor,
                              person_index_base)
    fn = L.lib().locrec_sample_location_visits
    if capacity is None:
        cnt = C.c_int64(0)   # first call: count only
        L.check(fn(*args, None, None, None, None, None, None, C.byref(cnt)))
        capacity = cnt.value
    capacity = int(capacity)
    outs = [c.out(capacity, dt) for dt in _VISIT_DTYPES]
    m = 0
    if capacity > 0:
        cnt = C.c_int64(capacity)
        L.check(fn(*args, *[o[1] for o in outs], C.byref(cnt)))
        m = min(cnt.value, capacity)
    return {k: o[0][:m] for k, o in zip(VISIT_COLUMNS, outs)}


def location_visits_stats():
    """What this thread's last location-visits call did: rows and bytes written, HIP-event milliseconds of the
    count-and-scan phase and of the fill (locrec_sample_location_visits_stats)."""
    rows, nbytes, count_ms, fill_ms = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    L.check(L.lib().locrec_sample_location_visits_stats(C.byref(rows), C.byref(nbytes), C.byref(count_ms), C.byref(fill_ms)))
    return dict(rows=rows.value, bytes=nbytes.value, count_ms=count_ms.value, fill_ms=fill_ms.value)


def generate_places(regions, place_count, min_place_id, n_categories, min_category_id=0, seed=0, device=False):
    """withGeo / withCategories: a c x c grid per region, c = floor(sqrt(place_count // len(regions))), and a category
    drawn per place.  -> dict(id, latitude, longitude, region_id, category_id), regions in the given order."""
    ids, boxes = _region_tables(regions)
    c = _cols(device)
    ppr = int(place_count) // len(ids) if len(ids) and place_count > 0 else 0
    total = int(np.floor(np.sqrt(float(ppr)))) ** 2 * len(ids)
    outs = [c.out(total, dt) for dt in _PLACE_DTYPES]
    cnt = C.c_int64()
    L.check(L.lib().locrec_sample_places(len(ids), L.ptr(ids, C.c_int64), L.ptr(boxes, C.c_double), int(place_count),
                                         int(min_place_id), int(n_categories), int(min_category_id), int(seed), c.mem,
                                         *[o[1] for o in outs], C.byref(cnt)))
    return {k: o[0][:cnt.value] for k, o in zip(PLACE_COLUMNS, outs)}


def place_names(place_ids, category_ids, categories, min_category_id=0, capacity=None):
    """withNames: "<category name>-<id>" per place as the CSR deduplicator.encode_names makes (offsets int64[n + 1],
    UTF-16 code units), category names as they are.  capacity: write no more than that many units.
    -> (offsets, units)."""
    from .deduplicator import encode_names
    coff, cunits = encode_names(list(categories), lower=False, what="categories")
    c = _Cols(place_ids, category_ids)
    n = len(place_ids)
    assert len(category_ids) == n
    args = [n, c.col(place_ids, np.int64), c.col(category_ids, np.int64), int(min_category_id), len(coff) - 1,
            L.ptr(coff, C.c_int64), L.ptr(cunits, C.c_uint16) if len(cunits) else None, c.mem]
    fn = L.lib().locrec_sample_place_names
    off, offp = c.out(n + 1, np.int64)
    if capacity is None:
        cnt = C.c_int64(0)   # first call: the lengths and their scan
        L.check(fn(*args, None, None, C.byref(cnt)))
        capacity = cnt.value
    capacity = int(capacity)
    units, unitsp = _units_out(c, capacity)
    cnt = C.c_int64(capacity)
    L.check(fn(*args, offp, unitsp if capacity > 0 else None, C.byref(cnt)))
    return off[:n + 1], units[:min(capacity, cnt.value)]


def decode_names(offsets, units):
    """The Python strings of a names CSR (host side; CUDA tensors are copied to the host)."""
    if hasattr(offsets, "detach"):
        offsets, units = offsets.detach().cpu().numpy(), units.detach().cpu().numpy()
    off = np.asarray(offsets, np.int64)
    raw = np.ascontiguousarray(units).view(np.uint16)
    return [raw[off[i]:off[i + 1]].tobytes().decode("utf-16-le") for i in range(len(off) - 1)]


def generate(place_count, person_count, regions, categories, seed=0, shared_factor=True, year=2018, device=True):
    """SampleGeneratorMain.doMain to tables: ids by id_scheme, the visits over `year` (year_interval).
    -> dict(persons, location_visits, places, categories); places also carries the names CSR (name_offsets, name_units);
    categories is dict(category, category_id) on the host."""
    regions = [Region(*r) for r in regions]
    categories = list(categories)
    min_category_id, min_place_id, min_person_id = id_scheme(len(categories), place_count)
    from_ms, interval_hours, max_visits = year_interval(year)
    persons = generate_persons(regions, person_count, min_person_id, device=device)
    visits = generate_location_visits(persons, regions, from_ms, interval_hours, max_visits, seed=seed, shared_factor=shared_factor)
    places = generate_places(regions, place_count, min_place_id, len(categories), min_category_id, seed=seed, device=device)
    places["name_offsets"], places["name_units"] = place_names(places["id"], places["category_id"], categories, min_category_id)
    cats = {"category": categories, "category_id": np.arange(min_category_id, min_category_id + len(categories), dtype=np.int64)}
    return {"persons": persons, "location_visits": visits, "places": places, "categories": cats}
