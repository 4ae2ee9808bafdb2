"""CPU checks of the sample generator's boundary: the header declares its functions, the library exports them, the binding
names them with matching arity, the argument checks answer before any device is needed, and without a GPU nothing
computes (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = torch.cuda.is_available()
ARITY = {"locrec_sample_persons": 8, "locrec_sample_location_visits": 20, "locrec_sample_location_visits_stats": 4,
         "locrec_sample_places": 15, "locrec_sample_place_names": 11}


def header_text():
    with open(os.path.join(ROOT, "include", "locrec.h")) as f:
        return f.read()


def test_header_library_and_binding_agree(pkg):
    from locations_recommender_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    handle = C.CDLL(pkg.LIB_PATH)
    for name, arity in ARITY.items():
        m = re.search(r"\bint32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, f"{name} is not declared in include/locrec.h"
        assert len(m.group(1).split(",")) == arity, name
        assert hasattr(handle, name), f"{name} is not exported by the library"
        assert len(_lib.SIGNATURES[name]) == arity, name


def test_header_states_the_conventions():
    text = header_text()
    doc = text[text.index("The sample generator"):]
    for phrase in ("session time zone", "parity unpinned", "shared_factor = 1", "person_index_base", "category-name tables and counts are always",
                   "call with 0 to size the buffers", "floor division", "DESIGN.md section 9b"):
        assert phrase in doc, phrase


def test_python_names(pkg):
    from locations_recommender_amd import mains
    s = pkg.sample
    assert pkg.Region is s.Region and s.Region._fields == ("id", "name", "min_latitude", "max_latitude", "min_longitude", "max_longitude")
    for name in ("generate_persons", "generate_location_visits", "generate_places", "place_names", "id_scheme", "generate",
                 "location_visits_stats", "location_visits_count"):
        assert callable(getattr(s, name)), name
    for name in ("sample_generator_main", "parse_input", "load_persons", "calc_recommender_target", "knn_recommender_request",
                 "sg_recommender_request"):
        assert callable(getattr(mains, name)), name
    assert issubclass(mains.NoSuchElementException, LookupError)
    assert s.id_scheme(20, 30_000) == (0, 40, 60_040)
    assert s.year_interval(2018) == (1_514_764_800_000, 8736, 365) and s.year_interval(2020)[1:] == (8760, 366)


BOX = [55.0, 56.0, 37.0, 38.0]


def region_args(ids=(0, 1, 2), boxes=None):
    ids = np.asarray(ids, np.int64)
    boxes = np.asarray(boxes if boxes is not None else [BOX] * len(ids), np.float64)
    return ids, boxes


def call_persons(lib, ids, n_regions=None, person_count=10, min_person_id=100, mem=0, outs=True, cnt_ok=True):
    out = np.zeros(64, np.int64), np.zeros(64, np.int64)
    cnt = C.c_int64(-5)
    st = lib.locrec_sample_persons(len(ids) if n_regions is None else n_regions,
                                   ids.ctypes.data_as(C.POINTER(C.c_int64)) if ids is not None and len(ids) else None, person_count,
                                   min_person_id, mem, *[C.c_void_p(o.ctypes.data) if outs else None for o in out],
                                   C.byref(cnt) if cnt_ok else None)
    return st, cnt.value


def call_visits(lib, n_persons=1, ids=(0, 1, 2), boxes=None, from_ms=0, hours=8736, max_visits=365, shared=1, mem=0, cap=0,
                cnt_ok=True, persons_ok=True, regions_ok=True, boxes_ok=True, base=0):
    rid, bx = region_args(ids, boxes)
    pid, home = np.zeros(max(n_persons, 1), np.int64), np.zeros(max(n_persons, 1), np.int64)
    cnt = C.c_int64(cap)
    st = lib.locrec_sample_location_visits(
        n_persons, C.c_void_p(pid.ctypes.data) if persons_ok else None, C.c_void_p(home.ctypes.data) if persons_ok else None, base,
        len(rid), rid.ctypes.data_as(C.POINTER(C.c_int64)) if regions_ok and len(rid) else None,
        bx.ctypes.data_as(C.POINTER(C.c_double)) if boxes_ok and len(rid) else None, from_ms, hours, max_visits, 0, shared, mem,
        None, None, None, None, None, None, C.byref(cnt) if cnt_ok else None)
    return st, cnt.value


def call_places(lib, ids=(0, 1, 2), boxes=None, place_count=30, min_place_id=40, n_categories=20, min_category_id=0, mem=0,
                outs=True, cnt_ok=True, regions_ok=True, boxes_ok=True):
    rid, bx = region_args(ids, boxes)
    out = [np.zeros(64, np.int64), np.zeros(64, np.float64), np.zeros(64, np.float64), np.zeros(64, np.int64), np.zeros(64, np.int64)]
    cnt = C.c_int64(-5)
    st = lib.locrec_sample_places(len(rid), rid.ctypes.data_as(C.POINTER(C.c_int64)) if regions_ok and len(rid) else None,
                                  bx.ctypes.data_as(C.POINTER(C.c_double)) if boxes_ok and len(rid) else None, place_count,
                                  min_place_id, n_categories, min_category_id, 0, mem,
                                  *[C.c_void_p(o.ctypes.data) if outs else None for o in out], C.byref(cnt) if cnt_ok else None)
    return st, cnt.value


def call_names(lib, n=1, n_categories=1, coff=(0, 1), mem=0, cap=0, cnt_ok=True, cols_ok=True, coff_ok=True, cunits_ok=True,
               outs=False):
    ids, cats = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    coff = np.asarray(coff, np.int64)
    cunits = np.full(8, ord("a"), np.uint16)
    off, units = np.zeros(max(n, 1) + 1, np.int64), np.zeros(64, np.uint16)
    cnt = C.c_int64(cap)
    st = lib.locrec_sample_place_names(n, C.c_void_p(ids.ctypes.data) if cols_ok else None, C.c_void_p(cats.ctypes.data) if cols_ok else None,
                                       0, n_categories, coff.ctypes.data_as(C.POINTER(C.c_int64)) if coff_ok else None,
                                       cunits.ctypes.data_as(C.POINTER(C.c_uint16)) if cunits_ok else None, mem,
                                       C.c_void_p(off.ctypes.data) if outs else None, C.c_void_p(units.ctypes.data) if outs else None,
                                       C.byref(cnt) if cnt_ok else None)
    return st, cnt.value


def test_argument_checks_need_no_device(pkg):
    from locations_recommender_amd import _lib as L
    lib = pkg.lib()
    bad = L.E_INVALID_ARG
    ids = np.array([0, 1, 2], np.int64)
    # ---- locrec_sample_persons
    assert call_persons(lib, ids, person_count=0) == (L.OK, 0)
    assert call_persons(lib, ids, person_count=2) == (L.OK, 0)                 # fewer persons than regions: no rows
    assert call_persons(lib, ids, cnt_ok=False)[0] == bad
    assert call_persons(lib, ids, mem=7)[0] == bad
    assert call_persons(lib, ids, n_regions=0)[0] == bad
    assert call_persons(lib, None, n_regions=3)[0] == bad
    assert call_persons(lib, np.array([0, 5, 0], np.int64))[0] == bad and b"twice" in lib.locrec_last_error()
    assert call_persons(lib, np.array([0, -1, 2], np.int64))[0] == bad and b"negative" in lib.locrec_last_error()
    assert call_persons(lib, ids, person_count=-1)[0] == bad
    assert call_persons(lib, ids, outs=False)[0] == bad
    assert call_persons(lib, ids, person_count=30, min_person_id=2 ** 63 - 20)[0] == bad and b"int64" in lib.locrec_last_error()
    # ---- locrec_sample_location_visits
    assert call_visits(lib, n_persons=0, cap=9) == (L.OK, 0)
    assert call_visits(lib, cnt_ok=False)[0] == bad
    for kw in (dict(mem=2), dict(mem=-1), dict(cap=-1), dict(n_persons=-1), dict(ids=()), dict(regions_ok=False), dict(boxes_ok=False),
               dict(ids=(3, 3, 4)), dict(ids=(0, -2, 1)), dict(persons_ok=False), dict(shared=2), dict(max_visits=0), dict(hours=-1),
               dict(base=-1), dict(from_ms=2 ** 62),
               dict(boxes=[BOX, [56.0, 55.0, 37.0, 38.0], BOX]), dict(boxes=[BOX, BOX, [55.0, 56.0, 38.0, 37.0]]),
               dict(boxes=[[float("nan"), 56.0, 37.0, 38.0], BOX, BOX]), dict(boxes=[BOX, [55.0, float("inf"), 37.0, 38.0], BOX]),
               dict(boxes=[BOX, BOX, [55.0, 91.0, 37.0, 38.0]]), dict(boxes=[[55.0, 56.0, -181.0, 38.0], BOX, BOX])):
        assert call_visits(lib, **kw) == (bad, 0), kw
    # ---- locrec_sample_places
    assert call_places(lib, place_count=0) == (L.OK, 0)
    assert call_places(lib, place_count=2) == (L.OK, 0)                        # ppr == 0: no places, no division
    assert call_places(lib, cnt_ok=False)[0] == bad
    for kw in (dict(mem=7), dict(ids=()), dict(regions_ok=False), dict(boxes_ok=False), dict(ids=(1, 1, 2)), dict(ids=(-1, 1, 2)),
               dict(place_count=-1), dict(n_categories=0), dict(min_category_id=-1), dict(outs=False),
               dict(boxes=[[2.0, 1.0, 0.0, 0.0], BOX, BOX]), dict(boxes=[BOX, BOX, [0.0, 0.0, float("nan"), 1.0]]),
               dict(place_count=30, min_place_id=2 ** 63 - 5), dict(place_count=2 ** 52 + 1)):
        assert call_places(lib, **kw)[0] == bad, kw
    # ---- locrec_sample_place_names
    assert call_names(lib, cnt_ok=False)[0] == bad
    for kw in (dict(mem=3), dict(cap=-1), dict(n=-1), dict(n_categories=0), dict(coff_ok=False), dict(coff=(1, 0)), dict(coff=(-1, 0)),
               dict(cunits_ok=False), dict(cols_ok=False), dict(cap=4, outs=False)):
        assert call_names(lib, **kw) == (bad, 0), kw
    # ---- the stats of a call that never wrote: all zero, every pointer optional
    call_visits(lib, n_persons=0)
    n = C.c_int64(-1)
    assert lib.locrec_sample_location_visits_stats(C.byref(n), None, None, None) == L.OK and n.value == 0


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_for_the_generator(pkg):
    from locations_recommender_amd import _lib as L
    lib = pkg.lib()
    ids = np.array([0, 1, 2], np.int64)
    assert call_persons(lib, ids)[0] == L.E_DEVICE
    assert call_visits(lib)[0] == L.E_DEVICE
    assert call_places(lib)[0] == L.E_DEVICE
    assert call_names(lib)[0] == L.E_DEVICE
    regions = [(0, "a", *BOX), (1, "b", *BOX)]
    s = pkg.sample
    with pytest.raises(pkg.LocrecRuntimeError):
        s.generate_persons(regions, 10, 100)
    with pytest.raises(pkg.LocrecRuntimeError):
        s.generate_persons(regions, 10, 100, device=True)
    with pytest.raises(pkg.LocrecRuntimeError):
        s.generate_location_visits({"id": np.array([100]), "home_region_id": np.array([0])}, regions, 0, 8736, 365)
    with pytest.raises(pkg.LocrecRuntimeError):
        s.generate_places(regions, 30, 40, 20)
    with pytest.raises(pkg.LocrecRuntimeError):
        s.place_names(np.array([40]), np.array([0]), ["cafe"])
