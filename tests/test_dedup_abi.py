"""CPU checks of the place deduplicator's boundary: the header declares its functions, the library exports them, the
binding and the Python mirror name them with matching arity, the argument checks answer before any device is needed, and
without a GPU nothing computes (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = torch.cuda.is_available()
ARITY = {"locrec_lev_distances": 8, "locrec_find_duplicate_places": 22, "locrec_find_duplicate_places_stats": 6}


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


def test_header_states_the_limits():
    text = header_text()
    doc = text[text.index("The place deduplicator"):]
    for phrase in ("ALREADY LOWER-CASED", "Levenshtein.scala:18-57", "PlaceDeduplicator.scala:13-54", "earth radius",
                   "2^24 - 1", "-(1 + n_places + confirmed row)", "LOCREC_DEDUP_PAIR_BUDGET", "no length limit"):
        assert phrase in doc, phrase


def test_python_mirror_names(pkg):
    d = pkg.deduplicator
    assert pkg.PlaceDeduplicator is d.PlaceDeduplicator and pkg.lev is d.lev
    for name in ("lev", "lev_distances", "find_duplicate_places", "find_duplicate_places_stats", "encode_names"):
        assert callable(getattr(d, name)), name
    for name in ("dropDuplicates", "findDuplicates", "withoutDuplicates"):
        assert callable(getattr(d.PlaceDeduplicator, name)), name
    assert "anti-join" in d.PlaceDeduplicator.withoutDuplicates.__doc__
    off, units = d.encode_names(["Ab", "", "\U00010400"])
    assert off.tolist() == [0, 2, 2, 4] and units.tolist() == [ord("a"), ord("b"), 0xD801, 0xDC28]
    with pytest.raises(TypeError, match="row 1"):
        d.encode_names(["a", None])


def test_argument_checks_need_no_device(pkg):
    from locations_recommender_amd import _lib as L
    lib = pkg.lib()
    one, off = np.zeros(1, np.int64), np.array([0, 0], np.int64)
    dbl, out32 = np.zeros(1, np.float64), np.zeros(1, np.int32)
    p, o, d, o32 = (C.c_void_p(a.ctypes.data) for a in (one, off, dbl, out32))
    # ---- locrec_lev_distances
    assert lib.locrec_lev_distances(0, None, None, None, None, -1, L.MEM_HOST, None) == L.OK
    assert lib.locrec_lev_distances(1, o, None, o, None, -1, 7, o32) == L.E_INVALID_ARG                # mem
    assert lib.locrec_lev_distances(2 ** 31, o, None, o, None, -1, L.MEM_HOST, o32) == L.E_INVALID_ARG
    assert lib.locrec_lev_distances(-1, o, None, o, None, -1, L.MEM_HOST, o32) == L.E_INVALID_ARG
    for args in ((None, None, o, None, o32), (o, None, None, None, o32), (o, None, o, None, None)):
        assert lib.locrec_lev_distances(1, args[0], args[1], args[2], args[3], 3, L.MEM_HOST, args[4]) == L.E_INVALID_ARG
    # ---- locrec_find_duplicate_places
    fn = lib.locrec_find_duplicate_places

    def call(n_p=1, n_c=1, radius=60.0, k=5, mem=L.MEM_HOST, cap=0, cnt_ok=True, p_side=None, c_side=None, outs=(None, None, None)):
        cnt = C.c_int64(cap)
        ps = p_side or (p, p, d, d, o, None)
        cs = c_side or (p, p, d, d, o, None)
        st = fn(n_p, *ps, n_c, *cs, radius, k, mem, *outs, C.byref(cnt) if cnt_ok else None, None)
        return st, cnt.value
    assert call(n_p=0, n_c=0) == (L.OK, 0)
    assert call(n_p=0, n_c=1, cap=5) == (L.OK, 0)
    assert call(mem=7)[0] == L.E_INVALID_ARG
    assert call(cap=-1)[0] == L.E_INVALID_ARG
    assert call(cnt_ok=False)[0] == L.E_INVALID_ARG
    assert call(n_p=2 ** 31)[0] == L.E_INVALID_ARG and call(n_c=2 ** 31)[0] == L.E_INVALID_ARG
    assert call(n_p=-1)[0] == L.E_INVALID_ARG
    for radius in (float("nan"), 6371000.0, 1e9, float("inf")):
        assert call(radius=radius)[0] == L.E_INVALID_ARG
        assert b"earth radius" in lib.locrec_last_error()
    for missing in range(5):                                  # (the units may be NULL: all names may be empty)
        side = [p, p, d, d, o, None]
        side[missing] = None
        assert call(p_side=tuple(side))[0] == L.E_INVALID_ARG
        assert call(c_side=tuple(side))[0] == L.E_INVALID_ARG
    assert call(cap=1, outs=(p, None, o32))[0] == L.E_INVALID_ARG     # a capacity without somewhere to write
    # the stats of a call that never ran: all zero, every pointer optional
    n = C.c_int64(-1)
    assert lib.locrec_find_duplicate_places_stats(C.byref(n), None, None, None, None, None) == L.OK and n.value == 0


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_for_the_deduplicator(pkg):
    import pandas as pd
    d = pkg.deduplicator
    with pytest.raises(pkg.LocrecRuntimeError):
        d.lev("sitting", "kitten")
    frame = pd.DataFrame({"region_id": [0], "id": [1], "name": ["a"], "latitude": [1.0], "longitude": [2.0]})
    dd = pkg.PlaceDeduplicator(60, 5)
    for call in (dd.dropDuplicates, dd.findDuplicates, dd.withoutDuplicates):
        with pytest.raises(pkg.LocrecRuntimeError):
            call(frame, frame.assign(id=[2]))
