"""CPU checks of the stochastic graph's edge-family producers: the header declares them, the built library exports
them, the Python binding and mirror name them, and without a GPU they refuse to compute (no CPU fallback); and the
CPU restatement the device is compared with (tests/edge_cases.py) agrees with itself, with the hand-checked example
and with the already pinned oracle.calc_ratings."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import edge_cases
import prep_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = torch.cuda.is_available()
FUNCTIONS = ("locrec_calc_count_edges", "locrec_calc_similar_place_edges")
PYTHON_NAMES = ("calc_count_edges", "calc_similar_place_edges", "calc_person_likes_place_edges",
                "calc_person_likes_category_edges", "calc_category_selected_place_edges", "calc_place_similar_place_edges",
                "generate_stochastic_graph", "sg_graph_from_visits")


def test_header_library_and_binding_name_the_producers(pkg):
    from locations_recommender_amd import _lib
    text = open(os.path.join(ROOT, "include", "locrec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = C.CDLL(pkg.LIB_PATH)
    for name in FUNCTIONS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, text), f"{name} is not declared in include/locrec.h"
        assert hasattr(handle, name), f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["locrec_calc_count_edges"]) == 9
    assert len(_lib.SIGNATURES["locrec_calc_similar_place_edges"]) == 11


def test_python_mirror_names_and_constants(pkg):
    prep = pkg.prep
    for name in PYTHON_NAMES:
        assert callable(getattr(prep, name)), name
    assert prep.SIMILAR_PLACES_TOP_N == 50 and prep.PLACE_SIMILARITY_INTERVAL_MS == 7 * 24 * 3600 * 1000
    assert (prep.LIKED_PLACES_TOP_N, prep.LIKED_CATEGORIES_TOP_N, prep.SELECTED_PLACES_TOP_N) == (100, 100, 100)


def test_argument_checks_need_no_device(pkg):
    """What the entry points decide before touching the device: empty input, a negative interval, top_n <= 0 in the
    co-visit join, a bad `mem`, a row count beyond 2^31."""
    from locations_recommender_amd import _lib as L
    lib = pkg.lib()
    cnt = C.c_int64(5)
    assert lib.locrec_calc_count_edges(0, None, None, 3, L.MEM_HOST, None, None, None, C.byref(cnt)) == L.OK and cnt.value == 0
    one = np.zeros(1, np.int64)
    p = C.c_void_p(one.ctypes.data)
    for interval, top_n in ((-1, 50), (7, 0), (7, -1)):
        cnt = C.c_int64(0)
        assert lib.locrec_calc_similar_place_edges(1, p, p, p, interval, top_n, L.MEM_HOST, None, None, None, C.byref(cnt)) == L.OK
        assert cnt.value == 0
    cnt = C.c_int64(0)
    assert lib.locrec_calc_similar_place_edges(0, None, None, None, 7, 50, L.MEM_HOST, None, None, None, C.byref(cnt)) == L.OK
    assert lib.locrec_calc_count_edges(1, p, p, 3, 7, p, p, p, C.byref(cnt)) == L.E_INVALID_ARG
    assert lib.locrec_calc_count_edges(2 ** 31, p, p, 3, L.MEM_HOST, p, p, p, C.byref(cnt)) == L.E_INVALID_ARG
    assert lib.locrec_calc_similar_place_edges(2 ** 31, p, p, p, 7, 50, L.MEM_HOST, p, p, p, C.byref(cnt)) == L.E_INVALID_ARG
    assert lib.locrec_calc_similar_place_edges(1, p, p, p, 7, 50, L.MEM_HOST, p, p, p, None) == L.E_INVALID_ARG


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_for_the_edge_families(pkg):
    prep = pkg.prep
    pv = dict(person_id=edge_cases.HAND["person"], place_id=edge_cases.HAND["place"], timestamp=edge_cases.HAND["ts"],
              category_id=edge_cases.HAND["place"] % 7)
    calls = [lambda: prep.calc_count_edges(pv["person_id"], pv["place_id"], 3),
             lambda: prep.calc_similar_place_edges(pv["person_id"], pv["place_id"], pv["timestamp"], 7, 50),
             lambda: prep.calc_person_likes_place_edges(pv), lambda: prep.calc_person_likes_category_edges(pv),
             lambda: prep.calc_category_selected_place_edges(pv), lambda: prep.calc_place_similar_place_edges(pv),
             lambda: prep.generate_stochastic_graph(pv, 0.5, 0.5), lambda: prep.sg_graph_from_visits(pv, 0.5, 0.5)]
    assert len(calls) == len(PYTHON_NAMES)
    for call in calls:
        with pytest.raises(pkg.LocrecRuntimeError):
            call()


# ---- the restatement itself ---------------------------------------------------------------------------------

def rows_of(edges):
    return [(int(s), int(t), float(w)) for s, t, w in zip(*edges)]


def test_restatement_gives_the_hand_checked_example():
    h = edge_cases.HAND
    for loops in (True, False):
        assert rows_of(edge_cases.similar_place_edges(h["person"], h["place"], h["ts"], h["interval"], 50, loops)) == edge_cases.HAND_TOP_50
        assert rows_of(edge_cases.similar_place_edges(h["person"], h["place"], h["ts"], h["interval"], 1, loops)) == edge_cases.HAND_TOP_1
    counts = edge_cases.covisit_counts_loops(h["person"], h["place"], h["ts"], h["interval"])
    a, b, c = edge_cases.A, edge_cases.B, edge_cases.C_
    assert counts == {(a, b): 3, (b, a): 3, (b, c): 2, (c, b): 2}


def test_outer_comparison_equals_the_literal_double_loop():
    for seed, equal_ts in ((1, False), (2, True)):
        p, pl, ts = edge_cases.covisit_case(seed, 1500, persons=12, places=9, equal_timestamps=equal_ts, negative_ids=seed == 2)
        for interval in (0, edge_cases.INTERVAL_MS):
            assert edge_cases.covisit_counts(p, pl, ts, interval) == edge_cases.covisit_counts_loops(p, pl, ts, interval)


def test_rank_step_of_the_restatement_equals_the_pinned_oracle(oracle):
    for seed, n in ((0, 1), (1, 7), (2, 300), (3, 5000)):
        p, e = prep_cases.visits_case(seed, n, persons=max(2, n // 40), entities=50, negative_ids=seed % 3 == 1)
        for top_n in (0, 1, 2, 5, 100, 2 ** 40):
            s, t, w = edge_cases.count_edges(p, e, top_n)
            op, oe, orat = oracle.calc_ratings(p, e, top_n)
            assert np.array_equal(s, op) and np.array_equal(t, oe)
            for src in np.unique(s):                                   # weight = count / the source's kept total
                total = int(orat[op == src].sum())
                assert np.array_equal(w[s == src], orat[op == src] / float(total))
