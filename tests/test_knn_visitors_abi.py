"""CPU checks of the visitors' boundary (locrec_knn_visitors_*): header, library and binding name the four functions, the
argument checks that need no device, the Python mirror's requires.  What the calls compute is checked on the GPU
(tests/test_gpu_knn_visitors.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locrec_knn_visitors_query_batch", "locrec_knn_visitors_recommend_batch",
         "locrec_knn_visitors_recommend_ranked_batch", "locrec_knn_visitors_stats")


def test_header_library_and_binding_name_the_four_functions(pkg):
    from locations_recommender_amd import _lib as L
    with open(os.path.join(ROOT, "include", "locrec.h")) as f:
        header = f.read()
    lib = L.lib()
    for name in NAMES:
        assert re.search(r"\bint32_t %s\(" % name, header), name
        assert name in L.SIGNATURES and callable(getattr(lib, name))
    # the binding's argument counts are the header's
    for name in NAMES:
        decl = re.search(r"\bint32_t %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name]), name


def test_entry_points_check_their_arguments_without_a_device(pkg):
    from locations_recommender_amd import _lib as L
    lib = L.lib()
    bad, cnt, cap, off = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    six = [None] * 6
    assert lib.locrec_knn_visitors_query_batch(None, 0, *six, L.MEM_HOST, 0.5, 0.5, 10, None, None, C.byref(cnt),
                                               C.byref(bad)) == L.E_INVALID_ARG
    assert "index is NULL" in lib.locrec_last_error().decode() and bad.value == -1 and cnt.value == -7
    bad = C.c_int64(-7)
    assert lib.locrec_knn_visitors_recommend_batch(None, 0, *six, L.MEM_HOST, 0.5, 0.5, 10, C.byref(off), None, None, C.byref(cap),
                                                   C.byref(bad)) == L.E_INVALID_ARG
    assert "index is NULL" in lib.locrec_last_error().decode() and off.value == -7 and cap.value == -7 and bad.value == -1
    assert lib.locrec_knn_visitors_recommend_ranked_batch(None, 0, *six, L.MEM_HOST, 0.5, 0.5, 10, 0, None, None, None, 10, None, None,
                                                          None, None, C.byref(cnt), None) == L.E_INVALID_ARG
    assert "index is NULL" in lib.locrec_last_error().decode() and cnt.value == -7
    assert lib.locrec_knn_visitors_stats(None) == L.E_INVALID_ARG
    out = (C.c_int64 * 8)(*[-1] * 8)
    assert lib.locrec_knn_visitors_stats(out) == L.OK and all(x >= 0 for x in out)
    assert lib.locrec_knn_destroy(None) == L.OK


def test_python_surface_and_its_requires(pkg):
    from locations_recommender_amd import _lib as L, knn, mains, prep
    K = knn.KnnIndex
    assert K.VISITOR_STATS == ("tiles", "tiles_all", "tiles_topk", "beyond", "renumbered", "stage_launches", "scan_launches",
                               "host_syncs")
    assert set(K.visitors_stats()) == set(K.VISITOR_STATS)
    for name in ("visitors_query_batch", "visitors_recommend_batch", "visitors_recommend_ranked_batch"):
        assert list(inspect.signature(getattr(K, name)).parameters)[1:10] == [
            "p_rowptr", "p_idx", "p_val", "c_rowptr", "c_idx", "c_val", "pw", "cw", "k"]
    assert inspect.signature(K.visitors_recommend_ranked_batch).parameters["exclude"].default is None
    for name in ("findSimilarPersonsForVisitor", "makeRecommendationsForVisitor"):
        assert list(inspect.signature(getattr(knn.KnnRecommender, name)).parameters) == ["self", "placeVector", "categoryVector"]
    assert list(inspect.signature(prep.visitor_vectors).parameters) == ["visitor_ids", "place_ids", "category_ids", "places_top_n",
                                                                       "categories_top_n"]
    sig = inspect.signature(mains.knn_visitor_requests)
    assert list(sig.parameters) == ["data_dir", "region_ids", "visits", "target_region_ids", "place_weight", "category_weight",
                                    "k_nearest", "max_recommendations", "new_places"]
    assert sig.parameters["max_recommendations"].default == 10 and sig.parameters["new_places"].default is False
    # the mirror's requires, before any library call
    one = (np.array([0, 1]), np.array([3], np.int32), np.array([1.0]))
    with pytest.raises(L.IllegalArgumentException, match="one place and one category vector per visitor"):
        K._visitor_args(*one, np.array([0, 1, 2]), np.array([1, 2], np.int32), np.array([1.0, 1.0]))
    with pytest.raises(L.IllegalArgumentException, match="the dimension of the indices match the dimension of the values"):
        K._visitor_args(np.array([0, 1]), np.array([3, 4], np.int32), np.array([1.0]), *one)
    nv, ptrs, mem, keep = K._visitor_args(*one, *one)
    assert nv == 1 and mem == L.MEM_HOST and keep[1].dtype == np.int32 and keep[0].dtype == np.int64
    with pytest.raises(L.IllegalArgumentException, match="a visitor is a pair of SparseVectors"):
        knn.KnnRecommender._visitor_csr(knn.SparseVector(5, [1], [1.0]), ([1], [1.0]))
    csr = knn.KnnRecommender._visitor_csr(knn.SparseVector(5, [1, 3], [1.0, 2.0]), knn.SparseVector(2, [0], [4.0]))
    assert csr[0].tolist() == [0, 2] and csr[3].tolist() == [0, 1]
