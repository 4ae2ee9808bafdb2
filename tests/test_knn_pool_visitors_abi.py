"""CPU checks of the pool-visitors boundary (locrec_knn_pool_visitors_*): header, library and binding name the three
functions, the argument checks that need no device, the Python mirror's requires.  What the calls compute is checked on
the GPU (tests/test_gpu_knn_pool_visitors.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locrec_knn_pool_visitors_recommend_batch", "locrec_knn_pool_visitors_recommend_ranked_batch",
         "locrec_knn_pool_visitors_stats")


def test_header_library_and_binding_name_the_three_functions(pkg):
    from locations_recommender_amd import _lib as L
    with open(os.path.join(ROOT, "include", "locrec.h")) as f:
        header = f.read()
    lib = L.lib()
    for name in NAMES:
        assert re.search(r"\bint32_t %s\(" % name, header), name
        assert name in L.SIGNATURES and callable(getattr(lib, name))
        decl = re.search(r"\bint32_t %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name]), name      # the binding's argument counts are the header's
    # the pool forms take the per-index forms' arguments behind the pool and the index positions
    for name in NAMES[:2]:
        assert len(L.SIGNATURES[name]) == len(L.SIGNATURES[name.replace("_pool_", "_")]) + 1


def test_a_null_pool_is_refused_with_nothing_written(pkg):
    from locations_recommender_amd import _lib as L
    lib = L.lib()
    six = [None] * 6
    bad, cnt, cap, off = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    assert lib.locrec_knn_pool_visitors_recommend_batch(None, 0, None, *six, L.MEM_HOST, 0.5, 0.5, 10, C.byref(off), None, None,
                                                        C.byref(cap), C.byref(bad)) == L.E_INVALID_ARG
    assert "pool is NULL" in lib.locrec_last_error().decode()
    assert (off.value, cap.value, bad.value) == (-7, -7, -7)
    assert lib.locrec_knn_pool_visitors_recommend_ranked_batch(None, 0, None, *six, L.MEM_HOST, 0.5, 0.5, 10, 0, None, None, None, 10,
                                                               None, None, None, None, C.byref(cnt), C.byref(bad)) == L.E_INVALID_ARG
    assert "pool is NULL" in lib.locrec_last_error().decode() and (cnt.value, bad.value) == (-7, -7)


def test_stats_refuse_null_and_are_non_negative(pkg):
    from locations_recommender_amd import _lib as L, knn
    lib = L.lib()
    assert lib.locrec_knn_pool_visitors_stats(None) == L.E_INVALID_ARG
    out = (C.c_int64 * 12)(*[-1] * 12)
    assert lib.locrec_knn_pool_visitors_stats(out) == L.OK and all(x >= 0 for x in out)
    assert knn.KnnPool.VISITOR_STATS == ("waves", "member_tiles", "stage_launches", "fill_launches", "scan_launches",
                                         "aggregate_launches", "finish_launches", "delegated_members", "beyond", "emitted_rows",
                                         "readback_bytes", "host_syncs")
    st = knn.KnnPool.visitors_stats()
    assert tuple(st) == knn.KnnPool.VISITOR_STATS and all(v >= 0 for v in st.values())


def test_python_surface_and_its_requires(pkg):
    from locations_recommender_amd import _lib as L, knn, mains
    P = knn.KnnPool
    vectors = ["p_rowptr", "p_idx", "p_val", "c_rowptr", "c_idx", "c_val"]
    assert list(inspect.signature(P.visitors_recommend_batch).parameters) == ["self", "index_of", *vectors, "pw", "cw", "k"]
    assert list(inspect.signature(P.visitors_recommend_ranked_batch).parameters) == [
        "self", "index_of", *vectors, "pw", "cw", "k", "place_ids", "place_region_ids", "target_region_ids", "max_recommendations",
        "exclude"]
    assert inspect.signature(P.visitors_recommend_ranked_batch).parameters["exclude"].default is None
    sig = inspect.signature(mains.knn_visitor_requests_pooled)
    assert list(sig.parameters) == ["data_dir", "visits", "home_region_ids", "target_region_ids", "place_weight", "category_weight",
                                    "k_nearest", "max_recommendations", "new_places", "pooled"]
    assert sig.parameters["max_recommendations"].default == 10 and sig.parameters["new_places"].default is False
    assert isinstance(sig.parameters["pooled"].default, bool)
    # the mirror's requires, before any library call (a pool object that was never created: no handle is touched)
    pool = P.__new__(P)
    pool.indexes, pool._h = [], None
    one = (np.array([0, 1]), np.array([3], np.int32), np.array([1.0]))
    two = (np.array([0, 1, 2]), np.array([3, 4], np.int32), np.array([1.0, 2.0]))
    with pytest.raises(L.IllegalArgumentException, match="one index position per visitor"):
        pool.visitors_recommend_batch([0], *two, *two, 0.5, 0.5, 10)
    with pytest.raises(L.IllegalArgumentException, match="one index position per visitor"):
        pool.visitors_recommend_ranked_batch([0, 0, 0], *two, *two, 0.5, 0.5, 10, [1], [0], [0, 0], 5)
    with pytest.raises(L.IllegalArgumentException, match="one place and one category vector per visitor"):
        pool.visitors_recommend_batch([0], *one, *two, 0.5, 0.5, 10)
    with pytest.raises(L.IllegalArgumentException, match="one region per place and one target region per person"):
        pool.visitors_recommend_ranked_batch([0, 0], *two, *two, 0.5, 0.5, 10, [1], [0], [0], 5)
    with pytest.raises(L.IllegalArgumentException, match=r"one exclusion list per visitor \(nv \+ 1 offsets\)"):
        pool.visitors_recommend_ranked_batch([0, 0], *two, *two, 0.5, 0.5, 10, [1], [0], [0, 0], 5, exclude=([0, 1], [7]))
    with pytest.raises(L.IllegalArgumentException, match="the exclusion offsets end beyond the listed ids"):
        pool.visitors_recommend_ranked_batch([0, 0], *two, *two, 0.5, 0.5, 10, [1], [0], [0, 0], 5, exclude=([0, 1, 3], [7]))
    nv, gi, ptrs, mem, keep = P._visitor_pool_args([1, 0], *two, *two)
    assert nv == 2 and gi.dtype == np.int32 and gi.tolist() == [1, 0] and mem == L.MEM_HOST
    # the rows of a CSR as a CSR of their own (what the mains hand a call without the refused visitors)
    ptr, (idx, val) = mains._csr_rows(np.array([0, 2, 2, 5]), (np.array([1, 2, 3, 4, 5], np.int32), np.arange(5.0)), [2, 0])
    assert ptr.tolist() == [0, 3, 5] and idx.tolist() == [3, 4, 5, 1, 2] and idx.dtype == np.int32 and val.tolist() == [2.0, 3.0, 4.0, 0.0, 1.0]
    assert mains._per_visitor({7: 1, 9: 2}, np.array([7, 9]), "home").tolist() == [1, 2]
    assert mains._per_visitor(3, np.array([7, 9]), "home").tolist() == [3, 3]
    with pytest.raises(L.IllegalArgumentException, match="one target region per visitor"):
        mains._per_visitor([1], np.array([7, 9]), "target")
