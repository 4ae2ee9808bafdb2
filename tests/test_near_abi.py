"""CPU checks of the "within reach" boundary - locrec_rank_recommendations_batch_near,
locrec_knn_recommend_ranked_batch_near and locrec_sg_recommend_ranked_batch_near: the symbols exist with their arities,
the Python surface has its names and defaults, and with host arrays a bad radius, centre, place coordinate or list
answers LOCREC_E_INVALID_ARG before any device work - for the KNN and SG calls before the handle is looked at."""
import ctypes as C
import inspect

import numpy as np
import pytest

ARITY = {"locrec_rank_recommendations_batch_near": 23, "locrec_knn_recommend_ranked_batch_near": 21,
         "locrec_sg_recommend_ranked_batch_near": 26}
BAD_OFFSETS = {"decreasing": [0, 4, 2, 6], "negative": [-1, 2, 4, 6], "beyond": [0, 2, 4, 7]}
# what is wrong -> (the argument, its three values, the word the message must hold)
BAD_CIRCLES = {"nan radius": ("rad", [1.0, np.nan, 1.0], b"radius_meters"),
               "negative radius": ("rad", [1.0, 1.0, -1e-300], b"radius_meters"),
               "-inf radius": ("rad", [-np.inf, 1.0, 1.0], b"radius_meters"),
               "latitude beyond the pole": ("clat", [10.0, 90.0000001, 10.0], b"center_latitudes"),
               "nan longitude": ("clon", [10.0, 10.0, np.nan], b"center_longitudes")}


def test_symbols_exist_and_prototypes_bind(pkg):
    from locations_recommender_amd import _lib as L
    raw = C.CDLL(pkg.LIB_PATH)
    for name, arity in ARITY.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(L.SIGNATURES[name]) == arity
        assert getattr(L.lib(), name).argtypes == L.SIGNATURES[name]
    # the excluding ranker's arguments, five coordinate arrays and out_meters
    assert len(L.SIGNATURES["locrec_rank_recommendations_batch_excluding"]) == 23 - 6
    # the ranked batch's, the five arrays, the unvisited flag and out_meters
    assert len(L.SIGNATURES["locrec_knn_recommend_ranked_batch"]) == 21 - 7
    assert len(L.SIGNATURES["locrec_sg_recommend_ranked_batch_excluding"]) == 26 - 6


def test_python_surface(pkg):
    from locations_recommender_amd import mains
    assert list(inspect.signature(pkg.prep.rank_recommendations_batch_near).parameters) == [
        "offsets", "ids", "scores", "place_ids", "place_region_ids", "place_latitudes", "place_longitudes", "target_region_ids",
        "center_latitudes", "center_longitudes", "radius_meters", "max_recommendations", "excluded_offsets", "excluded_ids"]
    sig = inspect.signature(pkg.prep.rank_recommendations_batch_near).parameters
    assert sig["excluded_offsets"].default is None and sig["excluded_ids"].default is None
    sig = inspect.signature(pkg.KnnIndex.recommend_ranked_batch_near).parameters
    assert sig["unvisited"].default is False and list(sig)[-6:-1] == [
        "target_region_ids", "center_latitudes", "center_longitudes", "radius_meters", "max_recommendations"]
    sig = inspect.signature(pkg.SgGraph.recommend_ranked_batch_near).parameters
    assert sig["excluded"].default is None and sig["on_device"].default is True
    assert list(inspect.signature(mains.knn_recommender_requests_near).parameters) == [
        "data_dir", "persons", "lines", "positions", "radius_meters", "place_weight", "category_weight", "k_nearest",
        "max_recommendations", "new_places"]
    assert list(inspect.signature(mains.sg_recommender_requests_near).parameters) == [
        "data_dir", "persons", "lines", "positions", "radius_meters", "epsilon", "max_iterations", "max_recommendations",
        "new_places"]
    for f in (mains.knn_recommender_requests_near, mains.sg_recommender_requests_near):
        p = inspect.signature(f).parameters
        assert p["max_recommendations"].default == 10 and p["new_places"].default is False


def p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def arrays(**changed):
    """Three segments of two rows over six places on the equator; `changed` replaces an array (None: NULL)."""
    a = dict(off=np.array([0, 2, 4, 6], np.int64), ids=np.arange(6, dtype=np.int64), scores=np.ones(6),
             pl=np.arange(6, dtype=np.int64), reg=np.zeros(6, np.int64), plat=np.zeros(6), plon=np.linspace(-180.0, 180.0, 6),
             tgt=np.zeros(3, np.int64), clat=np.zeros(3), clon=np.zeros(3), rad=np.array([0.0, 10.0, np.inf]),
             xoff=None, xid=np.arange(8, dtype=np.int64))
    for k, v in changed.items():
        a[k] = None if v is None else np.array(v, a[k].dtype if a[k] is not None else np.int64)
    return a


def rank_call(L, outs, n_excluded=6, n_segments=3, **changed):
    from locations_recommender_amd import _lib
    a = arrays(**changed)
    oi, osc, om, oc = outs
    return L.lib().locrec_rank_recommendations_batch_near(
        n_segments, p(a["off"]), 6, p(a["ids"]), p(a["scores"]), 6, p(a["pl"]), p(a["reg"]), p(a["plat"]), p(a["plon"]),
        p(a["tgt"]), p(a["clat"]), p(a["clon"]), p(a["rad"]), 2, p(a["xoff"]), n_excluded, p(a["xid"]), _lib.MEM_HOST,
        p(oi), p(osc), p(om), p(oc))


def test_ranker_refusals_need_no_device(pkg):
    from locations_recommender_amd import _lib as L
    outs = np.full(6, 77, np.int64), np.full(6, 7.5), np.full(6, 7.5), np.full(3, 77, np.int64)
    for what, (name, values, word) in BAD_CIRCLES.items():
        assert rank_call(L, outs, **{name: values}) == L.E_INVALID_ARG, what
        assert word in L.lib().locrec_last_error(), what
    assert rank_call(L, outs, plon=[0.0, 1.0, -180.5, 2.0, 3.0, 4.0]) == L.E_INVALID_ARG
    assert b"place_longitudes" in L.lib().locrec_last_error()
    for name in ("plat", "plon", "clat", "clon", "rad"):
        assert rank_call(L, outs, **{name: None}) == L.E_INVALID_ARG, name               # NULL with n_places, n_segments > 0
    for bad in BAD_OFFSETS.values():
        assert rank_call(L, outs, xoff=bad) == L.E_INVALID_ARG
        assert b"excluded_offsets" in L.lib().locrec_last_error()
    assert rank_call(L, outs, xoff=[0, 2, 4, 6], xid=None) == L.E_INVALID_ARG               # NULL ids with n_excluded > 0
    assert rank_call(L, outs, xoff=[0, 0, 0, 0], n_excluded=-1) == L.E_INVALID_ARG
    assert rank_call(L, outs, xoff=[0, 0, 0, 0], n_excluded=2 ** 31) == L.E_INVALID_ARG
    assert rank_call(L, outs, n_segments=-1) == L.E_INVALID_ARG
    assert (outs[0] == 77).all() and (outs[1] == 7.5).all() and (outs[2] == 7.5).all() and (outs[3] == 77).all()
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.prep.rank_recommendations_batch_near([0, 2], [1, 2], [1.0, 2.0], [1], [0], [0.0], [0.0], [0], [0.0], [0.0], [np.nan], 5)


def sg_call(L, graph, outs, n_excluded=6, **changed):
    a = arrays(**changed)
    v = np.array([1, 2, 3], np.int64)
    oi, op, om, cnt, rows, its, conv = outs
    f64 = lambda x: L.ptr(x, C.c_double)
    i64 = lambda x: L.ptr(x, C.c_int64)
    return L.lib().locrec_sg_recommend_ranked_batch_near(
        graph, 3, i64(v), 0.15, 0.01, 20, 6, i64(a["pl"]), i64(a["reg"]), f64(a["plat"]), f64(a["plon"]), i64(a["tgt"]),
        f64(a["clat"]), f64(a["clon"]), f64(a["rad"]), 4, i64(a["xoff"]), n_excluded, i64(a["xid"]), i64(oi), f64(op), f64(om),
        i64(cnt), i64(rows), i64(its), L.ptr(conv, C.c_int32))


def test_sg_refusals_come_before_the_handle(pkg):
    from locations_recommender_amd import _lib as L
    outs = (np.full(12, -7, np.int64), np.full(12, -7.0), np.full(12, -7.0), np.full(3, -7, np.int64), np.full(3, -7, np.int64),
            np.full(3, -7, np.int64), np.full(3, -7, np.int32))
    assert sg_call(L, None, outs) == L.E_INVALID_ARG
    assert b"graph is NULL" in L.lib().locrec_last_error()
    not_a_graph = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)      # any non-NULL address will do
    for what, (name, values, word) in BAD_CIRCLES.items():
        assert sg_call(L, not_a_graph, outs, **{name: values}) == L.E_INVALID_ARG, what
        assert word in L.lib().locrec_last_error(), what
    assert sg_call(L, not_a_graph, outs, plon=[0.0, 1.0, -180.5, 2.0, 3.0, 4.0]) == L.E_INVALID_ARG
    assert b"place_longitudes" in L.lib().locrec_last_error()
    assert sg_call(L, not_a_graph, outs, plat=None) == L.E_INVALID_ARG
    for bad in BAD_OFFSETS.values():
        assert sg_call(L, not_a_graph, outs, xoff=bad) == L.E_INVALID_ARG
        assert b"excluded_offsets" in L.lib().locrec_last_error()
    assert sg_call(L, not_a_graph, outs, xoff=[0, 0, 0, 0], n_excluded=-1) == L.E_INVALID_ARG
    for o in outs:
        assert (o == -7).all()


def knn_call(L, index, outs, **changed):
    a = arrays(**changed)
    q = np.array([5, 6, 7], np.int64)
    oi, osc, om, cnt = outs
    f64 = lambda x: L.ptr(x, C.c_double)
    i64 = lambda x: L.ptr(x, C.c_int64)
    return L.lib().locrec_knn_recommend_ranked_batch_near(
        index, 3, i64(q), 0.5, 0.5, 10, 6, i64(a["pl"]), i64(a["reg"]), f64(a["plat"]), f64(a["plon"]), i64(a["tgt"]),
        f64(a["clat"]), f64(a["clon"]), f64(a["rad"]), 4, 0, i64(oi), f64(osc), f64(om), i64(cnt))


def test_knn_refusals_come_before_the_handle(pkg):
    from locations_recommender_amd import _lib as L
    outs = np.full(12, -7, np.int64), np.full(12, -7.0), np.full(12, -7.0), np.full(3, -7, np.int64)
    assert knn_call(L, None, outs) == L.E_INVALID_ARG
    assert b"index is NULL" in L.lib().locrec_last_error()
    not_an_index = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    for what, (name, values, word) in BAD_CIRCLES.items():
        assert knn_call(L, not_an_index, outs, **{name: values}) == L.E_INVALID_ARG, what
        assert word in L.lib().locrec_last_error(), what
    assert knn_call(L, not_an_index, outs, plon=[0.0, 1.0, -180.5, 2.0, 3.0, 4.0]) == L.E_INVALID_ARG
    assert b"place_longitudes" in L.lib().locrec_last_error()
    assert knn_call(L, not_an_index, outs, plon=None) == L.E_INVALID_ARG
    for o in outs:
        assert (o == -7).all()
