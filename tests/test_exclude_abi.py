"""CPU checks of the "only new places" boundary - locrec_rank_recommendations_batch_excluding,
locrec_knn_recommend_ranked_batch_unvisited, locrec_knn_fetch_ranked_unvisited and
locrec_sg_recommend_ranked_batch_excluding: the symbols exist with their arities, and the NULL and range refusals,
the host offsets of the _excluding calls among them, answer LOCREC_E_INVALID_ARG before any device work."""
import ctypes as C
import inspect

import numpy as np
import pytest

ARITY = {"locrec_rank_recommendations_batch_excluding": 17, "locrec_knn_recommend_ranked_batch_unvisited": 14,
         "locrec_knn_fetch_ranked_unvisited": 10, "locrec_sg_recommend_ranked_batch_excluding": 20}
BAD_OFFSETS = {"decreasing": [0, 4, 2, 6], "negative": [-1, 2, 4, 6], "beyond": [0, 2, 4, 7]}


def test_symbols_exist_and_prototypes_bind(pkg):
    from locations_recommender_amd import _lib as L
    raw = C.CDLL(pkg.LIB_PATH)
    for name, arity in ARITY.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(L.SIGNATURES[name]) == arity
        assert getattr(L.lib(), name).argtypes == L.SIGNATURES[name]
    # each takes its plain sibling's arguments, the _excluding calls three more
    assert len(L.SIGNATURES["locrec_rank_recommendations_batch"]) == 17 - 3
    assert L.SIGNATURES["locrec_knn_recommend_ranked_batch_unvisited"] == L.SIGNATURES["locrec_knn_recommend_ranked_batch"]
    assert L.SIGNATURES["locrec_knn_fetch_ranked_unvisited"] == L.SIGNATURES["locrec_knn_fetch_ranked"]
    assert len(L.SIGNATURES["locrec_sg_recommend_ranked_batch"]) == 20 - 3


def test_python_surface(pkg):
    from locations_recommender_amd import mains, stochastic
    assert inspect.signature(pkg.KnnIndex.recommend_ranked_batch).parameters["unvisited"].default is False
    assert inspect.signature(pkg.KnnIndex.fetch_ranked).parameters["unvisited"].default is False
    assert inspect.signature(pkg.SgGraph.recommend_ranked_batch).parameters["excluded"].default is None
    assert list(inspect.signature(pkg.prep.rank_recommendations_batch_excluding).parameters)[-2:] == ["excluded_offsets", "excluded_ids"]
    assert callable(stochastic.out_neighbours)
    for f in ("knn_recommend_places_batch", "knn_recommender_request", "sg_recommend_places_batch", "sg_recommender_request"):
        assert inspect.signature(getattr(mains, f)).parameters["new_places"].default is False
    # the two request loops keep their pinned signatures (test_knn_pool_abi, test_sg_pool_abi): their siblings
    assert list(inspect.signature(mains.knn_recommender_requests_new_places).parameters) == [
        "data_dir", "persons", "lines", "place_weight", "category_weight", "k_nearest", "max_recommendations"]
    assert list(inspect.signature(mains.sg_recommender_requests_new_places).parameters) == [
        "data_dir", "persons", "lines", "epsilon", "max_iterations", "max_recommendations", "pooled"]


def p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def rank_call(L, excluded_offsets, n_excluded=6, excluded_ids=True, n_segments=3, outs=None):
    from locations_recommender_amd import _lib
    a = dict(off=np.array([0, 2, 4, 6], np.int64), ids=np.arange(6, dtype=np.int64), scores=np.ones(6),
             pl=np.arange(6, dtype=np.int64), reg=np.zeros(6, np.int64), tgt=np.zeros(3, np.int64),
             xoff=None if excluded_offsets is None else np.array(excluded_offsets, np.int64),
             xid=np.arange(8, dtype=np.int64) if excluded_ids else None)
    oi, osc, oc = outs
    return L.lib().locrec_rank_recommendations_batch_excluding(
        n_segments, p(a["off"]), 6, p(a["ids"]), p(a["scores"]), 6, p(a["pl"]), p(a["reg"]), p(a["tgt"]), 2, p(a["xoff"]),
        n_excluded, p(a["xid"]), _lib.MEM_HOST, p(oi), p(osc), p(oc))


def test_ranker_refusals_need_no_device(pkg):
    from locations_recommender_amd import _lib as L
    outs = np.full(6, 77, np.int64), np.full(6, 7.5), np.full(3, 77, np.int64)
    for bad in BAD_OFFSETS.values():
        assert rank_call(L, bad, outs=outs) == L.E_INVALID_ARG
        assert b"excluded_offsets" in L.lib().locrec_last_error()
    assert rank_call(L, None, outs=outs) == L.E_INVALID_ARG                                  # NULL offsets
    assert rank_call(L, [0, 2, 4, 6], excluded_ids=False, outs=outs) == L.E_INVALID_ARG      # NULL ids with n_excluded > 0
    assert rank_call(L, [0, 0, 0, 0], n_excluded=-1, outs=outs) == L.E_INVALID_ARG
    assert rank_call(L, [0, 0, 0, 0], n_excluded=2 ** 31, outs=outs) == L.E_INVALID_ARG
    assert rank_call(L, [0, 2, 4, 6], n_segments=-1, outs=outs) == L.E_INVALID_ARG
    assert (outs[0] == 77).all() and (outs[1] == 7.5).all() and (outs[2] == 77).all()        # nothing written
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.prep.rank_recommendations_batch_excluding([0, 2], [1, 2], [1.0, 2.0], [1], [0], [0], 5, [0, 3], [1, 2])


def sg_call(L, graph, v, excluded_offsets, n_excluded, outs, n=3):
    pl, reg, tgt = np.array([1, 2], np.int64), np.array([0, 0], np.int64), np.zeros(3, np.int64)
    xoff = None if excluded_offsets is None else np.array(excluded_offsets, np.int64)
    xid = np.arange(8, dtype=np.int64)
    oi, op, cnt, rows, its, conv = outs
    return L.lib().locrec_sg_recommend_ranked_batch_excluding(
        graph, n, L.ptr(v, C.c_int64), 0.15, 0.01, 20, 2, L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), 4,
        L.ptr(xoff, C.c_int64), n_excluded, L.ptr(xid, C.c_int64), L.ptr(oi, C.c_int64), L.ptr(op, C.c_double),
        L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64), L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32))


def test_sg_refusals_need_no_device(pkg):
    from locations_recommender_amd import _lib as L
    outs = (np.full(12, -7, np.int64), np.full(12, -7.0), np.full(3, -7, np.int64), np.full(3, -7, np.int64),
            np.full(3, -7, np.int64), np.full(3, -7, np.int32))
    v = np.array([1, 2, 3], np.int64)
    assert sg_call(L, None, v, [0, 2, 4, 6], 6, outs) == L.E_INVALID_ARG
    assert b"graph is NULL" in L.lib().locrec_last_error()
    # the lists are refused before the handle is looked at: any non-NULL address will do
    not_a_graph = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    for bad in BAD_OFFSETS.values():
        assert sg_call(L, not_a_graph, v, bad, 6, outs) == L.E_INVALID_ARG
        assert b"excluded_offsets" in L.lib().locrec_last_error()
    assert sg_call(L, not_a_graph, v, None, 6, outs) == L.E_INVALID_ARG
    assert sg_call(L, not_a_graph, v, [0, 0, 0, 0], -1, outs) == L.E_INVALID_ARG
    assert sg_call(L, not_a_graph, v, [0, 0, 0, 0], 2 ** 31, outs) == L.E_INVALID_ARG
    assert sg_call(L, not_a_graph, None, [0, 2, 4, 6], 6, outs) == L.E_INVALID_ARG
    for o in outs:
        assert (o == -7).all()


def test_knn_refusals_need_no_device(pkg):
    from locations_recommender_amd import _lib as L
    pl, reg, tgt, q = np.array([1, 2], np.int64), np.zeros(2, np.int64), np.zeros(2, np.int64), np.array([5, 6], np.int64)
    oi, osc, cnt = np.full(8, -7, np.int64), np.full(8, -7.0), np.full(2, -7, np.int64)
    tail = (2, L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), 4, L.ptr(oi, C.c_int64), L.ptr(osc, C.c_double),
            L.ptr(cnt, C.c_int64))
    assert L.lib().locrec_knn_recommend_ranked_batch_unvisited(None, 2, L.ptr(q, C.c_int64), 0.5, 0.5, 10, *tail) == L.E_INVALID_ARG
    assert L.lib().locrec_knn_fetch_ranked_unvisited(None, 2, *tail) == L.E_INVALID_ARG
    assert b"index is NULL" in L.lib().locrec_last_error()
    assert (oi == -7).all() and (osc == -7.0).all() and (cnt == -7).all()
