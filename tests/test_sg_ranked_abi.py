"""CPU checks of the ranked SG batch's boundary (locrec_sg_recommend_ranked_batch and its stats entry): the symbols
exist, the prototypes bind, and the argument checks that need no device answer LOCREC_E_INVALID_ARG."""
import ctypes as C

import numpy as np

NAMES = ("locrec_sg_recommend_ranked_batch", "locrec_sg_recommend_ranked_batch_stats")


def test_symbols_exist_and_prototypes_bind(pkg):
    from locations_recommender_amd import _lib as L
    raw = C.CDLL(pkg.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in L.SIGNATURES
        assert getattr(L.lib(), n).argtypes == L.SIGNATURES[n]
    assert len(L.SIGNATURES["locrec_sg_recommend_ranked_batch"]) == 17
    assert len(L.SIGNATURES["locrec_sg_recommend_ranked_batch_stats"]) == 5
    assert hasattr(pkg.SgGraph, "ranked_batch_stats") and hasattr(pkg.StochasticRecommender, "makeRecommendationsRankedBatch")


def call(L, graph, n, v, outs):
    pl, reg, tgt = np.array([1, 2], np.int64), np.array([0, 0], np.int64), np.zeros(max(n, 1), np.int64)
    oi, op, cnt, rows, its, conv = outs
    return L.lib().locrec_sg_recommend_ranked_batch(
        graph, n, L.ptr(v, C.c_int64), 0.15, 0.01, 20, 2, L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), 4,
        L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64), L.ptr(its, C.c_int64),
        L.ptr(conv, C.c_int32))


def sentinel_outputs(n, stride):
    return (np.full(n * stride, -7, np.int64), np.full(n * stride, -7.0), np.full(n, -7, np.int64), np.full(n, -7, np.int64),
            np.full(n, -7, np.int64), np.full(n, -7, np.int32))


def test_argument_checks_need_no_device(pkg):
    from locations_recommender_amd import _lib as L
    outs = sentinel_outputs(3, 4)
    v = np.array([1, 2, 3], np.int64)
    assert call(L, None, 3, v, outs) == L.E_INVALID_ARG
    assert b"graph is NULL" in L.lib().locrec_last_error()
    # a NULL vertex_ids with n_targets > 0 is refused before the handle is looked at: any non-NULL address will do
    not_a_graph = C.create_string_buffer(1 << 16)
    assert call(L, C.cast(not_a_graph, C.c_void_p), 3, None, outs) == L.E_INVALID_ARG
    assert call(L, C.cast(not_a_graph, C.c_void_p), -1, v, outs) == L.E_INVALID_ARG
    for o in outs:
        assert (o == -7).all()


def test_stats_entry_answers_without_a_call(pkg):
    st = pkg.SgGraph.ranked_batch_stats()
    assert sorted(st) == sorted(("tiles", "groups", "emitted_rows", "readback_bytes", "host_syncs"))
    assert all(isinstance(x, int) and x >= 0 for x in st.values())
    from locations_recommender_amd import _lib as L
    assert L.lib().locrec_sg_recommend_ranked_batch_stats(None, None, None, None, None) == L.OK
