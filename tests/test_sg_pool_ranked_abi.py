"""CPU checks of the ranked pool's boundary (locrec_sg_pool_recommend_ranked_batch and its stats entry): the symbols exist,
the prototypes bind, the argument check that needs no device answers LOCREC_E_INVALID_ARG with nothing written, and the
Python surface is there.  What the call computes is checked on the GPU (tests/test_gpu_sg_pool_ranked.py)."""
import ctypes as C
import inspect

import numpy as np

NAMES = ("locrec_sg_pool_recommend_ranked_batch", "locrec_sg_pool_recommend_ranked_batch_stats")


def test_symbols_exist_and_prototypes_bind(pkg):
    from locations_recommender_amd import _lib as L
    raw = C.CDLL(pkg.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in L.SIGNATURES
        assert getattr(L.lib(), n).argtypes == L.SIGNATURES[n]
    assert len(L.SIGNATURES["locrec_sg_pool_recommend_ranked_batch"]) == 19
    assert len(L.SIGNATURES["locrec_sg_pool_recommend_ranked_batch_stats"]) == 8


def test_null_pool_is_refused_with_nothing_written(pkg):
    from locations_recommender_amd import _lib as L
    n, stride = 3, 4
    gi, v = np.array([0, 0, 1], np.int32), np.array([1, 2, 3], np.int64)
    pl, reg, tgt = np.array([1, 2], np.int64), np.array([0, 0], np.int64), np.zeros(n, np.int64)
    oi, op = np.full(n * stride, -7, np.int64), np.full(n * stride, -7.0)
    cnt, rows, its, conv = (np.full(n, -7, np.int64), np.full(n, -7, np.int64), np.full(n, -7, np.int64),
                            np.full(n, -7, np.int32))
    bad = C.c_int64(-5)
    status = L.lib().locrec_sg_pool_recommend_ranked_batch(
        None, n, L.ptr(gi, C.c_int32), L.ptr(v, C.c_int64), 0.15, 0.01, 20, 2, L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64),
        L.ptr(tgt, C.c_int64), stride, L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64),
        L.ptr(rows, C.c_int64), L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32), C.byref(bad))
    assert status == L.E_INVALID_ARG and b"pool is NULL" in L.lib().locrec_last_error()
    for o in (oi, op, cnt, rows, its, conv):
        assert (o == -7).all()
    assert bad.value == -5


def test_stats_entry_accepts_nulls(pkg):
    from locations_recommender_amd import _lib as L
    assert L.lib().locrec_sg_pool_recommend_ranked_batch_stats(None, None, None, None, None, None, None, None) == L.OK
    tiles = C.c_int64(-1)
    assert L.lib().locrec_sg_pool_recommend_ranked_batch_stats(None, C.byref(tiles), None, None, None, None, None, None) == L.OK
    assert tiles.value >= 0
    st = pkg.SgPool.ranked_stats()
    assert tuple(st) == pkg.SgPool.RANKED_STATS and all(isinstance(x, int) and x >= 0 for x in st.values())


def test_python_surface(pkg):
    from locations_recommender_amd import mains
    assert pkg.SgPool.RANKED_STATS == ("tile_waves", "tiles", "rounds", "groups", "emit_launches", "emitted_rows",
                                       "readback_bytes", "host_syncs")
    assert list(inspect.signature(pkg.SgPool.recommend_ranked_batch).parameters) == [
        "self", "graph_index", "vertex_ids", "alpha", "epsilon", "max_iterations", "place_ids", "place_region_ids",
        "target_region_ids", "max_recommendations"]
    assert callable(pkg.SgPool.ranked_stats)
    sig = inspect.signature(mains.sg_recommender_requests_ranked)
    assert list(sig.parameters) == ["data_dir", "persons", "lines", "epsilon", "max_iterations", "max_recommendations"]
    assert sig.parameters["max_recommendations"].default == 10
    # the unranked main keeps its signature
    sig = inspect.signature(mains.sg_recommender_requests)
    assert list(sig.parameters) == ["data_dir", "persons", "lines", "epsilon", "max_iterations", "max_recommendations", "pooled"]
    assert sig.parameters["max_recommendations"].default == 10 and sig.parameters["pooled"].default is True
    assert pkg.SgPool.STATS == ("tile_waves", "rounds", "sweep_launches", "finalize_launches", "polls", "readback_bytes")
