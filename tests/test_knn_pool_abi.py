"""CPU checks of the KNN pool's boundary (locrec_knn_pool_*): the argument checks that need no device, and the Python
surface.  What the pool computes is checked on the GPU (tests/test_gpu_knn_pool.py)."""
import ctypes as C
import inspect


def test_pool_entry_points_check_their_arguments_without_a_device(pkg):
    from locations_recommender_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    for indexes, n in ((None, 1), ((C.c_void_p * 1)(None), 0), ((C.c_void_p * 1)(None), 65536)):
        assert lib.locrec_knn_pool_create(indexes, n, C.byref(h)) == L.E_INVALID_ARG and not h.value
        assert "1 .. 65535 indexes" in lib.locrec_last_error().decode()
    assert lib.locrec_knn_pool_create((C.c_void_p * 1)(None), 1, C.byref(h)) == L.E_INVALID_ARG and not h.value
    assert "index 0 is NULL" in lib.locrec_last_error().decode()
    assert lib.locrec_knn_pool_create((C.c_void_p * 1)(None), 1, None) == L.E_INVALID_ARG
    assert "out_pool is NULL" in lib.locrec_last_error().decode()
    cap, off, bad = C.c_int64(0), C.c_int64(-7), C.c_int64(-7)
    assert lib.locrec_knn_pool_recommend_batch(None, 0, None, None, 0.5, 0.5, 10, C.byref(off), None, None, C.byref(cap),
                                               C.byref(bad)) == L.E_INVALID_ARG
    assert "pool is NULL" in lib.locrec_last_error().decode() and off.value == -7 and bad.value == -7
    cnt = C.c_int64(-7)
    assert lib.locrec_knn_pool_recommend_ranked_batch(None, 0, None, None, 0.5, 0.5, 10, 0, None, None, None, 10, None, None,
                                                      C.byref(cnt), C.byref(bad)) == L.E_INVALID_ARG
    assert "pool is NULL" in lib.locrec_last_error().decode() and cnt.value == -7 and bad.value == -7
    lib.locrec_knn_pool_destroy(None)
    assert lib.locrec_knn_pool_stats(*[None] * 10) == L.OK
    waves = C.c_int64(-1)
    assert lib.locrec_knn_pool_stats(C.byref(waves), *[None] * 9) == L.OK and waves.value >= 0
    syncs = C.c_int64(-1)
    assert lib.locrec_knn_pool_stats(*[None] * 9, C.byref(syncs)) == L.OK and syncs.value >= 0


def test_python_surface(pkg):
    from locations_recommender_amd import _lib as L, knn, mains
    assert pkg.KnnPool is knn.KnnPool
    assert knn.KnnPool.STATS == ("waves", "member_tiles", "fill_launches", "scan_launches", "aggregate_launches",
                                 "finish_launches", "delegated_members", "emitted_rows", "readback_bytes", "host_syncs")
    assert len(L.SIGNATURES["locrec_knn_pool_stats"]) == len(knn.KnnPool.STATS)
    for name in ("recommend_batch", "recommend_ranked_batch", "stats", "close"):
        assert callable(getattr(knn.KnnPool, name))
    assert set(knn.KnnPool.stats()) == set(knn.KnnPool.STATS)
    sig = inspect.signature(mains.knn_recommender_requests)
    assert list(sig.parameters) == ["data_dir", "persons", "lines", "place_weight", "category_weight", "k_nearest",
                                    "max_recommendations", "pooled"]
    assert sig.parameters["max_recommendations"].default == 10 and isinstance(sig.parameters["pooled"].default, bool)
