"""CPU checks of the pool's boundary (locrec_sg_pool_*): the argument checks that need no device, and the Python
surface.  What the pool computes is checked on the GPU (tests/test_gpu_sg_pool.py)."""
import ctypes as C
import inspect


def test_pool_entry_points_check_their_arguments_without_a_device(pkg):
    from locations_recommender_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    for graphs, n in ((None, 1), ((C.c_void_p * 1)(None), 0), ((C.c_void_p * 1)(None), 65536)):
        assert lib.locrec_sg_pool_create(graphs, n, C.byref(h)) == L.E_INVALID_ARG and not h.value
        assert "1 .. 65535 graphs" in lib.locrec_last_error().decode()
    assert lib.locrec_sg_pool_create((C.c_void_p * 1)(None), 1, C.byref(h)) == L.E_INVALID_ARG
    assert "graph 0 is NULL" in lib.locrec_last_error().decode()
    assert lib.locrec_sg_pool_create((C.c_void_p * 1)(None), 1, None) == L.E_INVALID_ARG
    cap, off = C.c_int64(0), C.c_int64(-7)
    assert lib.locrec_sg_pool_recommend_batch(None, 0, None, None, 0.15, 0.01, 20, C.byref(off), None, None, C.byref(cap),
                                              None, None, None) == L.E_INVALID_ARG
    assert "pool is NULL" in lib.locrec_last_error().decode() and off.value == -7
    lib.locrec_sg_pool_destroy(None)
    assert lib.locrec_sg_pool_stats(None, None, None, None, None, None) == L.OK
    rounds = C.c_int64(-1)
    assert lib.locrec_sg_pool_stats(None, C.byref(rounds), None, None, None, None) == L.OK and rounds.value >= 0


def test_python_surface(pkg):
    from locations_recommender_amd import mains, stochastic
    assert pkg.SgPool is stochastic.SgPool
    assert stochastic.SgPool.STATS == ("tile_waves", "rounds", "sweep_launches", "finalize_launches", "polls", "readback_bytes")
    for name in ("recommend_batch", "stats", "close"):
        assert callable(getattr(stochastic.SgPool, name))
    sig = inspect.signature(mains.sg_recommender_requests)
    assert list(sig.parameters) == ["data_dir", "persons", "lines", "epsilon", "max_iterations", "max_recommendations", "pooled"]
    assert sig.parameters["max_recommendations"].default == 10 and isinstance(sig.parameters["pooled"].default, bool)
