"""CPU checks of the offline evaluation's boundary - locrec_eval_ranked_batch, its stats call and locrec_holdout_split:
the symbols exist with their arities, the Python surface has its names and defaults, and with host arrays every refusal
of the header answers LOCREC_E_INVALID_ARG before any device work, the message naming the argument and nothing
written."""
import ctypes as C
import inspect

import numpy as np

ARITY = {"locrec_eval_ranked_batch": 16, "locrec_eval_ranked_batch_stats": 4, "locrec_holdout_split": 14}
BAD_OFFSETS = {"decreasing": [0, 4, 2, 6], "negative": [-1, 2, 4, 6], "beyond": [0, 2, 4, 7]}


def test_symbols_exist_and_prototypes_bind(pkg):
    from locations_recommender_amd import _lib as L
    raw = C.CDLL(pkg.LIB_PATH)
    for name, arity in ARITY.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(L.SIGNATURES[name]) == arity
        assert getattr(L.lib(), name).argtypes == L.SIGNATURES[name]
    assert pkg.prep.EVAL_MAX_CUTOFFS == 8


def test_python_surface(pkg):
    from locations_recommender_amd import mains
    prep = pkg.prep
    assert list(inspect.signature(prep.holdout_split).parameters) == ["place_visits", "cut_timestamp", "new_places_only"]
    assert inspect.signature(prep.holdout_split).parameters["new_places_only"].default is True
    assert list(inspect.signature(prep.relevant_lists).parameters) == ["held", "person_ids", "target_region_ids"]
    assert list(inspect.signature(prep.evaluate_ranked).parameters) == [
        "rec_ids", "rec_counts", "rel_offsets", "rel_ids", "cutoffs", "per_segment"]
    assert inspect.signature(prep.evaluate_ranked).parameters["per_segment"].default is False
    assert callable(prep.evaluate_ranked_stats)
    assert list(inspect.signature(mains.knn_holdout_evaluation).parameters) == [
        "place_visits", "places", "cut_timestamp", "place_weight", "category_weight", "k_nearest", "cutoffs", "new_places", "batch"]
    assert list(inspect.signature(mains.sg_holdout_evaluation).parameters) == [
        "place_visits", "places", "cut_timestamp", "alpha", "epsilon", "max_iterations", "beta_person_place",
        "beta_person_category", "cutoffs", "new_places", "batch"]
    for f in (mains.knn_holdout_evaluation, mains.sg_holdout_evaluation):
        p = inspect.signature(f).parameters
        assert p["new_places"].default is True and p["batch"].default == 16384


def test_relevant_lists_on_host_arrays(pkg):
    """The search over the sorted triples needs no device for numpy columns."""
    held = {"person_id": np.array([-4, 1, 1, 1, 2], np.int64), "region_id": np.array([2, 0, 0, 3, 1], np.int64),
            "place_id": np.array([5, 7, 8, 1, 9], np.int64)}
    off, ids = pkg.prep.relevant_lists(held, [1, 2, 1, 9, -4, 1, 2], [0, 1, 3, 0, 2, 1, 0])
    assert off.tolist() == [0, 2, 3, 4, 4, 5, 5, 5] and ids.tolist() == [7, 8, 9, 1, 5]
    off, ids = pkg.prep.relevant_lists({k: v[:0] for k, v in held.items()}, [1], [0])
    assert off.tolist() == [0, 0] and len(ids) == 0


def p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


OUTS = ("rel", "hits", "met", "means", "cov", "ev")


def eval_call(L, outs, n_segments=3, width=2, n_rel=6, n_cutoffs=2, **changed):
    """Three rows of two ids, three lists of two; `changed` replaces an array (None: NULL)."""
    a = dict(rec=np.arange(6, dtype=np.int64), cnt=np.array([2, 1, 0], np.int64), off=np.array([0, 2, 4, 6], np.int64),
             ids=np.arange(6, dtype=np.int64), cut=np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], np.int64))
    o = dict(zip(OUTS, outs))
    for k, v in changed.items():
        if k in o:
            o[k] = v
        else:
            a[k] = None if v is None else np.array(v, np.int64)
    return L.lib().locrec_eval_ranked_batch(
        n_segments, width, p(a["rec"]), p(a["cnt"]), p(a["off"]), n_rel, p(a["ids"]), n_cutoffs,
        None if a["cut"] is None else L.ptr(a["cut"], C.c_int64), L.MEM_HOST, p(o["rel"]), p(o["hits"]), p(o["met"]),
        L.ptr(o["means"], C.c_double), L.ptr(o["cov"], C.c_int64), L.ptr(o["ev"], C.c_int64))


def test_evaluator_refusals_need_no_device(pkg):
    from locations_recommender_amd import _lib as L
    outs = (np.full(3, 77, np.int64), np.full(6, 77, np.int64), np.full(30, 7.5), np.full(12, 7.5), np.full(2, 77, np.int64),
            np.full(1, 77, np.int64))

    def refused(word, **kw):
        assert eval_call(L, outs, **kw) == L.E_INVALID_ARG, kw
        assert word in L.lib().locrec_last_error(), (kw, L.lib().locrec_last_error())

    refused(b"n_cutoffs", n_cutoffs=0)
    refused(b"n_cutoffs", n_cutoffs=9)
    refused(b"cutoffs", cut=[3, 0])
    refused(b"cutoffs", cut=[-1, 5])
    refused(b"cutoffs", cut=None)
    refused(b"width", width=-1)
    refused(b"n_segments", n_segments=-1)
    refused(b"n_segments", n_segments=2 ** 31)
    refused(b"n_rel", n_rel=-1)
    refused(b"n_rel", n_rel=2 ** 31)
    refused(b"n_segments x width", n_segments=2 ** 16, width=2 ** 15)
    refused(b"n_segments x width", n_segments=3, width=2 ** 62)
    for bad in BAD_OFFSETS.values():
        refused(b"rel_offsets", off=bad)
    refused(b"rec_counts", cnt=[2, 3, 0])
    refused(b"rec_counts", cnt=[2, -1, 0])
    refused(b"out_means", means=None)
    refused(b"out_coverage", cov=None)
    refused(b"out_evaluated", ev=None)
    refused(b"out_relevant", rel=None)
    refused(b"rec_ids", rec=None)
    refused(b"rel_ids", ids=None)
    for o, fill in zip(outs, (77, 77, 7.5, 7.5, 77, 77)):
        assert (o == fill).all()
    # no segments: zeros, and still no device
    assert eval_call(L, outs, n_segments=0, off=[0]) == L.OK
    assert (outs[3][:12] == 0).all() and (outs[4] == 0).all() and outs[5][0] == 0
    assert pkg.prep.evaluate_ranked_stats() == {"table_entries": 0, "evaluated": 0, "host_syncs": 0, "path": 0}


def split_call(L, n=4, cap=4, **changed):
    a = dict(person=np.arange(4, dtype=np.int64), ts=np.arange(4, dtype=np.int64), place=np.arange(4, dtype=np.int64),
             region=np.zeros(4, np.int64), rows=np.full(4, 77, np.int32), nt=np.full(1, 77, np.int64),
             op=np.full(4, 77, np.int64), org=np.full(4, 77, np.int64), opl=np.full(4, 77, np.int64), nh=np.full(1, cap, np.int64))
    a.update(changed)
    st = L.lib().locrec_holdout_split(n, p(a["person"]), p(a["ts"]), p(a["place"]), p(a["region"]), 2, 1, L.MEM_HOST, p(a["rows"]),
                                      None if a["nt"] is None else L.ptr(a["nt"], C.c_int64), p(a["op"]), p(a["org"]), p(a["opl"]),
                                      None if a["nh"] is None else L.ptr(a["nh"], C.c_int64))
    return st, a


def test_split_refusals_need_no_device(pkg):
    from locations_recommender_amd import _lib as L
    for kw in (dict(n=-1), dict(n=2 ** 31), dict(cap=-1), dict(nt=None), dict(nh=None), dict(person=None), dict(ts=None),
               dict(place=None), dict(region=None)):
        st, a = split_call(L, **kw)
        assert st == L.E_INVALID_ARG, kw
        for k in ("rows", "op", "org", "opl"):
            assert (a[k] == 77).all(), (kw, k)
        assert a["nt"] is None or a["nt"][0] == 77
    st, a = split_call(L, n=0)                     # an empty table: zeros, and no device work
    assert st == L.OK and a["nt"][0] == 0 and a["nh"][0] == 0
