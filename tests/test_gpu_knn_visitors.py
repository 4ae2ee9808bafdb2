"""KNN for visitors (locrec_knn_visitors_*; csrc/knn_visitors.h): rating vectors that are no rows of the index.

Contract: for a visitor v and an index built from the persons P every result equals what the person calls return for v
on an index built from P + {v}, v under an id no person has.  The expected values are the oracle's on that data set
(tests/knn_visitor_cases.py).  Ids, counts and similarity BITS are compared exactly, place ids and row counts exactly,
estimated ratings at 1e-6 relative."""
import numpy as np
import pytest

import knn_visitor_cases as vc
import rank_batch_cases as rb
import rank_exclude_cases as rx

pytestmark = pytest.mark.gpu
RTOL = 1e-6
N = vc.N_ALL - vc.N_VISITORS
NVS = (1, 16, 17, 33)


def make_index(pkg, d):
    return pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"], d["c_val"],
                        d["c_dim"], d.get("r_rowptr"), d.get("r_place"), d.get("r_rating"))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def picks(nv):
    """nv of the forty visitors, one of them listed twice (identical rows)."""
    js = list(range(nv))
    if nv > 1:
        js[-1] = js[0]
    return js


def on_device(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.fixture(scope="module")
def index(pkg):
    d, visitors = vc.base()
    ix = make_index(pkg, d)
    yield ix
    ix.close()


def check_query(ix, arrays, want, k):
    """want[i] = (ids, sims) of visitor i"""
    ids, sims, cnt = ix.visitors_query_batch(*arrays, 0.5, 0.5, k)
    assert ids.shape == (len(want), k)
    for i, (eid, esim) in enumerate(want):
        m = len(eid)
        assert cnt[i] == m, (i, cnt[i], m)
        assert np.array_equal(ids[i, :m], eid), i
        assert np.array_equal(bits(sims[i, :m]), bits(esim)), i
        assert (ids[i, m:] == -1).all() and (sims[i, m:] == 0.0).all()


def check_rows(got, want):
    off, places, est = got
    assert off[0] == 0 and len(off) == len(want) + 1
    for i, (ep, ee) in enumerate(want):
        assert off[i + 1] - off[i] == len(ep), (i, off[i + 1] - off[i], len(ep))
        assert np.array_equal(places[off[i]:off[i + 1]], ep), i
        np.testing.assert_allclose(est[off[i]:off[i + 1]], ee, rtol=RTOL, atol=0)


def expect_stats(pkg, nv, k, n, form, renumbered=1):
    st = pkg.KnnIndex.visitors_stats()
    tiles = (nv + 15) // 16
    assert st["tiles"] == tiles and st["stage_launches"] == 1 and st["scan_launches"] == tiles, st
    if form == "query" or k < n:
        assert st["tiles_topk"] == tiles and st["tiles_all"] == 0, st
    else:
        assert st["tiles_all"] == tiles and st["tiles_topk"] == 0, st
    assert st["renumbered"] == renumbered, st
    return st


def ranked_case(d, rows, nv):
    """rank_batch_cases' case over the row call's rows: the places are the place dimensions, three regions."""
    off, places, est = rows
    place_ids = np.arange(d["p_dim"], dtype=np.int64)
    return dict(offsets=off, ids=places, scores=est, place_ids=place_ids, regions=place_ids % 3,
                targets=(np.arange(nv) % 3).astype(np.int64))


@pytest.mark.parametrize("k", vc.KS)
@pytest.mark.parametrize("nv", NVS)
def test_query_equals_the_index_with_the_visitor(pkg, index, nv, k):
    d, visitors = vc.base()
    js = picks(nv)
    check_query(index, vc.csr([visitors[j] for j in js]), [vc.expected_similar(True, j, k) for j in js], k)
    st = expect_stats(pkg, nv, k, N, "query")
    assert st["beyond"] == 3 * nv                  # two place entries and one category entry a visitor: vector length only


@pytest.mark.parametrize("k", vc.KS)
@pytest.mark.parametrize("nv", NVS)
def test_recommend_and_ranked_equal_the_index_with_the_visitor(pkg, oracle, index, nv, k):
    d, visitors = vc.base()
    js = picks(nv)
    arrays = vc.csr([visitors[j] for j in js])
    rows = index.visitors_recommend_batch(*arrays, 0.5, 0.5, k)
    expect_stats(pkg, nv, k, N, "recommend")
    check_rows(rows, [vc.expected_recommend(True, j, k) for j in js])
    # ranked: against the oracle's ranker over the row call's rows, without and with the visitors' rated places left out
    case = ranked_case(d, rows, nv)
    for limit in (10, 300):
        got = index.visitors_recommend_ranked_batch(*arrays, 0.5, 0.5, k, case["place_ids"], case["regions"], case["targets"], limit)
        expect_stats(pkg, nv, k, N, "ranked")
        width = min(limit, len(case["place_ids"]))
        assert rb.same(got, rx.widened(rb.expected(oracle.rank_recommendations, case, limit), width))
    rated = [visitors[j]["p_idx"][visitors[j]["p_idx"] < d["p_dim"]].astype(np.int64) for j in js]
    for lists in (rated, [np.empty(0, np.int64)] * nv):
        ex = rx.with_lists(case, lists)
        got = index.visitors_recommend_ranked_batch(*arrays, 0.5, 0.5, k, case["place_ids"], case["regions"], case["targets"], 10,
                                                    exclude=(ex["ex_offsets"], ex["ex_ids"]))
        assert rb.same(got, rx.widened(rx.expected(oracle.rank_recommendations, ex, 10), 10))
        for i in range(nv):
            assert not np.isin(got[0][i, :got[2][i]], lists[i]).any()      # no excluded place in any row


@pytest.mark.parametrize("k", (50, N, 2_000_000))
def test_device_tensors_are_read_where_they_lie(pkg, index, k):
    d, visitors = vc.base()
    js = picks(17)
    arrays = on_device(vc.csr([visitors[j] for j in js]))
    check_query(index, arrays, [vc.expected_similar(True, j, k) for j in js], min(k, N + 5))
    check_rows(index.visitors_recommend_batch(*arrays, 0.5, 0.5, k), [vc.expected_recommend(True, j, k) for j in js])
    expect_stats(pkg, 17, k, N, "recommend")


@pytest.mark.parametrize("builder", ("host", "from_device"))
def test_both_other_builders_attach_the_renumbering(pkg, builder, monkeypatch):
    d, visitors = vc.base()
    if builder == "host":
        monkeypatch.setenv("LOCREC_KNN_HOST_BUILD", "1")
        ix = make_index(pkg, d)
    else:
        import torch
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
        ix = pkg.KnnIndex.from_device(t(d["person_ids"], np.int64), t(d["p_rowptr"], np.int64), t(d["p_idx"], np.int32),
                                      t(d["p_val"], np.float64), d["p_dim"], t(d["c_rowptr"], np.int64), t(d["c_idx"], np.int32),
                                      t(d["c_val"], np.float64), d["c_dim"], t(d["r_rowptr"], np.int64), t(d["r_place"], np.int64),
                                      t(d["r_rating"], np.int64))
    js = picks(17)
    arrays = vc.csr([visitors[j] for j in js])
    for k in (1, 1025, N):
        check_query(ix, arrays, [vc.expected_similar(True, j, k) for j in js], k)
        check_rows(ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k), [vc.expected_recommend(True, j, k) for j in js])
        expect_stats(pkg, 17, k, N, "recommend")
    ix.close()


def test_special_visitors(pkg, index):
    d, _ = vc.base()
    allc, nobody, copy = vc.all_categories_visitor(d), vc.nobody_visitor(d), vc.row_of(d, 1500)
    vs = [allc, nobody, copy]
    arrays = vc.csr(vs)
    for k in (N - 1, N, N + 1):
        check_query(index, arrays, [vc.oracle_similar(d, v, 0.5, 0.5, k) for v in vs], k)
        check_rows(index.visitors_recommend_batch(*arrays, 0.5, 0.5, k), [vc.oracle_recommend(d, v, 0.5, 0.5, k) for v in vs])
    ids, sims, cnt = index.visitors_query_batch(*arrays, 0.5, 0.5, N)
    assert cnt.tolist()[:2] == [N, 0] and ids[2, 0] == d["person_ids"][1500]


@pytest.mark.parametrize("n", (1, 255, 256, 257))
def test_row_guard_of_the_scan(pkg, n):
    d, visitors = vc.base()
    small = vc.explicit_ratings(vc.from_rows(d, np.arange(n)))
    ix = make_index(pkg, small)
    vs = visitors[:17]
    arrays = vc.csr(vs)
    for k in (1, n, 2_000_000):
        check_query(ix, arrays, [vc.oracle_similar(small, v, 0.5, 0.5, k) for v in vs], min(k, n + 3))
        check_rows(ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k), [vc.oracle_recommend(small, v, 0.5, 0.5, k) for v in vs])
        expect_stats(pkg, 17, k, n, "recommend", renumbered=pkg.KnnIndex.visitors_stats()["renumbered"])
    ix.close()


@pytest.mark.parametrize("places", (256, 257))
def test_fill_grid_of_long_visitors(pkg, index, places):
    d, _ = vc.base()
    rng = np.random.default_rng(places)
    v = dict(p_idx=np.sort(rng.choice(d["p_dim"], places, replace=False)).astype(np.int32),
             p_val=rng.integers(1, 9, places).astype(np.float64), c_idx=np.array([1, 4], np.int32), c_val=np.array([2.0, 5.0]))
    vs = [vc.row_of(d, 7), v]
    arrays = vc.csr(vs)
    check_query(index, arrays, [vc.oracle_similar(d, x, 0.5, 0.5, 50) for x in vs], 50)
    check_rows(index.visitors_recommend_batch(*arrays, 0.5, 0.5, N), [vc.oracle_recommend(d, x, 0.5, 0.5, N) for x in vs])


@pytest.mark.parametrize("renumbered", (False, True))
def test_bitmap_fold(pkg, renumbered):
    """p_dim = 300,000 > the 2^18 bits of the scan's bitmap: a visitor holding place i and a person holding only
    i + 2^18 share a bit and no place - place similarity 0, as the oracle says.  The bitmap is addressed by STORED
    indices, so the case stands on an index that keeps the caller's numbering (a GENERIC one: non-integer values, the
    stats say "not renumbered"); on the integer index of the same shape the popularity ranks are all small and nothing
    folds - kept as an extra."""
    from locations_recommender_amd import synth
    base = synth.small_knn_dataset(n=500, p_dim=300_000, seed=5, integer=renumbered)
    rows = [vc.row_of(base, r) for r in range(500)]
    fold = 1 << 18
    for j, i in enumerate((10, 77, 30_000)):
        rows[j]["p_idx"], rows[j]["p_val"] = np.array([i + fold], np.int32), np.array([3.0])
    if not renumbered:  # stored indices on both sides of the bitmap's size, and pairs that share a bit
        assert sum(int((r["p_idx"] >= fold).any()) for r in rows) > 3 and sum(int((r["p_idx"] < fold).any()) for r in rows) > 3
    ptrs = vc.csr(rows)
    d = dict(person_ids=base["person_ids"], p_rowptr=ptrs[0], p_idx=ptrs[1], p_val=ptrs[2], p_dim=300_000,
             c_rowptr=ptrs[3], c_idx=ptrs[4], c_val=ptrs[5], c_dim=base["c_dim"])
    d = dict(d, r_rowptr=d["p_rowptr"], r_place=d["p_idx"].astype(np.int64), r_rating=np.floor(d["p_val"]).astype(np.int64))
    ix = make_index(pkg, d)
    assert (ix.info()["mode"] == 0) == (not renumbered)
    # visitor 0 holds i where persons 0 .. 2 hold only i + 2^18 (a shared bit, no shared place); visitor 1 holds 10 + 2^18
    # itself (a match through the folded bit); visitor 2 holds both sides of the fold next to a person's places
    other = vc.row_of(d, 100)
    both_sides = np.unique(np.r_[other["p_idx"] % fold, other["p_idx"] % fold + fold])
    both_sides = both_sides[both_sides < 300_000].astype(np.int32)
    vs = [dict(p_idx=np.array([10, 77, 30_000], np.int32), p_val=np.array([1.0, 2.0, 3.0]), c_idx=np.array([0], np.int32),
               c_val=np.array([1.0])),
          dict(p_idx=np.array([10 + fold], np.int32), p_val=np.array([2.0]), c_idx=np.array([0], np.int32), c_val=np.array([1.0])),
          dict(p_idx=both_sides, p_val=np.arange(1, len(both_sides) + 1, dtype=np.float64), c_idx=np.array([1], np.int32),
               c_val=np.array([2.0]))]
    arrays = vc.csr(vs)
    for k in (50, 500):
        want = [vc.oracle_similar(d, v, 0.5, 0.5, k) for v in vs]
        check_query(ix, arrays, want, k)
        assert pkg.KnnIndex.visitors_stats()["renumbered"] == (1 if renumbered else 0)
        check_rows(ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k), [vc.oracle_recommend(d, v, 0.5, 0.5, k) for v in vs])
    # person 0 holds only 10 + 2^18: no place in common with visitor 0 (its similarity is the category part alone, below
    # visitor 1's, who holds that very place)
    p0 = d["person_ids"][0]
    s0 = dict(zip(*vc.oracle_similar(d, vs[0], 0.5, 0.5, 500))).get(p0, 0.0)
    s1 = dict(zip(*vc.oracle_similar(d, vs[1], 0.5, 0.5, 500)))[p0]
    assert s1 >= 0.5 and abs(s1 - s0 - 0.5) < 1e-12
    ix.close()


def test_generic_index_takes_any_finite_values_and_an_integer_index_refuses_them(pkg, index):
    d, visitors = vc.base(False)
    ix = make_index(pkg, d)
    assert ix.info()["mode"] == 0
    js = picks(17)
    arrays = vc.csr([visitors[j] for j in js])
    for k in (50, 1025, N, 2_000_000):
        check_query(ix, arrays, [vc.expected_similar(False, j, k) for j in js], min(k, N + 1))
        check_rows(ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k), [vc.expected_recommend(False, j, k) for j in js])
        expect_stats(pkg, 17, k, N, "recommend", renumbered=0)
    ix.close()
    # the same visitors on the integer index (renumbered place dimensions): refused, the first of them named
    _, integer_visitors = vc.base()
    mixed = vc.csr([integer_visitors[0], integer_visitors[1], visitors[2], visitors[3]])
    with pytest.raises(pkg.IllegalArgumentException, match="place value of visitor 2 is not an integer count") as e:
        index.visitors_query_batch(*mixed, 0.5, 0.5, 50)
    assert e.value.bad_visitor == 2


def test_wide_rows_as_candidates_and_a_wide_visitor(pkg):
    """Counts >= 256 (tests/test_gpu_row_fallback.py plants them): such rows are scored from the plain CSR, which is all
    the visitor scan reads."""
    from test_gpu_row_fallback import widen
    d, visitors = vc.base()
    wide = widen(widen(d, [3, 777, 2000]), [5, 1234], family="c", big=260)
    wide = vc.explicit_ratings({k: v for k, v in wide.items() if not k.startswith("r_")})
    ix = make_index(pkg, wide)
    v = dict(visitors[4], p_val=visitors[4]["p_val"].copy())
    v["p_val"][0] = 300.0
    vs = visitors[:3] + [v]
    arrays = vc.csr(vs)
    for k in (50, 1025, 2_000_000):
        check_query(ix, arrays, [vc.oracle_similar(wide, x, 0.5, 0.5, k) for x in vs], min(k, N + 1))
        check_rows(ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k), [vc.oracle_recommend(wide, x, 0.5, 0.5, k) for x in vs])
    ix.close()


def refused(pkg, index, visitors, message, bad, k=50, pw=0.5, cw=0.5, patch=None):
    arrays = list(vc.csr(visitors))
    if patch:
        patch(arrays)
    for call in (lambda: index.visitors_query_batch(*arrays, pw, cw, k),
                 lambda: index.visitors_recommend_batch(*arrays, pw, cw, k),
                 lambda: index.visitors_recommend_ranked_batch(*arrays, pw, cw, k, [1, 2], [0, 0], [0] * len(visitors), 5)):
        with pytest.raises(pkg.IllegalArgumentException, match=message) as e:
            call()
        assert e.value.bad_visitor == bad


def test_refusals_name_the_first_offending_visitor(pkg, index):
    d, visitors = vc.base()
    ok = visitors[0]
    def but(**kw):
        return dict(ok, **{k: np.asarray(v, np.int32 if k.endswith("idx") else np.float64) for k, v in kw.items()})
    refused(pkg, index, [ok], "Place weight must be in the interval", -1, pw=0.0, cw=1.0)
    refused(pkg, index, [ok], "Sum of weights must be 1.0", -1, pw=0.5, cw=0.25)
    refused(pkg, index, [ok], "K nearest must be positive", -1, k=0)
    refused(pkg, index, [ok, but(p_idx=[3, 3], p_val=[1, 1])], "place indices of visitor 1 not strictly ascending", 1)
    refused(pkg, index, [ok, ok, but(c_idx=[5, 2], c_val=[1, 1])], "category indices of visitor 2 not strictly ascending", 2)
    refused(pkg, index, [but(p_idx=[-1, 4], p_val=[1, 1]), ok], "place index of visitor 0 is negative", 0)
    refused(pkg, index, [ok, but(p_idx=[4], p_val=[np.inf])], "place value of visitor 1 is not finite", 1)
    refused(pkg, index, [ok, but(c_idx=[4], c_val=[np.nan])], "category value of visitor 1 is not finite", 1)
    refused(pkg, index, [ok, but(p_idx=[4, 9], p_val=[0, 0])], "place vector of visitor 1 has zero norm", 1)
    refused(pkg, index, [ok, but(p_idx=[], p_val=[]), but(c_idx=[], c_val=[])], "No such person: visitor 1 has no place vector", 1)
    refused(pkg, index, [ok, but(c_idx=[], c_val=[])], "No such person: visitor 1 has no category vector", 1)
    refused(pkg, index, [ok, but(p_idx=[4], p_val=[1.5])], "place value of visitor 1 is not an integer count", 1)
    # the first offending visitor wins over a later one, the place family over the category family
    refused(pkg, index, [ok, but(c_idx=[5, 2], c_val=[1, 1], p_idx=[4], p_val=[np.inf]), but(p_idx=[3, 3], p_val=[1, 1])],
            "place value of visitor 1 is not finite", 1)
    long = 1 << 21
    refused(pkg, index, [ok, but(p_idx=np.arange(long), p_val=np.ones(long))], "place vector of visitor 1 has 2\\^21 or more entries", 1)
    def turn_back(arrays):
        arrays[0] = np.array([0, 5, 3, len(arrays[1])], np.int64)
    refused(pkg, index, [ok, ok, ok], "place rowptr not monotone at visitor 1", 1, patch=turn_back)
    # ... and nothing of a refused call is left behind: the next call is right
    check_query(index, vc.csr([ok]), [vc.expected_similar(True, 0, 50)], 50)


def raw_call(pkg, index, form, arrays, nv=None, mem=None, pw=0.5, cw=0.5, k=50, null=(), ranked=None):
    """One visitors call through ctypes -> (status, message, *out_bad_visitor, the outputs).  The outputs start as
    sentinels (-7): a refused call must leave them.  null: positions of the six vector arrays, or output names, passed as
    NULL.  ranked: (place_ids, regions, targets, limit, exclude_offsets, exclude_ids), any of them None = NULL."""
    import ctypes as C
    from locations_recommender_amd import _lib as L
    nv0, ptrs, mem0, keep = pkg.KnnIndex._visitor_args(*arrays)
    nv = nv0 if nv is None else nv
    ptrs = [None if i in null else p for i, p in enumerate(ptrs)]
    rows = max(nv0, 1)
    out = {"ids": np.full((rows, max(k, 1)), -7, np.int64), "sims": np.full((rows, max(k, 1)), -7.0), "counts": np.full(rows, -7, np.int64),
           "offsets": np.full(rows + 1, -7, np.int64), "places": np.full(1 << 16, -7, np.int64), "est": np.full(1 << 16, -7.0)}
    o = lambda name, t: None if name in null else L.ptr(out[name], t)
    bad, cap = C.c_int64(-7), C.c_int64(1 << 16)
    head = (index._h, nv, *ptrs, mem0 if mem is None else mem, pw, cw, k)
    lib = L.lib()
    if form == "query":
        st = lib.locrec_knn_visitors_query_batch(*head, o("ids", C.c_int64), o("sims", C.c_double), o("counts", C.c_int64), C.byref(bad))
    elif form == "recommend":
        st = lib.locrec_knn_visitors_recommend_batch(*head, o("offsets", C.c_int64), o("places", C.c_int64), o("est", C.c_double),
                                                     None if "capacity" in null else C.byref(cap), C.byref(bad))
    else:
        pl, reg, tgt, limit, ex_off, ex_ids = ranked
        a = [None if x is None else L.as_i64(x) for x in (pl, reg, tgt, ex_off, ex_ids)]
        st = lib.locrec_knn_visitors_recommend_ranked_batch(
            *head, 0 if a[0] is None else len(a[0]), L.ptr(a[0], C.c_int64), L.ptr(a[1], C.c_int64), L.ptr(a[2], C.c_int64), limit,
            L.ptr(a[3], C.c_int64), L.ptr(a[4], C.c_int64), o("ids", C.c_int64), o("sims", C.c_double), o("counts", C.c_int64),
            C.byref(bad))
    untouched = all((v == -7).all() for v in out.values()) and cap.value == 1 << 16
    return st, lib.locrec_last_error().decode(), bad.value, untouched


def test_refusals_by_status_message_and_bad_visitor(pkg, index):
    """Every class of refusal through the C ABI itself: the returned status (LOCREC_E_NOT_FOUND is told apart from
    LOCREC_E_INVALID_ARG, which the Python mirror folds into one exception), locrec_last_error, *out_bad_visitor, and
    outputs that nobody wrote."""
    from locations_recommender_amd import _lib as L
    d, visitors = vc.base()
    ok = visitors[0]
    good = vc.csr([ok, visitors[1]])
    places = (np.arange(600), np.arange(600) % 3, [0, 1], 5)

    def expect(got, status, message, bad):
        assert got[0] == status and message in got[1] and got[2] == bad and got[3], (got, status, message, bad)

    for form in ("query", "recommend", "ranked"):
        rk = places + (None, None) if form == "ranked" else None
        # 1. NULL arguments and negative counts: no visitor is at fault
        expect(raw_call(pkg, index, form, good, nv=-1, ranked=rk), L.E_INVALID_ARG, "bad arguments", -1)
        expect(raw_call(pkg, index, form, good, null=(0,), ranked=rk), L.E_INVALID_ARG, "bad arguments", -1)
        expect(raw_call(pkg, index, form, good, null=(3,), ranked=rk), L.E_INVALID_ARG, "bad arguments", -1)
        expect(raw_call(pkg, index, form, good, mem=7, ranked=rk), L.E_INVALID_ARG, "mem must be LOCREC_MEM_HOST or LOCREC_MEM_DEVICE", -1)
        expect(raw_call(pkg, index, form, good, null=(1,), ranked=rk), L.E_INVALID_ARG, "NULL place array", -1)
        expect(raw_call(pkg, index, form, good, null=(5,), ranked=rk), L.E_INVALID_ARG, "NULL category array", -1)
        # 2. the requires
        expect(raw_call(pkg, index, form, good, pw=1.5, cw=-0.5, ranked=rk), L.E_INVALID_ARG, "Place weight must be in the interval", -1)
        expect(raw_call(pkg, index, form, good, k=0, ranked=rk), L.E_INVALID_ARG, "K nearest must be positive", -1)
        # 3. per visitor: an empty vector is "No such person" (NOT_FOUND), everything else a failed require (INVALID_ARG)
        def but(**kw):
            return dict(ok, **{key: np.asarray(v, np.int32 if key.endswith("idx") else np.float64) for key, v in kw.items()})
        per_visitor = (
            (but(p_idx=[], p_val=[]), L.E_NOT_FOUND, "No such person: visitor 1 has no place vector"),
            (but(c_idx=[], c_val=[]), L.E_NOT_FOUND, "No such person: visitor 1 has no category vector"),
            (but(p_idx=[3, 3], p_val=[1, 1]), L.E_INVALID_ARG, "place indices of visitor 1 not strictly ascending"),
            (but(p_idx=[-2], p_val=[1]), L.E_INVALID_ARG, "place index of visitor 1 is negative"),
            (but(c_idx=[2], c_val=[np.inf]), L.E_INVALID_ARG, "category value of visitor 1 is not finite"),
            (but(c_idx=[2], c_val=[0]), L.E_INVALID_ARG, "category vector of visitor 1 has zero norm"),
            (but(p_idx=[4], p_val=[2.5]), L.E_INVALID_ARG, "place value of visitor 1 is not an integer count below 65536"),
            (but(p_idx=[4], p_val=[65536.0]), L.E_INVALID_ARG, "place value of visitor 1 is not an integer count below 65536"),
        )
        for v, status, message in per_visitor:
            rk2 = places[:2] + ([0, 1, 2], 5, None, None) if form == "ranked" else None
            expect(raw_call(pkg, index, form, vc.csr([ok, v, v]), ranked=rk2), status, message, 1)
    expect(raw_call(pkg, index, "query", good, null=("counts",)), L.E_INVALID_ARG, "bad arguments", -1)
    expect(raw_call(pkg, index, "query", good, null=("ids",)), L.E_INVALID_ARG, "bad arguments", -1)
    expect(raw_call(pkg, index, "recommend", good, null=("offsets",)), L.E_INVALID_ARG, "bad arguments", -1)
    expect(raw_call(pkg, index, "recommend", good, null=("capacity",)), L.E_INVALID_ARG, "bad arguments", -1)
    # the ranked form's own arguments and the caller's exclusion lists
    pl, reg, tgt, limit = places
    expect(raw_call(pkg, index, "ranked", good, null=("counts",), ranked=places + (None, None)), L.E_INVALID_ARG, "NULL argument", -1)
    expect(raw_call(pkg, index, "ranked", good, ranked=(pl, reg, None, limit, None, None)), L.E_INVALID_ARG, "NULL argument", -1)
    expect(raw_call(pkg, index, "ranked", good, ranked=(pl, None, tgt, limit, None, None)), L.E_INVALID_ARG, "NULL argument", -1)
    expect(raw_call(pkg, index, "ranked", good, ranked=places + (None, [5, 6])), L.E_INVALID_ARG,
           "exclude_place_ids without exclude_offsets", -1)
    expect(raw_call(pkg, index, "ranked", good, ranked=places + ([0, 2, 1], [5, 6])), L.E_INVALID_ARG,
           "exclude_offsets must be non-decreasing", -1)
    expect(raw_call(pkg, index, "ranked", good, ranked=places + ([-1, 0, 1], [5, 6])), L.E_INVALID_ARG,
           "exclude_offsets must be non-decreasing", -1)
    expect(raw_call(pkg, index, "ranked", good, ranked=places + ([0, 1, 2], None)), L.E_INVALID_ARG, "NULL argument", -1)
    # a good call through the same helper writes its outputs
    st, _, bad, untouched = raw_call(pkg, index, "query", good)
    assert st == L.OK and bad == -1 and not untouched


def test_the_bounds_of_the_integer_refusal(pkg, index):
    """On the renumbered (integer) index a PLACE value must be an integer below 65536; 65535 is served, and so is any
    finite CATEGORY value (the category dimensions are never renumbered) - both bit-exact against the oracle."""
    d, visitors = vc.base()
    big = dict(visitors[0], p_val=visitors[0]["p_val"].copy())
    big["p_val"][1] = 65535.0
    frac = dict(visitors[1], c_val=visitors[1]["c_val"] * 0.37 + 0.011)
    vs = [big, frac]
    arrays = vc.csr(vs)
    for k in (50, N):
        check_query(index, arrays, [vc.oracle_similar(d, v, 0.5, 0.5, k) for v in vs], k)
        assert pkg.KnnIndex.visitors_stats()["renumbered"] == 1
        check_rows(index.visitors_recommend_batch(*arrays, 0.5, 0.5, k), [vc.oracle_recommend(d, v, 0.5, 0.5, k) for v in vs])


def test_device_row_pointers_are_checked_by_the_stage(pkg, index):
    """Device arrays: the host never sees the row pointers' middle, the stage kernel refuses a row that turns back or
    ends beyond the arrays before anything is read through it."""
    d, visitors = vc.base()
    arrays = list(vc.csr(visitors[:3]))
    total = len(arrays[1])
    for ptr, who in (([0, 5, 3, total], 1), ([0, total + 100, total + 200, total], 0), ([0, 5, -4, total], 1)):
        bad_ptr = list(arrays)
        bad_ptr[0] = np.array(ptr, np.int64)
        dev = on_device(bad_ptr)
        for call in (lambda: index.visitors_query_batch(*dev, 0.5, 0.5, 50), lambda: index.visitors_recommend_batch(*dev, 0.5, 0.5, 50)):
            with pytest.raises(pkg.IllegalArgumentException, match=f"place rowptr not monotone at visitor {who}") as e:
                call()
            assert e.value.bad_visitor == who
    check_query(index, on_device(arrays), [vc.expected_similar(True, j, 50) for j in range(3)], 50)


def test_no_visitors(pkg, index):
    empty = vc.csr([])
    ids, sims, cnt = index.visitors_query_batch(*empty, 0.5, 0.5, 50)
    assert ids.shape == (0, 50) and len(cnt) == 0
    off, places, est = index.visitors_recommend_batch(*empty, 0.5, 0.5, 50)
    assert off.tolist() == [0] and len(places) == 0
    oi, osc, oc = index.visitors_recommend_ranked_batch(*empty, 0.5, 0.5, 50, [1, 2], [0, 0], [], 5)
    assert oi.shape == (0, 2) and len(oc) == 0
    assert pkg.KnnIndex.visitors_stats()["tiles"] == 0


def test_the_handle_afterwards(pkg):
    from locations_recommender_amd import _lib as L
    d, visitors = vc.base()
    before_create = L.device_bytes_in_use()
    ix = make_index(pkg, d)
    persons = d["person_ids"][:40]
    arrays = vc.csr(visitors[:17])
    for k in (50, 1025, 2_000_000):
        want = ix.recommend_batch(persons, 0.5, 0.5, k)
        want_q = ix.query_batch(persons, 0.5, 0.5, min(k, 2000))
        for call in (lambda: ix.visitors_query_batch(*arrays, 0.5, 0.5, min(k, 3000)),
                     lambda: ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k),
                     lambda: ix.visitors_recommend_ranked_batch(*arrays, 0.5, 0.5, k, np.arange(600), np.zeros(600), np.zeros(17), 5)):
            ix.recommend_batch(persons[:17], 0.5, 0.5, k)       # something resident of the same size ...
            call()
            for stray in (lambda: ix.fetch_recommend(17), lambda: ix.fetch_topk(17, min(k, 3000))):   # ... is no visitor's
                with pytest.raises(pkg.IllegalArgumentException):
                    stray()
            got = ix.recommend_batch(persons, 0.5, 0.5, k)
            assert all(np.array_equal(a, b) for a, b in zip((got[0], got[1], bits(got[2])), (want[0], want[1], bits(want[2]))))
            got_q = ix.query_batch(persons, 0.5, 0.5, min(k, 2000))
            assert np.array_equal(got_q[0], want_q[0]) and np.array_equal(bits(got_q[1]), bits(want_q[1]))
    ix.close()
    assert L.device_bytes_in_use() == before_create


def test_recommender_methods_for_a_visitor(pkg):
    """KnnRecommender.findSimilarPersonsForVisitor / makeRecommendationsForVisitor: the person forms' frames."""
    from test_handle_cache import knn_frames
    d, visitors = vc.base()
    small = vc.explicit_ratings(vc.from_rows(d, np.arange(400)))
    v = visitors[3]
    place = pkg.SparseVector(small["p_dim"] + 2000, v["p_idx"], v["p_val"])
    category = pkg.SparseVector(small["c_dim"] + 100, v["c_idx"], v["c_val"])
    for k in (7, 2_000_000):
        rec = pkg.KnnRecommender(*knn_frames(pkg, small), 0.25, 0.75, k)
        near = rec.findSimilarPersonsForVisitor(place, category)
        eid, esim = vc.oracle_similar(small, v, 0.25, 0.75, k)
        assert list(near.columns) == ["person_id", "similarity"]
        assert np.array_equal(near["person_id"].to_numpy(), eid) and np.array_equal(bits(near["similarity"].to_numpy()), bits(esim))
        rows = rec.makeRecommendationsForVisitor(place, category)
        ep, ee = vc.oracle_recommend(small, v, 0.25, 0.75, k)
        assert list(rows.columns) == ["place_id", "estimated_rating"] and np.array_equal(rows["place_id"].to_numpy(), ep)
        np.testing.assert_allclose(rows["estimated_rating"].to_numpy(), ee, rtol=RTOL, atol=0)
        rec.close()
    pkg.lib().locrec_cache_clear()
