"""KNN for visitors (csrc/knn_visitors.h, knn_visitors_api.h, knn_visitors_plan.h, knn_visitors_side.h) AT the limits of its
stage, tiles and chunks: the cases of tests/knn_visitor_limit_cases.py (checked on the CPU by
test_knn_visitor_limit_cases.py).  Expected results are the oracle's on P + {v} (tests/knn_visitor_cases.py) with the
tolerances of test_gpu_knn_visitors.py: ids, counts, similarity bits, place ids and row counts exact, ratings at 1e-6
relative; refusals by status, message and *out_bad_visitor through the C ABI; stats against the model.  Each
test's docstring names one-line changes of the sources that it is built to catch ("Bites"); those marked (tried) were
made in an uncommitted build and failed the test on an MI355X, a change that would read or write out of bounds on the
device is marked "not tried", the rest follow from reading the sources.

Every refusal provoked here is made by the host, or by lkv_stage from the row pointers and the entries it may read,
BEFORE anything is read through the offending input."""
import contextlib
import ctypes as C
import os
import time

import numpy as np
import pytest

import knn_visitor_cases as vc
import knn_visitor_limit_cases as lim
import rank_batch_cases as rb
import rank_exclude_cases as rx
from test_gpu_knn_visitors import bits, check_query, check_rows, make_index, on_device, ranked_case, raw_call

pytestmark = pytest.mark.gpu
MEMS = ("host", "device")
SWITCH = "LOCREC_KNN_VISITORS_CHUNK_BYTES"


@contextlib.contextmanager
def switch(name, value):
    """An environment switch the library reads at every call."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def placed(arrays, mem):
    return on_device(arrays) if mem == "device" else arrays


def expect_stats(pkg, want, **more):
    st = pkg.KnnIndex.visitors_stats()
    for key, value in dict(want, **more).items():
        assert st[key] == value, (key, st, want)
    return st


def wrapper_stats(nv, k, n, places, device, rows):
    """call_stats of a recommend call through the Python wrapper: its LAST call always has room for the rows (a result
    beyond the first attempt's 65,536 rows is computed again with room for all of them)."""
    return lim.call_stats("recommend", nv, k, n, places, device, rows=rows, room=max(rows, lim.PYTHON_ROOM))


def expect_refusal(got, status, text, bad):
    assert got[0] == status and text in got[1] and got[2] == bad and got[3], (got, status, text, bad)


def status_of(code):
    from locations_recommender_amd import _lib as L
    return L.E_NOT_FOUND if code in lim.NOT_FOUND else L.E_INVALID_ARG


def raw_recommend(pkg, index, arrays, k, capacity, null_places=False):
    """locrec_knn_visitors_recommend_batch with outputs of `capacity` + 2 rows filled with -7
    -> (status, message, *inout_capacity, *out_bad_visitor, offsets, places, ratings)"""
    from locations_recommender_amd import _lib as L
    nv, ptrs, mem, keep = pkg.KnnIndex._visitor_args(*arrays)
    off, places, est = np.full(nv + 1, -7, np.int64), np.full(capacity + 2, -7, np.int64), np.full(capacity + 2, -7.0)
    bad, cap = C.c_int64(-7), C.c_int64(capacity)
    st = L.lib().locrec_knn_visitors_recommend_batch(index._h, nv, *ptrs, mem, 0.5, 0.5, k, L.ptr(off, C.c_int64),
                                                     None if null_places else L.ptr(places, C.c_int64), L.ptr(est, C.c_double),
                                                     C.byref(cap), C.byref(bad))
    return st, L.lib().locrec_last_error().decode(), cap.value, bad.value, off, places, est


_ORACLE = {}


def want_similar(name, d, v, k):
    """The oracle's list for the visitor `name` of the data `d` (by identity of the cached data), computed once."""
    key = ("s", id(d), name, k)
    if key not in _ORACLE:
        _ORACLE[key] = vc.oracle_similar(d, v, 0.5, 0.5, k)
    return _ORACLE[key]


def want_rows(name, d, v, k):
    key = ("r", id(d), name, k)
    if key not in _ORACLE:
        _ORACLE[key] = vc.oracle_recommend(d, v, 0.5, 0.5, k)
    return _ORACLE[key]


@pytest.fixture(scope="module")
def index300(pkg):
    d = lim.small_index(300)
    ix = make_index(pkg, d)
    yield d, ix
    ix.close()


@pytest.fixture(scope="module")
def index40(pkg):
    d = lim.small_index(lim.STAGE_N)
    ix = make_index(pkg, d)
    yield d, ix
    ix.close()


# ---- a. the stage's blocks --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("nv", lim.STAGE_NVS)
def test_stage_blocks_serve_every_visitor(pkg, index40, nv, mem):
    """Bites: `k > n` in knn_visitors_all (tried: the stats at K = n say tiles_topk); `v > a.nv` in lkv_stage's guard
    (thread nv reads row pointers behind the array; not tried, it reads out of bounds); a grid of `nv / 256` blocks (the visitors of the last block are never staged: at 257 the last one has no
    bounds, at 255 nobody has); `threadIdx.x` alone as the visitor (256 is staged over 0)."""
    d, ix = index40
    n = lim.STAGE_N
    batch, which = lim.stage_batch(nv)
    arrays = placed(vc.csr(batch), mem)
    for k in (5, n + 5):
        check_query(ix, arrays, [want_similar(int(j), d, batch[i], k) for i, j in enumerate(which)], k)
        expect_stats(pkg, lim.call_stats("query", nv, k, n, lim.rated_places(d), mem == "device"), beyond=3 * nv)
    for k in (5, n):
        rows = ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k)
        check_rows(rows, [want_rows(int(j), d, batch[i], k) for i, j in enumerate(which)])
        expect_stats(pkg, wrapper_stats(nv, k, n, lim.rated_places(d), mem == "device", len(rows[1])), beyond=3 * nv)


@pytest.mark.parametrize("mem", MEMS)
def test_offenders_either_side_of_the_block_seam(pkg, index40, mem):
    """Bites: `atomicMin` read as `atomicMax` (tried), or a plain store, on the report word (256 and 300 together: 300 wins; the
    category offender at 255 loses to the place offender at 256); `f << 4` dropped from the word (both families at 256:
    the smaller CODE wins, the category's); `(report[0] >> 8)` read as `>> 4`."""
    d, ix = index40
    ok_batch = lim.offender_batch({})
    for label, planted in lim.offenders():
        batch = lim.offender_batch(planted)
        who, fam, code = lim.first_refusal(batch, d["p_dim"], d["c_dim"], True)
        arrays = placed(vc.csr(batch), mem)
        for form in ("query", "recommend"):
            expect_refusal(raw_call(pkg, ix, form, arrays, k=5), status_of(code), lim.message(code, fam, who), who)
    # and nothing is left behind: the same batch without offenders is served
    arrays = placed(vc.csr(ok_batch[:20]), mem)
    _, which = lim.stage_batch(257)
    check_query(ix, arrays, [want_similar(int(which[i % 257]), d, ok_batch[i], 5) for i in range(20)], 5)


# ---- b. the length limit ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ("p", "c"))
def test_vectors_of_two_to_the_twenty_one_minus_one_entries(pkg, index300, family):
    """Bites: `>= (1 << 21)` read as `> (1 << 21)` (tried: 2^21 entries are served) or as `>= (1 << 21) - 1` (the served
    length is refused); `b + kept` read as `i` for the staged position (the squeeze: with 2,096,551 entries beyond the dimensions nothing moves either way here, but
    `bounds[2v + 1] = e` instead of `b + kept` makes the fill read two million entries, the unstaged ones as zeros:
    not tried); `longest` of knn_visitors_fill_blocks taken over slot 0 only (the long visitor's 600 kept places need 3
    blocks: as the last slot of a full tile it would be cut to the first slot's 256)."""
    d, ix = index300
    n = 300
    _, visitors = vc.base()
    long_one = lim.long_visitor(family)
    short = [vc.without_beyond(visitors[j], d["p_dim"], d["c_dim"]) for j in range(3, 18)]
    assert max(len(v["p_idx"]) for v in short) < 256
    w = {k: (want_similar("long " + family, d, long_one, k), want_rows("long " + family, d, long_one, k)) for k in (50, n)}
    ws = {k: [(want_similar(("short", j), d, v, k), want_rows(("short", j), d, v, k)) for j, v in enumerate(short)] for k in (50, n)}
    beyond_long = 2 ** 21 - 1 - (d["p_dim"] if family == "p" else d["c_dim"])
    # in a tile after a short visitor, and as the last slot of a full tile of 16
    for vs, idx in (([short[0], long_one], [0]), (short + [long_one], list(range(15)))):
        arrays = vc.csr(vs)
        k = 50
        check_query(ix, arrays, [ws[k][j][0] for j in idx] + [w[k][0]], k)
        expect_stats(pkg, lim.call_stats("query", len(vs), k, n, lim.rated_places(d), False), beyond=beyond_long, renumbered=1)
        assert lim.beyond_total(vs, d["p_dim"], d["c_dim"]) == beyond_long
    arrays = on_device(vc.csr([short[0], long_one]))
    check_rows(ix.visitors_recommend_batch(*arrays, 0.5, 0.5, n), [ws[n][0][1], w[n][1]])
    expect_stats(pkg, {}, beyond=beyond_long)
    # one entry more is refused, in either family, before the vector is walked
    from locations_recommender_amd import _lib as L
    too_long = lim.long_visitor(family, lim.LONG)
    for form in ("query", "recommend"):
        expect_refusal(raw_call(pkg, ix, form, vc.csr([short[0], too_long]), k=5), L.E_INVALID_ARG,
                       lim.message(lim.TOO_LONG, 0 if family == "p" else 1, 1), 1)


def test_a_tile_without_a_place_inside_the_dimensions(pkg, index300):
    """Bites: `int32_t longest = 1` read as `= 0` in knn_visitors_fill_blocks (a grid of zero blocks: the launch fails and
    the call with it); a fill that sets the bit of a squeezed entry.  Every slot's kept place vector is empty: the place
    similarity is 0 and the list is the categories' alone; a visitor WITH places in the tile behind it sees clean tables."""
    d, ix = index300
    _, visitors = vc.base()
    nowhere = [lim.nowhere_visitor(j) for j in range(16)]
    vs = nowhere + [visitors[20]]
    arrays = vc.csr(vs)
    for k in (50, 300):
        want = [want_similar(("nowhere", j), d, v, k) for j, v in enumerate(nowhere)] + [want_similar(20, d, visitors[20], k)]
        check_query(ix, arrays, want, k)
        expect_stats(pkg, lim.call_stats("query", 17, k, 300, lim.rated_places(d), False),
                     beyond=lim.beyond_total(vs, d["p_dim"], d["c_dim"]))
        # the categories alone: the list, bit for bit, of the same visitor with ANOTHER place nobody holds
        other = dict(nowhere[3], p_idx=np.array([d["p_dim"] + 50], np.int32), p_val=np.array([7.0]))
        assert all(np.array_equal(x, y) for x, y in zip(want[3], want_similar("nowhere other", d, other, k)))
    check_rows(ix.visitors_recommend_batch(*arrays, 0.5, 0.5, 300),
               [want_rows(("nowhere", j), d, v, 300) for j, v in enumerate(nowhere)] + [want_rows(20, d, visitors[20], 300)])


# ---- c. value bounds ------------------------------------------------------------------------------------------------------------

def test_place_values_at_the_integer_bound(pkg, index300):
    """Bites: `fabs(x) < 65536.0` read as `<= 65536.0` (tried: 65536 is served) or `x < 65536.0` (-65536 is served); `x != floor(x)`
    read as `x != trunc(x)` makes no difference, `x >= 1` added (the integral flag of create) refuses -1, 0 and -0.0."""
    from locations_recommender_amd import _lib as L
    d, ix = index300
    served, refused = lim.value_cases(d)
    vs = list(served.values())
    arrays = vc.csr(vs)
    for k in (50, 300):
        check_query(ix, arrays, [want_similar(("served", name), d, v, k) for name, v in served.items()], k)
        expect_stats(pkg, {}, renumbered=1, beyond=0)
        check_rows(ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k), [want_rows(("served", name), d, v, k) for name, v in served.items()])
    for name, v in refused.items():
        for form in ("query", "recommend"):
            expect_refusal(raw_call(pkg, ix, form, vc.csr([vs[0], v])), L.E_INVALID_ARG, lim.message(lim.FRACTION, 0, 1), 1)
    # parity with create (documented difference: the integer rule exists only where the index renumbers): every vector
    # of both tables is a legal ROW - P + {v} is built, in the generic form where v is no integer count >= 1
    for name, v in list(served.items()) + list(refused.items()):
        plus = make_index(pkg, vc.index_plus_visitor(d, v))
        integral = bool((v["p_val"] >= 1).all() and (v["p_val"] == np.floor(v["p_val"])).all())
        assert integral or plus.info()["mode"] == 0, name
        plus.close()


def test_values_whose_squares_leave_fp64_on_a_generic_index(pkg):
    """Bites: `!(sum > 0)` read as `sum == 0` makes no difference for these; `isfinite(x)` read as `isfinite(x * x)` refuses
    1e160, which create takes; the zero-norm test dropped serves 1e-170 with a norm of 0 (a division by zero per
    candidate).  Parity: create on P + {v} is refused exactly when the stage refuses v."""
    from locations_recommender_amd import _lib as L
    d = lim.small_index(300, False)
    ix = make_index(pkg, d)
    assert ix.info()["mode"] == 0
    cases = lim.generic_value_cases(d)
    ok = vc.without_beyond(vc.base(False)[1][3], d["p_dim"], d["c_dim"])
    for name, (v, code) in cases.items():
        if code == 0:
            for k in (50, 300):
                check_query(ix, vc.csr([ok, v]), [want_similar(("generic", "ok"), d, ok, k), want_similar(("generic", name), d, v, k)], k)
                expect_stats(pkg, {}, renumbered=0)
                check_rows(ix.visitors_recommend_batch(*vc.csr([v]), 0.5, 0.5, k), [want_rows(("generic", name), d, v, k)])
        else:
            fam = 1 if "category" in name else 0
            for form in ("query", "recommend"):
                expect_refusal(raw_call(pkg, ix, form, vc.csr([ok, v])), status_of(code), lim.message(code, fam, 1), 1)
        try:
            make_index(pkg, vc.index_plus_visitor(d, v)).close()
            created = True
        except pkg.IllegalArgumentException as e:
            created = False
            assert "zero norm" in str(e), name
        assert created == (code == 0), name
    ix.close()


# ---- d. chunks ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("nv", lim.CHUNK_NVS)
def test_chunks_of_neighbour_lists(pkg, index300, nv, mem):
    """Bites: `side.norm_p.p + v0` without `+ v0` in lkv_scan_tile (tried: every tile behind the first divides by the first
    tile's vector lengths, in the row calls too); `out_ids + v0 * k` read as `out_ids + v0` (tried: chunks overwrite each other); `knn_visitors_stage_row(v0 + t)`
    read as `(t)` (every chunk serves the first chunk's visitors); `out_counts + v0` without `+ v0`; `v0 += chunk` read as
    `v0 += kLkbQt` at a chunk of 32."""
    d, ix = index300
    n = lim.CHUNK_N
    vs = lim.distinct_visitors()[:nv]
    arrays = placed(vc.csr(vs), mem)
    device = mem == "device"
    for k in lim.CHUNK_KS:
        kk = lim.clipped(k, n)
        whole = ix.visitors_query_batch(*arrays, 0.5, 0.5, kk)
        expect_stats(pkg, lim.call_stats("query", nv, kk, n, lim.rated_places(d), device), beyond=3 * nv)
        if kk >= 50:   # pairwise different results: a row shifted by a chunk or by a tile cannot pass
            assert len({whole[1][i].tobytes() for i in range(nv)}) == nv
        for i in sorted({0, 4, 5, 15, 16, 31, 32, nv - 1} & set(range(nv))):
            eid, esim = want_similar(("distinct", i), d, vs[i], kk)
            m = len(eid)
            assert whole[2][i] == m and np.array_equal(whole[0][i, :m], eid) and np.array_equal(bits(whole[1][i, :m]), bits(esim)), (k, i)
        for size in lim.CHUNK_SIZES:
            budget = lim.budget_for(size, kk)
            with switch(SWITCH, str(budget)):
                got = ix.visitors_query_batch(*arrays, 0.5, 0.5, kk)
                st = expect_stats(pkg, lim.call_stats("query", nv, kk, n, lim.rated_places(d), device, budget), beyond=3 * nv)
            assert st["tiles"] == sum((cn + 15) // 16 for _, cn in lim.chunks_of(nv, kk, budget))
            assert np.array_equal(got[0], whole[0]) and np.array_equal(bits(got[1]), bits(whole[1])) and np.array_equal(got[2], whole[2]), \
                (k, size, np.flatnonzero((got[0] != whole[0]).any(axis=1))[:5])
    # the switch's clamps: a budget below one list still serves one visitor a chunk; no number is the default
    with switch(SWITCH, "1"):
        got = ix.visitors_query_batch(*arrays, 0.5, 0.5, 50)
        expect_stats(pkg, {}, tiles=nv, host_syncs=(2 if device else 1) + 2 * nv)
    with switch(SWITCH, "many"):
        again = ix.visitors_query_batch(*arrays, 0.5, 0.5, 50)
        expect_stats(pkg, lim.call_stats("query", nv, 50, n, lim.rated_places(d), device))
    assert np.array_equal(got[0], again[0]) and np.array_equal(bits(got[1]), bits(again[1]))


# ---- e. capacity ----------------------------------------------------------------------------------------------------------------

def test_more_rows_than_the_first_attempt_holds(pkg):
    """Bites: `total > cap` read as `total >= cap` (tried: capacity = total is not served) or the test dropped (the copy runs past
    the caller's arrays: not tried); `*inout_capacity = total` moved behind the return; in the Python wrapper `cap.value <=
    len(places)` read as `<` (never ends in two calls: the rows are the first attempt's garbage)."""
    from locations_recommender_amd import _lib as L
    d = lim.small_index(300)
    ix = make_index(pkg, d)
    n = 300
    vs = [lim.everybody_visitor(d, j) for j in range(lim.CAPACITY_NV)]
    arrays = vc.csr(vs)
    want = [want_rows(("everybody", j % 6), d, v, n) for j, v in enumerate(vs)]
    total = sum(len(w[0]) for w in want)
    assert total > lim.PYTHON_ROOM and not hasattr(ix, "_visitor_room")
    rows = ix.visitors_recommend_batch(*arrays, 0.5, 0.5, n)
    assert len(rows[1]) == total == rows[0][-1] and ix._visitor_room == total        # the second call was made
    check_rows(rows, want)
    expect_stats(pkg, wrapper_stats(lim.CAPACITY_NV, n, n, lim.rated_places(d), False, total))
    # the C ABI
    st, msg, cap, bad, off, places, est = raw_recommend(pkg, ix, arrays, n, total - 1)
    assert st == L.OK and cap == total and bad == -1 and np.array_equal(off, rows[0])
    assert (places == -7).all() and (est == -7.0).all()                                # sized, not written
    expect_stats(pkg, lim.call_stats("recommend", lim.CAPACITY_NV, n, n, lim.rated_places(d), False, rows=total, room=total - 1))
    st, msg, cap, bad, off, places, est = raw_recommend(pkg, ix, arrays, n, total)
    assert st == L.OK and cap == total and np.array_equal(off, rows[0])
    assert np.array_equal(places[:total], rows[1]) and np.array_equal(bits(est[:total]), bits(rows[2]))
    assert (places[total:] == -7).all() and (est[total:] == -7.0).all()
    st, msg, cap, bad, off, places, est = raw_recommend(pkg, ix, arrays, n, total, null_places=True)
    assert st == L.E_INVALID_ARG and "NULL output buffer" in msg and bad == -1 and (est == -7.0).all()
    ix.close()


# ---- f. the row refusal -------------------------------------------------------------------------------------------------------

def test_row_refusal_at_three_times_two_to_the_thirty(pkg):
    """Bites: `worst > kVisitorsMaxRowBytes` read as `>=` (tried: the served side is refused); `nv * max(1, n_places) * 16` taken in
    int32; the refusal moved behind knn_visitors_recommend (it would run before it is refused: the time shows it)."""
    from locations_recommender_amd import _lib as L
    d = lim.row_refusal_index()
    ix = make_index(pkg, d)
    served = lim.nobody_batch(d, lim.ROW_NV)
    t0 = time.perf_counter()
    off, places, est = ix.visitors_recommend_batch(*served, 0.5, 0.5, 2_000_000)
    print("served side of the row refusal: %.2f s for %d visitors x %d rated places" % (time.perf_counter() - t0, lim.ROW_NV, lim.ROW_PLACES))
    assert len(off) == lim.ROW_NV + 1 and not off.any() and len(places) == 0
    expect_stats(pkg, lim.call_stats("recommend", lim.ROW_NV, 2_000_000, 4, lim.ROW_PLACES, False, rows=0), beyond=2 * lim.ROW_NV)
    refused = lim.nobody_batch(d, lim.ROW_NV + 1)
    st, msg, cap, bad, off, places, est = raw_recommend(pkg, ix, refused, 2_000_000, 64)
    assert st == L.E_INVALID_ARG and "split it" in msg and "%d visitors" % (lim.ROW_NV + 1) in msg and bad == -1 and cap == 64
    assert (off == -7).all() and (places == -7).all() and (est == -7.0).all()
    with pytest.raises(pkg.IllegalArgumentException, match="split it") as e:
        ix.visitors_recommend_ranked_batch(*refused, 0.5, 0.5, 50, [7, 10], [0, 0], np.zeros(lim.ROW_NV + 1, np.int64), 2)
    assert e.value.bad_visitor == -1
    # the neighbour lists have no such limit
    ids, sims, cnt = ix.visitors_query_batch(*refused, 0.5, 0.5, 2)
    assert not cnt.any() and (ids == -1).all()
    ix.close()


# ---- g. index edges -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ("no persons", "one person", "no ratings"))
def test_index_edges(pkg, oracle, which):
    """Bites: `k > n` in knn_visitors_all (tried: one person at K = 1); `if (ix->n == 0)` dropped from an entry point (a scan of zero rows: a grid of zero blocks fails the call);
    `std::fill(out_ids, out_ids + nv * k, -1)` read as `+ nv`; `tiles = max(1, ...)` without the max on an index without
    ratings (arrays of size 0); `if (np > 0) ++st.host_syncs` counting a wait that is not made."""
    d = {"no persons": lim.empty_index, "one person": lambda: lim.small_index(1),
         "no ratings": lambda: lim.without_ratings(lim.small_index(lim.STAGE_N))}[which]()
    ix = make_index(pkg, d)
    n = len(d["person_ids"])
    _, visitors = vc.base()
    vs = visitors[:17]
    places = lim.rated_places(d) if n else 0
    for mem in MEMS:
        arrays = placed(vc.csr(vs), mem)
        for k in (1, 2_000_000):
            kk = lim.clipped(k, n)
            if n == 0:
                ids, sims, cnt = ix.visitors_query_batch(*arrays, 0.5, 0.5, kk)
                assert ids.shape == (17, kk) and (ids == -1).all() and (sims == 0.0).all() and not cnt.any()
            else:
                check_query(ix, arrays, [want_similar((which, j), d, v, kk) for j, v in enumerate(vs)], kk)
            st = expect_stats(pkg, lim.call_stats("query", 17, kk, n, places, mem == "device"), beyond=3 * 17)
            assert n > 0 or st["renumbered"] == 0                    # (an index without persons renumbers nothing)
            rows = ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k)
            if n == 0 or which == "no ratings":
                assert len(rows[0]) == 18 and not rows[0].any() and len(rows[1]) == 0 and len(rows[2]) == 0
            else:
                check_rows(rows, [want_rows((which, j), d, v, k) for j, v in enumerate(vs)])
            expect_stats(pkg, wrapper_stats(17, k, n, places, mem == "device", len(rows[1])), beyond=3 * 17)
            case = ranked_case(d, rows, 17)
            got = ix.visitors_recommend_ranked_batch(*arrays, 0.5, 0.5, k, case["place_ids"], case["regions"], case["targets"], 10)
            if len(rows[1]) == 0:
                assert got[0].shape == (17, 10) and (got[0] == -1).all() and (got[1] == 0.0).all() and not got[2].any()
            else:
                assert rb.same(got, rx.widened(rb.expected(oracle.rank_recommendations, case, 10), 10))
            expect_stats(pkg, {}, tiles=2 if n else 0, stage_launches=1, beyond=3 * 17)
    # a person call on the same handle afterwards
    if n == 0:
        with pytest.raises(pkg.IllegalArgumentException):
            ix.query(1000, 0.5, 0.5, 5)
    else:
        pid = int(d["person_ids"][0])
        gi, gs = ix.query(pid, 0.5, 0.5, 5)
        oi, osim = oracle.knn_similar(d, pid, 0.5, 0.5, 5)
        assert np.array_equal(gi, oi) and np.array_equal(bits(gs), bits(osim))
    ix.close()


# ---- h. arguments -------------------------------------------------------------------------------------------------------------

def test_argument_refusals_of_the_stage(pkg, index300):
    """Bites: `in_ptr[f][0] != 0` dropped on the host (rows shifted by one entry are served) or `ends[2 * f] != 0` on the
    device; `total[f] >= 2^31` dropped (the sizes of the copies wrap: not tried beyond the refusal itself, which is made
    before anything is copied); lkv_device_array dropped (a host pointer given to a kernel: not tried, it faults);
    `kVisErrEmpty` mapped to INVALID_ARG (tried)."""
    import torch
    from locations_recommender_amd import _lib as L
    d, ix = index300
    _, visitors = vc.base()
    good = [visitors[0], visitors[1]]
    arrays = list(vc.csr(good))

    def good_call_is_right():
        check_query(ix, vc.csr(good), [want_similar(0, d, good[0], 50), want_similar(1, d, good[1], 50)], 50)

    for fam, at in (("place", 0), ("category", 3)):
        shifted = list(arrays)
        shifted[at] = arrays[at] + (arrays[at] < arrays[at][-1])        # starts at 1, ends where it ended: still monotone
        assert shifted[at][0] == 1 and shifted[at][-1] == arrays[at][-1]
        for mem in MEMS:
            for form in ("query", "recommend"):
                expect_refusal(raw_call(pkg, ix, form, placed(shifted, mem)), L.E_INVALID_ARG, fam + " rowptr must start at 0", -1)
            good_call_is_right()
    # 2^31 entries claimed by the row pointers of one-element arrays: refused from the pointers alone, before any copy
    # (knn_visitors_stage: the range test of total[] stands before the first hipMemcpyAsync of an element array)
    one = vc.csr([dict(p_idx=np.array([3], np.int32), p_val=np.array([1.0]), c_idx=np.array([1], np.int32), c_val=np.array([1.0]))])
    for fam, at in (("place", 0), ("category", 3)):
        huge = list(one)
        huge[at] = np.array([0, 2 ** 31], np.int64)
        for form in ("query", "recommend"):
            expect_refusal(raw_call(pkg, ix, form, huge), L.E_INVALID_ARG, fam + " element count out of range [0, 2^31)", -1)
        good_call_is_right()
    # host arrays announced as device arrays: refused by the pointer's attributes, nothing is read through them
    st, msg, bad, untouched = raw_call(pkg, ix, "query", arrays, mem=L.MEM_DEVICE)
    assert st == L.E_INVALID_ARG and bad == -1 and untouched
    assert "is not a device array" in msg or "does not live on the index's device" in msg, msg
    assert msg.startswith("place rowptr")
    good_call_is_right()
    # device row pointers with host element arrays
    mixed = pkg.KnnIndex._visitor_args(*arrays)
    dev = on_device(arrays)
    ptrs = [C.c_void_p(dev[i].data_ptr()) if i in (0, 3) else mixed[1][i] for i in range(6)]
    out = np.full((2, 5), -7, np.int64), np.full((2, 5), -7.0), np.full(2, -7, np.int64)
    bad = C.c_int64(-7)
    torch.cuda.synchronize()
    st = L.lib().locrec_knn_visitors_query_batch(ix._h, 2, *ptrs, L.MEM_DEVICE, 0.5, 0.5, 5, L.ptr(out[0], C.c_int64),
                                                 L.ptr(out[1], C.c_double), L.ptr(out[2], C.c_int64), C.byref(bad))
    msg = L.lib().locrec_last_error().decode()
    assert st == L.E_INVALID_ARG and msg.startswith("place indices") and bad.value == -1 and (out[0] == -7).all(), msg
    good_call_is_right()
    # three visitors without any entry, the element arrays NULL: "No such person", the first of them
    nothing = vc.csr([dict(p_idx=np.zeros(0, np.int32), p_val=np.zeros(0), c_idx=np.zeros(0, np.int32), c_val=np.zeros(0))] * 3)
    assert all(p is None for i, p in enumerate(pkg.KnnIndex._visitor_args(*nothing)[1]) if i not in (0, 3))
    for mem in MEMS:
        for form in ("query", "recommend"):
            expect_refusal(raw_call(pkg, ix, form, placed(nothing, mem)), L.E_NOT_FOUND, lim.message(lim.EMPTY, 0, 0), 0)
    good_call_is_right()


# ---- i. the inputs are read only ----------------------------------------------------------------------------------------------

def test_inputs_are_read_only(pkg, index300):
    """Bites: `a.out_idx[f] = side.idx_p.p` read as the input array for device memory (the squeeze and the renumbering
    written into the caller's tensors: "a staged vector lies where its input lies" is about the offset, not the array; not
    tried)."""
    import torch
    d, ix = index300
    _, visitors = vc.base()
    vs = visitors[:17]                                                       # entries beyond the dimensions: the squeeze moves entries
    assert lim.beyond_total(vs, d["p_dim"], d["c_dim"]) == 51
    host = [a.copy() for a in vc.csr(vs)]
    before = [a.copy() for a in host]
    dev = on_device(host)
    dev_before = [t.clone() for t in dev]
    place_ids = np.arange(d["p_dim"], dtype=np.int64)
    for arrays in (host, dev):
        ix.visitors_query_batch(*arrays, 0.5, 0.5, 50)
        ix.visitors_recommend_batch(*arrays, 0.5, 0.5, 300)
        ix.visitors_recommend_ranked_batch(*arrays, 0.5, 0.5, 50, place_ids, place_ids % 3, np.arange(17) % 3, 10)
    torch.cuda.synchronize()
    for a, b in zip(host, before):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(dev, dev_before):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- j. the handles' visitor state ----------------------------------------------------------------------------------------------

def test_side_records_of_handles_that_come_and_go(pkg):
    """Every handle owns its visitor state - the renumbering its builder left and the stage buffers - as a member
    (knn_index.h: KnnVisitorSide), so handles that come and go, whatever addresses they get, serve their own visitors and
    take their buffers with them.  Bites: the builder leaving `new_of_old` anywhere two live handles share, or not at all
    (the second build's renumbering, or none, serves the first's visitors: other neighbours, `renumbered` 0); state that is
    not freed with the handle (device_bytes_in_use does not return)."""
    from locations_recommender_amd import _lib as L, synth
    start = L.device_bytes_in_use()
    _, visitors = vc.base()
    vs = [vc.without_beyond(v, 600, 20) for v in visitors[:17]]
    arrays = vc.csr(vs)

    def data(seed, integer=True):
        s = synth.small_knn_dataset(n=300, p_dim=600, seed=seed, integer=integer)
        return vc.explicit_ratings(s) if integer else dict(s, r_rowptr=s["p_rowptr"], r_place=s["p_idx"].astype(np.int64),
                                                           r_rating=np.floor(s["p_val"]).astype(np.int64))

    def right(name, d, ix, renumbered=1):
        check_query(ix, arrays, [want_similar((name, j), d, v, 50) for j, v in enumerate(vs)], 50)
        expect_stats(pkg, {}, renumbered=renumbered)
        check_rows(ix.visitors_recommend_batch(*arrays, 0.5, 0.5, 300), [want_rows((name, j), d, v, 300) for j, v in enumerate(vs)])

    da, db, dc_ = data(21), data(22), data(23)
    a, b = make_index(pkg, da), make_index(pkg, db)
    assert any(not np.array_equal(want_similar(("a", j), da, v, 50)[1], want_similar(("b", j), db, v, 50)[1]) for j, v in enumerate(vs))
    for _ in range(2):
        right("a", da, a)
        right("b", db, b)
    a.close()
    right("b", db, b)
    c = make_index(pkg, dc_)                 # whatever address it gets
    right("c", dc_, c)
    right("b", db, b)
    dg = data(22, integer=False)
    g = make_index(pkg, dg)
    assert g.info()["mode"] == 0
    right("g", dg, g, renumbered=0)
    right("c", dc_, c, renumbered=1)
    right("g", dg, g, renumbered=0)
    for ix in (b, c, g):
        ix.close()
    assert L.device_bytes_in_use() == start


# ---- k. the aggregation behind a visitors call --------------------------------------------------------------------------------

def test_aggregation_of_a_visitors_call(pkg, monkeypatch):
    """A visitors recommendation is aggregated place-major (lkb_aggregate_tile) for EVERY K: the LDS aggregation of the
    person batches (knn_aggregate_buckets / knn_aggregate) never runs for it, so aggregate_stats() stays at zero and
    LOCREC_KNN_AGG_SORT cannot change a bit; the person batch on the same handle afterwards still takes the bucket form.
    Bites: a visitors call that leaves `have_agg` or the out_rows of a person batch in a state the next aggregation reads."""
    from test_gpu_aggregate_buckets import SORT, make_index as make_with
    d, visitors = vc.base()
    n = len(d["person_ids"])
    js = list(range(17))
    arrays = vc.csr([visitors[j] for j in js])
    ix, ix_sort = make_with(pkg, d), make_with(pkg, d, monkeypatch, SORT)
    persons = d["person_ids"][:20]
    for k in (50, n):
        ix.aggregate_stats()
        rows = ix.visitors_recommend_batch(*arrays, 0.5, 0.5, k)
        st = ix.aggregate_stats()
        print("aggregate_stats after a visitors call at K =", k, st)
        assert st == {"buckets": 0, "sort": 0, "flagged": 0}
        check_rows(rows, [vc.expected_recommend(True, j, k) for j in js])
        other = ix_sort.visitors_recommend_batch(*arrays, 0.5, 0.5, k)
        assert np.array_equal(rows[0], other[0]) and np.array_equal(rows[1], other[1]) and np.array_equal(bits(rows[2]), bits(other[2]))
        want = ix_sort.recommend_batch(persons, 0.5, 0.5, 50)
        got = ix.recommend_batch(persons, 0.5, 0.5, 50)
        st = ix.aggregate_stats()
        assert st["buckets"] > 0 and st["flagged"] == 0, st
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
    ix.close()
    ix_sort.close()
