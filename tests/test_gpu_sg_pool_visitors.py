"""Visitors across a pool of graphs (locrec_sg_pool_visitors_*): ONE CSR of visitors, visitor v asked of member
graph_index[v].  Every visitor equals bit for bit what SgGraph.visitors_recommend_batch returns for it on its member alone,
whatever shares its call; a subset is checked against the oracle on G + v (test_gpu_sg_visitors.check_reference's rules,
RTOL the project's standing bound).  The cases come from sg_pool_visitor_cases.py (proven on the CPU by
test_sg_pool_visitor_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import sg_pool_visitor_cases as pc
import sg_visitor_cases as cases
from test_gpu_sg_visitors import check_reference, oracle_count_edges, rows_of, same_bits

pytestmark = pytest.mark.gpu
RTOL = 1e-6   # test_gpu_sg_batch.py's RTOL: the project's standing bound for probabilities
ALPHA = cases.ALPHA


def build(pkg, monkeypatch, graph, env=None):
    if env:
        monkeypatch.setenv(env, "1")
    sg = pkg.SgGraph(*graph)
    if env:
        monkeypatch.delenv(env)
    return sg


def pool_call(pool, asked, eps, max_it):
    return pool.visitors_recommend_batch(*pc.call_csr(asked), ALPHA, eps, max_it)


def own_rows(sgs, asked, eps, max_it):
    """position -> the rows of SgGraph.visitors_recommend_batch on the visitor's member, called with that member's visitors"""
    out = {}
    for g, sg in enumerate(sgs):
        at = pc.of_member(asked, g)
        if at:
            batch = sg.visitors_recommend_batch(*cases.csr([asked[i][1] for i in at]), ALPHA, eps, max_it)
            out.update({i: rows_of(batch, j) for j, i in enumerate(at)})
    return out


def check_equals_own(pool, sgs, asked, eps, max_it):
    got = pool_call(pool, asked, eps, max_it)
    assert len(got[0]) == len(asked) + 1 and got[0][0] == 0
    want = own_rows(sgs, asked, eps, max_it)
    for i in range(len(asked)):
        assert same_bits(rows_of(got, i), want[i]), (i, asked[i][0], eps, max_it)
    return got


@pytest.fixture(scope="module")
def mixed(pkg):
    """the mixed pool: the KAT graph and degree_case in its four forms"""
    mp = pytest.MonkeyPatch()
    graphs, asked, checked = pc.mixed_case()
    envs = (None, None, "LOCREC_SG_NO_DICT", "LOCREC_SG_NO_COL16", None)
    sgs = [build(pkg, mp, g, e) for g, e in zip(graphs, envs)]
    mp.undo()
    pool = pkg.SgPool(sgs)
    yield graphs, asked, checked, sgs, pool
    pool.close()
    for sg in sgs:
        sg.close()


@pytest.mark.parametrize("eps,max_it", cases.PARAMS)
def test_mixed_pool_equals_own_calls_and_oracle(pkg, oracle, mixed, eps, max_it):
    graphs, asked, checked, sgs, pool = mixed
    dicts = [sg.info()["weight_dictionary"] > 0 for sg in sgs]
    assert dicts[1] and not dicts[2] and dicts[3] and not dicts[4]
    got = check_equals_own(pool, sgs, asked, eps, max_it)
    for i in checked:
        g, v = asked[i]
        want = oracle.sg_recommend(*cases.plus(graphs[g], v), v[0], ALPHA, eps, max_it)
        check_reference(rows_of(got, i), want, eps, (i, g, eps, max_it))
    pool_call(pool, asked, eps, max_it)   # (own_rows ran other calls since: the counters are the last call's)
    st = pool.visitors_stats()
    assert (st["tile_waves"], st["set_up_launches"], st["begin_launches"], st["member_tiles"]) == (2, 2, 2, 5)
    assert (st["visitors"], st["stagings"], st["consumes"]) == (38, 1, 2)
    assert st["staged_edges"] == sum(len(v[1]) for _, v in asked)
    assert st["finalize_launches"] == st["rounds"]
    # the layout classes present: wave 0 holds the KAT graph and three forms, wave 1 the default form alone
    cls = [(g != 3, dicts[g]) for g in range(4)]   # (16-bit columns, dictionary)
    c0, c1 = len(set(cls)), 1
    executed = [int(got[3][i]) + 1 if got[4][i] else max_it for i in range(len(asked))]   # sweeps of every visitor
    second = set(pc.of_member(asked, 1)[16:])
    need0 = max(executed[i] for i in range(len(asked)) if i not in second)
    need1 = max(executed[i] for i in second)
    # rounds = r0 + r1 and sweep launches = c0 r0 + c1 r1: both waves' rounds follow, and each covers its slowest column
    r0, rem = divmod(st["sweep_launches"] - c1 * st["rounds"], c0 - c1)
    r1 = st["rounds"] - r0
    assert rem == 0 and need0 <= r0 <= max_it and need1 <= r1 <= max_it, (st, need0, need1)
    if eps == 0 or max_it == 0:   # no poll ends a wave early
        assert (r0, r1) == (max_it, max_it)


def test_slot_table_is_cleaned_between_waves(pkg, oracle):
    graph, visitors = pc.slot_case()
    sg = pkg.SgGraph(*graph)
    pool = pkg.SgPool([sg])
    asked = [(0, v) for v in visitors]
    for eps, max_it in pc.SLOT_PARAMS:
        got = pool_call(pool, asked, eps, max_it)
        assert pool.visitors_stats()["tile_waves"] == 2
        alone = rows_of(pool_call(pool, asked[16:], eps, max_it), 0)
        assert same_bits(rows_of(got, 16), alone)
        assert same_bits(alone, rows_of(sg.visitors_recommend_batch(*cases.csr(visitors[16:]), ALPHA, eps, max_it), 0))
        want = oracle.sg_recommend(*cases.plus(graph, visitors[16]), visitors[16][0], ALPHA, eps, max_it)
        check_reference(rows_of(got, 16), want, eps, (eps, max_it))
    pool.close()
    sg.close()


def test_a_member_drops_out_of_the_waves(pkg):
    graphs, asked = pc.drop_out_case()
    sgs = [pkg.SgGraph(*g) for g in graphs]
    pool = pkg.SgPool(sgs)
    for eps, max_it in ((0.01, 20), (1e-6, 200), (0.01, 0)):
        check_equals_own(pool, sgs, asked, eps, max_it)
        pool_call(pool, asked, eps, max_it)
        st = pool.visitors_stats()
        assert (st["tile_waves"], st["member_tiles"], st["set_up_launches"]) == (3, 6, 3)
    pool.close()
    for sg in sgs:
        sg.close()


def test_bits_do_not_depend_on_the_company(pkg):
    graph, v = cases.degree_case()
    sgs = [pkg.SgGraph(*graph) for _ in range(2)]
    pool = pkg.SgPool(sgs)
    x, others = v[3], v[4:] + v[:3]
    for eps, max_it in ((0.01, 20), (1e-6, 200), (0.01, 0)):
        alone = rows_of(pool_call(pool, [(0, x)], eps, max_it), 0)
        assert same_bits(alone, rows_of(sgs[0].visitors_recommend_batch(*cases.csr([x]), ALPHA, eps, max_it), 0))
        full = [(0, o) for o in others[:15]] + [(0, x)]
        assert same_bits(rows_of(pool_call(pool, full, eps, max_it), 15), alone)              # column 15 of a full tile
        seventeen = [(0, o) for o in others[:15]] + [(0, v[0]), (0, x)]
        assert same_bits(rows_of(pool_call(pool, seventeen, eps, max_it), 16), alone)         # the 17th of its member
        behind = [(1, others[i % 17]) for i in range(20)] + [(0, x)]
        assert same_bits(rows_of(pool_call(pool, behind, eps, max_it), 20), alone)            # behind 20 visitors of another member
        both = pool_call(pool, [(0, x), (1, others[0]), (1, x)], eps, max_it)                 # the same edges to two copies
        assert same_bits(rows_of(both, 0), alone) and same_bits(rows_of(both, 2), alone)
        twice = pool_call(pool, [(0, x), (0, x)], eps, max_it)                                # given twice: computed twice
        assert same_bits(rows_of(twice, 0), alone) and same_bits(rows_of(twice, 1), alone)
    pool.close()
    for sg in sgs:
        sg.close()


def test_members_and_columns_stop_at_different_rounds(pkg):
    stop, (fast, slow), eps = cases.stop_case()
    kat, kat_v = cases.kat_case()
    sgs = [pkg.SgGraph(*stop), pkg.SgGraph(*kat)]
    pool = pkg.SgPool(sgs)
    asked = [(0, fast), (1, kat_v[0]), (0, slow)]
    got = pool_call(pool, asked, eps, cases.STOP_MAX_IT)
    assert [(int(got[3][i]), bool(got[4][i])) for i in (0, 2)] == [(3, True), (cases.STOP_MAX_IT, False)]
    own_kat = rows_of(sgs[1].visitors_recommend_batch(*cases.csr(kat_v[:1]), ALPHA, eps, cases.STOP_MAX_IT), 0)
    assert same_bits(rows_of(got, 1), own_kat)
    # the fast column and the fast member are untouched by the rounds that only the slow column needs
    for i, v in ((0, fast), (2, slow)):
        assert same_bits(rows_of(got, i), rows_of(sgs[0].visitors_recommend_batch(*cases.csr([v]), ALPHA, eps, cases.STOP_MAX_IT), 0))
    assert same_bits(rows_of(pool_call(pool, asked[1:2], eps, cases.STOP_MAX_IT), 0), own_kat)
    pool.close()
    for sg in sgs:
        sg.close()


def places_table():
    """degree_case's live vertices 0 .. 39 and the KAT graph's 2, 3, 5 among them, over regions 0 and 2; three listed twice,
    two in a second region (1), one place no graph knows.  No place has region 7."""
    ids = np.r_[np.arange(0, 40), [5, 6, 7], [10, 11], [777_777]].astype(np.int64)
    regions = np.r_[np.where(np.arange(0, 40) % 2 == 0, 0, 2), [2, 0, 2], [1, 1], [0]].astype(np.int64)
    return ids, regions


@pytest.mark.parametrize("budget", ["1", "97", None])
def test_ranked_form(pkg, mixed, monkeypatch, budget):
    from locations_recommender_amd import prep
    graphs, asked, checked, sgs, pool = mixed
    if budget is not None:
        monkeypatch.setenv("LOCREC_SG_RANKED_ROW_BUDGET", budget)
    gi, off, t, w = pc.call_csr(asked)
    ids, regions = places_table()
    n = len(asked)
    targets = np.array([(0, 2, 1, 7)[i % 4] for i in range(n)], np.int64)
    for eps, max_it, limit in ((0.01, 20, 10), (0.01, 0, 400), (0.01, 20, 0)):
        plain = pool.visitors_recommend_batch(gi, off, t, w, ALPHA, eps, max_it)
        for exclude in (None, (off, t)):
            oi, op, cnt, its, conv = pool.visitors_recommend_ranked_batch(gi, off, t, w, ALPHA, eps, max_it, ids, regions, targets,
                                                                         limit, exclude=exclude)
            row_counts = pool.row_counts.copy()
            st = pool.visitors_stats()
            assert (st["tile_waves"], st["set_up_launches"], st["member_tiles"], st["consumes"]) == (2, 2, 5, 2)
            assert pool.ranked_stats()["tiles"] == 5
            x = exclude if exclude is not None else (np.zeros(n + 1, np.int64), np.zeros(0, np.int64))
            wi, wp, wcnt = prep.rank_recommendations_batch_excluding(plain[0], plain[1], plain[2], ids, regions, targets, limit, *x)
            assert np.array_equal(cnt, wcnt) and np.array_equal(its, plain[3]) and np.array_equal(conv, plain[4])
            assert np.array_equal(row_counts, np.diff(plain[0]))
            assert (cnt[targets == 7] == 0).all() and (limit == 0) == (cnt.max() == 0)
            for i in range(n):
                assert np.array_equal(oi[i, :cnt[i]], wi[i, :cnt[i]]), (i, eps, max_it, limit)
                assert op[i, :cnt[i]].tobytes() == wp[i, :cnt[i]].tobytes(), (i, eps, max_it, limit)
                if exclude is not None:
                    assert not np.isin(oi[i, :cnt[i]], asked[i][1][1]).any()
            for g, sg in enumerate(sgs):   # the member's own ranked visitors call
                at = pc.of_member(asked, g)
                if not at:
                    continue
                moff, mt, mw = cases.csr([asked[i][1] for i in at])
                mi, mp, mcnt, mits, mconv = sg.visitors_recommend_ranked_batch(
                    moff, mt, mw, ALPHA, eps, max_it, ids, regions, targets[at], limit, exclude=None if exclude is None else (moff, mt))
                assert np.array_equal(mcnt, cnt[at]) and np.array_equal(mits, its[at]) and np.array_equal(mconv, conv[at])
                for j, i in enumerate(at):
                    assert np.array_equal(mi[j, :mcnt[j]], oi[i, :cnt[i]]) and mp[j, :mcnt[j]].tobytes() == op[i, :cnt[i]].tobytes()


def raw_call(pool, gi, off, t, w, eps, max_it, room=1 << 14, null_rows=False, nv=None):
    """the C entry with sentinel-filled outputs -> (status, outputs, capacity, bad visitor)"""
    from locations_recommender_amd import _lib as L
    nv = len(off) - 1 if nv is None else nv
    out_off = np.full(max(nv, 0) + 1, -7, np.int64)
    ids, probs = np.full(max(room, 1), -7, np.int64), np.full(max(room, 1), -7.0)
    its, conv = np.full(max(nv, 1), -7, np.int64), np.full(max(nv, 1), -7, np.int32)
    cap, bad = C.c_int64(room), C.c_int64(-5)
    st = L.lib().locrec_sg_pool_visitors_recommend_batch(
        pool._h, nv, L.ptr(gi, C.c_int32), L.ptr(off, C.c_int64), L.ptr(t, C.c_int64), L.ptr(w, C.c_double), ALPHA, eps, max_it,
        L.ptr(out_off, C.c_int64), None if null_rows else L.ptr(ids, C.c_int64), None if null_rows else L.ptr(probs, C.c_double),
        C.byref(cap), L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32), C.byref(bad))
    return st, (out_off, ids, probs, its, conv), cap.value, bad.value


def untouched(outs):
    return all((a == -7).all() for a in outs)


def test_refusals_and_the_capacity_protocol(pkg):
    from locations_recommender_amd import _lib as L
    graph, _ = cases.kat_case()
    # member 0: the KAT graph; member 1: the same with a source-only vertex 77; member 2: nobody's
    sgs = [pkg.SgGraph(*graph), pkg.SgGraph(*cases.plus(graph, (77, [2], [1.0]))), pkg.SgGraph(*graph)]
    pool = pkg.SgPool(sgs)
    i32, i64, f64 = (lambda a: np.array(a, np.int32)), (lambda a: np.array(a, np.int64)), (lambda a: np.array(a, np.float64))
    # six visitors of one edge each, on members 1, 0, 0, 1, 0, 0
    gi, off = i32([1, 0, 0, 1, 0, 0]), i64([0, 1, 2, 3, 4, 5, 6])
    t, w = i64([2, 3, 5, 2, 3, 5]), f64([1.0, 0.5, 0.25, 1.0, 1.0, 1.0])

    def refused(status, bad, text, gi=gi, off=off, t=t, w=w, eps=0.05, max_it=1000, nv=None):
        st, outs, cap, got_bad = raw_call(pool, gi, off, t, w, eps, max_it, nv=nv)
        assert st == status and untouched(outs) and cap == 1 << 14 and got_bad == bad, (text, st, got_bad)
        assert text in L.lib().locrec_last_error().decode()

    def but(a, i, x):
        b = a.copy()
        b[i] = x
        return b

    refused(L.E_INVALID_ARG, -1, "bad arguments", gi=None)
    refused(L.E_INVALID_ARG, -1, "bad arguments", off=None, nv=6)
    refused(L.E_INVALID_ARG, -1, "null array", t=None)
    refused(L.E_INVALID_ARG, -1, "null array", w=None)
    refused(L.E_INVALID_ARG, -1, "bad arguments", nv=-1)
    refused(L.E_INVALID_ARG, -1, "edge_offsets", off=i64([1, 1, 2, 3, 4, 5, 6]))
    refused(L.E_INVALID_ARG, -1, "edge_offsets", off=i64([0, 1, 3, 2, 4, 5, 6]))
    refused(L.E_INVALID_ARG, -1, "epsilon must be non-negative", eps=-0.1)
    refused(L.E_INVALID_ARG, -1, "max iterations number must be non-negative", max_it=-1)
    # the require()s come before the graph indices, the graph indices before the visitors
    refused(L.E_INVALID_ARG, -1, "epsilon must be non-negative", gi=but(gi, 2, 9), eps=-0.1)
    refused(L.E_INVALID_ARG, 2, "names graph 3: the pool holds graphs 0 .. 2", gi=but(gi, 2, 3))
    refused(L.E_INVALID_ARG, 4, "names graph -1", gi=but(gi, 4, -1))
    refused(L.E_INVALID_ARG, 5, "names graph 3", gi=but(gi, 5, 3), t=but(t, 1, 100))   # position 5's index beats visitor 1's id
    # the visitors in call order, each against its own member
    refused(L.E_NOT_FOUND, 2, "visitor 2 has no edges", off=i64([0, 1, 2, 2, 4, 5, 6]))
    refused(L.E_NOT_FOUND, 1, "No such vertex in the graph: 100", t=but(t, 1, 100))
    refused(L.E_NOT_FOUND, 4, "No such vertex in the graph: 77", t=but(t, 4, 77))   # 77 is no vertex of member 0 ...
    refused(L.E_INVALID_ARG, 3, "no inbound edge", t=but(t, 3, 77))                 # ... and a source-only one of member 1
    refused(L.E_INVALID_ARG, 2, "twice", off=i64([0, 1, 2, 4, 4, 5, 6]), t=but(t, 3, 5), gi=but(gi, 3, 0))
    for x in (np.nan, np.inf, -np.inf):
        refused(L.E_INVALID_ARG, 3, "not finite", w=but(w, 3, x))
    # two bad visitors on different members: the smaller position wins, whichever member comes first in pool order
    refused(L.E_NOT_FOUND, 0, "No such vertex in the graph: 100", t=but(but(t, 0, 100), 1, 101))    # member 1's before member 0's
    refused(L.E_NOT_FOUND, 1, "No such vertex in the graph: 101", t=but(but(t, 3, 100), 1, 101))    # member 0's before member 1's
    with pytest.raises(pkg.IllegalArgumentException, match="No such vertex in the graph: 101") as e:
        pool.visitors_recommend_batch(gi, off, but(t, 1, 101), w, ALPHA, 0.05, 10)
    assert e.value.bad_visitor == 1
    # the ranked entry refuses the same, and its own arguments before the graph indices
    ids, regions = places_table()
    tgt = np.zeros(6, np.int64)
    with pytest.raises(pkg.IllegalArgumentException, match="names graph 3") as e:
        pool.visitors_recommend_ranked_batch(but(gi, 2, 3), off, t, w, ALPHA, 0.05, 10, ids, regions, tgt, 5)
    assert e.value.bad_visitor == 2
    with pytest.raises(pkg.IllegalArgumentException, match="twice") as e:
        pool.visitors_recommend_ranked_batch(but(gi, 3, 0), i64([0, 1, 2, 4, 4, 5, 6]), but(t, 3, 5), w, ALPHA, 0.05, 10, ids, regions, tgt, 5)
    assert e.value.bad_visitor == 2
    with pytest.raises(pkg.IllegalArgumentException, match="excluded_offsets") as e:
        pool.visitors_recommend_ranked_batch(but(gi, 2, 3), off, t, w, ALPHA, 0.05, 10, ids, regions, tgt, 5,
                                             exclude=([0, 2, 1, 2, 2, 2, 2], [5, 6]))
    assert e.value.bad_visitor == -1
    # nobody: empty outputs
    st, outs, cap, bad = raw_call(pool, None, i64([0]), None, None, 0.05, 10)
    assert st == L.OK and outs[0][0] == 0 and cap == 0 and bad == -1 and untouched(outs[1:])
    assert len(pool.visitors_recommend_ranked_batch([], [0], [], [], ALPHA, 0.05, 10, ids, regions, [], 5)[2]) == 0
    # zero and negative weights are served
    st, outs, cap, bad = raw_call(pool, gi, off, t, f64([0.0, -0.25, 1.0, 1.0, 0.0, -1.0]), 0.05, 10)
    assert st == L.OK and bad == -1
    # the capacity protocol: one short (offsets and counters only), exact, and NULL row arrays
    st, full, need, _ = raw_call(pool, gi, off, t, w, 0.05, 1000)
    assert st == L.OK and need == full[0][6] > 0 and (full[3] >= 0).all()
    st, outs, cap, _ = raw_call(pool, gi, off, t, w, 0.05, 1000, room=need - 1)
    assert st == L.OK and cap == need and np.array_equal(outs[0], full[0]) and untouched(outs[1:3])
    assert np.array_equal(outs[3], full[3]) and np.array_equal(outs[4], full[4])
    st, outs, cap, _ = raw_call(pool, gi, off, t, w, 0.05, 1000, room=need)
    assert st == L.OK and cap == need and outs[1].tobytes() == full[1][:need].tobytes() and outs[2].tobytes() == full[2][:need].tobytes()
    st, outs, cap, _ = raw_call(pool, gi, off, t, w, 0.05, 1000, room=need, null_rows=True)
    assert st == L.E_INVALID_ARG
    st, outs, cap, _ = raw_call(pool, gi, off, t, w, 0.05, 1000, room=0, null_rows=True)
    assert st == L.OK and cap == need
    pool.close()
    for sg in sgs:
        sg.close()


def flat(r):
    return b"".join(np.asarray(a).tobytes() for part in r for a in (part if isinstance(part, tuple) else (part,)))


def test_handle_and_pool_state_around_a_call(pkg):
    from locations_recommender_amd import _lib as L
    graph, visitors = cases.synth_case()
    kat, kat_v = cases.kat_case()
    sgs = [pkg.SgGraph(*graph), pkg.SgGraph(*kat)]
    pool = pkg.SgPool(sgs)
    person = int(graph[0].max())            # a source-only target
    ids = np.arange(40, 340).astype(np.int64)
    regions = (ids % 3).astype(np.int64)
    targets = [person, 41, 3, person]
    pgi, pv = np.array([0, 1, 0, 0], np.int32), np.array([person, 2, 41, 3], np.int64)
    asked = pc.interleave([visitors[:20], kat_v[:1]])
    gi, off, t, w = pc.call_csr(asked)

    def everything():
        sg = sgs[0]
        return (sg.recommend(person, ALPHA, 0.01, 20), sg.recommend(41, ALPHA, 0.01, 20), sg.recommend_batch(targets, ALPHA, 0.01, 20),
                sg.recommend_ranked_batch(targets, ALPHA, 0.01, 20, ids, regions, [0, 2, 0, 2], 10),
                sg.visitors_recommend_batch(*cases.csr(visitors[:5]), ALPHA, 0.01, 20),
                sgs[1].recommend(2, ALPHA, 0.01, 20),
                pool.recommend_batch(pgi, pv, ALPHA, 0.01, 20),
                pool.recommend_ranked_batch(pgi, pv, ALPHA, 0.01, 20, ids, regions, [0, 2, 0, 1], 10))

    before = flat(everything())
    sgs[0].recommend(person, ALPHA, 0.01, 20)   # the member's slots point at the single request's Q when the visitors arrive
    first = pool.visitors_recommend_batch(gi, off, t, w, ALPHA, 0.01, 20)
    assert flat(everything()) == before
    pool.visitors_recommend_ranked_batch(gi, off, t, w, ALPHA, 0.01, 20, ids, regions, np.zeros(len(gi), np.int64), 10)
    assert flat(everything()) == before
    # person calls and visitors calls alternate on one pool
    p1 = flat(pool.recommend_batch(pgi, pv, ALPHA, 0.01, 20))
    v1 = flat(pool.visitors_recommend_batch(gi, off, t, w, ALPHA, 0.01, 20))
    p2 = flat(pool.recommend_batch(pgi, pv, ALPHA, 0.01, 20))
    assert p1 == p2 and v1 == flat(first)
    # a repeated call of the same shape allocates the call's staging (two buffers) and nothing for the tables
    counts = []
    for _ in range(2):
        a0 = L.device_allocations()
        assert flat(pool.visitors_recommend_batch(gi, off, t, w, ALPHA, 0.01, 20)) == v1
        counts.append(L.device_allocations() - a0)
    assert counts == [2, 2]
    pool.close()
    for sg in sgs:
        sg.close()


def test_plain_copy_read_back(pkg, monkeypatch):
    graph, v = cases.degree_case()
    sgs = [build(pkg, monkeypatch, graph, "LOCREC_SG_NO_PACK"), pkg.SgGraph(*graph)]
    pool = pkg.SgPool(sgs)
    asked = pc.interleave([v[:17], v[5:8]])
    check_equals_own(pool, sgs, asked, 0.01, 20)
    ids, regions = places_table()
    gi, off, t, w = pc.call_csr(asked)
    tgt = np.array([(0, 2)[i % 2] for i in range(len(asked))], np.int64)
    oi, op, cnt, its, conv = pool.visitors_recommend_ranked_batch(gi, off, t, w, ALPHA, 0.01, 20, ids, regions, tgt, 10)
    for g, sg in enumerate(sgs):
        at = pc.of_member(asked, g)
        mi, mp, mcnt, mits, mconv = sg.visitors_recommend_ranked_batch(*cases.csr([asked[i][1] for i in at]), ALPHA, 0.01, 20, ids,
                                                                       regions, tgt[at], 10)
        assert np.array_equal(mcnt, cnt[at]) and np.array_equal(mits, its[at])
        for j, i in enumerate(at):
            assert np.array_equal(mi[j, :mcnt[j]], oi[i, :cnt[i]]) and mp[j, :mcnt[j]].tobytes() == op[i, :cnt[i]].tobytes()
    pool.close()
    for sg in sgs:
        sg.close()


def test_sg_visitor_requests_pooled_on_two_parquet_sets(pkg, oracle, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from locations_recommender_amd import mains, prep
    rng = np.random.default_rng(19)
    bpp, bpc = 0.5, 0.5
    sets = {}
    # two region sets: [0, 2] knows places 40 .. 339, [1, 2] places 200 .. 499
    for name, first in (("region0_region2", 40), ("region1_region2", 200)):
        n = 4_000
        pv = {"person_id": rng.integers(5_000, 5_200, n), "place_id": first + rng.zipf(1.4, n) % 300, "category_id": rng.integers(0, 12, n),
              "timestamp": rng.integers(0, 10 ** 9, n)}
        src, dst, w = prep.generate_stochastic_graph(pv, bpp, bpc)
        pq.write_table(pa.table({"source_id": src, "target_id": dst, "balanced_weight": w}), tmp_path / f"stochastic_graph_{name}")
        sets[name] = (src, dst, w)
    ids = np.arange(40, 500).astype(np.int64)
    regions = (ids % 3).astype(np.int64)
    pq.write_table(pa.table({"id": ids, "latitude": np.zeros(len(ids)), "longitude": np.zeros(len(ids)),
                             "region_id": pa.array(regions, pa.int32())}), tmp_path / "places_sample")
    # 19 visitors at home in region 0, 4 in region 1, all bound for region 2; one whose every visit is unknown to its set
    m = 400
    visits = {"visitor_id": rng.integers(9_000, 9_023, m), "place_id": 40 + rng.zipf(1.3, m) % 460, "category_id": rng.integers(0, 12, m)}
    assert len(np.unique(visits["visitor_id"])) == 23
    lost = 9_021   # at home in region 1: places and categories that set has no vertex for
    keep = visits["visitor_id"] != lost
    visits = {k: np.r_[a[keep], x] for (k, a), x in zip(visits.items(), ([lost] * 3, [41, 42, 43], [900, 901, 902]))}
    homes = {int(v): (0 if v < 9_019 else 1) for v in np.unique(visits["visitor_id"])}
    live = {name: np.unique(s[1]) for name, s in sets.items()}
    only_one = sum(np.isin(p, live["region0_region2"]) != np.isin(p, live["region1_region2"]) for p in visits["place_id"])
    assert only_one > 0
    for new_places in (False, True):
        got = [mains.sg_visitor_requests_pooled(str(tmp_path), visits, homes, 2, 0.01, 20, max_recommendations=7, new_places=new_places,
                                                beta_person_place=bpp, beta_person_category=bpc, pooled=pooled) for pooled in (True, False)]
        assert len(got[0]) == len(got[1]) == 23
        for a, b in zip(*got):
            if isinstance(a, Exception):
                assert type(a) is type(b) and "has no edges" in str(a) and "has no edges" in str(b)
                continue
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()
        assert [i for i, g in enumerate(got[0]) if isinstance(g, Exception)] == [21]
        for entry in got[0][::3]:
            if isinstance(entry, Exception):
                continue
            vid, gi_, gp = entry
            name = "region0_region2" if homes[vid] == 0 else "region1_region2"
            mine = visits["visitor_id"] == vid
            keep_p, keep_c = np.isin(visits["place_id"][mine], live[name]), np.isin(visits["category_id"][mine], live[name])
            fams = [oracle_count_edges(visits["place_id"][mine][keep_p], bpp), oracle_count_edges(visits["category_id"][mine][keep_c], bpc)]
            t, vw = np.concatenate([f[0] for f in fams]), np.concatenate([f[1] for f in fams])
            oi, op, _, _ = oracle.sg_recommend(*cases.plus(sets[name], (vid, t, vw)), vid, ALPHA, 0.01, 20)
            if new_places:
                sel = ~np.isin(oi, t)
                oi, op = oi[sel], op[sel]
            wi, wp = oracle.rank_recommendations(oi, op, ids, regions, 2, 7)
            assert gi_.tolist() == wi.tolist(), vid
            np.testing.assert_allclose(gp, wp, rtol=RTOL, atol=0)
    pkg.lib().locrec_cache_clear()
