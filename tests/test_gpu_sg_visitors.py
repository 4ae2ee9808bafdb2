"""SG for visitors (locrec_sg_visitors_*): persons the resident graph G has no vertex for, given by their out-edges.

A visitor gets what makeRecommendations(V) returns on G + v - G's edge list followed by the visitor's edges under a new
id: the oracle on that list, and an SgGraph rebuilt from it, are the references (ids and (iterations, converged) equal,
probabilities within RTOL, test_gpu_sg_batch.py's rules).  A visitor's result depends on G and its own edges only, bit for
bit, whatever shares its tile.  The cases come from sg_visitor_cases.py (proven on the CPU by test_sg_visitor_cases.py)."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import sg_visitor_cases as cases

pytestmark = pytest.mark.gpu
RTOL = 1e-6   # test_gpu_sg_batch.py's RTOL: the project's standing bound for probabilities
ALPHA = cases.ALPHA


def rows_of(batch, i):
    off, ids, probs, its, conv = batch
    return ids[off[i]:off[i + 1]], probs[off[i]:off[i + 1]], int(its[i]), bool(conv[i])


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and tuple(a[2:]) == tuple(b[2:])


def check_reference(got, want, eps, what):
    """test_gpu_sg_batch.check_against_oracle's rules for one request"""
    ids, probs, it, conv = got
    wi, wp, wit, wconv = want
    assert np.array_equal(ids, wi), what
    if not (eps == 0 and (conv or wconv)):   # (an exact fp64 fixed point: the sweep that reaches it depends on the order of the sums)
        assert (it, conv) == (wit, bool(wconv)), what
    np.testing.assert_allclose(probs, wp, rtol=RTOL, atol=0, err_msg=str(what))


def call(sg, visitors, eps, max_it):
    return sg.visitors_recommend_batch(*cases.csr(visitors), ALPHA, eps, max_it)


def check_against_oracle(oracle, sg, graph, visitors, eps, max_it):
    batch = call(sg, visitors, eps, max_it)
    assert len(batch[0]) == len(visitors) + 1 and batch[0][0] == 0
    for i, v in enumerate(visitors):
        want = oracle.sg_recommend(*cases.plus(graph, v), v[0], ALPHA, eps, max_it)
        check_reference(rows_of(batch, i), want, eps, (v[0], eps, max_it))
    return batch


@pytest.fixture(scope="module")
def synth(pkg):
    graph, visitors = cases.synth_case()
    sg = pkg.SgGraph(*graph)
    yield graph, visitors, sg
    sg.close()


@pytest.fixture(scope="module")
def rebuilt(pkg):
    """SgGraph(E u v).recommend(V) for every visitor of the synthetic case at every parameter set: each graph built once"""
    graph, visitors = cases.synth_case()
    out = {}
    for i, v in enumerate(visitors):
        g = pkg.SgGraph(*cases.plus(graph, v))
        for eps, max_it in cases.PARAMS:
            out[i, eps, max_it] = g.recommend(v[0], ALPHA, eps, max_it)
        g.close()
    return out


def test_reference_kat_graph(pkg, oracle):
    graph, visitors = cases.kat_case()
    sg = pkg.SgGraph(*graph)
    for eps, max_it in cases.KAT_PARAMS:
        check_against_oracle(oracle, sg, graph, visitors, eps, max_it)
    assert sg.visitors_stats()["tiles"] == 1
    sg.close()


@pytest.mark.parametrize("eps,max_it", cases.PARAMS)
def test_synthetic_graph_40_visitors(oracle, synth, rebuilt, eps, max_it):
    graph, visitors, sg = synth
    batch = check_against_oracle(oracle, sg, graph, visitors, eps, max_it)
    for i in range(len(visitors)):
        check_reference(rows_of(batch, i), rebuilt[i, eps, max_it], eps, (i, eps, max_it, "rebuilt"))
    st = sg.visitors_stats()
    assert (st["tiles"], st["visitors"], st["set_up_launches"]) == (3, 40, 3)
    assert st["staged_edges"] == sum(len(v[1]) for v in visitors) and 0 < st["table_slots"] <= st["staged_edges"]


@pytest.mark.parametrize("form", ["default", "LOCREC_SG_NO_DICT", "LOCREC_SG_NO_COL16", "fp64 weights"])
def test_degree_class_graph(pkg, oracle, monkeypatch, form):
    graph, visitors = cases.degree_case(distinct_weights=form == "fp64 weights")
    if form.startswith("LOCREC"):
        monkeypatch.setenv(form, "1")
    sg = pkg.SgGraph(*graph)
    if form.startswith("LOCREC"):
        monkeypatch.delenv(form)
    assert (sg.info()["weight_dictionary"] > 0) == (form in ("default", "LOCREC_SG_NO_COL16"))
    for eps, max_it in cases.PARAMS:
        check_against_oracle(oracle, sg, graph, visitors, eps, max_it)
    sg.close()


def test_bits_do_not_depend_on_the_company(synth):
    graph, visitors, sg = synth
    x, others = visitors[0], visitors[1:]
    for eps, max_it in ((0.01, 20), (1e-6, 200), (0.01, 0)):
        alone = rows_of(call(sg, [x], eps, max_it), 0)
        assert same_bits(rows_of(call(sg, [x] + others[:7], eps, max_it), 0), alone)         # column 0
        assert same_bits(rows_of(call(sg, others[:15] + [x], eps, max_it), 15), alone)       # column 15 of a full tile
        assert same_bits(rows_of(call(sg, others[:16] + [x], eps, max_it), 16), alone)       # the 17th of 17
        twice = call(sg, [x, others[3], x], eps, max_it)                                      # twice in one call
        assert same_bits(rows_of(twice, 0), alone) and same_bits(rows_of(twice, 2), alone)
        assert same_bits(rows_of(call(sg, [x], eps, max_it), 0), alone)                       # a second call


def test_columns_of_a_tile_stop_at_different_sweeps(pkg, oracle):
    graph, (fast, slow), eps = cases.stop_case()
    sg = pkg.SgGraph(*graph)
    both = check_against_oracle(oracle, sg, graph, [fast, slow, fast], eps, cases.STOP_MAX_IT)
    assert [(int(i), bool(c)) for i, c in zip(both[3], both[4])] == [(3, True), (cases.STOP_MAX_IT, False), (3, True)]
    assert same_bits(rows_of(call(sg, [fast], eps, cases.STOP_MAX_IT), 0), rows_of(both, 0))
    assert same_bits(rows_of(call(sg, [slow], eps, cases.STOP_MAX_IT), 0), rows_of(both, 1))
    assert same_bits(rows_of(both, 2), rows_of(both, 0))
    sg.close()


def places_table():
    ids = np.r_[np.arange(40, 340), [45, 46, 47], [50, 51], [777_777]].astype(np.int64)     # listed twice; a second region
    regions = np.r_[np.where(np.arange(40, 340) % 2 == 0, 0, 2), [2, 0, 2], [1, 1], [0]].astype(np.int64)
    return ids, regions


@pytest.mark.parametrize("budget", ["1", "97", None])
def test_ranked_form(pkg, synth, monkeypatch, budget):
    from locations_recommender_amd import prep
    graph, visitors, sg = synth
    if budget is not None:
        monkeypatch.setenv("LOCREC_SG_RANKED_ROW_BUDGET", budget)
    visitors = visitors[:21]
    off, t, w = cases.csr(visitors)
    ids, regions = places_table()
    targets = np.array([(0, 2, 1, 7)[i % 4] for i in range(len(visitors))], np.int64)
    for eps, max_it, limit in ((0.01, 20, 10), (0.01, 0, 400), (0.01, 20, 0)):
        plain = sg.visitors_recommend_batch(off, t, w, ALPHA, eps, max_it)
        for exclude in (None, (off, t)):
            oi, op, cnt, its, conv = sg.visitors_recommend_ranked_batch(off, t, w, ALPHA, eps, max_it, ids, regions, targets, limit,
                                                                       exclude=exclude)
            x = exclude if exclude is not None else (np.zeros(len(visitors) + 1, np.int64), np.zeros(0, np.int64))
            wi, wp, wcnt = prep.rank_recommendations_batch_excluding(plain[0], plain[1], plain[2], ids, regions, targets, limit, *x)
            assert np.array_equal(cnt, wcnt) and np.array_equal(its, plain[3]) and np.array_equal(conv, plain[4])
            assert (cnt[targets == 7] == 0).all() and (limit == 0) == (cnt.max() == 0)
            for i in range(len(visitors)):
                assert np.array_equal(oi[i, :cnt[i]], wi[i, :cnt[i]]), (i, eps, max_it, limit)
                assert op[i, :cnt[i]].tobytes() == wp[i, :cnt[i]].tobytes(), (i, eps, max_it, limit)
                if exclude is not None:
                    assert not np.isin(oi[i, :cnt[i]], visitors[i][1]).any()
    assert sg.visitors_stats()["tiles"] == 2 and sg.ranked_batch_stats()["tiles"] == 2


def raw_call(pkg, sg, off, t, w, eps, max_it, room=4096, null_rows=False, nv=None):
    """the C entry with sentinel-filled outputs -> (status, outputs, capacity, bad visitor)"""
    from locations_recommender_amd import _lib as L
    nv = len(off) - 1 if nv is None else nv
    out_off = np.full(max(nv, 0) + 1, -7, np.int64)
    ids, probs = np.full(room, -7, np.int64), np.full(room, -7.0)
    its, conv = np.full(max(nv, 1), -7, np.int64), np.full(max(nv, 1), -7, np.int32)
    cap, bad = C.c_int64(room), C.c_int64(-5)
    st = L.lib().locrec_sg_visitors_recommend_batch(
        sg._h, nv, L.ptr(off, C.c_int64), L.ptr(t, C.c_int64), L.ptr(w, C.c_double), ALPHA, eps, max_it, L.ptr(out_off, C.c_int64),
        None if null_rows else L.ptr(ids, C.c_int64), None if null_rows else L.ptr(probs, C.c_double), C.byref(cap),
        L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32), C.byref(bad))
    return st, (out_off, ids, probs, its, conv), cap.value, bad.value


def untouched(outs):
    return all((a == -7).all() for a in outs)


def test_refusals(pkg, monkeypatch):
    from locations_recommender_amd import _lib as L
    graph, visitors = cases.kat_case()
    sg = pkg.SgGraph(*graph)
    sg_plus = pkg.SgGraph(*cases.plus(graph, (77, [2], [1.0])))   # 77: a source-only vertex of this graph
    i64, f64 = (lambda a: np.array(a, np.int64)), (lambda a: np.array(a, np.float64))
    good = (i64([0, 2, 3]), i64([2, 3, 5]), f64([0.5, 0.5, 1.0]))

    def refused(handle, off, t, w, status, bad, text, eps=0.05, max_it=1000, nv=None):
        st, outs, cap, got_bad = raw_call(pkg, handle, off, t, w, eps, max_it, nv=nv)
        assert st == status and untouched(outs) and cap == 4096 and got_bad == bad, (text, st, got_bad)
        assert text in L.lib().locrec_last_error().decode()

    refused(sg, None, good[1], good[2], L.E_INVALID_ARG, -1, "bad arguments", nv=2)
    refused(sg, good[0], None, good[2], L.E_INVALID_ARG, -1, "null array")
    refused(sg, good[0], good[1], None, L.E_INVALID_ARG, -1, "null array")
    refused(sg, good[0], good[1], good[2], L.E_INVALID_ARG, -1, "bad arguments", nv=-1)
    refused(sg, i64([1, 2, 3]), good[1], good[2], L.E_INVALID_ARG, -1, "edge_offsets")
    refused(sg, i64([0, 2, 1]), good[1], good[2], L.E_INVALID_ARG, -1, "edge_offsets")
    refused(sg, *good, L.E_INVALID_ARG, -1, "epsilon must be non-negative", eps=-0.1)
    refused(sg, *good, L.E_INVALID_ARG, -1, "max iterations number must be non-negative", max_it=-1)
    refused(sg, i64([0, 2, 2, 3]), good[1], good[2], L.E_NOT_FOUND, 1, "has no edges")
    refused(sg, good[0], i64([2, 3, 100]), good[2], L.E_NOT_FOUND, 1, "No such vertex in the graph: 100")
    refused(sg_plus, good[0], i64([2, 3, 77]), good[2], L.E_INVALID_ARG, 1, "no inbound edge")
    refused(sg, good[0], i64([2, 2, 5]), good[2], L.E_INVALID_ARG, 0, "twice")
    for x in (np.nan, np.inf, -np.inf):
        refused(sg, good[0], good[1], f64([0.5, x, 1.0]), L.E_INVALID_ARG, 0, "not finite")
    # the smallest offender among several: visitor 1 (unknown id) before visitor 2 (repeated target), behind a good one
    refused(sg, i64([0, 1, 2, 4]), i64([2, 100, 3, 3]), f64([1, 1, .5, .5]), L.E_NOT_FOUND, 1, "No such vertex in the graph: 100")
    refused(sg, i64([0, 1, 3, 4]), i64([2, 3, 3, 100]), f64([1, .5, .5, 1]), L.E_INVALID_ARG, 1, "twice")
    with pytest.raises(pkg.IllegalArgumentException, match="twice") as e:
        sg.visitors_recommend_batch([0, 2], [2, 2], [0.5, 0.5], ALPHA, 0.05, 10)
    assert e.value.bad_visitor == 0
    # the ranked entry refuses the same, and its own arguments
    ids, regions = places_table()
    with pytest.raises(pkg.IllegalArgumentException, match="No such vertex in the graph: 100") as e:
        sg.visitors_recommend_ranked_batch([0, 1, 2], [2, 100], [1.0, 1.0], ALPHA, 0.05, 10, ids, regions, [0, 0], 5)
    assert e.value.bad_visitor == 1
    with pytest.raises(pkg.IllegalArgumentException, match="excluded_offsets"):
        sg.visitors_recommend_ranked_batch([0, 1, 2], [2, 3], [1.0, 1.0], ALPHA, 0.05, 10, ids, regions, [0, 0], 5,
                                           exclude=([0, 2, 1], [5, 6]))
    # nobody: empty outputs
    st, outs, cap, bad = raw_call(pkg, sg, i64([0]), None, None, 0.05, 10)
    assert st == L.OK and outs[0][0] == 0 and cap == 0 and bad == -1 and untouched(outs[1:])
    assert len(sg.visitors_recommend_ranked_batch([0], [], [], ALPHA, 0.05, 10, ids, regions, [], 5)[2]) == 0
    # zero and negative weights are served
    st, outs, cap, bad = raw_call(pkg, sg, good[0], good[1], f64([0.0, -0.25, 1.0]), 0.05, 10)
    assert st == L.OK and bad == -1
    # the capacity protocol: one short (offsets and counters only), exact, and NULL row arrays
    st, full, need, _ = raw_call(pkg, sg, *good, 0.05, 1000)
    assert st == L.OK and need == full[0][2] > 0 and (full[3] >= 0).all()
    st, outs, cap, _ = raw_call(pkg, sg, *good, 0.05, 1000, room=need - 1)
    assert st == L.OK and cap == need and np.array_equal(outs[0], full[0]) and untouched(outs[1:3])
    assert np.array_equal(outs[3], full[3]) and np.array_equal(outs[4], full[4])
    st, outs, cap, _ = raw_call(pkg, sg, *good, 0.05, 1000, room=need)
    assert st == L.OK and cap == need and outs[1].tobytes() == full[1][:need].tobytes() and outs[2].tobytes() == full[2][:need].tobytes()
    st, outs, cap, _ = raw_call(pkg, sg, *good, 0.05, 1000, room=need, null_rows=True)
    assert st == L.E_INVALID_ARG
    st, outs, cap, _ = raw_call(pkg, sg, *good, 0.05, 1000, room=0, null_rows=True)
    assert st == L.OK and cap == need
    sg.close()
    sg_plus.close()
    # handles a batch refuses
    for by_target in (False, True):
        sh = pkg.SgGraph(*graph, shard_index=0, shard_count=2, by_target=by_target)
        refused(sh, *good, L.E_INVALID_ARG, -1, "sharded")
        sh.close()
    monkeypatch.setenv("LOCREC_SG_FUSED", "1")
    fused = pkg.SgGraph(*cases.synth_case()[0])
    monkeypatch.delenv("LOCREC_SG_FUSED")
    v = cases.synth_case()[1][0]
    refused(fused, *cases.csr([v]), L.E_INVALID_ARG, -1, "fused or persistent")
    fused.close()


def test_handle_serves_as_before(synth):
    graph, visitors, sg = synth
    person = int(graph[0].max())            # a source-only target
    place, category = 41, 3
    ids, regions = places_table()
    targets = [person, place, category, person]

    def everything():
        return (sg.recommend(person, ALPHA, 0.01, 20), sg.recommend(place, ALPHA, 0.01, 20),
                sg.recommend_batch(targets, ALPHA, 0.01, 20),
                sg.recommend_ranked_batch(targets, ALPHA, 0.01, 20, ids, regions, [0, 2, 0, 2], 10))

    def flat(r):
        return b"".join(np.asarray(a).tobytes() for part in r for a in (part if isinstance(part, tuple) else (part,)))

    before = flat(everything())
    sg.recommend(person, ALPHA, 0.01, 20)   # the handle's slots point at the single request's Q when the visitors arrive
    call(sg, visitors[:20], 0.01, 20)
    assert flat(everything()) == before
    off, t, w = cases.csr(visitors[:5])
    sg.visitors_recommend_ranked_batch(off, t, w, ALPHA, 0.01, 20, ids, regions, [0] * 5, 10)
    assert flat(everything()) == before


def test_visitor_edges_and_recommender(pkg, oracle, capsys):
    from locations_recommender_amd import prep
    rng = np.random.default_rng(3)
    n = 6_000
    pv = {"person_id": rng.integers(5_000, 5_300, n), "place_id": 100 + rng.zipf(1.5, n) % 400, "category_id": rng.integers(0, 12, n),
          "timestamp": rng.integers(0, 10 ** 9, n)}
    bpp, bpc = 0.4, 0.6
    src, dst, w = prep.generate_stochastic_graph(pv, bpp, bpc)
    asked = np.array([5_003, 5_100, 5_299])
    rows = np.isin(pv["person_id"], asked)
    assert np.isin(asked, pv["person_id"]).all()
    ids, off, t, vw, dropped = prep.visitor_edges(pv["person_id"][rows], pv["place_id"][rows], pv["category_id"][rows], bpp, bpc)
    assert np.array_equal(ids, asked) and not dropped.any()
    for i, p in enumerate(asked):   # the person's rows of the balanced edge list: places, then categories, each by id
        own = src == p
        assert np.array_equal(t[off[i]:off[i + 1]], dst[own]) and vw[off[i]:off[i + 1]].tobytes() == w[own].tobytes()
    # the graph of everybody else's visits: the visits to places nobody else went to are dropped, and counted
    src, dst, w = prep.generate_stochastic_graph({k: a[~rows] for k, a in pv.items()}, bpp, bpc)
    sg = pkg.SgGraph(src, dst, w)
    live = np.unique(dst)
    ids, off, t, vw, dropped = prep.visitor_edges(pv["person_id"][rows], pv["place_id"][rows], pv["category_id"][rows], bpp, bpc, graph=sg)
    for i, p in enumerate(asked):
        mine = pv["person_id"] == p
        assert dropped[i, 0] == (~np.isin(pv["place_id"][mine], live)).sum() and dropped[i, 1] == 0
        assert np.isin(t[off[i]:off[i + 1]], live).all()
    assert dropped[:, 0].sum() > 0
    sg.close()
    # makeRecommendationsForVisitor: the reference's console line, the oracle's rows
    edges = pd.DataFrame({"source_id": src, "target_id": dst, "balanced_weight": w})
    for eps, max_it, line in ((0.01, 20, "Converged in {} iterations\n"), (1e-9, 3, "Number of iterations {} reached the maximum 3\n")):
        rec = pkg.StochasticRecommender(edges, epsilon=eps, maxIterations=max_it)
        capsys.readouterr()
        df = rec.makeRecommendationsForVisitor(pd.DataFrame({"target_id": t[off[1]:off[2]], "balanced_weight": vw[off[1]:off[2]]}))
        out = capsys.readouterr().out
        wi, wp, wit, wconv = oracle.sg_recommend(*cases.plus((src, dst, w), (asked[1], t[off[1]:off[2]], vw[off[1]:off[2]])),
                                                 asked[1], ALPHA, eps, max_it)
        assert out == line.format(wit) and wconv == line.startswith("Conv")
        assert df["id"].tolist() == wi.tolist()
        np.testing.assert_allclose(df["probability"].to_numpy(), wp, rtol=RTOL, atol=0)
        rec.close()
    pkg.lib().locrec_cache_clear()


def test_sg_visitor_requests_on_a_parquet_set(pkg, oracle, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from locations_recommender_amd import mains, prep
    rng = np.random.default_rng(9)
    n = 5_000
    pv = {"person_id": rng.integers(5_000, 5_200, n), "place_id": 40 + rng.zipf(1.4, n) % 300, "category_id": rng.integers(0, 12, n),
          "timestamp": rng.integers(0, 10 ** 9, n)}
    bpp, bpc = 0.5, 0.5
    src, dst, w = prep.generate_stochastic_graph(pv, bpp, bpc)
    pq.write_table(pa.table({"source_id": src, "target_id": dst, "balanced_weight": w}), tmp_path / "stochastic_graph_region0_region2")
    ids, regions = places_table()
    pq.write_table(pa.table({"id": ids, "latitude": np.zeros(len(ids)), "longitude": np.zeros(len(ids)),
                             "region_id": pa.array(regions, pa.int32())}), tmp_path / "places_sample")
    m = 300   # newcomers: 19 visitors (two tiles), visits to known and to unknown places
    visits = {"visitor_id": rng.integers(9_000, 9_019, m), "place_id": 40 + rng.zipf(1.4, m) % 330, "category_id": rng.integers(0, 12, m)}
    live = np.unique(dst)
    for new_places in (False, True):
        got = mains.sg_visitor_requests(str(tmp_path), [0, 2], visits, {int(v): int(v) % 3 for v in np.unique(visits["visitor_id"])},
                                        0.01, 20, max_recommendations=7, new_places=new_places, beta_person_place=bpp,
                                        beta_person_category=bpc)
        assert [g[0] for g in got] == np.unique(visits["visitor_id"]).tolist() and len(got) > 16
        for vid, gi, gp in got:
            mine = visits["visitor_id"] == vid
            keep_p, keep_c = np.isin(visits["place_id"][mine], live), np.isin(visits["category_id"][mine], live)
            fams = [oracle_count_edges(visits["place_id"][mine][keep_p], bpp), oracle_count_edges(visits["category_id"][mine][keep_c], bpc)]
            t, vw = np.concatenate([f[0] for f in fams]), np.concatenate([f[1] for f in fams])
            oi, op, _, _ = oracle.sg_recommend(*cases.plus((src, dst, w), (vid, t, vw)), vid, ALPHA, 0.01, 20)
            if new_places:
                keep = ~np.isin(oi, t)
                oi, op = oi[keep], op[keep]
            wi, wp = oracle.rank_recommendations(oi, op, ids, regions, vid % 3, 7)
            assert gi.tolist() == wi.tolist(), vid
            np.testing.assert_allclose(gp, wp, rtol=RTOL, atol=0)
    pkg.lib().locrec_cache_clear()


def oracle_count_edges(targets, beta):
    """calc_count_edges for one source whose distinct targets stay within the top N, restated: count / total, times beta"""
    t, cnt = np.unique(targets, return_counts=True)
    assert len(t) <= 100
    return t, (cnt / cnt.sum()) * beta
