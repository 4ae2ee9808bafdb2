"""A pool of resident graphs serving one mixed batch of (graph, vertex) requests (locrec_sg_pool_*, stochastic.SgPool,
mains.sg_recommender_requests).

Every request of a pool call must equal the single request on the same handle bit for bit - ids, probability bits, the
0-based iteration counter and the converged flag - whatever shares its launches: other graphs' tiles, graphs of another
layout class, graphs that drop out after the first tile wave, tiles that finish at other rounds.  A subset is compared
with the oracle at rtol 1e-6 (with epsilon 0 the counters of a converged request may be one apart from the oracle's, as
test_gpu_sg_batch.check_against_oracle documents).  Afterwards every member serves requests as a fresh handle."""
import ctypes as C

import numpy as np
import pytest
from test_gpu_sg_batch import (check_against_oracle, d2_trajectory, kat, kat_edges, mixed_targets, rows_of,  # noqa: F401
                               same_bits)

pytestmark = pytest.mark.gpu
ALPHA = 0.15
TILE = 16


def edges_of(g):
    return g["source_id"], g["target_id"], g["balanced_weight"]


def interleave(per_graph):
    """[(graph, [vertices])] -> (graph_index, vertex_ids), the graphs' requests taken in turn."""
    gi, v = [], []
    for k in range(max(len(t) for _, t in per_graph)):
        for g, t in per_graph:
            if k < len(t):
                gi.append(g)
                v.append(int(t[k]))
    return np.array(gi, np.int32), np.array(v, np.int64)


def check_pool_against_singles(pool, gi, v, eps, max_it):
    """The pool call, every request compared with SgGraph.recommend on the same handle (once per distinct pair)."""
    batch = pool.recommend_batch(gi, v, ALPHA, eps, max_it)
    assert len(batch[0]) == len(v) + 1 and batch[0][0] == 0
    singles = {}
    for i, (g, x) in enumerate(zip(gi.tolist(), v.tolist())):
        if (g, x) not in singles:
            singles[g, x] = pool.graphs[g].recommend(x, ALPHA, eps, max_it)
        assert same_bits(rows_of(batch, i), singles[g, x]), (i, g, x, eps, max_it)
    return batch


@pytest.fixture(scope="module")
def mixed(pkg):
    """Five members: the reference's test graph, three synthetic ones whose category and place ids overlap, and one
    nobody asks.  About 40 targets (three tiles, the last one partial) on the largest, so that the others drop out after
    the first tile wave."""
    from locations_recommender_amd import synth
    data = [synth.sg_dataset(3_000, 300, 20, seed=77), synth.sg_dataset(500, 60, 20, seed=78),
            synth.sg_dataset(200, 30, 5, seed=79)]
    edges = [kat_edges(kat())] + [edges_of(g) for g in data] + [edges_of(data[2])]
    graphs = [pkg.SgGraph(*e) for e in edges]
    pool = pkg.SgPool(graphs)
    # 45 (a place) and 2 (a category) are asked of two graphs each
    big = np.r_[mixed_targets(data[0], 300, 20, seed=5), 45, 2]
    assert len(np.unique(big)) > 2 * TILE and len(np.unique(big)) % TILE != 0
    p1 = int(data[1]["first_person"])
    gi, v = interleave([(0, [1, 1, 3, 5]), (1, big), (2, [p1, 45, 2, p1 + 7, 45, p1, 3, 41]), (3, [45])])
    yield {"edges": edges, "graphs": graphs, "pool": pool, "gi": gi, "v": v}
    pool.close()
    for g in graphs:
        g.close()


@pytest.mark.parametrize("eps,max_it", [(0.01, 20), (0.0, 100), (0.01, 0), (1e-6, 200)])
def test_mixed_pool_matches_single_requests_and_oracle(pkg, oracle, mixed, eps, max_it):
    gi, v, pool = mixed["gi"], mixed["v"], mixed["pool"]
    batch = check_pool_against_singles(pool, gi, v, eps, max_it)
    st = pool.stats()
    assert st["tile_waves"] == 3                        # 33 .. 47 distinct targets on graph 1, at most 16 elsewhere
    assert st["finalize_launches"] == st["rounds"] and st["rounds"] <= st["sweep_launches"] <= 4 * st["rounds"]
    if eps == 0 or max_it <= 4:
        assert st["polls"] == 0 and st["rounds"] == 3 * max_it
    for g in (0, 1, 2, 3):
        which = np.flatnonzero(gi == g)[::5 if g == 1 else 2]
        check_against_oracle(oracle, *mixed["edges"][g], batch, v, eps, max_it, which)
    # duplicates of a (graph, vertex) pair are copies
    first = {}
    for i, key in enumerate(zip(gi.tolist(), v.tolist())):
        if key in first:
            assert same_bits(rows_of(batch, i), rows_of(batch, first[key]))
        first.setdefault(key, i)
    assert len(first) < len(v)


def test_mixed_pool_gives_the_reference_lists(pkg, mixed):
    """StochasticRecommenderTest.scala:39-94: targets [1, 1, 3, 5] on the reference's graph, beside every other member's
    requests, at the reference's two parameter sets; target 1 gives its expected lists exactly."""
    gi, v, pool = mixed["gi"], mixed["v"], mixed["pool"]
    cases = [c for c in kat()["cases"] if "expected_error" not in c]
    assert cases
    for case in cases:
        batch = check_pool_against_singles(pool, gi, v, case["epsilon"], case["max_iterations"])
        want = sorted((tuple(x) for x in case["expected_sorted_by_probability_desc"]), key=lambda t: t[0])
        mine = np.flatnonzero(gi == 0)
        assert v[mine].tolist() == [1, 1, 3, 5]
        for i in mine[:2]:
            ids, probs, _, _ = rows_of(batch, i)
            assert list(zip(ids.tolist(), probs.tolist())) == want, case["name"]


def test_graphs_and_columns_stop_at_different_rounds(pkg, oracle):
    """The two-cycle graph of test_targets_of_a_tile_stop_at_different_sweeps beside the reference's graph: columns of a
    tile, tiles of a wave and graphs stop at different rounds; finished ones must stay as they were."""
    rng = np.random.default_rng(17)
    n = 400
    src = np.r_[rng.integers(1000, 1000 + n, 4000), rng.integers(0, 30, 600), 2000, 2001]
    dst = np.r_[rng.integers(0, 30, 4000), rng.integers(0, 30, 600), 2001, 2000]
    w = np.r_[rng.random(4600) / 30, 1.0, 1.0]
    slow, fast = 2000, 1000
    ds, df = d2_trajectory(src, dst, w, slow, 60), d2_trajectory(src, dst, w, fast, 60)
    k = next(i for i in range(60) if df[i] < ds[i] / 100)
    eps = float(np.sqrt(np.sqrt(df[k] * ds[k])))
    targets = np.r_[slow, fast, np.arange(1001, 1040), 5, 2001].astype(np.int64)
    ksrc, kdst, kw = kat_edges(kat())
    graphs = [pkg.SgGraph(src, dst, w), pkg.SgGraph(ksrc, kdst, kw)]
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(0, targets), (1, [1, 3, 5])])
    batch = check_pool_against_singles(pool, gi, v, eps, 200)
    its = batch[3]
    assert len(set(its[gi == 0].tolist())) > 1 and batch[4].all()
    assert set(its[gi == 1].tolist()) != set(its[gi == 0].tolist())
    check_against_oracle(oracle, src, dst, w, batch, v, eps, 200, np.flatnonzero(gi == 0)[::4])
    check_against_oracle(oracle, ksrc, kdst, kw, batch, v, eps, 200, np.flatnonzero(gi == 1))
    st = pool.stats()
    assert st["tile_waves"] == 3 and st["polls"] > 0 and st["rounds"] < 3 * 200
    pool.close()
    for g in graphs:
        g.close()


def test_layout_classes_share_a_pool(pkg, oracle, monkeypatch):
    """uint16 / int32 columns x dictionary / fp64 weights in one pool: one sweep launch per class present and round, one
    finalize launch per round.  (The member created under both switches is the fourth class.)"""
    from locations_recommender_amd import synth
    g = synth.sg_dataset(n_persons=2_000, n_places=200, n_categories=10, seed=41)
    rng = np.random.default_rng(21)
    fw = rng.random(20_000) / 40
    fsrc = rng.integers(1000, 1300, 20_000).astype(np.int64)
    fdst = rng.integers(0, 40, 20_000).astype(np.int64)
    ftargets = np.r_[rng.choice(np.arange(1000, 1300), 30, replace=False), np.arange(0, 40, 4), [1000, 1003, 0]]

    def create(edges, *envs):
        for e in envs:
            monkeypatch.setenv(e, "1")
        h = pkg.SgGraph(*edges)
        for e in envs:
            monkeypatch.delenv(e)
        return h

    edges = [edges_of(g), edges_of(g), (fsrc, fdst, fw), edges_of(g), edges_of(g)]
    graphs = [create(edges[0], "LOCREC_SG_NO_DICT"), create(edges[1], "LOCREC_SG_NO_COL16"), create(edges[2]),
              create(edges[3]), create(edges[4], "LOCREC_SG_NO_DICT", "LOCREC_SG_NO_COL16")]
    dicts = [h.info()["weight_dictionary"] > 0 for h in graphs]
    assert dicts == [False, True, False, True, False]            # both weight forms are present
    some = mixed_targets(g, 200, 10, seed=3)
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(0, some[:20]), (1, some[10:24]), (2, ftargets), (3, some[:5]), (4, some[18:40])])
    for eps, max_it in ((0.01, 20), (0.0, 12), (0.01, 0)):
        batch = check_pool_against_singles(pool, gi, v, eps, max_it)
        st = pool.stats()
        assert st["sweep_launches"] <= 4 * st["rounds"] and st["finalize_launches"] == st["rounds"]
        if max_it > 0:
            assert st["sweep_launches"] > st["rounds"]         # more than one class was launched
        for k in range(5):
            check_against_oracle(oracle, *edges[k], batch, v, eps, max_it, np.flatnonzero(gi == k)[::6])
    pool.close()
    for h in graphs:
        h.close()


def test_launches_are_shared(pkg):
    """The point of the pool: twelve graphs' rounds are ONE sweep and ONE finalize launch each, and a second tile wave
    exists only because one graph has a seventeenth target.  No loop over graphs meets these counts."""
    from locations_recommender_amd import synth
    data = [synth.sg_dataset(400, 50, 8, seed=100 + i) for i in range(12)]
    graphs = [pkg.SgGraph(*edges_of(g)) for g in data]
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(i, [int(g["first_person"]) + 3, 41]) for i, g in enumerate(data)])
    check_pool_against_singles(pool, gi, v, 0.0, 10)
    assert pool.stats() == dict(pool.stats(), tile_waves=1, rounds=10, sweep_launches=10, finalize_launches=10, polls=0)
    per_graph = [(i, [int(g["first_person"]) + 3, 41]) for i, g in enumerate(data)]
    per_graph[5] = (5, (int(data[5]["first_person"]) + np.arange(17)).tolist())
    gi, v = interleave(per_graph)
    check_pool_against_singles(pool, gi, v, 0.0, 10)
    st = pool.stats()
    assert st["tile_waves"] == 2 and st["rounds"] == 20 and st["sweep_launches"] == 20 and st["finalize_launches"] == 20
    assert st["polls"] == 0 and st["readback_bytes"] > 0
    pool.close()
    for g in graphs:
        g.close()


def test_few_private_rows(pkg):
    """T = 65,530 with uint16 columns: tiles of five on that member (test_uint16_columns_with_few_private_rows), so its
    twelve targets take three tile waves while the small member beside it is done after the first."""
    from locations_recommender_amd import synth
    T, n_persons = 65_530, 1_500
    live = np.arange(T, dtype=np.int64)
    persons = 100_000 + np.arange(n_persons, dtype=np.int64)
    src = np.concatenate([persons[live % n_persons], live, persons[:40]])
    dst = np.concatenate([live, (live * 7 + 1) % T, np.arange(40, dtype=np.int64)])
    outdeg = np.bincount(np.searchsorted(np.unique(src), src))
    w = 1.0 / outdeg[np.searchsorted(np.unique(src), src)]
    small = synth.sg_dataset(200, 30, 5, seed=79)
    graphs = [pkg.SgGraph(src, dst, w), pkg.SgGraph(*edges_of(small))]
    assert graphs[0].live_count() == T
    targets = [100_000, 5, 100_001, 100_002, 100_003, 100_004, 7, 100_005, 100_000, 65_529, 100_006, 100_039]
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(0, targets), (1, [int(small["first_person"]), 41, 2])])
    for eps, max_it in ((0.01, 20), (0.0, 12)):
        check_pool_against_singles(pool, gi, v, eps, max_it)
        assert pool.stats()["tile_waves"] == 3
    pool.close()
    for g in graphs:
        g.close()


def test_plain_copy_read_back(pkg, monkeypatch):
    """A member created under LOCREC_SG_NO_PACK: polls and read-back of the whole pool go through plain copies."""
    from locations_recommender_amd import synth
    data = [synth.sg_dataset(500, 60, 20, seed=78), synth.sg_dataset(200, 30, 5, seed=79)]
    monkeypatch.setenv("LOCREC_SG_NO_PACK", "1")
    graphs = [pkg.SgGraph(*edges_of(data[0]))]
    monkeypatch.delenv("LOCREC_SG_NO_PACK")
    graphs.append(pkg.SgGraph(*edges_of(data[1])))
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(0, (int(data[0]["first_person"]) + np.arange(0, 40, 2)).tolist() + [44, 3]),
                        (1, [int(data[1]["first_person"]), 41, 2])])
    for eps, max_it in ((0.01, 20), (0.0, 7)):
        check_pool_against_singles(pool, gi, v, eps, max_it)
        assert pool.stats()["tile_waves"] == 2
    pool.close()
    for g in graphs:
        g.close()


def test_handle_state_around_a_pool_call(pkg):
    """Single requests, per-graph batches and a group run give a fresh handle's bits before and after a pool call; a
    second identical pool call returns the same arrays and allocates nothing on the device."""
    from locations_recommender_amd import _lib, synth
    data = [synth.sg_dataset(500, 60, 20, seed=78), synth.sg_dataset(200, 30, 5, seed=79)]
    edges = [kat_edges(kat())] + [edges_of(g) for g in data]
    single_v = [1, int(data[0]["first_person"]) + 11, int(data[1]["first_person"]) + 4]          # persons: source-only
    batch_v = [[5, 3, 1], [int(data[0]["first_person"]) + 2, 44, 3, int(data[0]["first_person"]) + 11],
               [int(data[1]["first_person"]), 41]]
    want_single, want_batch = [], []
    for e, sv, bv in zip(edges, single_v, batch_v):
        h = pkg.SgGraph(*e)
        want_single.append(h.recommend(sv, ALPHA, 0.01, 20))
        h.close()
        h = pkg.SgGraph(*e)
        want_batch.append(h.recommend_batch(bv, ALPHA, 0.01, 20))
        h.close()
    graphs = [pkg.SgGraph(*e) for e in edges]
    grp = pkg.SgGroup(graphs)

    def members_are_fresh():
        for h, sv, bv, ws, wb in zip(graphs, single_v, batch_v, want_single, want_batch):
            assert same_bits(h.recommend(sv, ALPHA, 0.01, 20), ws)
            assert all(np.array_equal(a, b) for a, b in zip(h.recommend_batch(bv, ALPHA, 0.01, 20), wb))
        grp.iterate_async(single_v, ALPHA, 0.01, 20)
        for h, ws in zip(graphs, want_single):
            assert same_bits(h.fetch(), ws)
        for h, sv, ws in zip(graphs, single_v, want_single):   # (leaves every handle's slots pointing at its Q)
            assert same_bits(h.recommend(sv, ALPHA, 0.01, 20), ws)

    members_are_fresh()
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(k, bv + [sv]) for k, (bv, sv) in enumerate(zip(batch_v, single_v))])
    first = check_pool_against_singles(pool, gi, v, 0.01, 20)
    members_are_fresh()
    allocs = _lib.device_allocations()
    second = pool.recommend_batch(gi, v, ALPHA, 0.01, 20)
    assert _lib.device_allocations() == allocs, "a repeated pool call of the same shape allocated device memory"
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert first[2].tobytes() == second[2].tobytes()
    members_are_fresh()
    pool.close()
    grp.close()
    for h in graphs:
        h.close()


def test_capacity_protocol_empty_list_and_refusals(pkg, monkeypatch):
    from locations_recommender_amd import _lib as L
    from locations_recommender_amd import synth
    src, dst, w = kat_edges(kat())
    small = synth.sg_dataset(200, 30, 5, seed=79)
    graphs = [pkg.SgGraph(src, dst, w), pkg.SgGraph(*edges_of(small))]
    pool = pkg.SgPool(graphs)
    gi = np.array([0, 1, 0, 0, 1], np.int32)
    v = np.array([5, 41, 3, 1, int(small["first_person"])], np.int64)
    off, _, _, want_its, want_conv = batch = pool.recommend_batch(gi, v, ALPHA, 0.05, 1000)
    total = int(off[-1])
    assert total > 2

    def call(gi, v, offsets, ids, probs, cap, its, conv, bad, eps=0.05, max_it=1000):
        L.check(L.lib().locrec_sg_pool_recommend_batch(
            pool._h, len(v), L.ptr(gi, C.c_int32), L.ptr(v, C.c_int64), ALPHA, eps, max_it, L.ptr(offsets, C.c_int64),
            L.ptr(ids, C.c_int64), L.ptr(probs, C.c_double), C.byref(cap), L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32),
            C.byref(bad) if bad is not None else None))

    off2 = np.full(6, -1, np.int64)
    ids, probs = np.full(2, -7, np.int64), np.full(2, -7.0)
    its, conv = np.full(5, -1, np.int64), np.full(5, -1, np.int32)
    cap, bad = C.c_int64(2), C.c_int64(-5)
    call(gi, v, off2, ids, probs, cap, its, conv, bad)        # too little room: offsets and counters only
    assert cap.value == total and bad.value == -1 and np.array_equal(off2, off)
    assert np.array_equal(its, want_its) and np.array_equal(conv.astype(bool), want_conv)
    assert (ids == -7).all() and (probs == -7.0).all()
    ids, probs = np.empty(total, np.int64), np.empty(total)
    cap = C.c_int64(total)
    call(gi, v, off2, ids, probs, cap, its, conv, bad)        # repeated with room: the rows
    assert cap.value == total and np.array_equal(ids, batch[1]) and probs.tobytes() == batch[2].tobytes()
    ids[:] = -7
    call(gi, v, off2, ids, probs, cap, None, None, None)      # counters and the position may be NULL
    assert np.array_equal(ids, batch[1])
    # the empty list
    e_off, e_ids, e_probs, e_its, e_conv = pool.recommend_batch([], [], ALPHA, 0.05, 1000)
    assert e_off.tolist() == [0] and len(e_ids) == len(e_probs) == len(e_its) == len(e_conv) == 0
    cap = C.c_int64(9)
    call(gi[:0], v[:0], off2, ids, probs, cap, its, conv, bad)
    assert cap.value == 0 and off2[0] == 0 and bad.value == -1
    # a graph index outside the pool, an unknown vertex: nothing is written but the position
    for bad_gi, bad_v, where, msg in (([0, 1, -1, 0, 1], v, 2, "names graph -1"), ([0, 1, 0, 2, 1], v, 3, "names graph 2"),
                                      (gi, [5, 41, 100, 1, 41], 2, "No such vertex in the graph: 100"),
                                      ([0, 1, 0, 0, 0], [5, 41, 3, 1, 41], 4, "No such vertex in the graph: 41"),
                                      ([0, 5, 0, 0, 1], [5, 41, 100, 1, 2], 1, "names graph 5")):
        off3 = np.full(6, -7, np.int64)
        ids, probs = np.full(64, -7, np.int64), np.full(64, -7.0)
        its, conv = np.full(5, -7, np.int64), np.full(5, -7, np.int32)
        cap, bad = C.c_int64(64), C.c_int64(-5)
        with pytest.raises(pkg.IllegalArgumentException, match=msg):
            call(np.array(bad_gi, np.int32), np.array(bad_v, np.int64), off3, ids, probs, cap, its, conv, bad)
        assert bad.value == where
        assert (off3 == -7).all() and (ids == -7).all() and (probs == -7.0).all() and (its == -7).all() and (conv == -7).all()
        assert cap.value == 64
        with pytest.raises(pkg.IllegalArgumentException, match=msg) as err:
            pool.recommend_batch(bad_gi, bad_v, ALPHA, 0.05, 1000)
        assert err.value.bad_request == where
    # the constructor's require()s
    with pytest.raises(pkg.IllegalArgumentException, match="epsilon must be non-negative"):
        pool.recommend_batch([0], [1], ALPHA, -0.1, 10)
    with pytest.raises(pkg.IllegalArgumentException, match="max iterations number must be non-negative"):
        pool.recommend_batch([0], [1], ALPHA, 0.1, -1)
    assert all(np.array_equal(a, b) for a, b in zip(pool.recommend_batch(gi, v, ALPHA, 0.05, 1000), batch))
    pool.close()
    # create's refusals
    h = C.c_void_p()
    assert L.lib().locrec_sg_pool_create(None, 1, C.byref(h)) == L.E_INVALID_ARG
    arr = (C.c_void_p * 2)(graphs[0]._h, None)
    assert L.lib().locrec_sg_pool_create(arr, 2, C.byref(h)) == L.E_INVALID_ARG and not h.value
    assert L.lib().locrec_sg_pool_create(arr, 0, C.byref(h)) == L.E_INVALID_ARG
    with pytest.raises(pkg.IllegalArgumentException, match="graph 2 appears twice"):
        pkg.SgPool([graphs[0], graphs[1], graphs[0]])
    for by_target in (False, True):
        sh = pkg.SgGraph(src, dst, w, shard_index=0, shard_count=2, by_target=by_target)
        with pytest.raises(pkg.IllegalArgumentException, match="graph 1: a sharded graph"):
            pkg.SgPool([graphs[0], sh])
        sh.close()
    for env, value, msg in (("LOCREC_SG_FUSED", "1", "graph 1: .*fused or persistent"), ("LOCREC_SG_GS", "4", "graph 1 .*LOCREC_SG_GS")):
        monkeypatch.setenv(env, value)
        odd = pkg.SgGraph(*edges_of(small))
        monkeypatch.delenv(env)
        with pytest.raises(pkg.IllegalArgumentException, match=msg):
            pkg.SgPool([graphs[1], odd])
        odd.close()
    for g in graphs:
        g.close()


def test_python_class_and_the_request_lines_of_the_main(pkg, tmp_path):
    """SgPool round trip, then mains.sg_recommender_requests on a sample written by the generator and builder mains (300
    persons, 300 places, as test_the_whole_walk_through): every good line equals sg_recommender_request's result, every
    bad line carries that function's exception, and pooled=False gives the same list."""
    import sample_cases as sc
    from locations_recommender_amd import mains
    D = sc.defaults()
    d = str(tmp_path)
    mains.sample_generator_main(d, 300, 300, D["regions"], D["categories"])
    sets = mains.stochastic_graph_builder_main(d, 400, 0.5, 0.5)
    assert (0,) in sets and (0, 1) in sets and (1, 2) in sets
    persons = mains.load_persons(d)
    # SgPool on two of the written graphs
    edges = [mains.load_stochastic_graph(mains.generate_file_name(rs, d, "stochastic_graph")) for rs in ([0], [0, 1], [1, 2])]
    vertices = [np.union1d(e[0], e[1]) for e in edges]
    graphs = [pkg.SgGraph(*e) for e in edges[:2]]
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(0, vertices[0][[0, 5, -1, 5]]), (1, vertices[1][[3, -2]])])
    check_pool_against_singles(pool, gi, v, 0.01, 20)
    assert set(pool.stats()) == set(pkg.SgPool.STATS)
    pool.close()
    for g in graphs:
        g.close()
    # a person of persons_sample whom the graph of the home region lacks (no visit joined a place there): found, not assumed
    home = persons["home_region_id"]
    lacking = np.setdiff1d(persons["id"][home == 0], vertices[0])
    assert len(lacking) > 0, "every person of region 0 is a vertex of its graph: choose fewer visits or days"
    absent = int(lacking[0])
    in0 = np.intersect1d(persons["id"][home == 0], vertices[1])   # persons of region 0 in the graphs of [0] and [0, 1]
    in0 = np.intersect1d(in0, vertices[0])
    in1 = np.intersect1d(persons["id"][home == 1], vertices[2])   # persons of region 1 in the graph of [1, 2]
    assert len(in0) >= 3 and len(in1) >= 2
    lines = [f"{in0[0]}", f"{in0[1]} 1", "x", f"{in1[0]} 2", f"{absent}", "5 1", f"{in0[0]}", f"{in0[2]}  0", f"{in1[1]} 2",
             f"{in0[0]} 1"]
    want = []
    for line in lines:
        try:
            want.append(mains.sg_recommender_request(d, persons, line, 0.01, 20, max_recommendations=7))
        except Exception as e:
            want.append(e)
    kinds = [type(x) for x in want if isinstance(x, Exception)]
    assert kinds == [pkg.IllegalArgumentException, pkg.IllegalArgumentException, mains.NoSuchElementException]
    assert str(want[2]).startswith("Failed to parse input") and str(want[4]) == f"No such vertex in the graph: {absent}"
    assert str(want[5]) == "Person not found: 5"
    assert len({tuple(sorted({x[0][1], x[0][2]})) for x in want if not isinstance(x, Exception)}) >= 3   # region sets
    assert any(len(x[1]) > 0 for x in want if not isinstance(x, Exception))
    for pooled in (True, False):
        got = mains.sg_recommender_requests(d, persons, lines, 0.01, 20, max_recommendations=7, pooled=pooled)
        assert len(got) == len(lines)
        for line, a, b in zip(lines, got, want):
            if isinstance(b, Exception):
                assert type(a) is type(b) and str(a) == str(b), (pooled, line)
            else:
                assert a[0] == b[0], (pooled, line)
                assert np.array_equal(a[1], b[1]) and sc.same_bits(np.asarray(a[2]), np.asarray(b[2])), (pooled, line)
    assert mains.sg_recommender_requests(d, persons, [], 0.01, 20) == []
