"""GPU: the ranked pool (locrec_sg_pool_recommend_ranked_batch, SgPool.recommend_ranked_batch,
mains.sg_recommender_requests_ranked): one mixed batch of (graph, vertex, target region) requests over a pool's resident
graphs, every member's tile emitted and ranked on the device.

Two expected values are used throughout, and every comparison is exact - ids, counts, probability bits, the iteration
counter and the converged flag (nothing is computed after the iteration, rows are only moved, and SG ids are unique per
request, so (probability desc, id asc) is a total order):
  (a) per member, SgGraph.recommend_ranked_batch on the same handle;
  (b) pool.recommend_batch's rows through mains.rank_recommendations_batch."""
import ctypes as C

import numpy as np
import pytest
import rank_batch_cases as rb
from test_gpu_sg_batch import d2_trajectory, kat, kat_edges, mixed_targets, same_bits
from test_gpu_sg_pool import edges_of, interleave
from test_gpu_sg_ranked import LIMITS, NOBODYS_REGION, PLACE0, main_requests, places_table, region_popcounts, same_all

pytestmark = pytest.mark.gpu
ALPHA = 0.15
TILE = 16
PARAMS = ((0.01, 20), (0.0, 3), (0.5, 1), (0.01, 0))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_against_members(pool, gi, v, t, eps, max_it, pl, reg, limit, got):
    """(a): every request of the pool call against SgGraph.recommend_ranked_batch on its member alone."""
    oi, op, cnt, its, conv = got
    for g in np.unique(gi):
        at = np.flatnonzero(gi == g)
        wi, wp, wc, wits, wconv = pool.graphs[g].recommend_ranked_batch(v[at], ALPHA, eps, max_it, pl, reg, t[at], limit)
        assert np.array_equal(cnt[at], wc) and np.array_equal(its[at], wits) and np.array_equal(conv[at], wconv), (g, eps, max_it)
        for j, i in enumerate(at):
            c = int(wc[j])
            assert np.array_equal(oi[i, :c], wi[j, :c]) and np.array_equal(bits(op[i, :c]), bits(wp[j, :c])), (g, i, eps, max_it)
            assert (oi[i, c:] == -1).all() and (op[i, c:] == 0.0).all()


def check_pool(mains, pool, gi, v, t, eps, max_it, pl, reg, limit, unranked=None):
    """The ranked pool call against (b) and (a).  -> (the call's result, the unranked call's offsets)."""
    off, ids, probs, its, conv = unranked if unranked is not None else pool.recommend_batch(gi, v, ALPHA, eps, max_it)
    want = (mains.rank_recommendations_batch(off, ids, probs, pl, reg, t, limit), its, conv, np.diff(off))
    got = pool.recommend_ranked_batch(gi, v, ALPHA, eps, max_it, pl, reg, t, limit)
    assert same_all(got, want), (eps, max_it, limit)
    assert np.array_equal(pool.row_counts, np.diff(off)), (eps, max_it, limit)
    check_against_members(pool, gi, v, t, eps, max_it, pl, reg, limit, got)
    return got, off


def member_tiles(gi, v, tile=TILE):
    return sum(-(-len(set(v[gi == g].tolist())) // tile) for g in np.unique(gi))


@pytest.fixture(scope="module")
def mixed(pkg):
    """Five members: the reference's test graph, three synthetic ones of different sizes whose ids overlap, and one nobody
    asks.  33 distinct targets (three tiles, the last partial) on the largest; the others drop out after the first wave."""
    from locations_recommender_amd import mains, synth
    data = [synth.sg_dataset(200, 30, 5, seed=79), synth.sg_dataset(500, 60, 20, seed=78),
            synth.sg_dataset(3_000, 300, 20, seed=77)]
    edges = [kat_edges(kat())] + [edges_of(g) for g in data] + [edges_of(data[0])]
    graphs = [pkg.SgGraph(*e) for e in edges]
    pool = pkg.SgPool(graphs)
    pl, reg = places_table()                     # ids 40 .. 339, 900000 .., category 3 and person 345 of the largest
    bv, bt, own = main_requests(pl, reg)         # one vertex with three regions, a place in its own region, nobody's region
    p1, p2 = int(data[0]["first_person"]), int(data[1]["first_person"])
    per_graph = [(0, [1, 1, 3, 5]), (1, [p1, 45, 2, p1 + 7, 45, p1, 3, 41]), (2, [p2, 45, 2, p2 + 9, 77]),
                 (3, bv.tolist())]
    per_region = [(0, [1, 1, 0, 2]), (1, [0, 1, 2, 0, 2, 1, 1, 0]), (2, [2, 0, 1, NOBODYS_REGION, 1]), (3, bt.tolist())]
    gi, v = interleave(per_graph)
    _, t = interleave(per_region)
    # (45, a place, and 2, a category, are asked of three members each - main_requests has both; (graph 0, vertex 1,
    # region 1) is repeated)
    keys = list(zip(gi.tolist(), v.tolist(), t.tolist()))
    assert len(set(keys)) < len(keys) and (0, 1, 1) in keys and keys.count((0, 1, 1)) == 2
    for shared in (45, 2):
        assert len({g for g, x in zip(gi.tolist(), v.tolist()) if x == shared}) >= 2
    assert len(np.unique(v[gi == 3])) == 33 and 45 in v[gi == 3] and 2 in v[gi == 3]      # two full tiles and a part
    # the emit rows: all different; the largest needs more than one emit block (256 rows), the smallest a fraction of a
    # wave.  With the source-only vertices (no sweep) no count is a multiple of 64; the live rows alone are no multiple of
    # 64 on the three small members, while the largest has 320 of them, five full waves (a multi-block member whose last
    # wave is partial is the 3,000-place member of test_stats_bound_the_read_back)
    live = [g.live_count() for g in graphs[:4]]
    nv = [g.info()["vertices"] for g in graphs[:4]]
    assert len(set(live)) == 4 and all(x % 64 for x in live[:3]) and all(x % 64 for x in nv)
    assert live[0] < 64 and nv[0] < 64 and live[3] > 256 and sorted(live) == live
    yield dict(mains=mains, data=data, edges=edges, graphs=graphs, pool=pool, gi=gi, v=v, t=t.astype(np.int64), pl=pl, reg=reg,
               own=own)
    pool.close()
    for g in graphs:
        g.close()


@pytest.mark.parametrize("eps,max_it", PARAMS)
def test_mixed_pool(mixed, eps, max_it):
    m = mixed
    pool, gi, v, t, pl, reg = m["pool"], m["gi"], m["v"], m["t"], m["pl"], m["reg"]
    got, off = check_pool(m["mains"], pool, gi, v, t, eps, max_it, pl, reg, 10)
    st = pool.ranked_stats()
    assert st["tile_waves"] == 3 and st["tiles"] == member_tiles(gi, v) == 6 and st["groups"] == 1 and st["emit_launches"] == 3
    cnt = got[2]
    assert (cnt == 10).any() and (cnt == 0).any() and not cnt[t == NOBODYS_REGION].any()
    if max_it == 0:   # the source-only vertices are emit rows and hold D's value: a person listed as a place can appear
        assert np.array_equal(pool.row_counts, np.array([pool.graphs[g].info()["vertices"] - 1 for g in gi]))
    # the place that is its own target, inside its own region: absent
    full = pool.recommend_ranked_batch(gi, v, ALPHA, eps, max_it, pl, reg, t, 2 ** 40)
    i = int(np.flatnonzero((gi == 3) & (v == m["own"]))[0])
    assert full[2][i] > 0 and m["own"] not in full[0][i, :full[2][i]].tolist()
    # the three positions of the repeated vertex: its own region each
    rep = np.flatnonzero((gi == 3) & (v == v[gi == 3][0]))
    assert len(rep) == 3 and len(set(t[rep].tolist())) == 3
    if max_it > 0:
        assert len({tuple(full[0][i, :5].tolist()) for i in rep}) == 3


def test_mixed_pool_limits(mixed):
    m = mixed
    pool, gi, v, t, pl, reg = m["pool"], m["gi"], m["v"], m["t"], m["pl"], m["reg"]
    unranked = pool.recommend_batch(gi, v, ALPHA, 0.01, 20)
    for limit in LIMITS:
        got, off = check_pool(m["mains"], pool, gi, v, t, 0.01, 20, pl, reg, limit, unranked)
        if limit > 0:
            assert got[0].shape[1] == min(limit, int(np.diff(off).max()))
            assert (got[2] == 0).any() and got[2].max() == min(limit, int(got[2].max()))
            if limit <= 10:
                assert (got[2] == limit).any()           # some request returns exactly N rows
            if limit >= 256:
                assert got[2].max() > 64
        else:
            assert got[0].shape == (len(v), 0) and not got[2].any()


def test_columns_of_one_tile_at_different_parities(pkg):
    """The two-cycle graph of test_graphs_and_columns_stop_at_different_rounds, ranked: the columns of one tile stop at
    sweep counts of both parities, so the emit reads both x buffers."""
    from locations_recommender_amd import mains
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
    graphs = [pkg.SgGraph(src, dst, w), pkg.SgGraph(*kat_edges(kat()))]
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(0, targets), (1, [1, 3, 5])])
    t = (np.arange(len(v)) % 3).astype(np.int64)
    pl = np.r_[np.arange(0, 30), 2000, 2001, 1, 3, 5, 1005].astype(np.int64)
    reg = (np.arange(len(pl)) % 3).astype(np.int64)
    got, _ = check_pool(mains, pool, gi, v, t, eps, 200, pl, reg, 10)
    first_tile = [int(got[3][np.flatnonzero((gi == 0) & (v == x))[0]]) for x in targets[:TILE]]
    assert len({x % 2 for x in first_tile}) == 2 and got[4].all(), first_tile
    assert got[2][gi == 0].max() > 0
    pool.close()
    for g in graphs:
        g.close()


def test_one_vertex_with_more_requests_than_a_tile_has_columns(mixed):
    """40 requests of one vertex on one member (one column, 40 segments) next to a member with a single request."""
    m = mixed
    pool, pl, reg = m["pool"], m["pl"], m["reg"]
    person = int(m["data"][2]["first_person"]) + 77
    gi = np.r_[np.full(40, 3), 1].astype(np.int32)
    v = np.r_[np.full(40, person), 45].astype(np.int64)
    t = np.r_[np.arange(40) % 4, 1].astype(np.int64)
    t[t == 3] = NOBODYS_REGION
    for max_it in (20, 0):
        got, _ = check_pool(m["mains"], pool, gi, v, t, 0.01, max_it, pl, reg, 10)
        assert got[2][:40][t[:40] != NOBODYS_REGION].min() == 10 and not got[2][t == NOBODYS_REGION].any()
        st = pool.ranked_stats()
        assert st["tile_waves"] == 1 and st["tiles"] == 2 and st["emit_launches"] == 1


def emit_plan(gi, v, caps, budget, tile=TILE):
    """The host's plan, restated: requests in emit order (tile wave, member, distinct target in order of appearance, input
    position) and the groups of that order within `budget` rows.  -> [(wave, member, group)] per emit position."""
    uniq = {}
    for i, (g, x) in enumerate(zip(gi.tolist(), v.tolist())):
        uniq.setdefault(g, {}).setdefault(x, []).append(i)
    order = []
    waves = max(-(-len(u) // tile) for u in uniq.values())
    for k in range(waves):
        for g in sorted(uniq):
            for x in list(uniq[g])[k * tile:(k + 1) * tile]:
                order += [(k, g, i) for i in uniq[g][x]]
    plan, group, rows, first = [], 0, 0, True
    for k, g, i in order:
        if not first and rows + caps[i] > budget:
            group, rows = group + 1, 0
        first = False
        rows += caps[i]
        plan.append((k, g, group))
    return plan


@pytest.mark.parametrize("budget", [1, 97, 1000])
def test_row_budget_does_not_change_the_result(mixed, monkeypatch, budget):
    m = mixed
    pool, gi, v, t, pl, reg = m["pool"], m["gi"], m["v"], m["t"], m["pl"], m["reg"]
    # the room of every request: its region's places among the LIVE vertices of its member (a sweep ran)
    caps = np.zeros(len(v), np.int64)
    for g in np.unique(gi):
        dst = m["edges"][g][1]
        caps[gi == g] = region_popcounts({"source_id": dst, "target_id": dst}, pl, reg, t[gi == g])
    plan = emit_plan(gi, v, caps, budget)
    n_groups = plan[-1][2] + 1
    by_budget = [emit_plan(gi, v, caps, b)[-1][2] + 1 for b in (1, 97, 1000)]
    assert len(v) >= by_budget[0] > by_budget[1] > by_budget[2] > 1       # groups rise as the budget falls
    assert by_budget[0] >= np.count_nonzero(caps)                         # (a request without room joins its neighbour's group)
    if budget == 97:
        by_group, by_tile = {}, {}
        for k, g, grp in plan:
            by_group.setdefault(grp, set()).add(g)
            by_tile.setdefault((k, g), set()).add(grp)
        assert any(len(x) > 1 for x in by_group.values()), "no group spans two members"
        assert any(len(x) > 1 for x in by_tile.values()), "no member's tile is split across two groups"
    for limit in (10, 300):
        base = pool.recommend_ranked_batch(gi, v, ALPHA, 0.01, 20, pl, reg, t, limit)
        assert pool.ranked_stats()["groups"] == 1 and base[2].max() > 0
        monkeypatch.setenv("LOCREC_SG_RANKED_ROW_BUDGET", str(budget))
        got = pool.recommend_ranked_batch(gi, v, ALPHA, 0.01, 20, pl, reg, t, limit)
        st = pool.ranked_stats()
        monkeypatch.delenv("LOCREC_SG_RANKED_ROW_BUDGET")
        assert rb.same(got[:3], base[:3]) and np.array_equal(got[3], base[3]) and np.array_equal(got[4], base[4])
        assert st["groups"] == n_groups and st["tiles"] == 6 and st["tile_waves"] == 3
        assert st["emit_launches"] == len({(k, grp) for k, _, grp in plan})   # one per tile wave and group part


COMMON_STATS = ("tiles", "groups", "emitted_rows", "readback_bytes", "host_syncs")
ONE_MEMBER_LIMITS = (0, 1, 10, 2 ** 40)


def one_member_world(pkg, which):
    """A graph, the pool of that graph alone and requests for it.  "synth": 17 distinct targets (two tiles, the second
    holds a single column), the first asked three times with three regions, one request for a region nobody is in.
    "kat": the reference's test graph has five vertices - all five, vertex 1 three times, one request for nobody's region.
    One places table serves both: the synthetic graph's places, and the KAT graph's vertices in three regions."""
    from locations_recommender_amd import synth
    if which == "kat":
        edges = kat_edges(kat())
        v = np.array([1, 2, 3, 4, 5, 1, 1], np.int64)
        t = np.array([0, 1, 2, NOBODYS_REGION, 1, 1, 2], np.int64)
    else:
        g = synth.sg_dataset(200, 30, 5, seed=79)
        edges = edges_of(g)
        p0 = int(g["first_person"])
        first = np.r_[p0 + np.array([0, 3, 11, 50, 51, 120, 199, 60, 61]), PLACE0 + np.array([0, 5, 6, 7, 29]), [0, 2, 4]]
        v = np.r_[first[:6], first[0], first[6:], first[0]].astype(np.int64)     # first[0] three times ...
        t = (np.arange(len(v)) % 3).astype(np.int64)
        t[[0, 6, len(v) - 1]] = [0, 1, 2]                                         # ... with regions 0, 1, 2
        t[3] = NOBODYS_REGION
        assert len(np.unique(v)) == TILE + 1 and len(v) == 19
    pl, reg = places_table(30)
    pl, reg = np.r_[pl, np.arange(1, 6)].astype(np.int64), np.r_[reg, [0, 1, 2, 0, 1]].astype(np.int64)
    sg = pkg.SgGraph(*edges)
    return dict(which=which, edges=edges, sg=sg, pool=pkg.SgPool([sg]), v=v, t=t, gi=np.zeros(len(v), np.int32), pl=pl, reg=reg)


def check_one_member(pkg, w, eps, max_it, monkeypatch, budgets=(None, 1, 97), limits=ONE_MEMBER_LIMITS):
    """A pool of one member and the ranked batch on that member, the same requests: equal results
    (check_against_members) and equal bookkeeping - the five counters both entries report.  Term by term: the caps
    (R * 8 = P * 8 bytes, one wait), 384 bytes and one wait per tile, 4 bytes and one wait per poll on the same schedule,
    the ranker's header and waits per group, the ranked rows per group, the (n + nu) * 8 bytes of the tail."""
    sg, pool, gi, v, t, pl, reg = w["sg"], w["pool"], w["gi"], w["v"], w["t"], w["pl"], w["reg"]
    src, dst = w["edges"][0], w["edges"][1]
    # the room of a request: its region's places among the emit rows - the live vertices, and every vertex when no sweep ran
    caps = region_popcounts({"source_id": src if max_it == 0 else dst, "target_id": dst}, pl, reg, t)
    assert caps.max() > 0 and not caps[t == NOBODYS_REGION].any()
    for budget in budgets:
        plan = emit_plan(gi, v, caps, 2 ** 62 if budget is None else budget)
        n_groups = plan[-1][2] + 1
        if budget is None:
            assert n_groups == 1
        if budget == 1:
            assert n_groups >= np.count_nonzero(caps) > 1       # a group per request with room
        if budget == 97 and w["which"] == "synth":              # groups of several requests; one ends inside the first tile
            assert 1 < n_groups < np.count_nonzero(caps) and len({grp for k, _, grp in plan if k == 0}) > 1
        for limit in limits:
            if budget is not None:
                monkeypatch.setenv("LOCREC_SG_RANKED_ROW_BUDGET", str(budget))
            got = pool.recommend_ranked_batch(gi, v, ALPHA, eps, max_it, pl, reg, t, limit)
            pst = pool.ranked_stats()
            check_against_members(pool, gi, v, t, eps, max_it, pl, reg, limit, got)   # (the member's call: the same requests)
            sst = pkg.SgGraph.ranked_batch_stats()
            if budget is not None:
                monkeypatch.delenv("LOCREC_SG_RANKED_ROW_BUDGET")
            case = (eps, max_it, budget, limit)
            assert {k: pst[k] for k in COMMON_STATS} == sst, (case, pst, sst)
            assert pst["groups"] == sst["groups"] == n_groups, case
            assert pst["tiles"] == member_tiles(gi, v) == pst["tile_waves"], case
            if limit == 0:
                assert got[0].shape == (len(v), 0) and not got[2].any()
            else:
                assert got[2].max() > 0 and not got[2][t == NOBODYS_REGION].any()


@pytest.fixture(scope="module", params=["kat", "synth"])
def one_member(pkg, request):
    w = one_member_world(pkg, request.param)
    yield w
    w["pool"].close()
    w["sg"].close()


@pytest.mark.parametrize("eps,max_it", [(0.01, 20), (0.01, 0)])
def test_one_member_pool_keeps_the_ranked_batch_s_books(pkg, one_member, monkeypatch, eps, max_it):
    """The two entries share one host scaffold: for a pool of exactly one member the pool call and the ranked batch on
    the member agree in tiles, groups, emitted_rows, readback_bytes and host_syncs, under every row budget (one group, a
    group per request, groups that end inside a tile) and every limit, with (max_it = 0) and without the source-only
    rows."""
    check_one_member(pkg, one_member, eps, max_it, monkeypatch)


def test_one_member_pool_keeps_the_books_with_plain_copy_states(pkg, monkeypatch):
    """The same with the member (and so the pool) created under LOCREC_SG_NO_PACK, which is read when a graph is
    created: both entries read their states back through a device buffer and a plain copy."""
    monkeypatch.setenv("LOCREC_SG_NO_PACK", "1")
    w = one_member_world(pkg, "synth")
    monkeypatch.delenv("LOCREC_SG_NO_PACK")
    try:
        check_one_member(pkg, w, 0.01, 20, monkeypatch, limits=(10,))
    finally:
        w["pool"].close()
        w["sg"].close()


def test_layout_classes_share_a_ranked_pool(pkg, monkeypatch):
    """uint16 / int32 columns x dictionary / fp64 weights in one pool (the pool of test_layout_classes_share_a_pool)."""
    from locations_recommender_amd import mains, synth
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
    t = (np.arange(len(v)) % 3).astype(np.int64)
    pl, reg = places_table(200)
    pl, reg = np.r_[pl, np.arange(0, 40, 3)], np.r_[reg, np.arange(0, 40, 3) % 3]   # the third member's live vertices
    for eps, max_it in ((0.01, 20), (0.0, 12), (0.01, 0)):
        got, _ = check_pool(mains, pool, gi, v, t, eps, max_it, pl, reg, 10)
        assert got[2].max() == 10 and got[2][gi == 2].max() > 0
    pool.close()
    for h in graphs:
        h.close()


def test_plain_copy_states(pkg, monkeypatch):
    """A member created under LOCREC_SG_NO_PACK: polls and states of the whole pool go through plain copies."""
    from locations_recommender_amd import mains, synth
    data = [synth.sg_dataset(500, 60, 20, seed=78), synth.sg_dataset(200, 30, 5, seed=79)]
    monkeypatch.setenv("LOCREC_SG_NO_PACK", "1")
    graphs = [pkg.SgGraph(*edges_of(data[0]))]
    monkeypatch.delenv("LOCREC_SG_NO_PACK")
    graphs.append(pkg.SgGraph(*edges_of(data[1])))
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(0, (int(data[0]["first_person"]) + np.arange(0, 40, 2)).tolist() + [44, 3]),
                        (1, [int(data[1]["first_person"]), 41, 2])])
    t = (np.arange(len(v)) % 3).astype(np.int64)
    pl, reg = places_table(60)
    for eps, max_it in ((0.01, 20), (0.0, 7), (0.01, 0)):
        got, _ = check_pool(mains, pool, gi, v, t, eps, max_it, pl, reg, 10)
        assert pool.ranked_stats()["tile_waves"] == 2 and got[2].max() == 10
    pool.close()
    for g in graphs:
        g.close()


def test_few_private_rows(pkg):
    """T = 65,530 with uint16 columns (test_few_private_rows): tiles of five on that member, three waves, beside a small
    member; ranked against a places table over the large member's live ids."""
    from locations_recommender_amd import mains, synth
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
    t = (np.arange(len(v)) % 3).astype(np.int64)
    pl = np.r_[np.arange(0, T, 7), T - 1].astype(np.int64)
    reg = (pl % 3).astype(np.int64)
    got, _ = check_pool(mains, pool, gi, v, t, 0.01, 20, pl, reg, 10)
    st = pool.ranked_stats()
    assert st["tile_waves"] == 3 and st["tiles"] == 4 and got[2][gi == 0].max() == 10
    pool.close()
    for g in graphs:
        g.close()


def test_launches_are_shared(pkg):
    """Twelve graphs' tiles are ONE emit launch, ONE group and ten shared rounds."""
    from locations_recommender_amd import mains, synth
    data = [synth.sg_dataset(400, 50, 8, seed=100 + i) for i in range(12)]
    graphs = [pkg.SgGraph(*edges_of(g)) for g in data]
    pool = pkg.SgPool(graphs)
    gi, v = interleave([(i, [int(g["first_person"]) + 3, 41]) for i, g in enumerate(data)])
    t = (np.arange(len(v)) % 3).astype(np.int64)
    pl, reg = places_table(50)
    check_pool(mains, pool, gi, v, t, 0.0, 10, pl, reg, 10)
    st = pool.ranked_stats()
    assert st == dict(st, tile_waves=1, tiles=12, rounds=10, groups=1, emit_launches=1)
    assert st["emitted_rows"] > 0 and st["host_syncs"] > 0
    pool.close()
    for g in graphs:
        g.close()


@pytest.mark.parametrize("big_places", [300, 3_000])
def test_stats_bound_the_read_back(pkg, mixed, big_places):
    """readback_bytes <= member tiles * 8192 + n * (16 * N + 64), whatever T is (the ranked batch's own bound,
    test_stats_bound_the_read_back, summed over members: per tile the 384-byte state and the polls - a poll is shared by
    a wave here -, per request the ranked rows, the count, the cap, the segment length and the column count), and below
    what the unranked pool call reads back for the same requests."""
    from locations_recommender_amd import synth
    m = mixed
    if big_places == 300:
        pool, graphs, edges, gi, v, t, pl, reg = m["pool"], None, m["edges"], m["gi"], m["v"], m["t"], m["pl"], m["reg"]
    else:
        g = synth.sg_dataset(n_persons=1_200, n_places=big_places, n_categories=20, seed=8)
        edges = m["edges"][:3] + [edges_of(g)]
        graphs = [pkg.SgGraph(*edges[3])]
        pool = pkg.SgPool(m["graphs"][:3] + graphs)
        pl, reg = places_table(big_places)
        person0 = int(g["first_person"])
        bv = np.r_[person0 + np.arange(0, 1200, 40), PLACE0 + np.arange(0, 3000, 500)].astype(np.int64)
        keep = m["gi"] < 3
        gi, v = np.r_[m["gi"][keep], np.full(len(bv), 3)].astype(np.int32), np.r_[m["v"][keep], bv].astype(np.int64)
        t = np.r_[m["t"][keep], np.arange(len(bv)) % 3].astype(np.int64)
        assert graphs[0].live_count() > 0.9 * big_places
    stride = 10
    for eps, max_it in ((0.01, 20), (1e-9, 200), (0.01, 0)):
        got, _ = check_pool(m["mains"], pool, gi, v, t, eps, max_it, pl, reg, stride)
        unranked_bytes = pool.stats()["readback_bytes"]     # (check_pool made the unranked call for these requests)
        st = pool.ranked_stats()
        tiles = member_tiles(gi, v)
        popcounts = sum(int(region_popcounts({"source_id": edges[g][0], "target_id": edges[g][1]}, pl, reg, t[gi == g]).sum())
                        for g in np.unique(gi))
        assert st["tiles"] == tiles and st["groups"] == 1 and st["host_syncs"] > 0 and got[2].max() == stride
        assert 0 < st["emitted_rows"] <= popcounts
        assert 0 < st["readback_bytes"] <= tiles * 8192 + len(v) * (16 * stride + 64), st
        assert st["readback_bytes"] < unranked_bytes
    if graphs:
        pool.close()
        graphs[0].close()


def test_handle_state_around_a_ranked_pool_call(pkg):
    """Single requests, per-graph batches and a group run give a fresh handle's bits before and after a ranked pool call
    (members_are_fresh of test_handle_state_around_a_pool_call); an unranked and a ranked call interleaved on the same
    pool each give their own first results again."""
    from locations_recommender_amd import mains, synth
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
    t = (np.arange(len(v)) % 3).astype(np.int64)
    pl, reg = places_table(60)
    ranked, _ = check_pool(mains, pool, gi, v, t, 0.01, 20, pl, reg, 10)
    members_are_fresh()
    unranked = pool.recommend_batch(gi, v, ALPHA, 0.01, 20)
    for _ in range(2):
        again = pool.recommend_ranked_batch(gi, v, ALPHA, 0.01, 20, pl, reg, t, 10)
        assert rb.same(again[:3], ranked[:3]) and np.array_equal(again[3], ranked[3]) and np.array_equal(again[4], ranked[4])
        again = pool.recommend_batch(gi, v, ALPHA, 0.01, 20)
        assert all(np.array_equal(a, b) for a, b in zip(again, unranked)) and again[2].tobytes() == unranked[2].tobytes()
    members_are_fresh()
    pool.close()
    grp.close()
    for h in graphs:
        h.close()


def test_refusals_and_the_empty_list(pkg):
    from locations_recommender_amd import _lib as L
    from locations_recommender_amd import synth
    src, dst, w = kat_edges(kat())
    small = synth.sg_dataset(200, 30, 5, seed=79)
    graphs = [pkg.SgGraph(src, dst, w), pkg.SgGraph(*edges_of(small))]
    pool = pkg.SgPool(graphs)
    gi = np.array([0, 1, 0, 0, 1], np.int32)
    v = np.array([5, 41, 3, 1, int(small["first_person"])], np.int64)
    t = np.array([0, 1, 2, 0, 1], np.int64)
    pl, reg = places_table(30)
    base = pool.recommend_ranked_batch(gi, v, ALPHA, 0.05, 1000, pl, reg, t, 10)
    assert base[2].max() > 0

    def call(gi, v, outs, bad, eps=0.05, max_it=1000, n_places=None, places=pl, regions=reg, targets=t, n=None):
        oi, op, cnt, rows, its, conv = outs
        return L.lib().locrec_sg_pool_recommend_ranked_batch(
            pool._h, len(v) if n is None else n, None if gi is None else L.ptr(gi, C.c_int32),
            None if v is None else L.ptr(v, C.c_int64), ALPHA, eps, max_it,
            len(pl) if n_places is None else n_places, None if places is None else L.ptr(places, C.c_int64),
            None if regions is None else L.ptr(regions, C.c_int64), None if targets is None else L.ptr(targets, C.c_int64), 10,
            L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64), L.ptr(its, C.c_int64),
            L.ptr(conv, C.c_int32), C.byref(bad) if bad is not None else None)

    def sentinels():
        return (np.full(50, -7, np.int64), np.full(50, -7.0), np.full(5, -7, np.int64), np.full(5, -7, np.int64),
                np.full(5, -7, np.int64), np.full(5, -7, np.int32))

    def untouched(outs):
        return all((o == -7).all() for o in outs)

    # the pool's cases: nothing is written but the position
    for bad_gi, bad_v, where, msg in (([0, 1, -1, 0, 1], v, 2, "names graph -1"), ([0, 1, 0, 2, 1], v, 3, "names graph 2"),
                                      (gi, [5, 41, 100, 1, 41], 2, "No such vertex in the graph: 100"),
                                      ([0, 1, 0, 0, 0], [5, 41, 3, 1, 41], 4, "No such vertex in the graph: 41"),
                                      ([0, 5, 0, 0, 1], [5, 41, 100, 1, 2], 1, "names graph 5")):
        outs, bad = sentinels(), C.c_int64(-5)
        status = call(np.array(bad_gi, np.int32), np.array(bad_v, np.int64), outs, bad)
        assert status in (L.E_INVALID_ARG, L.E_NOT_FOUND) and msg.encode() in L.lib().locrec_last_error()
        assert bad.value == where and untouched(outs)
        with pytest.raises(pkg.IllegalArgumentException, match=msg) as err:
            pool.recommend_ranked_batch(bad_gi, bad_v, ALPHA, 0.05, 1000, pl, reg, t, 10)
        assert err.value.bad_request == where
        with pytest.raises(pkg.IllegalArgumentException, match=msg) as err:     # the unranked call: the same message and position
            pool.recommend_batch(bad_gi, bad_v, ALPHA, 0.05, 1000)
        assert err.value.bad_request == where
    for eps, max_it, msg in ((-0.1, 10, "epsilon must be non-negative"), (0.1, -1, "max iterations number must be non-negative")):
        outs, bad = sentinels(), C.c_int64(-5)
        assert call(gi, v, outs, bad, eps=eps, max_it=max_it) == L.E_INVALID_ARG and msg.encode() in L.lib().locrec_last_error()
        assert untouched(outs) and bad.value == -5
        with pytest.raises(pkg.IllegalArgumentException, match=msg):
            pool.recommend_ranked_batch([0], [1], ALPHA, eps, max_it, pl, reg, [0], 10)
    # the ranked batch's cases
    for kwargs, msg in ((dict(targets=None), "null array"), (dict(places=None), "null array"), (dict(regions=None), "null array"),
                        (dict(n_places=-1), "out of range"), (dict(n_places=2 ** 31), "out of range")):
        outs, bad = sentinels(), C.c_int64(-5)
        assert call(gi, v, outs, bad, **kwargs) == L.E_INVALID_ARG and msg.encode() in L.lib().locrec_last_error(), kwargs
        assert untouched(outs) and bad.value == -5
    outs, bad = sentinels(), C.c_int64(-5)
    assert call(None, None, outs, bad, n=5) == L.E_INVALID_ARG and untouched(outs) and bad.value == -5
    # the empty list
    outs, bad = sentinels(), C.c_int64(-5)
    assert call(gi[:0], v[:0], outs, bad, targets=t[:0]) == L.OK and untouched(outs) and bad.value == -1
    none = np.empty(0, np.int64)
    oi, op, cnt, its, conv = pool.recommend_ranked_batch([], [], ALPHA, 0.05, 1000, pl, reg, none, 10)
    assert oi.shape == (0, 0) and len(cnt) == len(its) == len(conv) == 0
    # no places at all: the iteration still runs, every count is 0; the position and the counters may be NULL
    oi, op, cnt, its, conv = pool.recommend_ranked_batch(gi, v, ALPHA, 0.05, 1000, none, none, t, 10)
    assert not cnt.any() and np.array_equal(its, base[3]) and np.array_equal(conv, base[4])
    oi, op, cnt = np.full(50, -7, np.int64), np.full(50, -7.0), np.full(5, -7, np.int64)
    L.check(L.lib().locrec_sg_pool_recommend_ranked_batch(
        pool._h, 5, L.ptr(gi, C.c_int32), L.ptr(v, C.c_int64), ALPHA, 0.05, 1000, len(pl), L.ptr(pl, C.c_int64),
        L.ptr(reg, C.c_int64), L.ptr(t, C.c_int64), 10, L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64),
        None, None, None, None))
    w = base[0].shape[1]
    assert np.array_equal(cnt, base[2]) and np.array_equal(oi.reshape(5, 10)[:, :w], base[0])
    again = pool.recommend_ranked_batch(gi, v, ALPHA, 0.05, 1000, pl, reg, t, 10)
    assert rb.same(again[:3], base[:3])
    pool.close()
    for g in graphs:
        g.close()


def test_the_request_lines_of_the_main(pkg, tmp_path):
    """mains.sg_recommender_requests_ranked on the walk-through sample of
    test_python_class_and_the_request_lines_of_the_main (300 persons, 300 places, the same ten lines with the three bad
    ones): every good line equals sg_recommender_request's result, every bad line carries that function's exception."""
    import sample_cases as sc
    from locations_recommender_amd import mains
    D = sc.defaults()
    d = str(tmp_path)
    mains.sample_generator_main(d, 300, 300, D["regions"], D["categories"])
    sets = mains.stochastic_graph_builder_main(d, 400, 0.5, 0.5)
    assert (0,) in sets and (0, 1) in sets and (1, 2) in sets
    persons = mains.load_persons(d)
    edges = [mains.load_stochastic_graph(mains.generate_file_name(rs, d, "stochastic_graph")) for rs in ([0], [0, 1], [1, 2])]
    vertices = [np.union1d(e[0], e[1]) for e in edges]
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
    assert any(len(x[1]) > 0 for x in want if not isinstance(x, Exception))
    got = mains.sg_recommender_requests_ranked(d, persons, lines, 0.01, 20, max_recommendations=7)
    assert len(got) == len(lines)
    for line, a, b in zip(lines, got, want):
        if isinstance(b, Exception):
            assert type(a) is type(b) and str(a) == str(b), line
        else:
            assert a[0] == b[0], line
            assert np.array_equal(a[1], b[1]) and sc.same_bits(np.asarray(a[2]), np.asarray(b[2])), line
    assert mains.sg_recommender_requests_ranked(d, persons, [], 0.01, 20) == []
