"""GPU: one mixed batch of visitors over a pool of indexes (locrec_knn_pool_visitors_*, KnnPool.visitors_*) against each
member's own visitors calls.  Visitor i of a pool call must equal, bit for bit, what KnnIndex.visitors_recommend_batch /
visitors_recommend_ranked_batch returns for that vector on its member alone (that member's visitors in call order); a subset
is also compared with the oracle on the member's data PLUS the visitor, at the KNN tests' tolerance.  Members and visitors:
tests/knn_pool_visitor_cases.py."""
import ctypes as C

import numpy as np
import pytest

import knn_pool_visitor_cases as pc
import knn_visitor_cases as vc

pytestmark = pytest.mark.gpu
PW, CW = pc.PW, pc.CW
RTOL = 1e-6                   # tests/test_gpu_knn.py
LIMITS = (10, 257)            # the LDS lists; beyond LOCREC_RANK_BATCH_MAX_N


def make_index(pkg, d):
    return pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"], d["c_val"],
                        d["c_dim"], d.get("r_rowptr"), d.get("r_place"), d.get("r_rating"))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def on_device(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.fixture(scope="module")
def members(pkg):
    ds = pc.members()
    ixs = [make_index(pkg, d) for d in ds]
    pool = pkg.KnnPool(ixs)
    yield ds, ixs, pool
    pool.close()
    for ix in ixs:
        ix.close()


_alone = {}


def alone(ixs, k):
    """Every asked member's own visitors_recommend_batch on its visitors in call order, once per K: {visitor: (places, ratings)}."""
    if k not in _alone:
        rows = {}
        for m in sorted(pc.ASKED):
            at, sub = pc.of_member(m)
            off, p, e = ixs[m].visitors_recommend_batch(*sub, PW, CW, k)
            for j, i in enumerate(at):
                rows[int(i)] = (p[off[j]:off[j + 1]].copy(), e[off[j]:off[j + 1]].copy())
        _alone[k] = rows
    return _alone[k]


def ways(ds, k):
    return {m: pc.way(k, len(ds[m]["person_ids"])) for m in sorted(pc.ASKED)}


@pytest.mark.parametrize("k", pc.KS)
def test_rows_equal_each_members_own_visitors_call(pkg, members, k):
    ds, ixs, pool = members
    gi, vs, names = pc.visitors()
    want = alone(ixs, k)
    off, p, e = pool.visitors_recommend_batch(gi, *pc.arrays(), PW, CW, k)
    st = pool.visitors_stats()
    assert len(off) == len(gi) + 1 and off[0] == 0 and off[-1] == len(p) == len(e) > 0
    for i in range(len(gi)):
        wp, we = want[i]
        assert np.array_equal(p[off[i]:off[i + 1]], wp), (k, i, gi[i])
        assert np.array_equal(bits(e[off[i]:off[i + 1]]), bits(we)), (k, i, gi[i])
    for m in (4, 6):                                                   # nobody rated anything; nobody to be similar to
        at = np.flatnonzero(gi == m)
        assert np.all(off[at] == off[at + 1])
    a, b = names["twice"]                                              # computed twice, the same rows
    assert off[a + 1] > off[a] and np.array_equal(p[off[a]:off[a + 1]], p[off[b]:off[b + 1]])
    assert np.array_equal(bits(e[off[a]:off[a + 1]]), bits(e[off[b]:off[b + 1]]))
    assert off[names["long"] + 1] > off[names["long"]]
    w = ways(ds, k)
    assert st["delegated_members"] == sum(1 for x in w.values() if x == "delegated")
    assert st["stage_launches"] == 1 and st["beyond"] == pc.beyond_entries() > 0
    live = [m for m, x in w.items() if x == "shared" and pc.rated_places(ds[m]) > 0]
    waves = max([-(-pc.ASKED[m] // pc.QT) for m in live], default=0)
    assert st["waves"] == waves and st["member_tiles"] == sum(-(-pc.ASKED[m] // pc.QT) for m in live)
    assert (st["fill_launches"], st["scan_launches"], st["aggregate_launches"], st["finish_launches"]) == (2 * waves, waves, waves, 3 * waves)
    assert st["emitted_rows"] == sum(len(want[i][0]) for i in range(len(gi)) if gi[i] in live)
    # CUDA tensors: the same bytes
    doff, dp, de = pool.visitors_recommend_batch(gi, *on_device(pc.arrays()), PW, CW, k)
    assert np.array_equal(doff, off) and np.array_equal(dp, p) and np.array_equal(bits(de), bits(e))


def test_stats_of_the_shared_launches(pkg, members):
    """K = 2,000,000: every member with persons shares.  Members 0 - 3 are live (member 4 has no rated place, member 6 no
    persons): 1 + 1 + 3 + 1 tiles in 3 waves, seven launches a wave and ONE stage launch, whatever the number of members."""
    ds, ixs, pool = members
    gi, vs, names = pc.visitors()
    pool.visitors_recommend_batch(gi, *pc.arrays(), PW, CW, 2_000_000)
    st = pool.visitors_stats()
    assert st["waves"] == 3 and st["member_tiles"] == 1 + 1 + 3 + 1
    assert st["stage_launches"] == 1 and st["fill_launches"] == 6 and st["scan_launches"] == 3
    assert st["aggregate_launches"] == 3 and st["finish_launches"] == 9 and st["delegated_members"] == 0
    assert st["beyond"] > 0 and st["emitted_rows"] > 0 and st["readback_bytes"] > 0
    # the stage's wait, one per wave, the end of the launches, the rows' copy (and a growth of the row buffer with rows to keep: waves 1 and 2 at most)
    assert 3 + st["waves"] <= st["host_syncs"] <= 3 + st["waves"] + 2
    # at least one asked member renumbers its place dimensions and one does not: read from a single-member visitors call
    renumbered = {}
    for m in (0, 1, 2, 3):
        at, sub = pc.of_member(m)
        ixs[m].visitors_recommend_batch(*sub, PW, CW, 2_000_000)
        renumbered[m] = pkg.KnnIndex.visitors_stats()["renumbered"]
    assert renumbered[1] == 0 and renumbered[0] == 1 and set(renumbered.values()) == {0, 1}


@pytest.mark.parametrize("k", pc.KS)
def test_ranked_equals_each_members_own_ranked_visitors_call(pkg, members, k):
    ds, ixs, pool = members
    gi, vs, names = pc.visitors()
    places, regions = pc.places_table()
    targets = pc.targets(k)
    ex_off, ex_ids = pc.exclusion_lists()
    for limit in LIMITS:
        for exclude in (None, (ex_off, ex_ids)):
            oi, osc, cnt = pool.visitors_recommend_ranked_batch(gi, *pc.arrays(), PW, CW, k, places, regions, targets, limit,
                                                                exclude=exclude)
            st = pool.visitors_stats()
            assert oi.shape == (len(gi), min(limit, len(places)))
            for m in sorted(pc.ASKED):
                at, sub = pc.of_member(m)
                ex = None
                if exclude is not None:
                    lens = np.diff(ex_off)[at]
                    ex = (np.r_[0, np.cumsum(lens)].astype(np.int64),
                          np.concatenate([ex_ids[ex_off[i]:ex_off[i + 1]] for i in at]))
                wi, ws, wc = ixs[m].visitors_recommend_ranked_batch(*sub, PW, CW, k, places, regions, targets[at], limit, exclude=ex)
                assert np.array_equal(oi[at], wi) and np.array_equal(cnt[at], wc), (k, limit, m, exclude is not None)
                assert np.array_equal(bits(osc[at]), bits(ws)), (k, limit, m)
            assert np.all(cnt[targets == 99] == 0) and cnt.max() > 0
            if exclude is not None:
                for i in range(len(gi)):
                    assert not np.isin(oi[i, :cnt[i]], ex_ids[ex_off[i]:ex_off[i + 1]]).any(), i
            if k == 2_000_000:
                assert st["waves"] == 3 and st["delegated_members"] == 0 and st["stage_launches"] == 1
    # CUDA tensors: the same bytes
    di, dsc, dcnt = pool.visitors_recommend_ranked_batch(gi, *on_device(pc.arrays()), PW, CW, k, places, regions, targets, LIMITS[1],
                                                         exclude=(ex_off, ex_ids))
    assert np.array_equal(di, oi) and np.array_equal(dcnt, cnt) and np.array_equal(bits(dsc), bits(osc))


@pytest.mark.parametrize("k", (2_000_000, 50))
def test_a_subset_against_the_oracle_on_the_index_plus_the_visitor(pkg, oracle, members, k):
    ds, ixs, pool = members
    gi, vs, names = pc.visitors()
    # three visitors each of members 0, 1 and 2: in one small pool call (members 0 and 1 have two visitors in the big one)
    picked = {0: [vs[i] for i in np.flatnonzero(gi == 0)] + [vc.with_beyond(vc.row_of(ds[5], 3), 300, 20, 4)],
              1: [vs[i] for i in np.flatnonzero(gi == 1)] + [vc.with_beyond(vc.row_of(ds[1], 9), 700, 20, 5)],
              2: [vs[i] for i in np.flatnonzero(gi == 2)[[0, 16, 36]]]}
    sub_gi = np.array([2, 0, 1, 1, 2, 0, 0, 2, 1], np.int32)
    taken = {m: iter(v) for m, v in picked.items()}
    sub_vs = [next(taken[int(m)]) for m in sub_gi]
    off, p, e = pool.visitors_recommend_batch(sub_gi, *vc.csr(sub_vs), PW, CW, k)
    total = 0
    for i, (m, v) in enumerate(zip(sub_gi, sub_vs)):
        op, oe = vc.oracle_recommend(ds[m], v, PW, CW, k)
        assert off[i + 1] - off[i] == len(op), (k, i, m)
        assert np.array_equal(p[off[i]:off[i + 1]], op), (k, i, m)
        np.testing.assert_allclose(e[off[i]:off[i + 1]], oe, rtol=RTOL, atol=0)
        total += len(op)
    assert total > 0


def raw_rows(pool, gi, arrays, pw, cw, k, room):
    """locrec_knn_pool_visitors_recommend_batch on sentinel-filled outputs -> (status, offsets, places, ratings, capacity, bad)."""
    from locations_recommender_amd import _lib as L
    nv, g, ptrs, mem, keep = pool._visitor_pool_args(gi, *arrays)
    off = np.full(nv + 1, -7, np.int64)
    places, est = np.full(max(room, 1), -7, np.int64), np.full(max(room, 1), -7.0)
    cap, bad = C.c_int64(room), C.c_int64(-9)
    st = L.lib().locrec_knn_pool_visitors_recommend_batch(pool._h, nv, L.ptr(g, C.c_int32), *ptrs, mem, pw, cw, k, L.ptr(off, C.c_int64),
                                                          L.ptr(places, C.c_int64), L.ptr(est, C.c_double), C.byref(cap), C.byref(bad))
    return st, off, places, est, cap.value, bad.value


def raw_ranked(pool, gi, arrays, k, places, regions, targets, limit, ex_off, ex_ids):
    from locations_recommender_amd import _lib as L
    nv, g, ptrs, mem, keep = pool._visitor_pool_args(gi, *arrays)
    pl, reg, tgt = L.as_i64(places), L.as_i64(regions), L.as_i64(targets)
    eo, ei = (None if ex_off is None else L.as_i64(ex_off)), (None if ex_ids is None else L.as_i64(ex_ids))
    oi, osc, cnt = np.full((nv, limit), -7, np.int64), np.full((nv, limit), -7.0), np.full(nv, -7, np.int64)
    bad = C.c_int64(-9)
    st = L.lib().locrec_knn_pool_visitors_recommend_ranked_batch(
        pool._h, nv, L.ptr(g, C.c_int32), *ptrs, mem, PW, CW, k, len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64),
        L.ptr(tgt, C.c_int64), limit, L.ptr(eo, C.c_int64), L.ptr(ei, C.c_int64), L.ptr(oi, C.c_int64), L.ptr(osc, C.c_double),
        L.ptr(cnt, C.c_int64), C.byref(bad))
    return st, oi, osc, cnt, bad.value


def but(v, **kw):
    return dict(v, **{k: np.asarray(x, v[k].dtype) for k, x in kw.items()})


def test_capacity_protocol_and_refusals(pkg, members):
    from locations_recommender_amd import _lib as L
    ds, ixs, pool = members
    gi, vs, names = pc.visitors()
    k = 2_000_000
    want_off, want_p, want_e = pool.visitors_recommend_batch(gi, *pc.arrays(), PW, CW, k)
    total = int(want_off[-1])
    st, off, p, e, cap, bad = raw_rows(pool, gi, pc.arrays(), PW, CW, k, total - 1)     # too little room: sizes only
    assert st == L.OK and cap == total and bad == -1 and np.array_equal(off, want_off)
    assert np.all(p == -7) and np.all(e == -7.0)
    st, off, p, e, cap, bad = raw_rows(pool, gi, pc.arrays(), PW, CW, k, total + 3)     # enough room
    assert st == L.OK and cap == total and np.array_equal(off, want_off)
    assert np.array_equal(p[:total], want_p) and np.array_equal(bits(e[:total]), bits(want_e)) and np.all(p[total:] == -7)
    st, off, p, e, cap, bad = raw_rows(pool, [], vc.csr([]), PW, CW, k, 5)              # nobody
    assert st == L.OK and off[0] == 0 and cap == 0 and bad == -1
    o, pp, ee = pool.visitors_recommend_batch([], *vc.csr([]), PW, CW, k)
    assert o.tolist() == [0] and len(pp) == 0 and len(ee) == 0
    oi, osc, oc = pool.visitors_recommend_ranked_batch([], *vc.csr([]), PW, CW, k, [1, 2], [0, 0], [], 5)
    assert oi.shape == (0, 2) and len(oc) == 0

    def refused(gi_, vs_, pw, cw, kk, status, message, where):
        st, off, p, e, cap, bad = raw_rows(pool, gi_, vc.csr(vs_), pw, cw, kk, 64)
        assert st == status and message in L.lib().locrec_last_error().decode(), (message, L.lib().locrec_last_error())
        assert bad == where
        assert np.all(off == -7) and np.all(p == -7) and np.all(e == -7.0) and cap == 64   # nothing else is written

    # twelve good visitors: members 2 2 2 1 2 2 2 2 2 0 2 2
    two, one, zero = [vs[i] for i in np.flatnonzero(gi == 2)], vs[np.flatnonzero(gi == 1)[1]], vs[names["all_beyond"]]
    g12 = np.array([2, 2, 2, 1, 2, 2, 2, 2, 2, 0, 2, 2], np.int32)
    v12 = two[:3] + [one] + two[3:8] + [zero] + two[8:10]
    st, off, p, e, cap, bad = raw_rows(pool, g12, vc.csr(v12), PW, CW, k, 1 << 20)
    assert st == L.OK and bad == -1 and off[-1] > 0
    for kk in (k, 50):
        # an index position out of range (index positions come before the requires and the vectors)
        g = g12.copy()
        g[4] = len(ixs)
        bad_vs = list(v12)
        bad_vs[2] = but(v12[2], p_val=np.full(len(v12[2]["p_val"]), np.nan))
        refused(g, bad_vs, PW, CW, kk, L.E_INVALID_ARG, f"visitor 4 names index {len(ixs)} of a pool of {len(ixs)}", 4)
        g[4] = -1
        refused(g, bad_vs, 0.0, CW, kk, L.E_INVALID_ARG, "visitor 4 names index -1", 4)
        refused(g12, bad_vs, 0.0, CW, kk, L.E_INVALID_ARG, "Place weight must be in the interval (0; 1)", -1)   # then the requires
        refused(g12, bad_vs, PW, CW, kk, L.E_INVALID_ARG, "place value of visitor 2 is not finite", 2)         # then the visitors
        # an offender of member 1 at position 3 together with one of member 0 at position 9: the first in CALL order
        both = list(v12)
        both[3] = but(one, c_val=np.r_[np.inf, one["c_val"][1:]])
        both[9] = but(zero, p_idx=np.r_[-1, zero["p_idx"][1:]])
        refused(g12, both, PW, CW, kk, L.E_INVALID_ARG, "category value of visitor 3 is not finite", 3)
        both[3] = one
        refused(g12, both, PW, CW, kk, L.E_INVALID_ARG, "place index of visitor 9 is negative", 9)
        # within a visitor the place family comes first
        both[9] = but(zero, p_idx=zero["p_idx"][::-1].copy(), c_val=np.zeros(len(zero["c_val"])))
        refused(g12, both, PW, CW, kk, L.E_INVALID_ARG, "place indices of visitor 9 not strictly ascending", 9)
        # a place value 0.5: served for the member that does not renumber, refused for one that does
        half = list(v12)
        half[3] = but(one, p_val=np.r_[0.5, one["p_val"][1:]])
        st, off, p, e, cap, bad = raw_rows(pool, g12, vc.csr(half), PW, CW, kk, 1 << 20)
        assert st == L.OK and bad == -1
        wo, wp, we = ixs[1].visitors_recommend_batch(*vc.csr([half[3]]), PW, CW, kk)
        assert np.array_equal(p[off[3]:off[4]], wp) and np.array_equal(bits(e[off[3]:off[4]]), bits(we)) and len(wp) > 0
        half[9] = but(zero, p_val=np.r_[0.5, zero["p_val"][1:]])
        refused(g12, half, PW, CW, kk, L.E_INVALID_ARG, "place value of visitor 9 is not an integer count below 65536", 9)
        # an empty category vector
        none = list(v12)
        none[5] = dict(v12[5], c_idx=np.zeros(0, np.int32), c_val=np.zeros(0))
        refused(g12, none, PW, CW, kk, L.E_NOT_FOUND, "No such person: visitor 5 has no category vector", 5)
        with pytest.raises(pkg.IllegalArgumentException, match="No such person") as err:
            pool.visitors_recommend_batch(g12, *vc.csr(none), PW, CW, kk)
        assert err.value.bad_visitor == 5
        with pytest.raises(pkg.IllegalArgumentException, match="No such person") as err:
            pool.visitors_recommend_ranked_batch(g12, *vc.csr(none), PW, CW, kk, [1, 2], [0, 0], np.zeros(12, np.int64), 2)
        assert err.value.bad_visitor == 5
    for pw, cw, kk, message in ((1.0, 0.5, k, "Place weight must be in the interval (0; 1)"),
                                (0.5, 0.0, k, "Category weight must be in the interval (0; 1)"),
                                (0.4, 0.5, k, "Sum of weights must be 1.0"),
                                (0.5, 0.5, 0, "K nearest must be positive")):
        refused(g12, v12, pw, cw, kk, L.E_INVALID_ARG, "requirement failed: " + message, -1)
    # bad exclusion offsets: before anything else of the call, outputs untouched
    places, regions = pc.places_table()
    good_off = np.arange(13, dtype=np.int64)
    ids = np.arange(12, dtype=np.int64)
    st, oi, osc, cnt, bad = raw_ranked(pool, g12, vc.csr(v12), k, places, regions, np.zeros(12), 10, good_off, ids)
    assert st == L.OK and bad == -1 and cnt.min() >= 0
    for wrong in (np.r_[good_off[:5], 3, good_off[6:]], np.r_[-1, good_off[1:]]):
        st, oi, osc, cnt, bad = raw_ranked(pool, g12, vc.csr(v12), k, places, regions, np.zeros(12), 10, wrong, ids)
        assert st == L.E_INVALID_ARG and "exclude_offsets must be non-decreasing" in L.lib().locrec_last_error().decode()
        assert bad == -1 and np.all(oi == -7) and np.all(osc == -7.0) and np.all(cnt == -7)
    st, oi, osc, cnt, bad = raw_ranked(pool, g12, vc.csr(v12), k, places, regions, np.zeros(12), 10, None, ids)
    assert st == L.E_INVALID_ARG and "exclude_place_ids without exclude_offsets" in L.lib().locrec_last_error().decode()
    assert np.all(cnt == -7)


def person_answers(ix, d, k):
    rows = np.flatnonzero((np.diff(d["p_rowptr"]) > 0) & (np.diff(d["c_rowptr"]) > 0))
    persons = d["person_ids"][rows[[0, 3, 3, len(rows) - 1]]]
    return [np.asarray(x) for x in (*ix.recommend(int(persons[0]), PW, CW, k), *ix.recommend_batch(persons, PW, CW, k))]


def same(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("k", (2_000_000, 50))
def test_members_and_pool_serve_as_before(pkg, members, k):
    ds, ixs, pool = members
    gi, vs, names = pc.visitors()
    places, regions = pc.places_table()
    rq_gi = np.array([0, 2, 1, 2, 3], np.int32)
    rq_pid = np.array([ds[m]["person_ids"][7] for m in rq_gi], np.int64)
    want_pool = pool.recommend_batch(rq_gi, rq_pid, PW, CW, k)
    want = {m: person_answers(ixs[m], ds[m], k) for m in (0, 1, 2)}
    want_vis = {m: ixs[m].visitors_recommend_batch(*pc.of_member(m)[1], PW, CW, k) for m in (0, 1, 2)}
    for call in (lambda: pool.visitors_recommend_batch(gi, *pc.arrays(), PW, CW, k),
                 lambda: pool.visitors_recommend_ranked_batch(gi, *pc.arrays(), PW, CW, k, places, regions, pc.targets(3), 10)):
        for m in (0, 1, 2):
            ixs[m].recommend_range_async(0, 20, PW, CW, k)          # something resident that the pool call must drop
        call()
        for m in (0, 1, 2):
            with pytest.raises(pkg.IllegalArgumentException):
                ixs[m].fetch_recommend(20)
            with pytest.raises(pkg.IllegalArgumentException, match="no matching batched recommendation"):
                ixs[m].fetch_ranked(20, places, regions, np.zeros(20, np.int64), 10)
            assert same(person_answers(ixs[m], ds[m], k), want[m]), m
            assert same(ixs[m].visitors_recommend_batch(*pc.of_member(m)[1], PW, CW, k), want_vis[m]), m
        assert same(pool.recommend_batch(rq_gi, rq_pid, PW, CW, k), want_pool)


def test_a_repeated_call_allocates_nothing_and_everything_is_freed(pkg):
    from locations_recommender_amd import _lib as L
    ds = pc.members()
    gi, vs, names = pc.visitors()
    start = L.device_bytes_in_use()
    ixs = [make_index(pkg, d) for d in ds]
    pool = pkg.KnnPool(ixs)
    try:
        first = pool.visitors_recommend_batch(gi, *pc.arrays(), PW, CW, 2_000_000)
        before = L.device_allocations()
        again = pool.visitors_recommend_batch(gi, *pc.arrays(), PW, CW, 2_000_000)
        assert L.device_allocations() == before
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
        # a visitor's result depends on its own vector and its member only: another order, other tile-mates
        order = np.random.default_rng(9).permutation(len(gi))
        off, p, e = pool.visitors_recommend_batch(gi[order], *vc.csr([vs[i] for i in order]), PW, CW, 2_000_000)
        for j, i in enumerate(order):
            assert np.array_equal(p[off[j]:off[j + 1]], first[1][first[0][i]:first[0][i + 1]]), i
            assert np.array_equal(bits(e[off[j]:off[j + 1]]), bits(first[2][first[0][i]:first[0][i + 1]])), i
        pool.visitors_recommend_ranked_batch(gi, *on_device(pc.arrays()), PW, CW, 50, *pc.places_table(), pc.targets(2), 10,
                                             exclude=pc.exclusion_lists())
    finally:
        pool.close()
        for ix in ixs:
            ix.close()
    assert L.device_bytes_in_use() == start
