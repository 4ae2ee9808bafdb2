"""GPU: a pool of resident KNN indexes (locrec_knn_pool_*, KnnPool) against each member's own calls.  Request i of a pool
call must equal, bit for bit, what KnnIndex.recommend_batch / recommend_ranked_batch returns for that person on that
member alone; a subset is also compared with the oracle at the KNN tests' tolerance.  The members are the smallest
shapes at which the shared launches can go wrong (see `members`)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PW, CW = 0.4, 0.6
RTOL = 1e-6                   # tests/test_gpu_knn.py
LIMITS = (10, 257)            # LIMITS of tests/test_gpu_knn_ranked.py: the LDS lists; beyond LOCREC_RANK_BATCH_MAX_N
KS = (2_000_000, 1500, 50)    # every member shared; n <= 1501 shared, the others on the tiled any-K path; all delegated
FINISH_TILE, SEG_RATERS, QT = 2048, 4096, 16   # kFinishTile, kSegRaters, kLkbQt of csrc/knn_large.hip


def with_ratings(d, seed=3, popular=None, none=False):
    """tests/test_gpu_knn_ranked.py's idea: every person rates the places of its place vector.  popular: EVERY person
    also rates that place; none: no rating rows at all."""
    rng = np.random.default_rng(seed)
    d = dict(d)
    n = len(d["person_ids"])
    if none:
        d["r_rowptr"], d["r_place"], d["r_rating"] = np.zeros(n + 1, np.int64), np.empty(0, np.int64), np.empty(0, np.int64)
        return d
    ptr, idx = d["p_rowptr"], d["p_idx"].astype(np.int64)
    if popular is not None:
        rows = [np.union1d(idx[ptr[i]:ptr[i + 1]], [popular]) for i in range(n)]
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=ptr[1:])
        idx = np.concatenate(rows)
    d["r_rowptr"], d["r_place"] = ptr.copy(), idx
    d["r_rating"] = rng.integers(1, 6, size=len(idx)).astype(np.int64)
    return d


def without_place_vector(d, row):
    """The person at `row` gets an empty place vector (no valid query)."""
    d = dict(d)
    a, b = d["p_rowptr"][row], d["p_rowptr"][row + 1]
    d["p_idx"], d["p_val"] = np.delete(d["p_idx"], np.s_[a:b]), np.delete(d["p_val"], np.s_[a:b])
    ptr = d["p_rowptr"].copy()
    ptr[row + 1:] -= b - a
    d["p_rowptr"] = ptr
    return d


def make_index(pkg, d):
    return pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"],
                        d["c_rowptr"], d["c_idx"], d["c_val"], d["c_dim"], d["r_rowptr"], d["r_place"], d["r_rating"])


EMPTY_ROW = 5   # of member 0: a person without a place vector


def datasets():
    """0: 200 persons (one scan block), one of them without a place vector   1: 257 persons (two blocks), fp64 values:
    the GENERIC format, another p_dim (another bitmap size)   2: 3,000 persons (twelve blocks), more than 2,048 rated
    places (two finish tiles)   3: 4,200 persons who all rate place 7 (two segments of kSegRaters)   4: nobody rated
    anything   5: a member nobody asks."""
    from locations_recommender_amd import synth
    ds = [with_ratings(without_place_vector(synth.small_knn_dataset(n=200, p_dim=300, seed=21), EMPTY_ROW), 1),
          with_ratings(synth.small_knn_dataset(n=257, p_dim=700, seed=22, integer=False), 2),
          with_ratings(synth.small_knn_dataset(n=3000, p_dim=5000, seed=23), 3),
          with_ratings(synth.small_knn_dataset(n=4200, p_dim=64, seed=24), 4, popular=7),
          with_ratings(synth.small_knn_dataset(n=200, p_dim=300, seed=25), none=True),
          with_ratings(synth.small_knn_dataset(n=200, p_dim=300, seed=26), 6)]
    blocks = [(len(d["person_ids"]) + 255) // 256 for d in ds]
    assert blocks[:3] == [1, 2, 12]
    assert len({d["p_dim"] for d in ds}) >= 3
    assert not np.all(ds[1]["p_val"] == np.round(ds[1]["p_val"]))
    rated = [len(np.unique(d["r_place"])) for d in ds]
    assert rated[2] > FINISH_TILE and max(rated[0], rated[1], rated[3]) <= FINISH_TILE and rated[4] == 0
    assert np.bincount(ds[3]["r_place"]).max() > SEG_RATERS
    assert np.bincount(ds[2]["r_place"]).max() <= SEG_RATERS
    assert len(np.intersect1d(ds[0]["person_ids"], ds[1]["person_ids"])) > 0
    return ds


@pytest.fixture(scope="module")
def members(pkg):
    ds = datasets()
    ixs = [make_index(pkg, d) for d in ds]
    pool = pkg.KnnPool(ixs)
    yield ds, ixs, pool
    pool.close()
    for ix in ixs:
        ix.close()


def valid_rows(d):
    return np.flatnonzero((np.diff(d["p_rowptr"]) > 0) & (np.diff(d["c_rowptr"]) > 0))


def the_requests(ds):
    """37 distinct persons of member 2 (three waves, the last tile partial), 1 - 3 of the others, member 5 unasked;
    repeated (index, person) pairs; one person id asked of members 0 and 1.  Interleaved."""
    rng = np.random.default_rng(5)
    shared_id = np.intersect1d(ds[0]["person_ids"][valid_rows(ds[0])], ds[1]["person_ids"][valid_rows(ds[1])])[0]
    per = {0: 2, 1: 1, 2: 37, 3: 2, 4: 2}
    gi, pid = [], []
    for m, cnt in per.items():
        d = ds[m]
        ids = d["person_ids"][rng.choice(valid_rows(d), cnt, replace=False)]
        gi += [m] * cnt
        pid += ids.tolist()
    gi += [0, 1, 2, 2, 0]
    pid += [int(shared_id), int(shared_id), pid[5], pid[5], pid[0]]       # the shared id; repeats of members 2 and 0
    order = rng.permutation(len(gi))
    return np.asarray(gi, np.int32)[order], np.asarray(pid, np.int64)[order]


def places_table(ds):
    ids = np.arange(-5, max(d["p_dim"] for d in ds) + 5, dtype=np.int64)
    return ids, ids % 3


_alone = {}


def alone(ixs, gi, pid, k):
    """Every member's own recommend_batch for its requests, once per K: {request: (places, ratings)}."""
    key = (k, gi.tobytes(), pid.tobytes())
    if key not in _alone:
        rows = {}
        for m in np.unique(gi):
            at = np.flatnonzero(gi == m)
            off, p, e = ixs[m].recommend_batch(pid[at], PW, CW, k)
            for j, i in enumerate(at):
                rows[int(i)] = (p[off[j]:off[j + 1]].copy(), e[off[j]:off[j + 1]].copy())
        _alone[key] = rows
    return _alone[key]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_pool_against_members(pool, ixs, gi, pid, k):
    off, p, e = pool.recommend_batch(gi, pid, PW, CW, k)
    want = alone(ixs, gi, pid, k)
    assert len(off) == len(gi) + 1 and off[0] == 0 and off[-1] == len(p) == len(e)
    for i in range(len(gi)):
        wp, we = want[i]
        assert np.array_equal(p[off[i]:off[i + 1]], wp), (k, i, gi[i])
        assert np.array_equal(bits(e[off[i]:off[i + 1]]), bits(we)), (k, i, gi[i])
    return off, p, e


@pytest.mark.parametrize("k", KS)
def test_rows_equal_each_members_own_batch(pkg, oracle, members, k):
    ds, ixs, pool = members
    gi, pid = the_requests(ds)
    assert 5 not in gi and np.sum(gi == 2) >= 37
    off, p, e = check_pool_against_members(pool, ixs, gi, pid, k)
    st = pool.stats()
    n = np.array([len(d["person_ids"]) for d in ds])
    shared = (k > 1024) & (k >= n - 1)
    asked = np.unique(gi)
    assert st["delegated_members"] == int(np.sum(~shared[asked]))
    if k == 2_000_000:
        # member 4 (no rating rows) joins no wave; member 2's 37 distinct requests make three waves
        assert st["waves"] == 3 and st["member_tiles"] == 4 + 1 + 1
        assert st["scan_launches"] == 3 and st["aggregate_launches"] == 3 and st["fill_launches"] == 6 and st["finish_launches"] == 9
        assert st["emitted_rows"] == sum(len(v[0]) for i, v in alone(ixs, gi, pid, k).items()
                                         if i in {int(np.flatnonzero((gi == gi[j]) & (pid == pid[j]))[0]) for j in range(len(gi))})
    if k == 50:
        assert st["waves"] == 0 and st["scan_launches"] == 0
    assert off[-1] > 0
    empty = np.flatnonzero(gi == 4)
    assert np.all(off[empty] == off[empty + 1])
    # a subset against the oracle
    for m in asked:
        for i in np.flatnonzero(gi == m)[:2]:
            op, oe = oracle.knn_recommend(ds[m], int(pid[i]), PW, CW, k)
            assert np.array_equal(p[off[i]:off[i + 1]], op), (k, m)
            np.testing.assert_allclose(e[off[i]:off[i + 1]], oe, rtol=RTOL, atol=0)


@pytest.mark.parametrize("k", KS)
def test_ranked_equals_each_members_own_ranked_batch(pkg, members, k):
    ds, ixs, pool = members
    gi, pid = the_requests(ds)
    places, regions = places_table(ds)
    rng = np.random.default_rng(k)
    targets = rng.choice([0, 1, 2, 99], len(gi)).astype(np.int64)     # 99: a region no place belongs to
    rep = [np.flatnonzero((gi == gi[j]) & (pid == pid[j])) for j in range(len(gi))]
    rep = max(rep, key=len)
    assert len(rep) >= 2
    targets[rep[0]], targets[rep[1]] = 0, 1                           # a repeated pair, two targets
    assert 99 in targets
    for limit in LIMITS:
        oi, osc, cnt = pool.recommend_ranked_batch(gi, pid, PW, CW, k, places, regions, targets, limit)
        st = pool.stats()
        assert oi.shape == (len(gi), min(limit, len(places)))
        for m in np.unique(gi):
            at = np.flatnonzero(gi == m)
            wi, ws, wc = ixs[m].recommend_ranked_batch(pid[at], PW, CW, k, places, regions, targets[at], limit)
            assert np.array_equal(oi[at], wi) and np.array_equal(cnt[at], wc), (k, limit, m)
            assert np.array_equal(bits(osc[at]), bits(ws)), (k, limit, m)
        assert np.all(cnt[targets == 99] == 0) and cnt.max() > 0
        if k == 2_000_000:
            assert st["waves"] == 3 and st["delegated_members"] == 0
            # only the waves' tile counts and the ranked rows reach the host through the pool
            tiles = [max(1, -(-len(np.unique(d["r_place"])) // FINISH_TILE)) for d in ds]
            counts = ((tiles[0] + tiles[1] + tiles[2] + tiles[3]) + 2 * tiles[2]) * QT * 4
            assert st["readback_bytes"] == counts + len(gi) * oi.shape[1] * 16 + len(gi) * 8


def test_one_launch_per_kernel_and_wave(pkg):
    """Twelve members, two requests each: one wave, every kernel launched once for all of them (the fill kernel twice:
    set and wipe), host waits = a constant plus one per wave.  Seventeen requests of one member: a second wave, twice the
    launches.  No loop over members meets these counts."""
    from locations_recommender_amd import synth
    ds = [with_ratings(synth.small_knn_dataset(n=200, p_dim=300, seed=40 + m), m) for m in range(12)]
    ixs = [make_index(pkg, d) for d in ds]
    pool = pkg.KnnPool(ixs)
    try:
        gi = np.repeat(np.arange(12, dtype=np.int32), 2)
        pid = np.concatenate([d["person_ids"][valid_rows(d)[:2]] for d in ds])
        for _ in range(2):   # (the second call finds the row buffer grown)
            pool.recommend_batch(gi, pid, PW, CW, 2_000_000)
        st = pool.stats()
        assert (st["waves"], st["member_tiles"], st["delegated_members"]) == (1, 12, 0)
        assert (st["fill_launches"], st["scan_launches"], st["aggregate_launches"], st["finish_launches"]) == (2, 1, 1, 3)
        assert st["host_syncs"] == 2 + st["waves"]      # the wave's tile counts; the end of the launches; the rows' copy
        check_pool_against_members(pool, ixs, gi, pid, 2_000_000)
        gi2 = np.r_[gi, np.full(15, 3, np.int32)]
        pid2 = np.r_[pid, ds[3]["person_ids"][valid_rows(ds[3])[2:17]]]
        for _ in range(2):
            pool.recommend_batch(gi2, pid2, PW, CW, 2_000_000)
        st = pool.stats()
        assert (st["waves"], st["member_tiles"]) == (2, 13)
        assert (st["fill_launches"], st["scan_launches"], st["aggregate_launches"], st["finish_launches"]) == (4, 2, 2, 6)
        assert st["host_syncs"] == 2 + st["waves"]
        check_pool_against_members(pool, ixs, gi2, pid2, 2_000_000)
    finally:
        pool.close()
        for ix in ixs:
            ix.close()


def member_answers(ix, d, k):
    rows = valid_rows(d)
    persons = d["person_ids"][rows[[0, 3, 3, len(rows) - 1]]]
    one = ix.recommend(int(persons[0]), PW, CW, k)
    batch = ix.recommend_batch(persons, PW, CW, k)
    ix.recommend_range_async(2, 20, PW, CW, k)
    ranged = ix.fetch_recommend(20)
    return [np.asarray(x) for x in (*one, *batch, *ranged)]


def same_answers(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                                     y.view(np.uint64) if y.dtype == np.float64 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("k", [2_000_000, 50])
def test_members_serve_as_fresh_handles_around_a_pool_call(pkg, members, k):
    ds, ixs, pool = members
    gi, pid = the_requests(ds)
    places, regions = places_table(ds)
    for m in (0, 1, 2):
        fresh = make_index(pkg, ds[m])
        want = member_answers(fresh, ds[m], k)
        fresh.close()
        assert same_answers(member_answers(ixs[m], ds[m], k), want), m
        ixs[m].recommend_range_async(0, 20, PW, CW, k)      # something resident that the pool call must drop
        pool.recommend_batch(gi, pid, PW, CW, k)
        with pytest.raises(pkg.IllegalArgumentException, match="no matching batched recommendation"):
            ixs[m].fetch_ranked(20, places, regions, np.zeros(20, np.int64), 10)
        assert same_answers(member_answers(ixs[m], ds[m], k), want), m
        pool.recommend_ranked_batch(gi, pid, PW, CW, k, places, regions, np.zeros(len(gi), np.int64), 10)
        with pytest.raises(pkg.IllegalArgumentException, match="no matching batched recommendation"):
            ixs[m].fetch_ranked(20, places, regions, np.zeros(20, np.int64), 10)
        assert same_answers(member_answers(ixs[m], ds[m], k), want), m


def test_a_repeated_call_allocates_nothing(pkg, members):
    from locations_recommender_amd import _lib as L
    ds, ixs, pool = members
    gi, pid = the_requests(ds)
    first = pool.recommend_batch(gi, pid, PW, CW, 2_000_000)
    before = L.device_allocations()
    again = pool.recommend_batch(gi, pid, PW, CW, 2_000_000)
    assert L.device_allocations() == before
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_the_row_buffer_grows_mid_call_and_keeps_its_rows(pkg, members):
    """33 distinct persons of dataset 2 at K = 2,000,000 on FRESH handles - a KnnIndex, and a KnnPool of another: three
    tiles; the first sizes the empty row buffer, the second outgrows it while the first tile's rows are in it.  Both
    paths process a member's queries in row order, and an index's rows ascend by (place count, category count): the
    persons are given in that order with distinct keys, so the returned offsets are the running totals the growth rule
    saw: buffer of off[16] + off[16] // 2 + 1024 rows after tile 0, off[32] rows wanted after tile 1."""
    ds, ixs, _ = members
    d = ds[2]
    n_p, n_c = np.diff(d["p_rowptr"]), np.diff(d["c_rowptr"])
    first_of_key = {}
    for r in valid_rows(d):
        first_of_key.setdefault((int(n_p[r]), int(n_c[r])), int(r))
    rows = [first_of_key[key] for key in sorted(first_of_key)[:33]]
    assert len(rows) == 33
    pid = d["person_ids"][rows]
    k = 2_000_000
    alone_ix, pooled_ix = make_index(pkg, d), make_index(pkg, d)
    pool = pkg.KnnPool([pooled_ix])
    try:
        got = {"index": alone_ix.recommend_batch(pid, PW, CW, k),
               "pool": pool.recommend_batch(np.zeros(33, np.int32), pid, PW, CW, k)}
        assert pool.stats()["waves"] == 3
    finally:
        pool.close()
        alone_ix.close()
        pooled_ix.close()
    for name, (off, p, e) in got.items():
        assert off[16] > 0 and off[32] > off[16] + off[16] // 2 + 1024, (name, off[16], off[32])   # a growth with rows to keep
        for i in (0, 15, 16, 31, 32):                          # either side of each tile boundary
            wp, we = ixs[2].recommend(int(pid[i]), PW, CW, k)
            assert np.array_equal(p[off[i]:off[i + 1]], wp), (name, i)
            assert np.array_equal(bits(e[off[i]:off[i + 1]]), bits(we)), (name, i)
    assert all(np.array_equal(a, b) for a, b in zip(got["index"][:2], got["pool"][:2]))
    assert np.array_equal(bits(got["index"][2]), bits(got["pool"][2]))


def raw_call(pool, gi, pid, pw, cw, k, room):
    """locrec_knn_pool_recommend_batch on sentinel-filled outputs -> (status, offsets, places, ratings, capacity, bad)."""
    from locations_recommender_amd import _lib as L
    gi, pid = np.asarray(gi, np.int32), np.asarray(pid, np.int64)
    off = np.full(len(gi) + 1, -7, np.int64)
    places, est = np.full(max(room, 1), -7, np.int64), np.full(max(room, 1), -7.0)
    cap, bad = C.c_int64(room), C.c_int64(-9)
    st = L.lib().locrec_knn_pool_recommend_batch(pool._h, len(gi), L.ptr(gi, C.c_int32), L.ptr(pid, C.c_int64), pw, cw, k,
                                                 L.ptr(off, C.c_int64), L.ptr(places, C.c_int64), L.ptr(est, C.c_double),
                                                 C.byref(cap), C.byref(bad))
    return st, off, places, est, cap.value, bad.value


def test_capacity_protocol_and_refusals(pkg, members):
    from locations_recommender_amd import _lib as L
    ds, ixs, pool = members
    gi, pid = the_requests(ds)
    k = 2_000_000
    want_off, want_p, want_e = pool.recommend_batch(gi, pid, PW, CW, k)
    total = int(want_off[-1])
    st, off, p, e, cap, bad = raw_call(pool, gi, pid, PW, CW, k, total - 1)          # too little room: sizes only
    assert st == L.OK and cap == total and bad == -1 and np.array_equal(off, want_off)
    assert np.all(p == -7) and np.all(e == -7.0)
    st, off, p, e, cap, bad = raw_call(pool, gi, pid, PW, CW, k, total + 3)          # enough room
    assert st == L.OK and cap == total and np.array_equal(off, want_off)
    assert np.array_equal(p[:total], want_p) and np.array_equal(bits(e[:total]), bits(want_e)) and np.all(p[total:] == -7)
    st, off, p, e, cap, bad = raw_call(pool, [], [], PW, CW, k, 5)                    # the empty list
    assert st == L.OK and off[0] == 0 and cap == 0 and bad == -1
    o, pp, ee = pool.recommend_batch([], [], PW, CW, k)
    assert o.tolist() == [0] and len(pp) == 0 and len(ee) == 0

    def refused(gi_, pid_, pw, cw, kk, status, message, where):
        st, off, p, e, cap, bad = raw_call(pool, gi_, pid_, pw, cw, kk, 64)
        assert st == status and message in L.lib().locrec_last_error().decode(), (message, L.lib().locrec_last_error())
        assert bad == where
        assert np.all(off == -7) and np.all(p == -7) and np.all(e == -7.0) and cap == 64     # nothing else is written
    unknown = 999_999_999
    empty_vec = int(ds[0]["person_ids"][EMPTY_ROW])
    assert ds[0]["p_rowptr"][EMPTY_ROW] == ds[0]["p_rowptr"][EMPTY_ROW + 1]
    g3, p3 = gi[:6].copy(), pid[:6].copy()
    g3[4] = len(ixs)
    refused(g3, p3, PW, CW, k, L.E_INVALID_ARG, f"names index {len(ixs)}", 4)
    g3[4] = -1
    p3[2] = unknown                                                                       # index positions come first
    refused(g3, p3, PW, CW, k, L.E_INVALID_ARG, "names index -1", 4)
    g3[4] = gi[4]
    refused(g3, p3, 0.0, CW, k, L.E_INVALID_ARG, "Place weight must be in the interval (0; 1)", -1)   # then the requires
    refused(g3, p3, PW, CW, k, L.E_NOT_FOUND, f"No such person: {unknown}", 2)
    g3[2], p3[2] = 0, empty_vec
    refused(g3, p3, PW, CW, k, L.E_NOT_FOUND, f"No such person: {empty_vec}", 2)
    for kk in (k, 50):
        with pytest.raises(pkg.IllegalArgumentException, match="No such person") as err:
            pool.recommend_batch(g3, p3, PW, CW, kk)
        assert err.value.bad_request == 2
        with pytest.raises(pkg.IllegalArgumentException, match="No such person") as err:
            pool.recommend_ranked_batch(g3, p3, PW, CW, kk, [1, 2], [0, 0], np.zeros(6, np.int64), 3)
        assert err.value.bad_request == 2
    for pw, cw, kk, message in ((0.0, 0.5, k, "Place weight must be in the interval (0; 1)"),
                                (1.0, 0.5, k, "Place weight must be in the interval (0; 1)"),
                                (0.5, 0.0, k, "Category weight must be in the interval (0; 1)"),
                                (0.4, 0.5, k, "Sum of weights must be 1.0"),
                                (0.5, 0.5, 0, "K nearest must be positive")):
        refused(gi[:6], pid[:6], pw, cw, kk, L.E_INVALID_ARG, "requirement failed: " + message, -1)
    # create's refusals
    h = C.c_void_p()
    lib = L.lib()
    assert lib.locrec_knn_pool_create((C.c_void_p * 2)(ixs[0]._h, None), 2, C.byref(h)) == L.E_INVALID_ARG and not h.value
    assert "index 1 is NULL" in lib.locrec_last_error().decode()
    assert lib.locrec_knn_pool_create((C.c_void_p * 3)(ixs[0]._h, ixs[1]._h, ixs[0]._h), 3, C.byref(h)) == L.E_INVALID_ARG
    assert "index 2 is listed twice" in lib.locrec_last_error().decode() and not h.value
    with pytest.raises(pkg.IllegalArgumentException, match="1 .. 65535 indexes"):
        pkg.KnnPool([])


def test_the_request_lines_of_the_main(pkg, tmp_path):
    """mains.knn_recommender_requests on a sample written by the generator and builder mains (300 persons, 300 places, as
    tests/test_gpu_sg_pool.py): every good line equals knn_recommender_request's result, every bad line carries that
    function's exception, with the pool and with one call per index.

    K = 20 (the K of tests/test_gpu_sample.py's request lines): equality of ids and rating BITS - the single request and
    the batch aggregate in the same order there.  K = 2,000,000 (the shipped K, the shared launches): these indexes hold
    94 - 196 persons, so the single request runs K_eff = n - 1 <= LOCREC_KNN_BATCH_MAX_K through the neighbour-major
    aggregation of csrc/knn.hip while every batch of K > 1024 - the member's own and the pool's - sums place-major
    (csrc/knn_large.hip): other orders of the same sums.  Measured on these indexes: KnnIndex.recommend against
    KnnIndex.recommend_batch differs in most rows, by at most 8 ulp.  There the pool and the per-index calls must agree
    bit for bit, and both must agree with the single request in the exceptions, the targets and the ratings to the KNN
    tests' tolerance; ids may differ only where two ratings are tied within it."""
    import sample_cases as sc
    from locations_recommender_amd import mains
    D = sc.defaults()
    d = str(tmp_path)
    mains.sample_generator_main(d, 300, 300, D["regions"], D["categories"])
    sets = mains.rating_vectors_builder_main(d, 400, 100, 10)
    assert (0,) in sets and (0, 1) in sets and (1, 2) in sets
    persons = mains.load_persons(d)

    def queries_of(rs):
        pp = mains.load_rating_vectors(mains.generate_file_name(rs, d, "place_rating_vectors"))[0]
        cp = mains.load_rating_vectors(mains.generate_file_name(rs, d, "category_rating_vectors"))[0]
        return np.intersect1d(pp, cp)
    home = persons["home_region_id"]
    q0, q01, q12 = queries_of([0]), queries_of([0, 1]), queries_of([1, 2])
    assert max(len(q0), len(q01), len(q12)) <= 1024
    # a person of persons_sample whom the index of its home region lacks (no visit joined a place there): found, not assumed
    lacking = np.setdiff1d(persons["id"][home == 0], q0)
    assert len(lacking) > 0, "every person of region 0 is in its index: choose fewer visits or days"
    absent = int(lacking[0])
    in0 = np.intersect1d(np.intersect1d(persons["id"][home == 0], q0), q01)
    in1 = np.intersect1d(persons["id"][home == 1], q12)
    assert len(in0) >= 3 and len(in1) >= 2
    lines = [f"{in0[0]}", f"{in0[1]} 1", "x", f"{in1[0]} 2", f"{absent}", "5 1", f"{in0[0]}", f"{in0[2]}  0", f"{in1[1]} 2",
             f"{in0[0]} 1"]
    for k in (20, 2_000_000):
        want = []
        for line in lines:
            try:
                want.append(mains.knn_recommender_request(d, persons, line, PW, CW, k, max_recommendations=7))
            except Exception as e:
                want.append(e)
        kinds = [type(x) for x in want if isinstance(x, Exception)]
        assert kinds == [pkg.IllegalArgumentException, pkg.IllegalArgumentException, mains.NoSuchElementException]
        assert str(want[2]).startswith("Failed to parse input") and str(want[4]) == f"No such person: {absent}"
        assert str(want[5]) == "Person not found: 5"
        assert len({tuple(sorted({x[0][1], x[0][2]})) for x in want if not isinstance(x, Exception)}) >= 3   # region sets
        assert any(len(x[1]) > 0 for x in want if not isinstance(x, Exception))
        got = {pooled: mains.knn_recommender_requests(d, persons, lines, PW, CW, k, max_recommendations=7, pooled=pooled)
               for pooled in (True, False)}
        for pooled in (True, False):
            assert len(got[pooled]) == len(lines)
            for line, a, b in zip(lines, got[pooled], want):
                if isinstance(b, Exception):
                    assert type(a) is type(b) and str(a) == str(b), (k, pooled, line)
                    continue
                assert a[0] == b[0] and len(a[1]) == len(b[1]), (k, pooled, line)
                if k <= 1024:
                    assert np.array_equal(a[1], b[1]) and sc.same_bits(np.asarray(a[2]), np.asarray(b[2])), (k, pooled, line)
                else:
                    np.testing.assert_allclose(a[2], b[2], rtol=RTOL, atol=0)
                    other = np.flatnonzero(a[1] != b[1])       # only where ratings are tied within the tolerance
                    for i in other:
                        tied = [j for j in (i - 1, i + 1) if 0 <= j < len(b[2]) and np.isclose(b[2][j], b[2][i], rtol=RTOL, atol=0)]
                        assert tied or i == len(b[2]) - 1, (k, pooled, line, i)
        for a, b in zip(got[True], got[False]):
            if not isinstance(a, Exception):
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and sc.same_bits(np.asarray(a[2]), np.asarray(b[2])), k
    assert mains.knn_recommender_requests(d, persons, [], PW, CW, 2_000_000) == []
