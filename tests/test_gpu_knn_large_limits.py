"""The tiled any-K top-K and the large-K aggregation (csrc/knn_large.hip) ON their structural limits (DESIGN.md,
"Limits of the tiled top-K"; the inputs: knn_large_limit_cases.py, proved on the CPU by test_knn_large_limit_cases.py to
hit every planted segment, run count, pass count, deciding bin and rater count exactly).

Bars: counts and neighbour ids equal to the oracle's (np.array_equal), similarities bit-identical, (-1, 0.0) padding
behind the count, a sample equal to the single request; recommended places equal to the oracle's, estimates within
1e-6 of it and bit-identical to the single request's.  One index and one set of oracle answers serve every test.

Each docstring names the limit and the misreading of it that the test is there to catch."""
import os

import numpy as np
import pytest

import knn_large_limit_cases as lc
from test_gpu_knn import make_index
from test_gpu_knn_any_k import RTOL, check_recommend_single, check_rows

pytestmark = pytest.mark.gpu
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))


class Shared:
    """An index and the oracle's answers on its data, computed once per (rows, weights, K)."""

    def __init__(self, pkg, oracle, d):
        self.o, self.d, self.ix, self.memo = oracle, d, make_index(pkg, d), {}

    def rows(self, rows, w, k):
        key = (tuple(int(r) for r in rows), w, k)
        if key not in self.memo:
            self.memo[key] = self.o.knn_similar_batch(self.d, np.asarray(rows, np.int64), w[0], w[1], k, nthreads=THREADS)
        return self.memo[key]

    def recommend(self, row, w, k):
        key = ("r", int(row), w, k)
        if key not in self.memo:
            self.memo[key] = self.o.knn_recommend(self.d, int(self.d["person_ids"][row]), w[0], w[1], k)
        return self.memo[key]


@pytest.fixture(scope="module")
def main(pkg, oracle):
    sh = Shared(pkg, oracle, lc.main_index()[0])
    yield sh
    sh.ix.close()


@pytest.fixture(scope="module")
def small(pkg, oracle):
    sh = Shared(pkg, oracle, lc.small_index())
    yield sh
    sh.ix.close()


def check_query(sh, rows, w, k, singles=(0,)):
    """query_batch of `rows` at K against the oracle; the listed positions equal to the single query."""
    pids = sh.d["person_ids"][np.asarray(rows)]
    ids, sims, cnt = sh.ix.query_batch(pids, w[0], w[1], k)
    check_rows(ids, sims, cnt, *sh.rows(rows, w, k), k, k)
    for j in singles:
        a, b = sh.ix.query(int(pids[j]), w[0], w[1], k)
        c = int(cnt[j])
        assert c == len(a) and np.array_equal(ids[j, :c], a) and np.array_equal(sims[j, :c], b), (k, j)
    return ids, sims, cnt


def check_recommend(sh, rows, w, k, against=None, singles=None):
    """recommend_batch of `rows` at K: the positions `against` equal the oracle's places with estimates within RTOL, the
    positions `singles` are bit-identical to the single recommend."""
    pids = sh.d["person_ids"][np.asarray(rows)]
    off, places, est = sh.ix.recommend_batch(pids, w[0], w[1], k)
    assert off[0] == 0 and len(off) == len(rows) + 1 and off[-1] == len(places) == len(est)
    for j in (range(len(rows)) if against is None else against):
        op, oe = sh.recommend(rows[j], w, k)
        assert np.array_equal(places[off[j]:off[j + 1]], op), (k, j, "places differ from the oracle")
        np.testing.assert_allclose(est[off[j]:off[j + 1]], oe, rtol=RTOL, atol=0)
    pick = list(range(len(rows)) if singles is None else singles)
    sub = np.r_[0, np.cumsum([off[j + 1] - off[j] for j in pick])].astype(np.int64)
    take = np.concatenate([np.arange(off[j], off[j + 1]) for j in pick]).astype(np.int64)
    check_recommend_single(sh.ix, pids[pick], w[0], w[1], k, sub, places[take], est[take])
    return off, places, est


@pytest.mark.parametrize("name", list(lc.RUN_TABLE))
def test_runs_and_merge_passes(main, name):
    """Segments of exactly 8,192, 8,193, 16,384, 16,385, 24,577 and 32,769 entries of ONE bin (R = kLktRun = 8,192), K on
    R, 2R, the segment and their neighbours.  Catches: lkt_sort_runs keeping K - 1 or len - 1 entries; a last run of one
    entry dropped (`R < most` read as `2R <= most`, `na` / `nb` / `full` of lkt_merge_pass off by one, `base >= n`); a
    third run not copied through pass 1; the result read from the wrong ping-pong array after an odd number of passes;
    the cut at K applied one entry early or late when K = R or 2R."""
    _, meta = lc.main_index()
    segment, ks, runs, passes, _ = lc.RUN_TABLE[name]
    q = meta["query"][name]
    member = int(meta["members"][(lc.FAMILY_INDEX[name], 1)][0])     # a second column whose segment differs
    for k in ks:
        f = lc.facts(q, k)
        assert (f["segment"], f["runs"], f["passes"]) == (segment, runs, passes)
        ids, _, cnt = check_query(main, [q, member], lc.HALF, k)
        assert cnt[0] == min(k, segment)
        assert np.array_equal(ids[0, :cnt[0]], lc.expected(q, k)[1]), "the closed form"
        check_recommend(main, [q, member], lc.HALF, k)


@pytest.mark.parametrize("nq", [16, 17, 33])
def test_mixed_tile(main, nq):
    """One tile whose columns have segments of 5 .. 32,769 entries: they need 0, 1, 2 and 3 merge passes but share one
    launch grid sized by the largest column (kLkbQt = 16 queries a tile).  Catches: the pass loop or the grid sized by
    the first or the last column; a finished column merged once more or its result taken from the array of the longest
    column's parity; segments laid end to end with a wrong offset; on the recommend side, at K = 1,025 and 8,193, the
    mask's K-th entry `keys[T.off[t] + K - 1]` read from the array another column's parity left (at 32,769 every column
    is complete and no K-th entry is read).  17 and 33 queries put ONE query into the last tile,
    give one query twice and come in shuffled order: catches a result slot computed from the tile's position."""
    rows = lc.mixed_rows(nq)
    pids = main.d["person_ids"][rows]
    before = main.ix.query_batch(pids, 0.5, 0.5, 50), main.ix.recommend_batch(pids, 0.5, 0.5, 50)
    for k in lc.MIXED_KS[nq]:
        ids, sims, cnt = check_query(main, rows, lc.HALF, k, singles=range(0, nq, 5))
        if nq > 16:
            assert rows[-1] == rows[3] and np.array_equal(ids[-1], ids[3]) and np.array_equal(sims[-1], sims[3]) and cnt[-1] == cnt[3]
        cut = [not lc.facts(r, k)["all"] for r in rows[:16]]
        assert any(cut) == (k < 32769), "below 32,769 the mask reads the K-th entry of columns of 1, 2 and 3 passes"
        off, places, est = check_recommend(main, rows, lc.HALF, k)      # every query: the oracle and the single recommend
        if nq > 16:
            assert np.array_equal(places[off[-2]:off[-1]], places[off[3]:off[4]]) and np.array_equal(est[off[-2]:off[-1]], est[off[3]:off[4]])
    after = main.ix.query_batch(pids, 0.5, 0.5, 50), main.ix.recommend_batch(pids, 0.5, 0.5, 50)
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), "a K = 50 batch changed after the tiled batches"


def test_deciding_bins(main):
    """lkt_select's walk over 4,096 bins by 1,024 threads of 4: the K-th candidate in bin 4095 with s = 1.0 exactly
    (int(s * 4096) = 4096, clamped), in bins 3699 = 4t + 3 and 3697 = 4t + 1 of thread 924 (3698 empty), in 3696 = 4t (the
    walk falls through to the first bin of the range without testing it), in 3652 (alone in thread 913's range) and in
    bin 0 (s < 1 / 4096 under pw = 2^-12); K on the first and the last entry of each.  Catches: a missing clamp in the
    collect's bin; `above` not carried over the upper bins of the range (the segment ends before the K-th entry);
    the owning thread chosen with `<=` for `<` at the last entry of a bin (two threads or none write the record); a
    fall-through that stops at 4t + 1; bin 0 taken for "no bin"."""
    _, meta = lc.main_index()
    q = meta["query"]["bins"]
    member = int(meta["members"][(lc.FAMILY_INDEX["bins"], 2)][0])
    for k, bstar, above, segment in lc.BIN_TABLE:
        f = lc.facts(q, k, lc.TINY_PW)
        assert (f["bstar"], f["above"], f["segment"]) == (bstar, above, segment)
        ids, sims, cnt = check_query(main, [q, member], lc.TINY_PW, k)
        assert cnt[0] == k and np.array_equal(ids[0], lc.expected(q, k, lc.TINY_PW)[1])
        assert np.all(sims[0, :1100] == 1.0)
        check_recommend(main, [q, member], lc.TINY_PW, k)


def test_candidate_count(main):
    """A query with exactly 1,030 candidates at K = 1,029, 1,030 and 1,031: `T.all = cand <= K` of the tiled batch and the
    `k >= cand` shortcut of the single recommend.  Both sides of either comparison must give the same rows at K = cand:
    catches a count other than min(K, cand), a K-th entry read at position K - 1 of a segment that ends before it when
    a complete column is taken for a cut one, and a batch that differs from the single request when the two take
    different branches.  On the whole index K = n - 2 is the last tiled K, n - 1 and the shipped 2,000,000 take no top-K."""
    d, meta = lc.main_index()
    n = len(d["person_ids"])
    q = meta["query"]["cand1030"]
    other = meta["query"]["only2048"]
    for k in lc.CAND_KS:
        ids, sims, cnt = check_query(main, [q, other], lc.HALF, k)
        assert cnt.tolist() == [min(k, 1030), 5]
        check_recommend(main, [q, other], lc.HALF, k)
    rows = [q, meta["query"]["run8193"], meta["query"]["bins"]]
    for k in (n - 2, n - 1):
        ids, sims, cnt = check_query(main, rows, lc.HALF, k)
        assert cnt.tolist() == [1030, 8193, 2120]
        check_recommend(main, rows, lc.HALF, k)
    k = 2_000_000
    check_query(main, rows[:2], lc.HALF, k)
    check_recommend(main, rows[:2], lc.HALF, k)


def test_aggregation_segments_and_finish_tiles(main):
    """Places with exactly 4,095, 4,096, 4,097, 8,192 and 8,193 raters (segments of kSegRaters = 4,096: 1, 1, 2, 2, 3) and
    exactly 2,049 rated places (finish tiles of kFinishTile = 2,048: the second holds one place).  K = 8,193 of 16,384
    candidates drops part of every limit place's raters, K = 16,383 one person, K = 16,384 nobody.  Catches: a segment
    table cut with `<=` (an empty or a lost last segment), a segment's last rater skipped, the last finish tile not
    launched or its base taken from its own count, rows of the place of rank 2,047 / 2,048 swapped or lost.  Three small
    queries in the same batch: rows only for the place of rank 2,048 (nothing in tile 0), rows in tile 0 only, no rows."""
    _, meta = lc.main_index()
    rows = [meta["query"][name] for name in (lc.AGG_FAMILY, "only2048", "tile0", "norows")]
    for k in lc.AGG_KS:
        off, places, est = check_recommend(main, rows, lc.HALF, k)
        first = lc.place_rank(places[off[0]:off[1]])
        assert {0, 1, 2, 3, 2046, 2047, 2048} <= set(first.tolist())
        assert np.array_equal(places[off[0]:off[1]], lc.expected_places(rows[0], k))
        assert lc.place_rank(places[off[1]:off[2]]).tolist() == [2048]
        assert lc.place_rank(places[off[2]:off[3]]).tolist() == [5, 2047]
        assert off[3] == off[4], "a query whose neighbours rated nothing gets no rows"
    for order in ([3, 1, 2, 0], [1, 3], [3]):
        check_recommend(main, [rows[j] for j in order], lc.HALF, 8193)


def test_host_given_neighbours_on_the_same_limits(main):
    """The third caller of the place-major aggregation: weights given on the host (recommend_neighbours with more than
    1,024 neighbours -> knn_large_aggregate).  The query of test_aggregation_segments_and_finish_tiles at K = 16,384 -
    all 16,384 candidates, so every limit place keeps all of its 4,095 .. 8,193 raters - has
    its neighbour list taken from `query` and handed back.  Catches: a host-weights path that sums in another order or
    misses a segment or the one-place finish tile where the request itself does not (places and estimates must equal
    `recommend` at the same K bit for bit), and a count or rows that the single-column kernels lose."""
    _, meta = lc.main_index()
    q, k = meta["query"][lc.AGG_FAMILY], 16384
    pid = int(main.d["person_ids"][q])
    ids, sims = main.ix.query(pid, 0.5, 0.5, k)
    assert len(ids) == k > 1024
    places, est = main.ix.recommend_neighbours(ids, sims)
    rplaces, rest = main.ix.recommend(pid, 0.5, 0.5, k)
    assert np.array_equal(places, rplaces) and np.array_equal(est, rest), "not the single request's bits"
    op, oe = main.recommend(q, lc.HALF, k)
    assert np.array_equal(places, op), "places differ from the oracle"
    np.testing.assert_allclose(est, oe, rtol=RTOL, atol=0)


def small_rows(d, pids):
    at = {int(p): r for r, p in enumerate(d["person_ids"])}
    return np.array([at[int(p)] for p in pids])


def test_all_pairs_in_creation_order(small):
    """all_pairs_topk at K = 1,025 walks the persons in creation order, 16 a tile: persons 16 .. 31 have no category
    vector (a tile with no valid query at all), so have 15 (the last slot of a tile), 32 (the first of the next) and the
    last person.  Catches: a tile of absent queries that reads a segment of size 0 at `K - 1`, keeps the previous tile's
    lists or counts, or skips its padding; count 0 for -1."""
    d, k = small.d, lc.SMALL_K
    before = small.ix.query_batch(d["person_ids"][40:90], 0.5, 0.5, 50)
    ids, sims, cnt = small.ix.all_pairs_topk(0.5, 0.5, k)
    bad = np.array(lc.SMALL_INVALID)
    assert np.all(cnt[bad] == -1) and np.all(ids[bad] == -1) and np.all(sims[bad] == 0.0)
    good = np.setdiff1d(np.arange(lc.SMALL_N), bad)
    check_rows(ids[good], sims[good], cnt[good], *small.rows(good, lc.HALF, k), k, "all pairs")
    assert np.all(cnt[good] == k)
    after = small.ix.query_batch(d["person_ids"][40:90], 0.5, 0.5, 50)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("nq", [33, 17])
def test_ranges_that_start_with_an_invalid_tile(small, nq):
    """The range forms walk the index's own row order, where the 19 persons without a category vector come first: the
    range [0, 33) has a first tile with no valid query, a second of 3 absent and 13 valid ones and a last tile of ONE
    query; [0, 17) ends with a tile whose only query is absent.  topk_range_async + fetch_topk: count -1 and padding for
    the absent, the oracle's rows for the others; recommend_range_async + fetch_recommend: no rows for the absent, the
    batch's bits and the oracle's places for the others (the 14 valid queries of [0, 33); in [0, 17) every query is
    absent, so that range checks the counts of -1, the padding and the empty rows alone).  Catches: offsets of an all-absent tile not written (the rows of
    the next tile land at a stale offset), `nt` of the last tile taken as 16."""
    d, k = small.d, lc.SMALL_K
    qids = small.ix.row_person_ids(0, nq)
    absent_ids = d["person_ids"][list(lc.SMALL_INVALID)]
    absent = np.isin(qids, absent_ids)
    assert absent[:19].all() and not absent[19:].any(), "the absent persons must fill the first tile of the range"
    rows = small_rows(d, qids)
    pids50 = d["person_ids"][100:140]
    before = small.ix.query_batch(pids50, 0.5, 0.5, 50), small.ix.recommend_batch(pids50, 0.5, 0.5, 50)
    small.ix.topk_range_async(0, nq, 0.5, 0.5, k)
    ids, sims, cnt = small.ix.fetch_topk(nq, k)
    assert np.all(cnt[absent] == -1) and np.all(ids[absent] == -1) and np.all(sims[absent] == 0.0)
    if (~absent).any():
        check_rows(ids[~absent], sims[~absent], cnt[~absent], *small.rows(rows[~absent], lc.HALF, k), k, "range")
    small.ix.recommend_range_async(0, nq, 0.5, 0.5, k)
    off, places, est = small.ix.fetch_recommend(nq)
    assert off[0] == 0 and off[-1] == len(places)
    assert np.all(np.diff(off)[absent] == 0), "a person that is not a valid query must get no rows"
    for j in np.flatnonzero(~absent):
        op, oe = small.recommend(rows[j], lc.HALF, k)
        assert np.array_equal(places[off[j]:off[j + 1]], op), j
        np.testing.assert_allclose(est[off[j]:off[j + 1]], oe, rtol=RTOL, atol=0)
    if (~absent).any():
        boff, bplaces, best = small.ix.recommend_batch(qids[~absent], 0.5, 0.5, k)
        assert np.array_equal(np.diff(off)[~absent], np.diff(boff))
        assert np.array_equal(places, bplaces) and np.array_equal(est, best)
        check_recommend_single(small.ix, qids[~absent], 0.5, 0.5, k, boff, bplaces, best)
    after = small.ix.query_batch(pids50, 0.5, 0.5, 50), small.ix.recommend_batch(pids50, 0.5, 0.5, 50)
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), "a K = 50 batch changed after the tiled ranges"
