"""Batched KNN at any K: the batch entry points with k_nearest beyond the per-query LDS lists
(LOCREC_KNN_BATCH_MAX_K = 1024) take the tiled top-K of knn_large.hip - per column of a 16-query tile the deciding
histogram bin, a segment of the candidates at or above it, LDS-sorted runs and merge passes in global memory.

The reference takes any kNearest (KnnRecommender.scala:15,20,47-48) and ships --k-nearest 2000000
(bin/knn_recommender.sh:35).  Bars: neighbour ids equal to the oracle's, similarities bit-identical, estimates within
1e-6 of the oracle and bit-identical to the single request."""
import os

import numpy as np
import pytest

from test_gpu_configs import bench_knn_input
from test_gpu_knn import make_index, sharded_request, with_ratings
from test_gpu_row_fallback import widen

pytestmark = pytest.mark.gpu
RTOL = 1e-6
THREADS = max(1, min(32, len(os.sched_getaffinity(0))))


def oracle_rows(oracle, d, rows, pw, cw, k):
    return oracle.knn_similar_batch(d, np.asarray(rows, np.int64), pw, cw, k, nthreads=THREADS)


def check_rows(ids, sims, cnt, oids, osims, ocnt, k, what):
    """Each row equals the oracle's, with its count and the (-1, 0.0) padding behind it."""
    assert ids.shape == sims.shape == (len(cnt), k)
    for j in range(len(cnt)):
        c = int(cnt[j])
        assert c == int(ocnt[j]), (what, j, c, int(ocnt[j]))
        assert np.array_equal(ids[j, :c], oids[j, :c]), (what, j, "neighbour ids differ from the oracle")
        assert np.array_equal(sims[j, :c], osims[j, :c]), (what, j, "similarities differ from the oracle bit-wise")
        assert np.all(ids[j, c:] == -1) and np.all(sims[j, c:] == 0.0), (what, j, "padding")


def check_single(ix, pids, pw, cw, k, ids, sims, cnt):
    """Each row equals the single request (locrec_knn_query)."""
    for j, pid in enumerate(pids):
        a, b = ix.query(int(pid), pw, cw, k)
        c = int(cnt[j])
        assert c == len(a) and np.array_equal(ids[j, :c], a) and np.array_equal(sims[j, :c], b), (k, j)


def check_recommend_single(ix, pids, pw, cw, k, off, places, est):
    for j, pid in enumerate(pids):
        p1, e1 = ix.recommend(int(pid), pw, cw, k)
        assert np.array_equal(p1, places[off[j]:off[j + 1]]), (k, j)
        assert np.array_equal(e1, est[off[j]:off[j + 1]]), (k, j, "estimates differ from the single request's bits")


def test_query_batch_any_k(pkg, oracle):
    """locrec_knn_query_batch at K beyond the LDS lists: shuffled input order with a duplicate, K cutting below and
    above one LDS run (8,192), K = N - 2, N - 1 and the shipped 2,000,000 (clamped to N - 1, H4)."""
    from locations_recommender_amd import synth
    n = 20_000
    d = synth.knn_dataset(n, 2_000, seed=31)
    ix = make_index(pkg, d)
    rng = np.random.default_rng(5)
    rows = rng.permutation(np.r_[rng.choice(n - 1, 39, replace=False), [n - 1]])
    rows = np.r_[rows, rows[7]]                                          # 41 queries, one twice
    pids = d["person_ids"][rows]
    for k in (1_025, 4_097, 8_193, n - 2, n - 1):
        ids, sims, cnt = ix.query_batch(pids, 0.5, 0.5, k)
        oids, osims, ocnt = oracle_rows(oracle, d, rows, 0.5, 0.5, k)
        check_rows(ids, sims, cnt, oids, osims, ocnt, k, k)
        check_single(ix, pids[::5], 0.5, 0.5, k, ids[::5], sims[::5], cnt[::5])
        assert np.array_equal(ids[7], ids[-1]) and np.array_equal(sims[7], sims[-1])
    k = 2_000_000
    ids, sims, cnt = ix.query_batch(pids[:3], 0.25, 0.75, k)
    oids, osims, ocnt = oracle_rows(oracle, d, rows[:3], 0.25, 0.75, k)
    check_rows(ids, sims, cnt, oids, osims, ocnt, k, k)
    check_single(ix, pids[:3], 0.25, 0.75, k, ids, sims, cnt)
    # the LDS path below the limit
    ids, sims, cnt = ix.query_batch(pids, 0.5, 0.5, 1_024)
    oids, osims, ocnt = oracle_rows(oracle, d, rows, 0.5, 0.5, 1_024)
    check_rows(ids, sims, cnt, oids, osims, ocnt, 1_024, 1_024)
    with pytest.raises(pkg.IllegalArgumentException, match="No such person"):
        ix.query_batch([10**12], 0.5, 0.5, 5_000)
    ix.close()


def tie_dataset(n=40_000, patterns=40, seed=3):
    """n persons built from `patterns` distinct (place, category) vectors; half of them share pattern 0, so a query
    sees groups of exactly equal similarities far larger than one LDS run.  Person ids are shuffled against the rows."""
    rng = np.random.default_rng(seed)
    pats_p, pats_c = [], []
    for j in range(patterns):
        pi = np.unique(np.r_[0, rng.choice(np.arange(1, 200), 4 + j % 5, replace=False)]).astype(np.int32)
        ci = np.unique(np.r_[0, rng.choice(np.arange(1, 20), 1 + j % 3, replace=False)]).astype(np.int32)
        pats_p.append((pi, rng.integers(1, 9, len(pi)).astype(np.float64)))
        pats_c.append((ci, rng.integers(1, 5, len(ci)).astype(np.float64)))
    who = np.where(np.arange(n) % 2 == 0, 0, (np.arange(n) // 2) % (patterns - 1) + 1)
    prp, pidx, pval, crp, cidx, cval = [0], [], [], [0], [], []
    for p in who:
        pidx.append(pats_p[p][0]); pval.append(pats_p[p][1]); prp.append(prp[-1] + len(pats_p[p][0]))
        cidx.append(pats_c[p][0]); cval.append(pats_c[p][1]); crp.append(crp[-1] + len(pats_c[p][0]))
    d = {"person_ids": (rng.permutation(n) * 3 + 1_000).astype(np.int64),
         "p_rowptr": np.array(prp, np.int64), "p_idx": np.concatenate(pidx), "p_val": np.concatenate(pval), "p_dim": 200,
         "c_rowptr": np.array(crp, np.int64), "c_idx": np.concatenate(cidx), "c_val": np.concatenate(cval), "c_dim": 20}
    return with_ratings(d), who


def test_ties_across_the_cut(pkg, oracle):
    """K cutting inside a tie group of ~20,000 equal similarities: the group is ordered by person id ascending (H1)
    through the merge passes; recommendations select the same persons as the single request."""
    d, who = tie_dataset()
    n = len(who)
    ix = make_index(pkg, d)
    rows = np.r_[np.flatnonzero(who == 0)[:5], np.flatnonzero(who == 5)[:5], np.flatnonzero(who == 17)[:3]]
    pids = d["person_ids"][rows]
    for k in (5_000, 10_000, 19_998, 25_000, n - 1):
        ids, sims, cnt = ix.query_batch(pids, 0.5, 0.5, k)
        oids, osims, ocnt = oracle_rows(oracle, d, rows, 0.5, 0.5, k)
        check_rows(ids, sims, cnt, oids, osims, ocnt, k, k)
        check_single(ix, pids[::4], 0.5, 0.5, k, ids[::4], sims[::4], cnt[::4])
    for k in (5_000, 10_000):
        off, places, est = ix.recommend_batch(pids, 0.5, 0.5, k)
        check_recommend_single(ix, pids, 0.5, 0.5, k, off, places, est)
        for j in (0, 6):
            op, oe = oracle.knn_recommend(d, int(pids[j]), 0.5, 0.5, k)
            assert np.array_equal(places[off[j]:off[j + 1]], op)
            np.testing.assert_allclose(est[off[j]:off[j + 1]], oe, rtol=RTOL, atol=0)
    ix.close()


def test_other_formats(pkg, oracle):
    """A GENERIC (fp64) index and an index with wide rows (the per-row fallback, counts >= 256) at K = 3,000: the
    batch equals the single queries and the oracle."""
    from locations_recommender_amd import synth
    g = synth.small_knn_dataset(n=5_000, p_dim=600, seed=12, integer=False)
    ix = make_index(pkg, g)
    assert not ix.info()["packed"]
    rows = np.arange(3, 5_000, 157)
    pids = g["person_ids"][rows]
    ids, sims, cnt = ix.query_batch(pids, 0.4, 0.6, 3_000)
    check_rows(ids, sims, cnt, *oracle_rows(oracle, g, rows, 0.4, 0.6, 3_000), 3_000, "generic")
    check_single(ix, pids, 0.4, 0.6, 3_000, ids, sims, cnt)
    ix.close()
    wide = np.array([3, 777, 4_000, 6_001])
    w = widen(synth.knn_dataset(8_000, 800, seed=4), wide)
    ix = make_index(pkg, w)
    rows = np.r_[wide, np.arange(11, 8_000, 400)]
    pids = w["person_ids"][rows]
    ids, sims, cnt = ix.query_batch(pids, 0.5, 0.5, 3_000)
    check_rows(ids, sims, cnt, *oracle_rows(oracle, w, rows, 0.5, 0.5, 3_000), 3_000, "wide")
    check_single(ix, pids, 0.5, 0.5, 3_000, ids, sims, cnt)
    ix.close()


def strip_categories(d, rows):
    """The listed persons lose their category vector: candidates of the others, but no valid query (:77-83)."""
    d = dict(d)
    keep = np.ones(len(d["c_idx"]), bool)
    for r in rows:
        keep[d["c_rowptr"][r]:d["c_rowptr"][r + 1]] = False
    lens = np.diff(d["c_rowptr"])
    lens[list(rows)] = 0
    crp = d["c_rowptr"].copy()
    crp[1:] = np.cumsum(lens)
    d["c_rowptr"], d["c_idx"], d["c_val"] = crp, d["c_idx"][keep], d["c_val"][keep]
    return d


def test_range_and_all_pairs_forms(pkg, oracle):
    """topk_range_async + fetch_topk at K = 5,000 over ranges holding persons without a category vector (count -1,
    padded); all_pairs_topk at K = 1,500 on 2,500 persons, in input order."""
    from locations_recommender_amd import synth
    n, k = 9_000, 5_000
    d = strip_categories(synth.knn_dataset(n, 700, seed=9), (10, 20))
    ix = make_index(pkg, d)
    qids_all = ix.row_person_ids(0, n)
    absent = (int(d["person_ids"][10]), int(d["person_ids"][20]))
    for r in (10, 20):
        j = int(np.flatnonzero(qids_all == d["person_ids"][r])[0])
        first = max(0, min(n - 24, j - 11))
        ix.topk_range_async(first, 24, 0.5, 0.5, k)
        ids, sims, cnt = ix.fetch_topk(24, k)
        for i, pid in enumerate(qids_all[first:first + 24]):
            if int(pid) in absent:
                assert cnt[i] == -1 and np.all(ids[i] == -1) and np.all(sims[i] == 0.0), "not a valid query"
                continue
            a, b = ix.query(int(pid), 0.5, 0.5, k)
            assert cnt[i] == len(a) and np.array_equal(ids[i, :len(a)], a) and np.array_equal(sims[i, :len(a)], b), i
            assert np.all(ids[i, len(a):] == -1) and np.all(sims[i, len(a):] == 0.0)
    ix.close()
    small = strip_categories(synth.knn_dataset(2_500, 300, seed=13), (7,))
    ix = make_index(pkg, small)
    ids, sims, cnt = ix.all_pairs_topk(0.5, 0.5, 1_500)
    assert cnt[7] == -1 and np.all(ids[7] == -1)
    rows = np.r_[np.arange(0, 7), np.arange(8, 2_500)]
    oids, osims, ocnt = oracle_rows(oracle, small, rows, 0.5, 0.5, 1_500)
    check_rows(ids[rows], sims[rows], cnt[rows], oids, osims, ocnt, 1_500, "all pairs")
    ix.close()


def test_sharded_request_any_k(pkg, oracle):
    """locrec_knn_query_shard beyond the LDS lists: 3 candidate shards merged by shard.merge_local_topk equal the
    unsharded request and the oracle."""
    from locations_recommender_amd import synth
    n = 12_000
    d = synth.knn_dataset(n, 900, seed=23)
    ix = make_index(pkg, d)
    for r in (0, 5_555, n - 1):
        pid = int(d["person_ids"][r])
        for k in (1_500, 2_000_000):
            ids, sims = sharded_request(pkg, ix, pid, 0.5, 0.5, k, 3)
            uid, usim = ix.query(pid, 0.5, 0.5, k)
            assert np.array_equal(ids, uid) and np.array_equal(sims, usim), (r, k)
            oids, osims, ocnt = oracle_rows(oracle, d, [r], 0.5, 0.5, min(k, n - 1))
            assert np.array_equal(ids, oids[0, :ocnt[0]]) and np.array_equal(sims, osims[0, :ocnt[0]]), (r, k)
    ix.close()


def test_replicas_any_k(pkg):
    """KnnReplicas over the device list [0, 0] at K = 3,000 equals the single-device batch."""
    from locations_recommender_amd import synth
    d = synth.knn_dataset(7_000, 600, seed=17)
    ix = make_index(pkg, d)
    rep = pkg.KnnReplicas([0, 0], d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"],
                          d["c_rowptr"], d["c_idx"], d["c_val"], d["c_dim"])
    pids = d["person_ids"][np.arange(5, 7_000, 173)]
    a = ix.query_batch(pids, 0.5, 0.5, 3_000)
    b = rep.query_batch(pids, 0.5, 0.5, 3_000)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    rep.close()
    ix.close()


def test_recommend_batch_any_k(pkg, oracle):
    """locrec_knn_recommend_batch and the range form for 1024 < K < N - 1: every query bit-identical to the single
    request and within 1e-6 of the oracle; the range form equals the batch; persons that are not valid queries get no
    rows; a K = 50 batch and a single request on the same handle are unchanged afterwards."""
    from locations_recommender_amd import synth
    n = 6_000
    d = with_ratings(strip_categories(synth.knn_dataset(n, 800, seed=27), (33,)))
    ix = make_index(pkg, d)
    rows = np.r_[np.arange(1, n, 211), [n - 1, 40, 40]]
    pids = d["person_ids"][rows]
    before = ix.recommend_batch(pids, 0.5, 0.5, 50)
    before1 = ix.recommend(int(pids[2]), 0.5, 0.5, 50)
    qids_all = ix.row_person_ids(0, n)
    j33 = int(np.flatnonzero(qids_all == d["person_ids"][33])[0])
    first = max(0, min(n - 40, j33 - 20))
    qids = qids_all[first:first + 40]
    valid = qids != d["person_ids"][33]
    for k in (1_025, 5_000, n // 2):
        off, places, est = ix.recommend_batch(pids, 0.5, 0.5, k)
        check_recommend_single(ix, pids, 0.5, 0.5, k, off, places, est)
        for j in range(0, len(pids), 4):
            op, oe = oracle.knn_recommend(d, int(pids[j]), 0.5, 0.5, k)
            assert np.array_equal(places[off[j]:off[j + 1]], op), (k, j)
            np.testing.assert_allclose(est[off[j]:off[j + 1]], oe, rtol=RTOL, atol=0)
        ix.recommend_range_async(first, 40, 0.5, 0.5, k)
        roff, rplaces, rest = ix.fetch_recommend(40)
        boff, bplaces, best = ix.recommend_batch(qids[valid], 0.5, 0.5, k)
        rlen = np.diff(roff)
        assert rlen[~valid].tolist() == [0], "a person that is not a valid query must get no rows"
        assert np.array_equal(rlen[valid], np.diff(boff))
        assert np.array_equal(rplaces, bplaces) and np.array_equal(rest, best)
    after = ix.recommend_batch(pids, 0.5, 0.5, 50)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    after1 = ix.recommend(int(pids[2]), 0.5, 0.5, 50)
    assert np.array_equal(before1[0], after1[0]) and np.array_equal(before1[1], after1[1])
    ix.close()


def test_steady_state_allocations(pkg):
    """A repeated mid-K batch of the same shape allocates nothing: the workspaces are grow-only handle members."""
    from locations_recommender_amd import synth, _lib
    d = with_ratings(synth.knn_dataset(10_000, 900, seed=29))
    ix = make_index(pkg, d)
    pids = d["person_ids"][np.arange(0, 10_000, 199)]
    first = (ix.query_batch(pids, 0.5, 0.5, 4_000), ix.recommend_batch(pids, 0.5, 0.5, 4_000))
    n0 = _lib.device_allocations()
    again = (ix.query_batch(pids, 0.5, 0.5, 4_000), ix.recommend_batch(pids, 0.5, 0.5, 4_000))
    assert _lib.device_allocations() == n0, "a repeated batch of the same shape allocated device memory"
    for a, b in zip(first, again):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    ix.close()


def test_cfg2_any_k_full_size(pkg, oracle):
    """configs[1] (1 M persons x 100 k places): query_batch of 32 at K = 5,000 and recommend_range_async of 64 at
    K = 100,000, sampled against the oracle; the range form equals the batch."""
    n = 1_000_000
    d = bench_knn_input(n, 100_000, 0x5EED0002)
    ix = make_index(pkg, d)
    rows = np.linspace(0, n - 1, 32).astype(np.int64)
    ids, sims, cnt = ix.query_batch(d["person_ids"][rows], 0.5, 0.5, 5_000)
    sample = np.array([0, 9, 20, 31])
    oids, osims, ocnt = oracle_rows(oracle, d, rows[sample], 0.5, 0.5, 5_000)
    check_rows(ids[sample], sims[sample], cnt[sample], oids, osims, ocnt, 5_000, "cfg2 query")
    first, k = 400_000, 100_000
    ix.recommend_range_async(first, 64, 0.5, 0.5, k)
    roff, rplaces, rest = ix.fetch_recommend(64)
    qids = ix.row_person_ids(first, 64)
    boff, bplaces, best = ix.recommend_batch(qids, 0.5, 0.5, k)
    assert np.array_equal(roff, boff) and np.array_equal(rplaces, bplaces) and np.array_equal(rest, best)
    for j in (0, 37):
        op, oe = oracle.knn_recommend(d, int(qids[j]), 0.5, 0.5, k)
        assert np.array_equal(rplaces[roff[j]:roff[j + 1]], op), j
        np.testing.assert_allclose(rest[roff[j]:roff[j + 1]], oe, rtol=RTOL, atol=0)
        p1, e1 = ix.recommend(int(qids[j]), 0.5, 0.5, k)
        assert np.array_equal(p1, op) and np.array_equal(e1, rest[roff[j]:roff[j + 1]])
    ix.close()


def test_cfg4_shipped_k_full_size(pkg, oracle):
    """configs[3] on one GPU (10 M persons x 1 M places): recommend_batch of 16 at the shipped K = 2,000,000, which is
    below N - 1 here and keeps its top-K meaning; 2 sampled queries against the oracle and the single request."""
    n = 10_000_000
    d = bench_knn_input(n, 1_000_000, 0x5EED0004)
    ix = make_index(pkg, d)
    rows = np.linspace(3, n - 4, 16).astype(np.int64)
    pids = d["person_ids"][rows]
    k = 2_000_000
    off, places, est = ix.recommend_batch(pids, 0.5, 0.5, k)
    for j in (0, 11):
        op, oe = oracle.knn_recommend(d, int(pids[j]), 0.5, 0.5, k)
        assert np.array_equal(places[off[j]:off[j + 1]], op), j
        np.testing.assert_allclose(est[off[j]:off[j + 1]], oe, rtol=RTOL, atol=0)
        p1, e1 = ix.recommend(int(pids[j]), 0.5, 0.5, k)
        assert np.array_equal(p1, op) and np.array_equal(e1, est[off[j]:off[j + 1]])
    ix.close()
