"""CPU: the cases of knn_large_limit_cases stand where they claim.  The selection of knn_large.hip is restated there in
numpy from the oracle's similarities; here every listed (query, K) is shown to hit the planted segment, runs, passes,
deciding bin, `above` and candidate count exactly, and the closed-form neighbour list is shown to be the oracle's answer
on the full data (ids equal, similarities bit-equal).  Expected values never come from the library under test."""
import os

import numpy as np
import pytest

import knn_large_limit_cases as lc

THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
CASES = lc.cases()


def oracle_list(oracle, row, k, weights):
    d, _ = lc.main_index()
    ids, sims, cnt = oracle.knn_similar_batch(d, np.array([row], np.int64), weights[0], weights[1], k)
    return ids[0, :cnt[0]], sims[0, :cnt[0]]


def test_the_restatement_on_hand_made_populations():
    """selection() on populations counted by hand: K inside the top bin, K at the last entry of a bin, at the first entry
    of the next, in bin 0, and K >= the total (b* = 0, above = total - pop(0), as lkt_select reports it)."""
    s = np.r_[np.full(10, 1.0), np.full(5, 0.75 + 1e-9), np.full(3, 1e-5)]      # bins 4095 (clamped), 3072, 0
    assert lc.bin_of([1.0, 0.999999, 0.75, 1.0 / 4096, 0.99 / 4096]).tolist() == [4095, 4095, 3072, 1, 0]
    for k, want in ((1, (4095, 0, 10)), (10, (4095, 0, 10)), (11, (3072, 10, 15)), (15, (3072, 10, 15)), (16, (0, 15, 18)),
                    (17, (0, 15, 18)), (18, (0, 15, 18)), (19, (0, 15, 18))):
        f = lc.selection(s, k)
        assert (f["bstar"], f["above"], f["segment"]) == want, k
        assert f["all"] == (k >= 18) and f["m"] == min(k, 18)
    for segment, runs, passes in ((1, 1, 0), (8192, 1, 0), (8193, 2, 1), (16384, 2, 1), (16385, 3, 2), (24577, 4, 2),
                                  (32768, 4, 2), (32769, 5, 3), (65537, 9, 4)):
        f = lc.selection(np.full(segment, 0.5), segment + 1)
        assert (f["runs"], f["passes"]) == (runs, passes), segment


def test_the_tables_are_the_limits():
    """The listed segments and Ks are the limits themselves: R, R + 1, 2R, 2R + 1, 3R + 1, 4R + 1 with R = 8,192; K = R,
    2R, the candidate count and its neighbours; every K beyond the LDS lists (1,024)."""
    assert [t[0] for t in lc.RUN_TABLE.values()] == [8192, 8193, 16384, 16385, 24577, 32769]
    assert lc.RUN_TABLE["run8192"][1] == (1025, 8191, 8192) and lc.RUN_TABLE["run8193"][1] == (1025, 8192, 8193)
    assert lc.RUN_TABLE["run16384"][1] == (8193, 16383, 16384) and lc.RUN_TABLE["run16385"][1] == (16384, 16385)
    assert lc.RUN_TABLE["run24577"][1] == (8193, 24577) and lc.RUN_TABLE["run32769"][1] == (1025, 8194, 32768, 32769)
    assert [(t[2], t[3]) for t in lc.RUN_TABLE.values()] == [(1, 0), (2, 1), (2, 1), (3, 2), (4, 2), (5, 3)]
    assert lc.CAND_KS == (lc.CAND - 1, lc.CAND, lc.CAND + 1) == (1029, 1030, 1031)
    assert all(c["k"] > 1024 for c in CASES) and len(CASES) == 35
    # the bins: 4t + 3 and 4t + 1 of one thread's range, 4t of the same range (the walk's fall-through), a 4t alone in
    # its range, the clamped top bin and bin 0; K at the first and the last entry of each (1,025 for K = 1 of the top bin)
    bins = [b for _, b, _, _ in lc.BIN_TABLE][::2]
    assert bins == [4095, 3699, 3697, 3696, 3652, 0]
    assert (3699 // 4, 3699 % 4, 3697 // 4, 3697 % 4, 3696 // 4, 3696 % 4, 3652 % 4) == (924, 3, 924, 1, 924, 0, 0)
    for (k0, b0, a0, s0), (k1, b1, a1, s1) in zip(lc.BIN_TABLE[::2], lc.BIN_TABLE[1::2]):
        assert (b0, a0, s0) == (b1, a1, s1) and k1 == s1 and k0 == max(a0 + 1, 1025), (k0, k1)


def test_the_index_is_what_the_module_says():
    """About 110,000 persons; families on disjoint indices; person ids unique and shuffled; the rows of every group of a
    run family spread over the whole table: each eighth of the rows holds its share of each group of 2,500 or more."""
    d, meta = lc.main_index()
    n = len(d["person_ids"])
    assert n == 109_676 and len(np.unique(d["person_ids"])) == n
    assert not np.array_equal(np.argsort(d["person_ids"]), np.arange(n))
    fam = meta["fam_of_row"]
    for name, prefix, per in (("p", "p", lc.P_PER), ("c", "c", lc.C_PER)):
        row_of = np.repeat(np.arange(n), np.diff(d[prefix + "_rowptr"]))
        assert np.array_equal(d[prefix + "_idx"] // per, fam[row_of]), name
    assert np.all(np.diff(d["p_rowptr"]) == 3)
    # the index orders its rows stably by (places, categories, head places): every place index is a head index here, so
    # the third key equals the first.  The spread is asserted on THAT order, which is what a segment is collected in.
    order = np.lexsort((np.diff(d["c_rowptr"]), np.diff(d["p_rowptr"])))
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    for (f, g), rows in meta["members"].items():
        if len(rows) >= 2500:
            share = np.bincount(pos[rows] * 8 // n, minlength=8) / len(rows)
            assert share.min() > 0.09 and share.max() < 0.16, (f, g, share)
    for name, (segment, _, runs, _, _) in lc.RUN_TABLE.items():          # every full LDS run holds every group of the family
        cand = lc.candidates(meta["query"][name])[0]
        cand = cand[np.argsort(pos[cand])]
        assert np.all(np.diff(d["c_rowptr"])[cand] == 1), "one family, one length: the rows keep their shuffled order"
        groups = [g for g in set(meta["pat_of_row"][cand].tolist()) if np.sum(meta["pat_of_row"][cand] == g) >= 190]
        assert len(groups) >= 2
        for r0 in range(0, segment - segment % 8192, 8192):
            assert set(groups) <= set(meta["pat_of_row"][cand[r0:r0 + 8192]].tolist()), (name, r0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_hits_its_limit(oracle, case):
    """The restated selection gives exactly the planted candidate count, segment, runs, passes, b* and `above`; the
    closed-form list (groups by similarity descending, person id ascending) is the oracle's on the full data."""
    f = lc.facts(case["row"], case["k"], case["weights"])
    for key, want in case["planted"].items():
        assert f[key] == want, (key, f[key], want)
    rows, ids, sims = lc.expected(case["row"], case["k"], case["weights"])
    oids, osims = oracle_list(oracle, case["row"], case["k"], case["weights"])
    assert len(ids) == f["m"] == len(oids)
    assert np.array_equal(ids, oids), "the closed form's ids differ from the oracle's"
    assert np.array_equal(sims, osims), "the closed form's similarities differ from the oracle's bits"
    d, _ = lc.main_index()
    assert np.array_equal(d["person_ids"][rows], ids)


def test_run_families_hold_two_similarities_in_one_bin():
    """Every run family: all candidates in one bin, at least three distinct similarities inside it; every listed K below
    the segment cuts inside a group of equal similarities (by person id) - but run24577 at K = 8,193, which ends exactly
    on the last entry of a group whose neighbour group stands one ulp below."""
    _, meta = lc.main_index()
    for name, (segment, ks, _, _, bstar) in lc.RUN_TABLE.items():
        _, ids, sims = lc.candidates(meta["query"][name])
        assert len(sims) == segment and set(lc.bin_of(sims).tolist()) == {bstar}
        assert len(np.unique(sims)) >= 3, name
        for k in ks:
            if k < segment:
                _, eids, esims = lc.expected(meta["query"][name], k)
                tie = ids[sims == esims[-1]]
                inside = np.sum(tie <= eids[-1]) < len(tie)
                assert inside != ((name, k) == ("run24577", 8193)), (name, k)
    _, eids, esims = lc.expected(meta["query"]["run24577"], 8194)
    assert esims[-2] - esims[-1] == np.spacing(esims[-1]), "the group behind K = 8,193 stands one ulp below"
    sims = lc.candidates(meta["query"]["run8193"])[2]
    u = np.unique(sims)
    assert np.min(np.diff(u)) == np.spacing(u[np.argmin(np.diff(u))]), "two groups of run8193 stand one ulp apart"


def test_bins_family_lands_where_planted():
    """Under pw = 2^-12: 1,100 twins at s = 1.0 exactly (int(s * 4096) = 4096, clamped to 4095), 300 / 200 / 250 in bins
    3699 / 3697 / 3696 (thread 924's range, 3698 empty), 150 in bin 3652 (thread 913's lowest bin, the other three empty)
    and 120 in bin 0 with s < 1 / 4096."""
    _, meta = lc.main_index()
    assert sum(lc.TINY_PW) == 1.0
    _, _, sims = lc.candidates(meta["query"]["bins"], lc.TINY_PW)
    pop = np.bincount(lc.bin_of(sims), minlength=lc.BINS)
    assert {int(b): int(pop[b]) for b in np.flatnonzero(pop)} == {4095: 1100, 3699: 300, 3697: 200, 3696: 250, 3652: 150, 0: 120}
    assert np.sum(sims == 1.0) == 1100 and int(1.0 * 4096) == 4096
    assert 0 < sims.min() and sims[lc.bin_of(sims) == 0].max() < 1.0 / 4096


@pytest.mark.parametrize("nq", [16, 17, 33])
def test_mixed_tile(oracle, nq):
    """One batch holds a query of every run family and small ones: the columns of its first tile need 0, 1, 2 and 3 merge
    passes under one launch grid, at every K of the batch (the run families' segments are one bin: they keep their size
    at any K).  17 and 33 queries: 16 / 32 distinct ones, one given twice, not in row order; the first tile is the mixed
    one, the second full tile of the 33 is mixed too at the largest K, the last tile holds one query.  The closed form of
    every query equals the oracle at the batch's largest K (smaller Ks are its prefixes)."""
    rows = lc.mixed_rows(nq)
    assert len(rows) == nq and len(set(rows.tolist())) == (16 if nq <= 17 else 32)
    assert nq == 16 or not np.array_equal(np.sort(rows), rows)
    d, _ = lc.main_index()
    k = max(lc.MIXED_KS[nq])
    assert lc.MIXED_KS[nq] == ((1025, 8193, 32769) if nq == 16 else (8193, 32769))
    assert sorted(rows[:16].tolist()) == sorted(lc.mixed_rows(16).tolist()), "the first tile is the mixed one"
    for kk in lc.MIXED_KS[nq]:
        segments = [lc.facts(r, kk)["segment"] for r in rows[:16]]
        assert {lc.facts(r, kk)["passes"] for r in rows[:16]} == {0, 1, 2, 3}, kk
        assert min(segments) == 5 and max(segments) == 32769 and {8192, 8193, 16384, 16385, 24577} <= set(segments), kk
        assert not all(lc.facts(r, kk)["all"] for r in rows[:16]) or kk == 32769, "a K below 32,769 cuts some column"
    if nq == 33:
        assert {lc.facts(r, k)["passes"] for r in rows[16:32]} == {0, 1, 2, 3}
    if nq > 16:
        assert len(rows[(nq - 1) // 16 * 16:]) == 1 and rows[-1] == rows[3], "the last tile holds the repeated query alone"
    oids, osims, ocnt = oracle.knn_similar_batch(d, rows, 0.5, 0.5, k, nthreads=THREADS)
    for j, r in enumerate(rows):
        _, ids, sims = lc.expected(int(r), k)
        assert ocnt[j] == len(ids) and np.array_equal(oids[j, :len(ids)], ids) and np.array_equal(osims[j, :len(ids)], sims), j


def test_ratings_stand_on_the_aggregation_limits(oracle):
    """Five places with exactly 4,095, 4,096, 4,097, 8,192 and 8,193 raters (1, 1, 2, 2 and 3 segments of 4,096), all in
    one family; exactly 2,049 distinct rated places (two finish tiles, the second of one place); for the family's query
    the places of rank 2,047 and 2,048 are both rated by neighbours, and K = 8,193 keeps some and drops some of each
    limit place's raters.  Three small queries: rows only for rank 2,048; none in the last finish tile; none at all."""
    d, meta = lc.main_index()
    places, counts = np.unique(d["r_place"], return_counts=True)
    assert len(places) == 2049 and np.array_equal(places, lc.place_id(np.arange(2049)))
    by_rank = dict(zip(lc.place_rank(places).tolist(), counts.tolist()))
    assert {r: by_rank[r] for r in lc.SPECIAL_RATERS} == {0: 4095, 1: 4096, 2: 4097, 3: 8192, 2046: 8193}
    assert [-(-c // 4096) for c in (4095, 4096, 4097, 8192, 8193)] == [1, 1, 2, 2, 3]
    assert set(np.unique(d["r_rating"]).tolist()) == {1, 2, 3, 4, 5}
    n = len(d["person_ids"])
    rater_row = np.repeat(np.arange(n), np.diff(d["r_rowptr"]))
    q = meta["query"][lc.AGG_FAMILY]
    fam = meta["fam_of_row"]
    for rank in lc.SPECIAL_RATERS:
        raters = rater_row[d["r_place"] == lc.place_id(rank)]
        assert np.all(fam[raters] == fam[q]) and q not in raters
        per_rating = np.bincount(d["r_rating"][d["r_place"] == lc.place_id(rank)], minlength=6)[1:]
        assert per_rating.min() > 0, "rating values vary by person"
        kept = np.isin(raters, lc.expected(q, 8193)[0]).sum()
        assert 0 < kept < len(raters), (rank, kept)
    for k in lc.AGG_KS:
        got = lc.expected_places(q, k)
        ranks = lc.place_rank(got)
        assert {0, 1, 2, 3, 2046, 2047, 2048} <= set(ranks.tolist()), k
        assert sorted(set((ranks // 2048).tolist())) == [0, 1]
        oplaces, _ = oracle.knn_recommend(d, int(d["person_ids"][q]), 0.5, 0.5, k)
        assert np.array_equal(got, oplaces), k
    for name, want_ranks, tiles in (("only2048", [2048], [1]), ("tile0", [5, 2047], [0]), ("norows", [], [])):
        got = lc.expected_places(meta["query"][name], 1025)
        assert lc.place_rank(got).tolist() == want_ranks and sorted(set((lc.place_rank(got) // 2048).tolist())) == tiles
        oplaces, _ = oracle.knn_recommend(d, int(d["person_ids"][meta["query"][name]]), 0.5, 0.5, 1025)
        assert np.array_equal(got, oplaces), name


def test_whole_index_ks():
    """K = n - 2 is the largest K that still takes the tiled top-K; n - 1 and the shipped 2,000,000 take no top-K at all.
    Every family is far smaller than n - 2: every candidate is a neighbour at all three."""
    d, meta = lc.main_index()
    n = len(d["person_ids"])
    assert n - 2 > 32769 + 1 and 2_000_000 > n - 1
    assert lc.facts(meta["query"]["run32769"], n - 2)["all"]


def test_small_index_in_creation_order(oracle):
    """1,100 persons; 16 .. 31 have no category vector (a whole tile of the all-pairs form), so have 15 (the last slot of
    a tile), 32 and n - 1; they have one place and everybody else two or more, so the index's row order (ascending
    vector lengths) starts with exactly these 19.  Every valid query has n - 1 = 1,099 candidates, and K = 1,025 cuts
    inside a group of equal similarities for most of them."""
    d = lc.small_index()
    n = len(d["person_ids"])
    assert n == 1100 and lc.SMALL_K == 1025 < n - 1
    nc, npl = np.diff(d["c_rowptr"]), np.diff(d["p_rowptr"])
    assert np.flatnonzero(nc == 0).tolist() == list(lc.SMALL_INVALID) == list(range(15, 33)) + [1099]
    assert np.all(npl[list(lc.SMALL_INVALID)] == 1) and np.all(np.delete(npl, list(lc.SMALL_INVALID)) >= 2)
    order = np.lexsort((nc, npl))                                  # (places, categories) ascending, stable
    assert sorted(order[:19].tolist()) == list(lc.SMALL_INVALID)
    valid = np.flatnonzero(nc > 0)
    ids, sims, cnt = oracle.knn_similar_batch(d, valid, 0.5, 0.5, 1099, nthreads=THREADS)
    assert np.all(cnt == 1099)
    inside = np.sum(sims[:, 1024] == sims[:, 1025])
    assert inside > len(valid) // 2, inside
