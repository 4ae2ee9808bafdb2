"""GPU: the segmented ranker (csrc/rank_batch.hip) on the limits of its chunk plan and of its two paths, and the ranked
KNN forms at the largest LDS list ("Limits of the rankers"; the inputs: rank_limit_cases.py, checked on the
CPU by test_rank_limit_cases.py).  Every comparison is rb.same against the oracle's single ranker per segment: ids,
counts and score bits are equal, because the ranker moves rows and computes nothing.  The limits are literals."""
import numpy as np
import pytest

import rank_batch_cases as rb
import rank_limit_cases as rl
from test_gpu_knn_ranked import CW, PW, expect, places_of, small  # noqa: F401 (small is a fixture)
from test_gpu_rank_batch import HOST_DEVICE, run

pytestmark = pytest.mark.gpu
DEFAULT_CHUNK = 4096
LIMITS = (1, 10, 256)


@pytest.fixture(scope="module")
def prep(pkg):
    return pkg.prep


_WANT = {}


def want(oracle, name, case, limit):
    """The oracle loop of one (case, limit): computed once, shared by the host and the device run."""
    if (name, limit) not in _WANT:
        _WANT[(name, limit)] = rb.expected(oracle.rank_recommendations, case, limit)
    return _WANT[(name, limit)]


# ---- the chunk plan at its boundaries -----------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", (None,) + rl.CHUNKS, ids=lambda c: "default" if c is None else str(c))
@HOST_DEVICE
def test_chunk_boundaries(prep, oracle, chunk, on_device, monkeypatch):
    """Segments of chunk - 1, chunk, chunk + 1, 2 chunk, 2 chunk + 1, 0, 3 chunk (in a region without places) and
    chunk + 1 rows: `len == chunk` is one block, `chunk + 1` has a second chunk of one row, `2 chunk` a last chunk that
    is exactly full; the segment that reads nothing lies between split ones and shifts the partial lists' slots.  A
    chunk's tiles start at the chunk's first row: a chunk of 255 rows is one partial tile, one of 257 a full tile and
    a tile of one row.
    Bites (tried): a chunk's end `r0 + chunk` read as `r0 + chunk - 1` in rb_select loses the planted best row at
    chunk - 1."""
    c = DEFAULT_CHUNK if chunk is None else chunk
    if chunk is not None:
        monkeypatch.setenv("LOCREC_RANK_BATCH_CHUNK", str(chunk))
    case = rl.chunk_case(rl.CHUNK_LENGTHS, c)
    assert np.diff(case["offsets"]).tolist() == [c - 1, c, c + 1, 2 * c, 2 * c + 1, 0, 3 * c, c + 1]
    for limit in LIMITS:
        got = run(prep, case, limit, on_device)
        st = prep.rank_recommendations_batch_stats()
        assert rb.same(got, want(oracle, ("chunk", c), case, limit)), limit
        assert (st["split"], st["chunks"], st["one_block"], st["sorted"]) == (4, 2 + 2 + 3 + 2, 8 - 4, 0), st
        planted = [s for s in range(8) if case["planted_row"][s] >= 0]
        assert got[0][planted, 0].tolist() == [case["planted_id"][s] for s in planted]
        assert (got[1][planted, 0].view(np.uint64) == rl.PLANTED_NAN).all()


@HOST_DEVICE
def test_every_row_a_chunk_of_its_own(prep, oracle, on_device, monkeypatch):
    """LOCREC_RANK_BATCH_CHUNK=1: 300 rows in 3 segments are 300 blocks with at most one entry each; a segment's answer
    is put together by rb_merge alone, from 100 partial lists of which two thirds are empty.
    Bites (tried): a chunk's end `r0 + chunk` read as `r0 + chunk - 1` (no chunk reads a row: every count is 0)."""
    monkeypatch.setenv("LOCREC_RANK_BATCH_CHUNK", "1")
    case = rl.chunk_case(rl.TINY_LENGTHS, 1)
    for limit in LIMITS:
        got = run(prep, case, limit, on_device)
        st = prep.rank_recommendations_batch_stats()
        assert rb.same(got, want(oracle, "tiny", case, limit)), limit
        assert (st["split"], st["chunks"], st["one_block"], st["sorted"]) == (3, 300, 0, 0), st
        assert got[2].tolist() == [min(limit, 34)] * 3


# ---- the global path ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", rl.GLOBAL_N)
@HOST_DEVICE
def test_global_path_around_the_emit_tiles(prep, oracle, N, on_device):
    """Segments with 0, N - 1, N, 3 N and N kept rows and two that the join empties, at N = 257 and around the second
    256-slot tile of rb_emit_sorted (511, 512, 513).
    Bites (tried): `j < have` read as `j + 1 < have` pads the last kept row of the segments with N - 1 and N rows."""
    case = rl.global_case(N)
    got = run(prep, case, N, on_device)
    st = prep.rank_recommendations_batch_stats()
    assert rb.same(got, want(oracle, "global", case, N))
    assert got[0].shape == (7, N) and got[2].tolist() == [0, N - 1, N, N, N, 0, 0]
    assert st["sorted"] == 7 and st["one_block"] == st["split"] == st["chunks"] == 0


@pytest.mark.parametrize("N", (10, 256))
def test_forced_global_path_equals_the_list(prep, oracle, N, monkeypatch):
    """The same segments through the LDS list (N = 10 and the largest, 256) and, under LOCREC_RANK_BATCH_SORT=1, through
    the global path: one result, the oracle's."""
    case = rl.global_case(N)
    listed = run(prep, case, N, True)
    assert prep.rank_recommendations_batch_stats()["sorted"] == 0
    monkeypatch.setenv("LOCREC_RANK_BATCH_SORT", "1")
    got = run(prep, case, N, True)
    assert prep.rank_recommendations_batch_stats()["sorted"] == 7
    assert rb.same(got, want(oracle, "global", case, N)) and rb.same(got, listed)
    assert got[2].tolist() == [0, N - 1, N, N, N, 0, 0]


@pytest.mark.parametrize("N,force", [(257, False), (5, True)], ids=["257", "forced-5"])
@HOST_DEVICE
def test_global_path_with_no_kept_row(prep, oracle, N, force, on_device, monkeypatch):
    """m = 0: no row of any segment is kept (some regions have places, whose segments are read and dropped, some have
    none), so nothing is sorted and rb_emit_sorted searches an array nobody wrote.
    Bites (tried): an early return for m = 0 that clears the output with zeros (the padding id is -1)."""
    if force:
        monkeypatch.setenv("LOCREC_RANK_BATCH_SORT", "1")
    case = rl.global_case(N, all_dropped=True)
    ids, scores, counts = run(prep, case, N, on_device)
    st = prep.rank_recommendations_batch_stats()
    assert rb.same((ids, scores, counts), want(oracle, "dropped", case, N))
    assert ids.shape == (7, N) and not counts.any() and (ids == -1).all() and not scores.view(np.uint64).any()
    assert st["sorted"] == 7


# ---- the ranked KNN forms at the largest list ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [50, 1500])
def test_knn_ranked_at_the_largest_list(pkg, oracle, small, k):
    """Limits 255 and 256 = LOCREC_RANK_BATCH_MAX_N: the last N that the LDS list serves (test_gpu_knn_ranked.py runs 10
    and 257).  Bites (tried): `N > LOCREC_RANK_BATCH_MAX_N` read as `>=` sends 256 to the global path (sorted > 0)."""
    d, ix = small
    places = places_of(d)[0]
    regions = places % 2                                     # about 300 places a region: a request can fill 256 entries
    rng = np.random.default_rng(k)
    valid = np.flatnonzero(np.diff(d["p_rowptr"]) > 0)
    rows = np.r_[rng.choice(valid, 30, replace=False), [valid[-1], valid[5], valid[5]]]
    persons = d["person_ids"][rows]
    targets = rng.choice([0, 1, 99], len(rows)).astype(np.int64)
    targets[-1], targets[-2] = 0, 1
    off, rp, re = ix.recommend_batch(persons, PW, CW, k)
    for limit in (255, 256):
        got = ix.recommend_ranked_batch(persons, PW, CW, k, places, regions, targets, limit)
        st = pkg.prep.rank_recommendations_batch_stats()
        wanted = expect(oracle, off, rp, re, places, regions, targets, limit)
        assert rb.same(got, wanted), limit
        assert st["sorted"] == 0 and st["host_assembled"] == 0 and st["one_block"] + st["split"] == len(rows)
        if k == 1500:
            assert wanted[2].max() == limit                  # requests with more rows than the list keeps
    nq, first = 48, 1180
    ix.recommend_range_async(first, nq, PW, CW, k)
    roff, rrp, rre = ix.fetch_recommend(nq)
    rt = rng.choice([0, 1], nq).astype(np.int64)
    for limit in (255, 256):
        ix.recommend_range_async(first, nq, PW, CW, k)
        got = ix.fetch_ranked(nq, places, regions, rt, limit)
        st = pkg.prep.rank_recommendations_batch_stats()
        assert rb.same(got, expect(oracle, roff, rrp, rre, places, regions, rt, limit)), limit
        assert st["sorted"] == 0 and st["host_assembled"] == 0
