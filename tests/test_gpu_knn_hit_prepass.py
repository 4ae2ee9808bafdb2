"""The hit pre-pass of the head / tail scan (csrc/knn_ht_prepass.h): sub-ranges sized per tile, one walk that stages
the hits in LDS, a counting sort there, whole-line flushes - and the two-pass route for a sub-range that overflows
the stage.

One hand-made data set of 700 persons (11 candidate slices, 44 query tiles, the last of 12 queries).  The index orders
its rows by (place count, category count, head count), stably: every tile of 16 persons gets a place count of its own,
growing from tile to tile, and one head count, so the index keeps the input order and the rows of every tile and slice
are known.  With LOCREC_KNN_HT_H = number of hot places the hot places are the head and every cold place is a tail
place (asserted on the frequencies).

  place A   held by all 64 rows of slice 2, so by all 16 queries of tiles 8 - 11: 1,024 hits of one slice and tile -
            more than any forced stage (the overflow route, between staged neighbours in the same launch) and more
            than 64 (the scan's second hit loop)
  place B   held by the 130 consecutive rows 254 .. 383: three slices, more than one 64-posting load, across a
            sub-range boundary; tile 15 reaches it through exactly two queries, tiles 16 - 23 through all sixteen
  fillers   three cold places per row (two where A or B is held), each held by about seven rows a hundred apart
  no tail   the rows of slices 8 and 9 (tiles 32 - 39) hold hot places only: tiles with nothing to do between tiles
            with work, and for every tile a sub-range without a hit

LOCREC_KNN_HT_PRE_STAGE sets the stage: at its lower clamp (64 hits) every tile takes sub-ranges of one slice, at
128 and 256 of one to eight (a boundary at every power-of-two position, the last sub-range partial), at 4096 (the largest stage of
the four-blocks-per-CU instantiation) one sub-range or two, by default (8192, the other instantiation) one.  The
widths are computed here from the documented rule and asserted, with the hit counts of the slices the case is about.

Ids, similarities and counts are compared bit for bit with the oracle, with the same index under
LOCREC_KNN_HT_PRE_V1=1 (the two-pass pre-pass) and under LOCREC_KNN_NO_HT=1 (no head / tail form at all); as a range
of rows, as a row list (all persons, and a list with rows left out so that the tiles shift and nq is no multiple of
16), through the seeding instantiation, and through the candidate-sharded request with two shards (slice0 > 0).
No switch of the tree selects the 32-query tile (cfg::kHtQt is a constant), so that instantiation has no case."""
import numpy as np
import pytest

from knn_prepass_model import width
from test_gpu_knn import make_index, sharded_request

pytestmark = pytest.mark.gpu

K = 10
PW, CW = 0.5, 0.5
N, HOT, COLD, C_DIM = 700, 64, 300, 12
PLACE_A, PLACE_B = HOT + COLD, HOT + COLD + 1
SEED = (("LOCREC_KNN_SEED_MIN_SLICES", "1"),)
STAGES = {"clamp": "1", "128": "128", "256": "256", "4096": "4096", "default": None}
STAGE_HITS = {"clamp": 64, "128": 128, "256": 256, "4096": 4096, "default": 8192}
WIDTH_MAX = 512
LEFT_OUT = (3, 130, 255, 400, 698)   # rows the shorter row list leaves out
SHARD_ROWS = (128, 254, 300, 520, 699)
_memo = {}


def no_tail(tile):
    return 32 <= tile < 40


def dataset():
    rng = np.random.default_rng(5)
    prp, pidx, pval, crp, cidx, cval = [0], [], [], [0], [], []
    next_cold = 0
    for i in range(N):
        tile = i // 16
        places = 8 + tile
        tail = []
        if not no_tail(tile):
            if 128 <= i < 192:
                tail.append(PLACE_A)
            if 254 <= i < 384:
                tail.append(PLACE_B)
            while len(tail) < 3:
                tail.append(HOT + next_cold % COLD)
                next_cold += 1
        ip = np.sort(np.array(list(rng.choice(HOT, size=places - len(tail), replace=False)) + tail, np.int64))
        ic = np.sort(rng.choice(C_DIM, size=4, replace=False))
        pidx.append(ip); pval.append(rng.integers(1, 9, size=len(ip)).astype(np.float64)); prp.append(prp[-1] + len(ip))
        cidx.append(ic); cval.append(rng.integers(1, 30, size=len(ic)).astype(np.float64)); crp.append(crp[-1] + len(ic))
    d = {"person_ids": rng.permutation(np.arange(9000, 9000 + N)).astype(np.int64),
         "p_rowptr": np.array(prp, np.int64), "p_idx": np.concatenate(pidx).astype(np.int32), "p_val": np.concatenate(pval),
         "p_dim": HOT + COLD + 2,
         "c_rowptr": np.array(crp, np.int64), "c_idx": np.concatenate(cidx).astype(np.int32), "c_val": np.concatenate(cval),
         "c_dim": C_DIM}
    freq = np.bincount(d["p_idx"], minlength=d["p_dim"])
    assert freq[:HOT].min() > freq[HOT:].max() > 0, "the hot places must be the head, and a tail must exist"
    assert freq[PLACE_A] == 64 and freq[PLACE_B] == 130
    return d


def hits_per_tile_and_slice(d, rows):
    """[tile][slice] hits of the query rows `rows` (in tiles of 16): a posting of a tail place is one hit for every
    query of the tile that holds the place."""
    holders = {}
    for r in range(N):
        for p in d["p_idx"][d["p_rowptr"][r]:d["p_rowptr"][r + 1]]:
            if p >= HOT:
                holders.setdefault(int(p), []).append(r)
    slices = (N + 63) // 64
    out = np.zeros(((len(rows) + 15) // 16, slices), np.int64)
    for j, r in enumerate(rows):
        for p in d["p_idx"][d["p_rowptr"][r]:d["p_rowptr"][r + 1]]:
            if p >= HOT:
                out[j // 16] += np.bincount(np.array(holders[int(p)]) // 64, minlength=slices)
    return out


def case(oracle):
    if "d" not in _memo:
        d = dataset()
        rows = np.arange(N)
        _memo["d"] = d
        _memo["oracle"] = oracle.knn_similar_batch(d, rows, PW, CW, K, nthreads=8)
        _memo["hits"] = hits_per_tile_and_slice(d, rows)
    return _memo["d"], _memo["oracle"], _memo["hits"]


def run(pkg, monkeypatch, d, env, form, want_kernel=2):
    """(ids, sims, counts) of every person of the form's list, in input order of that list."""
    monkeypatch.setenv("LOCREC_KNN_HT_H", str(HOT))
    for name, value in env:
        monkeypatch.setenv(name, value)
    ix = make_index(pkg, d)
    if form == "range":
        out = ix.all_pairs_topk(PW, CW, K)
    elif form == "rows":
        out = ix.query_batch(d["person_ids"], PW, CW, K)
    else:
        out = ix.query_batch(np.delete(d["person_ids"], LEFT_OUT), PW, CW, K)
    assert ix.scan_plan()["kernel"] == want_kernel, (env, ix.scan_kernel_name())
    ix.close()
    for name, _ in env:
        monkeypatch.delenv(name)
    monkeypatch.delenv("LOCREC_KNN_HT_H")
    return out


def partner(pkg, monkeypatch, d, name, form):
    """The answers of the two-pass pre-pass ("v1") and of the scan without the head / tail form ("no_ht"), once per form."""
    key = (name, form)
    if key not in _memo:
        if name == "v1":
            _memo[key] = run(pkg, monkeypatch, d, (("LOCREC_KNN_HT_PRE_V1", "1"),), form)
        else:
            _memo[key] = run(pkg, monkeypatch, d, (("LOCREC_KNN_NO_HT", "1"),), form, want_kernel=1)
    return _memo[key]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def stage_env(stage):
    return () if STAGES[stage] is None else (("LOCREC_KNN_HT_PRE_STAGE", STAGES[stage]),)


def test_the_data_set_holds_the_cases(oracle):
    d, _, hits = case(oracle)
    slices = hits.shape[1]
    assert slices == 11 and hits.shape[0] == 44
    for t in (8, 9, 10, 11):      # place A: 16 queries x 64 rows in slice 2; the tile's other slices fit any stage
        others = np.delete(hits[t], 2)
        assert hits[t, 2] >= 1024 and others.any() and others.max() <= 64
    assert hits[15, 3] >= 2 * 2 and hits[15, 4] == 2 * 64 and hits[15, 5] >= 2 * 64   # place B through two queries ...
    assert hits[16, 4] >= 16 * 64 and hits[16, 5] >= 16 * 64                            # ... and through sixteen
    assert not hits[32:40].any() and hits[31].any() and hits[40].any()   # tiles with nothing to do, between tiles with work
    assert not hits[:, 8:10].any()                                       # a sub-range without a hit, for every tile
    totals = [int(t) for t in hits.sum(axis=1) if t > 0]
    widths = {stage: {width(c, slices, t) for t in totals} for stage, c in STAGE_HITS.items()}
    assert widths["clamp"] == {1} and widths["128"] == {1, 2, 4} and widths["256"] == {1, 2, 4, 8}
    assert min(widths["4096"]) == 8 and max(widths["4096"]) >= slices   # one sub-range, or two: 8 slices and 3
    assert min(widths["default"]) >= slices                                 # one sub-range
    assert all(slices % w for ws in widths.values() for w in ws if w > 1), "the last sub-range is partial"
    # staged and overflowing sub-ranges in one launch: tile 15 under a stage of 128 takes slices of its own, and its
    # slice 4 fills the stage exactly (staged) while slice 5 exceeds it
    assert width(128, slices, int(hits[15].sum())) == 1 and hits[15, 4] == 128 < hits[15, 5]


@pytest.mark.parametrize("form", ["range", "rows", "rows_left_out"])
@pytest.mark.parametrize("stage", list(STAGES))
def test_prepass_matches_the_oracle_and_both_partners(pkg, oracle, monkeypatch, stage, form):
    d, (oi, os_, oc), _ = case(oracle)
    keep = np.delete(np.arange(N), LEFT_OUT) if form == "rows_left_out" else np.arange(N)
    for env in (stage_env(stage), stage_env(stage) + SEED):
        ids, sims, cnt = got = run(pkg, monkeypatch, d, env, form)
        assert np.array_equal(cnt, oc[keep]), env
        assert np.array_equal(ids, oi[keep]), "top-K ids differ from the oracle"
        assert np.array_equal(sims, os_[keep]), "similarities are not bit-identical"
        assert same(got, partner(pkg, monkeypatch, d, "v1", form)), "differs from the two-pass pre-pass"
        assert same(got, partner(pkg, monkeypatch, d, "no_ht", form)), "differs from the scan without the head / tail form"


def shard_answers(pkg, monkeypatch, d, env, want_kernel=2):
    """The merged answers of SHARD_ROWS through two candidate shards.  (LOCREC_KNN_NO_SINGLE: the request takes the
    tiled scan, as a tile of one query.)"""
    monkeypatch.setenv("LOCREC_KNN_HT_H", str(HOT))
    monkeypatch.setenv("LOCREC_KNN_NO_SINGLE", "1")
    for name, value in env:
        monkeypatch.setenv(name, value)
    ix = make_index(pkg, d)
    out = []
    for r in SHARD_ROWS:
        out.append(sharded_request(pkg, ix, int(d["person_ids"][r]), PW, CW, K, 2))
        assert ix.scan_plan()["kernel"] == want_kernel, (env, ix.scan_kernel_name())
    ix.close()
    for name, _ in env:
        monkeypatch.delenv(name)
    monkeypatch.delenv("LOCREC_KNN_NO_SINGLE")
    monkeypatch.delenv("LOCREC_KNN_HT_H")
    return out


@pytest.mark.parametrize("stage", list(STAGES))
def test_prepass_of_a_candidate_shard(pkg, oracle, monkeypatch, stage):
    """Two logical shards: the second one's scan starts at slice0 > 0, where the pre-pass first skips every entry's
    postings in front of the shard.  Against the oracle, the two-pass pre-pass and the scan without the head / tail form."""
    d, (oi, os_, oc), _ = case(oracle)
    if "shard_v1" not in _memo:
        _memo["shard_v1"] = shard_answers(pkg, monkeypatch, d, (("LOCREC_KNN_HT_PRE_V1", "1"),))
        _memo["shard_no_ht"] = shard_answers(pkg, monkeypatch, d, (("LOCREC_KNN_NO_HT", "1"),), want_kernel=1)
    for env in (stage_env(stage), stage_env(stage) + SEED):
        got = shard_answers(pkg, monkeypatch, d, env)
        for (ids, sims), r, v1, no_ht in zip(got, SHARD_ROWS, _memo["shard_v1"], _memo["shard_no_ht"]):
            m = int(oc[r])
            assert np.array_equal(ids, oi[r][:m]) and np.array_equal(sims, os_[r][:m]), (env, r)
            assert same((ids, sims), v1), "differs from the two-pass pre-pass"
            assert same((ids, sims), no_ht), "differs from the scan without the head / tail form"
