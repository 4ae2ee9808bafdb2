"""The KNN hit pre-pass (csrc/knn_ht_prepass.h) against a model of its contract, at the limits named in its code.

Every case builds an index under LOCREC_KNN_HT_H, runs ONE batch and reads what the pre-pass left on the device
(KnnIndex.ht_last_hits): tile_base, every `off` entry - empty slices and the closing total included - and the hit words,
sorted per tile and slice, must equal the model of knn_prepass_model.py; the final ids, similarities and counts must
equal the oracle, the same index under LOCREC_KNN_HT_PRE_V1=1 (whose hits go through the same view and the same
model) and under LOCREC_KNN_NO_HT=1, bit for bit.  The data sets and the assertions that they hold the counts the
cases are about are in knn_prepass_cases.py; those assertions also run without a GPU (test_knn_prepass_model.py) and
here before the first launch on a data set.

  C1  ht_build_hits<16, 16>, the shipped instantiation: stage unset, 4097 (its smallest), 8192, 100000 (clamped to
      8192) - sub-ranges of 4,097 - 8,191 hits (register records r >= 8), exactly 8,192 (full), more (overflow, between
      two staged sub-ranges of one tile), tiles of five sub-ranges with a partial last one, runs at every misalignment,
      empty sub-ranges
  C2  ht_build_hits<16, 8> at its top: stage 4096 - 2,576 and 3,840 hits (records 5 - 7), exactly 4,096, more
  C3  segments of 4, 8, 16, 32 and 64 lanes (C1 + C2), with an entry of 16 postings in one sub-range where it is 4
  C4  kHtMaxEntries: a tile of exactly 1,024 entries, and 1,025 (the batch leaves the head / tail form)
  C5  1,026 tiles: more than one chunk of ht_tile_bases
  C6  the hit word with lane 63, query 15, product 255 x 255; a tail-only dot of exactly 65,535 in an even query
  C7  0 / 1 / 63 / 64 / 65 / 127 / 128 / 129 / 1,024 hits of one slice and tile, with and without the seeding launch

Out of scope: the switch to ht_build_hits_v1 at 2^32 postings, the limit of 2^32 hits per tile (both need data no test
can hold), and the 32-query tile (cfg::kHtQt is a constant: no switch of the tree selects it).  The device tripwire of
ht_pre_entries (HtPreParams::error) is not exposed by the handle and is not read."""
import numpy as np
import pytest

import knn_prepass_cases as C
import knn_prepass_model as M
from test_gpu_knn import make_index

pytestmark = pytest.mark.gpu

K = 10
PW, CW = 0.5, 0.5
SEED = (("LOCREC_KNN_SEED_MIN_SLICES", "1"),)
V1 = (("LOCREC_KNN_HT_PRE_V1", "1"),)
NO_HT = (("LOCREC_KNN_NO_HT", "1"),)
FORMS = ("range", "rows", "rows_left_out")
_memo = {}


def run(pkg, monkeypatch, d, hot, env, rows=None, want_kernel=2):
    """One batch - every row as a range (rows = None), or the rows `rows` as a list - on a fresh index.
    -> ((ids, sims, counts), what ht_last_hits returned or None when the batch had no pre-pass)."""
    monkeypatch.setenv("LOCREC_KNN_HT_H", str(hot))
    for name, value in env:
        monkeypatch.setenv(name, value)
    try:
        ix = make_index(pkg, d)
        n = len(d["person_ids"])
        if want_kernel == 2:   # (without the head / tail form the rows' third sort key is another; answers come by person)
            assert np.array_equal(ix.row_person_ids(0, n), d["person_ids"]), "the index must keep the input order"
        out = ix.all_pairs_topk(PW, CW, K) if rows is None else ix.query_batch(d["person_ids"][rows], PW, CW, K)
        assert ix.scan_plan()["kernel"] == want_kernel, (env, ix.scan_kernel_name())
        nq = n if rows is None else len(rows)
        if want_kernel == 2:
            view = ix.ht_last_hits(nq)
            with pytest.raises(pkg.IllegalArgumentException, match="no matching hit pre-pass"):
                ix.ht_last_hits(nq + 1)
        else:
            view = None
            with pytest.raises(pkg.IllegalArgumentException, match="no matching hit pre-pass"):
                ix.ht_last_hits(nq)
        ix.close()
    finally:
        for name, _ in env:
            monkeypatch.delenv(name)
        monkeypatch.delenv("LOCREC_KNN_HT_H")
    return out, view


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_batch(pkg, monkeypatch, oracle, name, d, hot, envs, rows=None, oracle_rows=None, keep_entries=True):
    """The checks every case makes, for one batch of data set `name`: under each environment of `envs` the pre-pass
    equals the model and the answers equal the oracle (on oracle_rows, positions of the batch; default all), the
    two-pass pre-pass - checked against the model too - and the scan without the head / tail form."""
    n = len(d["person_ids"])
    qrows = np.arange(n) if rows is None else np.asarray(rows)
    key = (name, None if rows is None else tuple(qrows.tolist()))
    if key not in _memo:
        # (locrec_knn_query_batch serves a list in row order and hands the answers back in the caller's)
        model = M.prepass(d, np.arange(n), hot, np.sort(qrows), keep_entries=keep_entries)
        pos = np.arange(len(qrows)) if oracle_rows is None else np.asarray(oracle_rows)
        want = oracle.knn_similar_batch(d, qrows[pos], PW, CW, K, nthreads=8)
        v1, v1_view = run(pkg, monkeypatch, d, hot, V1, rows)
        M.check_view(v1_view, model, "two-pass pre-pass")
        no_ht, _ = run(pkg, monkeypatch, d, hot, NO_HT, rows, want_kernel=1)
        assert same(v1, no_ht), "the two partners differ"
        _memo[key] = (model, pos, want, no_ht)
    model, pos, want, no_ht = _memo[key]
    for env in envs:
        got, view = run(pkg, monkeypatch, d, hot, env, rows)
        assert view["tile_base"][-1] == len(view["hits"])
        M.check_view(view, model, env)
        assert np.array_equal(got[2][pos], want[2]), env
        assert np.array_equal(got[0][pos], want[0]), "top-K ids differ from the oracle"
        assert np.array_equal(got[1][pos], want[1]), "similarities are not bit-identical"
        assert same(got, no_ht), "differs from the two-pass pre-pass and the scan without the head / tail form"
    return model


def c1(name="c1"):
    if name not in _memo:
        d = C.c1_dataset()
        C.c1_check(M.prepass(d, np.arange(C.C1_N), C.C1_HOT, np.arange(C.C1_N)))
        _memo[name] = d
    return _memo[name]


def rows_of(form, n, left_out):
    return None if form == "range" else C.rows_of_form(n, form, left_out)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("stage", [None, "4097", "8192", "100000"])
def test_c1_shipped_instantiation(pkg, oracle, monkeypatch, stage, form):
    """ht_build_hits<16, 16> (stages above 4,096; the default is 8,192)."""
    assert M.records_per_thread(M.effective_stage(stage)) == 16
    env = () if stage is None else (("LOCREC_KNN_HT_PRE_STAGE", stage),)
    check_batch(pkg, monkeypatch, oracle, "c1", c1(), C.C1_HOT, [env], rows_of(form, C.C1_N, C.C1_LEFT_OUT))


@pytest.mark.parametrize("form", FORMS)
def test_c2_small_instantiation_at_its_top(pkg, oracle, monkeypatch, form):
    """ht_build_hits<16, 8> under its largest stage; with C1 every segment size (C3)."""
    assert M.records_per_thread(M.effective_stage("4096")) == 8
    check_batch(pkg, monkeypatch, oracle, "c1", c1(), C.C1_HOT, [(("LOCREC_KNN_HT_PRE_STAGE", "4096"),)],
                rows_of(form, C.C1_N, C.C1_LEFT_OUT))


def test_c4_tile_of_exactly_max_entries_and_one_more(pkg, oracle, monkeypatch):
    """ent <= kHtMaxEntries in enqueue_topk: 1,024 entries take the head / tail form; with 1,025 in one tile `ok` is
    false for the whole batch, use_ht stays false and the batch is planned by make_plan: kernel 1 (knn_scan)."""
    d, e = C.c4_dataset(), C.c4_dataset(extra=True)
    whole = lambda x: M.prepass(x, np.arange(C.C4_N), C.C4_HOT, np.arange(C.C4_N))
    C.c4_check(whole(d), whole(e))
    # sixteen light rows, then "any 16" of the heavy ones, the changed row among them, in an order of the caller's own
    rows = np.concatenate([[127], np.arange(64, 124, 4), np.arange(16)])
    model = check_batch(pkg, monkeypatch, oracle, "c4", d, C.C4_HOT, [(), (("LOCREC_KNN_HT_PRE_STAGE", "4096"),)], rows)
    assert model.entries.tolist() == [32, 1024]
    check_batch(pkg, monkeypatch, oracle, "c4", d, C.C4_HOT, [()])
    base, _ = run(pkg, monkeypatch, d, C.C4_HOT, (), rows)
    got, view = run(pkg, monkeypatch, e, C.C4_HOT, (), rows, want_kernel=1)   # (run() asserts that ht_last_hits refuses)
    assert view is None
    want = oracle.knn_similar_batch(e, rows, PW, CW, K, nthreads=8)
    assert same(got, want), "the batch that left the head / tail form differs from the oracle"
    # unaffected: the rows whose answer does not involve the changed person (its vector length changed, no dot did)
    changed = e["person_ids"][C.C4_N - 1]
    unaffected = np.array([r != C.C4_N - 1 and changed not in got[0][j] and changed not in base[0][j] for j, r in enumerate(rows)])
    assert unaffected.sum() >= 16
    assert same([x[unaffected] for x in got], [x[unaffected] for x in base])


def test_c5_more_than_1024_tiles(pkg, oracle, monkeypatch):
    """ht_tile_bases walks the tiles in chunks of 1,024 with a carry.  locrec_knn_query_batch hands its whole list to
    enqueue_topk as one batch, and nothing there bounds the tiles of a batch: 16,408 queries are 1,026 tiles."""
    d = C.c5_dataset()
    model = check_batch(pkg, monkeypatch, oracle, "c5", d, C.C5_HOT, [()], np.arange(C.C5_N), oracle_rows=C.C5_SAMPLE,
                        keep_entries=False)
    C.c5_check(model)


def test_c6_hit_word_and_accumulator_extremes(pkg, oracle, monkeypatch):
    d = C.c6_dataset()
    C.c6_check(M.prepass(d, np.arange(C.C6_N), C.C6_HOT, np.arange(C.C6_N)), d)
    for rows in (None, np.arange(C.C6_N)):
        check_batch(pkg, monkeypatch, oracle, "c6", d, C.C6_HOT, [(), SEED], rows)
    out, view = run(pkg, monkeypatch, d, C.C6_HOT, ())
    assert (63 << 21 | 15 << 16 | 255 * 255) in view["hits"][:view["off"][0, 1]].tolist()
    ids = d["person_ids"]
    assert ids[2] in out[0][0] and ids[0] in out[0][2], "the rows whose tail-only dot is 65,535 are each other's neighbours"


def test_c7_hit_loop_edges_of_the_scan(pkg, oracle, monkeypatch):
    """knn_scan_ht prefetches the first 64 hits of a slice and reads the rest with a clamped lane index; its seeding
    instantiation has its own copy of the loop."""
    d = C.c7_dataset()
    C.c7_check(M.prepass(d, np.arange(C.C7_N), C.C7_HOT, np.arange(C.C7_N)))
    for rows in (None, np.arange(C.C7_N)):
        check_batch(pkg, monkeypatch, oracle, "c7", d, C.C7_HOT, [(), SEED], rows)
    _, view = run(pkg, monkeypatch, d, C.C7_HOT, ())
    assert np.diff(view["off"][0].astype(np.int64)).tolist()[1:] == [C.C7_WANT[s] for s in range(1, 10)]
