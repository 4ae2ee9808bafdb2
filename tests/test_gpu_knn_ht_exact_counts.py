"""knn_scan_ht multiplies, per slice, exactly the elements its widest row holds (the slice descriptor's fourth word) -
not the whole dwordx4 groups the head / tail image stores.  The last group of each family is partial (1 .. 3 elements
of it are multiplied, or all 4), in the rotating registers and in the on-demand loops behind them.

Every data set is built by hand so that the head counts are known: the HOT places are held by far more rows than any
COLD place, so with LOCREC_KNN_HT_H = number of hot places the popularity renumbering makes exactly the hot places the
head and every cold place a tail place (asserted on the frequencies).  Ids and similarities are compared bit for bit
with the oracle and with the same index under LOCREC_KNN_NO_HT=1, on the seeding instantiation
(LOCREC_KNN_SEED_MIN_SLICES=1), without the barrier-free mode (LOCREC_KNN_NO_FAST=1) and with the counts rounded up to
four (LOCREC_KNN_HT_ROUND4=1, the A/B switch); the device builder and the host builder must agree."""
import numpy as np
import pytest

from test_gpu_knn import make_index

pytestmark = pytest.mark.gpu

K = 10
PW, CW = 0.5, 0.5
PATHS = ((), (("LOCREC_KNN_SEED_MIN_SLICES", "1"),), (("LOCREC_KNN_NO_FAST", "1"),), (("LOCREC_KNN_HT_ROUND4", "1"),),
         (("LOCREC_KNN_HOST_BUILD", "1"),), (("LOCREC_KNN_HOST_BUILD", "1"), ("LOCREC_KNN_HT_ROUND4", "1")))


def dataset(rows, hot, cold, c_dim, seed):
    """rows: (head places, tail places, categories) counts per person.  Hot places are 0 .. hot - 1, a row's cold places
    come round-robin from hot .. hot + cold - 1.  Returns the data set and the rows' (head, category) counts."""
    rng = np.random.default_rng(seed)
    prp, pidx, pval, crp, cidx, cval = [0], [], [], [0], [], []
    next_cold = 0
    for nh, nt, nc in rows:
        ip = list(rng.choice(hot, size=nh, replace=False))
        for _ in range(nt):
            ip.append(hot + next_cold % cold)
            next_cold += 1
        ip = np.sort(np.array(ip, np.int64))
        ic = np.sort(rng.choice(c_dim, size=nc, replace=False))
        pidx.append(ip); pval.append(rng.integers(1, 9, size=len(ip)).astype(np.float64)); prp.append(prp[-1] + len(ip))
        cidx.append(ic); cval.append(rng.integers(1, 30, size=len(ic)).astype(np.float64)); crp.append(crp[-1] + len(ic))
    n = len(rows)
    d = {"person_ids": rng.permutation(np.arange(5000, 5000 + n)).astype(np.int64),
         "p_rowptr": np.array(prp, np.int64), "p_idx": np.concatenate(pidx).astype(np.int32), "p_val": np.concatenate(pval),
         "p_dim": hot + cold,
         "c_rowptr": np.array(crp, np.int64), "c_idx": np.concatenate(cidx).astype(np.int32), "c_val": np.concatenate(cval),
         "c_dim": c_dim}
    freq = np.bincount(d["p_idx"], minlength=hot + cold)
    assert freq[:hot].min() > freq[hot:].max() > 0, "the hot places must be the head, and a tail must exist"
    return d, np.array([(nh, nc) for nh, _, nc in rows], np.int64)


def blocks(spec, last, tails=2):
    """One block of exactly 64 rows per (head count h, category count c) of spec, then `last` = (h, c, rows) with fewer
    than 64 rows.  The index orders its rows by (place count, category count, head count) and cuts slices of 64: every
    block gets a place count of its own (head + tail places), growing from block to block, so each block IS one slice,
    whose widest row is exactly (h, c).  Inside a block 52 rows are (h, c); 6 hold fewer head places (and more tail
    places: the same place count) and 6 fewer categories - the short lanes that meet zero words.  Returns the rows in a
    shuffled order and the (place, category) counts the slices must show."""
    rows, want = [], []
    place_count = 0
    for h, c, n in [(h, c, 64) for h, c in spec] + [last]:
        place_count = max(place_count + 1, h + tails)
        for i in range(n):
            hh = max(0, h - 1 - i % 3) if i % 10 == 3 else h
            cc = max(1, c - 1 - i % 2) if i % 10 == 7 else c
            rows.append((hh, place_count - hh, cc))
        want.append((h, c))
    rng = np.random.default_rng(len(rows))
    return [rows[i] for i in rng.permutation(len(rows))], np.array(want, np.int32)


def remainders():
    """Slices whose widest row holds 0, 1, 2 ... 9 head places and 1 ... 9 categories: every nel from 1 to 4 is the
    last group of either family in group 0 (where FIRST and the exits meet: counts 1 - 4) and in a later group of the
    rotating registers (counts 5 - 8), the place family has a slice with no element at all, and count 9 of the
    category family ends in the on-demand loop.  663 persons: 10 slices of 64 and one of 23."""
    rows, want = blocks([(0, 4), (1, 1), (2, 2), (3, 3), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 4)], last=(5, 3, 23))
    return dataset(rows, hot=16, cold=700, c_dim=20, seed=12), 16, want


def beyond_the_registers():
    """More than 16 head places and more than 8 categories: the on-demand loops behind the rotating registers end in a
    partial group of every nel (17 ... 20 places, 9 ... 12 categories) and run more than once (22 places, 13
    categories).  343 persons."""
    rows, want = blocks([(17, 9), (18, 10), (19, 11), (20, 12), (22, 13)], last=(23, 9, 23), tails=1)
    return dataset(rows, hot=48, cold=200, c_dim=16, seed=22), 48, want


def uniform(nh, nc, n=200):
    (d, counts) = dataset([(nh, 1 + i % 2, nc) for i in range(n)], hot=8, cold=150, c_dim=12, seed=31)
    return (d, counts), 8, np.array([(nh, nc)] * ((n + 63) // 64), np.int32)


CASES = {"remainders": remainders, "beyond": beyond_the_registers, "uniform_5_3": lambda: uniform(5, 3),
         "uniform_4_8": lambda: uniform(4, 8), "uniform_8_4": lambda: uniform(8, 4)}
PARTIAL = ("remainders", "beyond", "uniform_5_3")     # (the other two: every count a multiple of four)
_memo = {}


def case(name, oracle):
    """The data set and the oracle's answer for every person as a query, computed once."""
    if name not in _memo:
        (d, counts), h, want = CASES[name]()
        rows = np.arange(len(d["person_ids"]))
        _memo[name] = (d, counts, h, want, oracle.knn_similar_batch(d, rows, PW, CW, K, nthreads=8))
    return _memo[name]


def answers(pkg, monkeypatch, d, h, env, want_kernel):
    monkeypatch.setenv("LOCREC_KNN_HT_H", str(h))
    for name, value in env:
        monkeypatch.setenv(name, value)
    ix = make_index(pkg, d)
    out = ix.query_batch(d["person_ids"], PW, CW, K)
    assert ix.scan_plan()["kernel"] == want_kernel, (env, ix.scan_kernel_name())
    figures = (ix.ht_image_info()["head_words"], ix.ht_multiplied_words(), ix.ht_slice_counts())
    ix.close()
    for name, _ in env:
        monkeypatch.delenv(name)
    monkeypatch.delenv("LOCREC_KNN_HT_H")
    return out, figures


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("env", PATHS, ids=lambda e: "+".join(n for n, _ in e) or "default")
def test_partial_last_groups_match_the_oracle(pkg, oracle, monkeypatch, name, env):
    d, counts, h, want, (oi, os_, oc) = case(name, oracle)
    (ids, sims, cnt), (stored, multiplied, per_slice) = answers(pkg, monkeypatch, d, h, env, want_kernel=2)
    # the slices the data was built for did occur - so every partial last group the case is about has run
    round4 = any(n == "LOCREC_KNN_HT_ROUND4" for n, _ in env)
    assert np.array_equal(per_slice, (want + 3) & ~3 if round4 else want), per_slice.tolist()
    assert multiplied == 64 * int(per_slice.sum())
    assert np.array_equal(cnt, oc)
    assert np.array_equal(ids, oi), "top-K ids differ from the oracle"
    assert np.array_equal(sims, os_), "similarities are not bit-identical"
    real = int(counts.sum())
    assert real <= multiplied <= stored, (real, multiplied, stored)
    if round4 or name not in PARTIAL:
        assert multiplied == stored
    else:
        assert multiplied < stored, "these counts are no multiples of four: the scan must skip padding words"


@pytest.mark.parametrize("name", list(CASES))
def test_same_answers_without_the_head_tail_form(pkg, oracle, monkeypatch, name):
    d, _, h, _, _ = case(name, oracle)
    a, _ = answers(pkg, monkeypatch, d, h, (), want_kernel=2)
    b, figures = answers(pkg, monkeypatch, d, h, (("LOCREC_KNN_NO_HT", "1"),), want_kernel=1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert figures[:2] == (0, 0) and len(figures[2]) == 0


@pytest.mark.parametrize("host", [False, True])
def test_the_multiplied_words_figure(pkg, oracle, monkeypatch, host):
    """5 head places and 3 categories in every row: 5 + 3 words per lane are multiplied, 8 + 4 are stored.  Counts that
    are multiples of four: nothing to skip.  The A/B switch: every stored word again.  (The answers of these data sets
    are compared with the oracle by test_partial_last_groups_match_the_oracle.)"""
    build = (("LOCREC_KNN_HOST_BUILD", "1"),) if host else ()
    for name, nh, nc, per_lane in (("uniform_5_3", 5, 3, 8), ("uniform_4_8", 4, 8, 12), ("uniform_8_4", 8, 4, 12)):
        d, counts, h, _, _ = case(name, oracle)
        slices = (len(d["person_ids"]) + 63) // 64
        want_stored = 64 * slices * (((nh + 3) & ~3) + ((nc + 3) & ~3))
        _, (stored, multiplied, _) = answers(pkg, monkeypatch, d, h, build, want_kernel=2)
        assert (stored, multiplied) == (want_stored, 64 * slices * per_lane), (nh, nc)
        assert int(counts.sum()) <= multiplied
        _, (stored, multiplied, _) = answers(pkg, monkeypatch, d, h, build + (("LOCREC_KNN_HT_ROUND4", "1"),), want_kernel=2)
        assert stored == multiplied == want_stored, (nh, nc)
