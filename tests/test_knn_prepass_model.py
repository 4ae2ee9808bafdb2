"""The model of the KNN hit pre-pass (knn_prepass_model.py) against a brute-force loop, and the data sets of
test_gpu_knn_prepass_limits.py against the counts their cases are about (knn_prepass_cases.py).  No GPU."""
import numpy as np
import pytest

import knn_prepass_cases as C
import knn_prepass_model as M


def small_dataset(n=100, hot=6, cold=40, seed=3):
    """100 persons in an order the index does NOT keep: random place counts, random mixes of hot and cold places."""
    rng = np.random.default_rng(seed)
    prp, pidx, pval, crp, cidx, cval = [0], [], [], [0], [], []
    for _ in range(n):
        ip = np.sort(np.concatenate([rng.choice(hot, size=rng.integers(3, hot + 1), replace=False),
                                     hot + rng.choice(cold, size=rng.integers(0, 6), replace=False)]))
        ic = np.sort(rng.choice(12, size=rng.integers(2, 5), replace=False))
        pidx.append(ip); pval.append(rng.integers(1, 200, size=len(ip)).astype(np.float64)); prp.append(prp[-1] + len(ip))
        cidx.append(ic); cval.append(rng.integers(1, 30, size=len(ic)).astype(np.float64)); crp.append(crp[-1] + len(ic))
    d = {"person_ids": rng.permutation(np.arange(500, 500 + n)).astype(np.int64),
         "p_rowptr": np.array(prp, np.int64), "p_idx": np.concatenate(pidx).astype(np.int32), "p_val": np.concatenate(pval),
         "p_dim": hot + cold, "c_rowptr": np.array(crp, np.int64), "c_idx": np.concatenate(cidx).astype(np.int32),
         "c_val": np.concatenate(cval), "c_dim": 12}
    freq = np.bincount(d["p_idx"], minlength=d["p_dim"])
    assert freq[:hot].min() > freq[hot:].max() > 0
    return d


@pytest.mark.parametrize("rows", ["all", "list"])
def test_model_equals_the_triple_loop(rows):
    d = small_dataset()
    hot = 6
    order = M.index_order(d, hot)
    assert not np.array_equal(order, np.arange(100)) and sorted(order.tolist()) == list(range(100))
    keys = [(d["p_rowptr"][i + 1] - d["p_rowptr"][i], d["c_rowptr"][i + 1] - d["c_rowptr"][i],
             int((d["p_idx"][d["p_rowptr"][i]:d["p_rowptr"][i + 1]] < hot).sum()), i) for i in order]
    assert keys == sorted(keys), "rows ascend by (place count, category count, head count, input position)"
    qrows = np.arange(100) if rows == "all" else np.array([99, 3, 3, 57, 12, 0, 41, 77, 8, 64, 23, 5, 90, 31, 2, 18, 66, 45, 71])
    m = M.prepass(d, order, hot, qrows)
    want = M.brute_force(d, order, hot, qrows)
    assert m.slices == 2 and m.ntiles == (len(qrows) + 15) // 16
    total = 0
    for t in range(m.ntiles):
        run = 0
        for s in range(m.slices):
            words = want.get((t, s), [])
            assert m.off[t, s] == run and m.slice_words(t, s).tolist() == words, (t, s)
            run += len(words)
        assert m.off[t, m.slices] == run and m.tile_base[t] == total
        total += run
    assert m.tile_base[m.ntiles] == total == len(m.word) > 0


def test_width_and_segment_follow_the_documented_rule():
    # width: the power of two w with w * 10 > 7 * target >= (w / 2) * 10, target = (stage / 2) * slices / total
    assert [M.width(8192, 35, t) for t in (8192, 12000, 23800, 23900, 3000, 0)] == [16, 8, 8, 4, 64, 512]
    assert M.width(64, 11, 10 ** 6) == 1 and M.width(8192, 100000, 1) == 512
    # segment: the power of two in 4 .. 64 that holds 2 * total * width / (slices * entries)
    assert [M.segment(7424, 8, 35, 912), M.segment(7680, 8, 35, 640), M.segment(7680, 8, 35, 320), M.segment(7680, 8, 35, 160),
            M.segment(8192, 16, 35, 16), M.segment(0, 512, 35, 0)] == [4, 8, 16, 32, 64, 4]
    assert [M.effective_stage(v) for v in (None, "1", "4097", "8192", "100000")] == [8192, 64, 4097, 8192, 8192]


def whole(d, n, hot, **kw):
    return M.prepass(d, np.arange(n), hot, np.arange(n), **kw)


def test_c1_c2_c3_data_set_holds_its_sub_ranges_and_segments():
    C.c1_check(whole(C.c1_dataset(), C.C1_N, C.C1_HOT))


def test_c4_data_sets_hold_tiles_of_1024_and_1025_entries():
    C.c4_check(whole(C.c4_dataset(), C.C4_N, C.C4_HOT), whole(C.c4_dataset(extra=True), C.C4_N, C.C4_HOT))


def test_c5_data_set_holds_1026_tiles():
    C.c5_check(whole(C.c5_dataset(), C.C5_N, C.C5_HOT, keep_entries=False))


def test_c6_data_set_holds_the_extreme_hit_word_and_the_dot_of_65535():
    d = C.c6_dataset()
    C.c6_check(whole(d, C.C6_N, C.C6_HOT), d)


def test_c7_data_set_holds_the_hit_counts_of_the_scan_loops():
    C.c7_check(whole(C.c7_dataset(), C.C7_N, C.C7_HOT))
