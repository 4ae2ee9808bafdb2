"""GPU checks of locrec_eval_ranked_batch (csrc/eval.hip) at the limits of its walk and tables, on the cases of
tests/eval_limit_cases.py: first hits behind all-miss tiles, cutoffs on the 64-wide seams, cutoffs up to 2^63 - 1, runs
of equal relevant ids across the 64-lane steps, the segment counts around the block and radix shapes; that a cutoff's
value does not depend on the other cutoffs of the call; and that the order and repetition of a relevant list, ids in
front of the first offset and the order of the segments change nothing but that order.  The tolerances are those of
eval_cases.assert_matches_model; the precision at a cutoff above 2^53 is within one ulp (eval_limit_cases)."""
import numpy as np
import pytest
import torch

import eval_cases as ec
import eval_limit_cases as lc

pytestmark = pytest.mark.gpu
OUTPUTS = ("means", "coverage", "relevant", "hits", "metrics")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def same_bits(a, b):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_outputs(a, b, names=OUTPUTS):
    assert a["evaluated"] == b["evaluated"]
    for k in names:
        assert same_bits(a[k], b[k]), k


def evaluate(prep, case, cutoffs):
    got = prep.evaluate_ranked(*case, cutoffs, per_segment=True)
    assert prep.evaluate_ranked_stats()["host_syncs"] == 2
    return got


def check_case(prep, case, cutoffs):
    """The model, host and device inputs bit for bit, and the statistics.  Above 2^53 a cutoff's precision is compared
    by its restatement first and then taken from the model, so that everything else meets assert_matches_model."""
    rec, counts, off, rel = case
    want = ec.model_eval(rec, counts, off, rel, cutoffs)
    assert want["evaluated"] > 0 and want["hits"].sum() > 0, "a vacuous case"
    got = evaluate(prep, case, cutoffs)
    st = prep.evaluate_ranked_stats()
    assert st["path"] == 1 and st["evaluated"] == want["evaluated"] and st["table_entries"] == int(want["relevant"].sum())
    compared = dict(got, metrics=np.array(got["metrics"]))
    for j, k in enumerate(cutoffs):
        live = want["relevant"] > 0
        assert lc.precision_matches(got["metrics"][live, j, 0], want["hits"][live, j], k), (j, k)
        if k > 2 ** 53:
            compared["metrics"][:, j, 0] = want["metrics"][:, j, 0]
    ec.assert_matches_model(compared, want, cutoffs, len(counts))
    on_device = prep.evaluate_ranked(*[dev(a) for a in case], cutoffs, per_segment=True)
    assert prep.evaluate_ranked_stats()["host_syncs"] == 2
    assert all(torch.is_tensor(on_device[k]) for k in ("relevant", "hits", "metrics"))
    assert_same_outputs(got, on_device)
    return got, want


def test_first_hits_behind_all_miss_tiles(pkg):
    case, sets, firsts = lc.late_first_hit()
    for cutoffs in sets:
        got, _ = check_case(pkg.prep, case, cutoffs)
        for s, first in enumerate(firsts):
            for j, k in enumerate(cutoffs):
                assert got["metrics"][s, j, 2] == (1.0 / (first + 1) if first < k else 0.0), (first, k)


def test_cutoffs_on_the_tile_seams(pkg):
    case, sets = lc.seam_cutoffs()
    for cutoffs in sets:
        check_case(pkg.prep, case, cutoffs)


def test_cutoffs_up_to_the_end_of_int64(pkg):
    case, sets = lc.huge_cutoffs()
    got, want = check_case(pkg.prep, case, sets[0])
    # no list has more than 65 ids and no row more than 65 positions: from the cutoff 65 on only the precision's
    # divisor changes, and every other figure is the same computation - the same bits
    at65 = sets[0].index(65)
    for j, k in enumerate(sets[0]):
        if k > 65:
            assert same_bits(got["hits"][:, j], got["hits"][:, at65]) and same_bits(got["metrics"][:, j, 1:], got["metrics"][:, at65, 1:])
            assert same_bits(got["means"][j, 1:], got["means"][at65, 1:]) and got["coverage"][j] == got["coverage"][at65]
    got, _ = check_case(pkg.prep, case, sets[1])
    for j in range(1, 8):                                    # eight equal cutoffs: eight equal columns
        assert same_bits(got["hits"][:, j], got["hits"][:, 0]) and same_bits(got["metrics"][:, j], got["metrics"][:, 0])
        assert same_bits(got["means"][j], got["means"][0]) and got["coverage"][j] == got["coverage"][0]


def test_runs_of_equal_relevant_ids(pkg):
    got, _ = check_case(pkg.prep, lc.duplicate_runs(), [70, 4, 3, 11])
    assert got["relevant"].tolist() == [1, 129, 71] and got["hits"][0].tolist() == [1, 1, 0, 1]


@pytest.mark.parametrize("n_segments", lc.SEGMENT_COUNTS)
def test_segment_counts(pkg, n_segments):
    check_case(pkg.prep, lc.segment_count_case(n_segments), lc.SEGMENT_CUTOFFS)


def test_most_segments_not_evaluated(pkg):
    got, want = check_case(pkg.prep, lc.segment_count_case(1025, sparse=True), lc.SEGMENT_CUTOFFS)
    assert got["evaluated"] == 11 and got["means"][-1, 5] == want["means"][-1, 5] > 0.0


def test_a_cutoff_does_not_depend_on_the_others(pkg):
    prep = pkg.prep
    for case, sets in (lc.seam_cutoffs(), lc.late_first_hit()[:2]):
        for cutoffs in sets:
            whole = evaluate(prep, case, cutoffs)
            back = evaluate(prep, case, cutoffs[::-1])
            n = len(cutoffs)
            for j, k in enumerate(cutoffs):
                alone = evaluate(prep, case, [k])
                for other, i in ((alone, 0), (back, n - 1 - j)):
                    assert same_bits(whole["hits"][:, j], other["hits"][:, i]), (k, i)
                    assert same_bits(whole["metrics"][:, j], other["metrics"][:, i]), (k, i)
                    assert same_bits(whole["means"][j], other["means"][i]), (k, i)
                    assert whole["coverage"][j] == other["coverage"][i], (k, i)
                    assert same_bits(whole["relevant"], other["relevant"]) and whole["evaluated"] == other["evaluated"]


def test_the_lists_are_sets_and_the_segments_independent(pkg):
    prep, cutoffs = pkg.prep, lc.SEGMENT_CUTOFFS
    rec, counts, off, rel = case = ec.eval_case(8, 65, 70)
    rng = np.random.default_rng(3)
    lists = [rel[off[s]:off[s + 1]] for s in range(65)]
    base, want = check_case(prep, case, cutoffs)

    def csr(ls, front=()):
        o = np.zeros(len(ls) + 1, np.int64)
        np.cumsum([len(x) for x in ls], out=o[1:])
        return o + len(front), np.concatenate([np.array(front, np.int64)] + [np.asarray(x, np.int64) for x in ls])

    variants = {"permuted": csr([rng.permutation(x) for x in lists]),
                "twice": csr([np.concatenate([x, x[::-1]]) for x in lists]),
                "ids in front": csr(lists, front=rec[0, :5].tolist())}     # (recommended ids, but no segment's)
    for name, (o, r) in variants.items():
        assert len(r) != len(rel) or not np.array_equal(r, rel), name
        for move in (lambda a: a, dev):
            got = prep.evaluate_ranked(move(rec), move(counts), move(o), move(r), cutoffs, per_segment=True)
            assert prep.evaluate_ranked_stats()["host_syncs"] == 2
            assert_same_outputs(base, got)

    perm = rng.permutation(65)
    assert (perm != np.arange(65)).sum() > 50
    o, r = csr([lists[s] for s in perm])
    got = evaluate(prep, (rec[perm], counts[perm], o, r), cutoffs)
    for k in ("relevant", "hits", "metrics"):
        assert same_bits(got[k], base[k][perm]), k
    assert got["evaluated"] == base["evaluated"] and np.array_equal(got["coverage"], base["coverage"])
    # the means: another order of summation, so the model's bound and not the base's bits
    ec.assert_matches_model(got, dict(want, relevant=want["relevant"][perm]), cutoffs, 65, per_segment=False)
