"""The models of tests/eval_cases.py against answers worked out by hand (no library, no GPU): the GPU tests compare the
library with these models, so the models are checked against something that is neither."""
import math

import numpy as np

import eval_cases as ec


def one(row, count, relevant, cutoffs):
    R, per = ec.model_segment(row, count, relevant, cutoffs)
    return R, per


def test_hits_at_positions_0_and_3():
    R, per = one([10, 11, 12, 13, 14], 5, [10, 13, 99], [5])
    hits, precision, recall, rr, ap, ndcg = per[0]
    assert (R, hits) == (3, 2)
    assert precision == 2 / 5 and recall == 2 / 3 and rr == 1.0
    assert math.isclose(ap, (1 / 1 + 2 / 4) / 3, rel_tol=1e-15)
    assert math.isclose(ndcg, (1 + 1 / math.log2(5)) / (1 + 1 / math.log2(3) + 1 / 2), rel_tol=1e-15)
    # at cutoff 3 only the hit at position 0 is seen; the ideal list still has three places
    hits, precision, recall, rr, ap, ndcg = one([10, 11, 12, 13, 14], 5, [10, 13, 99], [3])[1][0]
    assert (hits, precision, recall, rr) == (1, 1 / 3, 1 / 3, 1.0)
    assert math.isclose(ap, 1 / 3, rel_tol=1e-15) and math.isclose(ndcg, 1 / (1 + 1 / math.log2(3) + 1 / 2), rel_tol=1e-15)


def test_a_repeated_id_hits_once():
    R, per = one([7, 7, 8], 3, [8, 7, 7], [3, 2])
    assert R == 2
    hits, precision, recall, rr, ap, ndcg = per[0]
    assert (hits, precision, recall, rr) == (2, 2 / 3, 1.0, 1.0)
    assert math.isclose(ap, (1 / 1 + 2 / 3) / 2, rel_tol=1e-15)
    assert math.isclose(ndcg, (1 + 1 / 2) / (1 + 1 / math.log2(3)), rel_tol=1e-15)   # hits at positions 0 and 2
    assert per[1][:4] == (1, 1 / 2, 1 / 2, 1.0)                                       # the second 7 is no hit


def test_no_relevant_id_means_zeros_and_not_evaluated():
    R, per = one([1, 2, 3], 3, [], [1, 3])
    assert R == 0 and per == [(0, 0.0, 0.0, 0.0, 0.0, 0.0)] * 2
    m = ec.model_eval(np.array([[1, 2, 3], [4, 5, 6]]), [3, 3], [0, 0, 1], [5], [2])
    assert m["evaluated"] == 1 and list(m["relevant"]) == [0, 1]
    assert m["means"][0].tolist() == [0.5, 1.0, 0.5, 0.5, m["metrics"][1, 0, 4], 1.0]   # over the one evaluated segment
    assert m["coverage"].tolist() == [4]


def test_a_cutoff_beyond_the_count():
    # two ids of a four-wide row; the padding (-1) is relevant and must not be seen
    R, per = one([5, 6, -1, -1], 2, [6, -1], [10])
    hits, precision, recall, rr, ap, ndcg = per[0]
    assert (R, hits, precision, recall, rr) == (2, 1, 1 / 10, 1 / 2, 1 / 2)
    assert math.isclose(ap, (1 / 2) / 2, rel_tol=1e-15)
    assert math.isclose(ndcg, (1 / math.log2(3)) / (1 + 1 / math.log2(3)), rel_tol=1e-15)
    m = ec.model_eval(np.array([[5, 6, -1, -1]]), [2], [0, 2], [6, -1], [10, 1])
    assert m["coverage"].tolist() == [2, 1]


def test_the_generated_cases_have_something_to_find():
    for n_segments in (1, 65, 300):
        for width in (1, 63, 64, 65, 128, 129):
            rec, counts, off, rel = ec.eval_case(n_segments * 1000 + width, n_segments, width)
            m = ec.model_eval(rec, counts, off, rel, [width])
            assert m["evaluated"] > 0 and m["hits"].sum() > 0, (n_segments, width)
            if n_segments >= 4:
                assert sorted(set(counts.tolist())) == sorted({0, 1, width - 1, width})
    m = ec.model_eval(*ec.corner_case(), [1, 4])
    assert m["relevant"].tolist() == [2, 1, 2, 2, 4, 0] and m["hits"][:, 1].tolist() == [1, 1, 2, 1, 3, 0]
    m = ec.model_eval(*ec.wide_case(), [3000])
    assert m["hits"][0, 0] > 300 and m["relevant"].min() > 4000


def test_holdout_model_on_a_table_worked_by_hand():
    #           row:  0   1   2   3   4   5   6   7   8   9
    person = [1,  1,  1,  2,  2,  3,  1,  2,  -4, -4]
    ts = [10, 20, 50, 10, 60, 70, 50, 50, 49, 51]
    place = [7,  8,  7,  7,  9,  7,  8,  9,  5,  5]
    region = [0,  0,  0,  0,  1,  0,  0,  1,  2,  2]
    # cut 50: train rows 0 1 3 8.  Person 3 has no train row; person 1 was at 7 and 8 before; person 2 at 7; -4 at 5.
    train, held = ec.model_holdout(person, ts, place, region, 50, False)
    assert train == [0, 1, 3, 8]
    assert held == [(-4, 2, 5), (1, 0, 7), (1, 0, 8), (2, 1, 9)]          # (2, 1, 9) twice in the table, once here
    train, held = ec.model_holdout(person, ts, place, region, 50, True)
    assert train == [0, 1, 3, 8] and held == [(2, 1, 9)]
    assert ec.model_holdout(person, ts, place, region, 5, False) == ([], [])                 # nobody has a train row
    assert ec.model_holdout(person, ts, place, region, 71, False) == (list(range(10)), [])


def test_holdout_cases_cover_their_corners():
    v = ec.holdout_case(3, 2000)
    train, held = ec.model_holdout(v["person_id"], v["timestamp"], v["place_id"], v["region_id"], 1000, False)
    _, new = ec.model_holdout(v["person_id"], v["timestamp"], v["place_id"], v["region_id"], 1000, True)
    assert 0 < len(train) < 2000 and 0 < len(new) < len(held)
    assert (v["timestamp"] == 1000).sum() > 50 and v["person_id"].min() < 0
    late = v["person_id"].min()
    assert late not in {p for p, _, _ in held} and late not in set(v["person_id"][train].tolist())
    behind = int((v["timestamp"] >= 1000).sum())
    assert len(held) < 0.8 * behind                                                     # the same triple many times
