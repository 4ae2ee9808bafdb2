"""The visitors' cases stand where they claim (tests/knn_visitor_cases.py): checked with the oracle alone, no GPU."""
import numpy as np

import knn_visitor_cases as vc


def test_the_forty_visitors_fill_their_lists_and_have_rows(oracle):
    d, visitors = vc.base()
    n = len(d["person_ids"])
    assert n == 2960 and len(visitors) == 40
    cands, rows = [], []
    for j in range(len(visitors)):
        ids, sims = vc.expected_similar(True, j, 2_000_000)
        cands.append(len(ids))
        assert vc.VISITOR_ID not in ids.tolist()                      # v is a candidate of nobody, itself included
        for k in (1, 50, 1025):
            assert len(vc.expected_similar(True, j, k)[0]) == k       # every list at K <= 1025 is full
        rows.append(len(vc.expected_recommend(True, j, 2_000_000)[0]))
    assert 1025 < min(cands) and max(cands) < n, (min(cands), max(cands))
    assert min(rows) >= 1 and max(rows) <= vc.P_DIM, (min(rows), max(rows))


def test_all_categories_visitor_has_exactly_n_candidates(oracle):
    d, _ = vc.base()
    n = len(d["person_ids"])
    v = vc.all_categories_visitor(d)
    ids_all, sims_all = vc.oracle_similar(d, v, 0.5, 0.5, 2_000_000)
    assert len(ids_all) == n
    # K = n is the first "every positive" K; K = n - 1 cuts exactly one: the last by (similarity asc, id desc)
    ids_n, _ = vc.oracle_similar(d, v, 0.5, 0.5, n)
    ids_cut, sims_cut = vc.oracle_similar(d, v, 0.5, 0.5, n - 1)
    assert np.array_equal(ids_n, ids_all) and len(ids_cut) == n - 1
    order = np.lexsort((-ids_all, sims_all))
    assert ids_all[order[0]] == ids_all[-1] and np.array_equal(ids_cut, ids_all[:-1]) and np.array_equal(sims_cut, sims_all[:-1])


def test_nobody_visitor_has_no_candidates(oracle):
    d, _ = vc.base()
    v = vc.nobody_visitor(d)
    assert len(vc.oracle_similar(d, v, 0.5, 0.5, 50)[0]) == 0
    assert len(vc.oracle_recommend(d, v, 0.5, 0.5, 2_000_000)[0]) == 0


def test_entries_beyond_the_dimensions_change_the_similarities(oracle):
    """... so a kernel that ignored them for the vector length fails the GPU tests."""
    d, visitors = vc.base()
    for j in (0, 17, 39):
        ids, sims = vc.expected_similar(True, j, 50)
        ids2, sims2 = vc.oracle_similar(d, vc.without_beyond(visitors[j], d["p_dim"], d["c_dim"]), 0.5, 0.5, 50)
        assert not np.array_equal(sims, sims2)
        assert sims2[0] > sims[0]           # a shorter vector: larger cosines


def test_copy_of_a_person_finds_it_first(oracle):
    d, _ = vc.base()
    for r in (3, 1500):
        ids, sims = vc.oracle_similar(d, vc.row_of(d, r), 0.25, 0.75, 5)
        assert ids[0] == d["person_ids"][r] or sims[1] == sims[0]
        assert abs(sims[0] - 1.0) < 1e-12   # pw + cw, up to the rounding of the two cosines
