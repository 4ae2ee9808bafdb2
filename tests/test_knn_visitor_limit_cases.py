"""The visitors' limit cases stand where they claim (tests/knn_visitor_limit_cases.py): lengths, exact sums, chunk sizes,
the row refusal's product and the report rule, checked on the CPU."""
import numpy as np

import knn_visitor_cases as vc
import knn_visitor_limit_cases as lim


def test_lengths_on_both_sides_of_the_limit():
    for family in ("p", "c"):
        served, refused = lim.long_visitor(family), lim.long_visitor(family, lim.LONG)
        assert len(served[family + "_idx"]) == 2 ** 21 - 1 == 2_097_151 and len(refused[family + "_idx"]) == 2 ** 21
        dim = lim.P_DIM if family == "p" else 20
        a = lim.stage_vector(served[family + "_idx"], served[family + "_val"], dim, family == "p")
        assert a["code"] == 0 and len(a["idx"]) == dim and a["beyond"] == 2 ** 21 - 1 - dim
        assert lim.stage_vector(refused[family + "_idx"], refused[family + "_val"], dim, family == "p")["code"] == lim.TOO_LONG
    assert lim.fill_blocks([600]) == 3 and lim.fill_blocks([20]) == 1 and lim.fill_blocks([0] * 16) == 1
    assert lim.fill_blocks([256]) == 1 and lim.fill_blocks([257]) == 2


def test_the_long_visitor_s_sum_of_squares_is_exact():
    """(2^21 - 1) entries of 65535: every partial sum is an integer below 2^53, so the left fold is exact - and so is any
    other order, which is what the header claims for the renumbered index."""
    m, x = 2 ** 21 - 1, 65535
    assert m * x * x < 2 ** 53 and (m + 1) * 65536 ** 2 == 2 ** 53        # the bound is the claim's, to the entry
    v = lim.long_visitor("p")
    exact = m * x * x
    assert float(exact) == exact
    assert lim.left_fold_norm(v["p_val"]) == float(np.sqrt(np.float64(exact)))
    assert float(np.sum(v["p_val"] ** 2)) == float(exact)                 # pairwise order: the same


def test_squares_that_leave_fp64():
    with np.errstate(over="ignore", under="ignore"):
        assert np.float64(1e160) * np.float64(1e160) == np.inf and np.float64(1e-170) * np.float64(1e-170) == 0.0
        assert np.float64(5e-324) ** 2 == 0.0
    d = lim.small_index(300, False)
    for label, (v, code) in lim.generic_value_cases(d).items():
        got = lim.first_refusal([v], d["p_dim"], d["c_dim"], False)
        assert (got[2] if got else 0) == code, label
    big = lim.generic_value_cases(d)["1e160 place"][0]
    assert lim.stage_vector(big["p_idx"], big["p_val"], d["p_dim"], False)["norm"] == np.inf


def test_value_cases_against_the_integer_rule():
    d = lim.small_index(300)
    served, refused = lim.value_cases(d)
    assert set(served) == {"-65535", "-1", "0 beside 4", "-0.0 beside 4", "65535"}
    assert set(refused) == {"65536", "-65536", "65535.5", "0.5", "5e-324"}
    for label, v in served.items():
        assert lim.first_refusal([v], d["p_dim"], d["c_dim"], True) is None, label
        assert (v["p_idx"] < d["p_dim"]).all()
    for label, v in refused.items():
        assert lim.first_refusal([v], d["p_dim"], d["c_dim"], True) == (0, 0, lim.FRACTION), label
    assert np.signbit(served["-0.0 beside 4"]["p_val"][0])
    # somebody of the index holds the two places: the values reach a dot product
    at = served["65535"]["p_idx"]
    assert np.isin(at, d["p_idx"]).all()


def test_chunk_budgets_give_the_chunk_sizes_named():
    n = lim.CHUNK_N
    for k in lim.CHUNK_KS:
        kk = lim.clipped(k, n)
        for size in lim.CHUNK_SIZES:
            budget = lim.budget_for(size, kk)
            assert lim.chunk_visitors(kk, budget) == size and lim.chunk_visitors(kk, budget - 1) < size
            brute = 0
            while (brute + 1) * kk * 20 <= budget:
                brute += 1
            assert brute == size
    assert lim.clipped(2_000_000, n) == 305
    assert lim.chunk_visitors(2_000_000) == 48 and lim.chunk_visitors(1) == (2 << 30) // 20 // 16 * 16
    # the chunks of every (nv, size): 5 is no whole tile, 16 and 32 are; tiles = the sum over chunks
    assert lim.chunks_of(17, 1, lim.budget_for(5, 1)) == [(0, 5), (5, 5), (10, 5), (15, 2)]
    assert lim.chunks_of(49, 50, lim.budget_for(16, 50)) == [(0, 16), (16, 16), (32, 16), (48, 1)]
    assert lim.chunks_of(49, 305, lim.budget_for(32, 305)) == [(0, 32), (32, 17)]
    assert lim.call_stats("query", 49, 1, n, 10, False, lim.budget_for(5, 1))["tiles"] == 10
    assert lim.call_stats("query", 49, 1, n, 10, False, lim.budget_for(32, 1))["tiles"] == 2 + 2
    assert lim.call_stats("query", 49, 1, n, 10, True)["host_syncs"] == 2 + 4 + 1
    assert lim.call_stats("recommend", 33, n, n, 10, False, rows=700)["host_syncs"] == 1 + 0 + 3 + 1
    assert lim.call_stats("recommend", 33, n - 1, n, 10, False, rows=70_000)["host_syncs"] == 1 + 3 + 3 + 0


def test_the_chunk_visitors_are_pairwise_different():
    vs = lim.distinct_visitors()
    assert len(vs) == 49
    keys = {(tuple(v["p_idx"].tolist()), tuple(v["p_val"].tolist()), tuple(v["c_idx"].tolist()), tuple(v["c_val"].tolist())) for v in vs}
    assert len(keys) == 49
    d = lim.small_index(lim.CHUNK_N)
    assert lim.first_refusal(vs, d["p_dim"], d["c_dim"], True) is None
    assert lim.beyond_total(vs, d["p_dim"], d["c_dim"]) == 3 * 49


def test_the_row_refusal_stands_on_three_times_two_to_the_thirty():
    assert lim.ROW_NV * lim.ROW_PLACES == 3 * 2 ** 30
    assert lim.worst_row_bytes(lim.ROW_NV, lim.ROW_PLACES) == lim.MAX_ROW_BYTES == 48 * 2 ** 30      # served: not above
    assert lim.worst_row_bytes(lim.ROW_NV + 1, lim.ROW_PLACES) == lim.MAX_ROW_BYTES + 16 * lim.ROW_PLACES
    d = lim.row_refusal_index()
    assert lim.rated_places(d) == lim.ROW_PLACES and len(d["person_ids"]) == 4 and d["r_rowptr"][-1] == lim.ROW_PLACES
    arrays = lim.nobody_batch(d, 5)
    assert arrays[0].tolist() == [0, 1, 2, 3, 4, 5] and (arrays[1] >= d["p_dim"]).all() and (arrays[4] >= d["c_dim"]).all()
    want = vc.csr([vc.nobody_visitor(d)] * 5)
    assert all(np.array_equal(a, b) for a, b in zip(arrays, want))


def test_the_capacity_case_passes_the_python_wrapper_s_room():
    """257 visitors who are everybody's neighbours get one row per rated place each: more than 65,536 rows."""
    d = lim.small_index(300)
    assert lim.CAPACITY_NV * lim.rated_places(d) > lim.PYTHON_ROOM
    v = lim.everybody_visitor(d, 1)
    assert len(v["c_idx"]) == d["c_dim"] and lim.first_refusal([v], d["p_dim"], d["c_dim"], True) is None


def test_the_first_offender_matches_a_brute_force_scan():
    d = lim.small_index(lim.STAGE_N)
    want = {"255 alone": (255, 0, lim.ORDER), "256 alone": (256, 0, lim.ORDER), "256 and 300": (256, 0, lim.FINITE),
            "category at 255, place at 256": (255, 1, lim.ORDER), "both families at 256": (256, 0, lim.NEGATIVE),
            "0 and 299": (0, 1, lim.ORDER)}
    for label, planted in lim.offenders():
        batch = lim.offender_batch(planted)
        assert len(batch) == lim.OFFENDER_NV > lim.STAGE_BLOCK
        for renumbered in (False, True):
            got = lim.first_refusal(batch, d["p_dim"], d["c_dim"], renumbered)
            assert got == lim.first_refusal_brute(batch, d["p_dim"], d["c_dim"], renumbered) == want[label], label
    assert lim.first_refusal(lim.offender_batch({}), d["p_dim"], d["c_dim"], True) is None
    # one vector, every code, vectorised against the kernel's loop - and the order of the tests inside one entry
    rng = np.random.default_rng(3)
    for _ in range(300):
        m = int(rng.integers(1, 7))
        idx = np.sort(rng.choice(40, m, replace=False)).astype(np.int64)
        val = rng.integers(0, 4, m).astype(np.float64)
        for _ in range(int(rng.integers(0, 3))):
            at, what = int(rng.integers(m)), int(rng.integers(5))
            if what == 0:
                idx[at] = -1
            elif what == 1 and at > 0:
                idx[at] = idx[at - 1]
            elif what == 2:
                val[at] = (np.inf, np.nan, -np.inf)[int(rng.integers(3))]
            elif what == 3:
                val[at] = (0.5, 65536.0, -65536.0, 65535.5, 5e-324)[int(rng.integers(5))]
            else:
                val[at] = (-3.0, 65535.0, -0.0)[int(rng.integers(3))]
        for rule in (False, True):
            with np.errstate(all="ignore"):
                assert lim.stage_vector(idx, val, 30, rule)["code"] == lim.stage_vector_brute(idx, val, 30, rule), (idx, val, rule)
    assert lim.message(lim.EMPTY, 1, 7) == "No such person: visitor 7 has no category vector"


def test_stage_batches_hold_every_distinct_visitor():
    for nv in lim.STAGE_NVS:
        batch, which = lim.stage_batch(nv)
        assert len(batch) == nv and set(which.tolist()) == set(range(lim.STAGE_DISTINCT)) and which[-1] != which[-2]
