"""CPU: the cases of rank_exclude_cases contain what their generators claim, measured with the oracle's single ranker -
the lists really change the rankings they are meant to change."""
import numpy as np
import pytest

import rank_batch_cases as rb
import rank_exclude_cases as rx

SEEDS = range(4)


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_lists_contain_what_they_claim(seed):
    case = rx.fuzz_case(seed)
    nseg = len(case["targets"])
    assert len(case["ex_offsets"]) == nseg + 1 and case["ex_offsets"][0] == 0 and case["ex_offsets"][-1] == len(case["ex_ids"])
    lens = np.diff(case["ex_offsets"])
    assert set(lens.tolist()) <= set(rx.LIST_LENGTHS) and lens[0] == rx.LIST_LENGTHS[seed % 7]
    if nseg >= 7:
        assert set(lens.tolist()) == set(rx.LIST_LENGTHS)
    dup = lacking = extremes = False
    for s in range(nseg):
        x = rx.list_of(case, s)
        seg = case["ids"][case["offsets"][s]:case["offsets"][s + 1]]
        dup |= len(np.unique(x)) < len(x)
        lacking |= bool((~np.isin(x, seg)).any())
        extremes |= rb.I64_MIN in x and rb.I64_MAX in x
    if nseg >= 7:
        assert dup and lacking and extremes
    assert np.array_equal(case["ids"], rb.fuzz_case(seed)["ids"])          # (the rows are fuzz_case's own)


def test_fuzz_lists_change_the_rankings(oracle):
    """At limit 10, over the four cases: of the segments that have rows under the plain ranking at least a third get a
    different row under exclusion, at least one of those keeps rows and at least one loses all of them."""
    had = changed = kept = lost = 0
    for seed in SEEDS:
        case = rx.fuzz_case(seed)
        plain = rx.widened(rb.expected(oracle.rank_recommendations, case, 10), rx.width_of(case, 10))
        excl = rx.expected(oracle.rank_recommendations, case, 10)
        for s in range(len(case["targets"])):
            if plain[2][s] == 0:
                assert excl[2][s] == 0
                continue
            had += 1
            differs = plain[2][s] != excl[2][s] or not np.array_equal(plain[0][s], excl[0][s]) or \
                plain[1][s].tobytes() != excl[1][s].tobytes()
            changed += differs
            kept += differs and excl[2][s] > 0
            lost += differs and excl[2][s] == 0
            assert not np.isin(excl[0][s, :excl[2][s]], rx.list_of(case, s)).any()
    assert had > 100 and 3 * changed >= had, (had, changed)
    assert kept >= 1 and lost >= 1, (kept, lost)


def test_filtered_and_expected_agree_with_a_direct_loop(oracle):
    case = rx.fuzz_case(1)
    off = case["offsets"]
    for limit in (1, 10):
        want = rx.expected(oracle.rank_recommendations, case, limit)
        assert want[0].shape[1] == rx.width_of(case, limit)
        for s in range(len(case["targets"])):
            ids, scores = case["ids"][off[s]:off[s + 1]], case["scores"][off[s]:off[s + 1]]
            keep = ~np.isin(ids, rx.list_of(case, s))
            ri, rs = oracle.rank_recommendations(ids[keep], scores[keep], case["place_ids"], case["regions"],
                                                 int(case["targets"][s]), limit)
            assert want[2][s] == len(ri) and np.array_equal(want[0][s, :len(ri)], ri)
            assert want[1][s, :len(ri)].tobytes() == np.asarray(rs).tobytes()
    empty = rx.empty_lists(rb.fuzz_case(1))
    assert rb.same(rx.expected(oracle.rank_recommendations, empty, 10), rb.expected(oracle.rank_recommendations, rb.fuzz_case(1), 10))


def test_handmade_case(oracle):
    case = rx.handmade()
    for limit in (1, 3, 10):
        ids, scores, counts = rx.expected(oracle.rank_recommendations, case, limit)
        for s, want in enumerate(rx.HANDMADE_IDS):
            assert ids[s, :counts[s]].tolist() == want[:limit]
    # without the lists every segment is the same ranking
    ids, _, counts = rb.expected(oracle.rank_recommendations, case, 10)
    assert all(ids[s, :counts[s]].tolist() == [10, 11, 12, 13, 14, 15] for s in range(4))


@pytest.mark.parametrize("chunks", rb.SEAM_CHUNKS)
def test_seam_lists(oracle, chunks):
    case = rb.seam_case(chunks)
    n = 64 * chunks + 1
    dup, sides = rx.seam_lists(chunks)
    rows = np.flatnonzero(np.isin(case["ids"], dup))
    assert rows.tolist() == [5, n - 1] and rows[0] // 64 != rows[1] // 64
    rows = np.flatnonzero(np.isin(case["ids"], sides))
    assert set(rows.tolist()) >= {64 * c - 1 for c in range(1, chunks + 1)} | {64 * c for c in range(1, chunks + 1)}
    ids, _, counts = rx.expected(oracle.rank_recommendations, rx.with_lists(case, [dup]), 10)
    assert counts[0] == min(10, n - 2) and 5000 not in ids[0].tolist() and ids[0, 0] == 5001
