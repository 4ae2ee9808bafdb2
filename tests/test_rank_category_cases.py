"""CPU: the cases of rank_category_cases stand where they claim, the numpy restatement
mains.rank_recommendations_by_category equals the composition of the oracle's single ranker and the greedy walk on
them, and the capped list's pruning rule - restated here in plain Python: arrival in shuffled tiles of 256, a buffer of
1024, the compaction with kill, keep N and threshold, and the chunk merge - equals the greedy walk on every case."""
import numpy as np
import pytest

import rank_batch_cases as rb
import rank_category_cases as rc
import rank_near_cases as rn

MAX_N = 256
SMALL_LIMITS = (1, 2, 10, 256)


@pytest.fixture(scope="module")
def mains(pkg):
    from locations_recommender_amd import mains
    return mains


@pytest.fixture(scope="module")
def distance(oracle):
    return rn.elementwise(oracle.distance_meters)


def kept_of(distance, case):
    return rn.all_kept(distance, case) if "radius" in case else None


def entries_of(oracle, case, s, kept=None):
    """Segment s as the list's entries (key, category): the key is the row's place in the uncapped ranking, which is the
    3-part key's order; only the rows the join keeps are entries."""
    uncapped = {k: v for k, v in case.items() if k != "caps"}
    one = dict(uncapped, offsets=case["offsets"][s:s + 2], targets=case["targets"][s:s + 1])
    for k in ("clat", "clon", "radius"):
        if k in case:
            one[k] = case[k][s:s + 1]
    if "al_ids" in case:
        one = rc.with_allow(one, [rc.allow_of(case, s)])
    if "ex_ids" in case:
        import rank_exclude_cases as rx
        one = rx.with_lists(one, [rx.list_of(case, s)])
    ids, _, _, cnt = rc.expected(oracle.rank_recommendations, one, 2 ** 40, [kept[s]] if kept is not None else None)
    rows, _ = rc.passing_rows(case, s, kept[s] if kept is not None else None)
    first = {}
    for j, p in enumerate(case["place_ids"][rows].tolist()):
        first.setdefault(p, int(case["cats"][rows[j]]))
    return [(j, first[i]) for j, i in enumerate(ids[0, :cnt[0]].tolist())]


def check_rule(entries, n, cap, chunk=4096, seed=0):
    """The block's list (in arrival order: the ranking shuffled) and the chunk merge against the greedy walk."""
    rng = np.random.default_rng(seed)
    arrive = [entries[i] for i in rng.permutation(len(entries))]
    want = rc.greedy(entries, n, cap)
    assert rc.block_list(arrive, n, cap, seed) == want
    assert rc.chunked(arrive, n, cap, chunk, seed) == want


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_cases_and_the_restatement(oracle, mains, distance, seed):
    """Odd seeds carry exclusion lists, seeds 2 and 3 circles."""
    case = rc.fuzz_case(seed, lists=seed % 2 == 1, circles=seed >= 2)
    assert set(np.unique(case["cats"]).tolist()) == set(rc.FEW.tolist())
    lens = np.diff(case["al_offsets"])
    assert (lens == 0).any() or len(lens) < 5
    kept = kept_of(distance, case)
    changed = False
    for limit in rc.LIMITS:
        capped = rc.with_caps(case, limit, seed)
        want = rc.expected(oracle.rank_recommendations, capped, limit, kept)
        a, kw = rc.args(capped, limit)
        assert rc.same(mains.rank_recommendations_by_category(*a, **kw, distance=distance), want), limit
        free = rc.expected(oracle.rank_recommendations, case, limit, kept)
        changed = changed or not np.array_equal(free[0], want[0])
    assert changed                                                   # a cap changes the output somewhere


@pytest.mark.parametrize("seed", range(2))
def test_one_category_per_place_never_binds(oracle, seed):
    case = rc.fuzz_case(seed, few=False, allow=False)
    assert len(np.unique(case["cats"])) == len(case["cats"])
    # between places a cap never binds; only an id repeated inside a segment shares a category with its other rows - so
    # the cap 1 answer is the uncapped ranking with the repeats of an id dropped
    nseg = len(case["targets"])
    full = rc.expected(oracle.rank_recommendations, case, 2 ** 40)
    for limit in (2, 10):
        want = rc.expected(oracle.rank_recommendations, dict(case, caps=np.ones(nseg, np.int64)), limit)
        for s in range(nseg):
            ranking = full[0][s, :full[3][s]]
            distinct = ranking[np.sort(np.unique(ranking, return_index=True)[1])][:limit]
            assert want[0][s, :want[3][s]].tolist() == distinct.tolist()


@pytest.mark.parametrize("seed", range(4))
def test_pruning_rule_on_the_fuzz_cases(oracle, distance, seed):
    case = rc.fuzz_case(seed, lists=seed % 2 == 1, circles=seed >= 2)
    kept = kept_of(distance, case)
    nseg = len(case["targets"])
    longest = int(np.argmax(np.diff(case["offsets"])))
    for s in sorted({0, longest, nseg // 2, nseg - 1}):
        entries = entries_of(oracle, case, s, kept)
        if s == longest and seed % 2 == 0 and seed < 2:
            assert len(entries) > 768                                # the buffer compacts before the rows run out
        for n in SMALL_LIMITS:
            for cap in rc.caps_for(n):
                check_rule(entries, n, cap, seed=seed)
        check_rule(entries, 10, 2, chunk=64, seed=seed)


def test_dominant_category(oracle, mains):
    case = rc.dominant_case()
    want = rc.expected(oracle.rank_recommendations, case, rc.DOMINANT_N)
    a, kw = rc.args(case, rc.DOMINANT_N)
    assert rc.same(mains.rank_recommendations_by_category(*a, **kw), want)
    assert want[3].tolist() == [4]
    taken = case["cats"][np.searchsorted(case["place_ids"], want[0][0])]
    assert taken.tolist() == [5, 5, 6, 6]                            # two rows of B
    free = rc.expected(oracle.rank_recommendations, {k: v for k, v in case.items() if k != "caps"}, rc.DOMINANT_N)
    assert not np.array_equal(free[0], want[0])
    # "the N-th best so far" would lose them: the 4th best row overall outscores every row of B
    entries = entries_of(oracle, case, 0)
    assert len(entries) == 1003
    check_rule(entries, rc.DOMINANT_N, 2)
    check_rule(entries, rc.DOMINANT_N, 2, chunk=64)


@pytest.mark.parametrize("n_cats", [1, 3])
def test_ascending_scores_kill_every_survivor(oracle, mains, n_cats):
    case = rc.ascending_case(n_cats=n_cats)
    want = rc.expected(oracle.rank_recommendations, case, 10)
    assert want[0][0, :want[3][0]].tolist() == list(range(5000, 5000 - 2 * n_cats, -1))
    a, kw = rc.args(case, 10)
    assert rc.same(mains.rank_recommendations_by_category(*a, **kw), want)
    entries = entries_of(oracle, case, 0)
    assert len(entries) == 5000 > 768
    # in arrival order (ascending scores: the ranking reversed) every compaction's survivors are killed later
    arrive = entries[::-1]
    assert rc.block_list(arrive, 10, 2, 0) == rc.greedy(entries, 10, 2)
    assert rc.chunked(arrive, 10, 2, 64, 0) == rc.greedy(entries, 10, 2)
    check_rule(entries, 10, 2)


@pytest.mark.parametrize("chunks", rb.SEAM_CHUNKS)
def test_seam_case(oracle, mains, chunks):
    for cap in (1, 3):
        case = rc.seam_case(chunks, cap)
        assert set(case["cats"].tolist()) == {0, 1}
        for limit in rb.SEAM_LIMITS:
            want = rc.expected(oracle.rank_recommendations, case, limit)
            a, kw = rc.args(case, limit)
            assert rc.same(mains.rank_recommendations_by_category(*a, **kw), want)
            assert want[3][0] == min(limit, 2 * cap, 64 * chunks + 1)
        entries = entries_of(oracle, case, 0)
        if chunks > 1:
            # a category's top-cap rows lie in different chunks: ids descend with the row, the winners are the last rows
            # and id 5000's early copy sits in the first chunk
            want = rc.expected(oracle.rank_recommendations, case, 10)
            rows = [int(np.flatnonzero(case["ids"] == i)[0]) // 64 for i in want[0][0, :want[3][0]]]
            assert len(set(rows)) > 1
        for n in (1, 4, 10):
            check_rule(entries, n, cap, chunk=64)


def test_listing_case(oracle, mains):
    case = rc.listing_case()
    want = rc.expected(oracle.rank_recommendations, case, 5)
    a, kw = rc.args(case, 5)
    assert rc.same(mains.rank_recommendations_by_category(*a, **kw), want)
    for s, ids in enumerate(rc.LISTING_IDS):
        assert want[0][s, :want[3][s]].tolist() == ids, s


def test_refusals_of_the_restatement(mains, pkg):
    case = rc.listing_case()
    a, kw = rc.args(dict(case, caps=np.array([1, 0, 1, 1], np.int64)), 5)
    with pytest.raises(pkg.IllegalArgumentException):
        mains.rank_recommendations_by_category(*a, **kw)
