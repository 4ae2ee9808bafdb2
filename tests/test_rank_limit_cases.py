"""CPU: the cases of rank_limit_cases stand where they claim.  Expected values come from the existing references
(oracle.rank_recommendations, mains.rank_recommendations_batch), never from the library under test."""
import numpy as np
import pytest

import rank_batch_cases as rb
import rank_limit_cases as rl

DEFAULT_CHUNK = 4096


@pytest.fixture(scope="module")
def mains(pkg):
    from locations_recommender_amd import mains
    return mains


# ---- the list's capacity: why no new case is added for it ---------------------------------------------------------------

def test_fill_trace_counts_what_it_says():
    """Hand-made: 1100 member rows from worst to best pass every threshold.  768 entries after three tiles do not
    compact (the rule is "more than 768"); the fourth tile makes 1024, the compaction keeps N = 10 and the last 76
    rows are appended to them."""
    n = 1100
    assert rl.fill_trace(np.ones(n, bool), np.arange(n)[::-1], 10) == (1024, 1)
    assert rl.fill_trace(np.ones(n, bool), np.arange(n), 10) == (1024, 1)          # best first: nothing after the cut
    assert rl.fill_trace(np.ones(768, bool), np.arange(768), 10) == (768, 0)
    assert rl.fill_trace(np.zeros(n, bool), np.arange(n), 10) == (0, 0)
    # fewer entries than N: the compaction keeps them all and sets no threshold
    assert rl.fill_trace(np.ones(1025, bool), np.arange(1025)[::-1], 2000) == (1025, 1)


def test_seam_case_fills_the_list_completely():
    """rb.seam_case(40), read whole by one block (no chunk switch): 2561 member rows, the winners at the end, so every
    row passes the threshold.  The list holds exactly 1024 entries before a compaction at every limit of the seam test:
    its capacity is covered by test_gpu_rank_batch.test_chunk_seam's runs without the switch."""
    case = rb.seam_case(40)
    for limit in rb.SEAM_LIMITS:
        most, compactions = rl.case_fill(case, limit)
        assert most == 1024 and compactions > 0, limit


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_cases_stay_below_the_capacity(seed):
    """Measured over seeds 0..7 and rb.fuzz_limits(256) cut to the list's N <= 256: at most 847 entries (seeds 0 and 4,
    their 5000-row segments).  The fuzz does not reach the capacity; the seam case does."""
    case = rb.fuzz_case(seed)
    most = max(rl.case_fill(case, limit)[0] for limit in rb.fuzz_limits(256) if 0 < limit <= 256)
    print("seed", seed, "most entries", most)
    assert most < 1024


# ---- the chunk plan ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", (DEFAULT_CHUNK,) + rl.CHUNKS)
def test_chunk_case(oracle, mains, chunk):
    case = rl.chunk_case(rl.CHUNK_LENGTHS, chunk)
    c = chunk
    assert np.diff(case["offsets"]).tolist() == [c - 1, c, c + 1, 2 * c, 2 * c + 1, 0, 3 * c, c + 1]
    assert case["targets"].tolist() == [0, 1, 2, 0, 1, 2, rl.NO_REGION, 1]
    assert not np.isin(rl.NO_REGION, case["regions"])
    assert case["planted_row"] == [0, c - 1, c, 2 * c - 1, 0, -1, -1, c - 1]          # row 0, chunk - 1, chunk, len - 1, ...
    bits = case["scores"].view(np.uint64)
    assert len(set(bits.tolist())) == 13                                             # the pool's 12 and the planted NaN
    for s in range(len(case["targets"])):
        a, b = case["offsets"][s], case["offsets"][s + 1]
        kept = int(rl.members(case, s).sum())
        if s == 6:
            assert kept == 0
            continue
        row = case["planted_row"][s]
        assert kept == (b - a) // 3 + int(row >= 0)                                   # a third, and the planted row
        if row < 0:
            continue
        ri, rs = oracle.rank_recommendations(case["ids"][a:b], case["scores"][a:b], case["place_ids"], case["regions"],
                                             int(case["targets"][s]), 2)
        assert ri[0] == case["planted_id"][s] == case["ids"][a + row]
        assert rs.view(np.uint64)[0] == rl.PLANTED_NAN == bits[a + row] and rs.view(np.uint64)[1] != rl.PLANTED_NAN
        # a tie across every seam of the segment: equal scores in the rows on both sides of it
        for seam in range(c, b - a, c):
            near = case["scores"][a + max(0, seam - 40):a + seam], case["scores"][a + seam:a + seam + 40]
            assert set(near[0].view(np.uint64).tolist()) & set(near[1].view(np.uint64).tolist())
    for limit in (1, 10, 256):
        want = rb.expected(oracle.rank_recommendations, case, limit)
        assert rb.same(mains.rank_recommendations_batch(*rb.args(case), limit), want)
        assert want[2].tolist() == [min(limit, (n // 3) + 1) if r >= 0 else 0
                                    for n, r in zip(np.diff(case["offsets"]).tolist(), case["planted_row"])]


def test_tiny_chunk_case(oracle):
    case = rl.chunk_case(rl.TINY_LENGTHS, 1)
    assert np.diff(case["offsets"]).tolist() == [100, 100, 100] and case["planted_row"] == [0, 0, 1]
    assert all(rl.members(case, s).sum() == 34 for s in range(3))
    want = rb.expected(oracle.rank_recommendations, case, 256)
    assert want[0].shape == (3, 100) and want[2].tolist() == [34, 34, 34]
    assert want[0][:, 0].tolist() == case["planted_id"]


# ---- the global path --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", rl.GLOBAL_N + (10,))
def test_global_case(oracle, mains, N):
    case = rl.global_case(N)
    assert [int(rl.members(case, s).sum()) for s in range(7)] == [0, N - 1, N, 3 * N, N, 0, 0]
    assert np.diff(case["offsets"]).min() > 0                               # the dropped segments have rows to drop
    assert case["targets"][5] == rl.NO_REGION and np.isin(case["targets"][6], case["regions"])
    want = rb.expected(oracle.rank_recommendations, case, N)
    assert want[0].shape == (7, N) and want[2].tolist() == [0, N - 1, N, N, N, 0, 0]
    assert rb.same(mains.rank_recommendations_batch(*rb.args(case), N), want)
    dropped = rl.global_case(N, all_dropped=True)
    assert all(dropped[k].tobytes() == case[k].tobytes() for k in ("offsets", "ids", "scores", "place_ids", "regions"))
    assert not any(rl.members(dropped, s).any() for s in range(7))
    # regions with places (their rows are read and dropped) and regions without (nothing is read)
    has = np.isin(dropped["targets"], dropped["regions"])
    assert has.any() and not has.all()
    want = rb.expected(oracle.rank_recommendations, dropped, N)
    assert want[0].shape == (7, N) and not want[2].any() and (want[0] == -1).all()


# ---- the graphs -------------------------------------------------------------------------------------------------------

def check_bit_shape(src, dst, w, n_live, n_vertices):
    vertices = np.unique(np.concatenate([src, dst]))
    assert len(vertices) == n_vertices and rl.live_count(src, dst) == n_live
    uniq, inv = np.unique(src, return_inverse=True)
    assert len(uniq) == n_vertices                                          # every vertex is a source
    np.testing.assert_allclose(np.bincount(inv, weights=w), 1.0, rtol=1e-12)
    return vertices


@pytest.mark.parametrize("n_live,n_vertices", rl.BIT_SIZES)
def test_sg_bit_graph(n_live, n_vertices):
    g = rl.sg_bit_graph(n_live, n_vertices)
    vertices = check_bit_shape(g["src"], g["dst"], g["w"], n_live, n_vertices)
    assert np.array_equal(np.sort(g["place_ids"]), vertices) and np.array_equal(g["place_ids"], g["regions"])
    assert not np.array_equal(g["place_ids"], vertices)                     # shuffled
    live = np.unique(g["dst"])
    assert g["person"] not in live and g["place"] in live
    # the persons lie between the live vertices: the numbering of the dead rows differs from the vertex order
    dead = np.setdiff1d(vertices, live)
    assert n_vertices - n_live == len(dead) and (n_vertices - n_live == 1 or np.diff(np.searchsorted(live, dead)).any())
    # every live vertex is reached from every target within three steps: two vertices two steps apart
    assert set(g["dst"][np.isin(g["src"], g["dst"][g["src"] == g["place"]])].tolist()) | \
        set(g["dst"][g["src"] == g["place"]].tolist()) == set(live.tolist())


def test_sg_bit_sizes_stand_on_the_words():
    """m is n_vertices without a sweep and n_live after one: both sets hold 63, 64, 65, 255, 256 and 257."""
    for want in (63, 64, 65, 255, 256, 257):
        assert want in [s[0] for s in rl.BIT_SIZES] and (want == 63 or want in [s[1] for s in rl.BIT_SIZES])


def test_sg_extreme_graph():
    g = rl.sg_extreme_graph()
    vertices = check_bit_shape(g["src"], g["dst"], g["w"], 28, 40)
    assert np.array_equal(vertices, g["vertices"]) and set(rl.EXTREME_IDS) <= set(vertices.tolist())
    assert rl.EXTREME_IDS == (rb.I64_MIN, rb.I64_MIN + 1, -1, 0, rb.I64_MAX - 1, rb.I64_MAX)
    assert np.array_equal(np.sort(g["place_ids"]), vertices)
    assert set(g["regions"].tolist()) == {rb.I64_MIN, -5, rb.I64_MAX}
    live = np.unique(g["dst"])
    kinds = np.isin(np.array(rl.EXTREME_IDS), live)
    assert kinds.any() and not kinds.all()                                  # extreme ids among the live and the dead
    assert -1 in live                                                       # the padding value is a row that comes back


@pytest.mark.parametrize("T,width", rl.NARROW_T)
def test_sg_narrow_tile_graph(T, width):
    g = rl.sg_narrow_tile_graph(T)
    assert rl.live_count(g["src"], g["dst"]) == T and len(np.unique(g["src"])) == T + 1500
    assert len(np.unique(np.concatenate([g["src"], g["dst"]]))) == T + 1500 and len(g["src"]) == 2 * T + 40
    assert width == (min(16, 65535 - T) if T + 2 <= 65536 else 16)
    assert len(g["targets"]) == 19 and len(np.unique(g["targets"])) == 17
    pl = g["place_ids"]
    assert len(pl) == len(np.unique(pl)) > 412 and (pl >= 100_000).sum() == 12
    assert np.isin(np.r_[np.arange(200), np.arange(T - 200, T)], pl).all() and np.isin(pl[pl < 100_000], g["dst"]).all()
    assert np.array_equal(g["regions"], pl % 3)
    asked = g["target_regions"].tolist()
    assert asked.count(rl.NO_REGION) == 1 and set(asked) == {0, 1, 2, rl.NO_REGION}
