"""Inputs of the excluding ranker's tests (locrec_rank_recommendations_batch_excluding): rank_batch_cases' cases with a
list of ids per segment to leave out.  Seeded generators, no GPU.  A case is rank_batch_cases' dict plus ex_offsets and
ex_ids; the expected value is an existing single ranker applied per segment to the rows that survive
~np.isin(ids, list)."""
import numpy as np

import rank_batch_cases as rb

LIST_LENGTHS = (0, 1, 2, 63, 64, 65, 1000)
LIMITS = (1, 10, 256, 257, 2 ** 40)
LACKING = 3_000_000        # ids from here on are in no fuzz case (places 1000..8999, non-places 10^6..10^6 + 49)
EXTREMES = (rb.I64_MIN, rb.I64_MAX, -1, 0)


def likely_winners(case, s):
    """The ids of segment s's rows that are places of its target region, best score first (Spark's order of doubles:
    NaN above +inf), then id - near enough to the ranking that the head of this list holds the segment's winners; the
    CPU test measures with the oracle how often excluding them changes the result."""
    a, b = case["offsets"][s], case["offsets"][s + 1]
    ids, scores = case["ids"][a:b], case["scores"][a:b]
    member = np.isin(ids, case["place_ids"][case["regions"] == case["targets"][s]])
    ids, scores = ids[member], scores[member]
    key = np.where(np.isnan(scores), np.inf, scores)
    order = np.lexsort((ids, -key, ~np.isnan(scores)))
    _, first = np.unique(ids[order], return_index=True)
    return ids[order][np.sort(first)]                      # distinct, in ranking order


def one_list(rng, winners, length):
    """`length` ids: winners first (half the list at the most, the whole ranking when it is shorter), then the int64
    extremes, ids the segment lacks and repeats of what is already listed; shuffled."""
    if length == 0:
        return np.empty(0, np.int64)
    if length == 1:
        return np.array([winners[0] if len(winners) else rb.I64_MIN], np.int64)
    out = list(winners[:max(1, length // 2)])
    out += list(EXTREMES[:max(1, min(4, length - len(out) - 1))]) if len(out) < length else []
    while len(out) < length:
        out.append(LACKING + int(rng.integers(0, 1000)) if rng.random() < 0.5 or not out else out[int(rng.integers(0, len(out)))])
    return rng.permutation(np.array(out[:length], np.int64))


def with_lists(case, lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    ids = np.concatenate(lists).astype(np.int64) if lists else np.empty(0, np.int64)
    return dict(case, ex_offsets=off, ex_ids=ids)


def fuzz_case(seed):
    """rank_batch_cases.fuzz_case(seed) with a list per segment; the lengths cycle through LIST_LENGTHS, starting
    somewhere else in every case."""
    case = rb.fuzz_case(seed)
    rng = np.random.default_rng(7000 + seed)
    nseg = len(case["targets"])
    lists = [one_list(rng, likely_winners(case, s), LIST_LENGTHS[(seed + s) % len(LIST_LENGTHS)]) for s in range(nseg)]
    return with_lists(case, lists)


def empty_lists(case):
    return with_lists(case, [np.empty(0, np.int64)] * len(case["targets"]))


def list_of(case, s):
    return case["ex_ids"][case["ex_offsets"][s]:case["ex_offsets"][s + 1]]


def filtered(case):
    """The case without the excluded rows (and without the lists): what a caller would hand to the plain ranker."""
    off = case["offsets"]
    keep = np.ones(len(case["ids"]), bool)
    lens = np.zeros(len(case["targets"]), np.int64)
    for s in range(len(case["targets"])):
        a, b = off[s], off[s + 1]
        keep[a:b] = ~np.isin(case["ids"][a:b], list_of(case, s))
        lens[s] = keep[a:b].sum()
    keep[:off[0]] = keep[off[-1]:] = False
    new_off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=new_off[1:])
    out = {k: v for k, v in case.items() if not k.startswith("ex_")}
    return dict(out, offsets=new_off, ids=case["ids"][keep], scores=case["scores"][keep])


def widened(result, width):
    """A ranked batch's (ids, scores, counts) padded to `width` columns with id -1 / score 0.0."""
    ri, rs, rc = (np.asarray(x) for x in result)
    oi, osc = np.full((len(rc), width), -1, np.int64), np.zeros((len(rc), width))
    oi[:, :ri.shape[1]], osc[:, :rs.shape[1]] = ri, rs
    return oi, osc, rc


def width_of(case, limit):
    nseg = len(case["targets"])
    return max(0, min(int(limit), int(np.diff(case["offsets"]).max()) if nseg else 0))


def expected(rank, case, limit):
    """The per-segment loop of `rank` over the surviving rows, in the excluding call's layout: W is the limit cut to the
    longest segment BEFORE the exclusion."""
    return widened(rb.expected(rank, filtered(case), limit), width_of(case, limit))


def args(case):
    return rb.args(case), (case["ex_offsets"], case["ex_ids"])


# ---- hand-made cases ---------------------------------------------------------------------------------------------------

def handmade():
    """Segments 0 and 1 hold the same six rows of region 4: ids 10..15, scores 6, 5, 5, 3, 2, 1 (11 and 12 tie); place 13
    is listed twice in the places table.  The lists: the winner alone; 12 (one of the tie) and 13 (the place listed
    twice), 12 twice; every id of the segment; nothing."""
    ids = np.tile(np.arange(10, 16, dtype=np.int64), 4)
    scores = np.tile(np.array([6.0, 5.0, 5.0, 3.0, 2.0, 1.0]), 4)
    place_ids = np.array([10, 11, 12, 13, 13, 14, 15, 99], np.int64)
    case = dict(offsets=np.arange(0, 25, 6, dtype=np.int64), ids=ids, scores=scores, place_ids=place_ids,
                regions=np.full(len(place_ids), 4, np.int64), targets=np.full(4, 4, np.int64))
    lists = [np.array([10], np.int64), np.array([12, 13, 12], np.int64), np.arange(15, 9, -1, dtype=np.int64), np.empty(0, np.int64)]
    return with_lists(case, lists)


HANDMADE_IDS = ([11, 12, 13, 14, 15], [10, 11, 14, 15], [], [10, 11, 12, 13, 14, 15])


def seam_lists(chunks, chunk=64):
    """rank_batch_cases.seam_case's ids are 5000 + (n - 1 - row), id 5000 again at row 5.  -> the lists of the seam tests:
    id 5000 (both its rows, in two chunks), and the ids of the rows on each side of every chunk boundary."""
    n = chunk * chunks + 1
    rows = np.concatenate([[c * chunk - 1, c * chunk] for c in range(1, chunks + 1)])
    sides = (5000 + (n - 1 - rows)).astype(np.int64)
    return np.array([5000], np.int64), sides
