"""Inputs of the segmented ranker's tests (locrec_rank_recommendations_batch): seeded generators, no GPU.
A case is a dict of the call's arrays: offsets, ids, scores, place_ids, regions, targets."""
import numpy as np

LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 5000)
TARGETS = (0, 1, 2, 99)          # 99: no such region
SEGMENT_COUNTS = (1, 3, 64, 257)
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def score_pool():
    """About 12 values, so that ties are the rule: NaN of both signs and two payloads, both zeros, both infinities,
    a denormal, and a few ordinary numbers."""
    bits = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFF0000000000123,   # four NaNs
            0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,   # +-0.0, +-inf
            0x0000000000000001]                                                                # a denormal
    return np.concatenate([np.array(bits, np.uint64).view(np.float64), np.array([1.5, -2.25, 0.5])])


def places(seed, n=2000):
    """n places in regions 0..2: 1900 distinct ids, 60 rows listed twice in their region, 40 ids listed in a second
    region as well."""
    rng = np.random.default_rng(1000 + seed)
    ids = rng.choice(np.arange(1000, 9000), n - 100, replace=False).astype(np.int64)
    reg = rng.integers(0, 3, len(ids)).astype(np.int64)
    twice = rng.choice(len(ids), 60, replace=False)
    other = rng.choice(len(ids), 40, replace=False)
    ids = np.concatenate([ids, ids[twice], ids[other]])
    reg = np.concatenate([reg, reg[twice], (reg[other] + 1) % 3])
    order = rng.permutation(len(ids))
    return ids[order], reg[order]


def fuzz_case(seed):
    nseg = SEGMENT_COUNTS[seed % len(SEGMENT_COUNTS)]
    rng = np.random.default_rng(seed)
    place_ids, regions = places(seed)
    lens = rng.choice(LENGTHS, nseg)
    lens[0] = 5000 if seed % 2 == 0 else 257       # a long segment in every second case, whatever was drawn
    offsets = np.zeros(nseg + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    n = int(offsets[-1])
    pool = score_pool()
    ids = np.where(rng.random(n) < 0.8, rng.choice(place_ids, n),                  # places, repeated inside a segment
                   rng.integers(10 ** 6, 10 ** 6 + 50, n)).astype(np.int64)        # persons / categories: no place
    scores = pool[rng.integers(0, len(pool), n)]
    targets = rng.choice(TARGETS, nseg).astype(np.int64)
    targets[0] = seed % 3
    return dict(offsets=offsets, ids=ids, scores=scores, place_ids=place_ids, regions=regions, targets=targets)


def fuzz_limits(max_n):
    return (-1, 0, 1, 2, 10, 64, max_n, max_n + 1, 2 ** 40)


def seam_case(chunks, chunk=64):
    """One segment of chunk * chunks + 1 rows of one region, every score a zero (one tie group that straddles every
    limit and every chunk boundary), ids descending so that the winners sit in the last chunks.  The smallest id, the
    last row and alone in the last chunk, is listed again in the first chunk: the same id with the same score in two
    chunks, told apart by the zero's sign (-0.0 marks the early row, which the input-row order puts first)."""
    n = chunk * chunks + 1
    ids = (5000 + np.arange(n)[::-1]).astype(np.int64)
    scores = np.zeros(n)
    ids[5] = 5000
    scores[5] = -0.0
    place_ids = np.arange(5000, 5000 + n, dtype=np.int64)
    return dict(offsets=np.array([0, n], np.int64), ids=ids, scores=scores, place_ids=place_ids,
                regions=np.full(n, 7, np.int64), targets=np.array([7], np.int64))


SEAM_CHUNKS = (1, 3, 40)
SEAM_LIMITS = (1, 4, 5, 10, 64, 65, 256)


def extremes_case():
    """Ids and region ids at the ends of int64 and below zero."""
    place_ids = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX, -2 ** 62, 2 ** 62, I64_MAX], np.int64)
    regions = np.array([I64_MIN, I64_MAX, I64_MIN, -5, I64_MAX, I64_MIN, I64_MAX, -5, -5, I64_MIN], np.int64)
    rng = np.random.default_rng(77)
    ids = np.concatenate([rng.choice(place_ids, 300), np.array([I64_MIN + 2, I64_MAX - 2, 7], np.int64)])
    scores = score_pool()[rng.integers(0, 12, len(ids))]
    offsets = np.array([0, 100, 100, 250, len(ids)], np.int64)
    targets = np.array([I64_MIN, I64_MAX, -5, I64_MAX], np.int64)
    return dict(offsets=offsets, ids=ids, scores=scores, place_ids=place_ids, regions=regions, targets=targets)


def expected(rank, case, limit):
    """The per-segment loop of an existing single ranker `rank(ids, scores, place_ids, regions, target, limit)` in the
    batch's layout: (ids[S, W], scores[S, W], counts[S]) with W = the limit cut to the longest segment."""
    off = case["offsets"]
    nseg = len(case["targets"])
    width = max(0, min(int(limit), int(np.diff(off).max()) if nseg else 0))
    out_ids, out_scores = np.full((nseg, width), -1, np.int64), np.zeros((nseg, width))
    counts = np.zeros(nseg, np.int64)
    for s in range(nseg):
        ri, rs = rank(case["ids"][off[s]:off[s + 1]], case["scores"][off[s]:off[s + 1]], case["place_ids"], case["regions"],
                      int(case["targets"][s]), width)
        counts[s] = len(ri)
        out_ids[s, :len(ri)], out_scores[s, :len(ri)] = ri, rs
    return out_ids, out_scores, counts


def same(got, want):
    """Equal ids, counts and score BITS (nothing is computed, only moved)."""
    gi, gs, gc = (np.asarray(x) for x in got)
    wi, ws, wc = want
    return (gi.shape == wi.shape and np.array_equal(gi, wi) and np.array_equal(gc, wc)
            and np.array_equal(np.ascontiguousarray(gs, np.float64).view(np.uint64), np.ascontiguousarray(ws).view(np.uint64)))


def args(case):
    return [case[k] for k in ("offsets", "ids", "scores", "place_ids", "regions", "targets")]
