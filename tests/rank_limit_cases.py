"""Inputs that stand on the limits of the device rankers ("Limits of the rankers"): the segmented ranker's
chunk plan, its two paths and its LDS list (csrc/rank_batch.hip), and the ranked SG batch's bitmap words, tile width and
ids (csrc/sg_ranked.h).  Seeded generators in rank_batch_cases' dict layout, numpy only, no GPU and no package import.
Every limit is a literal here: 1024 list entries, compaction above 768, tiles of 256 rows, N <= 256 on the list, the
default chunk of 4096 rows, 64 emit rows a bitmap word, uint16 columns up to 65535."""
import numpy as np

import rank_batch_cases as rb

LIST_CAP, LIST_COMPACT_ABOVE, TILE_ROWS = 1024, 768, 256
NO_REGION = 99                                              # no place of any table here is in this region
PLANTED_NAN = 0x7FF8000000000BE5                            # a NaN no pool has: the planted best row is told by its bits


# ---- the list of rb_select, as a count --------------------------------------------------------------------------------

def order_key(ids, scores):
    """Rank of every row in the ranker's order (score descending with NaN first and the zeros tied, id ascending, row
    ascending): 0 is the best row, no two rows share a rank."""
    ids, scores = np.asarray(ids, np.int64), np.asarray(scores, np.float64)
    nan = np.isnan(scores)
    order = np.lexsort((np.arange(len(ids)), ids, np.where(nan, 0.0, -scores), ~nan))
    rank = np.empty(len(ids), np.int64)
    rank[order] = np.arange(len(ids))
    return rank


def members(case, s):
    """Rows of segment s that the join keeps."""
    a, b = case["offsets"][s], case["offsets"][s + 1]
    return np.isin(case["ids"][a:b], case["place_ids"][case["regions"] == case["targets"][s]])


def fill_trace(member, key, N):
    """The counting rule of rb_select for one block's rows: tiles of 256 rows; before a tile, when more than 768 entries
    stand, the list is sorted and cut to min(count, N), and with count >= N the N-th entry becomes the threshold; a row
    is appended when it is a member and strictly better than the threshold.
    -> (most entries standing after any tile, compactions)."""
    entries, thr, most, compactions = [], None, 0, 0
    for t0 in range(0, len(member), TILE_ROWS):
        if len(entries) > LIST_COMPACT_ABOVE:
            entries.sort()
            compactions += 1
            if len(entries) >= N:
                entries = entries[:N]
                thr = entries[N - 1]
        for r in range(t0, min(t0 + TILE_ROWS, len(member))):
            if member[r] and (thr is None or key[r] < thr):
                entries.append(int(key[r]))
        most = max(most, len(entries))
    return most, compactions


def case_fill(case, N):
    """fill_trace over every segment of a case that one block reads whole (no chunk switch)."""
    most, compactions = 0, 0
    for s in range(len(case["targets"])):
        a, b = case["offsets"][s], case["offsets"][s + 1]
        f, c = fill_trace(members(case, s), order_key(case["ids"][a:b], case["scores"][a:b]), N)
        most, compactions = max(most, f), compactions + c
    return most, compactions


# ---- the chunk plan ---------------------------------------------------------------------------------------------------

# a length is (a, b, has_region): a * chunk + b rows, in a region that has places or in NO_REGION
CHUNK_LENGTHS = ((1, -1, True), (1, 0, True), (1, 1, True), (2, 0, True), (2, 1, True), (0, 0, True), (3, 0, False),
                 (1, 1, True))
# split: chunk + 1 twice, 2 chunk, 2 chunk + 1; 3 chunk in NO_REGION is not
CHUNK_SPLIT, CHUNK_CHUNKS = 4, 2 + 2 + 3 + 2
TINY_LENGTHS = ((0, 100, True),) * 3              # the 300 rows for chunk = 1: every row a chunk of its own
CHUNKS = (256, 255, 257)                          # LOCREC_RANK_BATCH_CHUNK beside the default 4096: the tile, and one either side


def segment_rows(rng, n, n_members, inside, outside, pool, avoid=None, reserve=-1):
    """n rows in shuffled order, n_members of them ids of `inside` (repeats allowed, never `avoid`), the others ids of
    `outside`; scores drawn from the pool.  The row `reserve` is none of the members."""
    if avoid is not None:
        inside = inside[inside != avoid]
    is_member = np.zeros(n, bool)
    free = np.setdiff1d(np.arange(n), [reserve])
    is_member[rng.choice(free, min(n_members, len(free)), replace=False)] = True
    ids = np.where(is_member, rng.choice(inside, n), rng.choice(outside, n)).astype(np.int64)
    return ids, pool[rng.integers(0, len(pool), n)]


def chunk_case(lengths, chunk, seed=5):
    """One call's segments with the lengths a * chunk + b of `lengths`.  A third of each segment's rows (rounded down)
    are members, and the planted row beside them; the scores are the pool's 12 values, so ties straddle every chunk
    seam.  In the segments that have rows and a region, the best row - a NaN of its own bit pattern with the region's
    smallest place id, which no other row of the segment has - is planted in turn at row 0, chunk - 1, chunk, len - 1
    (cut to the segment).
    Beside the call's arrays: lengths (as computed here), planted_row and planted_id per segment (-1: none)."""
    rng = np.random.default_rng(seed)
    place_ids, regions = rb.places(seed)
    pool = rb.score_pool()
    persons = np.arange(10 ** 6, 10 ** 6 + 50)
    lens = np.array([a * chunk + b for a, b, _ in lengths], np.int64)
    targets = np.array([s % 3 if lengths[s][2] else NO_REGION for s in range(len(lengths))], np.int64)
    ids, scores, planted_row, planted_id = [], [], [], []
    turn = 0
    for s, n in enumerate(lens.tolist()):
        inside = np.unique(place_ids[regions == s % 3])
        outside = np.concatenate([np.setdiff1d(place_ids, inside), persons])
        best = int(inside.min())
        row = -1
        if n > 0 and lengths[s][2]:
            row = min((0, chunk - 1, chunk, n - 1)[turn % 4], n - 1)
            turn += 1
        si, ss = segment_rows(rng, n, n // 3, inside, outside, pool, avoid=best, reserve=row)
        if row >= 0:
            si[row] = best
            ss[row] = np.array([PLANTED_NAN], np.uint64).view(np.float64)[0]
        ids.append(si)
        scores.append(ss)
        planted_row.append(row)
        planted_id.append(best if row >= 0 else -1)
    offsets = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    return dict(offsets=offsets, ids=np.concatenate(ids), scores=np.concatenate(scores), place_ids=place_ids,
                regions=regions, targets=targets, lengths=lens, planted_row=planted_row, planted_id=planted_id)


# ---- the global path --------------------------------------------------------------------------------------------------

GLOBAL_N = (257, 511, 512, 513)       # beyond the list; one less than two 256-slot tiles of rb_emit_sorted, two, one more


def global_members(N):
    """Member rows per segment of global_case(N).  The last two segments lose every row in the join: members of region 2
    asked for NO_REGION, and places of which none is in the target region."""
    return (0, N - 1, N, 3 * N, N, 0, 0)


GLOBAL_TARGETS = (0, 1, 2, 0, 1, NO_REGION, 2)
GLOBAL_TARGETS_DROPPED = (0, NO_REGION, 5, -1, NO_REGION, NO_REGION, 2)    # no row of any segment is kept: m = 0


def global_case(N, all_dropped=False, seed=9):
    """Segments with 0, N - 1, N, 3 N and N member rows, each with as many other rows beside them (40 where there is no
    member), then two segments whose rows the join drops.  all_dropped: the same rows under targets that keep no row
    of any segment - regions nobody has, and the two segments whose rows are no places of their region."""
    rng = np.random.default_rng(seed)
    place_ids, regions = rb.places(seed)
    pool = rb.score_pool()
    persons = np.arange(10 ** 6, 10 ** 6 + 50)
    ids, scores, lens = [], [], []
    for s, c in enumerate(global_members(N)):
        region = 2 if s >= 5 else GLOBAL_TARGETS[s]
        inside = np.unique(place_ids[regions == region])
        outside = np.concatenate([np.setdiff1d(place_ids, inside), persons])
        if s == 5:
            n, c = 3 * N, N
        else:
            n = 2 * c if c else 40
        si, ss = segment_rows(rng, n, c, inside, outside, pool)
        ids.append(si)
        scores.append(ss)
        lens.append(n)
    offsets = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    targets = np.array(GLOBAL_TARGETS_DROPPED if all_dropped else GLOBAL_TARGETS, np.int64)
    return dict(offsets=offsets, ids=np.concatenate(ids), scores=np.concatenate(scores), place_ids=place_ids,
                regions=regions, targets=targets)


# ---- the graphs of the ranked SG batch --------------------------------------------------------------------------------

BIT_SIZES = ((63, 64), (64, 65), (65, 128), (128, 255), (255, 256), (256, 257), (257, 513))   # (n_live, n_vertices)


def bit_graph_on(vid, n_live, rng, likes=3):
    """The bit graph over the vertex ids vid: vid[:n_cat] categories, vid[n_cat:n_live] places, the rest persons."""
    n_cat = 3
    cats, plc, persons = vid[:n_cat], vid[n_cat:n_live], vid[n_live:]
    liked = np.concatenate([rng.choice(plc, likes, replace=False) for _ in persons])
    src = np.concatenate([np.repeat(persons, likes), np.repeat(plc, n_cat), np.repeat(cats, len(plc))])
    dst = np.concatenate([liked, np.tile(cats, len(plc)), np.tile(plc, n_cat)])
    w = np.concatenate([np.full(len(liked), 1.0 / likes), np.full(len(plc) * n_cat, 1.0 / n_cat),
                        np.full(n_cat * len(plc), 1.0 / len(plc))])
    return src.astype(np.int64), dst.astype(np.int64), w, cats, plc, persons


def sg_bit_graph(n_live, n_vertices, seed=0):
    """n_live live vertices (3 categories, the rest places) and n_vertices - n_live persons (sources only) that like 3
    places each; every place points to every category and every category to every place, so every live vertex is
    reached from every target; a source's weights sum to 1.  The ids are a shuffle of 100 .. 100 + n_vertices - 1, so the
    persons lie between the live vertices.  The places table lists EVERY vertex once, shuffled, with region == vertex id:
    a request for region r returns vertex r or nothing.
    -> dict(src, dst, w, place_ids, regions, person, place): the last two are the two targets of the tests."""
    rng = np.random.default_rng(seed + 1000 * n_live + n_vertices)
    vid = (100 + rng.permutation(n_vertices)).astype(np.int64)
    src, dst, w, cats, plc, persons = bit_graph_on(vid, n_live, rng)
    table = vid[rng.permutation(n_vertices)]
    return dict(src=src, dst=dst, w=w, place_ids=table, regions=table.copy(), person=int(persons[0]), place=int(plc[0]))


EXTREME_IDS = (rb.I64_MIN, rb.I64_MIN + 1, -1, 0, rb.I64_MAX - 1, rb.I64_MAX)
EXTREME_REGIONS = (rb.I64_MIN, -5, rb.I64_MAX)


def sg_extreme_graph(seed=4):
    """The bit graph's shape on 40 vertices (28 live) whose ids include the ends of int64, -1 (the padding value of the
    result) and 0, spread over categories, places and persons; the places table lists every vertex once in one of the
    regions I64_MIN, -5, I64_MAX."""
    rng = np.random.default_rng(seed)
    n_vertices, n_live = 40, 28
    others = np.concatenate([rng.integers(-2 ** 62, 2 ** 62, n_vertices - len(EXTREME_IDS) - 2), [-2, 1]])
    vid = np.concatenate([EXTREME_IDS, others]).astype(np.int64)
    assert len(np.unique(vid)) == n_vertices
    vid = vid[rng.permutation(n_vertices)]
    src, dst, w, cats, plc, persons = bit_graph_on(vid, n_live, rng)
    table = vid[rng.permutation(n_vertices)]
    regions = np.array(EXTREME_REGIONS, np.int64)[rng.integers(0, 3, n_vertices)]
    return dict(src=src, dst=dst, w=w, place_ids=table, regions=regions, vertices=np.sort(vid))


# (live vertices, targets of a tile): min(16, 65535 - T) with uint16 columns, 16 without
NARROW_T = ((65533, 2), (65534, 1), (65535, 16))


def sg_narrow_tile_graph(T):
    """The graph of test_gpu_sg_limits.test_uint16_columns_at_their_limit (the same construction): T live vertices
    0 .. T - 1, 1500 source-only persons 100000 .., and its 19 targets (17 distinct).  The places table: the 200 live
    ids at either end of the rows, the vertices that the first 40 reach in four steps, and a dozen persons, regions
    id % 3; the targets' regions cycle 0, 1, 2 and one asks for NO_REGION."""
    n_persons = 1_500
    live = np.arange(T, dtype=np.int64)
    persons = 100_000 + np.arange(n_persons, dtype=np.int64)
    src = np.concatenate([persons[live % n_persons], live, persons[:40]])
    dst = np.concatenate([live, (live * 7 + 1) % T, np.arange(40, dtype=np.int64)])
    uniq, inv = np.unique(src, return_inverse=True)
    w = 1.0 / np.bincount(inv)[inv]
    targets = np.array([100_000, 5, T - 1, 100_001, 0, 100_039, 100_002, 100_003, T - 1, 100_004, 7, 100_005, 100_000,
                        100_006, 100_007, 100_008, 100_009, 100_010, 100_011], np.int64)
    # the first and the last 200 live rows, and what the first 40 reach in four steps (the targets' rows after sweeps)
    reached, step = [], np.arange(40, dtype=np.int64)
    for _ in range(4):
        step = (step * 7 + 1) % T
        reached.append(step)
    place_ids = np.unique(np.concatenate([np.arange(0, 200), np.arange(T - 200, T)] + reached))
    place_ids = np.concatenate([place_ids, persons[:12]]).astype(np.int64)
    place_ids = place_ids[np.random.default_rng(T).permutation(len(place_ids))]
    regions = place_ids % 3
    target_regions = (np.arange(len(targets)) % 3).astype(np.int64)
    target_regions[6] = NO_REGION
    return dict(src=src, dst=dst, w=w, targets=targets, place_ids=place_ids, regions=regions, target_regions=target_regions)


def live_count(src, dst):
    """Vertices that are some edge's target."""
    return len(np.unique(dst))
