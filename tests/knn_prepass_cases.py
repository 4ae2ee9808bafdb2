"""The data sets of tests/test_gpu_knn_prepass_limits.py and, for each, the assertions - on the model of
knn_prepass_model.py alone, no GPU - that the data set holds the counts its case is about.  test_knn_prepass_model.py
runs these assertions without a GPU; the GPU module runs them again before it launches anything.

Every data set is built from per-row lists of (tail place, value): build() adds head places so that the index keeps
the input order (it sorts by place count, category count, head count, stably: the place count grows whenever the
tail count grows from one row to the next, and inside one place count the head count never falls), and asserts
that the hot places are the more frequent ones, so that with LOCREC_KNN_HT_H = hot they are the head."""
import numpy as np

import knn_prepass_model as M

C_DIM = 12


def build(tails, hot, cold, seed, min_heads=4, person0=9000, head_value=None):
    """tails[i] = [(cold place number 0 .. cold - 1, value)] of row i.  -> the data set; places 0 .. hot - 1 are hot."""
    rng = np.random.default_rng(seed)
    n = len(tails)
    prp, pidx, pval, crp, cidx, cval = [0], [], [], [0], [], []
    places = len(tails[0]) + min_heads
    nxt = 0
    for i in range(n):
        t = len(tails[i])
        if i and t > len(tails[i - 1]):
            places = max(places + 1, t + min_heads)   # a longer tail starts a new place count ...
        heads = places - t                            # ... so the head count never falls inside one place count
        assert min_heads <= heads <= hot, (i, heads)
        hp = (nxt + np.arange(heads)) % hot       # round robin: every hot place is about equally frequent
        nxt += heads
        ip = np.array(list(hp) + [hot + p for p, _ in tails[i]], np.int64)
        hv = rng.integers(1, 9, size=heads) if head_value is None else np.full(heads, head_value)
        iv = np.array(list(hv) + [v for _, v in tails[i]], np.float64)
        by = np.argsort(ip)
        assert len(set(ip.tolist())) == len(ip), (i, "a place twice")
        pidx.append(ip[by]); pval.append(iv[by]); prp.append(prp[-1] + len(ip))
        ic = np.sort(rng.choice(C_DIM, size=4, replace=False))
        cidx.append(ic); cval.append(rng.integers(1, 30, size=4).astype(np.float64)); crp.append(crp[-1] + 4)
    d = {"person_ids": rng.permutation(np.arange(person0, person0 + n)).astype(np.int64),
         "p_rowptr": np.array(prp, np.int64), "p_idx": np.concatenate(pidx).astype(np.int32), "p_val": np.concatenate(pval),
         "p_dim": hot + cold,
         "c_rowptr": np.array(crp, np.int64), "c_idx": np.concatenate(cidx).astype(np.int32), "c_val": np.concatenate(cval),
         "c_dim": C_DIM}
    freq = np.bincount(d["p_idx"], minlength=d["p_dim"])
    assert freq[:hot].min() > freq[hot:].max(), ("the hot places must be the head", freq[:hot].min(), freq[hot:].max())
    ss = np.add.reduceat(d["p_val"] ** 2, d["p_rowptr"][:-1])
    assert ss.max() < 65536 and d["p_val"].max() < 256, "every row must stay in the packed 16-bit format"
    assert np.array_equal(M.index_order(d, hot), np.arange(n)), "the index must keep the input order"
    return d


class Pool:
    """`size` cold places from `first` on, handed out in turn: draw number j takes place j mod size, so a place is held by
    (draws / size) rows, spread evenly over the rows that draw."""

    def __init__(self, first, size):
        self.first, self.size, self.next = first, size, 0

    def take(self, k, rng):
        out = [(self.first + (self.next + j) % self.size, int(rng.integers(1, 9))) for j in range(k)]
        self.next += k
        return out


# ---- C1 / C2 / C3: 2,240 persons = 35 slices = 140 tiles ------------------------------------------------------------
#
# Sub-ranges of 8 slices start at rows 0, 512, 1024, 1536, 2048; of 16 slices at rows 0, 1024, 2048.
#   BC    held by 512 rows below row 1024: 256 below row 512, 256 from there on
#   BO    held by 304 rows of 512 .. 1023 which hold BC too
#   BA    held by the tile OVER and by 200 rows of 1024 .. 1535
#   FULL  a tile whose rows hold BC and nothing else: 16 x 512 = 8,192 hits in one sub-range of 16 slices under the
#         default stage, 16 x 256 = 4,096 in each of two sub-ranges of 8 slices under a stage of 4,096
#   OVER  a tile of rows 512 .. 1023 whose rows hold BC, BO, BA and a filler: under the default stage (width 8)
#         4,096 + a few hits in slices 0 - 7, 16 x (256 + 304) and more in slices 8 - 15 (overflow), 16 x 200 and a few in
#         slices 16 - 23
#   dense four kinds of tiles, twelve of each, spread over the index, whose rows hold many places of few holders:
#         (tail places per row, holders per place) = (56, 8), (40, 12), (20, 24), (10, 48) - under a stage of 4,096 about
#         7,500 hits per tile in sub-ranges of 8 slices and 0.46 x holders postings per entry and sub-range, doubled:
#         segments of 4, 8, 16 and 32 lanes.  The rows of a (56, 8) tile also share one place of their own: an entry
#         with 16 postings in one sub-range where the segment is 4.
#   light every other row: three tail places (BC, BO, BA count) filled up with fillers of 7 holders
C1_N, C1_HOT = 2240, 128
DENSE = ((56, 8), (40, 12), (20, 24), (10, 48))
C1_FULL_TILE, C1_OVER_TILE = 20, 33
C1_LEFT_OUT = (3, 130, 600, 1290, 2200)


def c1_dataset():
    rng = np.random.default_rng(11)
    ntiles = C1_N // 16
    kind = {}                                   # tile -> dense kind
    for k in range(4):
        for j in range(12):
            kind[1 + 3 * k + 11 * j] = k
    assert len(kind) == 48 and max(kind) < ntiles and C1_FULL_TILE not in kind and C1_OVER_TILE not in kind
    cold = 0
    pools = []
    for t, a in DENSE:
        pools.append(Pool(cold, 192 * t // a))
        cold += pools[-1].size
    own = cold                                   # one place of its own for every (56, 8) tile
    cold += 12
    BC, BO, BA = cold, cold + 1, cold + 2
    cold += 3
    light_tiles = [t for t in range(ntiles) if t not in kind and t not in (C1_FULL_TILE, C1_OVER_TILE)]
    low = [t for t in light_tiles if t < 32]
    high = [t for t in light_tiles if 32 <= t < 64]
    bc_tiles = set(low[:15] + high[:15])        # + FULL (below row 512) and OVER (above): 16 tiles = 256 rows each side
    bo_tiles = set(high[:18])                    # + OVER: 19 tiles = 304 rows
    ba_tiles = [t for t in light_tiles if 64 <= t < 96][:13]
    fill = Pool(cold, len(light_tiles) * 16 * 3 // 7)   # three draws per light row at the most: 7 holders or fewer
    cold += fill.size
    own_seen = 0
    tails = []
    for t in range(ntiles):
        for i in range(16):
            if t == C1_FULL_TILE:
                row = [(BC, 3)]
            elif t == C1_OVER_TILE:
                row = [(BC, 2), (BO, 5), (BA, 7)] + fill.take(1, rng)
            elif t in kind:
                k = kind[t]
                row = pools[k].take(DENSE[k][0], rng)
                if k == 0:
                    row.append((own + own_seen // 16, 4))
                    own_seen += 1
            else:
                row = []
                if t in bc_tiles:
                    row.append((BC, 1 + i % 7))
                if t in bo_tiles:
                    row.append((BO, 1 + i % 5))
                if t in ba_tiles and (ba_tiles.index(t) * 16 + i) < 200:
                    row.append((BA, 1 + i % 3))
                row += fill.take(3 - len(row), rng)
            tails.append(row)
    d = build(tails, C1_HOT, cold, seed=12)
    freq = np.bincount(d["p_idx"], minlength=d["p_dim"])[C1_HOT:]
    assert freq[BC] == 512 and freq[BO] == 304 and freq[BA] == 216
    return d


def rows_of_form(n, form, left_out):
    """The batch's query rows: every row, or every row but `left_out` (tiles shift, nq is no multiple of 16)."""
    return np.delete(np.arange(n), left_out) if form == "rows_left_out" else np.arange(n)


def c1_check(m):
    """m = the model of the whole index as one batch (range and full row list).  What C1, C2 and C3 rely on."""
    assert m.slices == 35 and m.ntiles == 140
    F, O = C1_FULL_TILE, C1_OVER_TILE
    # ---- C1, default stage = 8,192: ht_build_hits<16, 16>
    assert m.subranges(F, 8192) == [(0, 16, 8192, "full"), (16, 16, 0, "empty"), (32, 3, 0, "empty")]       # (b), (f)
    assert m.subranges(O, 8192) == [(0, 8, 4112, "staged"), (8, 8, 9232, "overflow"), (16, 8, 3216, "staged"),
                                    (24, 8, 32, "staged"), (32, 3, 16, "staged")]                            # (a), (c), (d)
    assert M.records_per_thread(8192) == 16 and 4112 > 8 * 512, "records r >= 8 are live"
    for stage in (8192, 4097, 4096):                                                                          # (e)
        assert {x for t in range(m.ntiles) for x in m.misalignments(t, stage)} == {0, 1, 2, 3}, stage
    assert m.routes(8192) == {"empty": 35, "staged": 280, "full": 1, "overflow": 31}
    # ---- 4,097: the smallest stage of <16, 16>; FULL's halves of 4,096 hits are staged, not full
    assert M.records_per_thread(4097) == 16 and M.records_per_thread(4096) == 8
    assert m.subranges(F, 4097)[:2] == [(0, 8, 4096, "staged"), (8, 8, 4096, "staged")]
    assert m.routes(4097) == {"empty": 50, "staged": 459, "full": 0, "overflow": 46}
    # ---- C2, stage 4,096: ht_build_hits<16, 8> at its top
    assert m.subranges(F, 4096)[:3] == [(0, 8, 4096, "full"), (8, 8, 4096, "full"), (16, 8, 0, "empty")]
    over = m.subranges(O, 4096)
    assert over[:5] == [(0, 4, 2576, "staged"), (4, 4, 1536, "staged"), (8, 4, 5392, "overflow"), (12, 4, 3840, "staged"),
                        (16, 4, 2576, "staged")] and len(over) == 9 and over[-1][1] == 3
    assert 5 * 512 < 2576 and 3840 < 4096, "records 5 - 7 are live in a staged sub-range"
    assert m.routes(4096) == {"empty": 50, "staged": 454, "full": 5, "overflow": 46}
    # ---- C3: segment sizes; where the segment is 4, an entry with 9 or more postings in one sub-range
    segs = {stage: sorted({m.segment(t, stage) for t in range(m.ntiles)}) for stage in (8192, 4097, 4096)}
    assert segs[8192] == [8, 16, 32, 64] and segs[4097] == segs[4096] == [4, 8, 16, 32, 64], segs
    four = [t for t in range(m.ntiles) if m.segment(t, 4096) == 4]
    assert len(four) == 12 and all(m.max_entry_postings(t, 4096) == 16 for t in four)
    assert all(m.entries[t] == 16 * 57 <= 1024 for t in four)
    assert all(route == "staged" for t in four for _, _, n, route in m.subranges(t, 4096) if n)


# ---- C4: kHtMaxEntries.  128 persons: 64 light rows, then 64 rows of 64 tail places each (four holders per place):
# any 16 of them are a tile of 1,024 entries.  `extra`: the last row holds one more tail place of its own - 1,025.
C4_N, C4_HOT = 128, 16


def c4_dataset(extra=False):
    rng = np.random.default_rng(21)
    heavy = Pool(0, 64 * 64 // 4)
    light = Pool(heavy.size, 64 * 2 // 4)
    cold = heavy.size + light.size + 1
    tails = [light.take(2, rng) for _ in range(64)] + [heavy.take(64, rng) for _ in range(64)]
    if extra:
        tails[-1] = tails[-1] + [(cold - 1, 3)]
    return build(tails, C4_HOT, cold, seed=22)


def c4_check(m, m_extra):
    assert m.ntiles == 8 and m.entries.tolist() == [32] * 4 + [1024] * 4
    assert m_extra.entries.tolist() == [32] * 4 + [1024] * 3 + [1025]
    assert all(m.subranges(t, 8192) == [(0, 2, int(m.counts[t].sum()), "staged")] for t in range(8))
    assert m.counts[4:].sum(axis=1).tolist() == [4096] * 4


# ---- C5: more than 1,024 tiles.  16,408 persons (257 slices, 1,026 tiles, the last of 8): three tail places, from row
# 8,200 on two, each place held by three rows.
C5_N, C5_HOT = 16408, 8
C5_SAMPLE = np.concatenate([np.arange(0, 1023 * 16, 75)[:216], np.arange(1023 * 16, C5_N)])   # 216 + the rows of tiles 1,023 - 1,025


def c5_dataset():
    rng = np.random.default_rng(31)
    pool = Pool(0, (8200 * 3 + 8208 * 2) // 3 + 1)
    return build([pool.take(3 if i < 8200 else 2, rng) for i in range(C5_N)], C5_HOT, pool.size, seed=32)


def c5_check(m):
    assert m.ntiles == 1026 and m.slices == 257 and m.entries[-1] == 8 * 2 and m.entries[0] == 48
    assert len(C5_SAMPLE) == 256 and set(range(1023 * 16, C5_N)) <= set(C5_SAMPLE.tolist())
    assert 20000 < m.tile_base[-1] < 200000 and m.tile_base[1024] < m.tile_base[1025] < m.tile_base[1026]
    assert (m.counts.sum(axis=1) > 0).all(), "every tile has hits: every tile_base entry differs from its neighbour"


# ---- C6: hit-word and accumulator extremes.  130 persons.
#   P      held with value 255 by row 15 (query 15 of tile 0) and row 63 (lane 63 of slice 0): the hit word with lane,
#          query and product at their maxima
#   Q1-Q4  held with values (255, 22, 5, 1) by rows 0 and 2, which hold nothing else: sum of squares 65,535, so the
#          tail-only dot of query 0 (even) with candidate 2 - and with itself - is exactly 65,535; row 1 (its odd
#          neighbour in the scan's packed accumulator) holds Q4 with value 1: a non-zero dot on the same candidates.
#          (255 x 255 + 255 x 2 needs two values of 255 in one row: a sum of squares of 130,050, which the packed 16-bit
#          format - the head / tail form's condition - does not hold.  By Cauchy-Schwarz a dot of 65,535 between two
#          rows whose sums of squares are below 65,536 needs two equal rows of sum of squares 65,535: these.)
C6_N, C6_HOT = 130, 8
C6_Q = ((1, 255), (2, 22), (3, 5), (4, 1))


def c6_dataset():
    rng = np.random.default_rng(41)
    pool = Pool(5, 130 // 3 + 2)
    tails = []
    for i in range(C6_N):
        if i in (0, 2):
            tails.append(list(C6_Q))
        elif i == 1:
            tails.append([(4, 1)] + pool.take(3, rng))
        elif i in (15, 63):
            tails.append([(0, 255)])
        else:
            tails.append(pool.take(1, rng))
    return build(tails, C6_HOT, 5 + pool.size, seed=42, min_heads=0)


def c6_check(m, d):
    word = (63 << 21) | (15 << 16) | (255 * 255)
    assert word == 0x7EFFE01 and word in m.slice_words(0, 0).tolist()
    w = m.slice_words(0, 0).astype(np.int64)

    def dot(q, lane):   # the tail-only dot of query q of tile 0 with the candidate in `lane` of slice 0
        return int((w & 0xFFFF)[(((w >> 16) & 31) == q) & ((w >> 21) == lane)].sum())
    assert dot(0, 2) == 65535 and dot(0, 0) == 65535 and dot(1, 2) == 1 and dot(1, 0) == 1
    ss = np.add.reduceat(d["p_val"] ** 2, d["p_rowptr"][:-1])
    assert ss[0] == ss[2] == 65535 and ss.max() == 65535


# ---- C7: the scan's hit loops.  640 persons = 10 slices; tile 0 (rows 0 - 15) reaches
#   slice 1: 1 hit      slice 2: 63          slice 3: 64        slice 4: 64 + 1      slice 5: 2 x 63 + 1 = 127
#   slice 6: 2 x 64     slice 7: 2 x 64 + 1  slice 8: 16 x 64   slice 9: none
# through places held by 1, 63 or 64 rows of the slice and by one, two or all sixteen of the tile's rows.
C7_N, C7_HOT = 640, 8
C7_WANT = {1: 1, 2: 63, 3: 64, 4: 65, 5: 127, 6: 128, 7: 129, 8: 1024, 9: 0}
# place -> (query rows of tile 0, slice, candidate rows of the slice that hold it)
C7_PLACES = {0: ((0,), 1, 1), 1: ((1,), 2, 63), 2: ((2,), 3, 64), 3: ((3,), 4, 64), 4: ((4,), 4, 1), 5: ((5, 6), 5, 63),
             6: ((7,), 5, 1), 7: ((8, 9), 6, 64), 8: ((10, 11), 7, 64), 9: ((12,), 7, 1), 10: (tuple(range(16)), 8, 64)}


def c7_dataset():
    rng = np.random.default_rng(51)
    own = Pool(len(C7_PLACES), 48)              # fillers of the query rows: one holder each
    pool = Pool(own.first + own.size, 624 * 2 // 4)
    tails = [[] for _ in range(C7_N)]
    for p, (queries, sl, rows) in C7_PLACES.items():
        for q in queries:
            tails[q].append((p, 1 + (p + q) % 7))
        for r in range(rows):
            tails[sl * 64 + 63 - r].append((p, 1 + (p + r) % 5))   # (a single holder is the slice's lane 63)
    for i in range(C7_N):
        want = 3 if i < 16 else 2
        assert len(tails[i]) <= want, i
        tails[i] += (own if i < 16 else pool).take(want - len(tails[i]), rng)
    return build(tails, C7_HOT, pool.first + pool.size, seed=52)


def c7_check(m):
    assert m.slices == 10 and {s: int(m.counts[0, s]) for s in C7_WANT} == C7_WANT
    assert m.subranges(0, 8192) == [(0, 10, int(m.counts[0].sum()), "staged")]
