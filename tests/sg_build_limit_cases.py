"""Edge lists that stand on the limits of the device build of the stochastic graph's layout
(csrc/sg_create_device.hip: its piece plan, its two radix sorts and its id table), and plan(): what DESIGN.md section 4
says the layout of an edge list must be, restated in numpy from the text and from neither builder's code.

Every generator returns dict(source, target, weight, requests, limit): `limit` is a sentence naming what the case stands
on, tests/test_sg_build_limit_cases.py asserts through plan() that the case does stand there, and
tests/test_gpu_sg_device_build_limits.py builds it on both builders.  Everything is drawn from synth.splitmix64 (the two
graphs moved here from tests/test_gpu_sg_limits.py keep their own construction) and the edge list is shuffled.  Unless a
case says otherwise a source's weights are count / total x beta with an odd total, so a row's sum depends on the order
of its terms.  `requests` holds the lowest and the highest vertex id, a source-only vertex where there is one (one of
them twice: the dead-slot re-patching between two requests is compared) and a row at the case's boundary."""
import numpy as np

SEED = 0x5EED5B02
SLOTS = 256                     # edge slots of a piece
DICT_MAX = 8192                 # entries of the weight dictionary
I64_MIN, I64_MAX = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
CLASS_ENDS = ((1, 4), (5, 8), (9, 16), (17, 32), (33, 64), (65, 128), (129, 255))   # remainders of class 0 .. 6


def _stream(n, salt):
    from locations_recommender_amd import synth
    return synth.splitmix64(np.arange(n, dtype=np.uint64) ^ np.uint64(SEED + salt))


# ---- what the layout must be ------------------------------------------------------------------------------------

def ceil_log2(v):
    return int(v - 1).bit_length()


def sweep_bytes(p, use16=None, dictionary=None):
    """device_sweep_bytes of plan `p`; use16 / dictionary override the form the data selects (the create-time switches
    LOCREC_SG_NO_COL16 / LOCREC_SG_NO_DICT)."""
    use16 = p["use16"] if use16 is None else use16
    dictionary = p["weight_dictionary"] > 0 if dictionary is None else dictionary
    return (p["pieces"] * SLOTS * ((2 if use16 else 4) + (2 if dictionary else 8)) + p["pieces"] * 8 + p["parts"] * 16
            + p["live"] * 16)


def plan(source, target, weight):
    """a live row (in-degree d > 0) owns d // 256 full pieces and, for rem = d % 256 > 0, one
    segment of class ceil_log2((rem + 3) // 4); a piece of class c holds 64 >> c segments, and a class's pieces are
    whole, so its last piece may carry segments no row owns."""
    source, target = np.asarray(source, np.int64), np.asarray(target, np.int64)
    bits = np.ascontiguousarray(weight, np.float64).view(np.uint64)
    ids = np.unique(np.concatenate([source, target]))
    rows, deg = np.unique(target, return_counts=True)
    nfull, rem = deg // SLOTS, deg % SLOTS
    rows_per_class = [0] * 7
    for r in rem[rem > 0]:
        rows_per_class[ceil_log2((int(r) + 3) // 4)] += 1
    pieces_per_class = [-(-n // (64 >> c)) for c, n in enumerate(rows_per_class)]
    nfull_total = int(nfull.sum())
    pieces = nfull_total + sum(pieces_per_class)
    parts = nfull_total + sum(n * (64 >> c) for c, n in enumerate(pieces_per_class))
    distinct = len(np.unique(bits))
    if pieces * SLOTS > len(source) and not np.any(bits == 0):      # padding slots hold +0.0
        distinct += 1
    p = dict(vertices=len(ids), edges=len(source), live=len(rows), n_short=int(np.sum(nfull <= 2)),
             rows_per_class=rows_per_class, pieces_per_class=pieces_per_class, nfull_total=nfull_total, pieces=pieces,
             parts=parts, wave_rows=int(np.sum(nfull > 8)), use16=len(rows) + 2 <= 65536, distinct=distinct,
             weight_dictionary=distinct if distinct <= DICT_MAX else 0,
             source_only=int(len(ids) - len(rows)))
    p["device_sweep_bytes"] = sweep_bytes(p)
    return p


def in_degree(case, v):
    return int(np.sum(case["target"] == v))


def out_degree(case, v):
    return int(np.sum(case["source"] == v))


# ---- building blocks --------------------------------------------------------------------------------------------

def _weights(src, salt):
    """count / total x beta per edge, the total of every source odd (its first edge is bumped when it is even)."""
    n = len(src)
    _, inv = np.unique(src, return_inverse=True)
    cnt = 1 + (_stream(n, salt) % np.uint64(3)).astype(np.int64)
    order = np.argsort(inv, kind="stable")
    first = order[np.concatenate(([True], inv[order][1:] != inv[order][:-1]))]
    tot = np.bincount(inv, weights=cnt).astype(np.int64)
    cnt[first] += (tot[inv[first]] % 2 == 0)
    tot = np.bincount(inv, weights=cnt).astype(np.int64)
    assert np.all(tot % 2 == 1)
    beta = np.where(inv % 3 == 0, 0.5, 1.0)
    return cnt / tot[inv].astype(np.float64) * beta


def _shuffled(src, tgt, w, salt, keep_last=False):
    n = len(src) - (1 if keep_last else 0)
    perm = np.argsort(_stream(n, salt), kind="stable")
    if keep_last:
        perm = np.concatenate([perm, [n]])
    return (np.ascontiguousarray(src[perm], np.int64), np.ascontiguousarray(tgt[perm], np.int64),
            np.ascontiguousarray(w[perm], np.float64))


def _rows_graph(rows, degs, dead, salt, dead_share=12):
    """Rows `rows` with exactly the in-degrees `degs`; a source is a vertex of `dead` (source-only) for dead_share
    sixteenths of the edges and a row otherwise; every 37th edge repeats the (source, target) pair before it.  Every
    vertex of `dead` is a source at least once (the graph must have room: more edges than len(dead))."""
    rows, degs, dead = np.asarray(rows, np.int64), np.asarray(degs, np.int64), np.asarray(dead, np.int64)
    tgt = np.repeat(rows, degs)
    n = len(tgt)
    r = _stream(n, salt)
    pick = r >> np.uint64(8)
    src = rows[(pick % np.uint64(len(rows))).astype(np.int64)]
    if len(dead):
        src = np.where(r % np.uint64(16) < dead_share, dead[(pick % np.uint64(len(dead))).astype(np.int64)], src)
    i = np.arange(n)
    rep = (i % 37 == 36) & (tgt == np.roll(tgt, 1))
    src = np.where(rep, np.roll(src, 1), src)
    if len(dead):
        assert n >= len(dead)
        src[np.arange(len(dead)) * (n // len(dead))] = dead    # one fixed edge per source-only vertex
    return src, tgt


def _requests(src, tgt, boundary):
    """Lowest and highest vertex id, the boundary rows, and two source-only vertices (the first of them twice)."""
    lo, hi = int(min(src.min(), tgt.min())), int(max(src.max(), tgt.max()))
    dead = np.setdiff1d(src, tgt)
    req = [lo, hi] + [int(b) for b in boundary]
    if len(dead):
        a, b = int(dead[len(dead) // 3]), int(dead[-1 if len(dead) < 3 else -2])
        req += [a, b, a]
    return req


def _classed_rows(rows_per_class, salt):
    """-> (class, position in its class) of the vertices 0 .. n-1: a fixed shuffle decides which vertex belongs to
    which class, so "ascending vertex inside a class" is not "ascending class"."""
    cls = np.repeat(np.arange(7), rows_per_class)
    n = len(cls)
    cls_of = np.empty(n, np.int64)
    cls_of[np.argsort(_stream(n, salt), kind="stable")] = cls
    pos = np.zeros(n, np.int64)
    for c in range(7):
        members = np.flatnonzero(cls_of == c)
        pos[members] = np.arange(len(members))
    return cls_of, pos


def _class_degrees(cls_of, pos):
    """The remainder of the k-th row of a class is the class's low end for even k and its high end for odd k."""
    ends = np.array(CLASS_ENDS, np.int64)
    return ends[cls_of, pos % 2]


# ---- 1. remainder classes ---------------------------------------------------------------------------------------

SPILL_DEAD0, SPILL_N_DEAD = 1000, 200


def class_spill():
    """Every class c has (64 >> c) + 1 rows, so its last row (in live order) opens a second piece.  In classes 0 .. 5
    that row also owns 1 or 2 full pieces, and so does the second row of the class's first piece.  The row with 3 full
    pieces is the last live row (the long area follows the short rows), so it IS the spilled row of its class: it is
    put in class 6, whose second piece (one segment per piece) the older graphs reach already - there the spilled row
    has 3 full pieces instead of 1 or 2."""
    per = [(64 >> c) + 1 for c in range(7)]
    cls_of, pos = _classed_rows(per, 11)
    degs = _class_degrees(cls_of, pos)
    nfull = np.zeros(len(degs), np.int64)
    for c in range(7):
        nfull[(cls_of == c) & (pos == per[c] - 1)] = 3 if c == 6 else 1 + c % 2
        nfull[(cls_of == c) & (pos == (0 if c == 6 else 1))] = 2 - c % 2
    degs = degs + nfull * SLOTS
    rows = np.arange(len(degs), dtype=np.int64)
    src, tgt = _rows_graph(rows, degs, SPILL_DEAD0 + np.arange(SPILL_N_DEAD), 12)
    s, t, w = _shuffled(src, tgt, _weights(src, 13), 14)
    spilled = [int(rows[(cls_of == c) & (pos == per[c] - 1)][0]) for c in (0, 3, 6)]
    return dict(source=s, target=t, weight=w, requests=_requests(s, t, spilled), cls_of=cls_of, pos=pos, nfull=nfull,
                limit="every remainder class has one row more than a piece holds: two pieces per class")


def class_exact():
    """Exactly 64 >> c rows per class: every class is one full piece, no segment is unowned (seg_out has no -1)."""
    per = [64 >> c for c in range(7)]
    cls_of, pos = _classed_rows(per, 21)
    degs = _class_degrees(cls_of, pos)
    degs[(pos == 0) & (cls_of % 2 == 0)] += SLOTS               # a full piece in front of some of the segments
    rows = np.arange(len(degs), dtype=np.int64)
    src, tgt = _rows_graph(rows, degs, 1000 + np.arange(150), 22)
    s, t, w = _shuffled(src, tgt, _weights(src, 23), 24)
    last = [int(rows[(cls_of == c) & (pos == per[c] - 1)][0]) for c in (0, 6)]
    return dict(source=s, target=t, weight=w, requests=_requests(s, t, last),
                limit="every remainder class fills exactly one piece: parts == full pieces + rows")


def classes_alternate(odd):
    """Only the classes 1, 3, 5 (odd) or 0, 2, 4, 6 are populated, three rows each; in the odd variant class 3 has
    (64 >> 3) + 1 = 9 rows, so a spilled class (two pieces) lies between two empty ones, and class 5's three rows spill
    as well.  Neighbouring classes then begin at the same piece and the same part."""
    per = [0] * 7
    for c in range(1 if odd else 0, 7, 2):
        per[c] = 3
    if odd:
        per[3] = 9
    cls_of, pos = _classed_rows(per, 31 + odd)
    degs = _class_degrees(cls_of, pos)
    degs[pos == 2] += SLOTS                                     # a full piece in front of each class's third segment
    rows = np.arange(len(degs), dtype=np.int64)
    src, tgt = _rows_graph(rows, degs, 500 + np.arange(40), 33 + odd)
    s, t, w = _shuffled(src, tgt, _weights(src, 35 + odd), 37 + odd)
    c_hi = 5 if odd else 6
    last = [int(rows[(cls_of == c) & (pos == per[c] - 1)][0]) for c in (3 if odd else 0, c_hi)]
    return dict(source=s, target=t, weight=w, requests=_requests(s, t, last),
                limit="empty remainder classes between populated ones: classes %s only" % ("1, 3, 5" if odd else "0, 2, 4, 6"))


# ---- 2. rows that are whole pieces, and the long area ------------------------------------------------------------

WHOLE_DEGREES = (256, 512, 768, 2048, 2304, 2560)
WHOLE_WEIGHTS = 12


def whole_piece_rows():
    """In-degrees of whole pieces only, at the 2 / 3 full-piece boundary of the long area and at 8 / 9 / 10 full
    pieces around the whole-wave rows: no row has a remainder, so there is no remainder piece, no padding slot and no
    +0.0 among the slot weights.  The weights are (1 + k) / 64, k < 12 (not count / total: the dictionary's size is the
    point, 12 exactly)."""
    rows = np.array([4, 1, 5, 0, 3, 2], np.int64)               # the degrees are not ascending in the vertex order
    src, tgt = _rows_graph(rows, WHOLE_DEGREES, 100 + np.arange(300), 41)
    w = (1.0 + (_stream(len(src), 42) % np.uint64(WHOLE_WEIGHTS)).astype(np.float64)) / 64.0
    s, t, w = _shuffled(src, tgt, w, 43)
    return dict(source=s, target=t, weight=w, requests=_requests(s, t, [int(rows[2]), int(rows[3]), int(rows[4])]),
                limit="every row is whole pieces (256 .. 2560 edges): pieces * 256 == edges, no padding, 12 weights")


LONG_DEGREES = (769, 1024, 2049, 2305)


def long_rows_only():
    """Every live row has more than two full pieces (n_short == 0): the long area begins at partial slot 3 T and the
    full pieces in front of row n_short are none."""
    rows = np.array([2, 0, 3, 1], np.int64)
    src, tgt = _rows_graph(rows, LONG_DEGREES, 50 + np.arange(400), 51, dead_share=14)
    s, t, w = _shuffled(src, tgt, _weights(src, 52), 53)
    return dict(source=s, target=t, weight=w, requests=_requests(s, t, [int(rows[0]), int(rows[1])]),
                limit="every live row sits in the long area: n_short == 0")


def closed_graph():
    """A ring of 300 vertices with chords and some repeated pairs: every source is also a target, so no vertex is
    source-only, no edge has a dead slot and the dead-slot sort has nothing to sort."""
    n = 300
    v = np.arange(n, dtype=np.int64)
    r = _stream(n, 61)
    chord = v[r % np.uint64(4) != 0]
    src = np.concatenate([v, chord, v[::7], v[::7]])                                    # ring, chords, repeated pairs
    tgt = np.concatenate([(v + 1) % n, (chord * 7 + 3) % n, (v[::7] + 1) % n, (v[::7] * 7 + 3) % n])
    s, t, w = _shuffled(src, tgt, _weights(src, 62), 63)
    return dict(source=s, target=t, weight=w, requests=[0, n - 1, 150, 0],
                limit="no source-only vertex: the dead-slot list is empty")


# ---- 3. vertex counts -------------------------------------------------------------------------------------------

TINY_KINDS = ("self_loop", "one_edge", "pair", "double_loop", "two_loops")


def tiny(kind):
    """The smallest graphs; the weights are plain literals."""
    s, t, w = dict(self_loop=([5], [5], [1.0]), one_edge=([3], [9], [1.0]), pair=([3, 9], [9, 3], [1.0, 0.5]),
                   double_loop=([5, 5], [5, 5], [0.25, 0.75]), two_loops=([5, 8], [5, 8], [1.0, 0.5]))[kind]
    s, t = np.array(s, np.int64), np.array(t, np.int64)
    lo, hi = int(min(s.min(), t.min())), int(max(s.max(), t.max()))
    return dict(source=s, target=t, weight=np.array(w, np.float64), requests=[lo, hi, lo],
                limit="%d vertices, %d edges (%s)" % (len(np.unique(np.r_[s, t])), len(s), kind))


VERTEX_COUNTS = (2, 3, 4, 5, 255, 256, 257)
VERTEX_ENDS = ("rows", "sources")
VERTEX_END_COUNTS = (5, 257)        # 2^k + 1: the highest index alone has the highest bit


def vertex_count(nv, ends=None):
    """nv vertices 0 .. nv-1.  The highest is a row with in-edges from at least two different sources, the
    second-highest a source-only vertex with out-edges into at least three different rows, the lowest a source-only
    vertex with at least two out-edges: at nv = 2^k and 2^k - 1 the highest bit of ceil_log2(nv) is used by the sort
    of the rows (by target) and by the sort of the dead slots (by source).  What the small counts drop: nv == 4 has
    two rows only, so the second-highest vertex reaches two different rows (one of them twice); nv == 3 has one row, so
    both source-only vertices feed that row alone (three and two edges); nv == 2 has one source-only vertex, the
    lowest, with two out-edges, and the top row's second source is the row itself.

    At nv = 2^k + 1 the highest index alone has the highest bit, and a sort that is one bit short files it under key
    0 - which does no harm while key 0 is absent from that sort (the lowest vertex is no target, the highest no source).
    `ends` (nv >= 5) relabels the same graph so that it does harm: "rows" swaps the two lowest vertices (the lowest and
    the highest are both rows, their in-edges interleaved in the edge list), "sources" swaps the two highest (the
    lowest and the highest are both source-only, their out-edges interleaved)."""
    top, hub = nv - 1, nv - 2
    if nv == 2:
        src, tgt = [0, 0, 1], [1, 1, 1]
    elif nv == 3:
        src, tgt = [1, 1, 1, 0, 0, 2], [2, 2, 2, 2, 2, 2]
    elif nv == 4:
        src, tgt = [2, 2, 2, 0, 0, 1, 3], [1, 3, 1, 1, 3, 3, 1]
    else:
        rows = np.concatenate([np.arange(1, hub), [top]]).astype(np.int64)
        r = _stream(len(rows), 70 + nv)
        feed = np.where(r % np.uint64(3) == 0, hub, rows[((r >> np.uint64(8)) % np.uint64(len(rows))).astype(np.int64)])
        src = np.concatenate([[hub, hub, hub, 0, 0, 1], feed, rows[::3]])              # every row has an in-edge
        tgt = np.concatenate([[1, 2, top, 1, top, top], rows, (rows[::3] * 5 + 1) % hub])
        tgt = np.where(tgt == 0, top, tgt)                                            # vertex 0 stays source-only
    src, tgt = np.array(src, np.int64), np.array(tgt, np.int64)
    w = _weights(src, 71)
    if ends is not None:
        assert nv >= 5 and ends in VERTEX_ENDS
        label = np.arange(nv, dtype=np.int64)
        a, b = (0, 1) if ends == "rows" else (hub, top)
        label[[a, b]] = b, a
        src, tgt = label[src], label[tgt]
    s, t, w = _shuffled(src, tgt, w, 72 + nv + {None: 0, "rows": 300, "sources": 601}[ends])
    dead = np.setdiff1d(s, t)
    requests = [0, top, int(dead[-1]), int(dead[0]), int(dead[-1])]
    what = {None: "the highest a row and the second-highest a source of dead slots",
            "rows": "the lowest and the highest both rows", "sources": "the lowest and the highest both sources of dead slots"}
    return dict(source=s, target=t, weight=w, requests=requests, limit="%d vertices, %s" % (nv, what[ends]))


# ---- 4. the grid-stride id range --------------------------------------------------------------------------------

STRIDE_TRIP = 1024 * 256            # edges one trip of the id-range kernel covers
STRIDE_ROWS, STRIDE_DEAD = 3000, 2000


def stride(ne):
    """ne edges over dense ids 0 .. M.  The LAST edge is the only occurrence of the smallest id (0, its source) and of
    the largest id (M, its target): at ne == 262,145 it is the one edge of the id-range kernel's second trip, at
    262,144 the last edge of the first.  Rows of every class; one row takes what is left of the edge count."""
    n = ne - 1
    r = _stream(STRIDE_ROWS, 81)
    degs = 1 + (r % np.uint64(160)).astype(np.int64)
    degs[:6] = (769, 2304, 2049, 256, 767, 0)
    degs[5] = n - int(degs.sum())
    assert degs[5] > 9 * SLOTS
    rows = 1 + np.argsort(_stream(STRIDE_ROWS, 82), kind="stable").astype(np.int64)    # ids 1 .. STRIDE_ROWS
    dead = STRIDE_ROWS + 1 + np.arange(STRIDE_DEAD, dtype=np.int64)
    m = STRIDE_ROWS + STRIDE_DEAD + 1                                                  # the largest id
    src, tgt = _rows_graph(rows, degs, dead, 83)
    src, tgt = np.concatenate([src, [0]]), np.concatenate([tgt, [m]])
    s, t, w = _shuffled(src, tgt, _weights(src, 84), 85, keep_last=True)
    return dict(source=s, target=t, weight=w, requests=[0, m, int(rows[5]), int(dead[7]), int(rows[0]), int(dead[7])],
                limit="%d edges: the last one alone carries the smallest and the largest id" % ne)


# ---- 5. the ends of the id range --------------------------------------------------------------------------------

ID_END_KINDS = ("low", "high", "both", "table_last", "sort_first")
TABLE_SPAN = 8 * 3 + (1 << 20)      # three edges: the table serves spans below 8 E + 2^20


def id_ends(kind):
    """class_spill's edges with monotonically remapped ids (the vertex order, hence the layout, is class_spill's):
    `low` dense from INT64_MIN, `high` dense up to INT64_MAX, `both` with the lowest vertex at INT64_MIN, the highest at
    INT64_MAX and the rest dense around 0 (span 2^64 - 1: span + 1 wraps to 0).  `table_last` / `sort_first`: three
    edges whose span is 8 * 3 + 2^20 - 1 (the last the table serves) and 8 * 3 + 2^20 (the first the sort takes)."""
    if kind in ("table_last", "sort_first"):
        span = TABLE_SPAN - 1 if kind == "table_last" else TABLE_SPAN
        lo = -(1 << 19)
        src = np.array([lo, lo + 7, lo + span], np.int64)
        tgt = np.array([lo + 7, lo + span, lo + 7], np.int64)
        return dict(source=src, target=tgt, weight=_weights(src, 91), requests=[lo, lo + span, lo + 7, lo],
                    limit="three edges, id span %d = 8 E + 2^20%s" % (span, " - 1" if kind == "table_last" else ""))
    c = class_spill()
    lo, hi = int(min(c["source"].min(), c["target"].min())), int(max(c["source"].max(), c["target"].max()))

    def remap(ids):
        ids = np.asarray(ids, np.int64)
        if kind == "low":
            return I64_MIN + (ids - lo)
        if kind == "high":
            return I64_MAX - (hi - ids)
        out = ids - 500
        out = np.where(ids == lo, I64_MIN, out)
        return np.where(ids == hi, I64_MAX, out)

    return dict(source=remap(c["source"]), target=remap(c["target"]), weight=c["weight"],
                requests=[int(x) for x in remap(c["requests"])],
                limit=dict(low="dense ids from INT64_MIN", high="dense ids up to INT64_MAX",
                           both="ids from INT64_MIN to INT64_MAX: span 2^64 - 1")[kind])


# ---- 6. the two format limits (the graphs of tests/test_gpu_sg_limits.py) -----------------------------------------

def uint16_limit(t_plus_2):
    """T = t_plus_2 - 2 live rows of two edges each (one from a person, one from a live vertex) and 1,500 persons that
    are sources only: column values run to T (real edges use T - 1 and T), a batch's first private row is T + 1.
    Weights are 1 / out-degree."""
    T, n_persons = t_plus_2 - 2, 1_500
    live = np.arange(T, dtype=np.int64)
    persons = 100_000 + np.arange(n_persons, dtype=np.int64)           # sources only: their edges read column T
    src = np.concatenate([persons[live % n_persons], live, persons[:40]])
    dst = np.concatenate([live, (live * 7 + 1) % T, np.arange(40, dtype=np.int64)])
    uniq, inv = np.unique(src, return_inverse=True)
    w = 1.0 / np.bincount(inv)[inv]
    # persons (a private row each: column T + 1 onwards in a batch), the first and the last live vertex
    targets = np.array([100_000, 5, T - 1, 100_001, 0, 100_039, 100_002, 100_003, T - 1, 100_004, 7, 100_005, 100_000,
                        100_006, 100_007, 100_008, 100_009, 100_010, 100_011], np.int64)
    return dict(source=src, target=dst, weight=w, requests=targets, persons=persons,
                limit="T + 2 = %d live rows and slots: uint16 columns hold T + 2 <= 65536" % t_plus_2)


def dictionary_limit(distinct):
    """24,000 edges with distinct - 1 different weights; the padding's +0.0 is the dictionary's last entry.  The weights
    are exact multiples of 2^-19 (sums stay below 1) and the graph is drawn from numpy's generator, as it was."""
    rng = np.random.default_rng(23)
    ne, m = 24_000, distinct - 1                                        # m edge weights + the padding's +0.0
    values = (1.0 + np.arange(m)) / 2.0 ** 19                           # distinct, exact, sums stay below 1
    w = values[np.r_[np.arange(m), rng.integers(0, m, ne - m)]]
    src = rng.integers(1000, 1300, ne).astype(np.int64)
    dst = rng.integers(0, 40, ne).astype(np.int64)
    targets = np.r_[rng.choice(np.arange(1000, 1300), 20, replace=False), np.arange(0, 40, 4), [1000, 0]].astype(np.int64)
    return dict(source=src, target=dst, weight=w, requests=targets, edge_weights=m,
                limit="%d distinct slot weights, +0.0 included: the dictionary holds 8192" % distinct)
