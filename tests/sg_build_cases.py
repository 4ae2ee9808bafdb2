"""Edge lists for the comparison of the two builders of the stochastic graph's layout (locrec_sg_create on the host,
locrec_sg_create_from_device by kernels): small graphs that hit every class of the layout.

layout_graph(): one graph whose live rows have exactly the in-degrees DEGREES - every remainder class ceil_log2((rem +
3) / 4) = 0 .. 6 at both of its edges, rem == 0, the 2 / 3 full-piece boundary of the long area (767, 768, 769), and 8
and 9 full pieces around kLongRow (2048 + 1, 2304 + 3) - plus 70 rows of degree 1 .. 4, so the 4-slot segments of
class 0 (77 rows) spill into a second piece.  The degrees are exact, so the list has sum(DEGREES) + 175 = 9,648 edges.
Sources are a mix of live vertices (long rows among them) and source-only vertices; two source-only vertices (HUB_A,
HUB_B) have many out-edges spread over many rows; some (source, target) pairs repeat with different weights; a source's
weights are count / total x beta with an odd total, so a row's sum depends on the order of its terms; the list is
shuffled.  Everything is drawn from synth.splitmix64."""
import numpy as np

DEGREES = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 2048 + 1, 2304 + 3)
N_SMALL = 70
N_LIVE = len(DEGREES) + N_SMALL
DEAD0, N_DEAD = 1000, 600           # source-only vertices DEAD0 .. DEAD0 + N_DEAD - 1
HUB_A, HUB_B = DEAD0, DEAD0 + 1     # source-only vertices with many out-edges
SEED = 0x5EED5B01


def _stream(n, salt):
    from locations_recommender_amd import synth
    return synth.splitmix64(np.arange(n, dtype=np.uint64) ^ np.uint64(SEED + salt))


def layout_graph():
    """-> dict(source, target, weight: the shuffled edge list with dense ids; live: vertex of every degree in DEGREES
    order followed by the small rows; requests: the vertices the tests ask for)."""
    degs = np.array(DEGREES + tuple(1 + i % 4 for i in range(N_SMALL)), np.int64)
    # which vertex gets which degree: a fixed shuffle, so "ascending vertex inside a class" is not "ascending degree"
    live = np.argsort(_stream(N_LIVE, 1), kind="stable").astype(np.int64)
    tgt = np.repeat(live, degs)
    n = len(tgt)
    r = _stream(n, 2)
    kind = r % np.uint64(16)
    pick = (r >> np.uint64(8))
    src = DEAD0 + 2 + (pick % np.uint64(N_DEAD - 2)).astype(np.int64)                 # a source-only vertex
    src = np.where(kind < 4, (pick % np.uint64(N_LIVE)).astype(np.int64), src)       # a live vertex (any row class)
    long_ids = live[[DEGREES.index(d) for d in (769, 2049, 2307)]]
    src = np.where(kind == 4, long_ids[(pick % np.uint64(3)).astype(np.int64)], src)  # a long row as source
    src = np.where(kind == 5, np.where(pick % np.uint64(5) < 3, HUB_A, HUB_B), src)   # the two hubs
    # repeated (source, target) pairs: every 37th edge copies the source of the edge before it in its row
    rep = (np.arange(n) % 37 == 36) & (np.arange(n) > 0) & (tgt == np.roll(tgt, 1))
    src = np.where(rep, np.roll(src, 1), src)
    cnt = 1 + (_stream(n, 3) % np.uint64(3)).astype(np.int64)
    # odd total per source: bump the source's first edge when the total is even
    order = np.argsort(src, kind="stable")
    first = order[np.concatenate(([True], src[order][1:] != src[order][:-1]))]
    tot = np.bincount(src, weights=cnt, minlength=DEAD0 + N_DEAD).astype(np.int64)
    cnt[first] += (tot[src[first]] % 2 == 0)
    tot = np.bincount(src, weights=cnt, minlength=DEAD0 + N_DEAD).astype(np.int64)
    assert np.all(tot[np.unique(src)] % 2 == 1)
    beta = np.where(src % 3 == 0, 0.5, 1.0)
    w = cnt / tot[src].astype(np.float64) * beta
    perm = np.argsort(_stream(n, 4), kind="stable")                                    # neither by source nor by target
    src, tgt, w = src[perm], tgt[perm].astype(np.int64), w[perm]
    assert np.array_equal(np.bincount(tgt, minlength=N_LIVE)[live], degs)
    other = int(src[(src >= DEAD0 + 2)][0])
    requests = [int(live[DEGREES.index(33)]), int(long_ids[2]), HUB_A, HUB_B, HUB_A, other]
    return dict(source=src.astype(np.int64), target=tgt, weight=w, live=live, requests=requests)


def spread_ids(ids, top):
    """A monotone map onto ids 2^40 apart, negative ones included, with the two ends of the int64 range: vertex 0 ->
    INT64_MIN + 1, vertex `top` (the graph's largest) -> INT64_MAX."""
    ids = np.asarray(ids, np.int64)
    out = (ids - 800) * (1 << 40)
    out = np.where(ids == 0, np.iinfo(np.int64).min + 1, out)
    return np.where(ids == top, np.iinfo(np.int64).max, out)


def one_edge_rows(n=70_000):
    """n live rows of one edge each from 50 source-only vertices: T + 2 > 65,536 selects int32 columns."""
    e = np.arange(n, dtype=np.int64)
    src = n + 10 + (_stream(n, 5) % np.uint64(50)).astype(np.int64)
    out = np.bincount(src - n - 10, minlength=50)
    return src, e, 1.0 / out[src - n - 10]


def many_weights(n=9_000):
    """n edges with n distinct weights (more than the dictionary's 8,192 entries) into 40 rows."""
    r = _stream(n, 6)
    src = 500 + (r % np.uint64(300)).astype(np.int64)
    dst = ((r >> np.uint64(20)) % np.uint64(40)).astype(np.int64)
    w = (1.0 + np.arange(n)) / (4.0 * n)
    return src, dst, w
