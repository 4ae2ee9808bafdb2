"""Inputs that stand ON the limits of SG for visitors (csrc/sg_visitors.h, sg_visitors_plan.h, the VIS branch of
sg_finalize_batch_body in sg_batch.hip; DESIGN.md, "Visitors"), and plain-Python restatements of what the sources decide:
the stage of a tile (sg_visitors_stage), the rows of the layout, the rounds and polls of sg_batch_tiles_of, and the
iteration itself with its x (d2_trajectory's, extended).  Shared by the CPU checks of the cases themselves
(test_sg_visitor_limit_cases.py) and the GPU tests (test_gpu_sg_visitor_limits.py).  Seeded; numpy, sg_visitor_cases and
rank_limit_cases only: nothing of the library under test.

The limits are written here as literals on purpose: a test that asks the library where its limit lies cannot catch a
moved limit.  Every visitor that is compared with the oracle at an epsilon > 0 keeps sg_visitor_cases' margin for the
parameter sets it is run at; candidates that miss it are replaced here (new weights or new targets from the same seed)."""
import functools

import numpy as np

import rank_limit_cases as rl
import sg_visitor_cases as vc
from sg_visitor_cases import ALPHA

TILE = 16            # visitors of a tile, whatever T and the column width
BLOCK = 256          # threads of sg_vis_set_up's one block: the stride of its three loops
PARAMS = ((0.01, 20), (0.01, 0))
SWEEPS = (0.0, 30)   # a fixed number of sweeps (no fixed point is reached that early on these graphs)
ROUND_PARAMS = ((0.01, 1), (0.01, 4), (0.01, 5), (0.01, 6))   # the host polls only above 4
SENSITIVE = 1e-3     # what a dropped or stale staged edge moves some returned probability by, relative, at least
SIGN_MARGIN = 1e-9


# ---- restatements ---------------------------------------------------------------------------------------------------------

def live_rows(graph):
    """vertex id -> live row (sg.hip): the vertices with an inbound edge, rows of at most two full pieces first, ascending
    id inside either class"""
    ids, deg = np.unique(graph[1], return_counts=True)
    long_area = np.array([vc.row_class(int(d)) != "short" for d in deg])
    order = np.r_[ids[~long_area], ids[long_area]]
    return {int(v): r for r, v in enumerate(order)}


def stage(tile, rows):
    """sg_visitors_stage for one tile of visitors -> (row, column, slot, weight) of its staged edges: rows ascending, then
    columns; a row's slot is its rank among the tile's distinct rows"""
    e = sorted((rows[int(t)], c, float(w)) for c, v in enumerate(tile) for t, w in zip(v[1], v[2]))
    distinct = sorted({r for r, _, _ in e})
    slot = {r: i for i, r in enumerate(distinct)}
    return [(r, c, slot[r], w) for r, c, w in e]


def tiles_of(visitors):
    return [visitors[i:i + TILE] for i in range(0, len(visitors), TILE)]


def call_counts(graph, visitors):
    """-> per tile (staged edges, weight lines); visitors_stats' staged_edges is the sum of the first, table_slots the
    largest of the second"""
    rows = live_rows(graph)
    out = []
    for tile in tiles_of(visitors):
        st = stage(tile, rows)
        out.append((len(st), len({s[2] for s in st})))
    return out


def run_model(edges, v, eps, max_it):
    """makeRecommendations (StochasticRecommender.scala:92-128) in numpy: d2_trajectory's iteration with step()'s two exits
    -> (vertex ids, x, iterations, converged, x before the last sweep that ran)"""
    src, dst, w = edges
    vid, inv = np.unique(np.concatenate([src, dst]), return_inverse=True)
    cs, ct = inv[:len(src)], inv[len(src):]
    u = (vid == v).astype(np.float64)
    x = before = np.full(len(vid), 1.0 / len(vid))
    e2 = eps * eps
    for k in range(max_it):
        xn = ALPHA * u + (1 - ALPHA) * np.bincount(ct, weights=x[cs] * w, minlength=len(vid))
        d2 = float(np.sum((xn - x) ** 2))
        before, x = x, xn
        if d2 <= e2:
            return vid, x, k, True, before
    return vid, x, max_it, False, before


def model_rows(graph, visitor, eps, max_it):
    """what the model returns for a visitor: {id: probability} of the rows with id != V and probability > 0 (:84-88)"""
    vid, x = run_model(vc.plus(graph, visitor), visitor[0], eps, max_it)[:2]
    keep = (vid != visitor[0]) & (x > 0)
    return dict(zip(vid[keep].tolist(), x[keep].tolist()))


def moved(a, b):
    """the largest relative change of a returned probability between two results of the model (a row that comes or goes
    counts as 1)"""
    worst = 0.0
    for k in set(a) | set(b):
        if k not in a or k not in b:
            return 1.0
        worst = max(worst, abs(a[k] - b[k]) / max(a[k], b[k]))
    return worst


def without_edges(visitor, targets):
    keep = ~np.isin(visitor[1], list(targets))
    return (visitor[0], visitor[1][keep], visitor[2][keep])


def with_edges(visitor, targets, weights):
    return (visitor[0], np.r_[visitor[1], np.asarray(targets, np.int64)], np.r_[visitor[2], np.asarray(weights, np.float64)])


def converged_at(graph, visitor, eps, max_it):
    """the sweep whose sum is the first <= eps^2 (the column is left out from the launch behind it), or None"""
    d2 = vc.d2_trajectory(vc.plus(graph, visitor), visitor[0], max_it, stop=eps * eps)
    return len(d2) - 1 if len(d2) and d2[-1] <= eps * eps else None


def rounds_and_polls(graph, visitors, eps, max_it):
    """sg_batch_tiles_of's schedule restated -> (finalize launches, polls) of a call: a tile's rounds are launched up to
    the next check (4, 6, 8, 12, 16, ...), the host reads "all columns done" there when epsilon > 0 and max_iterations > 4
    and the check lies below max_iterations, and stops when the word is set.  The word is set by the launch in which no
    column is active any more: the one behind the last column's converging sweep."""
    poll = eps > 0 and max_it > 4
    launches = polls = 0
    for tile in tiles_of(visitors):
        at = [converged_at(graph, v, eps, max_it) for v in tile]
        word_set_by = None if any(a is None for a in at) else max(at) + 1   # (launch index; it has to be launched)
        i, check = 0, 4
        while i < max_it:
            stop = min(max_it, check) if poll else max_it
            launches += stop - i
            i = stop
            if poll and stop == check and stop < max_it:
                polls += 1
                if word_set_by is not None and word_set_by < stop:
                    break
                assert check < 8, "the schedule beyond 8 is not restated here"
                check += 2
    return launches, polls


# ---- A: the graph of the set-up cases ---------------------------------------------------------------------------------------

T_A, N_SOURCES_A, SOURCE0, CYCLE, LIGHT_ROW, LIGHT_SOURCE = 600, 2_000, 10_000, (600, 601), 602, 20_000


@functools.lru_cache(maxsize=None)
def graph_a():
    """600 live vertices 0 .. 599 and 2,000 source-only ones, each pointing at three of them (every row has in-degree 10);
    86 live vertices point at two live ones; weights 1 / out-degree.  Three more live vertices: the two-cycle 600 <-> 601,
    where mass swings (a visitor that enters it is stopped by the maximum: case F), and 602, whose one inbound edge is
    light - a tenth of source 20,000 - and which points on at row 7 (case E's negative weight)."""
    j = np.arange(N_SOURCES_A)
    src = [SOURCE0 + j] * 3
    dst = [(j + k) % T_A for k in (0, 197, 401)]
    i = np.arange(0, T_A, 7)
    src += [i, i]
    dst += [(i * 11 + 5) % T_A, (i * 13 + 2) % T_A]
    assert not (dst[3] == dst[4]).any()
    src += [np.array([CYCLE[0], CYCLE[1], LIGHT_ROW]), np.full(10, LIGHT_SOURCE)]
    dst += [np.array([CYCLE[1], CYCLE[0], 7]), np.r_[LIGHT_ROW, np.arange(100, 109)]]
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    _, inv, cnt = np.unique(src, return_inverse=True, return_counts=True)
    return src, dst, 1.0 / cnt[inv]


def make_visitor(graph, rng, vid, targets, params, fixed=None):
    """random weights that add up to 1 until the margin holds (fixed: the weights of the first attempt)"""
    targets = np.asarray(targets, np.int64)
    for attempt in range(20):
        w = rng.random(len(targets)) + 0.1
        w = w / w.sum()
        if attempt == 0 and fixed is not None:
            w = np.asarray(fixed, np.float64)
        v = (vid, targets, w)
        if vc.has_margin(graph, v, params):
            return v
    raise AssertionError("no weights keep the margin")


@functools.lru_cache(maxsize=None)
def stride_tile(edges):
    """one tile of 16 visitors with 255, 256 or 257 staged edges: 16 each, visitor 9 with 15, 16 or 17; random rows of
    0 .. 599, and visitor 9 holds row 599, so that the last staged edge is its own"""
    rng = np.random.default_rng(edges)
    g = graph_a()
    out = []
    for i in range(TILE):
        n = 16 + (edges - 256 if i == 9 else 0)
        t = rng.choice(T_A - 1, n - (i == 9), replace=False)
        out.append(make_visitor(g, rng, 70_000 + i, np.r_[t, [T_A - 1]] if i == 9 else t, PARAMS))
    return out


@functools.lru_cache(maxsize=None)
def same_rows_tile(moved_edge):
    """16 visitors at the same 16 rows 40, 70, .. 490: 256 edges in 16 lines, lines * 16 == 256.  moved_edge: visitor 5's
    edge to row 490 goes to row 555 instead, a 17th line with one column."""
    rng = np.random.default_rng(16)
    g = graph_a()
    rows = 40 + 30 * np.arange(16)
    out = []
    for i in range(TILE):
        t = rows.copy()
        if moved_edge and i == 5:
            t[-1] = 555
        out.append(make_visitor(g, rng, 71_000 + i, t, PARAMS))
    return out


@functools.lru_cache(maxsize=None)
def dense_tile_17():
    """16 visitors at all of same_rows_tile's 17 rows: run in front of it, every word of its 17 lines is non-zero"""
    rng = np.random.default_rng(17)
    rows = np.r_[40 + 30 * np.arange(16), 555]
    return [make_visitor(graph_a(), rng, 72_000 + i, rows, PARAMS) for i in range(TILE)]


@functools.lru_cache(maxsize=None)
def every_row_visitor():
    """one visitor with an edge to every live row of graph_a: lines == T == staged edges"""
    rng = np.random.default_rng(18)
    g = graph_a()
    live = np.unique(g[1])
    return [make_visitor(g, rng, 73_000, rng.permutation(live), PARAMS)]


@functools.lru_cache(maxsize=None)
def wide_tile():
    """a full tile with 100 edges a visitor: 1,600 staged edges, seven strides of the scatter"""
    rng = np.random.default_rng(19)
    g = graph_a()
    return [make_visitor(g, rng, 74_000 + i, rng.choice(T_A, 100, replace=False), PARAMS) for i in range(TILE)]


@functools.lru_cache(maxsize=None)
def reset_call(wide):
    """two tiles: the first with 272 staged edges, 17 a visitor, (or wide_tile's 1,600), its visitors 0, 1, 2 at rows 597, 598, 599 among
    others - staged behind position 256, in lines beyond the second tile's; the second three visitors with one edge
    each.  A row of the first tile that is not put back adds its stale line to the second tile's columns 0, 1, 2."""
    rng = np.random.default_rng(20 + wide)
    g = graph_a()
    first = []
    for i in range(TILE):
        t = rng.choice(590, 99 if wide else 17 - 3 * (i < 3), replace=False)
        if i < 3 or wide:
            t = np.r_[t, [597, 598, 599]] if i < 3 else np.r_[t, rng.choice(np.arange(590, 597), 1)]
        first.append(make_visitor(g, rng, 75_000 + 100 * wide + i, t, PARAMS))
    second = [make_visitor(g, rng, 75_050 + 100 * wide + i, [10 + i], PARAMS, fixed=[1.0]) for i in range(3)]
    return first + second


# ---- B: tables between tiles --------------------------------------------------------------------------------------------------

ROWS_A = 14 * np.arange(40)          # 0 .. 546: vertices with out-edges, the walk goes on behind them
ROWS_B = 7 + 14 * np.arange(40)      # 7 .. 553
ROWS_NEITHER = (13, 27, 41)


@functools.lru_cache(maxsize=None)
def tables_case():
    """Three tiles of one call on graph_a.  Tile 0: 16 visitors at all 40 rows of A.  Tile 1: 16 visitors at B only, every
    row of B named by one visitor (2 or 3 rows each): as many lines as tile 0's, one column each.  Tile 2: three visitors
    with three rows of A (new weights), one of B and one of neither."""
    rng = np.random.default_rng(21)
    g = graph_a()
    t0 = [make_visitor(g, rng, 76_000 + i, rng.permutation(ROWS_A), PARAMS) for i in range(TILE)]
    t1 = [make_visitor(g, rng, 76_100 + i, ROWS_B[i::TILE], PARAMS) for i in range(TILE)]
    t2 = [make_visitor(g, rng, 76_200 + i, np.r_[ROWS_A[[5 * i + 20, 5 * i + 1, 39 - i]], ROWS_B[30 + i], ROWS_NEITHER[i]], PARAMS)
          for i in range(3)]
    return t0 + t1 + t2


def places_a():
    """a place table over graph_a: every live id, regions id % 3; some ids listed twice, one id that is no vertex"""
    ids = np.r_[np.arange(T_A + 3), [45, 46, 47], [777_777]].astype(np.int64)
    return ids, np.r_[np.arange(T_A + 3) % 3, [2, 0, 1], [0]].astype(np.int64)


# ---- C: sixteen visitors whatever T --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def narrow_case(T):
    """rank_limit_cases.sg_narrow_tile_graph(T) and 17 visitors with 1 .. 6 distinct live targets among rows 0 .. 199,
    T - 200 .. T - 1 and the rows the graph's first 40 reach; visitor 0 points at row 0, visitors 15 and 16 at row T - 1.
    Visitors 0, 15 and 16 keep the margin."""
    g = rl.sg_narrow_tile_graph(T)
    graph = (g["src"], g["dst"], g["w"])
    rng = np.random.default_rng(T)
    pool = np.intersect1d(g["place_ids"], np.arange(T))
    out = []
    for i in range(17):
        must = {0: [0], 15: [T - 1], 16: [T - 1, T - 200]}.get(i, [])
        for _ in range(20):
            more = rng.choice(np.setdiff1d(pool, must), 1 + i % 6 - len(must), replace=False)
            t = np.r_[must, more].astype(np.int64)
            w = rng.random(len(t)) + 0.1
            v = (900_000 + i, rng.permutation(t), w / w.sum())
            if i not in (0, 15, 16) or vc.has_margin(graph, v, PARAMS):
                break
        else:
            raise AssertionError("no candidate keeps the margin")
        out.append(v)
    return g, graph, out


# ---- D: degenerate graphs -----------------------------------------------------------------------------------------------------

D_PARAMS = PARAMS + (SWEEPS,)


def _f(a):
    return np.asarray(a, np.float64)


def _i(a):
    return np.asarray(a, np.int64)


@functools.lru_cache(maxsize=None)
def one_edge_case():
    """G = 1 -> 2: T = 1, N = 2; the visitor (2, 1.0)"""
    graph = (_i([1]), _i([2]), _f([1.0]))
    return graph, [(9, _i([2]), _f([1.0]))]


def dead_count_epsilon():
    """an epsilon for one_edge_case whose square lies half-way between sweep 0's sum and that sum without the x0^2 of one
    source-only vertex: a finalize that counts a source-only vertex too few stops at sweep 0, the reference goes on"""
    graph, (v,) = one_edge_case()
    d2 = vc.d2_trajectory(vc.plus(graph, v), v[0], 1)
    return float(np.sqrt(d2[0] - (1.0 / 3) ** 2 / 2))


@functools.lru_cache(maxsize=None)
def cycle_case():
    """a 5-cycle: N == T, no source-only vertex; the visitor points at two of its vertices"""
    graph = (_i([0, 1, 2, 3, 4]), _i([1, 2, 3, 4, 0]), _f([1.0] * 5))
    return graph, [(9, _i([3, 1]), _f([0.75, 0.25]))]


@functools.lru_cache(maxsize=None)
def wave_only_case():
    """2,400 sources at one live vertex: the graph's only row is a wave row (n_short == 0).  17 visitors with different
    weights to it: a full weight line on a wave row, and a second tile."""
    graph = (1_000 + np.arange(2_400, dtype=np.int64), np.zeros(2_400, np.int64), np.full(2_400, 1.0))
    return graph, [(50_000 + i, _i([0]), _f([(i + 1) / 17.0])) for i in range(17)]


@functools.lru_cache(maxsize=None)
def every_row_tile():
    """a full tile in which every visitor points at every live row of sg_visitor_cases.degree_case's graph: lines == T ==
    40, 640 edges, every (slot, column) pair written over short, medium and wave rows at once"""
    graph, _ = vc.degree_case()
    rng = np.random.default_rng(40)
    live = np.unique(graph[1])
    return graph, [make_visitor(graph, rng, 60_000 + i, rng.permutation(live), PARAMS) for i in range(TILE)]


# ---- E: weights ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def zero_weight_case():
    """six visitors of graph_a; (plain visitors, the same with visitor 1 carrying an extra edge of weight +0.0 to row 300
    and visitor 4 one of -0.0 to row 301 - rows none of the six names)"""
    rng = np.random.default_rng(50)
    g = graph_a()
    plain = [make_visitor(g, rng, 77_000 + i, rng.choice(290, 4 + i, replace=False), PARAMS) for i in range(6)]
    extra = list(plain)
    extra[1] = with_edges(plain[1], [300], [0.0])
    extra[4] = with_edges(plain[4], [301], [-0.0])
    return plain, extra


NEGATIVE_PARAMS = ((0.01, 20),)


@functools.lru_cache(maxsize=None)
def negative_weight_case():
    """a visitor of graph_a with the weight -0.25 to row 602, whose one inbound edge of G weighs 0.1: x(602) is negative
    from the first sweep, and so is what 602 passes on to row 7"""
    rng = np.random.default_rng(51)
    g = graph_a()
    for _ in range(20):
        t = np.r_[rng.choice(290, 5, replace=False), [LIGHT_ROW]]
        w = rng.random(5) + 0.1
        v = (78_000, t.astype(np.int64), np.r_[w / w.sum(), [-0.25]])
        if vc.has_margin(g, v, NEGATIVE_PARAMS) and sign_margin(g, v, *NEGATIVE_PARAMS[0]):
            return v
    raise AssertionError("no candidate keeps both margins")


def sign_margin(graph, visitor, eps, max_it):
    """every final x is at least SIGN_MARGIN of the largest in magnitude - its sign is then the same under any order of
    summation - or the sum of no term but exact zeros (a vertex whose sources all hold 0.0: 0.0 in any order)"""
    edges = vc.plus(graph, visitor)
    vid, x, _, _, before = run_model(edges, visitor[0], eps, max_it)
    src, dst, w = edges
    cs, ct = np.searchsorted(vid, src), np.searchsorted(vid, dst)
    terms = np.bincount(ct, weights=np.abs(before[cs] * w), minlength=len(vid))
    small = np.abs(x) < SIGN_MARGIN * np.abs(x).max()
    exact_zero = (terms == 0) & (vid != visitor[0])
    return bool((~small | exact_zero).all())


# ---- F: rounds and polls with two tiles ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rounds_case():
    """17 visitors of graph_a: visitor 3 enters the two-cycle and is not done at any poll, the others are done before the
    first; the 17th makes a second tile"""
    rng = np.random.default_rng(60)
    g = graph_a()
    out = [make_visitor(g, rng, 79_000 + i, rng.choice(T_A, 3 + i % 5, replace=False), ROUND_PARAMS) for i in range(17)]
    out[3] = make_visitor(g, rng, 79_003, [CYCLE[0]], ROUND_PARAMS, fixed=[1.0])
    return out


# ---- G: the protocol across a tile seam ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def seam_case(n):
    """n visitors (17 or 18) of graph_a: rounds_case's without the slow one, and new ones"""
    rng = np.random.default_rng(70)
    g = graph_a()
    base = [v for i, v in enumerate(rounds_case()) if i != 3]
    more = [make_visitor(g, rng, 79_100 + i, rng.choice(T_A, 4, replace=False), PARAMS) for i in range(n - len(base))]
    return base + more


def offenders(n):
    """the last of seam_case(n) made an offender -> (what, visitors, status name, text of the refusal)"""
    good = seam_case(n)
    last = good[-1]
    t, w = last[1], last[2]
    yield "unknown id", good[:-1] + [(last[0], np.r_[t[:-1], [555_555]], w)], "E_NOT_FOUND", "No such vertex in the graph: 555555"
    yield "repeated target", good[:-1] + [(last[0], np.r_[t, t[:1]], np.r_[w, w[:1]])], "E_INVALID_ARG", "twice"
    yield "source-only target", good[:-1] + [(last[0], np.r_[t[:-1], [SOURCE0 + 5]], w)], "E_INVALID_ARG", "no inbound edge"
    yield "NaN weight", good[:-1] + [(last[0], t, np.r_[w[:-1], [np.nan]])], "E_INVALID_ARG", "not finite"
