"""The cases of tests/sg_visitor_limit_cases.py stand where the GPU tests (test_gpu_sg_visitor_limits.py) need them, proven
on the CPU: the staged edges and weight lines of every tile by the stage restated; the disjoint row sets; every compared
visitor's margin to a tie of the iteration counter, confirmed by the oracle; and conditions ON THE INPUTS that keep a
faulty set-up from hiding inside the probabilities' tolerance - in the numpy model a staged edge that is dropped, or a
stale weight that is added, moves some returned probability of the affected visitor by SENSITIVE = 1e-3 relative at least
(a thousand times RTOL), and the signs of the negative-weight case have a margin."""
import numpy as np
import pytest

import sg_visitor_cases as vc
import sg_visitor_limit_cases as lim
from test_sg_visitor_cases import check_margin, check_visitors

RUNS = ((0.01, 20), lim.SWEEPS)   # the parameter sets at which sweeps run: a result depends on the visitor's edges there


def sensitive(graph, visitor, changed):
    return all(lim.moved(lim.model_rows(graph, visitor, *p), lim.model_rows(graph, changed, *p)) >= lim.SENSITIVE for p in RUNS)


def dropped_from(graph, tile, first):
    """the tile's visitors without the staged edges of positions first .. -> {column: the visitor without them}"""
    rows = lim.live_rows(graph)
    back = {r: v for v, r in rows.items()}
    lost = {}
    for r, c, _, _ in lim.stage(tile, rows)[first:]:
        lost.setdefault(c, []).append(back[r])
    return {c: lim.without_edges(tile[c], t) for c, t in lost.items()}


def test_restatements():
    assert (lim.TILE, lim.BLOCK) == (16, 256)
    # sg_visitors_plan_check.cpp's literal: three visitors, rows shared between them
    tile = [(1, [9, 2], [0.5, 0.25]), (2, [9], [1.0]), (3, [4, 2, 30], [0.0, -3.0, 7.0])]
    st = lim.stage(tile, {k: k for k in range(40)})
    assert [s[0] for s in st] == [2, 2, 4, 9, 9, 30] and [s[1] for s in st] == [0, 2, 2, 0, 1, 2]
    assert [s[2] for s in st] == [0, 0, 1, 2, 2, 3] and [s[3] for s in st] == [0.25, -3.0, 0.0, 0.5, 1.0, 7.0]
    # the rows of the degree-class graph: the short rows first, then the medium and the wave row, ascending id in either
    rows = lim.live_rows(vc.degree_case()[0])
    assert rows[0] == 0 and rows[3] == 1 and rows[39] == 37 and rows[1] == 38 and rows[2] == 39
    # the model is d2_trajectory's iteration: the same counter and flag as verdict() of its sums
    g, v = lim.graph_a(), lim.stride_tile(256)[0]
    d2 = vc.d2_trajectory(vc.plus(g, v), v[0], 20)
    assert lim.run_model(vc.plus(g, v), v[0], 0.01, 20)[2:4] == vc.verdict(d2, 0.01, 20)[:2]


def test_graph_a(oracle):
    src, dst, w = g = lim.graph_a()
    live, sources = np.unique(dst), np.setdiff1d(src, dst)
    assert live.tolist() == list(range(603)) and len(sources) == 2_001
    assert len(np.unique(np.stack([src, dst]), axis=1)[0]) == len(src)   # no parallel edges
    out = dict(zip(*np.unique(src, return_counts=True)))
    assert all(x == 1.0 / out[s] for s, x in zip(src.tolist(), w.tolist()))
    assert all(out[s] == 3 for s in sources[:2_000]) and out[lim.LIGHT_SOURCE] == 10
    assert all(vc.row_class(int(d)) == "short" for d in np.bincount(dst))   # row == id
    assert lim.live_rows(g) == {i: i for i in range(603)}
    assert 50 <= np.isin(src, live).sum() - 3 <= 200   # a few live -> live edges
    assert np.bincount(dst)[lim.LIGHT_ROW] == 1 and w[dst == lim.LIGHT_ROW].tolist() == [0.1]


@pytest.mark.parametrize("edges", [255, 256, 257])
def test_stride_tiles(oracle, edges):
    g, tile = lim.graph_a(), lim.stride_tile(edges)
    check_visitors(g, tile)
    assert len(tile) == 16 and [len(v[1]) for v in tile] == [16] * 9 + [edges - 240] + [16] * 6
    (n, lines), = lim.call_counts(g, tile)
    assert n == edges and lines < edges
    st = lim.stage(tile, lim.live_rows(g))
    assert st[-1][:2] == (599, 9)   # the last staged edge is visitor 9's
    assert sensitive(g, tile[9], lim.without_edges(tile[9], [599]))
    if edges > lim.BLOCK:
        lost = dropped_from(g, tile, lim.BLOCK)
        assert list(lost) == [9] and len(lost[9][1]) == 16 and sensitive(g, tile[9], lost[9])
    check_margin(oracle, g, tile[8:11], lim.PARAMS)


def test_same_rows_tiles(oracle):
    g = lim.graph_a()
    a, b, dense = lim.same_rows_tile(False), lim.same_rows_tile(True), lim.dense_tile_17()
    assert lim.call_counts(g, a) == [(256, 16)] and lim.call_counts(g, b) == [(256, 17)] and 16 * lim.TILE == lim.BLOCK
    assert lim.call_counts(g, dense + b) == [(272, 17), (256, 17)]
    for tile in (a, b, dense):
        check_visitors(g, tile)
    assert [len(set(v[1]) & {555}) for v in b] == [0] * 5 + [1] + [0] * 10
    # behind the dense tile an uncleared line 16 (row 555 in both tiles) adds the dense visitor's weight to row 555 in the
    # 15 columns that have no edge to it; the scatter overwrites it in column 5
    for c in (0, 15):
        stale = float(dense[c][2][dense[c][1] == 555][0])
        assert stale > 0 and sensitive(g, b[c], lim.with_edges(b[c], [555], [stale]))
    check_margin(oracle, g, a[:2] + b[4:6] + dense[:1], lim.PARAMS)


def test_every_row_visitor_and_wide_tile(oracle):
    g = lim.graph_a()
    one, wide = lim.every_row_visitor(), lim.wide_tile()
    check_visitors(g, one + wide)
    assert lim.call_counts(g, one) == [(603, 603)] and sorted(one[0][1].tolist()) == list(range(603))
    (n, lines), = lim.call_counts(g, wide)
    assert n == 1600 == 16 * 100 and lines > lim.BLOCK and n > 6 * lim.BLOCK
    assert sensitive(g, one[0], lim.without_edges(one[0], range(lim.BLOCK, 603)))   # (row == id: positions 256 ..)
    assert sensitive(g, one[0], lim.without_edges(one[0], [602]))
    lost = dropped_from(g, wide, lim.BLOCK)
    assert sorted(lost) == list(range(16)) and all(sensitive(g, wide[c], v) for c, v in lost.items())
    lost = dropped_from(g, wide, 1599)
    (c, v), = lost.items()
    assert sensitive(g, wide[c], v)
    check_margin(oracle, g, one + wide[::5], lim.PARAMS)


@pytest.mark.parametrize("wide", [False, True])
def test_reset_calls(oracle, wide):
    g, visitors = lim.graph_a(), lim.reset_call(wide)
    check_visitors(g, visitors)
    first, second = visitors[:16], visitors[16:]
    counts = lim.call_counts(g, visitors)
    assert counts[0][0] == (1606 if wide else 272) and counts[1] == (3, 3) and counts[0][0] > lim.BLOCK
    st = lim.stage(first, lim.live_rows(g))
    named = {int(v[1][0]) for v in second}
    for c in range(3):
        # rows 597 .. 599 of the first tile's column c: staged behind the first stride, in lines beyond the second tile's
        # three, not named by the second tile - left in place they add their weights to the second tile's column c
        late = [(i, s) for i, s in enumerate(st) if s[1] == c and s[0] >= 597]
        assert [s[0] for _, s in late] == [597, 598, 599] and all(i >= lim.BLOCK and s[2] >= 3 and s[3] > 0 for i, s in late)
        assert not named & {597, 598, 599}
        assert sensitive(g, second[c], lim.with_edges(second[c], [s[0] for _, s in late], [s[3] for _, s in late]))
    check_margin(oracle, g, first[:3] + second, lim.PARAMS)


def test_tables_case(oracle):
    g, visitors = lim.graph_a(), lim.tables_case()
    check_visitors(g, visitors)
    A, B = set(lim.ROWS_A.tolist()), set(lim.ROWS_B.tolist())
    assert len(A) == len(B) == 40 and not A & B and not (A | B) & set(lim.ROWS_NEITHER) and max(A | B) < 600
    t0, t1, t2 = lim.tiles_of(visitors)
    assert lim.call_counts(g, visitors) == [(640, 40), (40, 40), (15, 15)]
    assert all(set(v[1].tolist()) == A for v in t0) and all((v[2] > 0).all() for v in t0)
    assert sorted(np.concatenate([v[1] for v in t1]).tolist()) == sorted(B) and len(t1) == 16   # each row of B once
    for i, v in enumerate(t2):
        t = set(v[1].tolist())
        assert len(t & A) == 3 and len(t & B) == 1 and t - A - B == {lim.ROWS_NEITHER[i]}
        assert not np.array_equal(v[2][:3], [t0[i][2][t0[i][1] == r][0] for r in v[1][:3]])   # new weights
    # tile 2's 15 lines: tile 0's slots 15 .. 39 are stale there, and rows of A change tile twice
    assert len(set().union(*[set(v[1].tolist()) for v in t2]) & A) == 9
    # a line of tile 1 that is not cleared holds tile 0's weights of the row of A with the same slot, in every column
    rows_a, rows_b = sorted(A), sorted(B)
    for c in (0, 7):
        stale = [(rows_b[k], float(t0[c][2][t0[c][1] == rows_a[k]][0])) for k in range(16, 40) if rows_b[k] not in t1[c][1]]
        assert len(stale) >= 21 and sensitive(g, t1[c], lim.with_edges(t1[c], [r for r, _ in stale], [x for _, x in stale]))
    # a row of A that keeps tile 0's slot in tile 1 (no reset): its line there is another row's, or beyond tile 1's
    check_margin(oracle, g, t0[:2] + t1[:2] + t2, lim.PARAMS)
    ids, regions = lim.places_a()
    assert len(ids) == len(regions) and np.isin(np.arange(603), ids).all()


@pytest.mark.parametrize("T", [65533, 65534, 65535])
def test_narrow_case(oracle, T):
    g, graph, visitors = lim.narrow_case(T)
    assert len(np.unique(graph[1])) == T and len(visitors) == 17 and len(g["targets"]) == 19
    check_visitors(graph, visitors)
    reached = np.intersect1d(g["place_ids"], np.arange(T))
    for v in visitors:
        assert 1 <= len(v[1]) <= 6 and np.isin(v[1], reached).all()
    assert 0 in visitors[0][1] and T - 1 in visitors[15][1] and T - 1 in visitors[16][1]
    assert min(16, 65535 - T) == {65533: 2, 65534: 1, 65535: 0}[T]   # the persons' tile with uint16 columns (int32 at 65535: 16)
    check_margin(oracle, graph, [visitors[0], visitors[15], visitors[16]], lim.PARAMS)


def test_degenerate_graphs(oracle):
    graph, visitors = lim.one_edge_case()
    assert len(np.unique(graph[1])) == 1 and len(np.union1d(graph[0], graph[1])) == 2
    check_visitors(graph, visitors)
    check_margin(oracle, graph, visitors, lim.D_PARAMS)
    # sweep 0's sum holds the x0^2 = 1/9 of the one source-only vertex: an epsilon^2 inside that ninth, with the margin
    eps = lim.dead_count_epsilon()
    d2 = vc.d2_trajectory(vc.plus(graph, visitors[0]), 9, 20)
    assert d2[0] - 1 / 9 < eps * eps < d2[0] and vc.verdict(d2, eps, 20) == (2, True, True)
    assert vc.verdict(np.r_[d2[0] - 1 / 9, d2[1:]], eps, 20)[:2] == (0, True)
    check_margin(oracle, graph, visitors, ((eps, 20),))
    graph, visitors = lim.cycle_case()
    assert len(np.setdiff1d(graph[0], graph[1])) == 0 and len(np.unique(graph[1])) == 5 and len(visitors[0][1]) == 2
    check_visitors(graph, visitors)
    check_margin(oracle, graph, visitors, lim.D_PARAMS)
    graph, visitors = lim.wave_only_case()
    assert np.unique(graph[1]).tolist() == [0] and vc.row_class(len(graph[1])) == "wave" and len(visitors) == 17
    assert len({float(v[2][0]) for v in visitors}) == 17 and lim.call_counts(graph, visitors) == [(16, 1), (1, 1)]
    check_visitors(graph, visitors)
    check_margin(oracle, graph, visitors, lim.D_PARAMS)
    graph, visitors = lim.every_row_tile()
    deg = np.bincount(graph[1])
    assert {vc.row_class(int(d)) for d in deg} == {"short", "medium", "wave"}
    assert lim.call_counts(graph, visitors) == [(640, 40)] and all(sorted(v[1].tolist()) == list(range(40)) for v in visitors)
    check_visitors(graph, visitors)
    check_margin(oracle, graph, visitors[::5], lim.D_PARAMS)


def test_weight_cases(oracle):
    g = lim.graph_a()
    plain, extra = lim.zero_weight_case()
    check_visitors(g, plain + extra)
    named = set(np.concatenate([v[1] for v in plain]).tolist())
    assert not named & {300, 301}
    assert [len(e[1]) - len(p[1]) for p, e in zip(plain, extra)] == [0, 1, 0, 0, 1, 0]
    zeros = [extra[1][2][-1], extra[4][2][-1]]
    assert zeros == [0.0, 0.0] and np.signbit(zeros).tolist() == [False, True] and (extra[1][1][-1], extra[4][1][-1]) == (300, 301)
    check_margin(oracle, g, plain, lim.PARAMS)
    # the negative weight: every sign has a margin, x(602) and x(7) are negative, the oracle returns the model's rows
    v = lim.negative_weight_case()
    check_visitors(g, [v])
    assert v[1][-1] == lim.LIGHT_ROW and v[2][-1] == -0.25 and (v[2][:-1] > 0).all()
    check_margin(oracle, g, [v], lim.NEGATIVE_PARAMS)
    for eps, max_it in lim.NEGATIVE_PARAMS:
        assert lim.sign_margin(g, v, eps, max_it)
        vid, x, it, _, _ = lim.run_model(vc.plus(g, v), v[0], eps, max_it)
        assert it >= 2 and x[vid == lim.LIGHT_ROW][0] < 0 and x[vid == 7][0] < 0 and (x < 0).sum() >= 2
        ids = oracle.sg_recommend(*vc.plus(g, v), v[0], vc.ALPHA, eps, max_it)[0]
        assert sorted(ids.tolist()) == sorted(lim.model_rows(g, v, eps, max_it)) and not np.isin([lim.LIGHT_ROW, 7], ids).any()
    # the margin is no tautology: exact zeros pass by the other clause, a tiny sum does not
    cancel = (v[0], v[1], np.r_[v[2][:-1], [0.0]])
    assert lim.sign_margin(g, cancel, 0.01, 20)
    tie = lim.with_edges(lim.without_edges(v, [lim.LIGHT_ROW]), [300], [1e-12])   # x(300) is 1e-12 of x(V)
    assert not lim.sign_margin(g, tie, 0.01, 20)


def test_rounds_and_seam_cases(oracle):
    g, visitors = lim.graph_a(), lim.rounds_case()
    check_visitors(g, visitors)
    assert len(visitors) == 17 and visitors[3][1].tolist() == [lim.CYCLE[0]]
    at = [lim.converged_at(g, v, 0.01, 6) for v in visitors]
    # the first tile is never done; the second's word is set by launch 3, before the poll behind launch 3
    assert at[3] is None and None not in at[:3] + at[4:] and at[16] + 1 < 4
    assert [lim.rounds_and_polls(g, visitors, *p) for p in lim.ROUND_PARAMS] == [(2, 0), (8, 0), (9, 2), (10, 2)]
    check_margin(oracle, g, visitors, lim.ROUND_PARAMS)
    live = np.unique(g[1])
    for n in (17, 18):
        good = lim.seam_case(n)
        assert len(good) == n and len({v[0] for v in good}) == n
        check_visitors(g, good)
        kinds = {what: vs for what, vs, _, _ in lim.offenders(n)}
        assert len(kinds) == 4
        for what, vs in kinds.items():
            check_visitors(g, vs[:-1])
            assert len(vs) == n and all(np.array_equal(a[1], b[1]) for a, b in zip(vs[:-1], good[:-1]))
        t = kinds["unknown id"][-1][1]
        assert not np.isin(t[-1], np.union1d(g[0], g[1])) and np.isin(t[:-1], live).all()
        t = kinds["repeated target"][-1][1]
        assert len(np.unique(t)) == len(t) - 1 and np.isin(t, live).all()
        t = kinds["source-only target"][-1][1]
        assert t[-1] in g[0] and t[-1] not in live
        assert np.isnan(kinds["NaN weight"][-1][2]).sum() == 1
