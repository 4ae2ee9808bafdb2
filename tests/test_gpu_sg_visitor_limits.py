"""SG for visitors (csrc/sg_visitors.h, sg_visitors_plan.h, the VIS branch of sg_finalize_batch_body) AT the limits of its
set-up kernel, its per-call tables and its tiles: the cases of tests/sg_visitor_limit_cases.py (proven on the CPU by
test_sg_visitor_limit_cases.py).  The references are test_gpu_sg_visitors.py's: the oracle on G + v (ids and (iterations,
converged) equal, the counter exempt at epsilon 0, probabilities within RTOL = 1e-6), and where a test says "bits" byte
equality of ids, probabilities, counter and flag.  A visitor served alone in a call of its own has fresh tables: equal bits
with that call is the sharp check on what one tile leaves behind for the next.

Each test's docstring names one-line changes of the sources that it is built to catch ("Bites")."""
import numpy as np
import pytest

import sg_visitor_cases as vc
import sg_visitor_limit_cases as lim
from test_gpu_sg_visitors import ALPHA, call, check_reference, raw_call, rows_of, same_bits, untouched

pytestmark = pytest.mark.gpu
_ORACLE = {}


def want(oracle, graph, v, eps, max_it):
    """the oracle's result on G + v, computed once a (graph, visitor, parameters)"""
    key = (id(graph), v[0], v[1].tobytes(), v[2].tobytes(), eps, max_it)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.sg_recommend(*vc.plus(graph, v), v[0], ALPHA, eps, max_it)
    return _ORACLE[key]


def check_call(oracle, sg, graph, visitors, eps, max_it, only=None):
    batch = call(sg, visitors, eps, max_it)
    assert len(batch[0]) == len(visitors) + 1 and batch[0][0] == 0
    for i, v in enumerate(visitors):
        if only is None or i in only:
            check_reference(rows_of(batch, i), want(oracle, graph, v, eps, max_it), eps, (v[0], eps, max_it))
    return batch


def expect_counts(sg, graph, visitors):
    """visitors_stats of the last call against the stage restated"""
    counts = lim.call_counts(graph, visitors)
    st = sg.visitors_stats()
    assert (st["tiles"], st["visitors"], st["set_up_launches"]) == (len(counts), len(visitors), len(counts)), st
    assert st["staged_edges"] == sum(c[0] for c in counts) and st["table_slots"] == max(c[1] for c in counts), (st, counts)
    return st


def alone_bits(sg, batch, visitors, eps, max_it, which):
    for i in which:
        assert same_bits(rows_of(batch, i), rows_of(call(sg, [visitors[i]], eps, max_it), 0)), (i, eps, max_it)


@pytest.fixture(scope="module")
def sga(pkg):
    sg = pkg.SgGraph(*lim.graph_a())
    assert sg.live_count() == lim.T_A + 3
    yield sg
    sg.close()


# ---- A: the set-up kernel's strides -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edges", [255, 256, 257])
def test_a_tile_of_255_256_257_edges(oracle, sga, edges):
    """Bites: the scatter loop of sg_vis_set_up made one pass (edge 256 of the 257 is never written: its visitor loses an
    edge, the CPU proof shows by more than 1e-3); `i < a.n1` read as `i < a.n1 - 1`."""
    g, visitors = lim.graph_a(), lim.stride_tile(edges)
    for eps, max_it in lim.PARAMS + (lim.SWEEPS,):
        check_call(oracle, sga, g, visitors, eps, max_it)
        assert expect_counts(sga, g, visitors)["staged_edges"] == edges


@pytest.mark.parametrize("lines", [16, 17])
def test_a_tile_of_16_and_17_weight_lines(oracle, sga, lines):
    """256 edges in 16 lines (lines * 16 == 256: one stride of the clear exactly), and with one edge moved to a 17th line.
    Behind a tile that left every word of those 17 lines non-zero the results keep their bits.
    Bites: the clear made one pass, or limited to 256 words (line 16 keeps the first tile's weights in 15 columns)."""
    g, visitors, dense = lim.graph_a(), lim.same_rows_tile(lines == 17), lim.dense_tile_17()
    for eps, max_it in lim.PARAMS + (lim.SWEEPS,):
        batch = check_call(oracle, sga, g, visitors, eps, max_it)
        st = expect_counts(sga, g, visitors)
        assert (st["staged_edges"], st["table_slots"]) == (256, lines)
        behind = call(sga, dense + visitors, eps, max_it)
        assert sga.visitors_stats()["table_slots"] == 17
        for i in range(lim.TILE):
            assert same_bits(rows_of(behind, lim.TILE + i), rows_of(batch, i)), (i, eps, max_it)


def test_a_visitor_at_every_live_row(oracle, sga):
    """lines == T == staged edges: every row of the slot table holds a slot, the weight table is T lines of one column.
    Bites: `sl > 0` for `sl >= 0` (row 0's edge is lost); the scatter or the clear made one pass."""
    g, visitors = lim.graph_a(), lim.every_row_visitor()
    for eps, max_it in lim.PARAMS + (lim.SWEEPS,):
        check_call(oracle, sga, g, visitors, eps, max_it)
        st = expect_counts(sga, g, visitors)
        assert st["table_slots"] == st["staged_edges"] == sga.live_count() == 603


def test_a_full_tile_of_1600_edges(oracle, sga):
    """seven strides of the scatter, 568 lines (36 strides of the clear)"""
    g, visitors = lim.graph_a(), lim.wide_tile()
    for eps, max_it in lim.PARAMS:
        check_call(oracle, sga, g, visitors, eps, max_it)
        assert expect_counts(sga, g, visitors)["staged_edges"] == 1600


@pytest.mark.parametrize("wide", [False, True])
def test_a_previous_tile_of_more_than_one_stride(oracle, sga, wide):
    """Two tiles, the first of 272 (1,606) staged edges, the second of 3.  Bites: the loop that puts the previous tile's
    rows back to -1 made one pass or dropped (rows 597 .. 599 keep slots beyond the second tile's 3 lines, whose words
    still hold the first tile's weights: they are added to the second tile's columns 0 .. 2); p0 / p1 taken from tile t."""
    g, visitors = lim.graph_a(), lim.reset_call(wide)
    for eps, max_it in lim.PARAMS + (lim.SWEEPS,):
        batch = check_call(oracle, sga, g, visitors, eps, max_it)
        st = expect_counts(sga, g, visitors)
        assert st["tiles"] == 2 and st["staged_edges"] == (1609 if wide else 275)
        alone_bits(sga, batch, visitors, eps, max_it, range(lim.TILE, lim.TILE + 3))


# ---- B: the tables between tiles ----------------------------------------------------------------------------------------------

def test_b_tables_between_three_tiles(oracle, sga):
    """Bites: the clear limited to 256 words or made one pass (tile 1's lines 16 .. 39 keep tile 0's weights in 15 columns
    each); the first loop dropped, or p0 / p1 taken from tile t (tile 0's rows of A keep their slots in tile 1, and in tile
    2 those of A it does not name); `__syncthreads()` moved below the scatter (a row of tiles 0 and 2, or 1 and 2, may get
    its -1 after its slot)."""
    g, visitors = lim.graph_a(), lim.tables_case()
    for eps, max_it in lim.PARAMS + (lim.SWEEPS,):
        batch = check_call(oracle, sga, g, visitors, eps, max_it)
        st = expect_counts(sga, g, visitors)
        assert (st["tiles"], st["set_up_launches"], st["staged_edges"], st["table_slots"]) == (3, 3, 695, 40)
        if max_it > 0:
            alone_bits(sga, batch, visitors, eps, max_it, range(len(visitors)))


def ranked_equals_plain(sg, visitors, eps, max_it, ids, regions, targets, limit, exclude, plain):
    """visitors_recommend_ranked_batch against prep.rank_recommendations_batch_excluding of the plain call's rows: bits"""
    from locations_recommender_amd import prep
    off, t, w = vc.csr(visitors)
    oi, op, cnt, its, conv = sg.visitors_recommend_ranked_batch(off, t, w, ALPHA, eps, max_it, ids, regions, targets, limit,
                                                               exclude=exclude)
    x = exclude if exclude is not None else (np.zeros(len(visitors) + 1, np.int64), np.zeros(0, np.int64))
    wi, wp, wcnt = prep.rank_recommendations_batch_excluding(plain[0], plain[1], plain[2], ids, regions, targets, limit, *x)
    assert np.array_equal(cnt, wcnt) and np.array_equal(its, plain[3]) and np.array_equal(conv, plain[4])
    for i in range(len(visitors)):
        assert np.array_equal(oi[i, :cnt[i]], wi[i, :cnt[i]]), (i, eps, max_it, limit)
        assert op[i, :cnt[i]].tobytes() == wp[i, :cnt[i]].tobytes(), (i, eps, max_it, limit)
    return oi, cnt


@pytest.mark.parametrize("budget", [None, "1"])
def test_b_tables_between_three_tiles_ranked(sga, monkeypatch, budget):
    """the same three tiles through the ranked entry, whose tiles are consumed on the device"""
    if budget is not None:
        monkeypatch.setenv("LOCREC_SG_RANKED_ROW_BUDGET", budget)
    visitors = lim.tables_case()
    off, t, _ = vc.csr(visitors)
    ids, regions = lim.places_a()
    targets = (np.arange(len(visitors)) % 3).astype(np.int64)
    for eps, max_it, limit in ((0.01, 20, 10), (0.0, 30, 700)):
        plain = call(sga, visitors, eps, max_it)
        ranked_equals_plain(sga, visitors, eps, max_it, ids, regions, targets, limit, None, plain)
        assert sga.visitors_stats()["set_up_launches"] == 3 and sga.ranked_batch_stats()["tiles"] == 3
        oi, cnt = ranked_equals_plain(sga, visitors, eps, max_it, ids, regions, targets, limit, (off, t), plain)
        assert all(not np.isin(oi[i, :cnt[i]], v[1]).any() for i, v in enumerate(visitors)) and cnt.min() > 0
        # visitor 33's list holds every row it would get: count 0, its mates' as before
        mine = rows_of(plain, 33)[0]
        xoff = off.copy()
        xoff[34:] += len(mine) - len(visitors[33][1])
        xt = np.r_[t[:off[33]], mine, t[off[34]:]]
        _, cnt2 = ranked_equals_plain(sga, visitors, eps, max_it, ids, regions, targets, limit, (xoff, xt), plain)
        assert cnt2[33] == 0 and np.array_equal(np.delete(cnt2, 33), np.delete(cnt, 33))


# ---- C: sixteen visitors whatever T --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [65533, 65534, 65535])
def test_c_sixteen_visitors_whatever_T(pkg, oracle, monkeypatch, T):
    """uint16 columns at T = 65533 and 65534, where the persons' tiles are 2 and 1 wide and the visitors' private rows
    T + 1 + b lie beyond 65535: 17 visitors are two tiles on every handle.
    Bites: SgVisitorTiles::tile_max returning sg_batch_tile_max(g) (9 and 17 tiles)."""
    g, graph, visitors = lim.narrow_case(T)
    on = pkg.SgGraph(*graph)
    monkeypatch.setenv("LOCREC_SG_NO_COL16", "1")
    off = pkg.SgGraph(*graph)
    monkeypatch.delenv("LOCREC_SG_NO_COL16")
    assert on.live_count() == T
    narrow = on.info()["device_sweep_bytes"] < off.info()["device_sweep_bytes"]
    assert narrow == (T + 2 <= 65536)
    own = [h.recommend_batch(g["targets"], ALPHA, 0.01, 20) for h in (on, off)]
    batches = {}
    for eps, max_it in lim.PARAMS:
        for name, h in (("on", on), ("off", off)):
            batches[name] = check_call(oracle, h, graph, visitors, eps, max_it, only=(0, 15, 16) if max_it else (0,))
            assert h.visitors_stats()["tiles"] == 2 and h.visitors_stats()["set_up_launches"] == 2
        for i in range(17):
            assert same_bits(rows_of(batches["on"], i), rows_of(batches["off"], i)), (i, eps, max_it)
        alone_bits(on, batches["on"], visitors, eps, max_it, (15,))
        assert same_bits(rows_of(call(on, visitors[:16], eps, max_it), 15), rows_of(batches["on"], 15))
        for h in (on, off):
            ranked_equals_plain(h, visitors, eps, max_it, g["place_ids"], g["regions"], g["target_regions"][:17], 10, None,
                                batches["on"])
            assert h.ranked_batch_stats()["tiles"] == 2 and h.visitors_stats()["tiles"] == 2
    # the slots are back at D and the persons' narrow tiles are intact
    for h, before in zip((on, off), own):
        after = h.recommend_batch(g["targets"], ALPHA, 0.01, 20)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after, before))
    on.close()
    off.close()


# ---- D: degenerate graphs -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["one_edge_case", "cycle_case", "wave_only_case", "every_row_tile"])
def test_d_degenerate_graphs(pkg, oracle, name):
    """T = 1; N == T (no source-only vertex: n_plain_dead = 0); the only row a wave row (n_short = 0); lines == T over the
    three row classes at once.
    Bites: `b.x0 = 1.0 / g->nv` (N + 1 vertices: at T = 1 a third becomes a half); `n_plain_dead = N - T - 1` (the counter
    of the 5-cycle, where it becomes -1, and of every graph whose source-only vertices move); batch_add_visitors skipped for
    wave rows."""
    graph, visitors = getattr(lim, name)()
    sg = pkg.SgGraph(*graph)
    # (at T = 1 also an epsilon that sweep 0's sum passes only with the source-only vertex's x0^2 in it)
    for eps, max_it in lim.D_PARAMS + (((lim.dead_count_epsilon(), 20),) if name == "one_edge_case" else ()):
        check_call(oracle, sg, graph, visitors, eps, max_it)
        st = expect_counts(sg, graph, visitors)
    if name == "wave_only_case":
        assert st["tiles"] == 2 and st["table_slots"] == 1 == sg.live_count()
    if name == "every_row_tile":
        assert (st["staged_edges"], st["table_slots"]) == (640, 40)
    sg.close()


# ---- E: weights ---------------------------------------------------------------------------------------------------------------

def test_e_zero_weights_leave_every_bit(sga):
    """an edge of weight +0.0 or -0.0 gives its row a slot and a line: +0.0 (-0.0) times a finite x leaves every column's
    sum as it is, the visitor's own and its tile mates'"""
    plain, extra = lim.zero_weight_case()
    for eps, max_it in lim.PARAMS + (lim.SWEEPS,):
        a = call(sga, plain, eps, max_it)
        edges = sga.visitors_stats()["staged_edges"]
        b = call(sga, extra, eps, max_it)
        assert sga.visitors_stats()["staged_edges"] == edges + 2
        for i in range(len(plain)):
            assert same_bits(rows_of(a, i), rows_of(b, i)), (i, eps, max_it)


def test_e_negative_weight(oracle, sga):
    """x(602) and x(7) are negative from the first sweep on (the CPU proof: every sign has a margin): neither is returned"""
    g, v = lim.graph_a(), lim.negative_weight_case()
    for eps, max_it in lim.NEGATIVE_PARAMS:
        batch = check_call(oracle, sga, g, [v], eps, max_it)
        ids = rows_of(batch, 0)[0]
        assert not np.isin([lim.LIGHT_ROW, 7], ids).any() and sorted(ids.tolist()) == sorted(lim.model_rows(g, v, eps, max_it))


# ---- F: rounds and polls with two tiles ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps,max_it", lim.ROUND_PARAMS)
def test_f_rounds_and_polls_of_two_tiles(oracle, sga, eps, max_it):
    """the host polls only above 4 sweeps; a tile whose columns are all done stops at its next poll, one with a column in the
    two-cycle runs to the maximum"""
    g, visitors = lim.graph_a(), lim.rounds_case()
    check_call(oracle, sga, g, visitors, eps, max_it)
    st = expect_counts(sga, g, visitors)
    assert (st["finalize_launches"], st["polls"]) == lim.rounds_and_polls(g, visitors, eps, max_it)
    assert (st["polls"] == 0) == (max_it <= 4)


# ---- G: the protocol across a tile seam ---------------------------------------------------------------------------------------

ROOM = 1 << 15


def test_g_capacity_protocol_with_two_tiles(pkg, sga):
    from locations_recommender_amd import _lib as L
    args = vc.csr(lim.seam_case(17))
    st, full, need, _ = raw_call(pkg, sga, *args, 0.01, 20, room=ROOM)
    assert st == L.OK and need == full[0][17] > full[0][16] > 0 and (full[3] >= 0).all()
    st, outs, cap, _ = raw_call(pkg, sga, *args, 0.01, 20, room=need - 1)   # one short: offsets and counters only
    assert st == L.OK and cap == need and np.array_equal(outs[0], full[0]) and untouched(outs[1:3])
    assert np.array_equal(outs[3], full[3]) and np.array_equal(outs[4], full[4])
    st, outs, cap, _ = raw_call(pkg, sga, *args, 0.01, 20, room=need)
    assert st == L.OK and cap == need and outs[1].tobytes() == full[1][:need].tobytes() and outs[2].tobytes() == full[2][:need].tobytes()
    st, outs, cap, _ = raw_call(pkg, sga, *args, 0.01, 20, room=0, null_rows=True)
    assert st == L.OK and cap == need and np.array_equal(outs[0], full[0]) and np.array_equal(outs[3], full[3])


@pytest.mark.parametrize("n", [17, 18])
def test_g_offender_behind_the_seam(pkg, sga, n):
    """the offender is the first (second) visitor of the second tile: nothing is staged or launched"""
    from locations_recommender_amd import _lib as L
    for what, visitors, status, text in lim.offenders(n):
        call(sga, lim.seam_case(n), 0.01, 20)
        assert sga.visitors_stats()["finalize_launches"] > 0
        st, outs, cap, bad = raw_call(pkg, sga, *vc.csr(visitors), 0.01, 20, room=ROOM)
        assert st == getattr(L, status) and bad == n - 1 and untouched(outs) and cap == ROOM, (what, st, bad)
        assert text in L.lib().locrec_last_error().decode(), what
        assert set(sga.visitors_stats().values()) == {0}, what
