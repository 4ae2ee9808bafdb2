"""The cases of the pool visitors tests (sg_pool_visitor_cases.py) have the properties the GPU tests rely on, proven on the
CPU: who is asked of which member and in which wave, that every visitor is no vertex of ITS member and names live vertices
of it only, that the oracle ends no checked run within one sweep of a tie, and that a slot left behind by the previous
tile would move the slot case's last visitor by far more than the GPU test's tolerance."""
import numpy as np

import sg_pool_visitor_cases as pc
import sg_visitor_cases as cases
from test_sg_visitor_cases import check_margin, check_visitors

RTOL = 1e-6   # test_gpu_sg_pool_visitors.py's


def test_interleave_keeps_every_members_order():
    got = pc.interleave([["a", "b", "c"], [], ["x"]])
    assert got == [(0, "a"), (2, "x"), (0, "b"), (0, "c")]
    gi, off, t, w = pc.call_csr([(1, (5, [2, 3], [.5, .5])), (0, (6, [4], [1.]))])
    assert gi.tolist() == [1, 0] and off.tolist() == [0, 2, 3] and t.tolist() == [2, 3, 4] and gi.dtype == np.int32


def test_mixed_case(oracle):
    graphs, asked, checked = pc.mixed_case()
    assert len(graphs) == 5 and len(asked) == 38
    counts = [len(pc.of_member(asked, g)) for g in range(5)]
    assert counts == [1, 18, 16, 3, 0]   # one visitor, two waves, one full tile, three, nobody
    assert [g for g, _ in asked[:8]] == [0, 1, 2, 3, 1, 2, 3, 1]   # interleaved in call order
    for g in range(4):
        check_visitors(graphs[g], [asked[i][1] for i in pc.of_member(asked, g)])
    # the oracle is asked about every asked member, the hub visitors, the all-hubs visitor and a visitor of the second wave
    assert {asked[i][0] for i in checked} == {0, 1, 2, 3}
    on1 = [pc.of_member(asked, 1).index(i) for i in checked if asked[i][0] == 1]
    assert on1 == [0, 1, 2, 3, 16]
    deg = np.bincount(graphs[1][1], minlength=cases.N_LIVE)
    hubs = [sorted(cases.row_class(int(deg[t])) for t in asked[pc.of_member(asked, 1)[j]][1][1] if t < len(cases.HUBS)) for j in range(4)]
    assert hubs == [["short"], ["medium"], ["wave"], ["medium", "short", "wave"]]
    for i in checked:
        g, v = asked[i]
        check_margin(oracle, graphs[g], [v], cases.PARAMS)   # (the KAT visitor too: the pool runs it at PARAMS)
    # the fp64 form differs from the default one in its weights only: more than 8192 distinct values
    assert np.array_equal(graphs[4][0], graphs[1][0]) and len(np.unique(graphs[4][2])) > 8192 >= len(np.unique(graphs[1][2]))


def test_slot_case(oracle):
    graph, visitors = pc.slot_case()
    assert len(visitors) == 17
    check_visitors(graph, visitors)
    last = visitors[16]
    for v in visitors[:16]:
        assert pc.HUB in v[1] and v[2][list(v[1]).index(pc.HUB)] == 0.8 and len(v[1]) == 4   # four lines, the hub's weight large
    assert pc.HUB not in last[1] and len(np.intersect1d(last[1], visitors[0][1])) == 1 and len(last[1]) == 2   # two lines
    deg = np.bincount(graph[1], minlength=cases.N_LIVE)
    assert cases.row_class(int(deg[pc.HUB])) == "wave"
    check_margin(oracle, graph, [last], pc.SLOT_PARAMS)
    # tile 0's product at the hub's row, added by hand: the probabilities move by far more than RTOL, at the hub's row and
    # (one hop on) at the rows it points at - the GPU test cannot pass with a slot left behind
    for sweeps in (1, 2, 20):
        vid, x, x_left = pc.with_left_over(graph, last, pc.HUB, 0.8, sweeps)
        oi, op, _, _ = oracle.sg_recommend(*cases.plus(graph, last), last[0], pc.ALPHA, 0.0, sweeps)
        np.testing.assert_allclose(x[np.isin(vid, oi)], op, rtol=1e-9, atol=0)   # the numpy iteration is the oracle's
        moved = np.abs(x_left - x) > 1000 * RTOL * np.abs(x)
        assert moved[np.searchsorted(vid, pc.HUB)]
        assert sweeps < 2 or moved.sum() >= 3


def test_drop_out_case():
    graphs, asked = pc.drop_out_case()
    counts = [len(pc.of_member(asked, g)) for g in range(3)]
    assert counts == [33, 2, 17]
    waves = [-(-c // 16) for c in counts]
    assert waves == [3, 1, 2]   # waves 1 and 2 run without member 1, wave 2 with member 0 only
    for g in range(3):
        check_visitors(graphs[g], [asked[i][1] for i in pc.of_member(asked, g)])
