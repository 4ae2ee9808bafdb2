"""The cases of the pool visitors tests (test_sg_pool_visitor_cases.py proves them on the CPU, test_gpu_sg_pool_visitors.py
runs them): members of a pool as edge lists and ONE call's visitors as (member, visitor), interleaved in call order.  The
graphs and visitors are sg_visitor_cases.py's - no graph is built here that is not built there."""
import functools

import numpy as np

import sg_visitor_cases as cases

ALPHA = cases.ALPHA
PARAMS = cases.PARAMS
FORMS = ("default", "LOCREC_SG_NO_DICT", "LOCREC_SG_NO_COL16", "fp64 weights")   # of degree_case, as test_gpu_sg_visitors builds them


def interleave(lists):
    """[(member, visitor)] in call order: the members' lists dealt round-robin, each member's own order kept"""
    out, at = [], [0] * len(lists)
    while any(a < len(l) for a, l in zip(at, lists)):
        for g, l in enumerate(lists):
            if at[g] < len(l):
                out.append((g, l[at[g]]))
                at[g] += 1
    return out


def call_csr(asked):
    """(graph_index, edge_offsets, target_ids, weights) of a pool visitors call"""
    return (np.array([g for g, _ in asked], np.int32),) + cases.csr([v for _, v in asked])


def of_member(asked, g):
    """the call positions of member g's visitors, in call order"""
    return [i for i, (m, _) in enumerate(asked) if m == g]


@functools.lru_cache(maxsize=None)
def mixed_case():
    """Five members: the KAT graph and degree_case in its four forms.  In call order, interleaved: 18 visitors on the
    default form (two waves), 16 on NO_DICT (one full tile), 3 on NO_COL16, 1 on the KAT graph, nobody on the fp64 form.
    -> (graphs [5 edge lists], asked [(member, visitor)], checked: the call positions the oracle is asked about)"""
    kat, kat_v = cases.kat_case()
    deg, deg_v = cases.degree_case()
    deg64, _ = cases.degree_case(distinct_weights=True)
    graphs = [kat, deg, deg, deg, deg64]
    asked = interleave([kat_v[:1], deg_v[:18], deg_v[:16], [deg_v[3], deg_v[7], deg_v[17]], []])
    # one visitor per asked member, the three hub visitors and the all-hubs visitor (on the member of two waves), its 17th
    checked = [of_member(asked, 0)[0], of_member(asked, 2)[5], of_member(asked, 3)[0]] + [of_member(asked, 1)[j] for j in (0, 1, 2, 3, 16)]
    return graphs, asked, sorted(checked)


HUB, SHARED = 2, 7   # the slot case: tile 0's hub row (the wave row of degree_case) and the row visitor 16 shares with tile 0
TILE0_TARGETS, TILE0_WEIGHTS = (0, 1, HUB, SHARED), (0.05, 0.05, 0.8, 0.1)
SLOT_PARAMS = ((0.01, 20), (1e-6, 200))


@functools.lru_cache(maxsize=None)
def slot_case():
    """One member (degree_case) with 17 visitors.  The 16 of tile 0 point at the hub row with weight 0.8 and at three more
    rows: four lines of the weight table, the hub's the third.  Visitor 16 points at SHARED and one other row, not at the
    hub: its tile has two lines, so a slot left at the hub's row would still name a line that holds tile 0's 0.8.
    -> (graph, visitors[17])"""
    graph, _ = cases.degree_case()
    tile0 = [(60_000 + i, np.array(TILE0_TARGETS, np.int64), np.array(TILE0_WEIGHTS)) for i in range(16)]
    rng = np.random.default_rng(41)
    for _ in range(20):
        w = rng.random(2) + 0.1
        last = (60_016, np.array([SHARED, 9], np.int64), w / w.sum())
        if cases.has_margin(graph, last, SLOT_PARAMS):
            return graph, tile0 + [last]
    raise AssertionError("no weights keep the margin")


def with_left_over(graph, visitor, row, weight, sweeps):
    """x of makeRecommendations(V) on G + v after `sweeps` sweeps, in numpy - and the same with weight * x_V added to the
    sum of `row` in every sweep: what a slot left at `row` by the previous tile would add.  -> (ids, x, x with the left-over)"""
    src, dst, w = cases.plus(graph, visitor)
    vid, inv = np.unique(np.concatenate([src, dst]), return_inverse=True)
    cs, ct = inv[:len(src)], inv[len(src):]
    me, at = int(np.searchsorted(vid, visitor[0])), int(np.searchsorted(vid, row))
    u = (vid == visitor[0]).astype(np.float64)
    out = []
    for extra in (0.0, weight):
        x = np.full(len(vid), 1.0 / len(vid))
        for _ in range(sweeps):
            s = np.bincount(ct, weights=x[cs] * w, minlength=len(vid))
            s[at] += extra * x[me]
            x = ALPHA * u + (1 - ALPHA) * s
        out.append(x)
    return vid, out[0], out[1]


@functools.lru_cache(maxsize=None)
def drop_out_case():
    """Three members (copies of degree_case's graph) with 33, 2 and 17 visitors: waves 1 and 2 run without member 1,
    wave 2 with member 0 only.  -> (graphs, asked)"""
    graph, v = cases.degree_case()
    lists = [[v[i % 18] for i in range(33)], [v[4], v[9]], [v[(5 * i + 1) % 18] for i in range(17)]]
    return [graph] * 3, interleave(lists)
