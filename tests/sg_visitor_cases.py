"""The cases of the SG visitors tests (test_sg_visitor_cases.py proves them on the CPU, test_gpu_sg_visitors.py runs them):
a graph G as an edge list, and visitors - persons G has no vertex for - as (id, target_ids, weights); G + v is G's list
followed by the visitor's edges under its id.

Every visitor of a case keeps a margin to a tie of the iteration counter: for each (epsilon, max_iterations) of PARAMS the
squared differences of the last two sweeps of makeRecommendations on G + v lie on opposite sides of epsilon^2 by a factor of
MARGIN at least (or the last lies above it by that factor when the maximum ends the run), so the device and the oracle,
which add in different orders, must agree on (iterations, converged).  Candidates that miss the margin are replaced here."""
import functools
import json
import os

import numpy as np

ALPHA = 0.15
MARGIN = 1 + 1e-9
PARAMS = ((0.01, 20), (0.0, 100), (0.01, 0), (1e-6, 200))
KAT_PARAMS = ((0.01, 1), (0.05, 1000))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLOTS, LONG_ROW = 256, 8   # sg_layout_plan.h: kSgPlanSlots, kSgPlanLongRow


def row_class(degree):
    """sg_in_long_area / sg_wave_row of sg_layout_plan.h, restated: which loop of the finalize sums a row."""
    nfull = degree // SLOTS
    if not nfull > 2:
        return "short"
    return "wave" if nfull > LONG_ROW else "medium"


def plus(graph, visitor):
    """G + v"""
    src, dst, w = graph
    vid, t, vw = visitor
    return (np.r_[src, np.full(len(t), vid, np.int64)], np.r_[dst, np.asarray(t, np.int64)], np.r_[w, np.asarray(vw, np.float64)])


def d2_trajectory(edges, v, n, stop=0.0):
    """isConverged's sum (StochasticRecommender.scala:130-141) of sweeps 0 .. for target v, in numpy; ends after n sweeps or
    behind the first sum <= stop."""
    src, dst, w = edges
    vid, inv = np.unique(np.concatenate([src, dst]), return_inverse=True)
    cs, ct = inv[:len(src)], inv[len(src):]
    u = (vid == v).astype(np.float64)
    x = np.full(len(vid), 1.0 / len(vid))
    out = []
    for _ in range(n):
        xn = ALPHA * u + (1 - ALPHA) * np.bincount(ct, weights=x[cs] * w, minlength=len(vid))
        out.append(float(np.sum((xn - x) ** 2)))
        x = xn
        if out[-1] <= stop:
            break
    return np.array(out)


def verdict(d2, eps, max_it):
    """(iterations, converged, has the margin) of step() (:92-106) on the sums d2 of the sweeps: sweep k runs when k <
    max_it and no earlier sum was <= eps^2."""
    e2 = eps * eps
    for k in range(max_it):
        if d2[k] <= e2:
            ok = d2[k] * MARGIN <= e2 and (k == 0 or d2[k - 1] >= e2 * MARGIN)
            return k, True, ok
        if not d2[k] >= e2 * MARGIN:
            return k, False, False
    return max_it, False, True


def has_margin(graph, visitor, params):
    """every (epsilon, max_iterations) with epsilon > 0 (with 0 the counter is exempt: the run ends at an exact fixed point)"""
    need = max(m for _, m in params)
    low = min((e * e for e, _ in params if e > 0), default=0.0) / 4
    d2 = d2_trajectory(plus(graph, visitor), visitor[0], need, stop=low)
    d2 = np.r_[d2, np.zeros(need - len(d2))]   # (behind the stop every sum counts as below every epsilon^2: never looked at)
    return all(verdict(d2, e, m)[2] for e, m in params if e > 0)


def kat_case():
    """StochasticRecommenderTest.scala's graph without its source vertex 1, which comes back as the visitor"""
    with open(os.path.join(GOLD, "sg_kats.json")) as f:
        e = np.array(json.load(f)["edges"], dtype=np.float64)
    src, dst, w = e[:, 0].astype(np.int64), e[:, 1].astype(np.int64), e[:, 2]
    own = src == 1
    return (src[~own], dst[~own], w[~own]), [(1, dst[own], w[own])]


@functools.lru_cache(maxsize=None)
def synth_case(n=40):
    """synth.sg_dataset(3000, 300, 20, seed 77) without the edges of n persons, who come back as visitors: three tiles of
    16, 16 and 8.  A person qualifies when every target stays live without the n persons and the margin holds."""
    import __graft_entry__ as entry
    entry.load_package()
    from locations_recommender_amd import synth
    g = synth.sg_dataset(n_persons=3_000, n_places=300, n_categories=20, seed=77)
    src, dst, w = g["source_id"], g["target_id"], g["balanced_weight"]
    person0 = int(g["first_person"])
    rng = np.random.default_rng(5)
    cand = person0 + rng.choice(3_000, 2 * n, replace=False)
    # the graph without ALL candidates: a candidate that is not chosen stays out too (a smaller G is as good a G)
    out = np.isin(src, cand)
    graph = (src[~out], dst[~out], w[~out])
    live = np.unique(graph[1])
    visitors = []
    for p in cand:
        own = src == p
        v = (int(p), dst[own], w[own])
        if np.isin(v[1], live).all() and has_margin(graph, v, PARAMS):
            visitors.append(v)
        if len(visitors) == n:
            break
    assert len(visitors) == n, "too few candidates keep the margin"
    return graph, visitors


HUBS = ((0, 700), (1, 1000), (2, 2400))   # (live vertex, in-degree): a short, a medium and a wave row
N_SOURCES, N_LIVE, SOURCE0 = 2_600, 40, 10_000


@functools.lru_cache(maxsize=None)
def degree_case(distinct_weights=False):
    """About 2,600 source-only vertices and 40 live ones; three hub rows of in-degree 700, 1,000 and 2,400, one of each
    class of the finalize.  Visitors 0, 1, 2 point at one hub each, visitor 3 at all three (and two plain rows), the rest at
    random rows: 18 visitors, two tiles.  The weights are eight values (the handle streams a dictionary index), or with
    distinct_weights more than 8192 different ones (it streams the fp64 weights); no source's weights add up to more than 1."""
    rng = np.random.default_rng(123)
    s, t = [], []
    for (hub, deg), first in zip(HUBS, (1_000, 0, 100)):   # distinct sources per hub: no parallel edges
        s.append(SOURCE0 + (first + np.arange(deg)) % N_SOURCES)
        t.append(np.full(deg, hub))
    plain = np.arange(len(HUBS), N_LIVE)
    for k in range(2):   # every source also points at two plain rows (different ones: k decides the parity)
        s.append(SOURCE0 + np.arange(N_SOURCES))
        t.append(plain[(2 * rng.integers(0, len(plain) // 2, N_SOURCES) + k) % len(plain)])
    for k in (1, 5, 11):   # live -> plain live: the walk goes on behind the first hop
        s.append(np.arange(N_LIVE))
        t.append(plain[(np.arange(N_LIVE) * 3 + k) % len(plain)])
    src, dst = np.concatenate(s).astype(np.int64), np.concatenate(t).astype(np.int64)
    w = rng.integers(1, 9, len(src)) / 32.0   # (at most five out-edges a vertex)
    if distinct_weights:
        w = w * (1 - np.arange(len(src)) * 1e-9)
        assert len(np.unique(w)) > 8192
    graph = (src, dst, w)

    def visitor(vid, targets):
        for _ in range(20):   # new weights until the margin holds
            vw = rng.random(len(targets)) + 0.1
            v = (vid, np.asarray(targets, np.int64), vw / vw.sum())
            if has_margin(graph, v, PARAMS):
                return v
        raise AssertionError("no weights keep the margin")

    lists = [[0], [1], [2], [0, 1, 2, 5, 17]]
    lists += [rng.choice(N_LIVE, int(rng.integers(1, 7)), replace=False).tolist() for _ in range(14)]
    return graph, [visitor(50_000 + i, tg) for i, tg in enumerate(lists)]


STOP_MAX_IT = 12


@functools.lru_cache(maxsize=None)
def stop_case():
    """Two visitors of one tile that stop at different sweeps: 400 persons over 30 live vertices, and a two-cycle 2000 <->
    2001 of its own where mass swings back and forth.  Visitor 0 spreads over the 30 and converges at sweep 3 for the
    returned epsilon (between its sums of sweeps 2 and 3); visitor 1 enters the two-cycle and is stopped by STOP_MAX_IT.
    -> (graph, [fast, slow], epsilon)"""
    rng = np.random.default_rng(17)
    src = np.r_[rng.integers(1000, 1400, 4000), rng.integers(0, 30, 600), 2000, 2001].astype(np.int64)
    dst = np.r_[rng.integers(0, 30, 4000), rng.integers(0, 30, 600), 2001, 2000].astype(np.int64)
    w = np.r_[rng.random(4600) / 30, 1.0, 1.0]
    graph = (src, dst, w)
    fast = (9000, np.arange(30, dtype=np.int64), np.full(30, 1 / 30))
    slow = (9001, np.array([2000], np.int64), np.array([1.0]))
    df = d2_trajectory(plus(graph, fast), fast[0], STOP_MAX_IT)
    eps = float(np.sqrt(np.sqrt(df[2] * df[3])))
    return graph, [fast, slow], eps


def csr(visitors):
    """(edge_offsets, target_ids, weights) of a visitors call"""
    off = np.zeros(len(visitors) + 1, np.int64)
    np.cumsum([len(v[1]) for v in visitors], out=off[1:])
    return off, np.concatenate([np.asarray(v[1], np.int64) for v in visitors]), np.concatenate([np.asarray(v[2], np.float64) for v in visitors])
