"""The cases of the SG visitors tests (sg_visitor_cases.py) stand where they claim, proven on the CPU: the hub rows of the
degree-class graph fall into the three row classes of the finalize and visitors point at each; every visitor is no vertex
of its graph and names live vertices only, each once; and on G + v the oracle ends no run within one sweep of a tie."""
import numpy as np
import pytest

import sg_visitor_cases as cases


def check_visitors(graph, visitors):
    src, dst, _ = graph
    live = np.unique(dst)
    vertices = np.union1d(src, dst)
    for vid, t, w in visitors:
        assert vid not in vertices
        assert len(t) >= 1 and len(np.unique(t)) == len(t) and np.isin(t, live).all()
        assert np.isfinite(w).all()


def check_margin(oracle, graph, visitors, params):
    """the oracle's own (iterations, converged) is the one the squared differences predict, and those keep the margin"""
    for v in visitors:
        edges = cases.plus(graph, v)
        need = max(m for _, m in params)
        d2 = cases.d2_trajectory(edges, v[0], need)
        for eps, max_it in params:
            if eps == 0:
                continue
            it, conv, ok = cases.verdict(d2, eps, max_it)
            assert ok, (v[0], eps, max_it)
            _, _, oit, oconv = oracle.sg_recommend(*edges, v[0], cases.ALPHA, eps, max_it)
            assert (oit, oconv) == (it, conv), (v[0], eps, max_it)


def test_row_classes_restated():
    assert [cases.row_class(d) for d in (1, 767, 768, 2303, 2304, 100_000)] == ["short", "short", "medium", "medium", "wave", "wave"]


def test_degree_case(oracle):
    graph, visitors = cases.degree_case()
    src, dst, w = graph
    sources = np.setdiff1d(src, dst)
    live = np.unique(dst)
    assert len(live) == cases.N_LIVE and 2_500 <= len(sources) <= 2_700
    deg = np.bincount(dst, minlength=cases.N_LIVE)
    assert [(int(deg[h]), cases.row_class(int(deg[h]))) for h, _ in cases.HUBS] == [(700, "short"), (1000, "medium"), (2400, "wave")]
    assert all(cases.row_class(int(d)) == "short" for d in deg[len(cases.HUBS):])
    assert len(np.unique(np.stack([src, dst]), axis=1)[0]) == len(src)   # no parallel edges
    check_visitors(graph, visitors)
    hit = [{cases.row_class(int(deg[t])) for t in v[1] if t < len(cases.HUBS)} for v in visitors]
    assert hit[0] == {"short"} and hit[1] == {"medium"} and hit[2] == {"wave"} and hit[3] == {"short", "medium", "wave"}
    assert len(visitors) > 16   # more than one tile
    check_margin(oracle, graph, visitors, cases.PARAMS)


def test_synth_case(oracle):
    graph, visitors = cases.synth_case()
    assert len(visitors) == 40 and len({v[0] for v in visitors}) == 40
    check_visitors(graph, visitors)
    check_margin(oracle, graph, visitors[::4], cases.PARAMS)   # (has_margin decided every one: the oracle confirms a tenth)


def test_stop_case(oracle):
    graph, visitors, eps = cases.stop_case()
    check_visitors(graph, visitors)
    check_margin(oracle, graph, visitors, ((eps, cases.STOP_MAX_IT),))
    got = [oracle.sg_recommend(*cases.plus(graph, v), v[0], cases.ALPHA, eps, cases.STOP_MAX_IT)[2:] for v in visitors]
    assert got == [(3, True), (cases.STOP_MAX_IT, False)]


def test_kat_case(oracle):
    graph, visitors = cases.kat_case()
    check_visitors(graph, visitors)
    assert visitors[0][0] == 1 and sorted(visitors[0][1].tolist()) == [2, 3, 5]
    check_margin(oracle, graph, visitors, cases.KAT_PARAMS)
    full = cases.plus(graph, visitors[0])
    assert len(full[0]) == 9
