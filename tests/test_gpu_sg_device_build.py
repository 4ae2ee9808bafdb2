"""The stochastic graph's layout built on the device (csrc/sg_create_device.hip: locrec_sg_create_from_device) against
the layout locrec_sg_create builds on the host from the same arrays.

The contract is layout identity, and a row's sum runs in slot order, so every comparison is exact: the same vertex ids,
the same probability BITS, the same iteration counter and converged flag, the same locrec_sg_info / device_bytes /
weight_dictionary / live_count.  Both handles of a comparison are created under the same environment.  The
device-built result is also compared with the oracle at the tolerance of tests/test_gpu_sg.py.

The graphs (tests/sg_build_cases.py) are the smallest that can go wrong: a plan or a placement error shows in a row of
a given class, not at a given size."""
import json
import os

import numpy as np
import pytest
import torch

import prep_cases
import sg_build_cases as cases

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-6          # tests/test_gpu_sg.py (BASELINE.json north_star)
ALPHA = 0.15
SETTINGS = ((0.01, 20), (0.0, 7))


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def build_both(pkg, s, t, w):
    host = pkg.SgGraph(s, t, w)
    device = pkg.SgGraph.from_device(dev(s, np.int64), dev(t, np.int64), dev(w, np.float64))
    return host, device


def facts(g):
    return dict(g.info(), live_count=g.live_count())


def same_result(a, b, what=None):
    assert np.array_equal(a[0], b[0]), what
    assert np.array_equal(np.asarray(a[1]).view(np.uint64), np.asarray(b[1]).view(np.uint64)), what   # the bits
    assert (a[2], a[3]) == (b[2], b[3]), what


def compare(pkg, oracle, s, t, w, requests, batch=True, settings=SETTINGS):
    """Host-built vs device-built handle of one edge list over `requests` (in this order on both handles, so the
    dead-slot patching from one request to the next is compared too), then the batched call."""
    host, device = build_both(pkg, s, t, w)
    try:
        assert facts(host) == facts(device)
        for eps, max_it in settings:
            for v in requests:
                a = host.recommend(v, ALPHA, eps, max_it)
                b = device.recommend(v, ALPHA, eps, max_it)
                same_result(a, b, (v, eps, max_it))
                oi, op, oit, oconv = oracle.sg_recommend(s, t, w, v, ALPHA, eps, max_it)
                assert np.array_equal(b[0], oi) and (b[2], b[3]) == (oit, oconv), (v, eps, max_it)
                np.testing.assert_allclose(b[1], op, rtol=RTOL, atol=0)
            if batch:
                targets = list(dict.fromkeys(requests))
                a = host.recommend_batch(targets, ALPHA, eps, max_it)
                b = device.recommend_batch(targets, ALPHA, eps, max_it)
                for x, y in zip(a, b):
                    assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (eps, max_it)
        return facts(device)
    finally:
        host.close()
        device.close()


@pytest.fixture(scope="module")
def layout():
    return cases.layout_graph()


# ---- 1. the reference's known answers ---------------------------------------------------------------------------

def test_reference_kats_from_device_tensors(pkg):
    """The 9-edge graph of StochasticRecommenderTest as tests/test_gpu_sg.py loads it, built from device tensors."""
    with open(os.path.join(GOLD, "sg_kats.json")) as f:
        g = json.load(f)
    e = np.array(g["edges"], dtype=np.float64)
    s, t, w = e[:, 0].astype(np.int64), e[:, 1].astype(np.int32), e[:, 2]
    sg = pkg.SgGraph.from_device(dev(s, np.int64), dev(t, np.int64), dev(w, np.float64))
    answers = 0
    for case in g["cases"]:
        if "expected_error" in case:
            with pytest.raises(pkg.IllegalArgumentException, match="No such vertex in the graph: 100"):
                sg.recommend(case["vertex_id"], ALPHA, case["epsilon"], case["max_iterations"])
            continue
        ids, probs, _, _ = sg.recommend(case["vertex_id"], ALPHA, case["epsilon"], case["max_iterations"])
        rows = sorted(zip(ids.tolist(), probs.tolist()), key=lambda r: -r[1])
        assert rows == [tuple(x) for x in case["expected_sorted_by_probability_desc"]], case["name"]
        answers += 1
    assert answers == 2
    sg.close()


# ---- 2. every layout class in one graph -------------------------------------------------------------------------

def test_every_layout_class(pkg, oracle, layout):
    f = compare(pkg, oracle, layout["source"], layout["target"], layout["weight"], layout["requests"])
    assert f["live_count"] == cases.N_LIVE and 0 < f["weight_dictionary"] <= 8192


# ---- 3. id spaces -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["dense", "spread", "dense_ranked_by_sort"])
def test_id_spaces(pkg, oracle, layout, monkeypatch, space):
    """The table over [min id, max id], the sort of the 2 E ids forced by the ids (2^40 apart, negative, both ends of
    int64) and forced by LOCREC_SG_NO_DENSE_IDS: the same vertex order, so the same layout."""
    s, t = layout["source"], layout["target"]
    requests = layout["requests"]
    if space == "dense":
        s, t, requests = s - 50, t - 50, [v - 50 for v in requests]           # dense, some of them negative
    elif space == "spread":
        top = int(max(s.max(), t.max()))
        requests = [int(x) for x in cases.spread_ids(requests, top)]
        s, t = cases.spread_ids(s, top), cases.spread_ids(t, top)
        assert min(s.min(), t.min()) == np.iinfo(np.int64).min + 1 and s.max() == np.iinfo(np.int64).max
    else:
        monkeypatch.setenv("LOCREC_SG_NO_DENSE_IDS", "1")
    compare(pkg, oracle, s, t, layout["weight"], requests)


# ---- 4. create-time switches ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,value", [("LOCREC_SG_NO_COL16", "1"), ("LOCREC_SG_NO_DICT", "1"), ("LOCREC_SG_GS", "2"),
                                        ("LOCREC_SG_FUSED", "1")])
def test_create_time_switches(pkg, oracle, layout, monkeypatch, name, value):
    """Both handles under the same switch.  LOCREC_SG_FUSED is the host fallback of the device entry point (the
    experiment keeps its host-only layout; its handles refuse the batched call)."""
    monkeypatch.setenv(name, value)
    f = compare(pkg, oracle, layout["source"], layout["target"], layout["weight"], layout["requests"],
                batch=name != "LOCREC_SG_FUSED")
    if name == "LOCREC_SG_NO_DICT":
        assert f["weight_dictionary"] == 0


# ---- 5. where the data itself selects the format ----------------------------------------------------------------

def test_more_live_rows_than_uint16_columns_hold(pkg, oracle):
    s, t, w = cases.one_edge_rows()
    f = compare(pkg, oracle, s, t, w, [int(s[0]), int(t[5]), int(s[1])])
    assert f["live_count"] == 70_000 and f["live_count"] + 2 > 65_536


def test_more_distinct_weights_than_the_dictionary_holds(pkg, oracle):
    s, t, w = cases.many_weights()
    assert len(np.unique(w)) > 8192
    f = compare(pkg, oracle, s, t, w, [int(s[0]), int(t[0]), int(s[1])])
    assert f["weight_dictionary"] == 0


# ---- 6. group membership ----------------------------------------------------------------------------------------

def test_device_built_graphs_in_a_group(pkg, layout):
    from locations_recommender_amd import synth
    specs = [synth.sg_dataset(n_persons=500, n_places=80, n_categories=10, seed=32),
             synth.sg_dataset(n_persons=900, n_places=120, n_categories=10, seed=34)]
    edges = [(g["source_id"], g["target_id"], g["balanced_weight"]) for g in specs]
    edges.append((layout["source"], layout["target"], layout["weight"]))
    targets = [int(specs[0]["first_person"]), int(specs[1]["first_person"]) + 3, cases.HUB_A]
    results = []
    for make in (lambda e: pkg.SgGraph(*e),
                 lambda e: pkg.SgGraph.from_device(dev(e[0], np.int64), dev(e[1], np.int64), dev(e[2], np.float64))):
        graphs = [make(e) for e in edges]
        grp = pkg.SgGroup(graphs)
        got = []
        grp.sweeps_async(targets, ALPHA, 9)
        grp.synchronize()
        got.append([g.fetch() for g in graphs])
        for eps, max_it in SETTINGS:
            grp.iterate_async(targets, ALPHA, eps, max_it)
            got.append([g.fetch() for g in graphs])
        results.append(got)
        grp.close()
        for g in graphs:
            g.close()
    for a, b in zip(*results):
        for x, y in zip(a, b):
            same_result(x, y)
    assert all(len(r[0]) >= 10 for r in results[1][0])


# ---- 7. hygiene -------------------------------------------------------------------------------------------------

def test_inputs_unchanged_repeatable_and_memory_returned(pkg, layout):
    from locations_recommender_amd import _lib as L
    cols = [dev(layout["source"], np.int64), dev(layout["target"], np.int64), dev(layout["weight"], np.float64)]
    kept = [c.clone() for c in cols]
    before = L.device_bytes_in_use()
    first = pkg.SgGraph.from_device(*cols)
    for c, k in zip(cols, kept):
        assert torch.equal(c.view(torch.int64), k.view(torch.int64))
    second = pkg.SgGraph.from_device(*cols)
    assert facts(first) == facts(second)
    for v in layout["requests"]:
        same_result(first.recommend(v, ALPHA, 0.0, 7), second.recommend(v, ALPHA, 0.0, 7), v)
    stats = pkg.SgGraph.device_build_stats()
    assert sorted(stats) == ["dictionary_ms", "plan_ms", "ranking_ms", "scatter_ms"] and all(x > 0 for x in stats.values())
    first.close()
    second.close()
    assert L.device_bytes_in_use() == before


def test_host_build_repeatable_and_memory_returned(pkg, layout):
    """The same of locrec_sg_create: two builds of one edge list are one layout, and closing them returns every byte."""
    from locations_recommender_amd import _lib as L
    before = L.device_bytes_in_use()
    first = pkg.SgGraph(layout["source"], layout["target"], layout["weight"])
    second = pkg.SgGraph(layout["source"], layout["target"], layout["weight"])
    assert facts(first) == facts(second)
    for v in layout["requests"]:
        same_result(first.recommend(v, ALPHA, 0.0, 7), second.recommend(v, ALPHA, 0.0, 7), v)
    first.close()
    second.close()
    assert L.device_bytes_in_use() == before


def test_wrong_device_or_host_memory_is_refused(pkg):
    s = torch.tensor([1, 2], dtype=torch.int64)
    w = torch.tensor([1.0, 1.0], dtype=torch.float64)
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.SgGraph.from_device(s, s.flip(0).cuda(), w.cuda())        # a CPU tensor among CUDA tensors
    from locations_recommender_amd import _lib as L
    import ctypes as C
    h = C.c_void_p()
    a = np.array([1, 2], np.int64)
    p = C.c_void_p(a.ctypes.data)                                     # host memory behind the C entry point
    assert pkg.lib().locrec_sg_create_from_device(2, p, p, p, C.byref(h)) == L.E_INVALID_ARG and h.value is None


def test_empty_edge_list(pkg):
    empty = [np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)]
    host = pkg.SgGraph(*empty)
    device = pkg.SgGraph.from_device(dev(empty[0], np.int64), dev(empty[1], np.int64), dev(empty[2], np.float64))
    assert facts(host) == facts(device) and facts(device)["vertices"] == 0
    errors = []
    for g in (host, device):
        with pytest.raises(pkg.IllegalArgumentException) as e:
            g.recommend(1, ALPHA, 0.01, 20)
        errors.append(str(e.value))
        g.close()
    assert errors[0] == errors[1]


def test_graph_from_device_place_visits(pkg):
    """prep.sg_graph_from_visits with device columns (no host hop) against SgGraph over the same edge columns copied to
    the host."""
    prep = pkg.prep
    visits, places, visits_from = prep_cases.join_case(11, 400, 6000, "moscow")
    as_dev = lambda d: {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in d.items()}  # noqa: E731
    pv = prep.calc_place_visits(as_dev(visits), as_dev(places), visits_from)
    s, t, w = prep.generate_stochastic_graph(pv, 0.7, 0.3)
    assert s.is_cuda and len(s) > 1000
    device = prep.sg_graph_from_visits(pv, 0.7, 0.3)
    host = pkg.SgGraph(s.cpu().numpy(), t.cpu().numpy(), w.cpu().numpy())
    assert facts(host) == facts(device)
    person = int(pv["person_id"][0])
    for v in (person, int(pv["place_id"][0]), person):
        for eps, max_it in SETTINGS:
            same_result(host.recommend(v, ALPHA, eps, max_it), device.recommend(v, ALPHA, eps, max_it), (v, eps, max_it))
    host.close()
    device.close()
