"""Batched SG requests (locrec_sg_recommend_batch): many targets of ONE graph per sweep.

Every target of a batch must equal the single request on the same graph bit for bit - ids, probability bits, the
0-based iteration counter and the converged flag - whatever else shares its tile: persons (source-only, each with a
private row of x) next to places and categories, duplicates, targets that converge at different sweeps.  The handle
serves single requests exactly as before afterwards."""
import ctypes as C
import json
import os

import numpy as np
import pandas as pd
import pytest
from test_jni_shim import I, Jvm, shim  # noqa: F401  (the fake-JVM harness and its fixture)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-6
ALPHA = 0.15
TILE = 16  # targets per shared sweep (kBatchB in sg_batch.hip)


def kat():
    with open(os.path.join(GOLD, "sg_kats.json")) as f:
        return json.load(f)


def kat_edges(g):
    e = np.array(g["edges"], dtype=np.float64)
    return e[:, 0].astype(np.int64), e[:, 1].astype(np.int64), e[:, 2]


def rows_of(batch, i):
    off, ids, probs, its, conv = batch
    return ids[off[i]:off[i + 1]], probs[off[i]:off[i + 1]], int(its[i]), bool(conv[i])


def same_bits(a, b):
    """(ids, probs, iterations, converged) of two requests: identical, probabilities bit for bit."""
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and tuple(a[2:]) == tuple(b[2:])


def check_against_single(sg, targets, eps, max_it):
    batch = sg.recommend_batch(targets, ALPHA, eps, max_it)
    assert len(batch[0]) == len(targets) + 1 and batch[0][0] == 0
    for i, v in enumerate(targets):
        want = sg.recommend(int(v), ALPHA, eps, max_it)
        assert same_bits(rows_of(batch, i), want), (i, int(v), eps, max_it)
    return batch


def check_against_oracle(oracle, src, dst, w, batch, targets, eps, max_it, which):
    for i in which:
        oi, op, oit, oconv = oracle.sg_recommend(src, dst, w, int(targets[i]), ALPHA, eps, max_it)
        ids, probs, it, conv = rows_of(batch, i)
        assert np.array_equal(ids, oi), (i, int(targets[i]))
        if not (eps == 0 and (conv or oconv)):
            # (with epsilon 0 the loop ends at an exact fp64 fixed point, and the sweep that reaches it depends on the
            # order of the sums: the device's and the oracle's may be one apart; the batch still equals the single
            # request exactly, checked above)
            assert (it, conv) == (oit, oconv), (i, int(targets[i]))
        np.testing.assert_allclose(probs, op, rtol=RTOL, atol=0)


def mixed_targets(g, n_places, n_categories, seed, n=40):
    """About n targets: persons, places and categories, with duplicates, more than two tiles and not a multiple of
    the tile."""
    rng = np.random.default_rng(seed)
    person0 = int(g["first_person"])
    n_persons = int(g["source_id"].max()) - person0 + 1
    persons = person0 + rng.choice(n_persons, n // 2, replace=False)
    places = 40 + rng.choice(n_places, n // 4, replace=False)
    cats = rng.choice(n_categories, n // 8, replace=False)
    t = np.concatenate([persons, places, cats])
    t = np.concatenate([t, rng.choice(t, n - len(t))])  # duplicates
    rng.shuffle(t)
    assert len(np.unique(t)) > 2 * TILE and len(np.unique(t)) % TILE != 0
    return t.astype(np.int64)


def test_reference_kats(pkg):
    """StochasticRecommenderTest.scala:39-94's graph: targets [1, 1, 3, 5] at both parameter sets; target 1 gives the
    reference's expected lists exactly; an unknown vertex is refused before anything is written."""
    g = kat()
    src, dst, w = kat_edges(g)
    sg = pkg.SgGraph(src, dst, w)
    for case in g["cases"]:
        if "expected_error" in case:
            continue
        targets = [1, 1, 3, 5]
        batch = check_against_single(sg, targets, case["epsilon"], case["max_iterations"])
        want = sorted((tuple(x) for x in case["expected_sorted_by_probability_desc"]), key=lambda t: t[0])
        for i in (0, 1):
            ids, probs, _, _ = rows_of(batch, i)
            assert list(zip(ids.tolist(), probs.tolist())) == want, case["name"]
    from locations_recommender_amd import _lib as L
    off = np.full(5, -7, np.int64)
    ids, probs = np.full(64, -7, np.int64), np.full(64, -7.0)
    its, conv = np.full(4, -7, np.int64), np.full(4, -7, np.int32)
    cap = C.c_int64(64)
    v = np.array([1, 3, 100, 5], np.int64)
    with pytest.raises(pkg.IllegalArgumentException, match="No such vertex in the graph: 100"):
        L.check(L.lib().locrec_sg_recommend_batch(sg._h, 4, L.ptr(v, C.c_int64), ALPHA, 0.05, 1000, L.ptr(off, C.c_int64),
                                                  L.ptr(ids, C.c_int64), L.ptr(probs, C.c_double), C.byref(cap),
                                                  L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32)))
    assert (off == -7).all() and (ids == -7).all() and (probs == -7.0).all() and (its == -7).all() and (conv == -7).all()
    assert cap.value == 64
    sg.close()


@pytest.mark.parametrize("eps,max_it", [(0.01, 20), (0.0, 100), (0.01, 0), (1e-6, 200)])
def test_random_graph_matches_single_requests_and_oracle(pkg, oracle, eps, max_it):
    from locations_recommender_amd import synth
    g = synth.sg_dataset(n_persons=3_000, n_places=300, n_categories=20, seed=77)
    src, dst, w = g["source_id"], g["target_id"], g["balanced_weight"]
    targets = mixed_targets(g, 300, 20, seed=5)
    sg = pkg.SgGraph(src, dst, w)
    batch = check_against_single(sg, targets, eps, max_it)
    check_against_oracle(oracle, src, dst, w, batch, targets, eps, max_it, range(len(targets)))
    sg.close()


def d2_trajectory(src, dst, w, v, n):
    """isConverged's sum (:130-141) of sweeps 0 .. n-1 for target v, in numpy (float64, any summation order)."""
    vid, inv = np.unique(np.concatenate([src, dst]), return_inverse=True)
    cs, ct = inv[:len(src)], inv[len(src):]
    u = (vid == v).astype(np.float64)
    x = np.full(len(vid), 1.0 / len(vid))
    out = []
    for _ in range(n):
        xn = ALPHA * u + (1 - ALPHA) * np.bincount(ct, weights=x[cs] * w, minlength=len(vid))
        out.append(float(np.sum((xn - x) ** 2)))
        x = xn
    return np.array(out)


def test_targets_of_a_tile_stop_at_different_sweeps(pkg, oracle):
    """An epsilon between two targets' isConverged sums (found on the host, with a wide margin) makes the targets of
    one tile stop at different sweeps: finished columns must stay as they were while the others go on."""
    rng = np.random.default_rng(17)
    n = 400
    src = np.r_[rng.integers(1000, 1000 + n, 4000), rng.integers(0, 30, 600), 2000, 2001]
    dst = np.r_[rng.integers(0, 30, 4000), rng.integers(0, 30, 600), 2001, 2000]
    w = np.r_[rng.random(4600) / 30, 1.0, 1.0]
    # 2000 <-> 2001: a two-cycle of its own, where a target's mass swings back and forth far longer than in the rest
    slow, fast = 2000, 1000
    ds, df = d2_trajectory(src, dst, w, slow, 60), d2_trajectory(src, dst, w, fast, 60)
    k = next(i for i in range(60) if df[i] < ds[i] / 100)
    eps = float(np.sqrt(np.sqrt(df[k] * ds[k])))
    targets = np.r_[slow, fast, np.arange(1001, 1040), 5, 2001].astype(np.int64)
    sg = pkg.SgGraph(src, dst, w)
    batch = check_against_single(sg, targets, eps, 200)
    assert len(set(batch[3].tolist())) > 1 and batch[4].all()
    check_against_oracle(oracle, src, dst, w, batch, targets, eps, 200, range(0, len(targets), 4))
    sg.close()


def test_cfg3_full_size(pkg, oracle):
    from locations_recommender_amd import synth
    g = synth.sg_dataset()
    src, dst, w = g["source_id"], g["target_id"], g["balanced_weight"]
    targets = mixed_targets(g, 10_000, 20, seed=9)
    sg = pkg.SgGraph(src, dst, w)
    for eps, max_it in ((0.01, 20), (0.0, 100), (0.01, 0)):
        batch = check_against_single(sg, targets, eps, max_it)
        check_against_oracle(oracle, src, dst, w, batch, targets, eps, max_it, (0, 7) if max_it == 100 else range(6))
    sg.close()


def layout_variants_case(pkg, oracle, src, dst, w, targets, env=None, monkeypatch=None, expect_dict=None):
    if env:
        monkeypatch.setenv(env, "1")
    sg = pkg.SgGraph(src, dst, w)
    if env:
        monkeypatch.delenv(env)
    if expect_dict is not None:
        assert (sg.info()["weight_dictionary"] > 0) == expect_dict
    for eps, max_it in ((0.01, 20), (0.0, 60), (0.01, 0)):
        batch = check_against_single(sg, targets, eps, max_it)
        check_against_oracle(oracle, src, dst, w, batch, targets, eps, max_it, range(0, len(targets), 5))
    sg.close()


def test_fp64_weight_stream_form(pkg, oracle):
    """More distinct weights than the dictionary takes: the batched sweep streams the fp64 weights."""
    rng = np.random.default_rng(21)
    w = rng.random(20_000) / 40
    src = rng.integers(1000, 1300, 20_000).astype(np.int64)
    dst = rng.integers(0, 40, 20_000).astype(np.int64)
    targets = np.r_[rng.choice(np.arange(1000, 1300), 30, replace=False), np.arange(0, 40, 4), [1000, 1003, 0]]
    layout_variants_case(pkg, oracle, src, dst, w, targets.astype(np.int64), expect_dict=False)


@pytest.mark.parametrize("env", ["LOCREC_SG_NO_DICT", "LOCREC_SG_NO_COL16"])
def test_switches_set_before_create(pkg, oracle, monkeypatch, env):
    from locations_recommender_amd import synth
    g = synth.sg_dataset(n_persons=2_000, n_places=200, n_categories=10, seed=41)
    targets = mixed_targets(g, 200, 10, seed=3)
    layout_variants_case(pkg, oracle, g["source_id"], g["target_id"], g["balanced_weight"], targets, env=env,
                         monkeypatch=monkeypatch, expect_dict=None if env == "LOCREC_SG_NO_COL16" else False)


def test_uint16_columns_with_few_private_rows(pkg, oracle):
    """T + 1 + 16 > 65536 >= T + 2: uint16 columns still address every live vertex and D, but only five private rows
    per tile - the batch runs tiles of five."""
    T, n_persons = 65_530, 1_500
    live = np.arange(T, dtype=np.int64)
    persons = 100_000 + np.arange(n_persons, dtype=np.int64)
    src = np.concatenate([persons[live % n_persons], live, persons[:40]])
    dst = np.concatenate([live, (live * 7 + 1) % T, np.arange(40, dtype=np.int64)])
    outdeg = np.bincount(np.searchsorted(np.unique(src), src))
    w = 1.0 / outdeg[np.searchsorted(np.unique(src), src)]
    sg = pkg.SgGraph(src, dst, w)
    assert sg.live_count() == T
    targets = np.array([100_000, 5, 100_001, 100_002, 100_003, 100_004, 7, 100_005, 100_000, 65_529, 100_006, 100_039],
                       np.int64)
    for eps, max_it in ((0.01, 20), (0.0, 12)):
        batch = check_against_single(sg, targets, eps, max_it)
        check_against_oracle(oracle, src, dst, w, batch, targets, eps, max_it, (0, 1, 10))
    sg.close()


def test_handle_state_around_a_batch(pkg):
    """Single requests before and after a batch give a fresh handle's bits; the batch's rows do too."""
    from locations_recommender_amd import synth
    g = synth.sg_dataset(n_persons=2_500, n_places=250, n_categories=12, seed=8)
    src, dst, w = g["source_id"], g["target_id"], g["balanced_weight"]
    p0 = int(g["first_person"])
    v1, v2, v3 = p0 + 11, p0 + 12, 45
    others = np.r_[p0 + np.arange(20, 60), 40 + np.arange(10)]

    def fresh(v):
        h = pkg.SgGraph(src, dst, w)
        r = h.recommend(v, ALPHA, 0.01, 20)
        h.close()
        return r

    sg = pkg.SgGraph(src, dst, w)
    assert same_bits(sg.recommend(v1, ALPHA, 0.01, 20), fresh(v1))
    targets = np.r_[others[:7], v1, others[7:30], v2, others[30:]].astype(np.int64)
    batch = sg.recommend_batch(targets, ALPHA, 0.01, 20)
    assert same_bits(rows_of(batch, 7), fresh(v1))
    assert same_bits(rows_of(batch, 31), fresh(v2))
    assert same_bits(sg.recommend(v1, ALPHA, 0.01, 20), fresh(v1))
    assert same_bits(sg.recommend(v3, ALPHA, 0.01, 20), fresh(v3))
    assert same_bits(sg.recommend(v2, ALPHA, 0.01, 20), fresh(v2))
    batch2 = sg.recommend_batch(targets, ALPHA, 0.01, 20)  # a second batch after single requests: the same rows
    assert all(np.array_equal(a, b) for a, b in zip(batch, batch2))
    sg.close()


def test_capacity_protocol_empty_list_and_refusals(pkg):
    from locations_recommender_amd import _lib as L
    g = kat()
    src, dst, w = kat_edges(g)
    sg = pkg.SgGraph(src, dst, w)
    v = np.array([5, 1, 3, 1], np.int64)
    off, _, _, want_its, want_conv = batch = sg.recommend_batch(v, ALPHA, 0.05, 1000)
    total = int(off[-1])
    assert total > 2

    def call(targets, offsets, ids, probs, cap, its, conv):
        L.check(L.lib().locrec_sg_recommend_batch(sg._h, len(targets), L.ptr(targets, C.c_int64), ALPHA, 0.05, 1000,
                                                  L.ptr(offsets, C.c_int64), L.ptr(ids, C.c_int64), L.ptr(probs, C.c_double),
                                                  C.byref(cap), L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32)))

    off2 = np.full(5, -1, np.int64)
    ids, probs = np.full(2, -7, np.int64), np.full(2, -7.0)
    its, conv = np.full(4, -1, np.int64), np.full(4, -1, np.int32)
    cap = C.c_int64(2)
    call(v, off2, ids, probs, cap, its, conv)           # too little room: offsets and counters only
    assert cap.value == total and np.array_equal(off2, off)
    assert np.array_equal(its, want_its) and np.array_equal(conv.astype(bool), want_conv)
    assert (ids == -7).all() and (probs == -7.0).all()
    ids, probs = np.empty(total, np.int64), np.empty(total)
    cap = C.c_int64(total)
    call(v, off2, ids, probs, cap, its, conv)           # repeated with room: the rows
    assert cap.value == total and np.array_equal(ids, batch[1]) and probs.tobytes() == batch[2].tobytes()
    # counters may be NULL
    L.check(L.lib().locrec_sg_recommend_batch(sg._h, 4, L.ptr(v, C.c_int64), ALPHA, 0.05, 1000, L.ptr(off2, C.c_int64),
                                              L.ptr(ids, C.c_int64), L.ptr(probs, C.c_double), C.byref(cap), None, None))
    assert np.array_equal(ids, batch[1])
    # the empty list
    e_off, e_ids, e_probs, e_its, e_conv = sg.recommend_batch(np.empty(0, np.int64), ALPHA, 0.05, 1000)
    assert e_off.tolist() == [0] and len(e_ids) == len(e_probs) == len(e_its) == len(e_conv) == 0
    # the constructor's require()s
    with pytest.raises(pkg.IllegalArgumentException, match="epsilon must be non-negative"):
        sg.recommend_batch([1], ALPHA, -0.1, 10)
    with pytest.raises(pkg.IllegalArgumentException, match="max iterations number must be non-negative"):
        sg.recommend_batch([1], ALPHA, 0.1, -1)
    sg.close()
    # sharded handles (both forms) are refused
    for by_target in (False, True):
        sh = pkg.SgGraph(src, dst, w, shard_index=0, shard_count=2, by_target=by_target)
        with pytest.raises(pkg.IllegalArgumentException, match="sharded"):
            sh.recommend_batch([1, 3], ALPHA, 0.05, 1000)
        sh.close()


def test_experiment_handles(pkg, monkeypatch):
    """Handles of the fused experiment are refused; the grid-stride sweep switch is served (same bits)."""
    from locations_recommender_amd import synth
    g = synth.sg_dataset(n_persons=1_500, n_places=150, n_categories=8, seed=4)
    src, dst, w = g["source_id"], g["target_id"], g["balanced_weight"]
    monkeypatch.setenv("LOCREC_SG_FUSED", "1")
    sg = pkg.SgGraph(src, dst, w)
    monkeypatch.delenv("LOCREC_SG_FUSED")
    with pytest.raises(pkg.IllegalArgumentException, match="fused or persistent"):
        sg.recommend_batch([int(g["first_person"])], ALPHA, 0.01, 20)
    sg.close()
    monkeypatch.setenv("LOCREC_SG_GS", "4")
    sg = pkg.SgGraph(src, dst, w)
    monkeypatch.delenv("LOCREC_SG_GS")
    check_against_single(sg, mixed_targets(g, 150, 8, seed=2), 0.01, 20)
    sg.close()


def test_python_class(pkg, capsys):
    g = kat()
    src, dst, w = kat_edges(g)
    edges = pd.DataFrame({"source_id": src, "target_id": dst.astype(np.int32), "balanced_weight": w})
    for eps, max_it in ((0.05, 1000), (0.01, 1)):
        rec = pkg.StochasticRecommender(edges, epsilon=eps, maxIterations=max_it)
        capsys.readouterr()
        targets = [1, 1, 3, 5]
        singles = [rec.makeRecommendations(vertexId=v) for v in targets]
        single_out = capsys.readouterr().out
        df = rec.makeRecommendationsBatch(targets)
        assert capsys.readouterr().out == single_out
        assert list(df.columns) == ["vertex_id", "id", "probability"]
        assert len(df) == sum(len(s) for s in singles)
        at = 0
        for v, s in zip(targets, singles):
            part = df.iloc[at:at + len(s)]
            at += len(s)
            assert (part["vertex_id"] == v).all()
            assert part["id"].tolist() == s["id"].tolist()
            assert part["probability"].to_numpy().tobytes() == s["probability"].to_numpy().tobytes()
        with pytest.raises(pkg.IllegalArgumentException, match="No such vertex in the graph: 100"):
            rec.makeRecommendationsBatch([1, 100])
        quiet = pkg.StochasticRecommender(edges, epsilon=eps, maxIterations=max_it, quiet=True)
        capsys.readouterr()
        quiet.makeRecommendationsBatch(targets)
        assert capsys.readouterr().out == ""
        rec.close()
        quiet.close()


def test_jni_native_on_the_device(shim):
    """sgRecommendBatch through the fake-JVM harness: sized, then filled; rows and counters as sgRecommend's."""
    j = shim
    assert isinstance(j, Jvm)
    g = kat()
    src, dst, w = kat_edges(g)
    h = j.ok("sgCreate", C.c_int64, j.arr(src, np.int64), j.arr(dst, np.int64), j.arr(w, np.float64))
    nv = j.ok("sgVertexCount", C.c_int64, I(h))
    targets = [1, 1, 3, 5]
    for case in g["cases"]:
        if "expected_error" in case:
            off, ic = j.arr(n=3, dtype=np.int64), j.arr(n=4, dtype=np.int64)
            j.expect("IllegalArgumentException", "No such vertex in the graph: 100", "sgRecommendBatch", C.c_int64, I(h),
                     j.arr([1, 100], np.int64), ALPHA, float(case["epsilon"]), I(case["max_iterations"]), off, None, None, ic)
            continue
        eps, mx = float(case["epsilon"]), case["max_iterations"]
        off, ic = j.arr(n=5, dtype=np.int64), j.arr(n=8, dtype=np.int64)
        va = j.arr(targets, np.int64)
        need = j.ok("sgRecommendBatch", C.c_int64, I(h), va, ALPHA, eps, I(mx), off, None, None, ic)
        bi, bp = j.arr(n=need, dtype=np.int64), j.arr(n=need, dtype=np.float64)
        assert j.ok("sgRecommendBatch", C.c_int64, I(h), va, ALPHA, eps, I(mx), off, bi, bp, ic) == need
        o, counters = j.read(off), j.read(ic)
        assert o[0] == 0 and o[4] == need
        for t, v in enumerate(targets):
            gi, gp, sic = j.arr(n=nv, dtype=np.int64), j.arr(n=nv, dtype=np.float64), j.arr(n=2, dtype=np.int64)
            n = j.ok("sgRecommend", C.c_int64, I(h), I(v), ALPHA, eps, I(mx), gi, gp, sic)
            assert n == o[t + 1] - o[t]
            assert np.array_equal(j.read(bi)[o[t]:o[t + 1]], j.read(gi, n))
            assert j.read(bp)[o[t]:o[t + 1]].tobytes() == j.read(gp, n).tobytes()
            assert counters[2 * t:2 * t + 2].tolist() == j.read(sic).tolist()
    j.ok("sgDestroy", None, I(h))
