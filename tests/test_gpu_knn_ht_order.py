"""The head / tail image stores a row's elements in the order csrc/knn_ht_order.h chooses (different panel rows of the 16
lanes one LDS cycle serves on different slots), not in ascending order.  Integer dots are exact in any order, so nothing
a caller sees may change: ids, counts and similarity bits equal the oracle's and those of the same index built with
LOCREC_KNN_HT_ASCENDING=1 (the A/B switch), ratings are within 1e-6 of the oracle's, the host builder and the device
builder give the same image (the same answers and the same figures of locrec_knn_ht_lds_model), the modelled conflict
cycles never exceed the ascending image's, and the multiplied words and per-slice counts are those of the ascending image.

Data sets by hand, as in test_gpu_knn_ht_exact_counts.py (the head is exactly the hot places: LOCREC_KNN_HT_H), on the
seeding instantiation too: 63, 64, 65 and 130 persons (a partial last slice), a head of 32 places that every row crowds
into (two panel rows per slot), slices whose widest row runs the on-demand loops (17+ head places, 9+ categories), a wide
row's stand-in in the middle of a slice, and rows of up to 135 head places (every count range of the build kernel)."""
import numpy as np
import pytest

from test_gpu_knn import make_index
from test_gpu_knn_ht_exact_counts import dataset

pytestmark = pytest.mark.gpu

K = 10
PW, CW = 0.5, 0.5
RTOL = 1e-6
SEEDING = (("LOCREC_KNN_SEED_MIN_SLICES", "1"),)
HOST = (("LOCREC_KNN_HOST_BUILD", "1"),)
ASCENDING = (("LOCREC_KNN_HT_ASCENDING", "1"),)


def with_ratings(d):
    d = dict(d)
    d["r_rowptr"], d["r_place"] = d["p_rowptr"].copy(), d["p_idx"].astype(np.int64)
    d["r_rating"] = np.random.default_rng(3).integers(1, 6, size=len(d["p_idx"])).astype(np.int64)
    return d


def mixed_rows(n, hot, max_head, max_cat, seed):
    """(head places, tail places, categories) per person: head counts 0 .. max_head and category counts 1 .. max_cat,
    so that every slice has short rows (padding in front of the count) beside its widest."""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, min(hot, max_head) + 1)), 1 + i % 2, int(rng.integers(1, max_cat + 1))) for i in range(n)]


def small(n):
    d, _ = dataset(mixed_rows(n, 16, 9, 8, seed=n), hot=16, cold=300, c_dim=20, seed=100 + n)
    return with_ratings(d), 16


def crowded_head():
    """a head of 32 places of which a row holds up to 20: two panel rows per slot, and the 16 lanes of a group name
    both of them at most positions of the ascending order"""
    d, _ = dataset(mixed_rows(130, 32, 20, 6, seed=5), hot=32, cold=300, c_dim=12, seed=41)
    return with_ratings(d), 32


def long_rows():
    """head counts up to 135 of 160 hot places: sorted by their counts, the first slice ends between 32 and 128 (the
    build's largest LDS stage), the last beyond 128 (the build works in global memory)"""
    rows = mixed_rows(130, 160, 135, 6, seed=8)
    rows[5] = (135, 1, 5)
    d, _ = dataset(rows, hot=160, cold=300, c_dim=12, seed=43)
    return with_ratings(d), 160


def on_demand_loops():
    """widest rows of 17 .. 22 head places and 9 .. 13 categories: groups behind the rotating registers"""
    rows = mixed_rows(130, 48, 22, 13, seed=6)
    rows[7] = (22, 1, 13)
    rows[90] = (17, 2, 9)
    d, _ = dataset(rows, hot=48, cold=300, c_dim=16, seed=42)
    return with_ratings(d), 48


def wide_row_inside():
    """persons 20 and 100 hold a count of 300: kept out of the image, their lanes are stand-ins (all zero)"""
    d, h = small(130)
    v = d["p_val"].copy()
    for r in (20, 100):
        assert d["p_rowptr"][r + 1] > d["p_rowptr"][r]
        v[d["p_rowptr"][r]] = 300.0
    d["p_val"] = v
    return d, h


CASES = {"n63": lambda: small(63), "n64": lambda: small(64), "n65": lambda: small(65), "n130": lambda: small(130),
         "crowded_head": crowded_head, "on_demand_loops": on_demand_loops, "wide_row_inside": wide_row_inside,
         "long_rows": long_rows}
RATED = 6   # persons whose ratings are compared
_memo = {}


def case(name, oracle):
    """The data set and the oracle's answers, computed once."""
    if name not in _memo:
        d, h = CASES[name]()
        rows = np.arange(len(d["person_ids"]))
        sims = oracle.knn_similar_batch(d, rows, PW, CW, K, nthreads=8)
        step = max(1, len(rows) // RATED)
        rated = rows[::step][:RATED]
        recs = [oracle.knn_recommend(d, int(d["person_ids"][r]), PW, CW, K) for r in rated]
        _memo[name] = (d, h, sims, rated, recs)
    return _memo[name]


def build(pkg, monkeypatch, d, h, env, rated):
    """-> (ids, sims, counts), recommendations of `rated`, figures of the image"""
    env = (("LOCREC_KNN_HT_H", str(h)),) + env
    for name, value in env:
        monkeypatch.setenv(name, value)
    try:
        ix = make_index(pkg, d)
        out = ix.query_batch(d["person_ids"], PW, CW, K)
        assert ix.scan_plan()["kernel"] == 2, ix.scan_kernel_name()
        off, places, est = ix.recommend_batch(d["person_ids"][rated], PW, CW, K)
        recs = [(places[off[j]:off[j + 1]], est[off[j]:off[j + 1]]) for j in range(len(rated))]
        model = ix.ht_lds_model()
        figures = {"model": model, "stored": ix.ht_image_info()["head_words"], "multiplied": ix.ht_multiplied_words(),
                   "per_slice": ix.ht_slice_counts(), "wide": ix.ht_image_info()["wide_rows"]}
        ix.close()
    finally:
        for name, _ in env:
            monkeypatch.delenv(name)
    return out, recs, figures


@pytest.mark.parametrize("name", list(CASES))
def test_the_ordered_image_changes_no_answer(pkg, oracle, monkeypatch, name):
    d, h, (oi, os_, oc), rated, orecs = case(name, oracle)
    asc_out, _, asc = build(pkg, monkeypatch, d, h, ASCENDING, rated)
    built = {}
    for label, env in (("device", ()), ("device+seeding", SEEDING), ("host", HOST), ("host+seeding", HOST + SEEDING)):
        (ids, sims, cnt), recs, fig = build(pkg, monkeypatch, d, h, env, rated)
        built[label] = fig
        assert np.array_equal(cnt, oc), label
        assert np.array_equal(ids, oi), (label, "top-K ids differ from the oracle")
        assert np.array_equal(sims, os_), (label, "similarities are not bit-identical")
        assert all(np.array_equal(x, y) for x, y in zip((ids, sims, cnt), asc_out)), (label, "differs from the ascending image")
        for (places, est), (oplaces, oest) in zip(recs, orecs):
            assert np.array_equal(places, oplaces), label
            np.testing.assert_allclose(est, oest, rtol=RTOL, atol=0)
        # the same slices, the same words multiplied; no more modelled conflict cycles than the ascending order has
        assert fig["stored"] == asc["stored"] and fig["multiplied"] == asc["multiplied"], label
        assert np.array_equal(fig["per_slice"], asc["per_slice"]), label
        m, a = fig["model"], asc["model"]
        print(f"{name} {label}: group reads {m['group_reads']}, cycles {m['cycles']} (ascending {a['cycles']})")
        assert m["group_reads"] == a["group_reads"] == 4 * int(fig["per_slice"].sum()) > 0, label
        assert m["cycles"] - m["group_reads"] <= a["cycles"] - a["group_reads"], label
        assert m["cycles"] >= m["group_reads"]
    # host-built and device-built images: the same figures (the seeding pass reads the same image)
    assert built["device"]["model"] == built["host"]["model"] == built["device+seeding"]["model"] == built["host+seeding"]["model"]
    if name == "wide_row_inside":
        assert asc["wide"] == 2 and built["device"]["wide"] == 2
    m, a = built["device"]["model"], asc["model"]
    if name in ("crowded_head", "on_demand_loops", "long_rows"):
        assert m["cycles"] < a["cycles"], "several head places per slot: the order must remove conflict cycles here"
    if name == "long_rows":
        heads = built["device"]["per_slice"][:, 0]
        assert heads.max() > 128 and ((heads > 32) & (heads <= 128)).any(), heads.tolist()
    if name == "on_demand_loops":
        per_slice = built["device"]["per_slice"]
        assert per_slice[:, 0].max() >= 17 and per_slice[:, 1].max() >= 9, per_slice.tolist()


def test_the_switch_builds_the_ascending_image_in_both_builders(pkg, oracle, monkeypatch):
    """LOCREC_KNN_HT_ASCENDING=1: host and device builders agree on the ascending image's figures too, and the counts
    rounded up to four (LOCREC_KNN_HT_ROUND4) keep the ordered image's answers: the elements stay in front of the exact
    count, the words up to the rounded one are zero."""
    d, h, (oi, os_, oc), rated, _ = case("on_demand_loops", oracle)
    _, _, dev = build(pkg, monkeypatch, d, h, ASCENDING, rated)
    _, _, host = build(pkg, monkeypatch, d, h, ASCENDING + HOST, rated)
    assert dev["model"] == host["model"]
    round4 = (("LOCREC_KNN_HT_ROUND4", "1"),)
    figs = []
    for env in (round4, round4 + HOST):
        (ids, sims, cnt), _, fig = build(pkg, monkeypatch, d, h, env, rated)
        assert np.array_equal(cnt, oc) and np.array_equal(ids, oi) and np.array_equal(sims, os_), env
        figs.append(fig["model"])
    assert figs[0] == figs[1]
