"""The inputs of test_gpu_knn_limits.py checked against plain numpy and the oracle, so that a case cannot quietly miss
its limit: the planted sums of squares, dots and maxima are exactly the stated integers; every decisive pair is inside
the oracle's top K for the K the GPU test uses, and removing the decisive row changes the oracle's ids (the GPU test
would fail if a kernel lost it); for the small-weight cases EVERY sampled heavy query has one-family-only neighbours in
its top K, so a flushed f16 scale factor cannot go unnoticed."""
import numpy as np
import pytest

import knn_limit_cases as lc


def check_groups(oracle, case, pw=0.5, cw=0.5):
    d = case["d"]
    for g in case["groups"]:
        pid = int(d["person_ids"][g["query"]])
        ids, sims = oracle.knn_similar(d, pid, pw, cw, g["k"])
        cand_ids = d["person_ids"][g["cands"]]
        assert np.all(np.isin(cand_ids, ids)), (g["name"], "a decisive row is outside the oracle's top K")
        for c in g["cands"]:
            less = lc.without(d, [c])
            ids2, _ = oracle.knn_similar(less, pid, pw, cw, g["k"])
            assert not np.array_equal(ids, ids2), (g["name"], "removing the decisive row changes nothing")


def group(case, name):
    return next(g for g in case["groups"] if g["name"] == name)


def test_the_planted_integers():
    assert sum(v * v for v in lc.TWIN16) == lc.U16_MAX == 65535
    assert sum(v * v for v in lc.TWIN32) == lc.U32_MAX == 2 ** 32 - 1
    assert 4 * 128 * 128 == 65536
    with np.errstate(over="ignore"):
        f16 = np.array(lc.NEAR_DOTS, np.float64).astype(np.float16).astype(np.float64)
    assert f16.tolist() == [np.inf, np.inf, np.inf, 65504.0, 65504.0, 65504.0]          # the round-to-inf edge is 65520
    for t in lc.ROUND_DOWN_DOTS:
        lo = float(np.float16(t))
        ulp = float(np.nextafter(np.float16(lo), np.float16(np.inf))) - lo
        assert lo < t and t - lo >= ulp / 2 - 1, (t, lo, ulp)                                 # (almost) half an ulp lost
    for w in lc.SMALL_WEIGHTS:
        assert w + (1.0 - w) == 1.0 and 0 < w < 1 and 0 < 1.0 - w < 1                         # what check_params() asks
        assert w / 165.0 * 1.006 < 2.0 ** -14                                                 # f16-subnormal scale factor


@pytest.mark.parametrize("value", [255, 256])
def test_byte_case(oracle, value):
    case = lc.byte_case(value)
    d = case["d"]
    for g in case["groups"]:
        _, val = lc.vector(d, g["family"], g["query"])
        assert val.max() == value and g["ss_query"] == value * value + 9 and g["dots"] == [value * value + 9]
    assert (value == 255) == (g["ss_query"] < 65536)
    assert len(case["wide"]) == (0 if value == 255 else 4)
    assert {0, 2999, 1500} <= {g["query"] for g in case["groups"]}                           # first, last, middle
    assert not np.array_equal(d["person_ids"], np.sort(d["person_ids"]))
    check_groups(oracle, case)


def test_u16_case(oracle):
    case = lc.u16_case()
    d = case["d"]
    for fam in ("p", "c"):
        g = group(case, f"{fam} near twins")
        assert g["ss_query"] == 65535 and g["dots"] == list(lc.NEAR_DOTS) and max(g["ss_cands"]) == 65535
        g = group(case, f"{fam} ss 65536")
        assert g["ss_query"] == 65536 == g["dots"][0] and lc.vector(d, fam, g["query"])[1].max() == 128
        for t in lc.ROUND_DOWN_DOTS:
            g = group(case, f"{fam} dot {t} at the K-th rank")
            assert g["dots"] == [t] and g["ss_query"] < 65536 and g["ss_cands"][0] < 65536
            ids, _ = oracle.knn_similar(d, int(d["person_ids"][g["query"]]), 0.5, 0.5, g["k"])
            assert ids[g["k"] - 1] == d["person_ids"][g["cands"][0]], "the pair is not at the K-th rank"
    assert len(case["wide"]) == 4
    check_groups(oracle, case)


@pytest.mark.parametrize("mirror", [False, True])
def test_weights_case(oracle, mirror):
    case = lc.weights_case(mirror)
    d, fam = case["d"], case["tiny"]
    assert case["ks"] == (256, 500)
    assert len(case["wide"]) == 0 and len(case["heavy"]) == 1000 and {0, 2999} <= set(case["heavy"].tolist())
    for f in ("p", "c"):
        _, ss = lc.family_dots(d, f, 0)
        assert np.all(ss[case["heavy"]] > 164 ** 2) and ss.max() < 65536
    sample = case["heavy"][::17][:60]
    for w in lc.SMALL_WEIGHTS:
        pw, cw = (w, 1.0 - w) if fam == "p" else (1.0 - w, w)
        for k in case["ks"]:
            ids, sims, cnt = oracle.knn_similar_batch(d, sample, pw, cw, k, nthreads=8)
            have = [lc.one_family_neighbours(d, int(r), fam, ids[j][:cnt[j]]) for j, r in enumerate(sample)]
            assert min(have) > 0, (w, k, have)    # ALL sampled queries: a flushed factor drops rows the oracle keeps


@pytest.mark.parametrize("n,n_wide", [(4000, 256), (4000, 257), (200_000, 390), (200_000, 391), (200, 200), (200, 199),
                                      (2_100_000, 4096), (2_100_000, 4097)])
def test_cap_case(n, n_wide):
    case = lc.cap_case(n, n_wide)
    assert len(case["wide"]) == n_wide and case["wide"][0] == 0 and case["wide"][-1] == n - 1
    assert min(4096, max(256, 4000 // 512)) == 256 and min(4096, max(256, 200_000 // 512)) == 390
    assert min(4096, max(256, 2_100_000 // 512)) == 4096


@pytest.mark.parametrize("dim,value", [(65536, 2 ** 16 - 1), (65536, 2 ** 16), (65537, 2 ** 15 - 1), (65537, 2 ** 15),
                                       (2 ** 20 - 2, 2 ** 12 - 1), (2 ** 20 - 2, 2 ** 12), (2 ** 20 - 1, 1)])
def test_packed_case(oracle, dim, value):
    vbits = min(24, 32 - int(np.ceil(np.log2(dim))))
    assert value in (2 ** vbits - 1, 2 ** vbits, 1)
    case = lc.packed_case(p_dim=dim, value=value)
    d = case["d"]
    idx, val = lc.vector(d, "p", case["groups"][0]["query"])
    assert idx[-1] == dim - 1 == d["p_idx"].max() and val[-1] == value
    assert d["p_val"].max() == max(value, 9)
    check_groups(oracle, case)
    if dim == 65536:
        case = lc.packed_case(c_dim=dim, fam="c", value=value)
        assert case["d"]["c_idx"].max() == dim - 1 and case["d"]["c_val"].max() == value
        check_groups(oracle, case)


@pytest.mark.parametrize("kind,ss", [("max", 2 ** 32 - 1), ("over", 2 ** 32), ("big", 2 ** 52 + 9)])
def test_pack32_case(oracle, kind, ss):
    case = lc.pack32_case(kind)
    g = case["groups"][0]
    assert g["ss_query"] == ss and g["dots"] == [ss]
    check_groups(oracle, case)


@pytest.mark.parametrize("p_dim,c_dim", [(600, 64), (600, 65), (8192, 20), (8193, 20), (4096, 20), (4097, 20),
                                         (131008, 64), (131024, 64), (300, 20)])
def test_panel_case(oracle, p_dim, c_dim):
    case = lc.panel_case(p_dim, c_dim)
    d = case["d"]
    assert d["p_idx"].max() == p_dim - 1 and d["c_idx"].max() == c_dim - 1
    r16 = ((p_dim + 15) & ~15) + ((c_dim + 15) & ~15)        # the single request's byte tables
    if p_dim > 100_000:
        assert r16 == {131008: 131072, 131024: 131088}[p_dim]
    assert len(case["wide"]) == 0
    check_groups(oracle, case)


@pytest.mark.parametrize("length", [2 ** 21 - 1, 2 ** 21])
def test_long_row_case(length):
    case = lc.long_row_case(length)
    d = case["d"]
    r = case["long_row"]
    assert d["p_rowptr"][r + 1] - d["p_rowptr"][r] == length and d["p_dim"] >= 2 ** 21
    assert np.all(np.diff(d["p_idx"][d["p_rowptr"][r]:d["p_rowptr"][r + 1]]) == 1)
