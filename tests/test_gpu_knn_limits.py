"""KNN at the numeric limits that select an index's format, panel and kernel ("Numeric limits"; the inputs:
knn_limit_cases.py, checked on the CPU by test_knn_limit_cases.py).

Every case runs on BOTH builders (device, and LOCREC_KNN_HOST_BUILD=1: their info() must be equal) with the path
asserted first - info()["mode"] (0 GENERIC, 1 PACK32, 2 PACK16), scan_plan() kernel / mode, the number of wide rows -
so that a case cannot silently run another format.  Then query_batch, single query, recommend and recommend_batch
against the oracle: ids and similarities with np.array_equal, estimates at rtol = 1e-6 (BASELINE.json north star),
batch estimates bit-equal to the single request's; K below and above the LDS limit and K = n - 1; the boundary rows
as queries and as candidates; the switches that move the same data to the other consumers of the same limits; one
sharded request per family of cases.

The expected paths are written out from the limits' table as literals, not asked from the library."""
import numpy as np
import pytest

import knn_limit_cases as lc
from test_gpu_knn import RTOL, make_index, sharded_request

pytestmark = pytest.mark.gpu

SWITCHES = ("LOCREC_KNN_NO_HT", "LOCREC_KNN_NO_FAST", "LOCREC_KNN_NO_SINGLE", "LOCREC_KNN_NO_DIRECT8", "LOCREC_KNN_FORCE_HASH",
            "LOCREC_KNN_SEED_MIN_SLICES", "LOCREC_KNN_NO_ROW_FALLBACK", "LOCREC_KNN_NO_PACK16")
NO_FALLBACK = ("LOCREC_KNN_NO_HT", "LOCREC_KNN_NO_ROW_FALLBACK", "LOCREC_KNN_NO_PACK16")   # the fallback needs all three forms
KS = (50, 500, 1024, 1025)     # 1024: the largest K of the LDS lists; 1025: the tiled top-K of knn_large.hip


def expected_path(switch, wide=0, c_dim=20, packable=True, packed_dims=True, kernel=2):
    """What the limits' table says an index of this data is, under `switch`:
    wide > 0 rows (at most min(4096, max(256, n / 512)), fewer than n, c_dim <= 64, place dimension packable) stay out
    of a head / tail index; otherwise they demote everybody to PACK32 - or to GENERIC when a value does not fit the
    32-bit element (packable=False).  Legal data is PACK16: head / tail scan for c_dim <= 64, row scan otherwise."""
    if not packed_dims:
        return {"mode": 0, "kernel": 1, "plan": 0, "wide": 0}
    if wide and switch not in NO_FALLBACK and c_dim <= 64:
        return {"mode": 2, "kernel": kernel, "plan": 3, "wide": wide}
    if wide:
        mode = 1 if packable else 0
        return {"mode": mode, "kernel": 1, "plan": mode, "wide": 0}
    if switch == "LOCREC_KNN_NO_PACK16":
        return {"mode": 1, "kernel": 1, "plan": 1, "wide": 0}
    if switch == "LOCREC_KNN_NO_HT" or c_dim > 64:
        return {"mode": 2, "kernel": 1, "plan": 2, "wide": 0}
    return {"mode": 2, "kernel": kernel, "plan": 3, "wide": 0}


class Oracle:
    """The oracle's answers of one case, computed once and shared by every builder and switch."""

    def __init__(self, oracle, d, rows):
        self.o, self.d, self.rows, self.memo = oracle, d, np.asarray(rows), {}

    def batch(self, pw, cw, k):
        key = (pw, cw, k)
        if key not in self.memo:
            self.memo[key] = self.o.knn_similar_batch(self.d, self.rows, pw, cw, k, nthreads=8)
        return self.memo[key]

    def recommend(self, row, pw, cw, k):
        key = ("r", row, pw, cw, k)
        if key not in self.memo:
            self.memo[key] = self.o.knn_recommend(self.d, int(self.d["person_ids"][row]), pw, cw, k)
        return self.memo[key]


def check_index(ix, ref, want, ks, pw, cw, singles, full, legal_row=None):
    d, rows = ref.d, ref.rows
    pids = d["person_ids"][rows]
    assert ix.info()["mode"] == want["mode"] and ix.ht_image_info()["wide_rows"] == want["wide"], (ix.info(), ix.ht_image_info(), want)
    if legal_row is not None:      # the plan of a tiled batch: a wide query would send the batch down the dense path
        ix.query_batch(d["person_ids"][legal_row], pw, cw, ks[0])
        plan = ix.scan_plan()
        assert (plan["kernel"], plan["mode"]) == (want["kernel"], want["plan"]), (ix.scan_kernel_name(), want)
    for k in ks:
        oi, os_, oc = ref.batch(pw, cw, k)
        ids, sims, cnt = ix.query_batch(pids, pw, cw, k)
        assert np.array_equal(cnt, oc), k
        assert np.array_equal(ids, oi), f"K = {k}: top-K ids differ from the oracle"
        assert np.array_equal(sims, os_), f"K = {k}: similarities are not bit-identical"
    k = ks[0]
    oi, os_, oc = ref.batch(pw, cw, k)
    for j in singles:
        a, b = ix.query(int(pids[j]), pw, cw, k)
        assert np.array_equal(a, oi[j][:oc[j]]) and np.array_equal(b, os_[j][:oc[j]]), (int(rows[j]), k)
    if not full:
        return
    for k in (ks[0], ks[-1]):
        off, places, est = ix.recommend_batch(pids, pw, cw, k)
        for j in singles[:4]:
            oplaces, oest = ref.recommend(int(rows[j]), pw, cw, k)
            assert np.array_equal(places[off[j]:off[j + 1]], oplaces), (int(rows[j]), k)
            np.testing.assert_allclose(est[off[j]:off[j + 1]], oest, rtol=RTOL, atol=0)
            p1, e1 = ix.recommend(int(pids[j]), pw, cw, k)
            assert np.array_equal(p1, oplaces)
            np.testing.assert_allclose(e1, oest, rtol=RTOL, atol=0)
            assert np.array_equal(e1, est[off[j]:off[j + 1]]), "batched estimates differ from the single request's bits"


def query_rows(case, extra=12):
    d = case["d"]
    n = len(d["person_ids"])
    planted = [r for g in case["groups"] for r in [g["query"]] + g["cands"]]
    rows = list(dict.fromkeys(planted + case["wide"][:6].tolist() + list(range(3, n, max(1, n // extra)))))
    return np.array(rows), list(range(min(len(rows), max(8, len(planted)))))


def run_case(pkg, oracle, monkeypatch, case, want_of, switches=SWITCHES, ks=None, pw=0.5, cw=0.5, shard_rows=(), rows=None,
             singles=None, env=()):
    """Both builders under the default environment (everything) and under every switch (batch + singles)."""
    d = case["d"]
    n = len(d["person_ids"])
    if rows is None:
        rows, singles = query_rows(case)
    ks = tuple(ks or KS + (n - 1,))
    group_ks = tuple(sorted({g["k"] for g in case["groups"]} - set(ks)))
    ref = Oracle(oracle, d, rows)
    legal = np.array([int(r) for r in rows if r not in set(case["wide"].tolist())][:8])
    legal = legal if len(legal) > 1 else None       # (one query alone is a single request: no tiled scan to ask about)
    for name, value in env:
        monkeypatch.setenv(name, value)
    for switch in ("",) + tuple(switches):
        if switch:
            monkeypatch.setenv(switch, "1")
        infos = []
        for host in (False, True):
            if host:
                monkeypatch.setenv("LOCREC_KNN_HOST_BUILD", "1")
            ix = make_index(pkg, d)
            monkeypatch.delenv("LOCREC_KNN_HOST_BUILD", raising=False)
            want = want_of(switch)
            check_index(ix, ref, want, (ks if not switch else (ks[0], 1025)) + (group_ks if not switch else ()), pw, cw, singles,
                        full=not switch, legal_row=legal)
            if not switch and not host:
                for r in shard_rows:
                    pid = int(d["person_ids"][r])
                    ids, sims = sharded_request(pkg, ix, pid, pw, cw, 50, 4)
                    oa, ob = oracle.knn_similar(d, pid, pw, cw, 50)
                    assert np.array_equal(ids, oa) and np.array_equal(sims, ob), r
            infos.append(ix.info())
            ix.close()
        assert infos[0] == infos[1], f"the two builders disagree under {switch or 'the default environment'}: {infos}"
        if switch:
            monkeypatch.delenv(switch)
    for name, _ in env:
        monkeypatch.delenv(name)


# ---- value < 256: the head / tail element's byte -----------------------------------------------------------------------

@pytest.mark.parametrize("value", [255, 256])
def test_counts_of_255_and_256(pkg, oracle, monkeypatch, value):
    """255 is the largest count a head / tail element holds; 256 makes a row wide (4 planted rows: twins in each family).
    Bites: `vmax >= 256.0` read as `> 256.0` keeps the 256s in the image, where `v << 16` carries into the next field
    (the twins' dot 65545 becomes 9); read as `>= 255.0` the first case reports 4 wide rows."""
    case = lc.byte_case(value)
    wide = 0 if value == 255 else 4
    assert len(case["wide"]) == wide
    g = case["groups"]
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw, wide=wide), shard_rows=(g[0]["query"], 7))


# ---- sums of squares < 65536: the u16 accumulators, the f16 conversion of a dot -------------------------------------------

def test_u16_accumulator_and_f16_edges(pkg, oracle, monkeypatch):
    """Twins with ss = 65535 (dot 65535 = the u16 maximum), dots 65504 .. 65534 around the f16 round-to-inf edge 65520,
    ss = 65536 from counts of 128 (wide by the sum alone), dots that lose half an f16 ulp at the query's K-th rank.
    Bites: `ss >= 65536.0` read as `> 65536.0` puts the 128s into PACK16, whose dot 65536 wraps to 0 (the twin drops out
    of the top K; its ss packs as 0 = "no row"); a bound converted to f16 round-to-nearest instead of upwards is below the
    exact similarity for the dots 2049 .. 32783, and the pair at the K-th rank (k = rank + 1) is pruned."""
    case = lc.u16_case()
    assert len(case["wide"]) == 4
    g = case["groups"]
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw, wide=4), shard_rows=(g[0]["query"], g[1]["query"]))


# ---- the query's f16 scale factor: subnormal and below ----------------------------------------------------------------------

@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("w", lc.SMALL_WEIGHTS)
def test_heavy_norms_and_small_weights(pkg, oracle, monkeypatch, mirror, w):
    """placeWeight 0.01 and a place norm above 164 make w / norm * 1.006 an f16 SUBNORMAL (2^-10 .. 2^-53: smaller
    still).  K = 256 runs the head / tail scan (asserted), K = 500 the row scan.  Bites: a flushed (or rounded-to-zero)
    factor makes the tiny family's part of the bound 0, and the one-family-only neighbours that every sampled query has
    in its top K (test_knn_limit_cases.py) are pruned."""
    case = lc.weights_case(mirror)
    pw, cw = (w, 1.0 - w) if case["tiny"] == "p" else (1.0 - w, w)
    assert pw + cw == 1.0
    rows = case["heavy"][::17][:60]
    rows = np.r_[rows, [1, 2, 1499]]                       # light queries against heavy candidates as well
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw), switches=("LOCREC_KNN_SEED_MIN_SLICES", "LOCREC_KNN_NO_FAST"),
             ks=case["ks"], pw=pw, cw=cw, rows=rows, singles=[0, 1, 59, 60], shard_rows=(int(rows[0]),) if w == 0.01 else ())


# ---- wide rows <= min(4096, max(256, n / 512)) and < n ------------------------------------------------------------------------

@pytest.mark.parametrize("n,n_wide,kept", [(4000, 256, True), (4000, 257, False), (200_000, 390, True), (200_000, 391, False),
                                           (200, 200, False), (200, 199, True)])
def test_wide_row_cap(pkg, oracle, monkeypatch, n, n_wide, kept):
    """At the cap the wide rows stay out of a head / tail index; one more demotes the index to PACK32.  Bites: `<= cap`
    read as `< cap`, 512 as 511, 256 as 255 or `n_wide < n` as `<=` each flip `kept` for one of these sizes."""
    case = lc.cap_case(n, n_wide)
    legal = np.setdiff1d(np.arange(0, n, max(1, n // 9)), case["wide"])[:6]
    if n == 200:
        legal = np.setdiff1d(np.arange(n), case["wide"])[:1]
    rows = np.r_[legal, case["wide"][[0, n_wide // 2, -1]]].astype(np.int64)
    ks = (50, 1025) if n > 10_000 else (50, 1025, n - 1) if n > 1025 else (50, n - 1)
    demoted = {"mode": 1, "kernel": 1, "plan": 1, "wide": 0}        # a count of 256 still fits PACK32's element
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw, wide=n_wide) if kept else demoted,
             switches=("LOCREC_KNN_NO_ROW_FALLBACK",), ks=ks, rows=rows, singles=list(range(len(rows))),
             shard_rows=(int(case["wide"][0]),) if n == 4000 else ())


def test_wide_row_cap_at_4096(pkg, oracle, monkeypatch):
    """n = 2,100,000: n / 512 = 4101, the cap is 4096.  Sampled queries only (oracle single requests)."""
    for n_wide, kept in ((4096, True), (4097, False)):
        case = lc.cap_case(2_100_000, n_wide)
        d = case["d"]
        rows = np.array([5, 1_050_001, int(case["wide"][1]), int(case["wide"][-1])])
        infos = []
        for host in (False, True):
            if host:
                monkeypatch.setenv("LOCREC_KNN_HOST_BUILD", "1")
            ix = make_index(pkg, d)
            monkeypatch.delenv("LOCREC_KNN_HOST_BUILD", raising=False)
            want = expected_path("", wide=n_wide) if kept else {"mode": 1, "kernel": 1, "plan": 1, "wide": 0}
            assert ix.info()["mode"] == want["mode"] and ix.ht_image_info()["wide_rows"] == want["wide"]
            ids, sims, cnt = ix.query_batch(d["person_ids"][rows], 0.5, 0.5, 50)
            if not host:
                for j, r in enumerate(rows):
                    oa, ob = oracle.knn_similar(d, int(d["person_ids"][r]), 0.5, 0.5, 50)
                    assert np.array_equal(ids[j][:cnt[j]], oa) and np.array_equal(sims[j][:cnt[j]], ob), (n_wide, int(r))
                first = ids, sims, cnt
            else:
                assert all(np.array_equal(a, b) for a, b in zip(first, (ids, sims, cnt)))
            infos.append(ix.info())
            ix.close()
        assert infos[0] == infos[1]


# ---- index and value share one 32-bit element --------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,value,packable", [(65536, 2 ** 16 - 1, True), (65536, 2 ** 16, False), (65537, 2 ** 15 - 1, True),
                                                (65537, 2 ** 15, False), (2 ** 20 - 2, 2 ** 12 - 1, True), (2 ** 20 - 2, 2 ** 12, False)])
def test_packed_element_split(pkg, oracle, monkeypatch, dim, value, packable):
    """vbits = min(24, 32 - ceil_log2(dim)): 16, 15, 12 bits for these dimensions; 2^vbits - 1 at the largest index is
    the largest element PACK32 holds (reached with the fallback off), 2^vbits is GENERIC.  Bites: `pvmax < 2^vbits` read
    as `<=` ORs the value's top bit into the index field (index dim - 1 is all ones: the bit is lost, the twins' dot drops
    by value^2); a ceil_log2 that is one short at 65537 does the same at 2^15."""
    case = lc.packed_case(p_dim=dim, value=value)
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw, wide=2, packable=packable),
             switches=("LOCREC_KNN_NO_ROW_FALLBACK", "LOCREC_KNN_NO_PACK16", "LOCREC_KNN_FORCE_HASH"), ks=(50, 1025, 1999),
             shard_rows=(case["groups"][0]["query"],) if dim == 65536 else ())


@pytest.mark.parametrize("value,packable", [(2 ** 16 - 1, True), (2 ** 16, False)])
def test_packed_element_split_of_the_category_family(pkg, oracle, monkeypatch, value, packable):
    """c_dim = 65536 (> 64: no head / tail form, so no fallback): the twins' 65535 is PACK32 by itself."""
    case = lc.packed_case(c_dim=65536, fam="c", value=value)
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw, wide=2, c_dim=65536, packable=packable),
             switches=("LOCREC_KNN_NO_PACK16",), ks=(50, 1025, 1999))


@pytest.mark.parametrize("value", [1, 256])
def test_place_dimension_no_packed_format_holds(pkg, oracle, monkeypatch, value):
    """p_dim = 2^20 - 1 is GENERIC whatever the values; with a count of 256 the twins are wide BY THEMSELVES, but a
    GENERIC image keeps every row, so they must not be listed as wide rows (the side kernels would add them a second time)."""
    case = lc.packed_case(p_dim=2 ** 20 - 1, value=value)
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw, packed_dims=False),
             switches=("LOCREC_KNN_NO_ROW_FALLBACK", "LOCREC_KNN_NO_SINGLE"), ks=(50, 1025, 1999))


@pytest.mark.parametrize("kind,packable", [("max", True), ("over", False), ("big", False)])
def test_pack32_accumulator(pkg, oracle, monkeypatch, kind, packable):
    """ss = 2^32 - 1: the twins' dot is the u32 maximum (PACK32 with the fallback off); ss = 2^32 and a count of 2^26 are
    GENERIC.  Bites: `pss < 4294967296.0` read as `<=` wraps the "over" twins' dot to 0."""
    case = lc.pack32_case(kind)
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw, wide=2, packable=packable),
             switches=("LOCREC_KNN_NO_ROW_FALLBACK", "LOCREC_KNN_NO_PACK16", "LOCREC_KNN_NO_FAST", "LOCREC_KNN_NO_SINGLE"),
             ks=(50, 1025, 1999), shard_rows=(case["groups"][0]["query"],) if kind == "max" else ())


# ---- panels and tables ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p_dim,c_dim", [(600, 64), (600, 65), (8192, 20), (8193, 20), (4096, 20), (4097, 20), (131008, 64),
                                         (131024, 64), (300, 20)])
def test_panel_and_table_limits(pkg, oracle, monkeypatch, p_dim, c_dim):
    """c_dim 64 / 65: the category panel's rows (head / tail scan or row scan); 2 * p_dim = 16384 bytes: direct or hashed
    panel of the row scan (LOCREC_KNN_NO_HT); 4096: the popular-dimension table; 131072 / 131088 bytes: the single request's
    byte tables; p_dim below the default head.  The last index of each family is in use.  Bites: `c_dim <= 64` read as
    `<= 65` writes category index 64 into the place plane's first row; `<= kDirectMaxBytes` read as `<` or a table one
    entry short loses the twins' last index."""
    case = lc.panel_case(p_dim, c_dim)
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw, c_dim=c_dim),
             switches=("LOCREC_KNN_NO_HT", "LOCREC_KNN_FORCE_HASH", "LOCREC_KNN_NO_DIRECT8", "LOCREC_KNN_NO_SINGLE", "LOCREC_KNN_NO_PACK16"),
             ks=(50, 1025, 1999), shard_rows=(case["groups"][0]["query"],) if p_dim == 131008 else ())


def test_head_width_request_above_the_clamp(pkg, oracle, monkeypatch):
    """LOCREC_KNN_HT_H=4096 asks for a head of 4096 dimensions; the element's 16-bit offset field holds 65536 / (2 * 16)
    = 2048 rows.  (kernel 3: a head above the default runs knn_scan in head / tail mode.)  Bites: without the clamp the
    offsets of head dimensions 2048 .. 4095 wrap onto rows 0 .. 2047."""
    case = lc.panel_case(8192, 20)
    run_case(pkg, oracle, monkeypatch, case, lambda sw: expected_path(sw, kernel=3), switches=("LOCREC_KNN_SEED_MIN_SLICES",),
             ks=(50, 1025), env=(("LOCREC_KNN_HT_H", "4096"),))


# ---- row length < 2^21 -----------------------------------------------------------------------------------------------------------

def test_row_of_2_21_entries_is_refused_by_both_builders(pkg, monkeypatch):
    """Bites: `>= (1 << 21)` read as `>` in either builder lets the row through (the device build's row-order key has 21
    bits per count: 2^21 carries into the next field); a builder without the check builds an index instead of raising."""
    case = lc.long_row_case(2 ** 21)
    pid = int(case["d"]["person_ids"][case["long_row"]])
    for host in (False, True):
        if host:
            monkeypatch.setenv("LOCREC_KNN_HOST_BUILD", "1")
        with pytest.raises(pkg.IllegalArgumentException, match=rf"place vector of person {pid} has 2\^21 or more entries"):
            make_index(pkg, case["d"])


def test_row_of_2_21_minus_1_entries_is_accepted(pkg, oracle, monkeypatch):
    """p_dim above 2^21 is GENERIC; the long row (ss = 2^21 - 1: wide by its sum) must not be listed as a wide row.  A few
    ordinary queries; the long row is a candidate of each."""
    case = lc.long_row_case(2 ** 21 - 1)
    d = case["d"]
    assert case["wide"].tolist() == [case["long_row"]]
    rows = np.array([0, 125, 299, 77])
    oi, os_, oc = oracle.knn_similar_batch(d, rows, 0.5, 0.5, 50, nthreads=8)
    assert d["person_ids"][case["long_row"]] in oi
    infos = []
    for host in (False, True):
        if host:
            monkeypatch.setenv("LOCREC_KNN_HOST_BUILD", "1")
        ix = make_index(pkg, d)
        assert ix.info()["mode"] == 0 and ix.ht_image_info()["wide_rows"] == 0
        ids, sims, cnt = ix.query_batch(d["person_ids"][rows], 0.5, 0.5, 50)
        assert np.array_equal(cnt, oc) and np.array_equal(ids, oi) and np.array_equal(sims, os_)
        for j in (1, 3):
            a, b = ix.query(int(d["person_ids"][rows[j]]), 0.5, 0.5, 50)
            assert np.array_equal(a, oi[j][:oc[j]]) and np.array_equal(b, os_[j][:oc[j]])
        infos.append(ix.info())
        ix.close()
    assert infos[0] == infos[1]
