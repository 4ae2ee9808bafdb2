"""Seeded KNN inputs that stand exactly ON the numeric limits which select an index's format, panel and kernel
("Numeric limits"), shared by the CPU checks of the cases themselves (test_knn_limit_cases.py) and the GPU
tests (test_gpu_knn_limits.py).  No GPU and no package import: plain numpy.

Every case is a few thousand ordinary rows (so each format's normal machinery runs) with the boundary rows planted at
the first, the last and a middle input position, person ids shuffled, ratings attached.  A case is a dict

    d        the usual dataset dict (person_ids, p_* / c_* CSR, p_dim, c_dim, r_* ratings)
    groups   [{"name", "family", "query": row, "cands": [rows], "dots": [ints], "ss_query": int, "ss_cands": [ints], "k": K}]
             `cands` must be inside the oracle's top K of `query`; their integer dots / sums of squares in `family`
             are the stated integers
    wide     the input rows that are "wide" by themselves (a count >= 256 or a sum of squares >= 65536)

The limits are written here as literals on purpose: a test that asks the library where its limit lies cannot catch a
moved limit."""
import numpy as np

BYTE_MAX = 255            # head / tail element: one byte per count
U16_MAX = 65535           # v_pk_mad_u16 accumulators, ss packed as two u16
F16_MAX = 65504           # largest finite f16; 65520 and above round to +inf
U32_MAX = 4294967295
TWIN16 = (255, 22, 5, 1)            # sum of squares 65535
TWIN32 = (65535, 362, 5, 1)         # sum of squares 2^32 - 1
NEAR_DOTS = (65535, 65534, 65520, 65519, 65505, 65504)
ROUND_DOWN_DOTS = (2049, 4097, 8195, 16391, 32783)   # u16 -> f16 loses (almost) half an ulp, downwards
SMALL_WEIGHTS = (0.01, 2.0 ** -10, 2.0 ** -20, 2.0 ** -53)


# ---- building blocks ------------------------------------------------------------------------------------------------

def ragged(rng, n, dim, kmin, kmax, vmax, skew=1.0, span=None):
    """CSR of n rows with kmin .. kmax distinct indices each (before duplicates collapse) drawn from [0, span) with a
    popularity skew (small indices are popular), integer counts 1 .. vmax."""
    span = dim if span is None else span
    lens = rng.integers(kmin, kmax + 1, n)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    idx = np.minimum((span * rng.random(len(rows)) ** skew).astype(np.int64), span - 1)
    keys = np.unique(rows * dim + idx)
    rows, idx = keys // dim, keys % dim
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, idx.astype(np.int32), rng.integers(1, vmax + 1, len(keys)).astype(np.float64)


def base(seed, n=3000, p_dim=600, c_dim=20, p_span=None, c_span=None, places=(1, 30), cats=(1, 4), skew=2.5, c_skew=1.0):
    rng = np.random.default_rng(seed)
    prp, pidx, pval = ragged(rng, n, p_dim, places[0], places[1], 9, skew, p_span)
    crp, cidx, cval = ragged(rng, n, c_dim, cats[0], cats[1], 9, c_skew, c_span)
    return {"person_ids": rng.permutation(np.arange(10_000, 10_000 + n)).astype(np.int64),
            "p_rowptr": prp, "p_idx": pidx, "p_val": pval, "p_dim": int(p_dim),
            "c_rowptr": crp, "c_idx": cidx, "c_val": cval, "c_dim": int(c_dim)}


def vector(d, fam, row):
    rp = d[fam + "_rowptr"]
    return d[fam + "_idx"][rp[row]:rp[row + 1]].copy(), d[fam + "_val"][rp[row]:rp[row + 1]].copy()


def plant(d, fam, vectors):
    """Replace the `fam` vectors of the rows in `vectors` ({row: (indices, values)}), in place."""
    n = len(d["person_ids"])
    rp = d[fam + "_rowptr"]
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    keep = ~np.isin(row_of, np.fromiter(vectors.keys(), np.int64, len(vectors)))
    rows = [row_of[keep]] + [np.full(len(v[0]), r, np.int64) for r, v in vectors.items()]
    idx = [d[fam + "_idx"][keep].astype(np.int64)] + [np.asarray(v[0], np.int64) for v in vectors.values()]
    val = [d[fam + "_val"][keep]] + [np.asarray(v[1], np.float64) for v in vectors.values()]
    rows, idx, val = np.concatenate(rows), np.concatenate(idx), np.concatenate(val)
    big = int(d[fam + "_dim"]) + 1
    order = np.argsort(rows * big + idx, kind="stable")
    assert len(np.unique(rows * big + idx)) == len(rows), "a planted vector repeats an index"
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    d[fam + "_rowptr"], d[fam + "_idx"], d[fam + "_val"] = rowptr, idx[order].astype(np.int32), val[order]


def finish(d, seed=3):
    """Ratings as tests' with_ratings() attaches them: one rating 1 .. 5 per visited place."""
    rng = np.random.default_rng(seed)
    d["r_rowptr"], d["r_place"] = d["p_rowptr"].copy(), d["p_idx"].astype(np.int64)
    d["r_rating"] = rng.integers(1, 6, size=len(d["p_idx"])).astype(np.int64)
    return d


def slots(n):
    """Input positions for planted rows: the first, the last, a middle one, then their neighbours."""
    k = 0
    while True:
        yield k
        yield n - 1 - k
        yield n // 2 + k
        k += 1


def without(d, rows):
    """The dataset with the listed input rows removed."""
    n = len(d["person_ids"])
    keep_row = np.ones(n, bool)
    keep_row[np.asarray(rows)] = False
    out = {"person_ids": d["person_ids"][keep_row], "p_dim": d["p_dim"], "c_dim": d["c_dim"]}
    for fam in ("p", "c", "r"):
        rp = d[fam + "_rowptr"]
        keep = np.repeat(keep_row, np.diff(rp))
        out[fam + "_rowptr"] = np.concatenate([[0], np.cumsum(np.diff(rp)[keep_row])]).astype(np.int64)
        for col in (("idx", "val") if fam != "r" else ("place", "rating")):
            out[fam + "_" + col] = d[fam + "_" + col][keep]
    return out


def family_dots(d, fam, row):
    """Exact integer dot of `row` with every row in one family (int64), and every row's sum of squares."""
    n, dim = len(d["person_ids"]), int(d[fam + "_dim"])
    rp, idx, val = d[fam + "_rowptr"], d[fam + "_idx"], d[fam + "_val"].astype(np.int64)
    q = np.zeros(dim, np.int64)
    q[idx[rp[row]:rp[row + 1]]] = val[rp[row]:rp[row + 1]]
    row_of = np.repeat(np.arange(n), np.diff(rp))
    # (object arithmetic would be exact beyond 2^63; these cases stay below 2^33 per term and 2^34 per row)
    dots = np.zeros(n, np.int64)
    np.add.at(dots, row_of, val * q[idx])
    ss = np.zeros(n, np.int64)
    np.add.at(ss, row_of, val * val)
    return dots, ss


def similarities(d, row, pw, cw):
    """KnnRecommender.scala:27-49 in numpy for ONE query: similarity to every row (0 where no family matches; the
    query itself is -1).  Used to place a pair at a query's K-th rank; the oracle stays the judge."""
    sim = np.zeros(len(d["person_ids"]))
    for fam, w in (("p", pw), ("c", cw)):
        dots, ss = family_dots(d, fam, row)
        with np.errstate(divide="ignore", invalid="ignore"):
            cos = dots / (np.sqrt(ss.astype(np.float64)) * np.sqrt(float(ss[row])))
        sim += np.where(dots > 0, cos, 0.0) * w
    sim[row] = -1.0
    return sim


def rank_of(d, query, cand, pw=0.5, cw=0.5):
    """0-based position of `cand` in `query`'s neighbour list (similarity desc, person id asc)."""
    sim = similarities(d, query, pw, cw)
    ids = d["person_ids"]
    return int(np.sum((sim > sim[cand]) | ((sim == sim[cand]) & (ids < ids[cand]))))


def _solve(query_vals, target, ss_max):
    """Counts b (0 = index absent) with sum(query_vals * b) == target and sum(b^2) <= ss_max, b[0] = query_vals[0]."""
    a0, a1, a2, a3 = query_vals
    for b1 in range(a1, -1, -1):
        for b2 in range(0, 2 * a2 + 1):
            b3 = target - a0 * a0 - a1 * b1 - a2 * b2
            if 0 <= b3 <= 255 and a0 * a0 + b1 * b1 + b2 * b2 + b3 * b3 <= ss_max:
                return [a0, b1, b2, b3]
    raise AssertionError(f"no vector for dot {target}")


def _sparse(indices, counts):
    keep = [k for k, c in enumerate(counts) if c > 0]
    return [indices[k] for k in keep], [float(counts[k]) for k in keep]


def _group(name, fam, query, cands, d, k=50):
    dots, ss = family_dots(d, fam, query)
    return {"name": name, "family": fam, "query": int(query), "cands": [int(c) for c in cands],
            "dots": [int(dots[c]) for c in cands], "ss_query": int(ss[query]), "ss_cands": [int(ss[c]) for c in cands], "k": k}


def _twins(d, fam, rows, indices, counts, share_other=True):
    """Give every row of `rows` the same `fam` vector and (share_other) the first row's vector in the other family."""
    other = "c" if fam == "p" else "p"
    plant(d, fam, {r: _sparse(indices, counts) for r in rows})
    if share_other:
        v = vector(d, other, rows[0])
        plant(d, other, {r: v for r in rows[1:]})


def wide_rows(d):
    n = len(d["person_ids"])
    wide = np.zeros(n, bool)
    for fam in ("p", "c"):
        rp, val = d[fam + "_rowptr"], d[fam + "_val"]
        row_of = np.repeat(np.arange(n), np.diff(rp))
        ss = np.zeros(n)
        np.add.at(ss, row_of, val * val)
        vmax = np.zeros(n)
        np.maximum.at(vmax, row_of, val)
        wide |= (vmax >= 256.0) | (ss >= 65536.0)
    return np.flatnonzero(wide)


def _case(d, groups):
    finish(d)
    return {"d": d, "groups": groups, "wide": wide_rows(d)}


# ---- the cases ------------------------------------------------------------------------------------------------------

def byte_case(value, seed=101):
    """Twin rows with one count of `value` (255: the largest a head / tail element's byte holds; 256: wide) in the place
    family (a popular and the rarest place) and, separately, in the category family."""
    d = base(seed)
    n, s = 3000, slots(3000)
    pa, pb, ca, cb = next(s), next(s), next(s), next(s)
    _twins(d, "p", [pa, pb], [1, d["p_dim"] - 1], [value, 3])
    _twins(d, "c", [ca, cb], [2, d["c_dim"] - 1], [value, 3])
    assert n == len(d["person_ids"])
    return _case(d, [_group(f"place count {value}", "p", pa, [pb], d), _group(f"place count {value} reversed", "p", pb, [pa], d),
                     _group(f"category count {value}", "c", ca, [cb], d), _group(f"category count {value} reversed", "c", cb, [ca], d)])


def u16_case(seed=102):
    """The u16 accumulator's top: twins with ss = 65535 (dot 65535), near-twins with dots around the f16 overflow edge,
    twins with ss = 65536 exactly from counts of 128 (wide by their sum), and pairs whose dot loses (almost) half an f16
    ulp downwards, each placed at its query's K-th rank (k = rank + 1)."""
    d = base(seed)
    n, s = 3000, slots(3000)
    groups = []
    for fam, ix4, ix2 in (("p", [0, 7, 300, 599], [3, 598]), ("c", [0, 5, 11, 19], [1, 18])):
        a = next(s)
        cands = [next(s) for _ in NEAR_DOTS]
        _twins(d, fam, [a] + cands, ix4, TWIN16)
        plant(d, fam, {c: _sparse(ix4, _solve(TWIN16, t, U16_MAX)) for c, t in zip(cands, NEAR_DOTS)})
        groups.append((f"{fam} near twins", fam, a, cands, 50))
        w = [next(s), next(s)]
        _twins(d, fam, w, ix4, [128, 128, 128, 128])
        groups.append((f"{fam} ss 65536", fam, w[0], [w[1]], 50))
        groups.append((f"{fam} ss 65536 reversed", fam, w[1], [w[0]], 50))
        for t in ROUND_DOWN_DOTS:
            q, c = next(s), next(s)
            x = int(np.sqrt(t))
            plant(d, fam, {q: _sparse(ix2, [x, 1]), c: _sparse(ix2, [x, t - x * x])})
            groups.append((f"{fam} dot {t} at the K-th rank", fam, q, [c], None))
    out = []
    for name, fam, q, cands, k in groups:
        out.append(_group(name, fam, q, cands, d, k if k else rank_of(d, q, cands[0]) + 1))
    assert n == len(d["person_ids"])
    return _case(d, out)


def weights_case(mirror=False, seed=103):
    """3,000 persons, a third of them with one count of 165 .. 249 in EACH family (norm above 164: with a weight of
    0.01 the query's f16 scale factor w / norm * 1.006 is subnormal), p_dim 600, c_dim 40, 1 - 2 categories each.
    mirror=False: many shared places, so the top 500 of a heavy query holds place-only neighbours (tiny PLACE weight).
    mirror=True: 1 - 2 places each, so it holds category-only neighbours (tiny CATEGORY weight).
    -> case with "heavy": the heavy rows, "tiny": the family whose weight is tiny, "ks": the Ks the GPU test uses.
    K = 256 is the largest K the head / tail scan's LDS lists hold (the scan whose f16 bound is in question); at K = 50 no
    sampled query has a one-family-only neighbour in its top K, at 256 and 500 all of them have (test_knn_limit_cases.py)."""
    d = base(seed + int(mirror), n=3000, p_dim=600, c_dim=40, places=(1, 2) if mirror else (1, 12), cats=(1, 2),
             skew=1.0 if mirror else 2.5)
    rng = np.random.default_rng(seed + 50)
    heavy = np.arange(0, 3000, 3)
    heavy[-1] = 2999                                   # first, last and middle positions included
    for fam in ("p", "c"):
        v = d[fam + "_val"]
        rp = d[fam + "_rowptr"]
        v[rp[heavy]] = rng.integers(165, 250, len(heavy)).astype(np.float64)
    case = _case(d, [])
    case["heavy"], case["tiny"], case["ks"] = heavy, "c" if mirror else "p", (256, 500)
    return case


def one_family_neighbours(d, row, fam, ids):
    """How many of the persons `ids` share an index with `row` in `fam` but none in the other family."""
    other = "c" if fam == "p" else "p"
    rows = np.flatnonzero(np.isin(d["person_ids"], ids))
    a, _ = family_dots(d, fam, row)
    b, _ = family_dots(d, other, row)
    return int(np.sum((a[rows] > 0) & (b[rows] == 0)))


def cap_case(n, n_wide, seed=104, value=256):
    """`n_wide` rows with one count of 256 (evenly spread, the first and last input rows among them; alternately in the
    place and the category family): the per-row fallback holds up to min(4096, max(256, n / 512)) of them, and fewer than n."""
    d = base(seed, n=n, places=(1, 12) if n > 10_000 else (1, 30))
    rows = np.unique(np.linspace(0, n - 1, n_wide).astype(np.int64)) if n_wide else np.zeros(0, np.int64)
    assert len(rows) == n_wide
    for fam, sel in (("p", rows[0::2]), ("c", rows[1::2])):
        v = d[fam + "_val"]
        v[d[fam + "_rowptr"][sel]] = float(value)
    case = _case(d, [])
    assert np.array_equal(case["wide"], rows)
    return case


def packed_case(p_dim=600, c_dim=20, fam="p", value=1, seed=105, n=2000):
    """Twin rows that hold `value` at the LARGEST index of `fam` (the index / value split of the 32-bit element:
    value < 2^vbits, vbits = min(24, 32 - ceil_log2(dim)); dim < 2^20 - 1); ordinary rows use indices below 600 / 20."""
    d = base(seed, n=n, p_dim=p_dim, c_dim=c_dim, p_span=min(p_dim, 600), c_span=min(c_dim, 20))
    s = slots(n)
    a, b = next(s), next(s)
    _twins(d, fam, [a, b], [3, int(d[fam + "_dim"]) - 1], [2, value])
    return _case(d, [_group(f"{fam} value {value} at index {int(d[fam + '_dim']) - 1}", fam, a, [b], d),
                     _group("reversed", fam, b, [a], d)])


def pack32_case(kind, seed=106, n=2000):
    """PACK32's own accumulator: "max" twins with ss = 2^32 - 1 (their dot is the u32 maximum), "over" twins of one count
    of 65536 (ss = 2^32: no packed format holds it), "big" twins with a count of 2^26 (above every vbits)."""
    d = base(seed, n=n)
    s = slots(n)
    a, b = next(s), next(s)
    counts = {"max": TWIN32, "over": (65536, 0, 0, 0), "big": (2 ** 26, 3, 0, 0)}[kind]
    _twins(d, "p", [a, b], [0, 7, 300, 599], counts)
    return _case(d, [_group(f"pack32 {kind}", "p", a, [b], d), _group(f"pack32 {kind} reversed", "p", b, [a], d)])


def panel_case(p_dim, c_dim, seed=107, n=2000):
    """Dimensions at a panel / table limit, ordinary rows spread over the whole of both families, twins that use the
    last index of each family."""
    d = base(seed, n=n, p_dim=p_dim, c_dim=c_dim, cats=(1, 3), c_skew=1.0)
    s = slots(n)
    a, b, c, e = next(s), next(s), next(s), next(s)
    _twins(d, "p", [a, b], [0, p_dim - 1], [4, 7])
    _twins(d, "c", [c, e], [0, c_dim - 1], [4, 7])
    return _case(d, [_group(f"last place {p_dim - 1}", "p", a, [b], d), _group(f"last category {c_dim - 1}", "c", c, [e], d)])


def long_row_case(length, seed=108, n=300):
    """One person (a middle input row) with `length` places; p_dim is above 2^21, so the format is GENERIC."""
    d = base(seed, n=n, p_dim=(1 << 21) + 8, p_span=600)
    row = n // 2
    plant(d, "p", {row: (np.arange(length, dtype=np.int64), np.ones(length))})
    case = _case(d, [])
    case["long_row"] = row
    return case
