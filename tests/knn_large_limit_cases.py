"""KNN inputs that stand exactly ON the structural limits of the tiled any-K top-K and the large-K aggregation
(csrc/knn_large.hip; DESIGN.md, "Limits of the tiled top-K"), shared by the CPU checks of the cases themselves
(test_knn_large_limit_cases.py) and the GPU tests (test_gpu_knn_large_limits.py).  No GPU and no package import: plain
numpy, and the oracle for the similarity of a pair of patterns.

The data is built from FAMILIES of patterns, so that the structure fixes every count:

  * a family has place and category indices of its own: persons of different families have similarity 0, a query's
    candidates are exactly the other persons of its family;
  * inside a family persons are copies of a few integer patterns: a query sees groups of bit-identical similarity,
    ordered by person id inside a group;
  * person ids are shuffled against the rows and the rows of all families and groups are shuffled over the whole
    table (every pattern of the run families has the same vector lengths, so the index's row order keeps them mixed):
    every LDS run holds entries of every group.

The selection of knn_large.hip is restated here in numpy (`selection`): the bin of a similarity, the populations, the
deciding bin b*, `above`, the segment, its runs and merge passes.  The expected neighbour list of a (query, K) is the
closed form `expected`: groups by similarity descending, person id ascending inside a group.

The limits are written here as literals on purpose: a test that asks the library where its limit lies cannot catch a
moved limit."""
import functools

import numpy as np

RUN = 8192                # kLktRun: entries one block sorts in LDS
BINS = 4096               # kLkHistBins: lkt_select walks them with 1,024 threads of 4 bins each
BINS_PER_THREAD = 4
TILE = 16                 # kLkbQt: queries per tile
SEG_RATERS = 4096         # kSegRaters: raters per aggregation segment
FINISH_TILE = 2048        # kFinishTile: places per finish block
LDS_MAX_K = 1024          # LOCREC_KNN_BATCH_MAX_K: the tiled top-K starts at 1,025
HALF = (0.5, 0.5)
TINY_PW = (2.0 ** -12, 1.0 - 2.0 ** -12)      # a place weight that puts a place-only neighbour into bin 0

P_PER, C_PER = 3, 4       # place / category indices of one family

Q321 = (3, 2, 1)
ONE_CAT = (1, 0, 0, 0)
# place patterns whose similarity to Q321 (same single category, weights 0.5 / 0.5) falls into ONE bin, all distinct
V4093 = ((7, 5, 2), (10, 7, 4), (10, 6, 3))
V4090 = ((5, 3, 2), (12, 9, 5), (7, 4, 2))
V4078 = ((12, 10, 3), (10, 8, 5), (4, 2, 1), (7, 6, 2))      # (10, 8, 5) and (4, 2, 1) are one ulp apart
Q632 = (6, 3, 2)          # sum of squares 49: a twin's cosine is exactly 1.0


def _run_family(name, variant, counts):
    return {"name": name, "query_pattern": 0,
            "patterns": [(Q321, ONE_CAT, 1)] + [(p, ONE_CAT, c) for p, c in zip(variant, counts)]}


FAMILIES = [
    _run_family("run8192", V4093, (4000, 4000, 192)),
    _run_family("run8193", V4078, (3000, 2500, 2500, 193)),
    _run_family("run16384", V4090, (8192, 8000, 192)),
    _run_family("run16385", V4093, (8192, 8192, 1)),
    _run_family("run24577", V4078, (8192, 8192, 8192, 1)),
    _run_family("run32769", V4090, (16384, 16384, 1)),
    # under TINY_PW: the query's 1,100 twins at s = 1.0 exactly (bin 4095, the clamp), groups in bins 3699 = 4 * 924 + 3,
    # 3697 = 4 * 924 + 1, 3696 = 4 * 924, 3652 = 4 * 913 (alone in its thread's range) and bin 0 (no shared category)
    {"name": "bins", "query_pattern": 0,
     "patterns": [(Q632, (6, 3, 2, 0), 1101), (Q632, (11, 0, 4, 0), 300), (Q632, (7, 0, 2, 0), 200), (Q632, (18, 0, 7, 0), 250),
                  (Q632, (9, 11, 9, 0), 150), ((7, 5, 2), (0, 0, 0, 1), 120)]},
    _run_family("cand1030", V4090, (400, 400, 230)),
    _run_family("only2048", V4093, (3, 2)),
    _run_family("tile0", V4093, (3, 2)),
    _run_family("norows", V4093, (3, 2)),
]
FAMILY_INDEX = {f["name"]: i for i, f in enumerate(FAMILIES)}

# segment -> (K values, runs, merge passes, deciding bin): the table of the limits
RUN_TABLE = {
    "run8192": (8192, (1025, 8191, 8192), 1, 0, 4093),
    "run8193": (8193, (1025, 8192, 8193), 2, 1, 4078),
    "run16384": (16384, (8193, 16383, 16384), 2, 1, 4090),
    "run16385": (16385, (16384, 16385), 3, 2, 4093),
    "run24577": (24577, (8193, 24577), 4, 2, 4078),
    "run32769": (32769, (1025, 8194, 32768, 32769), 5, 3, 4090),
}
# (K, b*, above, segment) of the bins family under TINY_PW: K at the first and the last entry of each deciding bin (the
# first entry of bin 4095 is K = 1, below the tiled path: 1,025 stands in for it)
BIN_TABLE = ((1025, 4095, 0, 1100), (1100, 4095, 0, 1100),
             (1101, 3699, 1100, 1400), (1400, 3699, 1100, 1400),
             (1401, 3697, 1400, 1600), (1600, 3697, 1400, 1600),
             (1601, 3696, 1600, 1850), (1850, 3696, 1600, 1850),
             (1851, 3652, 1850, 2000), (2000, 3652, 1850, 2000),
             (2001, 0, 2000, 2120), (2120, 0, 2000, 2120))
CAND = 1030
CAND_KS = (1029, 1030, 1031)

# ratings: 2,049 distinct rated places, place of rank r has id PLACE0 + 3 r
N_PLACES = 2049
PLACE0 = 5000
SPECIAL_RATERS = {0: 4095, 1: 4096, 2: 4097, 3: 8192, 2046: 8193}     # rank -> raters, all inside run16384
FILL0, FILL1 = 4, 2046                                                 # filler places: ranks FILL0 .. FILL1 - 1
AGG_FAMILY = "run16384"
AGG_KS = (8193, 16383, 16384)


def place_id(rank):
    return PLACE0 + 3 * rank


def place_rank(ids):
    return (np.asarray(ids) - PLACE0) // 3


# ---- the selection of knn_large.hip, restated -----------------------------------------------------------------------

def bin_of(s):
    return np.minimum((np.asarray(s, np.float64) * BINS).astype(np.int64), BINS - 1)


def selection(sims, k):
    """lkt_select + the plan of lkt_topk_tile for one column: `sims` are the similarities (> 0) of the candidates."""
    sims = np.asarray(sims, np.float64)
    assert np.all(sims > 0)
    pop = np.bincount(bin_of(sims), minlength=BINS)
    total = int(pop.sum())
    if total <= k:
        bstar, above, segment = 0, total - int(pop[0]), total
    else:
        at_or_above = np.cumsum(pop[::-1])[::-1]                 # candidates in bins >= b
        bstar = int(np.flatnonzero(at_or_above >= k)[-1])        # the highest bin from which K candidates stand
        above = int(at_or_above[bstar] - pop[bstar])
        segment = above + int(pop[bstar])
    runs = -(-segment // RUN)
    passes, r = 0, RUN
    while r < segment:
        r, passes = 2 * r, passes + 1
    return {"cand": total, "bstar": bstar, "above": above, "segment": segment, "runs": runs, "passes": passes,
            "all": total <= k, "bins": int(np.count_nonzero(pop)), "m": min(k, total)}


# ---- building the tables ---------------------------------------------------------------------------------------------

def _sparse(base, counts):
    idx = [base + j for j, c in enumerate(counts) if c > 0]
    return np.array(idx, np.int32), np.array([float(c) for c in counts if c > 0])


def _csr(pat_of_row, vectors):
    lens = np.array([len(v[0]) for v in vectors], np.int64)[pat_of_row]
    rowptr = np.zeros(len(pat_of_row) + 1, np.int64)
    np.cumsum(lens, out=rowptr[1:])
    idx, val = np.zeros(rowptr[-1], np.int32), np.zeros(rowptr[-1], np.float64)
    for g, (vi, vv) in enumerate(vectors):
        rows = np.flatnonzero(pat_of_row == g)
        if len(vi) and len(rows):
            at = rowptr[rows][:, None] + np.arange(len(vi))[None, :]
            idx[at], val[at] = vi[None, :], vv[None, :]
    return rowptr, idx, val


def _ratings_csr(n, rows, places, ratings):
    rows, places, ratings = (np.concatenate(x).astype(np.int64) for x in (rows, places, ratings))
    order = np.lexsort((places, rows))
    rows, places, ratings = rows[order], places[order], ratings[order]
    assert len(np.unique(rows * (1 << 32) + places)) == len(rows), "a person rates a place twice"
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, places, ratings


@functools.lru_cache(maxsize=None)
def main_index(seed=20):
    """-> (d, meta): the index of all families.  meta: fam_of_row, pat_of_row (pattern inside the family), members
    {(family, pattern): rows in generation order}, query {family name: row}."""
    rng = np.random.default_rng(seed)
    fam, pat = [], []
    for f, spec in enumerate(FAMILIES):
        for g, (_, _, count) in enumerate(spec["patterns"]):
            fam += [f] * count
            pat += [g] * count
    fam, pat = np.array(fam), np.array(pat)
    n = len(fam)
    shuffle = rng.permutation(n)                                 # rows of all families and groups interleaved
    fam, pat = fam[shuffle], pat[shuffle]
    first = np.cumsum([0] + [len(s["patterns"]) for s in FAMILIES])
    gpat = first[fam] + pat
    pvec = [_sparse(f * P_PER, p[0]) for f, s in enumerate(FAMILIES) for p in s["patterns"]]
    cvec = [_sparse(f * C_PER, p[1]) for f, s in enumerate(FAMILIES) for p in s["patterns"]]
    prp, pidx, pval = _csr(gpat, pvec)
    crp, cidx, cval = _csr(gpat, cvec)
    d = {"person_ids": (rng.permutation(n) * 3 + 1_000).astype(np.int64),
         "p_rowptr": prp, "p_idx": pidx, "p_val": pval, "p_dim": len(FAMILIES) * P_PER,
         "c_rowptr": crp, "c_idx": cidx, "c_val": cval, "c_dim": len(FAMILIES) * C_PER}
    members = {(f, g): np.flatnonzero((fam == f) & (pat == g)) for f, s in enumerate(FAMILIES) for g in range(len(s["patterns"]))}
    query = {s["name"]: int(members[(f, s["query_pattern"])][0]) for f, s in enumerate(FAMILIES)}
    meta = {"fam_of_row": fam, "pat_of_row": pat, "members": members, "query": query}

    # ratings, planted independently of the vectors
    rr, rp, rv = [], [], []

    def rate(rows, ranks):
        rows = np.asarray(rows, np.int64)
        rr.append(rows)
        rp.append(place_id(np.broadcast_to(np.asarray(ranks, np.int64), rows.shape)))
        rv.append(rng.integers(1, 6, len(rows)))

    def others(name):
        f = FAMILY_INDEX[name]
        rows = np.flatnonzero(fam == f)
        return rows[rows != query[name]]

    big = others(AGG_FAMILY)
    for rank, count in SPECIAL_RATERS.items():
        rate(rng.choice(big, count, replace=False), rank)
    only, tile0 = others("only2048"), others("tile0")
    rate(rng.choice(big, 60, replace=False), 2047)
    rate(rng.choice(big, 60, replace=False), 2048)
    rate(only, 2048)
    rate(tile0, 2047)
    rate(tile0, 5)
    span = FILL1 - FILL0
    for name, mul, add, step in (("run32769", 1, 0, 1), ("run24577", 7, 3, 1), ("cand1030", 13, 0, 1), ("run8192", 5, 1, 1),
                                 ("bins", 11, 0, 1), ("run8193", 3, 2, 3), ("run16385", 17, 5, 2)):
        rows = others(name)[::step]
        rate(rows, FILL0 + (mul * np.arange(len(rows)) + add) % span)
    d["r_rowptr"], d["r_place"], d["r_rating"] = _ratings_csr(n, rr, rp, rv)
    return d, meta


@functools.lru_cache(maxsize=None)
def pattern_sims(family, weights):
    """Similarity of every ordered pair of patterns of a family under `weights`, from the oracle (a similarity depends on
    the two vectors only): M[query pattern][candidate pattern], 0 where the pair is not a candidate."""
    import oracle_binding
    spec = FAMILIES[FAMILY_INDEX[family]]
    npat = len(spec["patterns"])
    two = np.repeat(np.arange(npat), 2)                          # every pattern twice: a twin's similarity too
    prp, pidx, pval = _csr(two, [_sparse(0, p[0]) for p in spec["patterns"]])
    crp, cidx, cval = _csr(two, [_sparse(0, p[1]) for p in spec["patterns"]])
    mini = {"person_ids": np.arange(2 * npat, dtype=np.int64), "p_rowptr": prp, "p_idx": pidx, "p_val": pval, "p_dim": P_PER,
            "c_rowptr": crp, "c_idx": cidx, "c_val": cval, "c_dim": C_PER}
    ids, sims, cnt = oracle_binding.knn_similar_batch(mini, np.arange(0, 2 * npat, 2), weights[0], weights[1], 2 * npat)
    m = np.zeros((npat, npat))
    for g in range(npat):
        got = ids[g, :cnt[g]]
        for h in range(npat):
            at = np.flatnonzero(got == 2 * h + 1)
            if len(at):
                m[g, h] = sims[g, at[0]]
                other = np.flatnonzero(got == 2 * h)
                assert h == g or (len(other) and sims[g, other[0]] == m[g, h])
    return m


def candidates(row, weights=HALF):
    """-> (rows, person ids, similarities) of the candidates of `row`: the other persons of its family with s > 0."""
    d, meta = main_index()
    f = int(meta["fam_of_row"][row])
    m = pattern_sims(FAMILIES[f]["name"], tuple(weights))
    rows = np.flatnonzero(meta["fam_of_row"] == f)
    rows = rows[rows != row]
    sims = m[int(meta["pat_of_row"][row])][meta["pat_of_row"][rows]]
    keep = sims > 0
    return rows[keep], d["person_ids"][rows[keep]], sims[keep]


def expected(row, k, weights=HALF):
    """The neighbour list of (row, K) in closed form: -> (rows, ids, sims), similarity descending, id ascending."""
    rows, ids, sims = candidates(row, weights)
    order = np.lexsort((ids, -sims))[:k]
    return rows[order], ids[order], sims[order]


def facts(row, k, weights=HALF):
    return selection(candidates(row, weights)[2], k)


def expected_places(row, k, weights=HALF):
    """The places somebody among the neighbours of (row, K) rated, ascending."""
    d, _ = main_index()
    rows = expected(row, k, weights)[0]
    rp = d["r_rowptr"]
    takes = [d["r_place"][rp[r]:rp[r + 1]] for r in rows]
    return np.unique(np.concatenate(takes)) if takes else np.zeros(0, np.int64)


# ---- the listed cases -------------------------------------------------------------------------------------------------

def cases():
    """Every listed (query, K): dicts {name, row, weights, k, planted}; `planted` holds the literals of the tables above
    that the restatement must reproduce."""
    _, meta = main_index()
    out = []
    for name, (segment, ks, runs, passes, bstar) in RUN_TABLE.items():
        for k in ks:
            full = segment <= k
            out.append({"name": f"{name} K={k}", "row": meta["query"][name], "weights": HALF, "k": k,
                        "planted": {"cand": segment, "segment": segment, "runs": runs, "passes": passes,
                                    "bstar": 0 if full else bstar, "above": segment if full else 0, "all": full, "bins": 1}})
    for k, bstar, above, segment in BIN_TABLE:
        out.append({"name": f"bins K={k}", "row": meta["query"]["bins"], "weights": TINY_PW, "k": k,
                    "planted": {"cand": 2120, "segment": segment, "runs": 1, "passes": 0, "bstar": bstar, "above": above,
                                "all": k >= 2120, "bins": 6}})
    for k in CAND_KS:
        full = CAND <= k
        out.append({"name": f"cand1030 K={k}", "row": meta["query"]["cand1030"], "weights": HALF, "k": k,
                    "planted": {"cand": CAND, "segment": CAND, "runs": 1, "passes": 0, "bstar": 0 if full else 4090,
                                "above": CAND if full else 0, "all": full, "bins": 1}})
    for name in ("only2048", "tile0", "norows"):
        out.append({"name": f"{name} K=1025", "row": meta["query"][name], "weights": HALF, "k": 1025,
                    "planted": {"cand": 5, "segment": 5, "runs": 1, "passes": 0, "bstar": 0, "above": 5, "all": True, "bins": 1}})
    return out


def mixed_rows(nq):
    """The mixed tile: one query of every family (segments 8,192 .. 32,769 and small ones: columns of one launch grid
    that need 0, 1, 2 and 3 merge passes) and five members of the large groups; nq = 16 distinct queries, or 17 / 33 with
    further members, one query given twice, in shuffled order: the sixteen stay together as the first tile (shuffled among
    themselves), the further members follow (shuffled), the repeated query is the last tile's only one."""
    _, meta = main_index()
    m = meta["members"]
    fi = FAMILY_INDEX
    rows = [meta["query"][s["name"]] for s in FAMILIES]
    rows += [int(m[(fi["run8192"], 1)][0]), int(m[(fi["run16385"], 1)][0]), int(m[(fi["run32769"], 3)][0]),
             int(m[(fi["bins"], 1)][0]), int(m[(fi["cand1030"], 1)][0])]
    assert len(set(rows)) == TILE
    if nq == TILE:
        return np.array(rows)
    k = 1
    while len(rows) < nq - 1:                                    # further members of the first eight families
        for f in range(8):
            for g in (1, 2):
                if len(rows) < nq - 1 and k < len(m[(f, g)]) and int(m[(f, g)][k]) not in rows:
                    rows.append(int(m[(f, g)][k]))
        k += 1
    rng = np.random.default_rng(nq)
    rows = np.r_[rng.permutation(np.array(rows[:TILE])), rng.permutation(np.array(rows[TILE:], np.int64))].astype(np.int64)
    return np.r_[rows, rows[3]]                                  # one query twice


MIXED_KS = {16: (1025, 8193, 32769), 17: (8193, 32769), 33: (8193, 32769)}


# ---- the small index, in creation order -------------------------------------------------------------------------------

SMALL_N = 1100
SMALL_K = 1025
SMALL_INVALID = tuple(range(15, 33)) + (SMALL_N - 1,)      # 16 .. 31: a whole tile of the all-pairs form; 15: the last slot
#                                                             of a tile; 32: the first slot of the next; the last person
SMALL_PATTERNS = (((3, 2, 1, 0), (1, 0)), ((7, 5, 2, 0), (1, 0)), ((10, 7, 4, 0), (2, 1)), ((5, 3, 0, 2), (1, 1)),
                  ((6, 3, 2, 0), (1, 2)), ((1, 1, 0, 0), (1, 0)), ((4, 0, 1, 1), (3, 1)), ((2, 1, 1, 1), (1, 0)))


@functools.lru_cache(maxsize=None)
def small_index(seed=21):
    """1,100 persons of eight patterns that all share place 0 and category 0 (every pair is a candidate pair: 1,099
    candidates a query, K = 1,025 cuts inside tie groups); the persons at SMALL_INVALID have ONE place and no category
    vector: candidates, but no valid queries.  Every other person has at least two places, so the index's row order
    (ascending vector lengths) puts the 19 invalid persons first."""
    rng = np.random.default_rng(seed)
    pat = rng.integers(0, len(SMALL_PATTERNS), SMALL_N)
    pat[list(SMALL_INVALID)] = len(SMALL_PATTERNS)
    pvec = [_sparse(0, p[0]) for p in SMALL_PATTERNS] + [_sparse(0, (2,))]
    cvec = [_sparse(0, p[1]) for p in SMALL_PATTERNS] + [_sparse(0, ())]
    prp, pidx, pval = _csr(pat, pvec)
    crp, cidx, cval = _csr(pat, cvec)
    d = {"person_ids": (rng.permutation(SMALL_N) * 7 + 50).astype(np.int64),
         "p_rowptr": prp, "p_idx": pidx, "p_val": pval, "p_dim": 4,
         "c_rowptr": crp, "c_idx": cidx, "c_val": cval, "c_dim": 2}
    d["r_rowptr"], d["r_place"] = prp.copy(), pidx.astype(np.int64)
    d["r_rating"] = rng.integers(1, 6, len(pidx)).astype(np.int64)
    return d
