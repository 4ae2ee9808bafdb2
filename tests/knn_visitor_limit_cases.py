"""Inputs that stand ON the limits of KNN for visitors (csrc/knn_visitors.h, knn_visitors_api.h, knn_visitors_plan.h,
knn_visitors_side.h), and plain-Python restatements of what the sources decide: the stage's walk
of one vector (lkv_stage), the report rule of a batch, and a call's tiles, chunks and waits (knn_visitors_plan.h and the
drivers' counters).  Shared by the CPU checks of the cases themselves (test_knn_visitor_limit_cases.py) and the GPU tests
(test_gpu_knn_visitor_limits.py).  Seeded; numpy and knn_visitor_cases only: nothing of the library under test.

The limits are written here as literals on purpose: a test that asks the library where its limit lies cannot catch a
moved limit."""
import functools

import numpy as np

import knn_visitor_cases as vc

LONG = 1 << 21                    # a vector of this many entries is refused; LONG - 1 are served
COUNT_BOUND = 65536.0             # a place value on a renumbered index: an integer with |x| below this
STAGE_BLOCK = 256                 # visitors of one block of lkv_stage
TILE = 16                         # visitors of one scan tile (kLkbQt)
FILL_BLOCK = 256                  # entries of one block of the fill launches
ENTRY_BYTES = 20                  # id, similarity, row of one entry of the device result arrays
CHUNK_BYTES = 2 << 30             # the default budget of a chunk of neighbour lists
MAX_ROW_BYTES = 48 << 30          # a recommendation call that may leave more rows than this is refused
ROW_BYTES = 16
PYTHON_ROOM = 1 << 16             # rows of the Python wrapper's first attempt
P_DIM = vc.P_DIM

# the stage's refusal codes, in the order the kernel tests them for one entry
PTR, TOO_LONG, EMPTY, NEGATIVE, ORDER, FINITE, FRACTION, ZERO = range(1, 9)
FAMILIES = ("place", "category")
NOT_FOUND = {EMPTY}               # LOCREC_E_NOT_FOUND; every other code is LOCREC_E_INVALID_ARG


def message(code, fam, who):
    """The text of the refusal (knn_visitors_stage's switch)."""
    name = FAMILIES[fam]
    return {PTR: f"{name} rowptr not monotone at visitor {who}",
            TOO_LONG: f"{name} vector of visitor {who} has 2^21 or more entries",
            EMPTY: f"No such person: visitor {who} has no {name} vector",
            NEGATIVE: f"{name} index of visitor {who} is negative",
            ORDER: f"{name} indices of visitor {who} not strictly ascending",
            FINITE: f"{name} value of visitor {who} is not finite",
            FRACTION: f"{name} value of visitor {who} is not an integer count below 65536",
            ZERO: f"{name} vector of visitor {who} has zero norm"}[code]


# ---- the stage ------------------------------------------------------------------------------------------------------------

def left_fold_norm(values):
    """sqrt of the left fold of squares in the given order (Distance.vectorLength; the stage's `sum = sum + x * x`)."""
    s = 0.0
    for x in np.asarray(values, np.float64).tolist():
        s = s + x * x
    return float(np.sqrt(np.float64(s)))


def stage_vector(idx, val, dim, integer_rule, new_of_old=None):
    """lkv_stage for one (visitor, family) whose row pointers are good -> dict(code, idx, val, beyond, norm): the refusal
    code or 0; without a refusal the kept entries in their order (indices through new_of_old when given), the number of
    entries at an index >= dim and the fp64 vector length.  integer_rule: the family is the place family of an index that
    renumbers its place dimensions.  The walk stops at the first offending entry; within an entry the order of the tests is
    negative index, order, finite, integer."""
    idx, val = np.asarray(idx, np.int64), np.asarray(val, np.float64)
    m = len(idx)
    if m >= LONG:
        return dict(code=TOO_LONG)
    if m == 0:
        return dict(code=EMPTY)
    first = {}                                                   # code -> position of its first offender
    def note(code, mask):
        at = np.flatnonzero(mask)
        if len(at):
            first[code] = int(at[0])
    note(NEGATIVE, idx < 0)
    note(ORDER, np.r_[False, idx[1:] <= idx[:-1]])
    note(FINITE, ~np.isfinite(val))
    if integer_rule:
        with np.errstate(invalid="ignore"):
            note(FRACTION, (val != np.floor(val)) | ~(np.abs(val) < COUNT_BOUND))
    if first:
        return dict(code=min(first, key=lambda c: (first[c], c)))
    norm = left_fold_norm(val)
    if not norm > 0:
        return dict(code=ZERO)
    keep = idx < dim
    kept = idx[keep] if new_of_old is None else np.asarray(new_of_old)[idx[keep]]
    return dict(code=0, idx=kept.astype(np.int32), val=val[keep], beyond=int((~keep).sum()), norm=norm)


def stage_vector_brute(idx, val, dim, integer_rule):
    """The same code by the kernel's loop, entry by entry (the check of stage_vector)."""
    m = len(idx)
    if m >= LONG:
        return TOO_LONG
    if m == 0:
        return EMPTY
    prev, s = -1, 0.0
    for i in range(m):
        ix, x = int(idx[i]), float(val[i])
        if ix < 0:
            return NEGATIVE
        if i > 0 and ix <= prev:
            return ORDER
        if not np.isfinite(x):
            return FINITE
        if integer_rule and (x != np.floor(x) or not abs(x) < COUNT_BOUND):
            return FRACTION
        prev = ix
        s = s + x * x
    return 0 if s > 0 else ZERO


def first_refusal(visitors, p_dim, c_dim, renumbered):
    """The report rule: every (visitor, family) with a refusal reports visitor << 8 | family << 4 | code and the smallest
    word wins -> (visitor, family, code) or None: the smallest visitor, within it the place family."""
    words = []
    for who, v in enumerate(visitors):
        for fam, (k, dim) in enumerate((("p", p_dim), ("c", c_dim))):
            code = stage_vector(v[k + "_idx"], v[k + "_val"], dim, renumbered and fam == 0)["code"]
            if code:
                words.append(who << 8 | fam << 4 | code)
    if not words:
        return None
    w = min(words)
    return w >> 8, (w >> 4) & 1, w & 0xF


def first_refusal_brute(visitors, p_dim, c_dim, renumbered):
    """The same by a scan in the order the rule names: visitors ascending, places before categories."""
    for who, v in enumerate(visitors):
        for fam, (k, dim) in enumerate((("p", p_dim), ("c", c_dim))):
            code = stage_vector_brute(v[k + "_idx"], v[k + "_val"], dim, renumbered and fam == 0)
            if code:
                return who, fam, code
    return None


def beyond_total(visitors, p_dim, c_dim):
    return sum(int((np.asarray(v["p_idx"]) >= p_dim).sum()) + int((np.asarray(v["c_idx"]) >= c_dim).sum()) for v in visitors)


# ---- the plan of a call (knn_visitors_plan.h) and the counters of the drivers -------------------------------------------

def chunk_visitors(k, budget=CHUNK_BYTES):
    """Visitors of one chunk of a neighbour-list call: their nv x K entries stay within the budget; whole tiles where a
    chunk holds one; one visitor at least."""
    c = max(1, budget // (max(1, k) * ENTRY_BYTES))
    return c // TILE * TILE if c >= TILE else c


def budget_for(chunk, k):
    """A budget (the text of LOCREC_KNN_VISITORS_CHUNK_BYTES) under which a chunk holds `chunk` visitors at this K."""
    return chunk * k * ENTRY_BYTES


def chunks_of(nv, k, budget=CHUNK_BYTES):
    c = chunk_visitors(k, budget)
    return [(v0, min(c, nv - v0)) for v0 in range(0, nv, c)]


def fill_blocks(kept_lengths):
    """Blocks of the fill launches of one tile: over the longest staged vector of its visitors, one at least."""
    return (max([1] + list(kept_lengths)) + FILL_BLOCK - 1) // FILL_BLOCK


def worst_row_bytes(nv, rated_places):
    return nv * max(1, rated_places) * ROW_BYTES


def call_stats(form, nv, k, n, rated_places, device, budget=CHUNK_BYTES, rows=None, room=PYTHON_ROOM):
    """What locrec_knn_visitors_stats says after a served call of nv > 0 visitors: form "query" or "recommend" (the
    ranked form adds the ranker's waits to the recommend form's: not restated).  rows: the rows a recommend call
    returns (None: host_syncs is left out); room: the capacity it was given.
    Waits: the stage reads the ends of device row pointers (1) and its report (1); a tile through the selection waits
    for its sizes (1); a chunk of lists waits for its copies (1); a tile's aggregation waits for its counts (1, where
    the index has rated places); the copy of rows that fit waits once."""
    stage = 2 if device else 1
    if n == 0:
        return dict(tiles=0, tiles_all=0, tiles_topk=0, stage_launches=1, scan_launches=0, host_syncs=stage)
    if form == "query":
        parts = chunks_of(nv, k, budget)
        tiles = sum((cn + TILE - 1) // TILE for _, cn in parts)
        return dict(tiles=tiles, tiles_all=0, tiles_topk=tiles, stage_launches=1, scan_launches=tiles,
                    host_syncs=stage + tiles + len(parts))
    tiles = (nv + TILE - 1) // TILE
    every = k >= n
    st = dict(tiles=tiles, tiles_all=tiles if every else 0, tiles_topk=0 if every else tiles, stage_launches=1, scan_launches=tiles)
    if rows is not None:
        st["host_syncs"] = stage + (0 if every else tiles) + (tiles if rated_places > 0 else 0) + (1 if 0 < rows <= room else 0)
    return st


# ---- data: small indexes out of knn_visitor_cases' base, and visitors -----------------------------------------------------

@functools.lru_cache(maxsize=None)
def small_index(n, integer=True):
    """The first n persons of the base data (p_dim = 600) with explicit ratings."""
    d, _ = vc.base(integer)
    s = vc.from_rows(d, np.arange(n))
    if integer:
        return vc.explicit_ratings(s)
    return dict(s, r_rowptr=np.asarray(s["p_rowptr"], np.int64), r_place=np.asarray(s["p_idx"], np.int64),
                r_rating=np.floor(s["p_val"]).astype(np.int64))


def rated_places(d):
    return len(np.unique(d["r_place"])) if "r_place" in d else 0


def but(v, **kw):
    return dict(v, **{k: np.asarray(x, np.int32 if k.endswith("idx") else np.float64) for k, x in kw.items()})


# a. stage blocks
STAGE_N = 40
STAGE_NVS = (255, 256, 257)
STAGE_DISTINCT = 6


def stage_batch(nv, seed=1):
    """(the visitors, which of the STAGE_DISTINCT base visitors each one is): drawn with repetition, every distinct one
    present, the last of the batch never equal to the one before it."""
    _, visitors = vc.base()
    rng = np.random.default_rng(seed + nv)
    which = rng.integers(0, STAGE_DISTINCT, nv)
    which[:STAGE_DISTINCT] = np.arange(STAGE_DISTINCT)
    if which[-1] == which[-2]:
        which[-1] = (which[-2] + 1) % STAGE_DISTINCT
    return [visitors[j] for j in which], which


def offenders():
    """[(label, {visitor: replacement})] planted into a batch of 301 good visitors: around the seam of the stage's
    blocks at 255 | 256, across blocks, and both families of one visitor."""
    _, visitors = vc.base()
    ok = visitors[0]
    place = but(ok, p_idx=[3, 3], p_val=[1, 1])                     # ORDER
    place2 = but(ok, p_idx=[4], p_val=[np.inf])                     # FINITE
    category = but(ok, c_idx=[5, 2], c_val=[1, 1])                  # ORDER
    both = but(ok, p_idx=[-1, 4], p_val=[1, 1], c_idx=[2], c_val=[np.nan])   # NEGATIVE place, FINITE category
    return [("255 alone", {255: place}), ("256 alone", {256: place}), ("256 and 300", {256: place2, 300: place}),
            ("category at 255, place at 256", {255: category, 256: place}), ("both families at 256", {256: both}),
            ("0 and 299", {0: category, 299: place})]


OFFENDER_NV = 301


def offender_batch(planted):
    good, _ = stage_batch(257)
    batch = [good[i % 257] for i in range(OFFENDER_NV)]
    for who, v in planted.items():
        batch[who] = v
    return batch


# b. the length limit
def long_visitor(family, length=LONG - 1):
    """A visitor whose place (or category) vector holds `length` entries at the indices 0 .. length - 1: all but the
    first 600 (20) lie beyond the dimensions.  Place values 65535: the largest count a renumbered index takes."""
    _, visitors = vc.base()
    short = vc.without_beyond(visitors[1], P_DIM, 20)
    if family == "p":
        return dict(short, p_idx=np.arange(length, dtype=np.int32), p_val=np.full(length, 65535.0))
    return dict(short, c_idx=np.arange(length, dtype=np.int32), c_val=np.full(length, 3.0))


def nowhere_visitor(j, p_dim=P_DIM):
    """No place inside the dimensions (nothing is set in the dense place table), categories of a base visitor."""
    _, visitors = vc.base()
    return dict(visitors[j], p_idx=np.array([p_dim + j, p_dim + 100 + 2 * j], np.int32), p_val=np.array([2.0, 1.0 + j % 3]))


# c. value bounds
def value_cases(d):
    """-> (served on a renumbered index, refused there as not an integer count): place vectors over places that persons
    of d hold, categories of a base visitor."""
    _, visitors = vc.base()
    ok = vc.without_beyond(visitors[2], d["p_dim"], d["c_dim"])
    at = vc.row_of(d, 8)["p_idx"][:2]                                 # two places somebody holds
    assert len(at) == 2
    served = {"-65535": [-65535.0, 3.0], "-1": [-1.0, 2.0], "0 beside 4": [0.0, 4.0], "-0.0 beside 4": [-0.0, 4.0],
              "65535": [65535.0, 1.0]}
    refused = {"65536": [65536.0, 1.0], "-65536": [2.0, -65536.0], "65535.5": [65535.5, 1.0], "0.5": [1.0, 0.5],
               "5e-324": [5e-324, 1.0]}
    make = lambda vals: but(ok, p_idx=at, p_val=vals)                 # noqa: E731
    return {k: make(v) for k, v in served.items()}, {k: make(v) for k, v in refused.items()}


def generic_value_cases(d):
    """On an index that keeps the caller's numbering -> {label: (visitor, refusal code or 0)}."""
    _, visitors = vc.base(False)
    ok = vc.without_beyond(visitors[2], d["p_dim"], d["c_dim"])
    at = vc.row_of(d, 8)["p_idx"][:2]
    cat = vc.row_of(d, 8)["c_idx"][:1]
    return {"1e160 place": (but(ok, p_idx=at, p_val=[1e160, 2.5]), 0),
            "1e160 category": (but(ok, c_idx=cat, c_val=[1e160]), 0),
            "1e-170 alone": (but(ok, p_idx=at[:1], p_val=[1e-170]), ZERO),
            "1e-170 category alone": (but(ok, c_idx=cat, c_val=[1e-170]), ZERO),
            "5e-324 beside 1": (but(ok, p_idx=at, p_val=[5e-324, 1.0]), 0),
            "0.5": (but(ok, p_idx=at, p_val=[1.0, 0.5]), 0)}


# d. chunks
CHUNK_N = 300
CHUNK_SIZES = (5, 16, 32)
CHUNK_NVS = (16, 17, 33, 49)
CHUNK_KS = (1, 50, CHUNK_N, 2_000_000)


def clipped(k, n):
    """The K a test passes for K = 2,000,000: the output arrays are nv x K (test_gpu_knn_visitors.check_query's clip)."""
    return min(k, n + 5)


@functools.lru_cache(maxsize=None)
def distinct_visitors(count=max(CHUNK_NVS)):
    """`count` pairwise different visitors: persons of the base data behind the CHUNK_N of the index, each with two
    places or more, with entries beyond the dimensions."""
    d, _ = vc.base()
    out, seen = [], set()
    for r in range(CHUNK_N, len(d["person_ids"])):
        v = vc.row_of(d, r)
        key = (tuple(v["p_idx"].tolist()), tuple(v["p_val"].tolist()), tuple(v["c_idx"].tolist()), tuple(v["c_val"].tolist()))
        if len(v["p_idx"]) < 2 or key in seen:
            continue
        seen.add(key)
        out.append(vc.with_beyond(v, d["p_dim"], d["c_dim"], len(out)))
        if len(out) == count:
            return out
    raise AssertionError("the base data has too few distinct rows")


# e. capacity
CAPACITY_NV = 257


def everybody_visitor(d, j):
    """Every category (every person a neighbour), one place; j makes the values differ."""
    v = vc.all_categories_visitor(d)
    return dict(v, c_val=v["c_val"] + (j % 3), p_val=np.array([1.0 + j % 2]))


# f. the row refusal: nv x rated places x 16 bytes against 48 GiB = 3 x 2^30 rows
ROW_PLACES = 3 << 16
ROW_NV = 1 << 14


def row_refusal_index():
    """Four persons who rate ROW_PLACES distinct places between them (vectors of the base data)."""
    d = small_index(4)
    per = ROW_PLACES // 4
    return dict({k: v for k, v in d.items() if not k.startswith("r_")},
                r_rowptr=np.arange(5, dtype=np.int64) * per, r_place=7 + 3 * np.arange(ROW_PLACES, dtype=np.int64),
                r_rating=1 + np.arange(ROW_PLACES, dtype=np.int64) % 5)


def nobody_batch(d, nv):
    v = vc.nobody_visitor(d)
    arrays = vc.csr([v])
    tile = lambda a, ptr: (np.arange(nv + 1, dtype=np.int64) * len(a)) if ptr else np.tile(a, nv)   # noqa: E731
    return (tile(arrays[1], True), tile(arrays[1], False), tile(arrays[2], False),
            tile(arrays[4], True), tile(arrays[4], False), tile(arrays[5], False))


# g. index edges
def empty_index():
    return dict(person_ids=np.zeros(0, np.int64), p_rowptr=np.zeros(1, np.int64), p_idx=np.zeros(0, np.int32), p_val=np.zeros(0),
                p_dim=P_DIM, c_rowptr=np.zeros(1, np.int64), c_idx=np.zeros(0, np.int32), c_val=np.zeros(0), c_dim=20)


def without_ratings(d):
    """d with rating arrays that hold no row (an index of persons who rated nothing)."""
    n = len(d["person_ids"])
    return dict({k: v for k, v in d.items() if not k.startswith("r_")}, r_rowptr=np.zeros(n + 1, np.int64),
                r_place=np.zeros(0, np.int64), r_rating=np.zeros(0, np.int64))
