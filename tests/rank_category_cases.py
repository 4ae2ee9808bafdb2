"""Inputs of the by-category ranker's tests (locrec_rank_recommendations_batch_by_category): rank_batch_cases',
rank_exclude_cases' and rank_near_cases' cases with a category per row of the place table, an allow-list per segment and
a cap per segment.  Seeded generators, no GPU.  A case is their dict plus cats (one per row of the place table) and,
where it has them, al_offsets / al_ids (the allow-lists, CSR) and caps (one per segment).

The expected value is composed of code that is not under test: an existing single ranker at limit = segment length on
the place table cut to the passing listings (as rank_near_cases.expected cuts it), then the greedy walk with a counter
per category."""
import numpy as np

import rank_batch_cases as rb
import rank_exclude_cases as rx
import rank_near_cases as rn

I64_MIN, I64_MAX = rb.I64_MIN, rb.I64_MAX
FEW = np.array([I64_MIN, -3, 0, 7, I64_MAX], np.int64)      # five categories, the ends of int64 among them: caps bind
UNKNOWN = np.array([I64_MIN + 1, 8, 10 ** 12, I64_MAX - 1], np.int64)    # categories no place has
LIMITS = (1, 2, 10, 256, 257, 2 ** 40)
NO_CAP = 2 ** 63 - 1
RADII = (0.0, 400.0, np.inf)


def caps_for(limit):
    """1, 2, N - 1, N, N + 1 and 2^63 - 1, cut to the legal range."""
    return sorted({min(max(c, 1), NO_CAP) for c in (1, 2, limit - 1, limit, limit + 1, NO_CAP)})


def categories(seed, n, few=True):
    """One category per row of the place table: five values, or one value per row (caps never bind)."""
    rng = np.random.default_rng(9000 + seed)
    return FEW[rng.integers(0, len(FEW), n)] if few else (10_000 + rng.permutation(n)).astype(np.int64)


def with_allow(case, lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    ids = np.concatenate(lists + [np.empty(0, np.int64)]).astype(np.int64)
    return dict(case, al_offsets=off, al_ids=ids)


def allow_lists(seed, case):
    """Per segment, in turn: empty (every category); one category of the table; an unsorted list that repeats a category and
    names unknown ones; unknown categories only (count 0); every category of the table, reversed."""
    rng = np.random.default_rng(11000 + seed)
    have = np.unique(case["cats"])
    lists = []
    for s in range(len(case["targets"])):
        kind = (seed + s) % 5
        if kind == 0 or len(have) == 0:
            lists.append(np.empty(0, np.int64))
        elif kind == 1:
            lists.append(have[rng.integers(0, len(have), 1)])
        elif kind == 2:
            pick = have[rng.integers(0, len(have), 3)]
            lists.append(rng.permutation(np.concatenate([pick, pick[:2], UNKNOWN[:2]])))
        elif kind == 3:
            lists.append(UNKNOWN.copy())
        else:
            lists.append(have[::-1].copy())
    return lists


def fuzz_case(seed, few=True, allow=True, lists=False, circles=False):
    """rank_batch_cases.fuzz_case(seed) - with lists: rank_exclude_cases'; with circles: rank_near_cases', the radii 0,
    400 m and +inf in turn - plus categories and, with allow, allow-lists.  The caps depend on the limit: with_caps."""
    case = rx.fuzz_case(seed) if lists else rb.fuzz_case(seed)
    if circles:
        case = rn.with_circles(case, seed)
        case["radius"] = np.array([RADII[(seed + s) % len(RADII)] for s in range(len(case["targets"]))])
    case = dict(case, cats=categories(seed, len(case["place_ids"]), few))
    return with_allow(case, allow_lists(seed, case)) if allow else case


def with_caps(case, limit, shift=0):
    """One cap per segment: caps_for(limit) in turn, starting at `shift`."""
    c = caps_for(limit)
    return dict(case, caps=np.array([c[(s + shift) % len(c)] for s in range(len(case["targets"]))], np.int64))


def dominant_case():
    """One segment: 1000 high-scoring rows of category A against 3 low-scoring rows of B, cap 2, N 4 - the answer holds two
    rows of B, which "the N-th best so far" would have pushed out."""
    n = 1003
    place_ids = np.arange(100, 100 + n, dtype=np.int64)
    cats = np.where(np.arange(n) < 1000, 5, 6).astype(np.int64)
    rng = np.random.default_rng(5)
    order = rng.permutation(n)
    scores = np.where(np.arange(n) < 1000, 1000.0 + np.arange(n), np.arange(n) - 999.0)      # A: 1000 .. 1999, B: 1, 2, 3
    return dict(offsets=np.array([0, n], np.int64), ids=place_ids[order], scores=scores[order], place_ids=place_ids,
                regions=np.zeros(n, np.int64), targets=np.zeros(1, np.int64), cats=cats, caps=np.array([2], np.int64))


DOMINANT_N = 4


def ascending_case(n=5000, n_cats=1, cap=2):
    """One segment whose scores ascend with the input row, in n_cats categories: every compaction's survivors are killed by
    the rows that arrive later."""
    place_ids = np.arange(1, n + 1, dtype=np.int64)
    return dict(offsets=np.array([0, n], np.int64), ids=place_ids.copy(), scores=np.arange(n, dtype=np.float64),
                place_ids=place_ids, regions=np.zeros(n, np.int64), targets=np.zeros(1, np.int64),
                cats=(np.arange(n) % n_cats).astype(np.int64), caps=np.array([cap], np.int64))


def seam_case(chunks, cap):
    """rank_batch_cases.seam_case with two interleaved categories (the place id's parity), so a category's top-cap rows
    lie in different chunks."""
    case = rb.seam_case(chunks)
    return dict(case, cats=(case["place_ids"] % 2).astype(np.int64), caps=np.array([cap], np.int64))


def listing_case():
    """Region 4: place 12 is listed twice with different categories (rows 2 and 3: categories 70 and 80) and once more in
    region 5 under category 90; places 10, 11 are of category 70, 13 of 80, 14 of 90.  Scores rise with the id.
    Segment 0: no list; 1: only 80 allowed (12's second listing counts); 2: only 90 (12's listing elsewhere does not
    count); 3: no list, cap 1."""
    place_ids = np.array([10, 11, 12, 12, 13, 14, 12], np.int64)
    regions = np.array([4, 4, 4, 4, 4, 4, 5], np.int64)
    cats = np.array([70, 70, 70, 80, 80, 90, 90], np.int64)
    ids = np.tile(np.arange(10, 15, dtype=np.int64), 4)
    scores = np.tile(np.arange(1.0, 6.0), 4)
    case = dict(offsets=np.arange(0, 21, 5, dtype=np.int64), ids=ids, scores=scores, place_ids=place_ids, regions=regions,
                targets=np.full(4, 4, np.int64), cats=cats,
                caps=np.array([NO_CAP, NO_CAP, NO_CAP, 1], np.int64))
    return with_allow(case, [np.empty(0, np.int64), np.array([80], np.int64), np.array([90], np.int64), np.empty(0, np.int64)])


LISTING_IDS = ([14, 13, 12, 11, 10], [13, 12], [14], [14, 13, 12])     # segment 3: one of 90, one of 80, one of 70 (12, first listing)


def allow_of(case, s):
    return case["al_ids"][case["al_offsets"][s]:case["al_offsets"][s + 1]] if "al_ids" in case else np.empty(0, np.int64)


def passing_rows(case, s, kept=None):
    """The rows of the place table that pass segment s's predicates (target region, circle, allow-list), in input order,
    with their distances (zeros without circles).  kept: rank_near_cases.all_kept's (rows, distances) of the segment."""
    if "radius" in case:
        rows, d = kept
    else:
        rows = rn.region_rows(case, s)
        d = np.zeros(len(rows))
    al = allow_of(case, s)
    if len(al):
        ok = np.isin(case["cats"][rows], al)
        rows, d = rows[ok], d[ok]
    return rows, d


def walk(ids, scores, first_cat, cap, width):
    """The greedy walk over a ranking: a row is taken iff fewer than cap rows of its category were taken before it."""
    used, out = {}, []
    for j, i in enumerate(ids.tolist()):
        if len(out) == width:
            break
        c = first_cat[i]
        if used.get(c, 0) < cap:
            used[c] = used.get(c, 0) + 1
            out.append(j)
    return np.array(out, np.int64)


def expected(rank, case, limit, kept=None):
    """-> (ids[S, W], scores[S, W], meters[S, W], counts[S]): per segment `rank` at limit = segment length on the
    (surviving) rows against the place table cut to the passing listings, then the walk; category and meters from the
    FIRST passing listing of each id.  W is the limit cut to the longest segment before any filter."""
    off, nseg = case["offsets"], len(case["targets"])
    width = rx.width_of(case, limit)
    out_ids, out_scores, out_meters = np.full((nseg, width), -1, np.int64), np.zeros((nseg, width)), np.zeros((nseg, width))
    counts = np.zeros(nseg, np.int64)
    for s in range(nseg):
        ids, scores = case["ids"][off[s]:off[s + 1]], case["scores"][off[s]:off[s + 1]]
        if "ex_ids" in case:
            keep = ~np.isin(ids, rx.list_of(case, s))
            ids, scores = ids[keep], scores[keep]
        rows, d = passing_rows(case, s, kept[s] if kept is not None else None)
        ri, rs = rank(ids, scores, case["place_ids"][rows], case["regions"][rows], int(case["targets"][s]), max(len(ids), 1))
        ri, rs = np.asarray(ri), np.asarray(rs)
        first = {}
        for j, p in enumerate(case["place_ids"][rows].tolist()):
            first.setdefault(p, j)
        cap = int(case["caps"][s]) if "caps" in case else NO_CAP
        take = walk(ri, rs, {p: int(case["cats"][rows[j]]) for p, j in first.items()}, cap, width)
        counts[s] = len(take)
        out_ids[s, :len(take)], out_scores[s, :len(take)] = ri[take], rs[take]
        for w, i in enumerate(ri[take].tolist()):
            out_meters[s, w] = d[first[i]]
    return out_ids, out_scores, out_meters, counts


def same(got, want, meters=True):
    """Equal ids, counts and score bits - and distance bits where the case has circles."""
    gi, gs, gm, gc = got
    wi, ws, wm, wc = want
    if not rb.same((gi, gs, gc), (wi, ws, wc)):
        return False
    if not meters or gm is None:
        return True
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    return np.asarray(gm).shape == wm.shape and np.array_equal(bits(np.asarray(gm)), bits(wm))


def args(case, limit):
    """prep.rank_recommendations_batch_by_category's (positional, keyword) arguments."""
    a = [case[k] for k in ("offsets", "ids", "scores", "place_ids", "regions", "targets")] + [limit, case["cats"]]
    kw = {}
    if "al_ids" in case:
        kw["allowed"] = (case["al_offsets"], case["al_ids"])
    if "caps" in case:
        kw["max_per_category"] = case["caps"]
    if "radius" in case:
        kw["circles"] = tuple(case[k] for k in ("lat", "lon", "clat", "clon", "radius"))
    if "ex_ids" in case:
        kw["excluded"] = (case["ex_offsets"], case["ex_ids"])
    return a, kw


# ---- the block's list procedure and the chunk merge, restated ---------------------------------------------------------------

BUFFER, TILE = 1024, 256


def compact(entries, n, cap):
    """The compaction of the capped list: entries are (key, category) with unique, totally ordered keys.  Order by
    (category, key); kill every entry with `cap` entries of its category in front of it; order the survivors by key; keep
    the best n.  -> (the kept entries, the threshold key or None)."""
    by_cat = sorted(entries, key=lambda e: (e[1], e[0]))
    live = [e for i, e in enumerate(by_cat) if not (i >= cap and by_cat[i - cap][1] == e[1])]
    live.sort(key=lambda e: e[0])
    return live[:n], (live[n - 1][0] if len(live) >= n else None)


def block_list(entries, n, cap, seed):
    """One block over `entries`: arrival in shuffled tiles of 256 (the order inside a tile is the atomics'), a buffer of
    1024 compacted when a tile might not fit, a push dropped when not below the threshold.  -> the final list."""
    rng = np.random.default_rng(seed)
    buf, thr = [], None
    for t0 in range(0, len(entries), TILE):
        if len(buf) > BUFFER - TILE:
            buf, new = compact(buf, n, min(cap, n))
            thr = new if new is not None else thr
        tile = entries[t0:t0 + TILE]
        for j in rng.permutation(len(tile)):
            if thr is None or tile[j][0] < thr:
                buf.append(tile[j])
        assert len(buf) <= BUFFER
    return compact(buf, n, min(cap, n))[0]


def chunked(entries, n, cap, chunk, seed):
    """The segment cut into chunks, each through block_list, the partial lists through block_list again (the merge)."""
    if len(entries) <= chunk:
        return block_list(entries, n, cap, seed)
    parts = [block_list(entries[c:c + chunk], n, cap, seed + 1 + c) for c in range(0, len(entries), chunk)]
    return block_list([e for p in parts for e in p], n, cap, seed)


def greedy(entries, n, cap):
    """The definition: walk the entries in key order, take one iff fewer than cap of its category were taken."""
    used, out = {}, []
    for e in sorted(entries, key=lambda e: e[0]):
        if len(out) == n:
            break
        if used.get(e[1], 0) < cap:
            used[e[1]] = used.get(e[1], 0) + 1
            out.append(e)
    return out
