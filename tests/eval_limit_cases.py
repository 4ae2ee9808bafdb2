"""Cases of the offline evaluation at the limits of its walk, tables and split: first hits behind skipped 64-wide tiles,
cutoffs on the tile seams, cutoffs up to 2^63 - 1, runs of equal relevant ids across the 64-lane steps of the R count,
segment counts around the evaluator's block and radix shapes; visit tables whose (person, place) pairs lie in several
regions, ids and times at the ends of int64, the exits of the split, a table far beyond one block of the device
primitives; and the requests of prep.relevant_lists.  No GPU, no library: the models stay those of eval_cases, the
generators are seeded, and tests/test_eval_limit_cases.py proves that each case holds what it is named for."""
import numpy as np

import eval_cases as ec

I64_MIN, I64_MAX = ec.I64_MIN, ec.I64_MAX
TILE = 64                                                     # positions a step of the evaluator's walk


def _csr(lists):
    offsets = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=offsets[1:])
    return offsets, np.array([int(x) for l in lists for x in l], np.int64)


# ---- the evaluator -------------------------------------------------------------------------------------------------------

LATE_FIRSTS = (63, 64, 65, 127, 128, 191, 199)
SEAM_HITS = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193, 198, 199)
SEAM_COUNTS = (200, 193, 192, 128, 65, 64, 63)
SEAM_CUTOFFS = ([63, 64, 65, 127, 128, 129, 191, 192], [193, 199, 200, 201, 1, 2])
HUGE_CUTOFFS = ([2 ** 31, 2 ** 40, 2 ** 53, 2 ** 62, 2 ** 63 - 1, 65, 64, 1], [7] * 8)
SEGMENT_COUNTS = (2, 3, 4, 5, 64, 128, 129, 256, 257, 1025)
SEGMENT_CUTOFFS = [1, 5, 64, 70]


def late_first_hit(width=200):
    """One full row per first-hit position of LATE_FIRSTS - every tile in front of it is all misses - with up to three
    further hits behind it (as many as the row has room for: none behind 199), and a last row whose hits (130, 150,
    191) all lie in tile 2.  The lists hold strangers too.
    -> (case, cutoff sets of at most eight: [first, first + 1] around each position, and the seams), firsts."""
    assert width >= 200
    firsts = list(LATE_FIRSTS) + [130]
    rec = np.arange(len(firsts) * width, dtype=np.int64).reshape(len(firsts), width) * 3 - 700
    lists = []
    for s, first in enumerate(firsts):
        at = [130, 150, 191] if s == len(LATE_FIRSTS) else [r for r in (first, first + 1, first + 3, first + 40) if r < width]
        lists.append([10 ** 7 + s] + [int(rec[s, r]) for r in reversed(at)] + [10 ** 7 + 100 + s])
    counts = np.full(len(firsts), width, np.int64)
    pairs = [k for first in LATE_FIRSTS for k in (first, first + 1)]
    return (rec, counts) + _csr(lists), [pairs[:8], pairs[8:], [64, 128, 192, 200]], firsts


def seam_cutoffs(width=200):
    """Rows of SEAM_COUNTS ids, each with a relevant id at every position of SEAM_HITS below its count: both sides of
    every tile seam (and of the row's two ends, so that neighbouring cutoffs differ there too).
    -> (case, SEAM_CUTOFFS)."""
    assert width >= 200
    n = len(SEAM_COUNTS)
    rec = np.arange(n * width, dtype=np.int64).reshape(n, width) * 5 - 2000
    counts = np.array(SEAM_COUNTS, np.int64)
    lists = []
    for s in range(n):
        # the ids behind the count are in the list as well: they are never read
        lists.append([int(rec[s, r]) for r in SEAM_HITS[::-1]] + [10 ** 7 + s])
    return (rec, counts) + _csr(lists), [list(c) for c in SEAM_CUTOFFS]


def huge_cutoffs(seed=11):
    """-> (eval_case(seed, 5, 65), HUGE_CUTOFFS): cutoffs from 2^31 to 2^63 - 1 beside 65, 64 and 1, and eight equal."""
    return ec.eval_case(seed, 5, 65), [list(c) for c in HUGE_CUTOFFS]


def duplicate_runs():
    """Three segments of width 70.  List 0 is one id 130 times (R = 1), recommended at position 3 and again at 10; list
    1 is 129 distinct ids, each twice, shuffled; list 2 is 70 times one id and then 70 distinct ones (R = 71).  The rows
    mix their list's ids with strangers.  -> case."""
    rng = np.random.default_rng(5)
    width = 70
    strangers = (10 ** 6 + np.arange(3 * width, dtype=np.int64)).reshape(3, width)
    rec = strangers.copy()
    one = -77
    rec[0, 3] = rec[0, 10] = one
    many = np.arange(129, dtype=np.int64) * 7 - 300
    rec[1, ::2] = rng.permutation(many)[:width // 2]
    head, tail = -5000, np.arange(70, dtype=np.int64) * 3 + 4000             # the run sorts in front of the distinct ids
    rec[2, 1::3] = rng.permutation(tail)[:len(rec[2, 1::3])]
    rec[2, 66] = head
    lists = [[one] * 130, rng.permutation(np.repeat(many, 2)).tolist(), [head] * 70 + tail.tolist()]
    return (rec, np.array([width, width - 1, width], np.int64)) + _csr(lists)


def segment_count_case(n_segments, sparse=False):
    """eval_case(seed, n_segments, 70), to be cut at SEGMENT_CUTOFFS.  sparse: only the segments s % 97 == 0 keep a
    list - eval_case's own where it is not empty, the row's first id where it is - so that the means divide by far
    fewer segments than there are."""
    rec, counts, off, rel = ec.eval_case(4000 + n_segments, n_segments, 70)
    if sparse:
        lists = []
        for s in range(n_segments):
            own = rel[off[s]:off[s + 1]].tolist()
            lists.append([] if s % 97 else own or [int(rec[s, 0])])
        off, rel = _csr(lists)
    return rec, counts, off, rel


def precision_matches(got, hits, k):
    """The restatement of `precision` for one cutoff: hits / k exactly up to 2^53; above it (double)k rounds before the
    division, so the quotient is within one ulp of the correctly rounded hits / k."""
    got, want = np.asarray(got, np.float64), np.array([int(h) / int(k) for h in np.asarray(hits)], np.float64)
    if int(k) <= 2 ** 53:
        return bool(np.array_equal(got, want))
    return bool((np.abs(got - want) <= np.spacing(want)).all())


# ---- the requests' lists -------------------------------------------------------------------------------------------------

def model_relevant_lists(held, persons, regions):
    """The lists of prep.relevant_lists: a dict from (person, region) to the places in held order, read once per
    request.  held: the three columns of the triples.  -> (offsets, ids)."""
    places = {}
    for p, r, place in zip(*(np.asarray(held[k]).tolist() for k in ("person_id", "region_id", "place_id"))):
        places.setdefault((p, r), []).append(place)
    return _csr([places.get((int(p), int(r)), []) for p, r in zip(persons, regions)])


# ---- the hold-out split --------------------------------------------------------------------------------------------------

def _visits(person, ts, place, region):
    place = np.asarray(place, np.int64)
    return {"person_id": np.asarray(person, np.int64), "timestamp": np.asarray(ts, np.int64), "place_id": place,
            "region_id": np.asarray(region, np.int64), "category_id": (place % 7).astype(np.int64)}


def _drawn_visits(seed, n, n_persons, n_places, cut):
    """holdout_case's recipe with the region drawn independently of the place."""
    rng = np.random.default_rng(seed)
    person = rng.integers(-(n_persons // 2), n_persons - n_persons // 2, n).astype(np.int64) * 1_000_003
    place = rng.integers(-5, n_places - 5, n).astype(np.int64)
    region = rng.integers(-1, 2, n).astype(np.int64)
    ts = rng.integers(cut - 50, cut + 50, n).astype(np.int64)
    ts[rng.random(n) < 0.1] = cut
    late = person == person.min()                             # one person is seen only behind the cut
    ts[late] = np.maximum(ts[late], cut)
    return _visits(person, ts, place, region)


def two_region_case(n=3000, seed=21, cut=1000):
    """n visits of 40 persons at 30 places, each visit in one of 3 regions whatever its place: a (person, place) pair
    lies in two and three regions on both sides of the cut.  -> (visits, cut)."""
    return _drawn_visits(seed, n, 40, 30, cut), cut


def multi_block_case(n=70_000, seed=22, cut=1000):
    """The same at n rows of 2,000 persons and 500 places - dense in duplicates, and far beyond what one block of a
    device sort or selection holds.  -> (visits, cut)."""
    return _drawn_visits(seed, n, 2000, 500, cut), cut


EXTREME_CUTS = (I64_MIN, I64_MIN + 1, 0, I64_MAX)


def extreme_ids_case():
    """Hand-made.  Persons, places and regions from {MIN, MIN + 1, -1, 0, MAX - 1, MAX}, timestamps from those, 1 and
    the same ends.  Adjacent persons share places, and for each of the pairs (MIN, MIN + 1), (-1, 0), (MAX - 1, MAX)
    the first has a place behind the cut 0 that lies above all its train places and IS the second's smallest train
    place: a lower bound on (person, place) that forgets the person finds it there.  -1 and MAX - 1 have no row at
    the time MIN, so at the cut MIN + 1 they are unseen persons between seen ones.  -> (visits, EXTREME_CUTS)."""
    a, b, m, z, y, x = I64_MIN, I64_MIN + 1, -1, 0, I64_MAX - 1, I64_MAX
    rows = [  # person, timestamp, place, region
        (a, a, a, a), (a, b, b, z), (a, m, a, x), (a, z, z, m), (a, 1, a, a), (a, y, z, z), (a, x, x, x), (a, z, z, m),
        (b, a, z, z), (b, m, x, a), (b, z, a, m), (b, 1, z, x), (b, x, y, y), (b, b, z, y),
        (m, b, a, z), (m, m, m, m), (m, z, z, a), (m, 1, m, z), (m, y, x, x), (m, x, z, a),
        (z, a, z, b), (z, m, y, y), (z, z, a, a), (z, z, z, z), (z, x, x, m), (z, 1, y, y),
        (y, b, a, a), (y, m, b, b), (y, z, x, x), (y, y, a, y), (y, x, z, z), (y, 1, x, x),
        (x, a, x, x), (x, m, x, y), (x, z, a, z), (x, 1, x, a), (x, x, y, y), (x, x, x, x), (x, y, y, y),
    ]
    order = np.random.default_rng(9).permutation(len(rows))
    cols = np.array([rows[i] for i in order], np.int64)
    return _visits(cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3]), EXTREME_CUTS


def nothing_kept_cases():
    """Tables with train rows and rows behind the cut of which none is kept.
    -> [(visits, cut, new_places_only, kept otherwise)]: (a) the rows behind the cut belong to persons without a train
    row - below, between and above the train persons - in both modes; (b) every (person, place) behind the cut has a
    train visit, under another region: nothing is kept for new places only, everything otherwise."""
    cut = 500
    rng = np.random.default_rng(31)
    seen, unseen = np.array([10, 20, 30], np.int64), np.array([5, 15, 25, 35, 11, 29], np.int64)
    person = np.concatenate([np.repeat(seen, 4), np.repeat(unseen, 3)])
    ts = np.concatenate([rng.integers(0, cut, 12), rng.integers(cut, 2 * cut, 18)])
    place = np.concatenate([np.tile([1, 2, 3, 4], 3), rng.integers(1, 5, 18)])        # the same places on both sides
    a = _visits(person, ts, place, place % 2)
    person = np.repeat(np.array([-3, -2, 7, 8], np.int64), 6)
    place = np.tile(np.array([40, 41, 42, 40, 41, 42], np.int64), 4)
    ts = np.tile(np.array([1, 2, 3, cut, cut + 1, cut + 2], np.int64), 4)
    region = np.tile(np.array([0, 0, 0, 1, 2, 1], np.int64), 4)
    b = _visits(person, ts, place, region)
    return [(a, cut, False, False), (a, cut, True, False), (b, cut, True, True)]


def one_triple_case():
    """500 rows behind the cut of one (person, region, place), and one train row of that person elsewhere.
    -> (visits, cut)."""
    n, cut = 501, 1000
    person = np.full(n, -12345, np.int64)
    ts = cut + (np.arange(n, dtype=np.int64) * 7) % 13
    place, region = np.full(n, 77, np.int64), np.full(n, 2, np.int64)
    ts[250], place[250], region[250] = cut - 1, 78, 3
    return _visits(person, ts, place, region), cut


# ---- the lists' requests -------------------------------------------------------------------------------------------------

LIST_KINDS = ("known", "below", "above", "between", "unknown_region", "unknown_person", "absent_pair")


def lists_case(seed):
    """held: the model's triples of two_region_case(seed) with triples of the extreme ids mixed in (persons MIN + 1 to
    MAX - 1, regions and places to both ends), sorted.  Requests, shuffled: every (person, region) of held, some twice;
    persons below the smallest, above the largest and strictly between two held persons; known persons with an unknown
    region and unknown persons with a known one; known persons and regions that share no triple.
    -> (held, persons, regions, kinds) - kinds names each request's entry of LIST_KINDS."""
    rng = np.random.default_rng(100 + seed)
    v, cut = two_region_case(seed=40 + seed)
    triples = set(ec.model_holdout(v["person_id"], v["timestamp"], v["place_id"], v["region_id"], cut, False)[1])
    ends = [I64_MIN, I64_MIN + 1, -1, 0, I64_MAX - 1, I64_MAX]
    for p in ends[1:5]:
        for r in (ends[int(rng.integers(6))], I64_MIN, I64_MAX):
            for _ in range(int(rng.integers(1, 6))):
                triples.add((p, r, ends[int(rng.integers(6))]))
    cols = np.array(sorted(triples), np.int64)
    held = {"person_id": cols[:, 0].copy(), "region_id": cols[:, 1].copy(), "place_id": cols[:, 2].copy()}
    pairs = sorted({(p, r) for p, r, _ in triples})
    persons, regions = sorted({p for p, _ in pairs}), sorted({r for _, r in pairs})
    gaps = [p + 1 for p, q in zip(persons, persons[1:]) if q - p > 1]
    requests = [(p, r, "known") for p, r in pairs] + [(p, r, "known") for p, r in pairs[::5]]
    requests += [(I64_MIN, r, "below") for r in regions[:3]] + [(I64_MAX, r, "above") for r in regions[-3:]]
    requests += [(gaps[i], regions[i % len(regions)], "between") for i in range(0, len(gaps), 3)]
    requests += [(p, r, "unknown_region") for p in persons[::7] for r in (-2, 2, 5, I64_MAX - 2)]
    requests += [(p, regions[-1 - i], "unknown_person") for i, p in enumerate(gaps[1::3][:3])]
    missing = [(p, r) for p in persons for r in regions if (p, r) not in set(pairs)]
    requests += [(p, r, "absent_pair") for p, r in missing[::11]]
    requests = [requests[i] for i in rng.permutation(len(requests))]
    return (held, np.array([q[0] for q in requests], np.int64), np.array([q[1] for q in requests], np.int64),
            [q[2] for q in requests])
