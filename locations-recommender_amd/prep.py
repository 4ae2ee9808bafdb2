"""The producers of the two hot paths' inputs, computed by liblocrec.so's kernels (csrc/prep.hip,
SURVEY.md 8f rows f-2 and f-4) behind the names of the reference's builder objects:

    calc_ratings                 RatingsBuilder.calcRatings               knn/RatingsBuilder.scala:32-48
    calc_rating_vectors          RatingVectorsBuilder.calcRatingVectors   knn/RatingVectorsBuilder.scala:10-25,52-84
    build_with_balanced_weights  StochasticGraphBuilder.buildWithBalancedWeights
                                                                          stochastic/StochasticGraphBuilder.scala:8-28
    calc_place_visits            PlaceVisits.calcPlaceVisits              PlaceVisits.scala:11-46
    distance_meters              Location.distanceMeters                  Location.scala:30-38
    rank_recommendations         printRecommendations of both mains       knn/KnnRecommenderMain.scala:90-101
    rank_recommendations_batch   ... for every segment of a batch's rows   (the same lines, per person)
    rank_recommendations_batch_excluding   ... leaving out a list of ids per segment (no counterpart: only new places)
    rank_recommendations_batch_near        ... within a radius of a centre per segment (no counterpart: within reach)
    rank_recommendations_batch_by_category ... with an allow-list of categories and a cap per category (no counterpart)
    calc_person_likes_place_edges / calc_person_likes_category_edges / calc_category_selected_place_edges
                                 the three counted edge families          stochastic/PersonLikesPlace.scala:12-37 (and siblings)
    calc_place_similar_place_edges  PlaceSimilarPlace.calcPlaceSimilarPlaceEdges
                                                                          stochastic/PlaceSimilarPlace.scala:18-63
    generate_stochastic_graph    StochasticGraphBuilderMain.generateStochasticGraph
                                                                          stochastic/StochasticGraphBuilderMain.scala:47-66
    max_timestamp / visits_from_timestamp   PlaceVisits.calcVisitsFromTimestamp   PlaceVisits.scala:50-61
    extract_region_ids           PlaceVisits.extractRegionIds             PlaceVisits.scala:69-78
    region_sets / RegionSetPlan  PlaceVisits.extractRegionsPlaceVisits    PlaceVisits.scala:63-67,80-87
    knn_indexes_by_region_set / sg_graphs_by_region_set   the per-set loops of both builder mains

Every function takes numpy arrays (host in, host out) or torch CUDA tensors (device in, device out:
nothing passes through the host, and the outputs of calc_rating_vectors go straight into
KnnIndex.from_device).  There is no CPU fallback: without the HIP library / a GPU they raise.
"""
import ctypes as C

import numpy as np

from . import _lib as L

DISTANCE_ACCURACY_METERS = 100.0   # PlaceVisits.scala:127
VISITED_PLACES_TOP_N = 100         # RatingsBuilder.scala:9
VISITED_CATEGORIES_TOP_N = 10      # RatingsBuilder.scala:10
# the stochastic graph's edge families
LIKED_PLACES_TOP_N = 100           # stochastic/PersonLikesPlace.scala:10
LIKED_CATEGORIES_TOP_N = 100       # stochastic/PersonLikesCategory.scala:10
SELECTED_PLACES_TOP_N = 100        # stochastic/CategorySelectedPlace.scala:10
SIMILAR_PLACES_TOP_N = 50          # stochastic/PlaceSimilarPlace.scala:16
PLACE_SIMILARITY_INTERVAL_MS = 7 * 86_400_000   # stochastic/PlaceSimilarPlace.scala:13-14
BETA_PLACE_PLACE = 1.0             # stochastic/StochasticGraphBuilderMain.scala:8
BETA_CATEGORY_PLACE = 1.0          # stochastic/StochasticGraphBuilderMain.scala:9


def _is_tensor(a):
    return type(a).__module__.startswith("torch") and hasattr(a, "data_ptr")


class _Cols:
    """Columns of one call, all host (numpy) or all device (torch CUDA tensors)."""

    def __init__(self, *arrays):
        self.device = any(_is_tensor(a) for a in arrays)
        if self.device:
            import torch
            self.torch = torch
            assert all(_is_tensor(a) and a.is_cuda for a in arrays), "all columns must be CUDA tensors (or all numpy)"
            self.dev = arrays[0].device
            L.require_current_device(arrays)
            torch.cuda.current_stream(self.dev).synchronize()   # the library works on its own stream
        self.mem = L.MEM_DEVICE if self.device else L.MEM_HOST
        self._keep = []

    def col(self, a, np_dtype):
        if self.device:
            want = getattr(self.torch, np.dtype(np_dtype).name)
            a = a.to(want).contiguous()
            self._keep.append(a)
            return C.c_void_p(a.data_ptr()) if a.numel() else None
        a = np.ascontiguousarray(a, np_dtype)
        self._keep.append(a)
        return C.c_void_p(a.ctypes.data) if a.size else None

    def out(self, n, np_dtype):
        n = max(int(n), 1)
        if self.device:
            a = self.torch.empty(n, dtype=getattr(self.torch, np.dtype(np_dtype).name), device=self.dev)
            return a, C.c_void_p(a.data_ptr())
        a = np.empty(n, np_dtype)
        return a, C.c_void_p(a.ctypes.data)


def calc_ratings(person_ids, entity_ids, top_n):
    """RatingsBuilder.calcRatings: visits -> (person_id, entity_id, rating = number of visits), keeping
    per person the entities whose SQL rank() by rating descending is <= top_n (ties share a rank: a tie
    straddling top_n is kept whole).  Rows ordered by (person, entity)."""
    c = _Cols(person_ids, entity_ids)
    n = len(person_ids)
    assert len(entity_ids) == n
    p, e = c.col(person_ids, np.int64), c.col(entity_ids, np.int64)
    (op, opp), (oe, oep), (orr, orp) = c.out(n, np.int64), c.out(n, np.int64), c.out(n, np.int64)
    cnt = C.c_int64()
    L.check(L.lib().locrec_calc_ratings(n, p, e, int(top_n), c.mem, opp, oep, orp, C.byref(cnt)))
    m = cnt.value
    return op[:m], oe[:m], orr[:m]


def calc_rating_vectors(person_ids, entity_ids, ratings):
    """RatingVectorsBuilder.calcRatingVectors: one SparseVector per person as CSR.
    -> person_ids (ascending), rowptr, indices (int32, ascending per person), values (float64), size."""
    c = _Cols(person_ids, entity_ids, ratings)
    n = len(person_ids)
    assert len(entity_ids) == n and len(ratings) == n
    p, e, r = c.col(person_ids, np.int64), c.col(entity_ids, np.int64), c.col(ratings, np.int64)
    (oid, oidp), (optr, optrp) = c.out(n, np.int64), c.out(n + 1, np.int64)
    (oidx, oidxp), (oval, ovalp) = c.out(n, np.int32), c.out(n, np.float64)
    npers, nnz, size = C.c_int64(), C.c_int64(), C.c_int64()
    L.check(L.lib().locrec_calc_rating_vectors(n, p, e, r, c.mem, oidp, optrp, oidxp, ovalp, C.byref(npers), C.byref(nnz),
                                               C.byref(size)))
    return oid[:npers.value], optr[:npers.value + 1], oidx[:nnz.value], oval[:nnz.value], int(size.value)


def build_with_balanced_weights(betas, all_edges):
    """StochasticGraphBuilder.buildWithBalancedWeights: every family's weight times its beta, families
    concatenated in the given order.  all_edges: (source_id, target_id, weight) triples or mappings with
    those keys.  -> (source_id, target_id, balanced_weight)."""
    fams = []
    for e in all_edges:
        fams.append((e["source_id"], e["target_id"], e["weight"]) if hasattr(e, "keys") or hasattr(e, "columns") else tuple(e))
    if len(betas) != len(fams) or not fams:
        raise L.IllegalArgumentException("one beta per edge family is required")
    c = _Cols(*[a for f in fams for a in f])
    nf = len(fams)
    counts = (C.c_int64 * nf)(*[len(f[0]) for f in fams])
    b = (C.c_double * nf)(*[float(x) for x in betas])
    src, dst, w = (C.c_void_p * nf)(), (C.c_void_p * nf)(), (C.c_void_p * nf)()
    for i, f in enumerate(fams):
        assert len(f[1]) == len(f[0]) and len(f[2]) == len(f[0])
        src[i], dst[i], w[i] = c.col(f[0], np.int64), c.col(f[1], np.int64), c.col(f[2], np.float64)
    total = sum(counts)
    (os_, osp), (ot, otp), (ow, owp) = c.out(total, np.int64), c.out(total, np.int64), c.out(total, np.float64)
    L.check(L.lib().locrec_build_balanced_edges(nf, b, counts, src, dst, w, c.mem, osp, otp, owp))
    return os_[:total], ot[:total], ow[:total]


def calc_place_visits(visits, places, visits_from, max_meters=DISTANCE_ACCURACY_METERS):
    """PlaceVisits.calcPlaceVisits.  visits: mapping with person_id, timestamp (int64), latitude,
    longitude, region_id; places: mapping with id, latitude, longitude, region_id, category_id;
    visits_from: the timestamp calcVisitsFromTimestamp yields (PlaceVisits.scala:48-58).
    -> dict(person_id, timestamp, place_id, region_id, category_id), ordered by (visit row, place row)."""
    vcols = [visits[k] for k in ("person_id", "timestamp", "latitude", "longitude", "region_id")]
    pcols = [places[k] for k in ("id", "latitude", "longitude", "region_id", "category_id")]
    c = _Cols(*vcols, *pcols)
    nv, npl = len(vcols[0]), len(pcols[0])
    va = [c.col(vcols[0], np.int64), c.col(vcols[1], np.int64), c.col(vcols[2], np.float64), c.col(vcols[3], np.float64),
          c.col(vcols[4], np.int64)]
    pa = [c.col(pcols[0], np.int64), c.col(pcols[1], np.float64), c.col(pcols[2], np.float64), c.col(pcols[3], np.int64),
          c.col(pcols[4], np.int64)]
    cnt = C.c_int64(0)   # first call: count only
    L.check(L.lib().locrec_calc_place_visits(nv, *va, npl, *pa, int(visits_from), float(max_meters), c.mem,
                                             None, None, None, None, None, C.byref(cnt)))
    m = cnt.value
    outs = [c.out(m, np.int64) for _ in range(5)]
    cnt = C.c_int64(m)
    if m:
        L.check(L.lib().locrec_calc_place_visits(nv, *va, npl, *pa, int(visits_from), float(max_meters), c.mem,
                                                 *[o[1] for o in outs], C.byref(cnt)))
    names = ("person_id", "timestamp", "place_id", "region_id", "category_id")
    return {k: o[0][:m] for k, o in zip(names, outs)}


def distance_meters(lat1, lon1, lat2, lon2):
    """Location.distanceMeters of n pairs, by the device code the join uses (NaN for an invalid Location)."""
    c = _Cols(lat1, lon1, lat2, lon2)
    n = len(lat1)
    a = [c.col(x, np.float64) for x in (lat1, lon1, lat2, lon2)]
    out, outp = c.out(n, np.float64)
    L.check(L.lib().locrec_distance_meters(n, *a, c.mem, outp))
    return out[:n]


def rank_recommendations(ids, scores, place_ids, place_region_ids, target_region_id, max_recommendations):
    """printRecommendations of both mains (KnnRecommenderMain.scala:90-101, StochasticRecommenderMain.scala:
    64-75): the target region's places JOIN the recommendations ON id, ORDER BY score DESC, LIMIT n.
    Ties: id ascending (Spark leaves them undefined).  -> (ids, scores)."""
    c = _Cols(ids, scores, place_ids, place_region_ids)
    n, npl = len(ids), len(place_ids)
    assert len(scores) == n and len(place_region_ids) == npl
    a = [c.col(ids, np.int64), c.col(scores, np.float64)]
    p = [c.col(place_ids, np.int64), c.col(place_region_ids, np.int64)]
    cap = max(0, min(n, int(max_recommendations)))
    (oi, oip), (osc, oscp) = c.out(cap, np.int64), c.out(cap, np.float64)
    cnt = C.c_int64()
    L.check(L.lib().locrec_rank_recommendations(n, a[0], a[1], npl, p[0], p[1], int(target_region_id), int(max_recommendations),
                                                c.mem, oip, oscp, C.byref(cnt)))
    return oi[:cnt.value], osc[:cnt.value]


RANK_BATCH_STATS = ("one_block", "split", "chunks", "sorted", "membership_form", "host_assembled", "host_syncs")


def rank_recommendations_batch(offsets, ids, scores, place_ids, place_region_ids, target_region_ids, max_recommendations):
    """rank_recommendations for many row ranges of one (ids, scores) pair at once (locrec_rank_recommendations_batch):
    segment s is rows offsets[s]:offsets[s + 1] and is ranked for target_region_ids[s].
    -> (ids[S, W], scores[S, W], counts[S]); row s holds counts[s] rows, then id -1 / score 0.0.  W is
    max_recommendations, cut to the longest segment (no segment can return more)."""
    if not _is_tensor(offsets):
        offsets = np.asarray(offsets, np.int64)
    c = _Cols(offsets, ids, scores, place_ids, place_region_ids, target_region_ids)
    nseg, n, npl = len(target_region_ids), len(ids), len(place_ids)
    assert len(offsets) == nseg + 1 and len(scores) == n and len(place_region_ids) == npl
    longest = int((offsets[1:] - offsets[:-1]).max()) if nseg else 0
    width = max(0, min(int(max_recommendations), longest, n))
    o = c.col(offsets, np.int64)
    a = [c.col(ids, np.int64), c.col(scores, np.float64)]
    p = [c.col(place_ids, np.int64), c.col(place_region_ids, np.int64)]
    t = c.col(target_region_ids, np.int64)
    (oi, oip), (osc, oscp), (oc, ocp) = c.out(nseg * width, np.int64), c.out(nseg * width, np.float64), c.out(nseg, np.int64)
    L.check(L.lib().locrec_rank_recommendations_batch(nseg, o, n, a[0], a[1], npl, p[0], p[1], t, width, c.mem, oip, oscp, ocp))
    if nseg == 0 or width == 0:
        oc[:nseg] = 0
    return oi[:nseg * width].reshape(nseg, width), osc[:nseg * width].reshape(nseg, width), oc[:nseg]


def rank_recommendations_batch_excluding(offsets, ids, scores, place_ids, place_region_ids, target_region_ids,
                                         max_recommendations, excluded_offsets, excluded_ids):
    """rank_recommendations_batch that leaves out, per segment, the ids of a list
    (locrec_rank_recommendations_batch_excluding): segment s ranks its rows whose id is not in
    excluded_ids[excluded_offsets[s]:excluded_offsets[s + 1]].  Host or device arrays, all of one kind; the result has
    rank_recommendations_batch's layout, and W is cut to the longest segment as there."""
    if not _is_tensor(offsets):
        offsets = np.asarray(offsets, np.int64)
    c = _Cols(offsets, ids, scores, place_ids, place_region_ids, target_region_ids, excluded_offsets, excluded_ids)
    nseg, n, npl, nex = len(target_region_ids), len(ids), len(place_ids), len(excluded_ids)
    assert len(offsets) == nseg + 1 and len(scores) == n and len(place_region_ids) == npl and len(excluded_offsets) == nseg + 1
    longest = int((offsets[1:] - offsets[:-1]).max()) if nseg else 0
    width = max(0, min(int(max_recommendations), longest, n))
    o = c.col(offsets, np.int64)
    a = [c.col(ids, np.int64), c.col(scores, np.float64)]
    p = [c.col(place_ids, np.int64), c.col(place_region_ids, np.int64)]
    t = c.col(target_region_ids, np.int64)
    x = [c.col(excluded_offsets, np.int64), c.col(excluded_ids, np.int64)]
    (oi, oip), (osc, oscp), (oc, ocp) = c.out(nseg * width, np.int64), c.out(nseg * width, np.float64), c.out(nseg, np.int64)
    L.check(L.lib().locrec_rank_recommendations_batch_excluding(nseg, o, n, a[0], a[1], npl, p[0], p[1], t, width, x[0], nex, x[1],
                                                                c.mem, oip, oscp, ocp))
    if nseg == 0 or width == 0:
        oc[:nseg] = 0
    return oi[:nseg * width].reshape(nseg, width), osc[:nseg * width].reshape(nseg, width), oc[:nseg]


def rank_recommendations_batch_near(offsets, ids, scores, place_ids, place_region_ids, place_latitudes, place_longitudes,
                                    target_region_ids, center_latitudes, center_longitudes, radius_meters,
                                    max_recommendations, excluded_offsets=None, excluded_ids=None):
    """rank_recommendations_batch within reach (locrec_rank_recommendations_batch_near): segment s ranks its rows whose
    id is a place of target_region_ids[s] with a listing there no further than radius_meters[s] (>= 0 or +inf) from
    (center_latitudes[s], center_longitudes[s]) by distance_meters - and, with excluded_offsets / excluded_ids, whose id
    is not in its list (rank_recommendations_batch_excluding's).  Host or device arrays, all of one kind.
    -> (ids[S, W], scores[S, W], meters[S, W], counts[S]): rank_recommendations_batch's layout, meters the distance of
    each row's first listing inside the circle (padding 0.0)."""
    if not _is_tensor(offsets):
        offsets = np.asarray(offsets, np.int64)
    lists = excluded_offsets is not None
    cols = [offsets, ids, scores, place_ids, place_region_ids, place_latitudes, place_longitudes, target_region_ids,
            center_latitudes, center_longitudes, radius_meters] + ([excluded_offsets, excluded_ids] if lists else [])
    c = _Cols(*cols)
    nseg, n, npl = len(target_region_ids), len(ids), len(place_ids)
    assert len(offsets) == nseg + 1 and len(scores) == n and len(place_region_ids) == npl
    assert len(place_latitudes) == npl and len(place_longitudes) == npl
    assert len(center_latitudes) == nseg and len(center_longitudes) == nseg and len(radius_meters) == nseg
    assert not lists or len(excluded_offsets) == nseg + 1
    longest = int((offsets[1:] - offsets[:-1]).max()) if nseg else 0
    width = max(0, min(int(max_recommendations), longest, n))
    o = c.col(offsets, np.int64)
    a = [c.col(ids, np.int64), c.col(scores, np.float64)]
    p = [c.col(place_ids, np.int64), c.col(place_region_ids, np.int64), c.col(place_latitudes, np.float64),
         c.col(place_longitudes, np.float64)]
    t = c.col(target_region_ids, np.int64)
    q = [c.col(x, np.float64) for x in (center_latitudes, center_longitudes, radius_meters)]
    x = [c.col(excluded_offsets, np.int64), c.col(excluded_ids, np.int64)] if lists else [None, None]
    (oi, oip), (osc, oscp), (om, omp), (oc, ocp) = (c.out(nseg * width, np.int64), c.out(nseg * width, np.float64),
                                                    c.out(nseg * width, np.float64), c.out(nseg, np.int64))
    L.check(L.lib().locrec_rank_recommendations_batch_near(nseg, o, n, a[0], a[1], npl, *p, t, *q, width, x[0],
                                                           len(excluded_ids) if lists else 0, x[1], c.mem, oip, oscp, omp, ocp))
    if nseg == 0 or width == 0:
        oc[:nseg] = 0
    shape = (nseg, width)
    return oi[:nseg * width].reshape(shape), osc[:nseg * width].reshape(shape), om[:nseg * width].reshape(shape), oc[:nseg]


def rank_recommendations_batch_by_category(offsets, ids, scores, place_ids, place_region_ids, target_region_ids,
                                           max_recommendations, place_category_ids, allowed=None, max_per_category=None,
                                           circles=None, excluded=None):
    """rank_recommendations_batch by category (locrec_rank_recommendations_batch_by_category): place_category_ids gives
    the category of every row of the place table; allowed=(offsets, category_ids) is one allow-list per segment (CSR; an
    empty list allows every category); max_per_category[s] >= 1 caps the rows of one category in segment s's output - a
    row is eligible iff fewer than the cap kept rows of its category precede it in the order (score desc, id asc, input
    row asc), and the output is the first max_recommendations eligible rows.  circles=(place_latitudes,
    place_longitudes, center_latitudes, center_longitudes, radius_meters) adds rank_recommendations_batch_near's circles,
    excluded=(offsets, ids) rank_recommendations_batch_excluding's lists.  A place listed several times in the target
    region passes if some listing passes every predicate given; the first passing listing in input order gives the
    category and the distance.  Host or device arrays, all of one kind.
    -> (ids[S, W], scores[S, W], meters[S, W] or None without circles, counts[S]) in rank_recommendations_batch's layout."""
    if not _is_tensor(offsets):
        offsets = np.asarray(offsets, np.int64)
    groups = [g for g in (allowed, circles, excluded) if g is not None]
    cols = [offsets, ids, scores, place_ids, place_region_ids, target_region_ids, place_category_ids]
    cols += [x for g in groups for x in g] + ([max_per_category] if max_per_category is not None else [])
    c = _Cols(*cols)
    nseg, n, npl = len(target_region_ids), len(ids), len(place_ids)
    assert len(offsets) == nseg + 1 and len(scores) == n and len(place_region_ids) == npl and len(place_category_ids) == npl
    assert allowed is None or len(allowed[0]) == nseg + 1
    assert excluded is None or len(excluded[0]) == nseg + 1
    assert max_per_category is None or len(max_per_category) == nseg
    assert circles is None or ([len(x) for x in circles] == [npl, npl, nseg, nseg, nseg])
    longest = int((offsets[1:] - offsets[:-1]).max()) if nseg else 0
    width = max(0, min(int(max_recommendations), longest, n))
    o = c.col(offsets, np.int64)
    a = [c.col(ids, np.int64), c.col(scores, np.float64)]
    p = [c.col(place_ids, np.int64), c.col(place_region_ids, np.int64)]
    pc = c.col(place_category_ids, np.int64)
    t = c.col(target_region_ids, np.int64)
    q = [c.col(x, np.float64) for x in circles] if circles is not None else [None] * 5
    x = [c.col(excluded[0], np.int64), c.col(excluded[1], np.int64)] if excluded is not None else [None, None]
    al = [c.col(allowed[0], np.int64), c.col(allowed[1], np.int64)] if allowed is not None else [None, None]
    caps = c.col(max_per_category, np.int64) if max_per_category is not None else None
    (oi, oip), (osc, oscp), (oc, ocp) = c.out(nseg * width, np.int64), c.out(nseg * width, np.float64), c.out(nseg, np.int64)
    om, omp = c.out(nseg * width, np.float64) if circles is not None else (None, None)
    L.check(L.lib().locrec_rank_recommendations_batch_by_category(
        nseg, o, n, a[0], a[1], npl, p[0], p[1], q[0], q[1], pc, t, q[2], q[3], q[4], width,
        x[0], len(excluded[1]) if excluded is not None else 0, x[1],
        al[0], len(allowed[1]) if allowed is not None else 0, al[1], caps, c.mem, oip, oscp, omp, ocp))
    if nseg == 0 or width == 0:
        oc[:nseg] = 0
    shape = (nseg, width)
    return (oi[:nseg * width].reshape(shape), osc[:nseg * width].reshape(shape),
            om[:nseg * width].reshape(shape) if om is not None else None, oc[:nseg])


def rank_recommendations_batch_stats():
    """What the last ranked batch of this thread did (locrec_rank_recommendations_batch_stats), as a dict."""
    v = [C.c_int64() for _ in RANK_BATCH_STATS]
    L.check(L.lib().locrec_rank_recommendations_batch_stats(*[C.byref(x) for x in v]))
    return dict(zip(RANK_BATCH_STATS, (x.value for x in v)))


def knn_index_from_visits(person_ids, place_ids, category_ids, places_top_n=VISITED_PLACES_TOP_N,
                          categories_top_n=VISITED_CATEGORIES_TOP_N):
    """RatingVectorsBuilderMain's pipeline (RatingVectorsBuilderMain.scala:38-73) on the device: place
    visits (person_id, place_id, category_id) -> place / category ratings -> rating vectors -> KnnIndex,
    with placeRatings = the place ratings.  With CUDA tensors nothing passes through the host."""
    from .knn import KnnIndex
    pp, pe, pr = calc_ratings(person_ids, place_ids, places_top_n)
    cp, ce, cr = calc_ratings(person_ids, category_ids, categories_top_n)
    ids, p_ptr, p_idx, p_val, p_dim = calc_rating_vectors(pp, pe, pr)
    ids_c, c_ptr, c_idx, c_val, c_dim = calc_rating_vectors(cp, ce, cr)
    # both sets come from the same visits, so they name the same persons (every visit has a place and a category)
    same = len(ids) == len(ids_c) and bool((ids == ids_c).all())
    if not same:
        raise L.IllegalArgumentException("place and category visits name different persons")
    if _is_tensor(ids):
        return KnnIndex.from_device(ids, p_ptr.contiguous(), p_idx.contiguous(), p_val.contiguous(), p_dim,
                                    c_ptr.contiguous(), c_idx.contiguous(), c_val.contiguous(), c_dim,
                                    p_ptr.contiguous(), pe.contiguous(), pr.contiguous())
    return KnnIndex(ids, p_ptr, p_idx, p_val, p_dim, c_ptr, c_idx, c_val, c_dim, p_ptr, pe, pr)


def visitor_vectors(visitor_ids, place_ids, category_ids, places_top_n=VISITED_PLACES_TOP_N,
                    categories_top_n=VISITED_CATEGORIES_TOP_N):
    """The same pipeline for visitors - persons an index does not hold (KnnIndex.visitors_*): their place visits
    (visitor_id, place_id, category_id) -> calc_ratings -> calc_rating_vectors, device in, device out.
    -> (visitor ids ascending, (p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val), (rated_offsets, rated_place_ids)):
    the CSR vectors a visitors call takes (a vector index is the entity id itself) and each visitor's rated place ids,
    the exclusion lists of "only new places"."""
    pp, pe, pr = calc_ratings(visitor_ids, place_ids, places_top_n)
    cp, ce, cr = calc_ratings(visitor_ids, category_ids, categories_top_n)
    ids, p_ptr, p_idx, p_val, _ = calc_rating_vectors(pp, pe, pr)
    ids_c, c_ptr, c_idx, c_val, _ = calc_rating_vectors(cp, ce, cr)
    if not (len(ids) == len(ids_c) and bool((ids == ids_c).all())):
        raise L.IllegalArgumentException("place and category visits name different persons")
    cont = (lambda a: a.contiguous()) if _is_tensor(ids) else np.ascontiguousarray
    # the rating rows are ordered by (person, place), one per entry of the place vector: the vector's row pointers
    return ids, tuple(cont(a) for a in (p_ptr, p_idx, p_val, c_ptr, c_idx, c_val)), (cont(p_ptr), cont(pe))


# ---- the stochastic graph from place visits (StochasticGraphBuilderMain.scala:47-66) ----------------------

def calc_count_edges(source_ids, target_ids, top_n):
    """One counted edge family: count per (source, target), SQL rank() by count descending within the
    source, keep rank <= top_n (ties kept whole), weight = count / the source's total of KEPT counts.
    -> (source_id, target_id, weight), ordered by (source, target): the rows of calc_ratings, weighted."""
    c = _Cols(source_ids, target_ids)
    n = len(source_ids)
    assert len(target_ids) == n
    a, b = c.col(source_ids, np.int64), c.col(target_ids, np.int64)
    (os_, osp), (ot, otp), (ow, owp) = c.out(n, np.int64), c.out(n, np.int64), c.out(n, np.float64)
    cnt = C.c_int64()
    L.check(L.lib().locrec_calc_count_edges(n, a, b, int(top_n), c.mem, osp, otp, owp, C.byref(cnt)))
    m = cnt.value
    return os_[:m], ot[:m], ow[:m]


def calc_similar_place_edges(person_ids, place_ids, timestamps, interval=PLACE_SIMILARITY_INTERVAL_MS,
                             top_n=SIMILAR_PLACES_TOP_N):
    """PlaceSimilarPlace.calcPlaceSimilarPlaceEdges: every ordered pair of visit rows of one person at two
    different places at most `interval` apart (in the timestamps' unit) counts for (place, that place); then
    rank / keep / normalise per source place as calc_count_edges.  -> (source_id, target_id, weight), ordered
    by (source, target)."""
    c = _Cols(person_ids, place_ids, timestamps)
    n = len(person_ids)
    assert len(place_ids) == n and len(timestamps) == n
    cols = [c.col(person_ids, np.int64), c.col(place_ids, np.int64), c.col(timestamps, np.int64)]
    cap = 1 << 20   # most results fit a first guess; the count says when a second, exact call is needed
    while True:
        (os_, osp), (ot, otp), (ow, owp) = c.out(cap, np.int64), c.out(cap, np.int64), c.out(cap, np.float64)
        cnt = C.c_int64(cap)
        L.check(L.lib().locrec_calc_similar_place_edges(n, *cols, int(interval), int(top_n), c.mem, osp, otp, owp,
                                                        C.byref(cnt)))
        m = cnt.value
        if m <= cap:
            return os_[:m], ot[:m], ow[:m]
        cap = m


def similar_place_edges_stats():
    """What this thread's last calc_similar_place_edges did: candidate pairs, chunks, and HIP-event milliseconds
    of its sort / emit / merge phases (locrec_similar_place_edges_stats)."""
    pairs, chunks = C.c_int64(), C.c_int64()
    ms = [C.c_double() for _ in range(3)]
    L.check(L.lib().locrec_similar_place_edges_stats(C.byref(pairs), C.byref(chunks), *[C.byref(x) for x in ms]))
    return dict(pairs=pairs.value, chunks=chunks.value, sort_ms=ms[0].value, emit_ms=ms[1].value, merge_ms=ms[2].value)


def _edges(cols):
    return dict(zip(("source_id", "target_id", "weight"), cols))


def calc_person_likes_place_edges(place_visits, top_n=LIKED_PLACES_TOP_N):
    """PersonLikesPlace.calcPersonLikesPlaceEdges (stochastic/PersonLikesPlace.scala:12-37)."""
    return _edges(calc_count_edges(place_visits["person_id"], place_visits["place_id"], top_n))


def calc_person_likes_category_edges(place_visits, top_n=LIKED_CATEGORIES_TOP_N):
    """PersonLikesCategory.calcPersonLikesCategoryEdges (stochastic/PersonLikesCategory.scala:12-37)."""
    return _edges(calc_count_edges(place_visits["person_id"], place_visits["category_id"], top_n))


def calc_category_selected_place_edges(place_visits, top_n=SELECTED_PLACES_TOP_N):
    """CategorySelectedPlace.calcCategorySelectedPlaceEdges (stochastic/CategorySelectedPlace.scala:12-37)."""
    return _edges(calc_count_edges(place_visits["category_id"], place_visits["place_id"], top_n))


def calc_place_similar_place_edges(place_visits, interval=PLACE_SIMILARITY_INTERVAL_MS, top_n=SIMILAR_PLACES_TOP_N):
    """PlaceSimilarPlace.calcPlaceSimilarPlaceEdges (stochastic/PlaceSimilarPlace.scala:18-63)."""
    return _edges(calc_similar_place_edges(place_visits["person_id"], place_visits["place_id"], place_visits["timestamp"],
                                           interval, top_n))


def generate_stochastic_graph(place_visits, beta_person_place, beta_person_category):
    """StochasticGraphBuilderMain.generateStochasticGraph (:47-66): the four edge families of the place visits
    of one region (or region pair) in the reference's order - place-place, category-place, person-place,
    person-category - balanced with the betas (1.0, 1.0, beta_person_place, beta_person_category).
    place_visits: the mapping calc_place_visits returns.  -> (source_id, target_id, balanced_weight); with
    CUDA tensors nothing passes through the host."""
    families = [calc_place_similar_place_edges(place_visits), calc_category_selected_place_edges(place_visits),
                calc_person_likes_place_edges(place_visits), calc_person_likes_category_edges(place_visits)]
    betas = [BETA_PLACE_PLACE, BETA_CATEGORY_PLACE, float(beta_person_place), float(beta_person_category)]
    return build_with_balanced_weights(betas, families)


def visitor_edges(visitor_ids, place_ids, category_ids, beta_person_place, beta_person_category, graph=None):
    """The out-edges of visitors - persons a graph has no vertex for (SgGraph.visitors_*) - from their place visits
    (visitor_id, place_id, category_id), one row a visit: the person -> place and person -> category families of
    generate_stochastic_graph (calc_count_edges with the builder's top-N constants), balanced with their betas by
    build_with_balanced_weights - the values a person of the graph gets - and merged per visitor, places first.
    graph: an SgGraph; a visit to a place the graph has no live vertex for is dropped before the places are counted, a
    visit to such a category before the categories are (an edge may only point at a live vertex).
    -> (visitor ids ascending, edge_offsets[nv + 1], target_ids, balanced_weights, dropped[nv, 2]): host arrays; dropped
    counts the visit rows left out of the place and of the category family.  A visitor all of whose visits are dropped
    keeps its position, without edges (a visitors call refuses it)."""
    host = lambda a: np.asarray(a.cpu().numpy() if _is_tensor(a) else a, np.int64)
    v, p, c = host(visitor_ids), host(place_ids), host(category_ids)
    if not (len(v) == len(p) == len(c)):
        raise L.IllegalArgumentException("visit columns of different lengths")
    ids = np.unique(v)
    dropped = np.zeros((len(ids), 2), np.int64)
    families = []
    for k, (targets, top_n) in enumerate(((p, LIKED_PLACES_TOP_N), (c, LIKED_CATEGORIES_TOP_N))):
        keep = np.ones(len(v), bool) if graph is None else graph.vertex_kinds(targets) == 2
        dropped[:, k] = np.bincount(np.searchsorted(ids, v[~keep]), minlength=len(ids))
        families.append(calc_count_edges(v[keep], targets[keep], top_n))
    s, t, w = build_with_balanced_weights([float(beta_person_place), float(beta_person_category)], families)
    order = np.argsort(s, kind="stable")  # per visitor: its places by id, then its categories by id
    offsets = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(np.bincount(np.searchsorted(ids, s), minlength=len(ids)), out=offsets[1:])
    return ids, offsets, np.ascontiguousarray(t[order]), np.ascontiguousarray(w[order]), dropped


def sg_graph_from_visits(place_visits, beta_person_place, beta_person_category):
    """Place visits -> the four edge families -> balanced edge list -> SgGraph: the SG counterpart of
    knn_index_from_visits.  With CUDA tensors the edge list stays in device memory and the graph's layout is built
    from it by kernels (SgGraph.from_device): nothing passes through the host.  With numpy arrays the list comes
    back to the host and goes through SgGraph (locrec_sg_create)."""
    from .stochastic import SgGraph
    s, t, w = generate_stochastic_graph(place_visits, beta_person_place, beta_person_category)
    if _is_tensor(s):
        return SgGraph.from_device(s.contiguous(), t.contiguous(), w.contiguous())
    return SgGraph(s, t, w)


# ---- every region set of the builder mains from one place-visit table (csrc/region_sets.hip) -------------------

PLACE_VISIT_COLUMNS = ("person_id", "timestamp", "place_id", "region_id", "category_id")   # PlaceVisits.scala:40-46


# ---- offline evaluation (csrc/eval.hip; the reference has no counterpart) ---------------------------------------

EVAL_MAX_CUTOFFS = 8
EVAL_METRICS = ("precision", "recall", "rr", "ap", "ndcg")            # the last axis of `metrics`
EVAL_MEANS = EVAL_METRICS + ("hit_rate",)                             # the columns of `means`
EVAL_STATS = ("table_entries", "evaluated", "host_syncs", "path")
HELD_COLUMNS = ("person_id", "region_id", "place_id")


def holdout_split(place_visits, cut_timestamp, new_places_only=True):
    """A visit table (calc_place_visits' mapping) cut at a time (locrec_holdout_split).
    -> (train_place_visits, held): the five columns of the rows with timestamp < cut_timestamp in input order, and
    dict(person_id, region_id, place_id) - the distinct triples among the rows at or behind the cut whose person has a
    train row (new_places_only: and whose (person, place) has none), sorted by person, region, place.  Device in,
    device out."""
    cols = [place_visits[k] for k in ("person_id", "timestamp", "place_id", "region_id")]
    c = _Cols(*cols)
    n = len(cols[0])
    a = [c.col(x, np.int64) for x in cols]
    (rows, rowsp), outs = c.out(n, np.int32), [c.out(n, np.int64) for _ in HELD_COLUMNS]   # no more triples than rows
    nt, nh = C.c_int64(), C.c_int64(n)
    L.check(L.lib().locrec_holdout_split(n, *a, int(cut_timestamp), int(bool(new_places_only)), c.mem, rowsp, C.byref(nt),
                                         *[o[1] for o in outs], C.byref(nh)))
    rows = rows[:nt.value].long() if c.device else rows[:nt.value].astype(np.int64)
    take = (lambda x: x[rows]) if c.device else (lambda x: np.asarray(x)[rows])
    train = {k: take(place_visits[k]) for k in PLACE_VISIT_COLUMNS}
    return train, {k: o[0][:nh.value] for k, o in zip(HELD_COLUMNS, outs)}


def relevant_lists(held, person_ids, target_region_ids):
    """Per request i the held-out places of person_ids[i] in target_region_ids[i], from holdout_split's sorted triples.
    -> (offsets[n + 1], place_ids): evaluate_ranked's relevant lists, where `held` lies (numpy or torch).  A search over
    the sorted triples - persons and regions are ranked among the triples' own, so that one int64 orders a
    (person, region) pair - without a loop over the requests."""
    hp, hr, hl = held["person_id"], held["region_id"], held["place_id"]
    if _is_tensor(hp):
        import torch as xp
        i64 = lambda a: xp.as_tensor(a, dtype=xp.int64, device=hp.device)
        search = lambda s, v, right=False: xp.searchsorted(s, v, right=right)
        unique, arange, repeat = xp.unique, (lambda m: xp.arange(m, device=hp.device)), xp.repeat_interleave
        zeros = lambda m: xp.zeros(m, dtype=xp.int64, device=hp.device)
        clip = lambda a, hi: xp.clamp(a, max=hi)
    else:
        xp = np
        i64 = lambda a: np.asarray(a, np.int64)
        search = lambda s, v, right=False: np.searchsorted(s, v, "right" if right else "left")
        unique, arange, repeat, zeros = np.unique, np.arange, np.repeat, (lambda m: np.zeros(m, np.int64))
        clip = lambda a, hi: np.minimum(a, hi)
    p, r = i64(person_ids), i64(target_region_ids)
    assert len(p) == len(r)
    offsets = zeros(len(p) + 1)
    if len(hp) == 0 or len(p) == 0:
        return offsets, hl[:0]
    up, ur = unique(hp), unique(hr)
    rank = lambda u, v: clip(search(u, v), len(u) - 1)
    hkey = rank(up, hp) * len(ur) + rank(ur, hr)          # ascending: the triples are sorted by (person, region)
    pi, ri = rank(up, p), rank(ur, r)
    known = (up[pi] == p) & (ur[ri] == r)
    key = pi * len(ur) + ri
    lo, hi = search(hkey, key), search(hkey, key, right=True)
    lengths = (hi - lo) * known
    offsets[1:] = xp.cumsum(lengths, 0)
    total = int(offsets[-1])
    return offsets, hl[repeat(lo - offsets[:-1], lengths) + arange(total)]


def evaluate_ranked(rec_ids, rec_counts, rel_offsets, rel_ids, cutoffs, per_segment=False):
    """Ranked rows against relevant lists (locrec_eval_ranked_batch): rec_ids[S, W] / rec_counts[S] as every
    *_ranked_batch call returns them, the lists as CSR (relevant_lists), cutoffs 1 to EVAL_MAX_CUTOFFS positive ints.
    Host or device arrays, all of one kind.
    -> dict(means[n_cutoffs, 6] (EVAL_MEANS, over the evaluated segments), coverage[n_cutoffs], evaluated,
    relevant[S]) - with per_segment=True also hits[S, n_cutoffs] and metrics[S, n_cutoffs, 5] (EVAL_METRICS), where
    the inputs lie; without it nothing per segment but `relevant` is copied."""
    if not _is_tensor(rec_ids):
        rec_ids = np.asarray(rec_ids, np.int64)
    if rec_ids.ndim != 2:
        raise L.IllegalArgumentException("rec_ids must be a matrix of one row per segment")
    c = _Cols(rec_ids, rec_counts, rel_offsets, rel_ids)
    nseg, width = int(rec_ids.shape[0]), int(rec_ids.shape[1])
    if len(rec_counts) != nseg or len(rel_offsets) != nseg + 1:
        raise L.IllegalArgumentException("one count per row and offsets of n + 1 entries are required")
    cut = np.ascontiguousarray(np.atleast_1d(cutoffs), np.int64)
    nc = len(cut)
    a = [c.col(rec_ids.reshape(-1), np.int64), c.col(rec_counts, np.int64), c.col(rel_offsets, np.int64), c.col(rel_ids, np.int64)]
    (rel, relp) = c.out(nseg, np.int64)
    (hits, hitsp), (met, metp) = (c.out(nseg * nc, np.int64), c.out(nseg * nc * 5, np.float64)) if per_segment else ((None, None),) * 2
    means, cov, ev = np.zeros((max(nc, 1), 6)), np.zeros(max(nc, 1), np.int64), C.c_int64()
    L.check(L.lib().locrec_eval_ranked_batch(nseg, width, *a[:3], len(rel_ids), a[3], nc, L.ptr(cut, C.c_int64), c.mem, relp, hitsp,
                                             metp, L.ptr(means, C.c_double), L.ptr(cov, C.c_int64), C.byref(ev)))
    out = {"means": means[:nc], "coverage": cov[:nc], "evaluated": int(ev.value), "relevant": rel[:nseg]}
    if per_segment:
        out["hits"], out["metrics"] = hits[:nseg * nc].reshape(nseg, nc), met[:nseg * nc * 5].reshape(nseg, nc, 5)
    return out


def evaluate_ranked_stats():
    """What the last evaluate_ranked of this thread did (locrec_eval_ranked_batch_stats), as a dict."""
    v = [C.c_int64() for _ in EVAL_STATS]
    L.check(L.lib().locrec_eval_ranked_batch_stats(*[C.byref(x) for x in v]))
    return dict(zip(EVAL_STATS, (x.value for x in v)))


def max_timestamp(timestamps):
    """max(timestamp) of PlaceVisits.calcVisitsFromTimestamp (PlaceVisits.scala:53-56) as an int.  No visits:
    IllegalArgumentException (the reference dereferences a null there)."""
    c = _Cols(timestamps)
    out = C.c_int64()
    L.check(L.lib().locrec_visits_max_timestamp(len(timestamps), c.col(timestamps, np.int64), c.mem, C.byref(out)))
    return int(out.value)


def extract_region_ids(region_ids):
    """PlaceVisits.extractRegionIds (PlaceVisits.scala:69-78): the distinct region ids, ascending (Spark leaves the
    order of distinct().collect() undefined; this project defines it, as it does for ties)."""
    c = _Cols(region_ids)
    n = len(region_ids)
    r = c.col(region_ids, np.int64)
    cnt = C.c_int64(0)   # first call: count only
    L.check(L.lib().locrec_extract_region_ids(n, r, c.mem, None, C.byref(cnt)))
    m = cnt.value
    out, outp = c.out(m, np.int64)
    if m:
        cnt = C.c_int64(m)
        L.check(L.lib().locrec_extract_region_ids(n, r, c.mem, outp, C.byref(cnt)))
    return out[:m]


def visits_from_timestamp(max_timestamp_ms, last_days_count, tz=None):
    """The day arithmetic of PlaceVisits.calcVisitsFromTimestamp (PlaceVisits.scala:57-60),
    Timestamp.valueOf(maxTimestamp.toLocalDateTime.minusDays(lastDaysCount)), on the host: epoch milliseconds ->
    the wall-clock time of `tz` (a datetime.tzinfo, UTC by default: the reference uses the JVM's default zone) ->
    minus whole days on that wall clock -> epoch milliseconds.  In UTC or at a fixed offset this is
    max - days * 86,400,000.  In a zone with daylight saving the wall-clock day keeps its time of day across a
    switch; a wall-clock result that falls into a DST gap or overlap is *parity unpinned*: java.sql.Timestamp
    resolves it through the legacy calendar, here it is datetime's fold=0 reading (the offset before the switch)."""
    from datetime import datetime, timedelta, timezone
    tz = timezone.utc if tz is None else tz
    epoch = datetime(1970, 1, 1, tzinfo=timezone.utc)
    local = (epoch + timedelta(milliseconds=int(max_timestamp_ms))).astimezone(tz).replace(tzinfo=None)
    back = (local - timedelta(days=int(last_days_count))).replace(tzinfo=tz)
    return (back - epoch) // timedelta(milliseconds=1)


def region_sets(region_ids):
    """PlaceVisits.extractRegionsPlaceVisits' sets (PlaceVisits.scala:64-65): regionIds.map(Seq(_)) ++
    regionIds.combinations(2) - every single region in the given order, then every pair.  -> list of tuples."""
    import itertools
    ids = [int(r) for r in region_ids]
    return [(r,) for r in ids] + list(itertools.combinations(ids, 2))


class RegionSetPlan:
    """The place visits of every region set from ONE partition of the table (locrec_region_partition): the row
    numbers grouped by region, ascending inside a group, so the rows of a set are one group or the stable merge of
    two (locrec_region_set_gather) - exactly placeVisits.where(region_id === a or region_id === b) in input order.
    place_visits: the mapping calc_place_visits returns; region_ids: the listed regions (any order, distinct).
    With CUDA tensors nothing but the len(region_ids) + 2 group offsets reaches the host."""

    def __init__(self, place_visits, region_ids):
        ids = sorted(int(r) for r in region_ids)
        if any(a == b for a, b in zip(ids, ids[1:])):
            raise L.IllegalArgumentException("region_ids must be distinct")
        cols = [place_visits[k] for k in PLACE_VISIT_COLUMNS]
        c = _Cols(*cols)
        self.device, self.mem, self.n = c.device, c.mem, len(cols[0])
        assert all(len(a) == self.n for a in cols)
        if c.device:
            self._torch = c.torch
            self._dev = c.dev
            self.columns = [a.to(c.torch.int64).contiguous() for a in cols]
            listed = c.torch.tensor(ids, dtype=c.torch.int64, device=c.dev)
            c.torch.cuda.current_stream(c.dev).synchronize()   # the upload and the casts above, before the library's stream
        else:
            self.columns = [np.ascontiguousarray(a, np.int64) for a in cols]
            listed = np.asarray(ids, np.int64)
        self.region_ids = ids
        self._rank = {r: i for i, r in enumerate(ids)}
        self.rows, rowsp = c.out(self.n, np.int32)
        offsets = (C.c_int64 * (len(ids) + 2))()
        L.check(L.lib().locrec_region_partition(self.n, c.col(self.columns[3], np.int64), len(ids), c.col(listed, np.int64),
                                                c.mem, rowsp, offsets))
        self.offsets = list(offsets)

    def _ptr(self, a):
        return a.data_ptr() if self.device else a.ctypes.data

    def count(self, region_set):
        """Rows of the set, from the offsets alone."""
        return sum(self.offsets[g + 1] - self.offsets[g] for g in self._groups(region_set))

    def _groups(self, region_set):
        regs = sorted(set(int(r) for r in region_set))
        if not 1 <= len(regs) <= 2:
            raise L.IllegalArgumentException("a region set is one region or a pair of regions")
        for r in regs:
            if r not in self._rank:
                raise L.IllegalArgumentException(f"region {r} is not one of the plan's regions")
        return [self._rank[r] for r in regs]

    def place_visits(self, region_set):
        """The mapping calc_place_visits returns, cut to the rows of the region set (one region or a pair)."""
        g = self._groups(region_set)
        a0, a1 = self.offsets[g[0]], self.offsets[g[0] + 1]
        b0, b1 = (self.offsets[g[1]], self.offsets[g[1] + 1]) if len(g) == 2 else (0, 0)
        total = (a1 - a0) + (b1 - b0)
        if self.device:
            L.require_current_device(self.columns)
            self._torch.cuda.current_stream(self._dev).synchronize()
            outs = [self._torch.empty(max(total, 1), dtype=self._torch.int64, device=self._dev) for _ in self.columns]
        else:
            outs = [np.empty(max(total, 1), np.int64) for _ in self.columns]
        nc = len(self.columns)
        if total:
            cin = (C.c_void_p * nc)(*[self._ptr(a) for a in self.columns])
            cout = (C.c_void_p * nc)(*[self._ptr(a) for a in outs])
            L.check(L.lib().locrec_region_set_gather(self.n, nc, cin, C.c_void_p(self._ptr(self.rows)), a0, a1, b0, b1, self.mem,
                                                     cout))
        return {k: o[:total] for k, o in zip(PLACE_VISIT_COLUMNS, outs)}


def _plan_of(place_visits, region_ids):
    return place_visits if isinstance(place_visits, RegionSetPlan) else RegionSetPlan(place_visits, region_ids)


def knn_indexes_by_region_set(place_visits, region_ids, places_top_n=VISITED_PLACES_TOP_N,
                              categories_top_n=VISITED_CATEGORIES_TOP_N):
    """RatingVectorsBuilderMain.generateRegionRatingVectors (:33-76) to device handles: yields (region_set, KnnIndex)
    for every set of region_sets(region_ids), each through knn_index_from_visits on the set's rows of one
    RegionSetPlan (place_visits may be a plan already).  A set without visits yields None for the handle."""
    plan = _plan_of(place_visits, region_ids)
    for rs in region_sets(region_ids):
        if plan.count(rs) == 0:
            yield rs, None
            continue
        pv = plan.place_visits(rs)
        yield rs, knn_index_from_visits(pv["person_id"], pv["place_id"], pv["category_id"], places_top_n, categories_top_n)


def sg_graphs_by_region_set(place_visits, region_ids, beta_person_place, beta_person_category):
    """StochasticGraphBuilderMain.generateRegionGraphs (:36-45) to device handles: yields (region_set, SgGraph) for
    every set of region_sets(region_ids) through sg_graph_from_visits; None for a set without visits."""
    plan = _plan_of(place_visits, region_ids)
    for rs in region_sets(region_ids):
        if plan.count(rs) == 0:
            yield rs, None
            continue
        yield rs, sg_graph_from_visits(plan.place_visits(rs), beta_person_place, beta_person_category)
