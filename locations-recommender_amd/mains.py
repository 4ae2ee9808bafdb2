"""The callers either side of the hot path, host side:

* f-1  the on-disk inputs -> device handles: the Parquet sets the reference's builders write
       (RatingVectorsBuilderMain.scala:67-73, StochasticGraphBuilderMain.scala:68-73) and its mains
       read back per request (KnnRecommenderMain.scala:69-88, StochasticRecommenderMain.scala:78-84),
       named by DataUtils.scala:34-58.  Here they are read ONCE with pyarrow into the CSR / edge
       arrays the C ABI takes, and the handle stays on the device between requests.
* f-3  the final ranking of the mains (KnnRecommenderMain.scala:90-107,
       StochasticRecommenderMain.scala:64-83): places of the TARGET region joined with the
       recommendations, ordered by score descending, limited to maxRecommendations.

Spark stores ml.linalg.SparseVector through VectorUDT as
struct<type: tinyint, size: int, indices: array<int>, values: array<double>> (type 0 = sparse,
1 = dense).  That layout is Spark's, not the reference's, and no Spark-written file exists in
/root/reference: the reader follows the published layout and is "parity unpinned" against a real
file (tests write files of this layout with pyarrow)."""
import os

import numpy as np

from . import _lib as L


def generate_file_name(region_ids, dir_path, file_prefix):
    """DataUtils.scala:52-58: <dir>/<prefix>_region<a>_region<b>, ids sorted and distinct."""
    regs = sorted(set(int(r) for r in region_ids))
    return f"{dir_path}/{file_prefix}_" + "_".join(f"region{r}" for r in regs)


def _read(path, columns=None):
    import pyarrow.parquet as pq
    return pq.read_table(path, columns=columns)  # a Spark output directory or a single file


def _list_column(col):
    """offsets (int64, n + 1) and flat values of a list<...> column, as numpy."""
    import pyarrow as pa
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if arr.null_count:
        raise L.IllegalArgumentException("null entry in a vector column")
    offs = np.asarray(arr.offsets.to_numpy(zero_copy_only=False), dtype=np.int64)
    vals = arr.values.to_numpy(zero_copy_only=False)
    return offs - offs[0], vals[offs[0]:offs[-1]]


def load_rating_vectors(path, vector_column="rating_vector"):
    """(person_id: long, rating_vector: VectorUDT) -> person_ids, rowptr, indices, values, dim,
    rows sorted by person_id."""
    import pyarrow as pa
    t = _read(path, ["person_id", vector_column])
    pid = np.asarray(t["person_id"].to_numpy(), dtype=np.int64)
    st = t[vector_column].combine_chunks()
    if not pa.types.is_struct(st.type):
        raise L.IllegalArgumentException(f"column {vector_column} is not a VectorUDT struct")
    typ = np.asarray(st.field("type").to_numpy(zero_copy_only=False), dtype=np.int64)
    voff, vals = _list_column(st.field("values"))
    if not np.all(typ == 0):
        # RatingVectorsBuilder.scala:74-77 only ever builds SparseVector; a dense vector here means the
        # file does not come from the reference's builder
        raise L.IllegalArgumentException("dense rating vectors are not produced by the reference's builder")
    size = np.asarray(st.field("size").to_numpy(zero_copy_only=False), dtype=np.int64)
    ioff, idx = _list_column(st.field("indices"))
    if not np.array_equal(ioff, voff):
        raise L.IllegalArgumentException("indices and values of a sparse vector differ in length")
    if len(pid) == 0:
        return pid, np.zeros(1, np.int64), np.empty(0, np.int32), np.empty(0, np.float64), 0
    if size.min() != size.max():
        raise L.IllegalArgumentException("rating vectors of different sizes in one file")
    order = np.argsort(pid, kind="stable")
    lens = np.diff(ioff)[order]
    rowptr = np.zeros(len(pid) + 1, np.int64)
    np.cumsum(lens, out=rowptr[1:])
    gather = np.concatenate([np.arange(ioff[r], ioff[r + 1]) for r in order]) if len(order) else np.empty(0, np.int64)
    return pid[order], rowptr, np.asarray(idx, np.int64)[gather].astype(np.int32), \
        np.asarray(vals, np.float64)[gather], int(size[0])


def load_place_ratings(path):
    """(person_id, place_id, rating: long) (RatingsBuilder.scala:38-47) as three int64 arrays."""
    t = _read(path, ["person_id", "place_id", "rating"])
    return tuple(np.asarray(t[c].to_numpy(), dtype=np.int64) for c in ("person_id", "place_id", "rating"))


def load_stochastic_graph(path):
    """(source_id, target_id, balanced_weight) (StochasticGraphBuilder.scala:12-16); ids of any
    integer width are widened to int64 (StochasticGraphBuilderTest.scala:20-23,56)."""
    t = _read(path, ["source_id", "target_id", "balanced_weight"])
    return (np.asarray(t["source_id"].to_numpy(), dtype=np.int64), np.asarray(t["target_id"].to_numpy(), dtype=np.int64),
            np.asarray(t["balanced_weight"].to_numpy(), dtype=np.float64))


def load_places(data_dir):
    """DataUtils.loadPlaces (:17-23): places_sample with region_id cast to long -> (id, region_id)."""
    t = _read(os.path.join(data_dir, "places_sample"), ["id", "region_id"])
    return np.asarray(t["id"].to_numpy(), dtype=np.int64), np.asarray(t["region_id"].to_numpy(), dtype=np.int64)


def _align(all_ids, ids, rowptr, idx, val):
    """Re-index one family's rows onto the union of person ids (absent persons get empty rows)."""
    pos = np.searchsorted(all_ids, ids)
    lens = np.zeros(len(all_ids), np.int64)
    lens[pos] = np.diff(rowptr)
    out = np.zeros(len(all_ids) + 1, np.int64)
    np.cumsum(lens, out=out[1:])
    return out, idx, val  # rows keep their relative order (both id lists are sorted), so idx / val are unchanged


def knn_index_from_parquet(data_dir, region_ids):
    """KnnRecommenderMain.makeRecommendations' three loads (:53-57) -> one device-resident KnnIndex."""
    from .knn import KnnIndex
    pp, prp, pidx, pval, pdim = load_rating_vectors(generate_file_name(region_ids, data_dir, "place_rating_vectors"))
    cp, crp, cidx, cval, cdim = load_rating_vectors(generate_file_name(region_ids, data_dir, "category_rating_vectors"))
    rp, rplace, rrating = load_place_ratings(generate_file_name(region_ids, data_dir, "place_ratings"))
    ids = np.union1d(np.union1d(pp, cp), rp)
    prp, pidx, pval = _align(ids, pp, prp, pidx, pval)
    crp, cidx, cval = _align(ids, cp, crp, cidx, cval)
    rows = np.searchsorted(ids, rp)
    order = np.argsort(rows, kind="stable")
    rrp = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=len(ids)), out=rrp[1:])
    return KnnIndex(ids, prp, pidx, pval, pdim, crp, cidx, cval, cdim, rrp, rplace[order], rrating[order])


def sg_graph_from_parquet(data_dir, region_ids):
    """StochasticRecommenderMain.loadStochasticGraph (:78-84) -> one device-resident SgGraph."""
    from .stochastic import SgGraph
    return SgGraph(*load_stochastic_graph(generate_file_name(region_ids, data_dir, "stochastic_graph")))


def read_parquet_frame(path, columns=None):
    """spark.read.parquet(path) for the host mirror: a pandas frame that remembers its input files
    (`attrs["inputFiles"]`, the stand-in for Spark's df.inputFiles the handle cache keys on)."""
    df = _read(path, columns).to_pandas()
    df.attrs["inputFiles"] = [path]
    return df


def knn_make_recommendations(data_dir, region_ids, person_id, place_weight, category_weight, k_nearest):
    """KnnRecommenderMain.makeRecommendations (KnnRecommenderMain.scala:53-67) as the unchanged main runs it for
    EVERY request - name the three Parquet sets of the region pair, construct a recommender, ask it - with the
    device index taken from the process-wide handle cache (keyed by the files' names, sizes and modification
    times): only the first request for a region pair reads the files and builds the index.
    -> (place_id, estimated_rating) arrays."""
    from . import _cache
    from .knn import KnnIndex
    _cache.require_gpu_backend("knn_make_recommendations")
    key = _cache.files_key([generate_file_name(region_ids, data_dir, f)
                            for f in ("place_rating_vectors", "category_rating_vectors", "place_ratings")])
    ix = KnnIndex.through_cache(key, lambda: knn_index_from_parquet(data_dir, region_ids))
    try:
        with ix.lock:
            return ix.recommend(person_id, place_weight, category_weight, k_nearest)
    finally:
        ix.close()  # drops the reference only


def sg_make_recommendations(data_dir, region_ids, vertex_id, epsilon, max_iterations, alpha=0.15):
    """StochasticRecommenderMain.makeRecommendations (StochasticRecommenderMain.scala:53-62), graph from the cache.
    -> (id, probability, iterations, converged)."""
    from . import _cache
    from .stochastic import SgGraph
    _cache.require_gpu_backend("sg_make_recommendations")
    key = _cache.files_key([generate_file_name(region_ids, data_dir, "stochastic_graph")])
    g = SgGraph.through_cache(key, lambda: sg_graph_from_parquet(data_dir, region_ids))
    try:
        with g.lock:
            return g.recommend(vertex_id, alpha, epsilon, max_iterations)
    finally:
        g.close()


def rank_recommendations(ids, scores, place_ids, place_region_ids, target_region_id, max_recommendations):
    """printRecommendations of both mains: places.where(region_id == target) JOIN recommendations
    ON id, ORDER BY score DESC, LIMIT maxRecommendations.  Rows whose id is not a place of the target
    region (persons, categories, places elsewhere) drop out in the join.  Ties: Spark leaves the
    order undefined; here (score desc, id asc, input order), NaN first and the two zeros tied."""
    ids, scores = np.asarray(ids, np.int64), np.asarray(scores, np.float64)
    allowed = np.unique(np.asarray(place_ids, np.int64)[np.asarray(place_region_ids, np.int64) == int(target_region_id)])
    keep = np.isin(ids, allowed)
    ids, scores = ids[keep], scores[keep]
    # Spark SQL's order of doubles: every NaN is one value above +inf, -0.0 equals 0.0 (lexsort compares with <)
    nan = np.isnan(scores)
    order = np.lexsort((ids, np.where(nan, 0.0, -scores), ~nan))[:max(0, int(max_recommendations))]
    return ids[order], scores[order]


def rank_recommendations_batch(offsets, ids, scores, place_ids, place_region_ids, target_region_ids, max_recommendations):
    """rank_recommendations for every segment offsets[s]:offsets[s + 1] of one (ids, scores) pair with
    target_region_ids[s]: the numpy restatement of prep.rank_recommendations_batch, with its result layout
    (ids[S, W], scores[S, W], counts[S]; padding id -1 / score 0.0; W = the limit cut to the longest segment)."""
    offsets, ids, scores = np.asarray(offsets, np.int64), np.asarray(ids, np.int64), np.asarray(scores, np.float64)
    nseg = len(target_region_ids)
    if len(offsets) != nseg + 1 or (nseg and (offsets[0] < 0 or offsets[-1] > len(ids) or np.any(np.diff(offsets) < 0))):
        raise L.IllegalArgumentException("offsets must be non-decreasing inside [0, n]")
    longest = int(np.diff(offsets).max()) if nseg else 0
    width = max(0, min(int(max_recommendations), longest))
    out_ids, out_scores = np.full((nseg, width), -1, np.int64), np.zeros((nseg, width), np.float64)
    counts = np.zeros(nseg, np.int64)
    for s in range(nseg):
        a, b = offsets[s], offsets[s + 1]
        ri, rs = rank_recommendations(ids[a:b], scores[a:b], place_ids, place_region_ids, target_region_ids[s], width)
        counts[s] = len(ri)
        out_ids[s, :len(ri)], out_scores[s, :len(ri)] = ri, rs
    return out_ids, out_scores, counts


def rank_recommendations_by_category(offsets, ids, scores, place_ids, place_region_ids, target_region_ids, max_recommendations,
                                     place_category_ids, allowed=None, max_per_category=None, circles=None, excluded=None,
                                     distance=None):
    """The numpy restatement of prep.rank_recommendations_batch_by_category, with its arguments and its result layout
    (ids[S, W], scores[S, W], meters[S, W] or None, counts[S]).  Per segment: the place table cut to the listings that
    pass every predicate given (target region, allow-list, circle); rank_recommendations at limit = segment length for
    the order; then a greedy walk with a counter per category, a row's category and distance being those of the first
    passing listing of its place.  distance: the haversine of four arrays (default prep.distance_meters)."""
    offsets, ids, scores = np.asarray(offsets, np.int64), np.asarray(ids, np.int64), np.asarray(scores, np.float64)
    place_ids, regions = np.asarray(place_ids, np.int64), np.asarray(place_region_ids, np.int64)
    cats = np.asarray(place_category_ids, np.int64)
    nseg = len(target_region_ids)
    if len(offsets) != nseg + 1 or (nseg and (offsets[0] < 0 or offsets[-1] > len(ids) or np.any(np.diff(offsets) < 0))):
        raise L.IllegalArgumentException("offsets must be non-decreasing inside [0, n]")
    if max_per_category is not None and np.any(np.asarray(max_per_category, np.int64) < 1):
        raise L.IllegalArgumentException("max_per_category must be >= 1 for every segment")
    if circles is not None and distance is None:
        from . import prep
        distance = prep.distance_meters
    longest = int(np.diff(offsets).max()) if nseg else 0
    width = max(0, min(int(max_recommendations), longest))
    out_ids, out_scores = np.full((nseg, width), -1, np.int64), np.zeros((nseg, width), np.float64)
    out_meters = np.zeros((nseg, width), np.float64) if circles is not None else None
    counts = np.zeros(nseg, np.int64)
    for s in range(nseg):
        a, b = offsets[s], offsets[s + 1]
        si, ss = ids[a:b], scores[a:b]
        if excluded is not None:
            xo, xi = np.asarray(excluded[0], np.int64), np.asarray(excluded[1], np.int64)
            keep = ~np.isin(si, xi[xo[s]:xo[s + 1]])
            si, ss = si[keep], ss[keep]
        rows = np.flatnonzero(regions == int(target_region_ids[s]))
        if allowed is not None:
            ao, ai = np.asarray(allowed[0], np.int64), np.asarray(allowed[1], np.int64)
            if ao[s + 1] > ao[s]:
                rows = rows[np.isin(cats[rows], ai[ao[s]:ao[s + 1]])]
        meters = np.zeros(len(rows))
        if circles is not None and len(rows):
            plat, plon, clat, clon, rad = (np.asarray(x, np.float64) for x in circles)
            meters = np.asarray(distance(np.full(len(rows), clat[s]), np.full(len(rows), clon[s]), plat[rows], plon[rows]), np.float64)
            rows, meters = rows[meters <= rad[s]], meters[meters <= rad[s]]
        ri, rs = rank_recommendations(si, ss, place_ids[rows], regions[rows], target_region_ids[s], len(si))
        first = {}
        for j, pid in enumerate(place_ids[rows].tolist()):    # the listing that counts: the first passing one
            first.setdefault(pid, j)
        cap = int(max_per_category[s]) if max_per_category is not None else None
        used, w = {}, 0
        for i, sc in zip(ri.tolist(), rs):
            if w == width:
                break
            j = first[i]
            c = int(cats[rows[j]])
            if cap is not None and used.get(c, 0) >= cap:
                continue
            used[c] = used.get(c, 0) + 1
            out_ids[s, w], out_scores[s, w] = i, sc
            if out_meters is not None:
                out_meters[s, w] = meters[j]
            w += 1
        counts[s] = w
    return out_ids, out_scores, out_meters, counts


def knn_recommend_places_batch(data_dir, region_ids, requests, place_weight, category_weight, k_nearest,
                               max_recommendations=10, new_places=False):
    """Many requests of one region pair to their end (KnnRecommenderMain.scala:53-67 and :90-101): requests is a
    sequence of (person_id, target_region_id); the index comes from the handle cache, the places from load_places.
    -> (place_ids[n, W], estimated_ratings[n, W], counts[n]), ranked on the device.
    new_places=True: the places a person has a place_ratings row for are left out (the unvisited ranked batch)."""
    from . import _cache
    from .knn import KnnIndex
    _cache.require_gpu_backend("knn_recommend_places_batch")
    persons = np.asarray([r[0] for r in requests], np.int64)
    targets = np.asarray([r[1] for r in requests], np.int64)
    place_ids, place_regions = load_places(data_dir)
    key = _cache.files_key([generate_file_name(region_ids, data_dir, f)
                            for f in ("place_rating_vectors", "category_rating_vectors", "place_ratings")])
    ix = KnnIndex.through_cache(key, lambda: knn_index_from_parquet(data_dir, region_ids))
    try:
        with ix.lock:
            return ix.recommend_ranked_batch(persons, place_weight, category_weight, k_nearest, place_ids, place_regions,
                                             targets, max_recommendations, unvisited=new_places)
    finally:
        ix.close()  # drops the reference only


def knn_visitor_requests(data_dir, region_ids, visits, target_region_ids, place_weight, category_weight, k_nearest,
                         max_recommendations=10, new_places=False):
    """Requests of persons the region set's index does not hold - they arrived after the cut of the visit table it was
    built from, or their visits have changed since.  visits: mapping with visitor_id, place_id, category_id (one row a
    place visit; host arrays or CUDA tensors); target_region_ids: a mapping visitor id -> region, one region for all, or
    one region per visitor in ascending visitor id.  The index comes from the handle cache under
    knn_make_recommendations' key, the vectors from prep.visitor_vectors, the answer from ONE ranked visitors call.
    -> a list of (visitor_id, place_ids, estimated_ratings), ascending visitor id.
    new_places=True: the places a visitor has rated are left out."""
    from . import _cache, prep
    from .knn import KnnIndex
    _cache.require_gpu_backend("knn_visitor_requests")
    ids, vectors, rated = prep.visitor_vectors(visits["visitor_id"], visits["place_id"], visits["category_id"])
    host_ids = np.asarray(ids.cpu().numpy() if hasattr(ids, "cpu") else ids, np.int64)
    if hasattr(target_region_ids, "keys"):
        targets = np.asarray([target_region_ids[int(v)] for v in host_ids], np.int64)
    elif np.ndim(target_region_ids) == 0:
        targets = np.full(len(host_ids), int(target_region_ids), np.int64)
    else:
        targets = np.asarray(target_region_ids, np.int64)
    if len(targets) != len(host_ids):
        raise L.IllegalArgumentException("requirement failed: one target region per visitor is required")
    exclude = None
    if new_places:
        exclude = tuple(np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a, np.int64) for a in rated)
    place_ids, place_regions = load_places(data_dir)
    key = _cache.files_key([generate_file_name(region_ids, data_dir, f)
                            for f in ("place_rating_vectors", "category_rating_vectors", "place_ratings")])
    ix = KnnIndex.through_cache(key, lambda: knn_index_from_parquet(data_dir, region_ids))
    try:
        with ix.lock:
            oi, osc, cnt = ix.visitors_recommend_ranked_batch(*vectors, place_weight, category_weight, k_nearest, place_ids,
                                                              place_regions, targets, max_recommendations, exclude=exclude)
    finally:
        ix.close()  # drops the reference only
    return [(int(v), oi[i, :cnt[i]].copy(), osc[i, :cnt[i]].copy()) for i, v in enumerate(host_ids)]


def _per_visitor(values, host_ids, what):
    """A mapping visitor id -> value, one value for all, or one per visitor in ascending visitor id -> int64[nv]."""
    if hasattr(values, "keys"):
        out = np.asarray([values[int(v)] for v in host_ids], np.int64)
    elif np.ndim(values) == 0:
        out = np.full(len(host_ids), int(values), np.int64)
    else:
        out = np.asarray(values.cpu().numpy() if hasattr(values, "cpu") else values, np.int64)
    if len(out) != len(host_ids):
        raise L.IllegalArgumentException(f"requirement failed: one {what} region per visitor is required")
    return out


def _csr_rows(rowptr, arrays, rows):
    """The listed rows of a CSR (rowptr and its element arrays; numpy arrays or tensors of one device) as a CSR of their
    own, in the given order."""
    if hasattr(rowptr, "is_cuda"):
        import torch as xp
        at = xp.as_tensor(np.asarray(rows, np.int64), device=rowptr.device)
        zeros, arange, repeat = (lambda n: xp.zeros(n, dtype=xp.int64, device=rowptr.device),
                                 lambda n: xp.arange(n, dtype=xp.int64, device=rowptr.device), xp.repeat_interleave)
    else:
        xp, at = np, np.asarray(rows, np.int64)
        rowptr = np.asarray(rowptr, np.int64)
        zeros, arange, repeat = (lambda n: np.zeros(n, np.int64)), (lambda n: np.arange(n, dtype=np.int64)), np.repeat
    lens = (rowptr[1:] - rowptr[:-1])[at]
    ptr = zeros(len(rows) + 1)
    ptr[1:] = xp.cumsum(lens, 0)
    take = repeat(rowptr[:-1][at] - ptr[:-1], lens) + arange(int(ptr[-1]))
    return ptr, tuple(a[take] for a in arrays)


def knn_visitor_requests_pooled(data_dir, visits, home_region_ids, target_region_ids, place_weight, category_weight, k_nearest,
                                max_recommendations=10, new_places=False, pooled=True):
    """knn_visitor_requests for a queue of cold-start persons that fans out over region sets as persons do: visits as in
    knn_visitor_requests; home_region_ids and target_region_ids per visitor - a mapping visitor id -> region, one region
    for all, or one per visitor in ascending visitor id.  Every visitor's index is the one of [home, target] from the
    handle cache (one handle per distinct region set, _knn_resolve_request_lines), the vectors come from ONE
    prep.visitor_vectors call - one numbering for all members - and ONE KnnPool.visitors_recommend_ranked_batch call serves
    everybody.
    -> a list in ascending visitor id of (visitor_id, place_ids, estimated_ratings); where a visitor's region set cannot
    be opened the entry is the exception instance; where the stage refuses a visitor the exception is recorded and the call
    repeated without the visitor (_call_without_bad_lines' contract).
    new_places=True: the places a visitor has rated are left out.
    pooled=False: one KnnIndex.visitors_recommend_ranked_batch call per distinct index instead of the pool call - the same
    result bit for bit; what such a queue cost before the pool."""
    from . import _cache, prep
    from .knn import KnnPool
    _cache.require_gpu_backend("knn_visitor_requests_pooled")
    ids, vectors, rated = prep.visitor_vectors(visits["visitor_id"], visits["place_id"], visits["category_id"])
    host_ids = np.asarray(ids.cpu().numpy() if hasattr(ids, "cpu") else ids, np.int64)
    homes = _per_visitor(home_region_ids, host_ids, "home")
    regions = _per_visitor(target_region_ids, host_ids, "target")
    lists = tuple(np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a, np.int64) for a in rated) if new_places else None
    out, targets, indexes = _knn_resolve_request_lines(
        data_dir, None, list(range(len(host_ids))), resolve=lambda i: (int(host_ids[i]), int(homes[i]), int(regions[i])))
    try:
        if targets:
            place_ids, place_regions = load_places(data_dir)
            pool = KnnPool(indexes) if pooled else None
            try:
                def call(gi, _, live):
                    if len(live) == len(host_ids):
                        vec, ex = vectors, lists
                    else:  # (without the visitors whose region set has no index, or whom the stage refused)
                        p_ptr, (p_idx, p_val) = _csr_rows(vectors[0], vectors[1:3], live)
                        c_ptr, (c_idx, c_val) = _csr_rows(vectors[3], vectors[4:6], live)
                        vec = (p_ptr, p_idx, p_val, c_ptr, c_idx, c_val)
                        ex = None
                        if lists is not None:
                            e_ptr, (e_ids,) = _csr_rows(lists[0], lists[1:2], live)
                            ex = (e_ptr, e_ids)
                    tgt = regions[np.asarray(live, np.int64)]
                    if pool is not None:
                        return pool.visitors_recommend_ranked_batch(gi, *vec, place_weight, category_weight, k_nearest, place_ids,
                                                                    place_regions, tgt, max_recommendations, exclude=ex)
                    return _knn_visitors_per_index(indexes, gi, vec, place_weight, category_weight, k_nearest, place_ids,
                                                   place_regions, tgt, max_recommendations, ex)
                live, rows = _call_without_bad_lines(out, targets, call)
            finally:
                if pool is not None:
                    pool.close()
            if live:
                oi, osc, cnt = rows
                for j, i in enumerate(live):
                    out[i] = (int(host_ids[i]), np.array(oi[j, :cnt[j]]), np.array(osc[j, :cnt[j]]))
    finally:
        for ix in indexes:
            ix.close()  # drops the reference only
    return out


def _knn_visitors_per_index(indexes, index_of, vectors, pw, cw, k, place_ids, place_regions, regions, max_recommendations, exclude):
    """KnnPool.visitors_recommend_ranked_batch's result from one KnnIndex.visitors_recommend_ranked_batch call per distinct
    index on that index's visitors in call order; a refused visitor raises with bad_visitor = its position in the call."""
    n = len(index_of)
    width = max(0, min(int(max_recommendations), len(place_ids)))
    oi, osc, cnt = np.full((n, width), -1, np.int64), np.zeros((n, width), np.float64), np.zeros(n, np.int64)
    for k_ix in np.unique(index_of):
        at = np.flatnonzero(index_of == k_ix)
        p_ptr, (p_idx, p_val) = _csr_rows(vectors[0], vectors[1:3], at)
        c_ptr, (c_idx, c_val) = _csr_rows(vectors[3], vectors[4:6], at)
        ex = None
        if exclude is not None:
            e_ptr, (e_ids,) = _csr_rows(exclude[0], exclude[1:2], at)
            ex = (e_ptr, e_ids)
        try:
            with indexes[k_ix].lock:
                oi[at], osc[at], cnt[at] = indexes[k_ix].visitors_recommend_ranked_batch(
                    p_ptr, p_idx, p_val, c_ptr, c_idx, c_val, pw, cw, k, place_ids, place_regions, regions[at],
                    max_recommendations, exclude=ex)
        except L.IllegalArgumentException as e:
            if getattr(e, "bad_visitor", -1) >= 0:
                e.bad_visitor = int(at[e.bad_visitor])
            raise
    return oi, osc, cnt


def sg_recommend_places_batch(data_dir, region_ids, requests, epsilon, max_iterations, alpha=0.15, max_recommendations=10,
                              on_device=True, new_places=False):
    """Many requests of one region pair (StochasticRecommenderMain.scala:53-75): requests is a sequence of
    (vertex_id, target_region_id).  -> (ids[n, W], probabilities[n, W], counts[n], iterations[n], converged[n]),
    emitted and ranked on the device (on_device=False: the host rows through the segmented ranker, the same result).
    new_places=True: the targets of a vertex's out-edges in the region set's edge list are left out of its ranking."""
    from . import _cache
    from .stochastic import SgGraph
    _cache.require_gpu_backend("sg_recommend_places_batch")
    vertices = np.asarray([r[0] for r in requests], np.int64)
    targets = np.asarray([r[1] for r in requests], np.int64)
    place_ids, place_regions = load_places(data_dir)
    excluded = _sg_visited_lists(data_dir, region_ids, vertices) if new_places else None
    key = _cache.files_key([generate_file_name(region_ids, data_dir, "stochastic_graph")])
    g = SgGraph.through_cache(key, lambda: sg_graph_from_parquet(data_dir, region_ids))
    try:
        with g.lock:
            return g.recommend_ranked_batch(vertices, alpha, epsilon, max_iterations, place_ids, place_regions, targets,
                                            max_recommendations, on_device=on_device, excluded=excluded)
    finally:
        g.close()


def sg_visitor_requests(data_dir, region_ids, visits, target_region_ids, epsilon, max_iterations, max_recommendations=10,
                        new_places=False, beta_person_place=1.0, beta_person_category=1.0, alpha=0.15):
    """knn_visitor_requests' SG sibling: requests of persons the region set's graph has no vertex for - they arrived
    after the cut of the visit table it was built from, or their visits have changed since.  visits: mapping with
    visitor_id, place_id, category_id (one row a place visit); target_region_ids: a mapping visitor id -> region, one
    region for all, or one region per visitor in ascending visitor id.  The graph comes from the handle cache under
    sg_make_recommendations' key, the edges from prep.visitor_edges (the betas are those the graph was built with; visits
    to places and categories the graph has no live vertex for are dropped), the answer from ONE ranked visitors call.
    -> a list of (visitor_id, place_ids, probabilities), ascending visitor id.
    new_places=True: a visitor's own targets are left out."""
    from . import _cache, prep
    from .stochastic import SgGraph
    _cache.require_gpu_backend("sg_visitor_requests")
    place_ids, place_regions = load_places(data_dir)
    key = _cache.files_key([generate_file_name(region_ids, data_dir, "stochastic_graph")])
    g = SgGraph.through_cache(key, lambda: sg_graph_from_parquet(data_dir, region_ids))
    try:
        with g.lock:
            ids, offsets, edge_targets, weights, _ = prep.visitor_edges(
                visits["visitor_id"], visits["place_id"], visits["category_id"], beta_person_place, beta_person_category, graph=g)
            if hasattr(target_region_ids, "keys"):
                targets = np.asarray([target_region_ids[int(v)] for v in ids], np.int64)
            elif np.ndim(target_region_ids) == 0:
                targets = np.full(len(ids), int(target_region_ids), np.int64)
            else:
                targets = np.asarray(target_region_ids, np.int64)
            if len(targets) != len(ids):
                raise L.IllegalArgumentException("requirement failed: one target region per visitor is required")
            oi, op, cnt, _, _ = g.visitors_recommend_ranked_batch(
                offsets, edge_targets, weights, alpha, epsilon, max_iterations, place_ids, place_regions, targets,
                max_recommendations, exclude=(offsets, edge_targets) if new_places else None)
    finally:
        g.close()  # drops the reference only
    return [(int(v), oi[i, :cnt[i]].copy(), op[i, :cnt[i]].copy()) for i, v in enumerate(ids)]


def sg_visitor_requests_pooled(data_dir, visits, home_region_ids, target_region_ids, epsilon, max_iterations, max_recommendations=10,
                               new_places=False, beta_person_place=1.0, beta_person_category=1.0, alpha=0.15, pooled=True):
    """sg_visitor_requests for a queue of cold-start persons that fans out over region sets as persons do - the SG sibling
    of knn_visitor_requests_pooled: visits as in sg_visitor_requests; home_region_ids and target_region_ids per visitor - a
    mapping visitor id -> region, one region for all, or one per visitor in ascending visitor id.  Every visitor's graph is
    the one of [home, target] from the handle cache (one handle per distinct region set), its edges come from
    prep.visitor_edges against ITS member's graph - a visit to a place one member lacks may be live in another - and ONE
    SgPool.visitors_recommend_ranked_batch call serves everybody.
    -> a list in ascending visitor id of (visitor_id, place_ids, probabilities); where a visitor's region set cannot be
    opened the entry is the exception instance; where the stage refuses a visitor - one left without edges in its graph -
    the exception is recorded and the call repeated without the visitor (_call_without_bad_lines' contract).
    new_places=True: a visitor's own targets are left out.
    pooled=False: one SgGraph.visitors_recommend_ranked_batch call per distinct graph instead of the pool call - the same
    result bit for bit; what such a queue cost before the pool."""
    from . import _cache, prep
    from .stochastic import SgPool
    _cache.require_gpu_backend("sg_visitor_requests_pooled")
    host = lambda a: np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a, np.int64)
    v, p, c = host(visits["visitor_id"]), host(visits["place_id"]), host(visits["category_id"])
    host_ids = np.unique(v)
    homes = _per_visitor(home_region_ids, host_ids, "home")
    regions = _per_visitor(target_region_ids, host_ids, "target")
    out, targets, graphs = _sg_resolve_request_lines(
        data_dir, None, list(range(len(host_ids))), resolve=lambda i: (int(host_ids[i]), int(homes[i]), int(regions[i])))
    try:
        if targets:
            place_ids, place_regions = load_places(data_dir)
            # every visitor's edges against its own member's graph: one prep.visitor_edges call per member
            edges = {}
            for k, g in enumerate(graphs):
                mine = [i for i in sorted(targets) if targets[i][1] == k]
                rows = np.isin(v, host_ids[mine])
                with g.lock:
                    _, off, t, w, _ = prep.visitor_edges(v[rows], p[rows], c[rows], beta_person_place, beta_person_category, graph=g)
                for j, i in enumerate(mine):  # (ascending visitor id on both sides)
                    edges[i] = (t[off[j]:off[j + 1]], w[off[j]:off[j + 1]])
            pool = SgPool(graphs) if pooled else None
            try:
                def call(gi, _, live):
                    off = np.zeros(len(live) + 1, np.int64)
                    np.cumsum([len(edges[i][0]) for i in live], out=off[1:])
                    t = np.concatenate([edges[i][0] for i in live]).astype(np.int64)
                    w = np.concatenate([edges[i][1] for i in live]).astype(np.float64)
                    serve = pool.visitors_recommend_ranked_batch if pool is not None else \
                        (lambda *a, **kw: _sg_visitors_per_graph(graphs, *a, **kw))
                    return serve(gi, off, t, w, alpha, epsilon, max_iterations, place_ids, place_regions,
                                 regions[np.asarray(live, np.int64)], max_recommendations, exclude=(off, t) if new_places else None)
                live, rows = _call_without_bad_lines(out, targets, call)
            finally:
                if pool is not None:
                    pool.close()
            if live:
                oi, op, cnt, _, _ = rows
                for j, i in enumerate(live):
                    out[i] = (int(host_ids[i]), np.array(oi[j, :cnt[j]]), np.array(op[j, :cnt[j]]))
    finally:
        for g in graphs:
            g.close()  # drops the reference only
    return out


def _sg_visitors_per_graph(graphs, graph_index, offsets, target_ids, weights, alpha, epsilon, max_iterations, place_ids,
                           place_regions, regions, max_recommendations, exclude=None):
    """SgPool.visitors_recommend_ranked_batch's result from one SgGraph.visitors_recommend_ranked_batch call per distinct
    graph on that graph's visitors in call order; a refused visitor raises with bad_visitor = its position in the call (the
    smallest over the graphs, as the pool call reports it)."""
    n = len(graph_index)
    width = max(0, int(max_recommendations))
    oi, op = np.full((n, width), -1, np.int64), np.zeros((n, width), np.float64)
    cnt, its, conv = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    refused = None
    for k in np.unique(graph_index):
        at = np.flatnonzero(graph_index == k)
        off, (t, w) = _csr_rows(offsets, (target_ids, weights), at)
        try:
            with graphs[k].lock:
                r = graphs[k].visitors_recommend_ranked_batch(off, t, w, alpha, epsilon, max_iterations, place_ids, place_regions,
                                                              regions[at], max_recommendations, exclude=(off, t) if exclude else None)
        except L.IllegalArgumentException as e:
            if getattr(e, "bad_visitor", -1) < 0:
                raise
            e.bad_visitor = int(at[e.bad_visitor])
            if refused is None or e.bad_visitor < refused.bad_visitor:
                refused = e
            continue
        oi[at, :r[0].shape[1]], op[at, :r[1].shape[1]], cnt[at], its[at], conv[at] = r
    if refused is not None:
        raise refused
    return oi, op, cnt, its, conv


def _sg_visited_lists(data_dir, region_ids, vertex_ids):
    """The exclusion lists of new_places for vertices of one region set: out_neighbours over its edge Parquet."""
    from .stochastic import out_neighbours
    source_ids, target_ids, _ = load_stochastic_graph(generate_file_name(region_ids, data_dir, "stochastic_graph"))
    return out_neighbours(source_ids, target_ids, vertex_ids)


def build_with_balanced_weights(betas, all_edges):
    """StochasticGraphBuilder.buildWithBalancedWeights (StochasticGraphBuilder.scala:8-28), the
    producer of the SG path's input: every family's `weight` times its beta,
    families concatenated in the given order (`union` keeps it) - the edge-list order the device
    layout preserves inside each row.  all_edges: sequence of (source_id, target_id, weight) column
    triples or mappings with those keys.  -> (source_id int64, target_id int64, balanced_weight)."""
    if len(betas) != len(all_edges) or not all_edges:
        raise L.IllegalArgumentException("one beta per edge family is required")
    src, dst, w = [], [], []
    for beta, e in zip(betas, all_edges):
        s, t, wt = (e["source_id"], e["target_id"], e["weight"]) if hasattr(e, "keys") or hasattr(e, "columns") else e
        src.append(np.asarray(s, np.int64))
        dst.append(np.asarray(t, np.int64))
        w.append(np.asarray(wt, np.float64) * float(beta))   # col("weight") * beta
    return np.concatenate(src), np.concatenate(dst), np.concatenate(w)


def calc_ratings(person_ids, entity_ids, top_n):
    """RatingsBuilder.calcRatings (RatingsBuilder.scala:32-48): visits -> (person_id, entity_id,
    rating = number of visits), keeping per person the entities whose rank() by rating descending
    is <= top_n.  rank() leaves gaps after ties: an entity's rank is 1 + the number
    of the person's entities with a STRICTLY larger count, so a tie straddling top_n is kept whole.
    No reference test covers it ("parity unpinned").  Rows come back ordered by (person, entity)."""
    p, e = np.asarray(person_ids, np.int64), np.asarray(entity_ids, np.int64)
    if len(p) == 0:
        return p, e, np.empty(0, np.int64)
    order = np.lexsort((e, p))
    p, e = p[order], e[order]
    first = np.r_[True, (p[1:] != p[:-1]) | (e[1:] != e[:-1])]
    gp, ge = p[first], e[first]
    cnt = np.diff(np.r_[np.flatnonzero(first), len(p)])          # count("*") per (person, entity)
    # rank within the person by count descending, ties sharing the smallest position
    o2 = np.lexsort((-cnt, gp))
    sp, sc = gp[o2], cnt[o2]
    pstart = np.r_[True, sp[1:] != sp[:-1]]
    pos = np.arange(len(sp)) - np.maximum.accumulate(np.where(pstart, np.arange(len(sp)), 0))
    newval = pstart | np.r_[True, sc[1:] != sc[:-1]]
    # positions of equal counts inherit the first position of their run
    run_first = np.maximum.accumulate(np.where(newval, np.arange(len(sp)), 0))
    rank = 1 + pos[run_first]
    keep = np.zeros(len(gp), bool)
    keep[o2] = rank <= int(top_n)
    return gp[keep], ge[keep], cnt[keep]


def calc_rating_vectors(person_ids, entity_ids, ratings):
    """RatingVectorsBuilder.calcRatingVectors (:10-25, 52-84): one SparseVector per person, size =
    max entity id + 1 (an id beyond Int range is an ArithmeticException, :36-41), indices ascending,
    values = rating.toDouble (:69).  -> person_ids, rowptr, indices(int32), values(float64), size."""
    p, e, r = np.asarray(person_ids, np.int64), np.asarray(entity_ids, np.int64), np.asarray(ratings, np.int64)
    if len(p) == 0:
        return p, np.zeros(1, np.int64), np.empty(0, np.int32), np.empty(0, np.float64), 0
    max_id = int(e.max())
    if max_id > 2**31 - 1 or int(e.min()) < 0:
        raise ArithmeticError(f"Index out of Int range: {max_id if max_id > 2**31 - 1 else int(e.min())}")
    order = np.lexsort((e, p))
    p, e, r = p[order], e[order], r[order]
    dup = np.r_[False, (p[1:] == p[:-1]) & (e[1:] == e[:-1])]   # TreeSet ordered by index: first one wins
    p, e, r = p[~dup], e[~dup], r[~dup]
    ids, counts = np.unique(p, return_counts=True)
    rowptr = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(counts, out=rowptr[1:])
    return ids, rowptr, e.astype(np.int32), r.astype(np.float64), max_id + 1


# ---- the builder mains' bodies (knn/RatingVectorsBuilderMain.scala:15-76, stochastic/StochasticGraphBuilderMain.scala:
# 18-45): the two sample tables -> place visits -> every region set's Parquet sets, computed on the device ---------------

def _column_i64(col):
    """A Parquet column as int64: integers of any width are widened (DataUtils.scala:14-31 casts region_id to long, and
    it may arrive as a dictionary-encoded Hive partition column); a timestamp of any unit becomes epoch milliseconds
    (floor), an INT96 / date-time the reader maps to a timestamp included."""
    import pyarrow as pa
    import pyarrow.compute as pc
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if pa.types.is_dictionary(arr.type):
        arr = arr.dictionary_decode()
    if arr.null_count:
        raise L.IllegalArgumentException("null entry in an id / timestamp column")
    if pa.types.is_timestamp(arr.type):
        per_ms = {"s": None, "ms": 1, "us": 1_000, "ns": 1_000_000}[arr.type.unit]
        raw = np.asarray(arr.cast(pa.int64()).to_numpy(zero_copy_only=False), dtype=np.int64)
        return raw * 1000 if per_ms is None else raw // per_ms
    if pa.types.is_string(arr.type) or pa.types.is_large_string(arr.type):
        arr = pc.cast(arr, pa.int64())   # a partition value read without a schema
    return np.asarray(arr.to_numpy(zero_copy_only=False), dtype=np.int64)


def _column_f64(col):
    return np.asarray(col.to_numpy(), dtype=np.float64)


def load_location_visits(data_dir):
    """DataUtils.loadLocationVisits (:25-31): location_visits_sample -> dict(person_id, timestamp (epoch ms), latitude,
    longitude, region_id), the mapping prep.calc_place_visits takes."""
    t = _read(os.path.join(data_dir, "location_visits_sample"), ["person_id", "timestamp", "latitude", "longitude", "region_id"])
    return {"person_id": _column_i64(t["person_id"]), "timestamp": _column_i64(t["timestamp"]),
            "latitude": _column_f64(t["latitude"]), "longitude": _column_f64(t["longitude"]),
            "region_id": _column_i64(t["region_id"])}


def load_places_full(data_dir):
    """DataUtils.loadPlaces (:17-23) with every column the builders use: places_sample -> dict(id, latitude, longitude,
    region_id, category_id)."""
    t = _read(os.path.join(data_dir, "places_sample"), ["id", "latitude", "longitude", "region_id", "category_id"])
    return {"id": _column_i64(t["id"]), "latitude": _column_f64(t["latitude"]), "longitude": _column_f64(t["longitude"]),
            "region_id": _column_i64(t["region_id"]), "category_id": _column_i64(t["category_id"])}


def load_place_visits(path):
    """What write_place_visits wrote (PlaceVisits.scala:40-46,116-121) -> dict of five int64 columns."""
    names = ("person_id", "timestamp", "place_id", "region_id", "category_id")
    t = _read(path, list(names))
    return {k: _column_i64(t[k]) for k in names}


def _host(a, dtype):
    """A numpy array of a column that may be a CUDA tensor (the one copy to the host a file needs)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype)


def _write_dir(path, table):
    """df.write.mode(SaveMode.Overwrite).parquet(path) with one part file: a directory holding part-00000.parquet and
    _SUCCESS.  Overwrite removes the part files of an earlier write, nothing else."""
    import pyarrow.parquet as pq
    os.makedirs(path, exist_ok=True)
    for name in os.listdir(path):
        if name.startswith("part-") or name == "_SUCCESS":
            os.remove(os.path.join(path, name))
    pq.write_table(table, os.path.join(path, "part-00000.parquet"))
    open(os.path.join(path, "_SUCCESS"), "w").close()


def write_place_visits(path, place_visits):
    """PlaceVisits.writePlaceVisits (:116-121): (person_id, timestamp, place_id, region_id, category_id); the timestamp
    as a Parquet timestamp of milliseconds."""
    import pyarrow as pa
    cols = {k: _host(place_visits[k], np.int64) for k in ("person_id", "timestamp", "place_id", "region_id", "category_id")}
    arrays = [pa.array(cols["person_id"], pa.int64()), pa.array(cols["timestamp"], pa.int64()).cast(pa.timestamp("ms")),
              pa.array(cols["place_id"], pa.int64()), pa.array(cols["region_id"], pa.int64()),
              pa.array(cols["category_id"], pa.int64())]
    _write_dir(path, pa.table(arrays, names=["person_id", "timestamp", "place_id", "region_id", "category_id"]))


def write_rating_vectors(path, person_ids, rowptr, indices, values, size, vector_column="rating_vector"):
    """(person_id: long, rating_vector: VectorUDT) (RatingVectorsBuilder.scala:10-25) in the struct layout the readers
    follow: type 0 (sparse), size, indices: array<int>, values: array<double>.  No person: an empty file of that schema."""
    import pyarrow as pa
    pid, idx, val = _host(person_ids, np.int64), _host(indices, np.int32), _host(values, np.float64)
    n = len(pid)
    ptr = np.zeros(1, np.int64) if rowptr is None or n == 0 else _host(rowptr, np.int64)
    if len(ptr) != n + 1 or ptr[-1] != len(idx) or len(val) != len(idx) or ptr[-1] >= 2**31:
        raise L.IllegalArgumentException("rowptr does not describe the indices / values (below 2^31 entries)")
    offs = pa.array((ptr - ptr[0]).astype(np.int32), pa.int32())
    vec = pa.StructArray.from_arrays(
        [pa.array(np.zeros(n, np.int8), pa.int8()), pa.array(np.full(n, int(size), np.int32), pa.int32()),
         pa.ListArray.from_arrays(offs, pa.array(idx, pa.int32())), pa.ListArray.from_arrays(offs, pa.array(val, pa.float64()))],
        fields=[pa.field("type", pa.int8()), pa.field("size", pa.int32()), pa.field("indices", pa.list_(pa.int32())),
                pa.field("values", pa.list_(pa.float64()))])
    _write_dir(path, pa.table([pa.array(pid, pa.int64()), vec], names=["person_id", vector_column]))


def write_place_ratings(path, person_ids, place_ids, ratings):
    """(person_id, place_id, rating: long) (RatingsBuilder.scala:38-47)."""
    import pyarrow as pa
    _write_dir(path, pa.table([pa.array(_host(person_ids, np.int64), pa.int64()), pa.array(_host(place_ids, np.int64), pa.int64()),
                               pa.array(_host(ratings, np.int64), pa.int64())], names=["person_id", "place_id", "rating"]))


def write_stochastic_graph(path, source_ids, target_ids, balanced_weights):
    """(source_id, target_id, balanced_weight) (StochasticGraphBuilder.scala:12-16), rows in the given order."""
    import pyarrow as pa
    _write_dir(path, pa.table([pa.array(_host(source_ids, np.int64), pa.int64()), pa.array(_host(target_ids, np.int64), pa.int64()),
                               pa.array(_host(balanced_weights, np.float64), pa.float64())],
                              names=["source_id", "target_id", "balanced_weight"]))


def _device_place_visits(data_dir, last_days_count, tz):
    """The common head of both builder mains (doMain): load the two tables, calcPlaceVisits on the device, write
    place_visits.  -> (place visits as CUDA tensors, the distinct region ids of the places, ascending)."""
    import torch
    from . import _cache, prep
    _cache.require_gpu_backend("the builder mains")
    visits, places = load_location_visits(data_dir), load_places_full(data_dir)
    dv = {k: torch.from_numpy(np.array(v)).cuda() for k, v in visits.items()}   # (a copy: arrow's buffers are read-only)
    dp = {k: torch.from_numpy(np.array(v)).cuda() for k, v in places.items()}
    visits_from = prep.visits_from_timestamp(prep.max_timestamp(dv["timestamp"]), last_days_count, tz)
    place_visits = prep.calc_place_visits(dv, dp, visits_from)
    write_place_visits(os.path.join(data_dir, "place_visits"), place_visits)
    return place_visits, prep.extract_region_ids(dp["region_id"]).tolist()


def rating_vectors_builder_main(data_dir, last_days_count, max_rated_places, max_rated_categories, tz=None):
    """RatingVectorsBuilderMain.doMain (:15-76) without Spark: location_visits_sample + places_sample -> place_visits and,
    for every region and every pair of regions, place_rating_vectors / category_rating_vectors / place_ratings under
    the names the recommender main reads back (DataUtils.scala:42-60).  Every step between the loads and the files
    runs on the device, the per-set rows coming from one prep.RegionSetPlan.  tz: the session time zone of
    calcVisitsFromTimestamp (UTC by default).  -> the region sets written, in order."""
    from . import prep
    place_visits, region_ids = _device_place_visits(data_dir, last_days_count, tz)
    plan = prep.RegionSetPlan(place_visits, region_ids)
    none = np.empty(0, np.int64)
    written = []
    for rs in prep.region_sets(region_ids):
        names = [generate_file_name(rs, data_dir, f) for f in ("place_rating_vectors", "category_rating_vectors", "place_ratings")]
        if plan.count(rs) == 0:
            write_rating_vectors(names[0], none, None, none, none, 0)
            write_rating_vectors(names[1], none, None, none, none, 0)
            write_place_ratings(names[2], none, none, none)
        else:
            pv = plan.place_visits(rs)
            pp, pe, pr = prep.calc_ratings(pv["person_id"], pv["place_id"], max_rated_places)
            cp, ce, cr = prep.calc_ratings(pv["person_id"], pv["category_id"], max_rated_categories)
            write_rating_vectors(names[0], *prep.calc_rating_vectors(pp, pe, pr))
            write_rating_vectors(names[1], *prep.calc_rating_vectors(cp, ce, cr))
            write_place_ratings(names[2], pp, pe, pr)
        written.append(rs)
    return written


def stochastic_graph_builder_main(data_dir, last_days_count, beta_person_place, beta_person_category, tz=None):
    """StochasticGraphBuilderMain.doMain (:18-45) without Spark: the two sample tables -> place_visits and one
    stochastic_graph set per region and per pair of regions (DataUtils.scala:33-35), every set's four edge families
    and their balancing computed on the device from one prep.RegionSetPlan.  -> the region sets written, in order."""
    from . import prep
    place_visits, region_ids = _device_place_visits(data_dir, last_days_count, tz)
    plan = prep.RegionSetPlan(place_visits, region_ids)
    none = np.empty(0, np.int64)
    written = []
    for rs in prep.region_sets(region_ids):
        name = generate_file_name(rs, data_dir, "stochastic_graph")
        if plan.count(rs) == 0:
            write_stochastic_graph(name, none, none, np.empty(0, np.float64))
        else:
            write_stochastic_graph(name, *prep.generate_stochastic_graph(plan.place_visits(rs), beta_person_place,
                                                                         beta_person_category))
        written.append(rs)
    return written


# ---- the head of the chain: SampleGeneratorMain.doMain (sample-generator/.../SampleGeneratorMain.scala:46-72) ---------------

def sample_generator_main(data_dir, place_count, person_count, regions, categories, seed=0, shared_factor=True, year=2018):
    """SampleGeneratorMain.doMain without Spark: persons_sample, location_visits_sample, places_sample and categories_sample
    under data_dir, generated on the device (sample.generate) and written with one part file each, the reference's
    partition columns as plain columns: timestamp as a Parquet timestamp of milliseconds, region_id / home_region_id as
    int32 (what Spark infers for a partition value), year_month as a string such as "201803"; places carry name and
    description.  The regions and category names are the caller's (the reference's own are literals of its program).
    -> the tables as sample.generate returns them (CUDA tensors), ready for prep.calc_place_visits."""
    import pyarrow as pa
    from . import _cache, sample
    _cache.require_gpu_backend("sample_generator_main")
    t = sample.generate(place_count, person_count, regions, categories, seed=seed, shared_factor=shared_factor, year=year,
                        device=True)
    persons, visits, places, cats = t["persons"], t["location_visits"], t["places"], t["categories"]
    _write_dir(os.path.join(data_dir, "persons_sample"),
               pa.table([pa.array(_host(persons["id"], np.int64), pa.int64()),
                         pa.array(_host(persons["home_region_id"], np.int32), pa.int32())], names=["id", "home_region_id"]))
    ym = _host(visits["year_month"], np.int32)
    _write_dir(os.path.join(data_dir, "location_visits_sample"),
               pa.table([pa.array(_host(visits["person_id"], np.int64), pa.int64()),
                         pa.array(_host(visits["latitude"], np.float64), pa.float64()),
                         pa.array(_host(visits["longitude"], np.float64), pa.float64()),
                         pa.array(_host(visits["timestamp"], np.int64), pa.int64()).cast(pa.timestamp("ms")),
                         pa.array(_host(visits["region_id"], np.int32), pa.int32()),
                         pa.array(np.char.zfill(ym.astype(str), 6) if len(ym) else np.empty(0, str), pa.string())],
                        names=["person_id", "latitude", "longitude", "timestamp", "region_id", "year_month"]))
    names = sample.decode_names(places["name_offsets"], places["name_units"])
    _write_dir(os.path.join(data_dir, "places_sample"),
               pa.table([pa.array(_host(places["id"], np.int64), pa.int64()),
                         pa.array(_host(places["latitude"], np.float64), pa.float64()),
                         pa.array(_host(places["longitude"], np.float64), pa.float64()),
                         pa.array(_host(places["category_id"], np.int64), pa.int64()),
                         pa.array(names, pa.string()), pa.array(names, pa.string()),
                         pa.array(_host(places["region_id"], np.int32), pa.int32())],
                        names=["id", "latitude", "longitude", "category_id", "name", "description", "region_id"]))
    _write_dir(os.path.join(data_dir, "categories_sample"),
               pa.table([pa.array(cats["category"], pa.string()), pa.array(cats["category_id"], pa.int64())],
                        names=["category", "category_id"]))
    return t


# ---- the tail of the chain: one request line of the recommender mains (RecommenderMainCommon.scala:16-56) -------------------

class NoSuchElementException(LookupError):
    """java.util.NoSuchElementException: the person of a request is not in persons_sample (RecommenderMainCommon.scala:54)."""


_INPUT_REGEX = r"(\d+)\s*(\d+)?"   # RecommenderMainCommon.scala:16; matched whole, ASCII digits and white space
_LONG_MAX = 2 ** 63 - 1


def parse_input(line):
    """RecommenderMainCommon.parseInput (:18-25): "person [region]" -> (person_id, region_id or None).  A line that does
    not match as a whole, or a number that does not fit a Long (String.toLong throws NumberFormatException, itself an
    IllegalArgumentException): IllegalArgumentException("Failed to parse input: ...")."""
    import re
    m = re.fullmatch(_INPUT_REGEX, line, flags=re.ASCII) if isinstance(line, str) else None
    if m is None:
        raise L.IllegalArgumentException(f"Failed to parse input: {line}")
    person, region = int(m.group(1)), (None if m.group(2) is None else int(m.group(2)))
    if person > _LONG_MAX or (region is not None and region > _LONG_MAX):
        raise L.IllegalArgumentException(f"Failed to parse input: {line}")
    return person, region


def load_persons(data_dir):
    """persons_sample (LocationVisitsSampleGenerator.scala:70-76; read by KnnRecommenderMain / StochasticRecommenderMain)
    -> dict(id, home_region_id) of int64 columns."""
    t = _read(os.path.join(data_dir, "persons_sample"), ["id", "home_region_id"])
    return {"id": _column_i64(t["id"]), "home_region_id": _column_i64(t["home_region_id"])}


def calc_recommender_target(persons, person_id_input_region_id):
    """RecommenderMainCommon.calcRecommenderTarget (:27-56): (person_id, region or None) -> (person_id, home_region_id,
    target_region_id), the target falling back to the person's home region.  A person that persons (dict(id,
    home_region_id)) does not hold: NoSuchElementException("Person not found: <id>")."""
    person_id, input_region = person_id_input_region_id
    rows = np.flatnonzero(_host(persons["id"], np.int64) == int(person_id))
    if len(rows) == 0:
        raise NoSuchElementException(f"Person not found: {person_id}")
    home = int(_host(persons["home_region_id"], np.int64)[rows[0]])   # where(id === personId).limit(1)
    return int(person_id), home, home if input_region is None else int(input_region)


def knn_recommender_request(data_dir, persons, line, place_weight, category_weight, k_nearest, max_recommendations=10,
                            new_places=False):
    """The body of KnnRecommenderMain's loop for one input line (KnnRecommenderMain.scala:36-51,90-101): parse, resolve
    the target, recommend from the region set [home, target], rank against the target region's places on the device.
    -> ((person_id, home_region_id, target_region_id), place_ids, estimated_ratings).
    new_places=True: without the places the person has rated (knn_recommend_places_batch's, for the one request)."""
    from . import prep
    target = calc_recommender_target(persons, parse_input(line))
    if new_places:
        oi, osc, cnt = knn_recommend_places_batch(data_dir, [target[1], target[2]], [(target[0], target[2])], place_weight,
                                                  category_weight, k_nearest, max_recommendations, new_places=True)
        return target, np.array(oi[0, :cnt[0]]), np.array(osc[0, :cnt[0]])
    ids, scores = knn_make_recommendations(data_dir, [target[1], target[2]], target[0], place_weight, category_weight, k_nearest)
    place_ids, place_regions = load_places(data_dir)
    return (target,) + tuple(prep.rank_recommendations(ids, scores, place_ids, place_regions, target[2], max_recommendations))


def knn_recommender_requests(data_dir, persons, lines, place_weight, category_weight, k_nearest, max_recommendations=10,
                             pooled=True):
    """The body of KnnRecommenderMain's loop (KnnRecommenderMain.scala:36-67,90-101) for a LIST of input lines, under
    sg_recommender_requests' contract: every line is parsed and resolved on its own, the index of [home, target] comes
    from the handle cache (one handle per distinct region set, knn_make_recommendations' key), and ONE
    KnnPool.recommend_ranked_batch call serves the good lines with the places table passed once - ranked on the device,
    max_recommendations rows a line come back.  A line whose person its index lacks is recorded and the call repeated
    without it.
    -> a list aligned with lines: ((person_id, home_region_id, target_region_id), place_ids, estimated_ratings), exactly
    what knn_recommender_request returns for that line, or the exception instance that function would have raised.
    pooled=False: one KnnIndex.recommend_ranked_batch call per distinct index instead of the pool call (the same
    result; what a queue cost before the pool)."""
    return _knn_recommender_requests(data_dir, persons, lines, place_weight, category_weight, k_nearest, max_recommendations,
                                     pooled, False)


def knn_recommender_requests_new_places(data_dir, persons, lines, place_weight, category_weight, k_nearest,
                                        max_recommendations=10):
    """knn_recommender_requests recommending only new places (that function's signature is fixed, so this is its sibling,
    as sg_recommender_requests_ranked is): every line's ranking leaves out the places its person has rated - what
    knn_recommender_request returns for the line with new_places=True, or the exception instance.  Served through
    _knn_requests_per_index by one unvisited ranked batch per distinct index; the pool has no unvisited form."""
    return _knn_recommender_requests(data_dir, persons, lines, place_weight, category_weight, k_nearest, max_recommendations,
                                     False, True)


def _knn_recommender_requests(data_dir, persons, lines, place_weight, category_weight, k_nearest, max_recommendations, pooled,
                              new_places):
    from . import _cache
    from .knn import KnnPool
    _cache.require_gpu_backend("knn_recommender_requests")
    out, targets, indexes = _knn_resolve_request_lines(data_dir, persons, lines)
    try:
        if targets:
            place_ids, place_regions = load_places(data_dir)
            pool = KnnPool(indexes) if pooled and not new_places else None
            try:
                def call(gi, v, live):
                    regions = np.asarray([targets[i][0][2] for i in live], np.int64)
                    if pool is None:
                        return _knn_requests_per_index(indexes, gi, v, place_weight, category_weight, k_nearest, place_ids,
                                                       place_regions, regions, max_recommendations, unvisited=new_places)
                    return pool.recommend_ranked_batch(gi, v, place_weight, category_weight, k_nearest, place_ids, place_regions,
                                                       regions, max_recommendations)
                live, rows = _call_without_bad_lines(out, targets, call)
            finally:
                if pool is not None:
                    pool.close()
            if live:
                oi, osc, cnt = rows
                for k, i in enumerate(live):
                    out[i] = (targets[i][0], np.array(oi[k, :cnt[k]]), np.array(osc[k, :cnt[k]]))
    finally:
        for ix in indexes:
            ix.close()  # drops the reference only
    return out


def _knn_requests_per_index(indexes, index_of, person_ids, pw, cw, k, place_ids, place_regions, regions, max_recommendations,
                            unvisited=False):
    """KnnPool.recommend_ranked_batch's result from one KnnIndex.recommend_ranked_batch call per distinct index; an unknown
    person raises with bad_request = the position of a request that names it, as the pool call does."""
    n = len(person_ids)
    width = max(0, min(int(max_recommendations), len(place_ids)))
    oi, osc, cnt = np.full((n, width), -1, np.int64), np.zeros((n, width), np.float64), np.zeros(n, np.int64)
    for k_ix in np.unique(index_of):
        at = np.flatnonzero(index_of == k_ix)
        try:
            with indexes[k_ix].lock:
                oi[at], osc[at], cnt[at] = indexes[k_ix].recommend_ranked_batch(person_ids[at], pw, cw, k, place_ids, place_regions,
                                                                                regions[at], max_recommendations,
                                                                                unvisited=unvisited)
        except L.IllegalArgumentException as e:
            head, _, unknown = str(e).rpartition(": ")
            if head == "No such person":  # (the library checks the ids in order and names the first)
                e.bad_request = int(at[np.flatnonzero(person_ids[at] == int(unknown))[0]])
            raise
    return oi, osc, cnt


def sg_recommender_request(data_dir, persons, line, epsilon, max_iterations, max_recommendations=10, new_places=False):
    """The body of StochasticRecommenderMain's loop for one input line (StochasticRecommenderMain.scala:36-51,64-75).
    -> ((person_id, home_region_id, target_region_id), ids, probabilities).
    new_places=True: without the targets of the person's out-edges (sg_recommend_places_batch's, for the one request)."""
    from . import prep
    target = calc_recommender_target(persons, parse_input(line))
    if new_places:
        from .stochastic import ALPHA
        oi, op, cnt, _, _ = sg_recommend_places_batch(data_dir, [target[1], target[2]], [(target[0], target[2])], epsilon,
                                                      max_iterations, ALPHA, max_recommendations, new_places=True)
        return target, np.array(oi[0, :cnt[0]]), np.array(op[0, :cnt[0]])
    ids, scores, _, _ = sg_make_recommendations(data_dir, [target[1], target[2]], target[0], epsilon, max_iterations)
    place_ids, place_regions = load_places(data_dir)
    return (target,) + tuple(prep.rank_recommendations(ids, scores, place_ids, place_regions, target[2], max_recommendations))


def sg_recommender_requests(data_dir, persons, lines, epsilon, max_iterations, max_recommendations=10, pooled=True):
    """The body of StochasticRecommenderMain's loop (StochasticRecommenderMain.scala:36-62,64-75) for a LIST of input
    lines: every line is parsed and resolved on its own, the graph of [home, target] comes from the handle cache (one
    handle per distinct region set), ONE pool call (stochastic.SgPool) serves all lines, and the rows are ranked per line
    against its own target region by one call of the segmented ranker.
    -> a list aligned with lines: ((person_id, home_region_id, target_region_id), ids, probabilities), exactly what
    sg_recommender_request returns for that line, or the exception instance that function would have raised (the
    reference wraps each line in Try, :44-49).  pooled=False: one SgGraph.recommend_batch call per distinct graph instead
    of the pool call (the same result; the A/B partner)."""
    return _sg_recommender_requests(data_dir, persons, lines, epsilon, max_iterations, max_recommendations, pooled, False)


def sg_recommender_requests_new_places(data_dir, persons, lines, epsilon, max_iterations, max_recommendations=10, pooled=True):
    """sg_recommender_requests recommending only new places (that function's signature is fixed, so this is its sibling,
    as sg_recommender_requests_ranked is): every line's ranking leaves out the targets of its person's out-edges in the
    edge Parquet of its region set (load_stochastic_graph, out_neighbours), ranked by the excluding form of the segmented
    ranker - what sg_recommender_request returns for the line with new_places=True, or the exception instance."""
    return _sg_recommender_requests(data_dir, persons, lines, epsilon, max_iterations, max_recommendations, pooled, True)


def _sg_recommender_requests(data_dir, persons, lines, epsilon, max_iterations, max_recommendations, pooled, new_places):
    from . import _cache, prep
    from .stochastic import ALPHA, SgPool
    _cache.require_gpu_backend("sg_recommender_requests")
    out, targets, graphs = _sg_resolve_request_lines(data_dir, persons, lines)
    try:
        def call(gi, v, live):
            if not pooled:
                return _sg_requests_per_graph(graphs, gi, v, ALPHA, epsilon, max_iterations)
            pool = SgPool(graphs)
            try:
                return pool.recommend_batch(gi, v, ALPHA, epsilon, max_iterations)
            finally:
                pool.close()
        live, rows = _call_without_bad_lines(out, targets, call)
        if live:
            off, ids, probs, _, _ = rows
            place_ids, place_regions = load_places(data_dir)
            regions = np.asarray([targets[i][0][2] for i in live], np.int64)
            if new_places:
                # one edge list per distinct graph; the lists in the lines' order
                v = np.asarray([targets[i][0][0] for i in live], np.int64)
                gi = np.asarray([targets[i][1] for i in live], np.int32)
                lists = [None] * len(live)
                for g_ix in np.unique(gi):
                    at = np.flatnonzero(gi == g_ix)
                    home, region = targets[live[at[0]]][0][1:3]
                    xoff, xids = _sg_visited_lists(data_dir, [home, region], v[at])
                    for j, k in enumerate(at):
                        lists[k] = xids[xoff[j]:xoff[j + 1]]
                xoff = np.zeros(len(live) + 1, np.int64)
                np.cumsum([len(x) for x in lists], out=xoff[1:])
                oi, op, cnt = prep.rank_recommendations_batch_excluding(off, ids, probs, place_ids, place_regions, regions,
                                                                        max_recommendations, xoff,
                                                                        np.concatenate(lists).astype(np.int64))
            else:
                oi, op, cnt = prep.rank_recommendations_batch(off, ids, probs, place_ids, place_regions, regions, max_recommendations)
            for k, i in enumerate(live):
                out[i] = (targets[i][0], np.array(oi[k, :cnt[k]]), np.array(op[k, :cnt[k]]))
    finally:
        for g in graphs:
            g.close()  # drops the reference only
    return out


def sg_recommender_requests_ranked(data_dir, persons, lines, epsilon, max_iterations, max_recommendations=10):
    """sg_recommender_requests with the ranking on the device: the same per-line contract (every line parsed and resolved
    on its own, graphs from the handle cache, the exception instance per bad line, a line whose vertex its graph lacks
    recorded and the call repeated without it), served by ONE SgPool.recommend_ranked_batch call with the places table
    passed once - no graph's probabilities leave the device, max_recommendations rows a line come back.
    -> the list sg_recommender_requests returns."""
    from . import _cache
    from .stochastic import ALPHA, SgPool
    _cache.require_gpu_backend("sg_recommender_requests_ranked")
    out, targets, graphs = _sg_resolve_request_lines(data_dir, persons, lines)
    try:
        if targets:
            place_ids, place_regions = load_places(data_dir)
            pool = SgPool(graphs)
            try:
                def call(gi, v, live):
                    regions = np.asarray([targets[i][0][2] for i in live], np.int64)
                    return pool.recommend_ranked_batch(gi, v, ALPHA, epsilon, max_iterations, place_ids, place_regions, regions,
                                                       max_recommendations)
                live, rows = _call_without_bad_lines(out, targets, call)
            finally:
                pool.close()
            if live:
                oi, op, cnt, _, _ = rows
                for k, i in enumerate(live):
                    out[i] = (targets[i][0], np.array(oi[k, :cnt[k]]), np.array(op[k, :cnt[k]]))
    finally:
        for g in graphs:
            g.close()  # drops the reference only
    return out


def _near_request_circles(lines, positions, radius_meters):
    """The circles of a near request list -> (lat[n], lon[n], radius[n]) float64: positions = (lat[n], lon[n]), the radius a
    scalar or one value per line."""
    lat, lon = (np.asarray(p, np.float64) for p in positions)
    rad = np.asarray(radius_meters, np.float64)
    rad = np.full(len(lines), float(rad)) if rad.ndim == 0 else rad
    if not len(lat) == len(lon) == len(rad) == len(lines):
        raise L.IllegalArgumentException("one position per line and a scalar radius or one per line are required")
    return lat, lon, rad


def _near_requests(kind, resolve_lines, per_handle, data_dir, persons, lines, positions, radius_meters, max_recommendations,
                   with_lines=False):
    """What both near request functions share: the lines resolved as ever, the place table with its coordinates
    (load_places_full), one near ranked batch per distinct handle (per_handle(handle, person_ids, regions, places, lat,
    lon, rad, target of the handle's first line) -> (ids, scores, meters, counts) for the lines of that handle), a bad
    line recorded and the call repeated without it.  -> per line ((person, home, target), ids, scores, meters) or the exception instance.
    with_lines: per_handle also gets the positions of its lines in `lines` (the by-category functions' lists and caps are
    per line), and positions None is no circles: lat, lon and rad are None and so are the meters."""
    from . import _cache
    _cache.require_gpu_backend(kind)
    circles = positions is not None
    lat, lon, rad = _near_request_circles(lines, positions, radius_meters) if circles else (None, None, None)
    out, targets, handles = resolve_lines(data_dir, persons, lines)
    try:
        if targets:
            places = load_places_full(data_dir)
            width = max(0, int(max_recommendations))

            def call(gi, v, live):
                at_lines = np.asarray(live, np.int64)
                regions = np.asarray([targets[i][0][2] for i in live], np.int64)
                n = len(live)
                oi, osc, om = np.full((n, width), -1, np.int64), np.zeros((n, width), np.float64), np.zeros((n, width), np.float64)
                cnt = np.zeros(n, np.int64)
                for k in np.unique(gi):
                    at = np.flatnonzero(gi == k)
                    try:
                        with handles[k].lock:
                            la = at_lines[at]
                            r = per_handle(handles[k], v[at], regions[at], places, *((lat[la], lon[la], rad[la]) if circles
                                                                                     else (None, None, None)),
                                           targets[live[at[0]]][0], *((la,) if with_lines else ()))
                    except L.IllegalArgumentException as e:
                        head, _, unknown = str(e).rpartition(": ")
                        if head in ("No such person", "No such vertex in the graph"):
                            e.bad_request = int(at[np.flatnonzero(v[at] == int(unknown))[0]])
                        raise
                    w = r[0].shape[1]
                    oi[at, :w], osc[at, :w], cnt[at] = r[0], r[1], r[3]
                    if circles:
                        om[at, :w] = r[2]
                return oi, osc, om, cnt
            live, rows = _call_without_bad_lines(out, targets, call)
            if live:
                oi, osc, om, cnt = rows
                for k, i in enumerate(live):
                    out[i] = (targets[i][0], np.array(oi[k, :cnt[k]]), np.array(osc[k, :cnt[k]]),
                              np.array(om[k, :cnt[k]]) if circles else None)
    finally:
        for h in handles:
            h.close()  # drops the reference only
    return out


def knn_recommender_requests_near(data_dir, persons, lines, positions, radius_meters, place_weight, category_weight, k_nearest,
                                  max_recommendations=10, new_places=False):
    """knn_recommender_requests within reach: line i is resolved as ever (parse_input, calc_recommender_target) and ranked
    among the places of its target region no further than radius_meters (a scalar or one value per line; >= 0 or +inf)
    from positions = (lat[n], lon[n])[i] - KnnIndex.recommend_ranked_batch_near, one call per distinct index, the place
    table from load_places_full.  new_places=True: without the places the person has rated.
    -> a list aligned with lines: ((person_id, home_region_id, target_region_id), place_ids, estimated_ratings, meters)
    or the exception instance; a line whose person its index lacks is recorded and the call repeated without it."""
    def per_index(ix, person_ids, regions, places, lat, lon, rad, _target):
        return ix.recommend_ranked_batch_near(person_ids, place_weight, category_weight, k_nearest, places["id"],
                                              places["region_id"], places["latitude"], places["longitude"], regions, lat, lon,
                                              rad, max_recommendations, unvisited=new_places)
    return _near_requests("knn_recommender_requests_near", _knn_resolve_request_lines, per_index, data_dir, persons, lines,
                          positions, radius_meters, max_recommendations)


def sg_recommender_requests_near(data_dir, persons, lines, positions, radius_meters, epsilon, max_iterations,
                                 max_recommendations=10, new_places=False):
    """sg_recommender_requests within reach, as knn_recommender_requests_near: SgGraph.recommend_ranked_batch_near, one call
    per distinct graph.  new_places=True: without the targets of the person's out-edges in its region set's edge Parquet.
    -> a list aligned with lines: ((person_id, home_region_id, target_region_id), ids, probabilities, meters) or the
    exception instance; a line whose vertex its graph lacks is recorded and the call repeated without it."""
    from .stochastic import ALPHA

    def per_graph(g, vertex_ids, regions, places, lat, lon, rad, target):
        excluded = _sg_visited_lists(data_dir, [target[1], target[2]], vertex_ids) if new_places else None
        return g.recommend_ranked_batch_near(vertex_ids, ALPHA, epsilon, max_iterations, places["id"], places["region_id"],
                                             places["latitude"], places["longitude"], regions, lat, lon, rad,
                                             max_recommendations, excluded=excluded)[:4]
    return _near_requests("sg_recommender_requests_near", _sg_resolve_request_lines, per_graph, data_dir, persons, lines,
                          positions, radius_meters, max_recommendations)


def _category_request_lists(lines, categories, max_per_category):
    """The lists and caps of a by-category request list.  categories: None, one list of category ids for every line, or
    one list per line (an empty list allows every category); max_per_category: None, a scalar or one value per line.
    -> (allowed (offsets[n + 1], ids) or None, caps[n] or None), per line."""
    n = len(lines)
    allowed = caps = None
    if categories is not None:
        per_line = len(categories) > 0 and all(np.ndim(c) == 1 for c in categories)
        lists = [np.asarray(c, np.int64) for c in categories] if per_line else [np.asarray(categories, np.int64).reshape(-1)] * n
        if len(lists) != n:
            raise L.IllegalArgumentException("one list of categories for every line or one per line is required")
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(x) for x in lists], out=off[1:])
        allowed = (off, np.concatenate(lists + [np.empty(0, np.int64)]).astype(np.int64))
    if max_per_category is not None:
        caps = np.asarray(max_per_category, np.int64)
        caps = np.full(n, int(caps), np.int64) if caps.ndim == 0 else caps
        if len(caps) != n:
            raise L.IllegalArgumentException("a scalar max_per_category or one per line is required")
    return allowed, caps


def _category_sub_lists(allowed, caps, at):
    """The lists and caps of the lines `at`, as a CSR of their own."""
    sub_allowed = None
    if allowed is not None:
        off, ids = allowed
        lists = [ids[off[i]:off[i + 1]] for i in at]
        sub_off = np.zeros(len(at) + 1, np.int64)
        np.cumsum([len(x) for x in lists], out=sub_off[1:])
        sub_allowed = (sub_off, np.concatenate(lists + [np.empty(0, np.int64)]).astype(np.int64))
    return sub_allowed, None if caps is None else caps[at]


def knn_recommender_requests_by_category(data_dir, persons, lines, place_weight, category_weight, k_nearest,
                                         max_recommendations=10, categories=None, max_per_category=None, new_places=False,
                                         positions=None, radius_meters=None):
    """knn_recommender_requests by category: line i is resolved as ever and ranked among the places of its target region
    whose category_id (places_sample) is in `categories` - None: any; one list of ids for every line, or one list per
    line - with at most max_per_category (None: no cap; a scalar or one value per line) places of one category -
    KnnIndex.recommend_ranked_batch_by_category, one call per distinct index.  positions = (lat[n], lon[n]) and
    radius_meters: within reach as well, as knn_recommender_requests_near.  new_places=True: without the places the
    person has rated.
    -> a list aligned with lines: ((person_id, home_region_id, target_region_id), place_ids, estimated_ratings, meters or
    None without positions) or the exception instance."""
    allowed, caps = _category_request_lists(lines, categories, max_per_category)

    def per_index(ix, person_ids, regions, places, lat, lon, rad, _target, at):
        sub_allowed, sub_caps = _category_sub_lists(allowed, caps, at)
        circles = None if lat is None else (places["latitude"], places["longitude"], lat, lon, rad)
        return ix.recommend_ranked_batch_by_category(person_ids, place_weight, category_weight, k_nearest, places["id"],
                                                     places["region_id"], regions, max_recommendations, places["category_id"],
                                                     allowed=sub_allowed, max_per_category=sub_caps, circles=circles,
                                                     unvisited=new_places)
    return _near_requests("knn_recommender_requests_by_category", _knn_resolve_request_lines, per_index, data_dir, persons,
                          lines, positions, radius_meters, max_recommendations, with_lines=True)


def sg_recommender_requests_by_category(data_dir, persons, lines, epsilon, max_iterations, max_recommendations=10,
                                        categories=None, max_per_category=None, new_places=False, positions=None,
                                        radius_meters=None):
    """sg_recommender_requests by category, as knn_recommender_requests_by_category:
    SgGraph.recommend_ranked_batch_by_category, one call per distinct graph.  new_places=True: without the targets of the
    person's out-edges in its region set's edge Parquet.
    -> a list aligned with lines: ((person_id, home_region_id, target_region_id), ids, probabilities, meters or None) or
    the exception instance."""
    from .stochastic import ALPHA
    allowed, caps = _category_request_lists(lines, categories, max_per_category)

    def per_graph(g, vertex_ids, regions, places, lat, lon, rad, target, at):
        sub_allowed, sub_caps = _category_sub_lists(allowed, caps, at)
        excluded = _sg_visited_lists(data_dir, [target[1], target[2]], vertex_ids) if new_places else None
        circles = None if lat is None else (places["latitude"], places["longitude"], lat, lon, rad)
        return g.recommend_ranked_batch_by_category(vertex_ids, ALPHA, epsilon, max_iterations, places["id"], places["region_id"],
                                                    regions, max_recommendations, places["category_id"], allowed=sub_allowed,
                                                    max_per_category=sub_caps, circles=circles, excluded=excluded)[:4]
    return _near_requests("sg_recommender_requests_by_category", _sg_resolve_request_lines, per_graph, data_dir, persons, lines,
                          positions, radius_meters, max_recommendations, with_lines=True)


def _sg_resolve_request_lines(data_dir, persons, lines, resolve=None):
    """The line-resolution loop of sg_recommender_requests and sg_recommender_requests_ranked: every line is parsed and
    resolved on its own (Try { ... } per line, :44-49) and the graph of [home, target] comes from the handle cache, one
    handle per distinct region set.
    -> (out, targets, graphs): out aligned with lines, the exception instance at every bad line and None elsewhere;
    targets[i] = ((person_id, home_region_id, target_region_id), index into graphs) for every good line i.  The caller
    closes the graphs.  resolve: what turns a line into that triple in place of parsing it."""
    from . import _cache
    from .stochastic import SgGraph

    def open_graph(region_ids):
        name = generate_file_name(region_ids, data_dir, "stochastic_graph")
        return name, lambda: SgGraph.through_cache(_cache.files_key([name]), lambda: sg_graph_from_parquet(data_dir, region_ids))
    return _resolve_request_lines(persons, lines, open_graph, resolve)


def _knn_resolve_request_lines(data_dir, persons, lines, resolve=None):
    """_sg_resolve_request_lines for the KNN main: the index of [home, target] from the handle cache under
    knn_make_recommendations' key, one handle per distinct region set.  -> (out, targets, indexes).
    resolve: what turns a line into (person_id, home_region_id, target_region_id) in place of parsing it."""
    from . import _cache
    from .knn import KnnIndex

    def open_index(region_ids):
        names = tuple(generate_file_name(region_ids, data_dir, f)
                      for f in ("place_rating_vectors", "category_rating_vectors", "place_ratings"))
        return names, lambda: KnnIndex.through_cache(_cache.files_key(list(names)),
                                                     lambda: knn_index_from_parquet(data_dir, region_ids))
    return _resolve_request_lines(persons, lines, open_index, resolve)


def _resolve_request_lines(persons, lines, open_handle, resolve=None):
    """Every line parsed and resolved on its own; open_handle([home, target]) -> (the region set's name, a function that
    takes its handle from the cache), called once per distinct name - a failure is remembered and raised for every line
    of that region set.  -> (out, targets, handles) as _sg_resolve_request_lines describes them."""
    out = [None] * len(lines)
    targets, handle_of, handles, failed = {}, {}, [], {}
    try:
        for i, line in enumerate(lines):
            try:
                target = resolve(line) if resolve is not None else calc_recommender_target(persons, parse_input(line))
                name, take = open_handle([target[1], target[2]])
                if name in failed:
                    raise failed[name]
                if name not in handle_of:
                    try:
                        h = take()
                    except Exception as e:
                        failed[name] = e
                        raise
                    handle_of[name] = len(handles)
                    handles.append(h)
                targets[i] = (target, handle_of[name])
            except Exception as e:  # Try { ... } per line
                out[i] = e
    except BaseException:
        for h in handles:
            h.close()
        raise
    return out, targets, handles


def _call_without_bad_lines(out, targets, call):
    """call(graph_index, vertex_ids, live) for the good lines `live`; a line whose vertex is not in its graph - or whose
    person is not in its index - (the call raises with bad_request set) is recorded in out and the call repeated without
    it.  -> (live, the call's result)."""
    live = sorted(targets)
    rows = None
    while live and rows is None:
        gi = np.asarray([targets[i][1] for i in live], np.int32)
        v = np.asarray([targets[i][0][0] for i in live], np.int64)
        try:
            rows = call(gi, v, live)
        except L.IllegalArgumentException as e:
            bad = getattr(e, "bad_request", getattr(e, "bad_visitor", -1))  # (a visitors call names the position so)
            if bad < 0:
                raise
            out[live.pop(bad)] = e  # the line's vertex is not in its graph: recorded, the call repeated without it
    return live, rows


def _sg_requests_per_graph(graphs, graph_index, vertex_ids, alpha, epsilon, max_iterations):
    """SgPool.recommend_batch's result from one SgGraph.recommend_batch call per distinct graph; an unknown vertex raises
    with bad_request = the position of a request that names it, as the pool call does."""
    n = len(vertex_ids)
    parts = [None] * n
    its, conv = np.zeros(n, np.int64), np.zeros(n, bool)
    for k in np.unique(graph_index):
        at = np.flatnonzero(graph_index == k)
        try:
            with graphs[k].lock:
                off, ids, probs, it, cv = graphs[k].recommend_batch(vertex_ids[at], alpha, epsilon, max_iterations)
        except L.IllegalArgumentException as e:
            head, _, unknown = str(e).rpartition(": ")
            if head == "No such vertex in the graph":  # (the library checks the ids in order and names the first)
                e.bad_request = int(at[np.flatnonzero(vertex_ids[at] == int(unknown))[0]])
            raise
        for j, i in enumerate(at):
            parts[i] = (ids[off[j]:off[j + 1]], probs[off[j]:off[j + 1]])
        its[at], conv[at] = it, cv
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(p[0]) for p in parts], out=off[1:])
    ids = np.concatenate([p[0] for p in parts]) if n else np.empty(0, np.int64)
    probs = np.concatenate([p[1] for p in parts]) if n else np.empty(0, np.float64)
    return off, ids, probs, its, conv


# ---- offline evaluation: split at a time, build from the train visits, rank, score (csrc/eval.hip) -------------------

def _holdout_requests(place_visits, cut_timestamp, new_places):
    """holdout_split, and the requests its triples ask for: one per (person, region) with held-out places, as host
    arrays in the triples' order."""
    from . import prep
    train, held = prep.holdout_split(place_visits, cut_timestamp, new_places_only=new_places)
    held = {k: _host(v, np.int64) for k, v in held.items()}   # the ranked calls take and return host arrays
    hp, hr = held["person_id"], held["region_id"]
    first = np.ones(len(hp), bool)
    first[1:] = (hp[1:] != hp[:-1]) | (hr[1:] != hr[:-1])
    return train, held, hp[first], hr[first]


def _evaluate_in_batches(rank, held, persons, regions, cutoffs, batch):
    """rank(persons, regions, n) -> (ids[S, W], counts[S]) for every batch of the requests, each scored by
    prep.evaluate_ranked.  The batches combine exactly: the metric SUMS (mean x evaluated) and the evaluated counts add
    up, never means of means; the coverage is the size of the union of the batches' recommended ids per cutoff.
    -> dict(means[n_cutoffs, 6], coverage[n_cutoffs], evaluated, relevant[n_requests], person_ids, region_ids)."""
    from . import prep
    cut = np.atleast_1d(np.asarray(cutoffs, np.int64))
    batch = max(1, int(batch))
    sums, evaluated, relevant = np.zeros((len(cut), 6)), 0, [np.empty(0, np.int64)]
    seen = [np.empty(0, np.int64) for _ in cut]
    for b in range(0, len(persons), batch):
        p, r = persons[b:b + batch], regions[b:b + batch]
        ids, counts = rank(p, r, int(cut.max()))
        off, rel = prep.relevant_lists(held, p, r)
        e = prep.evaluate_ranked(ids, counts, off, rel, cut)
        sums += e["means"] * e["evaluated"]
        evaluated += e["evaluated"]
        relevant.append(e["relevant"])
        live = np.arange(ids.shape[1])[None, :] < counts[:, None]
        for j, k in enumerate(cut):
            seen[j] = np.union1d(seen[j], ids[:, :k][live[:, :k]])
    return {"means": sums / evaluated if evaluated else sums, "coverage": np.array([len(s) for s in seen], np.int64),
            "evaluated": evaluated, "relevant": np.concatenate(relevant), "person_ids": persons, "region_ids": regions}


def knn_holdout_evaluation(place_visits, places, cut_timestamp, place_weight, category_weight, k_nearest, cutoffs,
                           new_places=True, batch=16384):
    """The hold-out protocol for the KNN recommender: the visit table (calc_place_visits' mapping, host or device) is
    cut at cut_timestamp, the index built from the train visits (prep.knn_index_from_visits), every train person ranked
    for each region it has held-out places in (recommend_ranked_batch, unvisited=new_places, `batch` requests a call)
    and the rows scored against those places at `cutoffs`.  new_places: only places the person has no train visit at
    are relevant - and recommended.  places: mapping with id and region_id.  -> _evaluate_in_batches' dict."""
    from . import prep
    train, held, persons, regions = _holdout_requests(place_visits, cut_timestamp, new_places)
    if len(persons) == 0:
        return _evaluate_in_batches(None, held, persons, regions, cutoffs, batch)
    pl, reg = _host(places["id"], np.int64), _host(places["region_id"], np.int64)
    ix = prep.knn_index_from_visits(train["person_id"], train["place_id"], train["category_id"])
    try:
        def rank(p, r, n):
            ids, _, counts = ix.recommend_ranked_batch(p, place_weight, category_weight, k_nearest, pl, reg, r, n,
                                                       unvisited=bool(new_places))
            return ids, counts
        return _evaluate_in_batches(rank, held, persons, regions, cutoffs, batch)
    finally:
        ix.close()


def sg_holdout_evaluation(place_visits, places, cut_timestamp, alpha, epsilon, max_iterations, beta_person_place,
                          beta_person_category, cutoffs, new_places=True, batch=16384):
    """The same protocol for the stochastic recommender: the graph is built from the train visits as
    prep.sg_graph_from_visits builds it (the edge list is kept, for the lists below), every train person's vertex ranked
    for each region it has held-out places in (recommend_ranked_batch), with new_places leaving out the person's
    out-neighbours - the places it has been to (stochastic.out_neighbours).  -> _evaluate_in_batches' dict."""
    from . import prep
    from .stochastic import SgGraph, out_neighbours
    train, held, persons, regions = _holdout_requests(place_visits, cut_timestamp, new_places)
    if len(persons) == 0:
        return _evaluate_in_batches(None, held, persons, regions, cutoffs, batch)
    pl, reg = _host(places["id"], np.int64), _host(places["region_id"], np.int64)
    s, t, w = prep.generate_stochastic_graph(train, beta_person_place, beta_person_category)
    g = SgGraph.from_device(s.contiguous(), t.contiguous(), w.contiguous()) if prep._is_tensor(s) else SgGraph(s, t, w)
    try:
        hs, ht = (_host(s, np.int64), _host(t, np.int64)) if new_places else (None, None)

        def rank(p, r, n):
            excluded = out_neighbours(hs, ht, p) if new_places else None
            ids, _, counts, _, _ = g.recommend_ranked_batch(p, alpha, epsilon, max_iterations, pl, reg, r, n, excluded=excluded)
            return ids, counts
        return _evaluate_in_batches(rank, held, persons, regions, cutoffs, batch)
    finally:
        g.close()
