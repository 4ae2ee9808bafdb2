"""Host-side mirror of knn/KnnRecommender.scala:9-25 over the C ABI.

Same constructor arguments, method name, column names and error behaviour as
the Scala class; the three DataFrames are pandas frames with the reference's
schemas (RatingVectorsBuilder.scala:81-82, RatingsBuilder.scala:38-47):
  placeRatingVectors / categoryRatingVectors: (person_id: long, rating_vector: SparseVector)
  placeRatings:                               (person_id: long, place_id: long, rating: long)
"""
import ctypes as C

import numpy as np

from . import _cache
from . import _lib as L


class SparseVector:
    """org.apache.spark.ml.linalg.SparseVector(size, indices, values)."""

    __slots__ = ("size", "indices", "values")

    def __init__(self, size, indices, values):
        self.size = int(size)
        self.indices = np.asarray(indices, dtype=np.int32)
        self.values = np.asarray(values, dtype=np.float64)
        if self.indices.shape != self.values.shape:
            raise L.IllegalArgumentException("requirement failed: Sparse vectors require that the dimension of the "
                                             "indices match the dimension of the values.")


def _vectors_to_csr(person_ids, frame):
    """Collect a (person_id, rating_vector) frame to CSR rows aligned with person_ids."""
    by_id = {int(p): v for p, v in zip(frame["person_id"], frame["rating_vector"])}
    sizes = {v.size for v in by_id.values()}
    if len(sizes) > 1:
        raise L.IllegalArgumentException(f"rating vectors of different sizes: {sorted(sizes)}")
    dim = sizes.pop() if sizes else 1
    rowptr = np.zeros(len(person_ids) + 1, dtype=np.int64)
    idx, val = [], []
    for i, p in enumerate(person_ids):
        v = by_id.get(int(p))
        if v is not None:
            idx.append(v.indices)
            val.append(v.values)
            rowptr[i + 1] = rowptr[i] + len(v.indices)
        else:
            rowptr[i + 1] = rowptr[i]
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int32)
    val = np.concatenate(val) if val else np.zeros(0, np.float64)
    return rowptr, L.as_i32(idx), L.as_f64(val), dim


class KnnIndex:
    """Owner of a locrec_knn_index handle (CSR in, device-resident afterwards)."""

    def __init__(self, person_ids, p_rowptr, p_idx, p_val, p_dim, c_rowptr, c_idx, c_val, c_dim,
                 r_rowptr=None, r_place=None, r_rating=None):
        lib = L.lib()
        self._h = C.c_void_p()
        self.person_ids = L.as_i64(person_ids)
        a = [L.as_i64(p_rowptr), L.as_i32(p_idx), L.as_f64(p_val), L.as_i64(c_rowptr), L.as_i32(c_idx), L.as_f64(c_val)]
        r = [None, None, None] if r_rowptr is None else [L.as_i64(r_rowptr), L.as_i64(r_place), L.as_i64(r_rating)]
        L.check(lib.locrec_knn_create(
            len(self.person_ids), L.ptr(self.person_ids, C.c_int64),
            L.ptr(a[0], C.c_int64), L.ptr(a[1], C.c_int32), L.ptr(a[2], C.c_double), int(p_dim),
            L.ptr(a[3], C.c_int64), L.ptr(a[4], C.c_int32), L.ptr(a[5], C.c_double), int(c_dim),
            L.ptr(r[0], C.c_int64), L.ptr(r[1], C.c_int64), L.ptr(r[2], C.c_int64), C.byref(self._h)))

    @classmethod
    def from_device(cls, person_ids, p_rowptr, p_idx, p_val, p_dim, c_rowptr, c_idx, c_val, c_dim,
                    r_rowptr=None, r_place=None, r_rating=None):
        """The same index from arrays that already live in DEVICE memory (torch tensors on the current
        GPU: int64 ids / row pointers / rating columns, int32 indices, float64 values): nothing passes
        through the host, the index is built by kernels (locrec_knn_create_from_device)."""
        import torch

        def dev(t, dtype):
            if t is None:
                return None
            assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), "device tensor of the ABI's dtype expected"
            return t

        t = [dev(person_ids, torch.int64), dev(p_rowptr, torch.int64), dev(p_idx, torch.int32), dev(p_val, torch.float64),
             dev(c_rowptr, torch.int64), dev(c_idx, torch.int32), dev(c_val, torch.float64),
             dev(r_rowptr, torch.int64), dev(r_place, torch.int64), dev(r_rating, torch.int64)]
        L.require_current_device(t)
        torch.cuda.current_stream().synchronize()  # the library reads the arrays on its own stream
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        ptr = [C.c_void_p(x.data_ptr()) if x is not None and x.numel() > 0 else None for x in t]
        L.check(L.lib().locrec_knn_create_from_device(
            int(t[0].numel()), ptr[0], ptr[1], ptr[2], ptr[3], int(p_dim), ptr[4], ptr[5], ptr[6], int(c_dim),
            ptr[7], ptr[8], ptr[9], C.byref(self._h)))
        self.person_ids = t[0].cpu().numpy()
        return self

    @classmethod
    def through_cache(cls, key, build):
        """The process-wide cached index for `key` (include/locrec.h, "Handle cache"); build() -> KnnIndex is
        called on a miss only and its handle becomes the cache's.  close() / garbage collection of the
        returned object drop a REFERENCE; the device index stays for the next constructor with this key."""
        h = _cache.acquire(L.CACHE_KNN, key)
        if h is None:
            before = L.device_bytes_in_use()
            built = build()
            h = _cache.publish(L.CACHE_KNN, key, built._h, L.device_bytes_in_use() - before)
            built._h = None          # owned by the cache now (or destroyed by it, if the key appeared meanwhile)
        self = cls.__new__(cls)
        self._h, self._cached, self.person_ids = h, True, None
        self.lock = _cache.handle_lock(h)
        return self

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_cached", False):
                _cache.release(L.CACHE_KNN, self._h)
            else:
                L.lib().locrec_knn_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def n(self):
        if self.person_ids is None:  # a cache hit never saw the input arrays
            if getattr(self, "_n", None) is None:
                self._n = self.info()["n"]
            return self._n
        return len(self.person_ids)

    def info(self):
        n, b, p = C.c_int64(), C.c_int64(), C.c_int32()
        L.check(L.lib().locrec_knn_info(self._h, C.byref(n), C.byref(b), C.byref(p)))
        bb = C.c_int64()
        L.check(L.lib().locrec_knn_batch_scan_bytes(self._h, C.byref(bb)))
        return {"n": n.value, "scan_bytes": b.value, "batch_scan_bytes": bb.value, "packed": bool(p.value), "mode": p.value}

    def ht_image_info(self):
        """{head_words, tail_postings, wide_rows} of the head / tail image (locrec_knn_ht_image_info)."""
        v = [C.c_int64() for _ in range(3)]
        L.check(L.lib().locrec_knn_ht_image_info(self._h, *[C.byref(x) for x in v]))
        return {"head_words": v[0].value, "tail_postings": v[1].value, "wide_rows": v[2].value}

    def ht_multiplied_words(self):
        """Words of the head / tail image knn_scan_ht multiplies per query tile: 64 x the exact element counts of every
        slice's widest row (locrec_knn_ht_multiplied_words); head_words of ht_image_info() counts the stored ones."""
        v = C.c_int64()
        L.check(L.lib().locrec_knn_ht_multiplied_words(self._h, C.byref(v)))
        return v.value

    def ht_slice_counts(self):
        """(place, category) element counts of every slice's widest row, as knn_scan_ht reads them: int32 array [slices, 2]."""
        ns = C.c_int64()
        L.check(L.lib().locrec_knn_ht_slice_counts(self._h, 0, None, None, C.byref(ns)))
        p, c = np.zeros(ns.value, np.int32), np.zeros(ns.value, np.int32)
        if ns.value:
            L.check(L.lib().locrec_knn_ht_slice_counts(self._h, ns.value, p.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       c.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ns)))
        return np.stack([p, c], axis=1)

    def ht_lds_model(self):
        """{group_reads, cycles} of the head / tail image under the LDS model of its element order
        (locrec_knn_ht_lds_model): reads of one position by one group of 16 lanes, and the cycles they take when
        different panel rows on one slot cost a cycle each.  cycles - group_reads = modelled conflict cycles."""
        r, c = C.c_int64(), C.c_int64()
        L.check(L.lib().locrec_knn_ht_lds_model(self._h, C.byref(r), C.byref(c)))
        return {"group_reads": r.value, "cycles": c.value}

    def aggregate_stats(self):
        """Queries the LDS aggregation has served on this index since the previous call (locrec_knn_aggregate_stats):
        {buckets, sort, flagged} - summed by knn_aggregate_buckets, summed by knn_aggregate (a redone query, an index with
        too many places, LOCREC_KNN_AGG_SORT), left flagged for the host.  Reads and resets the device counters."""
        v = (C.c_int64 * 3)()
        L.check(L.lib().locrec_knn_aggregate_stats(self._h, v))
        return {"buckets": int(v[0]), "sort": int(v[1]), "flagged": int(v[2])}

    def ht_last_hits(self, nq):
        """What the hit pre-pass of the last batched head / tail scan - of nq queries - left on the device
        (locrec_knn_ht_last_hits): {query_tile, tiles, slice0, nslices, tile_base int64[tiles + 1],
        off uint32[tiles, nslices - slice0 + 1], hits uint32[tile_base[-1]]}.  Raises when the last scan had no pre-pass."""
        qt, s0, s1 = C.c_int32(), C.c_int32(), C.c_int32()
        nt, total = C.c_int64(), C.c_int64()
        u32p = C.POINTER(C.c_uint32)
        head = [C.byref(x) for x in (qt, nt, s0, s1)]
        L.check(L.lib().locrec_knn_ht_last_hits(self._h, int(nq), 0, 0, 0, *head, None, None, None, C.byref(total)))
        base = np.zeros(nt.value + 1, np.int64)
        off = np.zeros((nt.value, s1.value - s0.value + 1), np.uint32)
        hits = np.zeros(total.value, np.uint32)
        L.check(L.lib().locrec_knn_ht_last_hits(self._h, int(nq), base.size, off.size, hits.size, *head, L.ptr(base, C.c_int64),
                                                off.ctypes.data_as(u32p), hits.ctypes.data_as(u32p), C.byref(total)))
        return {"query_tile": qt.value, "tiles": nt.value, "slice0": s0.value, "nslices": s1.value, "tile_base": base,
                "off": off, "hits": hits}

    def scan_plan(self):
        """Plan of the last batched scan: kernel (1 = knn_scan, 2 = knn_scan_ht, 3 = knn_scan in head/tail mode), mode, query tile, waves."""
        v = [C.c_int32() for _ in range(4)]
        L.check(L.lib().locrec_knn_scan_plan(self._h, *[C.byref(x) for x in v]))
        return {"kernel": v[0].value, "mode": v[1].value, "query_tile": v[2].value, "waves": v[3].value}

    def scan_kernel_name(self):
        p = self.scan_plan()
        return {1: "knn_scan", 2: "knn_scan_ht", 3: "knn_scan"}.get(p["kernel"], "none") + f"<mode {p['mode']}, QT {p['query_tile']}, {p['waves']} waves>"

    def query_tile(self):
        return self.scan_plan()["query_tile"]

    def vector_lengths(self):
        lp, lc = np.empty(self.n, np.float64), np.empty(self.n, np.float64)
        L.check(L.lib().locrec_knn_vector_lengths(self._h, L.ptr(lp, C.c_double), L.ptr(lc, C.c_double)))
        return lp, lc

    def cosine_similarity(self, person_a, person_b):
        """Distance.cosineSimilarity (Distance.scala:7-9) of the two persons' place and category vectors, any sign."""
        p, c = C.c_double(), C.c_double()
        L.check(L.lib().locrec_knn_cosine_similarity(self._h, int(person_a), int(person_b), C.byref(p), C.byref(c)))
        return p.value, c.value

    def query(self, person_id, pw, cw, k):
        cap = int(max(1, min(k, max(1, self.n))))
        ids = np.empty(cap, np.int64)
        sims = np.empty(cap, np.float64)
        cnt = C.c_int64(cap)
        L.check(L.lib().locrec_knn_query(self._h, int(person_id), float(pw), float(cw), int(k),
                                         L.ptr(ids, C.c_int64), L.ptr(sims, C.c_double), C.byref(cnt)))
        m = min(cnt.value, cap)
        return ids[:m], sims[:m]

    def _out_buffers(self, capacity):
        """Reusable output arrays (grown on demand): a request must not pay for two fresh
        half-megabyte allocations - and their page faults - every time."""
        buf = getattr(self, "_rec_buf", None)
        if buf is None or len(buf[0]) < capacity:
            buf = (np.empty(capacity, np.int64), np.empty(capacity, np.float64))
            self._rec_buf = buf
        return buf

    def recommend(self, person_id, pw, cw, k, capacity=1 << 12):
        while True:
            places, est = self._out_buffers(capacity)
            cnt = C.c_int64(len(places))
            L.check(L.lib().locrec_knn_recommend(self._h, int(person_id), float(pw), float(cw), int(k),
                                                 L.ptr(places, C.c_int64), L.ptr(est, C.c_double), C.byref(cnt)))
            if cnt.value <= len(places):
                return places[:cnt.value].copy(), est[:cnt.value].copy()
            capacity = cnt.value

    def recommend_batch(self, person_ids, pw, cw, k):
        """makeRecommendations for many persons: (offsets[nq + 1], place_ids, estimated_ratings);
        rows of person i are offsets[i]:offsets[i + 1], ordered by place id."""
        q = L.as_i64(person_ids)
        off = np.zeros(len(q) + 1, np.int64)
        cap = C.c_int64(0)
        places, est = np.empty(0, np.int64), np.empty(0, np.float64)
        for _ in range(2):  # first call sizes the result, second fills it
            L.check(L.lib().locrec_knn_recommend_batch(self._h, len(q), L.ptr(q, C.c_int64), float(pw), float(cw), int(k),
                                                       L.ptr(off, C.c_int64), L.ptr(places, C.c_int64),
                                                       L.ptr(est, C.c_double), C.byref(cap)))
            if cap.value <= len(places):
                break
            places, est = np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)
            cap = C.c_int64(len(places))
        return off, places[:off[-1]], est[:off[-1]]

    def recommend_range_async(self, first, nq, pw, cw, k):
        L.check(L.lib().locrec_knn_recommend_range_async(self._h, int(first), int(nq), float(pw), float(cw), int(k)))

    def fetch_recommend(self, nq):
        off = np.zeros(nq + 1, np.int64)
        cap = C.c_int64(0)
        L.check(L.lib().locrec_knn_fetch_recommend(self._h, int(nq), L.ptr(off, C.c_int64), None, None, C.byref(cap)))
        places, est = np.empty(max(1, cap.value), np.int64), np.empty(max(1, cap.value), np.float64)
        cap = C.c_int64(len(places))
        L.check(L.lib().locrec_knn_fetch_recommend(self._h, int(nq), L.ptr(off, C.c_int64), L.ptr(places, C.c_int64),
                                                   L.ptr(est, C.c_double), C.byref(cap)))
        return off, places[:off[-1]], est[:off[-1]]

    def _ranked_args(self, nq, place_ids, place_region_ids, target_region_ids, max_recommendations):
        pl, reg, tgt = L.as_i64(place_ids), L.as_i64(place_region_ids), L.as_i64(target_region_ids)
        if len(reg) != len(pl) or len(tgt) != nq:
            raise L.IllegalArgumentException("one region per place and one target region per person are required")
        width = max(0, min(int(max_recommendations), len(pl)))   # a person has at most one row per place
        out = np.empty((nq, width), np.int64), np.empty((nq, width), np.float64), np.zeros(nq, np.int64)
        return pl, reg, tgt, width, out

    def recommend_ranked_batch(self, person_ids, pw, cw, k, place_ids, place_region_ids, target_region_ids,
                               max_recommendations, unvisited=False):
        """The batched request to its end (locrec_knn_recommend_ranked_batch): makeRecommendations for every person,
        then per person the places of its target region, top max_recommendations by estimated rating - ranked on the
        device.  -> (place_ids[nq, W], estimated_ratings[nq, W], counts[nq]), rows padded with -1 / 0.0, in the
        caller's order; W = min(max_recommendations, number of places).
        unvisited=True (locrec_knn_recommend_ranked_batch_unvisited): only new places - a person's ranking leaves out
        the places the index holds a rating of that person for."""
        q = L.as_i64(person_ids)
        pl, reg, tgt, width, (oi, osc, cnt) = self._ranked_args(len(q), place_ids, place_region_ids, target_region_ids,
                                                                max_recommendations)
        call = L.lib().locrec_knn_recommend_ranked_batch_unvisited if unvisited else L.lib().locrec_knn_recommend_ranked_batch
        L.check(call(self._h, len(q), L.ptr(q, C.c_int64), float(pw), float(cw), int(k), len(pl), L.ptr(pl, C.c_int64),
                     L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), width, L.ptr(oi, C.c_int64), L.ptr(osc, C.c_double),
                     L.ptr(cnt, C.c_int64)))
        return oi, osc, cnt

    def recommend_ranked_batch_near(self, person_ids, pw, cw, k, place_ids, place_region_ids, place_latitudes, place_longitudes,
                                    target_region_ids, center_latitudes, center_longitudes, radius_meters, max_recommendations,
                                    unvisited=False):
        """recommend_ranked_batch within reach (locrec_knn_recommend_ranked_batch_near): person i's ranking keeps only the
        places of its target region with a listing no further than radius_meters[i] (>= 0 or +inf) from
        (center_latitudes[i], center_longitudes[i]) - prep.rank_recommendations_batch_near's rule.  unvisited=True: only
        new places as well.  -> (place_ids[nq, W], estimated_ratings[nq, W], meters[nq, W], counts[nq])."""
        q = L.as_i64(person_ids)
        pl, reg, tgt, width, (oi, osc, cnt) = self._ranked_args(len(q), place_ids, place_region_ids, target_region_ids,
                                                                max_recommendations)
        plat, plon = L.as_f64(place_latitudes), L.as_f64(place_longitudes)
        clat, clon, rad = L.as_f64(center_latitudes), L.as_f64(center_longitudes), L.as_f64(radius_meters)
        if len(plat) != len(pl) or len(plon) != len(pl) or not len(clat) == len(clon) == len(rad) == len(q):
            raise L.IllegalArgumentException("one coordinate pair per place and one centre and radius per person are required")
        om = np.zeros((len(q), width), np.float64)
        L.check(L.lib().locrec_knn_recommend_ranked_batch_near(
            self._h, len(q), L.ptr(q, C.c_int64), float(pw), float(cw), int(k), len(pl), L.ptr(pl, C.c_int64),
            L.ptr(reg, C.c_int64), L.ptr(plat, C.c_double), L.ptr(plon, C.c_double), L.ptr(tgt, C.c_int64),
            L.ptr(clat, C.c_double), L.ptr(clon, C.c_double), L.ptr(rad, C.c_double), width, int(bool(unvisited)),
            L.ptr(oi, C.c_int64), L.ptr(osc, C.c_double), L.ptr(om, C.c_double), L.ptr(cnt, C.c_int64)))
        return oi, osc, om, cnt

    def recommend_ranked_batch_by_category(self, person_ids, pw, cw, k, place_ids, place_region_ids, target_region_ids,
                                           max_recommendations, place_category_ids, allowed=None, max_per_category=None,
                                           circles=None, unvisited=False):
        """recommend_ranked_batch by category (locrec_knn_recommend_ranked_batch_by_category): place_category_ids gives the
        category of every row of the place table, allowed=(offsets[nq + 1], category_ids) one allow-list per person (an
        empty list allows every category), max_per_category[i] >= 1 caps the rows of one category in person i's ranking -
        prep.rank_recommendations_batch_by_category's rules.  circles=(place_latitudes, place_longitudes,
        center_latitudes, center_longitudes, radius_meters): within reach as well; unvisited=True: only new places as
        well.  -> (place_ids[nq, W], estimated_ratings[nq, W], meters[nq, W] or None without circles, counts[nq])."""
        q = L.as_i64(person_ids)
        pl, reg, tgt, width, (oi, osc, cnt) = self._ranked_args(len(q), place_ids, place_region_ids, target_region_ids,
                                                                max_recommendations)
        pcat = L.as_i64(place_category_ids)
        if len(pcat) != len(pl):
            raise L.IllegalArgumentException("one category per place is required")
        aoff = aids = caps = om = None
        if allowed is not None:
            aoff, aids = L.as_i64(allowed[0]), L.as_i64(allowed[1])
            if len(aoff) != len(q) + 1:
                raise L.IllegalArgumentException("one allow-list per person is required: offsets of nq + 1 entries")
        if max_per_category is not None:
            caps = L.as_i64(max_per_category)
            if len(caps) != len(q):
                raise L.IllegalArgumentException("one cap per person is required")
        c = [None] * 5
        if circles is not None:
            c = [L.as_f64(x) for x in circles]
            if len(c[0]) != len(pl) or len(c[1]) != len(pl) or not len(c[2]) == len(c[3]) == len(c[4]) == len(q):
                raise L.IllegalArgumentException("one coordinate pair per place and one centre and radius per person are required")
            om = np.zeros((len(q), width), np.float64)
        L.check(L.lib().locrec_knn_recommend_ranked_batch_by_category(
            self._h, len(q), L.ptr(q, C.c_int64), float(pw), float(cw), int(k), len(pl), L.ptr(pl, C.c_int64),
            L.ptr(reg, C.c_int64), L.ptr(c[0], C.c_double), L.ptr(c[1], C.c_double), L.ptr(pcat, C.c_int64), L.ptr(tgt, C.c_int64),
            L.ptr(c[2], C.c_double), L.ptr(c[3], C.c_double), L.ptr(c[4], C.c_double), width, int(bool(unvisited)),
            L.ptr(aoff, C.c_int64), 0 if aids is None else len(aids), L.ptr(aids, C.c_int64), L.ptr(caps, C.c_int64),
            L.ptr(oi, C.c_int64), L.ptr(osc, C.c_double), L.ptr(om, C.c_double), L.ptr(cnt, C.c_int64)))
        return oi, osc, om, cnt

    def fetch_ranked(self, nq, place_ids, place_region_ids, target_region_ids, max_recommendations, unvisited=False):
        """The same last stage for the range recommend_range_async left on the device (locrec_knn_fetch_ranked, or
        locrec_knn_fetch_ranked_unvisited): target_region_ids[i] belongs to internal row first + i."""
        pl, reg, tgt, width, (oi, osc, cnt) = self._ranked_args(int(nq), place_ids, place_region_ids, target_region_ids,
                                                                max_recommendations)
        call = L.lib().locrec_knn_fetch_ranked_unvisited if unvisited else L.lib().locrec_knn_fetch_ranked
        L.check(call(self._h, int(nq), len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), width,
                     L.ptr(oi, C.c_int64), L.ptr(osc, C.c_double), L.ptr(cnt, C.c_int64)))
        return oi, osc, cnt

    # visitors: rating vectors that are no rows of the index (locrec_knn_visitors_*)
    VISITOR_STATS = ("tiles", "tiles_all", "tiles_topk", "beyond", "renumbered", "stage_launches", "scan_launches",
                     "host_syncs")

    @staticmethod
    def _visitor_args(p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val):
        """(nv, the six pointers, mem, what keeps them alive): numpy arrays -> LOCREC_MEM_HOST, CUDA tensors of the ABI's
        dtypes on the current device -> LOCREC_MEM_DEVICE, read where they lie."""
        arrays = [p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val]
        on_device = [getattr(a, "is_cuda", False) for a in arrays]
        if any(on_device):
            import torch
            if not all(on_device):
                raise L.IllegalArgumentException("requirement failed: the six vector arrays are all host arrays or all device tensors")
            dtypes = [torch.int64, torch.int32, torch.float64] * 2
            for a, dt in zip(arrays, dtypes):
                if a.dtype != dt or not a.is_contiguous():
                    raise L.IllegalArgumentException("requirement failed: contiguous device tensors of the ABI's dtypes "
                                                     "(int64 row pointers, int32 indices, float64 values) are required")
            L.require_current_device(arrays)
            torch.cuda.current_stream().synchronize()  # the library reads the arrays on its own stream
            ptrs = [C.c_void_p(a.data_ptr()) if a.numel() > 0 else None for a in arrays]
            nv = int(p_rowptr.numel()) - 1
            if int(c_rowptr.numel()) - 1 != nv:
                raise L.IllegalArgumentException("requirement failed: one place and one category vector per visitor")
            return max(nv, 0), ptrs, L.MEM_DEVICE, arrays
        keep = [L.as_i64(p_rowptr), L.as_i32(p_idx), L.as_f64(p_val), L.as_i64(c_rowptr), L.as_i32(c_idx), L.as_f64(c_val)]
        nv = len(keep[0]) - 1
        if len(keep[3]) - 1 != nv or nv < 0:
            raise L.IllegalArgumentException("requirement failed: one place and one category vector per visitor")
        if len(keep[1]) != len(keep[2]) or len(keep[4]) != len(keep[5]):
            raise L.IllegalArgumentException("requirement failed: Sparse vectors require that the dimension of the "
                                             "indices match the dimension of the values.")
        ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in keep]
        return nv, ptrs, L.MEM_HOST, keep

    @staticmethod
    def _visitor_call(fn, *args):
        """fn(*args, &bad): a refused call raises with `bad_visitor` set on the exception (-1: no single visitor)."""
        bad = C.c_int64(-1)
        try:
            L.check(fn(*args, C.byref(bad)))
        except L.IllegalArgumentException as e:
            e.bad_visitor = bad.value
            raise

    def visitors_query_batch(self, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, pw, cw, k):
        """findSimilarPersons for visitors - rating vectors (CSR, the index's original numbering) that are no rows of
        the index: (person_ids[nv, k], similarities[nv, k], counts[nv]) in query_batch's layout, each row what
        query_batch returns for the visitor on an index built with it."""
        nv, ptrs, mem, keep = self._visitor_args(p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val)
        kk = max(int(k), 0)
        ids, sims, cnt = np.empty((nv, kk), np.int64), np.empty((nv, kk), np.float64), np.empty(nv, np.int64)
        self._visitor_call(L.lib().locrec_knn_visitors_query_batch, self._h, nv, *ptrs, mem, float(pw), float(cw), int(k),
                           L.ptr(ids, C.c_int64), L.ptr(sims, C.c_double), L.ptr(cnt, C.c_int64))
        return ids, sims, cnt

    def visitors_recommend_batch(self, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, pw, cw, k):
        """makeRecommendations for visitors: (offsets[nv + 1], place_ids, estimated_ratings) in recommend_batch's layout.
        Nothing stays resident after a visitors call, so a result that does not fit the output arrays is computed AGAIN
        by a second call (stage, scan and aggregation for the whole batch): the arrays start at 65,536 rows and remember
        the largest result this object has returned, so only a handle's first large request pays twice."""
        nv, ptrs, mem, keep = self._visitor_args(p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val)
        off = np.zeros(nv + 1, np.int64)
        room = max(getattr(self, "_visitor_room", 0), 1 << 16)  # what the largest call so far returned: one pass as a rule
        cap = C.c_int64(room)
        places, est = np.empty(room, np.int64), np.empty(room, np.float64)
        for _ in range(2):  # a call whose room is too small sizes the result, the second fills it
            self._visitor_call(L.lib().locrec_knn_visitors_recommend_batch, self._h, nv, *ptrs, mem, float(pw), float(cw),
                               int(k), L.ptr(off, C.c_int64), L.ptr(places, C.c_int64), L.ptr(est, C.c_double), C.byref(cap))
            if cap.value <= len(places):
                break
            places, est = np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)
            cap = C.c_int64(len(places))
        self._visitor_room = max(room, int(off[-1]))
        return off, places[:off[-1]].copy(), est[:off[-1]].copy()

    def visitors_recommend_ranked_batch(self, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, pw, cw, k, place_ids,
                                        place_region_ids, target_region_ids, max_recommendations, exclude=None):
        """The visitors' request to its end: per visitor the places of its target region, top max_recommendations by
        estimated rating, in recommend_ranked_batch's layout.  exclude = (offsets[nv + 1], place_ids): per visitor the
        places its ranking leaves out (its rated places, for "only new places")."""
        nv, ptrs, mem, keep = self._visitor_args(p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val)
        pl, reg, tgt, width, (oi, osc, cnt) = self._ranked_args(nv, place_ids, place_region_ids, target_region_ids,
                                                                max_recommendations)
        ex_off = ex_ids = None
        if exclude is not None:
            ex_off, ex_ids = L.as_i64(exclude[0]), L.as_i64(exclude[1])
            if len(ex_off) != nv + 1:
                raise L.IllegalArgumentException("requirement failed: one exclusion list per visitor (nv + 1 offsets)")
            if nv >= 0 and len(ex_off) and ex_off[-1] > len(ex_ids):
                raise L.IllegalArgumentException("requirement failed: the exclusion offsets end beyond the listed ids")
        self._visitor_call(L.lib().locrec_knn_visitors_recommend_ranked_batch, self._h, nv, *ptrs, mem, float(pw), float(cw),
                           int(k), len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), width,
                           L.ptr(ex_off, C.c_int64), L.ptr(ex_ids, C.c_int64), L.ptr(oi, C.c_int64), L.ptr(osc, C.c_double),
                           L.ptr(cnt, C.c_int64))
        return oi, osc, cnt

    @classmethod
    def visitors_stats(cls):
        """What this thread's last visitors call did (locrec_knn_visitors_stats)."""
        v = (C.c_int64 * 8)()
        L.check(L.lib().locrec_knn_visitors_stats(v))
        return dict(zip(cls.VISITOR_STATS, (int(x) for x in v)))

    def query_shard(self, person_id, pw, cw, k, shard_index, shard_count):
        """Local top-K of candidate shard shard_index of shard_count (include/locrec.h)."""
        cap = int(max(1, min(k, max(1, self.n))))
        ids = np.empty(cap, np.int64)
        sims = np.empty(cap, np.float64)
        cnt = C.c_int64(cap)
        L.check(L.lib().locrec_knn_query_shard(self._h, int(person_id), float(pw), float(cw), int(k),
                                               int(shard_index), int(shard_count),
                                               L.ptr(ids, C.c_int64), L.ptr(sims, C.c_double), C.byref(cnt)))
        m = min(cnt.value, cap)
        return ids[:m], sims[:m]

    def recommend_neighbours(self, neighbour_ids, similarities, capacity=1 << 12):
        """makeRecommendations0 (KnnRecommender.scala:51-70) for a given list of similar persons."""
        nb, sm = L.as_i64(neighbour_ids), L.as_f64(similarities)
        if len(nb) != len(sm):
            raise L.IllegalArgumentException("neighbour columns of different lengths")
        while True:
            places, est = self._out_buffers(capacity)
            capacity = len(places)
            cnt = C.c_int64(capacity)
            L.check(L.lib().locrec_knn_recommend_neighbours(self._h, len(nb), L.ptr(nb, C.c_int64), L.ptr(sm, C.c_double),
                                                            L.ptr(places, C.c_int64), L.ptr(est, C.c_double), C.byref(cnt)))
            if cnt.value <= capacity:
                return places[:cnt.value].copy(), est[:cnt.value].copy()
            capacity = cnt.value

    def query_batch(self, person_ids, pw, cw, k):
        q = L.as_i64(person_ids)
        kk = max(int(k), 0)  # a non-positive K is rejected by the library, with the reference's message
        ids = np.empty((len(q), kk), np.int64)
        sims = np.empty((len(q), kk), np.float64)
        cnt = np.empty(len(q), np.int64)
        L.check(L.lib().locrec_knn_query_batch(self._h, len(q), L.ptr(q, C.c_int64), float(pw), float(cw), int(k),
                                               L.ptr(ids, C.c_int64), L.ptr(sims, C.c_double), L.ptr(cnt, C.c_int64)))
        return ids, sims, cnt

    def all_pairs_topk(self, pw, cw, k):
        kk = max(int(k), 0)
        ids = np.empty((self.n, kk), np.int64)
        sims = np.empty((self.n, kk), np.float64)
        cnt = np.empty(self.n, np.int64)
        L.check(L.lib().locrec_knn_all_pairs_topk(self._h, float(pw), float(cw), int(k),
                                                  L.ptr(ids, C.c_int64), L.ptr(sims, C.c_double), L.ptr(cnt, C.c_int64)))
        return ids, sims, cnt

    # device-resident form (bench.py)
    def topk_range_async(self, first, nq, pw, cw, k):
        L.check(L.lib().locrec_knn_topk_range_async(self._h, int(first), int(nq), float(pw), float(cw), int(k)))

    def row_person_ids(self, first, nq):
        out = np.empty(nq, np.int64)
        L.check(L.lib().locrec_knn_row_person_ids(self._h, int(first), int(nq), L.ptr(out, C.c_int64)))
        return out

    def fetch_topk(self, nq, k):
        ids = np.empty((nq, k), np.int64)
        sims = np.empty((nq, k), np.float64)
        cnt = np.empty(nq, np.int64)
        L.check(L.lib().locrec_knn_fetch_topk(self._h, int(nq), int(k), L.ptr(ids, C.c_int64),
                                              L.ptr(sims, C.c_double), L.ptr(cnt, C.c_int64)))
        return ids, sims, cnt

    def replayed_intervals(self):
        """Flush intervals of the batched scan that overran a survivor queue and were replayed with
        synchronous insertion inside the kernel (statistics; results are never affected)."""
        v = C.c_int64()
        L.check(L.lib().locrec_knn_replayed_intervals(self._h, C.byref(v)))
        return v.value

    def set_stream(self, hip_stream):
        L.check(L.lib().locrec_knn_set_stream(self._h, C.c_void_p(hip_stream)))

    def synchronize(self):
        L.check(L.lib().locrec_knn_synchronize(self._h))

    def profile_enable(self, on=True):
        L.check(L.lib().locrec_knn_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        ms, n = C.c_double(), C.c_int64()
        L.check(L.lib().locrec_knn_profile_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class KnnPool:
    """Resident indexes that serve one mixed batch of (index, person) requests (locrec_knn_pool_*): at the shipped
    K ("every person of positive similarity is a neighbour") every member's current tile of 16 requests shares the
    launches of a wave; any other member is served by its own batch call.  The indexes stay owned by the caller."""

    STATS = ("waves", "member_tiles", "fill_launches", "scan_launches", "aggregate_launches", "finish_launches",
             "delegated_members", "emitted_rows", "readback_bytes", "host_syncs")

    def __init__(self, indexes):
        self.indexes = list(indexes)
        arr = (C.c_void_p * len(self.indexes))(*[ix._h for ix in self.indexes])
        self._h = C.c_void_p()
        L.check(L.lib().locrec_knn_pool_create(arr, len(self.indexes), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().locrec_knn_pool_destroy(self._h)
            self._h = None

    __del__ = close

    def _locked(self):
        import contextlib
        held = contextlib.ExitStack()
        for ix in self.indexes:  # every member's lock, in member order
            if getattr(ix, "lock", None) is not None:
                held.enter_context(ix.lock)
        return held

    def recommend_batch(self, index_of, person_ids, pw, cw, k):
        """makeRecommendations of indexes[index_of[i]] for person_ids[i], every i in one call:
        (offsets[n + 1], place_ids, estimated_ratings), request i's rows exactly what
        indexes[index_of[i]].recommend_batch returns for that person.  A refused call raises with `bad_request` set on
        the exception: the position of the first request that names no index of the pool or no person of its index
        (-1 when the refusal is about no single request)."""
        gi, q = L.as_i32(index_of), L.as_i64(person_ids)
        if len(gi) != len(q):
            raise L.IllegalArgumentException("one index position per person is required")
        off = np.zeros(len(q) + 1, np.int64)
        room = max(getattr(self, "_room", 0), 1 << 16)  # what the largest call so far returned: one pass as a rule
        cap = C.c_int64(room)
        places, est = np.empty(room, np.int64), np.empty(room, np.float64)
        bad = C.c_int64(-1)
        with self._locked():
            for _ in range(2):  # a call whose room is too small sizes the result, the second fills it
                try:
                    L.check(L.lib().locrec_knn_pool_recommend_batch(
                        self._h, len(q), L.ptr(gi, C.c_int32), L.ptr(q, C.c_int64), float(pw), float(cw), int(k),
                        L.ptr(off, C.c_int64), L.ptr(places, C.c_int64), L.ptr(est, C.c_double), C.byref(cap), C.byref(bad)))
                except L.IllegalArgumentException as e:
                    e.bad_request = bad.value
                    raise
                if cap.value <= len(places):
                    break
                places, est = np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)
                cap = C.c_int64(len(places))
        self._room = max(room, int(off[-1]))
        return off, places[:off[-1]].copy(), est[:off[-1]].copy()

    def recommend_ranked_batch(self, index_of, person_ids, pw, cw, k, place_ids, place_region_ids, target_region_ids,
                               max_recommendations):
        """The pool's batch to its end (locrec_knn_pool_recommend_ranked_batch): request i gets the places of
        target_region_ids[i], top max_recommendations by estimated rating, ranked on the device.
        -> (place_ids[n, W], estimated_ratings[n, W], counts[n]) in KnnIndex.recommend_ranked_batch's layout; request i
        equals that call on its member alone.  A refused call raises with `bad_request` set, as recommend_batch does."""
        gi, q = L.as_i32(index_of), L.as_i64(person_ids)
        if len(gi) != len(q):
            raise L.IllegalArgumentException("one index position per person is required")
        pl, reg, tgt = L.as_i64(place_ids), L.as_i64(place_region_ids), L.as_i64(target_region_ids)
        if len(reg) != len(pl) or len(tgt) != len(q):
            raise L.IllegalArgumentException("one region per place and one target region per person are required")
        width = max(0, min(int(max_recommendations), len(pl)))   # a person has at most one row per place
        oi, osc, cnt = np.empty((len(q), width), np.int64), np.empty((len(q), width), np.float64), np.zeros(len(q), np.int64)
        bad = C.c_int64(-1)
        with self._locked():
            try:
                L.check(L.lib().locrec_knn_pool_recommend_ranked_batch(
                    self._h, len(q), L.ptr(gi, C.c_int32), L.ptr(q, C.c_int64), float(pw), float(cw), int(k), len(pl),
                    L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), width, L.ptr(oi, C.c_int64),
                    L.ptr(osc, C.c_double), L.ptr(cnt, C.c_int64), C.byref(bad)))
            except L.IllegalArgumentException as e:
                e.bad_request = bad.value
                raise
        return oi, osc, cnt

    # visitors over the pool: rating vectors that are no rows of any member (locrec_knn_pool_visitors_*)
    VISITOR_STATS = ("waves", "member_tiles", "stage_launches", "fill_launches", "scan_launches", "aggregate_launches",
                     "finish_launches", "delegated_members", "beyond", "emitted_rows", "readback_bytes", "host_syncs")

    @staticmethod
    def _visitor_pool_args(index_of, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val):
        """KnnIndex._visitor_args and the index positions (a host array whatever `mem` is): one per visitor."""
        nv, ptrs, mem, keep = KnnIndex._visitor_args(p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val)
        gi = L.as_i32(index_of.cpu().numpy() if hasattr(index_of, "cpu") else index_of)
        if len(gi) != nv:
            raise L.IllegalArgumentException("requirement failed: one index position per visitor is required")
        return nv, gi, ptrs, mem, keep

    def _visitor_pool_call(self, fn, *args):
        """fn(*args, &bad) under every member's lock: a refused call raises with `bad_visitor` set (-1: no single visitor)."""
        bad = C.c_int64(-1)
        try:
            L.check(fn(*args, C.byref(bad)))
        except L.IllegalArgumentException as e:
            e.bad_visitor = bad.value
            raise

    def visitors_recommend_batch(self, index_of, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, pw, cw, k):
        """makeRecommendations of indexes[index_of[i]] for visitor i - row i of ONE CSR over all visitors (numpy arrays or
        CUDA tensors, as KnnIndex.visitors_recommend_batch takes them) - every i in one call:
        (offsets[nv + 1], place_ids, estimated_ratings), visitor i's rows exactly what
        indexes[index_of[i]].visitors_recommend_batch returns for that vector.  A refused call raises with `bad_visitor`
        set: the first offending position in call order.  The output arrays remember the largest result this object has
        returned (recommend_batch's two-pass protocol)."""
        nv, gi, ptrs, mem, keep = self._visitor_pool_args(index_of, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val)
        off = np.zeros(nv + 1, np.int64)
        room = max(getattr(self, "_visitor_room", 0), 1 << 16)
        cap = C.c_int64(room)
        places, est = np.empty(room, np.int64), np.empty(room, np.float64)
        with self._locked():
            for _ in range(2):  # a call whose room is too small sizes the result, the second fills it
                self._visitor_pool_call(L.lib().locrec_knn_pool_visitors_recommend_batch, self._h, nv, L.ptr(gi, C.c_int32),
                                        *ptrs, mem, float(pw), float(cw), int(k), L.ptr(off, C.c_int64),
                                        L.ptr(places, C.c_int64), L.ptr(est, C.c_double), C.byref(cap))
                if cap.value <= len(places):
                    break
                places, est = np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)
                cap = C.c_int64(len(places))
        self._visitor_room = max(room, int(off[-1]))
        return off, places[:off[-1]].copy(), est[:off[-1]].copy()

    def visitors_recommend_ranked_batch(self, index_of, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, pw, cw, k, place_ids,
                                        place_region_ids, target_region_ids, max_recommendations, exclude=None):
        """The pool's visitors to their end (locrec_knn_pool_visitors_recommend_ranked_batch): visitor i gets the places of
        target_region_ids[i], top max_recommendations by estimated rating, in KnnIndex.visitors_recommend_ranked_batch's
        layout and equal to that call on its member alone.  exclude = (offsets[nv + 1], place_ids): per visitor the places
        its ranking leaves out."""
        nv, gi, ptrs, mem, keep = self._visitor_pool_args(index_of, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val)
        pl, reg, tgt = L.as_i64(place_ids), L.as_i64(place_region_ids), L.as_i64(target_region_ids)
        if len(reg) != len(pl) or len(tgt) != nv:
            raise L.IllegalArgumentException("one region per place and one target region per person are required")
        width = max(0, min(int(max_recommendations), len(pl)))   # a visitor has at most one row per place
        oi, osc, cnt = np.empty((nv, width), np.int64), np.empty((nv, width), np.float64), np.zeros(nv, np.int64)
        ex_off = ex_ids = None
        if exclude is not None:
            ex_off, ex_ids = L.as_i64(exclude[0]), L.as_i64(exclude[1])
            if len(ex_off) != nv + 1:
                raise L.IllegalArgumentException("requirement failed: one exclusion list per visitor (nv + 1 offsets)")
            if len(ex_off) and ex_off[-1] > len(ex_ids):
                raise L.IllegalArgumentException("requirement failed: the exclusion offsets end beyond the listed ids")
        with self._locked():
            self._visitor_pool_call(L.lib().locrec_knn_pool_visitors_recommend_ranked_batch, self._h, nv, L.ptr(gi, C.c_int32),
                                    *ptrs, mem, float(pw), float(cw), int(k), len(pl), L.ptr(pl, C.c_int64),
                                    L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), width, L.ptr(ex_off, C.c_int64),
                                    L.ptr(ex_ids, C.c_int64), L.ptr(oi, C.c_int64), L.ptr(osc, C.c_double), L.ptr(cnt, C.c_int64))
        return oi, osc, cnt

    @classmethod
    def visitors_stats(cls):
        """What this thread's last pool-visitors call did (locrec_knn_pool_visitors_stats)."""
        v = (C.c_int64 * 12)()
        L.check(L.lib().locrec_knn_pool_visitors_stats(v))
        return dict(zip(cls.VISITOR_STATS, (int(x) for x in v)))

    @classmethod
    def stats(cls):
        """What this thread's last pool call did (locrec_knn_pool_stats)."""
        x = [C.c_int64() for _ in cls.STATS]
        L.check(L.lib().locrec_knn_pool_stats(*[C.byref(i) for i in x]))
        return dict(zip(cls.STATS, (i.value for i in x)))


class KnnRecommender:
    """new KnnRecommender(placeRatingVectors, categoryRatingVectors, placeRatings,
    placeWeight, categoryWeight, kNearest).makeRecommendations(personId)"""

    def __init__(self, placeRatingVectors, categoryRatingVectors, placeRatings,
                 placeWeight, categoryWeight, kNearest):
        # require()s, KnnRecommender.scala:17-20 (same messages; checked again in the library)
        if not (placeWeight > 0 and placeWeight < 1.0):
            raise L.IllegalArgumentException(f"requirement failed: Place weight must be in the interval (0; 1): {placeWeight}")
        if not (categoryWeight > 0 and categoryWeight < 1.0):
            raise L.IllegalArgumentException(f"requirement failed: Category weight must be in the interval (0; 1): {categoryWeight}")
        if not (placeWeight + categoryWeight == 1.0):
            raise L.IllegalArgumentException(
                f"requirement failed: Sum of weights must be 1.0: place: {placeWeight}, category: {categoryWeight}")
        if not (kNearest > 0):
            raise L.IllegalArgumentException("requirement failed: K nearest must be positive")
        self.placeWeight, self.categoryWeight, self.kNearest = float(placeWeight), float(categoryWeight), int(kNearest)
        _cache.require_gpu_backend("KnnRecommender")
        # what the three frames ARE - not the weights or K, which every request passes to the library
        key = "|".join((_cache.frame_key(placeRatingVectors, ("person_id", "rating_vector")),
                        _cache.frame_key(categoryRatingVectors, ("person_id", "rating_vector")),
                        _cache.frame_key(placeRatings, ("person_id", "place_id", "rating"))))
        self._index = KnnIndex.through_cache(
            key, lambda: self._collect(placeRatingVectors, categoryRatingVectors, placeRatings))

    @staticmethod
    def _collect(placeRatingVectors, categoryRatingVectors, placeRatings):
        """The three frames collected to CSR and built into a device index (a cache miss only)."""
        pids = sorted(set(int(p) for p in placeRatingVectors["person_id"]) |
                      set(int(p) for p in categoryRatingVectors["person_id"]) |
                      set(int(p) for p in placeRatings["person_id"]))
        prp, pidx, pval, pdim = _vectors_to_csr(pids, placeRatingVectors)
        crp, cidx, cval, cdim = _vectors_to_csr(pids, categoryRatingVectors)
        pos = {p: i for i, p in enumerate(pids)}
        rows = np.fromiter((pos[int(p)] for p in placeRatings["person_id"]), dtype=np.int64,
                           count=len(placeRatings["person_id"]))
        order = np.argsort(rows, kind="stable")
        rrp = np.zeros(len(pids) + 1, np.int64)
        np.add.at(rrp, rows + 1, 1)
        rrp = np.cumsum(rrp)
        rplace = L.as_i64(np.asarray(placeRatings["place_id"])[order])
        rrating = L.as_i64(np.asarray(placeRatings["rating"])[order])
        return KnnIndex(pids, prp, pidx, pval, pdim, crp, cidx, cval, cdim, rrp, rplace, rrating)

    def close(self):
        """Drops this object's reference; the device index stays cached for the next constructor."""
        self._index.close()

    def findSimilarPersons(self, personId):
        """(person_id, similarity) of the kNearest most similar persons (KnnRecommender.scala:27-49)."""
        import pandas as pd
        with self._index.lock:
            ids, sims = self._index.query(personId, self.placeWeight, self.categoryWeight, self.kNearest)
        return pd.DataFrame({"person_id": ids, "similarity": sims})

    def makeRecommendationsBatch(self, personIds):
        """Additive: makeRecommendations for many persons in one device pass ->
        (person_id, place_id, estimated_rating)."""
        import pandas as pd
        ids = L.as_i64(personIds)
        with self._index.lock:
            off, places, est = self._index.recommend_batch(ids, self.placeWeight, self.categoryWeight, self.kNearest)
        return pd.DataFrame({"person_id": np.repeat(ids, np.diff(off)), "place_id": places, "estimated_rating": est})

    @staticmethod
    def _visitor_csr(placeVector, categoryVector):
        for v in (placeVector, categoryVector):
            if not isinstance(v, SparseVector):
                raise L.IllegalArgumentException("requirement failed: a visitor is a pair of SparseVectors")
        return (np.array([0, len(placeVector.indices)], np.int64), placeVector.indices, placeVector.values,
                np.array([0, len(categoryVector.indices)], np.int64), categoryVector.indices, categoryVector.values)

    def findSimilarPersonsForVisitor(self, placeVector, categoryVector):
        """findSimilarPersons for somebody the frames do not know: the two rating vectors instead of a person id ->
        (person_id, similarity), what findSimilarPersons returns for that person once the frames hold it."""
        import pandas as pd
        with self._index.lock:
            ids, sims, cnt = self._index.visitors_query_batch(*self._visitor_csr(placeVector, categoryVector),
                                                              self.placeWeight, self.categoryWeight,
                                                              min(self.kNearest, max(1, self._index.n)))
        return pd.DataFrame({"person_id": ids[0, :cnt[0]], "similarity": sims[0, :cnt[0]]})

    def makeRecommendationsForVisitor(self, placeVector, categoryVector):
        """makeRecommendations for somebody the frames do not know -> (place_id, estimated_rating)."""
        import pandas as pd
        with self._index.lock:
            off, places, est = self._index.visitors_recommend_batch(*self._visitor_csr(placeVector, categoryVector),
                                                                    self.placeWeight, self.categoryWeight, self.kNearest)
        return pd.DataFrame({"place_id": places, "estimated_rating": est})

    def makeRecommendations(self, personId):
        """(place_id, estimated_rating) (KnnRecommender.scala:22-25,51-70)."""
        import pandas as pd
        with self._index.lock:
            places, est = self._index.recommend(personId, self.placeWeight, self.categoryWeight, self.kNearest)
        return pd.DataFrame({"place_id": places, "estimated_rating": est})
