"""Host-side mirror of stochastic/StochasticRecommender.scala:28-34,66-71 over the C ABI."""
import ctypes as C

import numpy as np

from . import _cache
from . import _lib as L

ALPHA = 0.15  # StochasticRecommender.scala:38


def out_neighbours(source_ids, target_ids, vertex_ids):
    """The targets of each requested vertex's out-edges in the edge list (source_ids, target_ids) - for a person vertex
    the places and categories it likes, the walk's first hop: the exclusion lists of "only new places".
    -> (offsets[n + 1], ids): the list of vertex_ids[i] is ids[offsets[i]:offsets[i + 1]], ascending, without
    duplicates; empty for a vertex without out-edges or unknown to the edge list; a vertex asked twice gets its list
    twice.  numpy on the host: the edge list is cut down to the requested sources first (np.isin), so only those edges
    are sorted, never all E."""
    s, t, v = L.as_i64(source_ids), L.as_i64(target_ids), L.as_i64(vertex_ids)
    if len(s) != len(t):
        raise L.IllegalArgumentException("edge columns of different lengths")
    keep = np.isin(s, v)
    s, t = s[keep], t[keep]
    order = np.lexsort((t, s))
    s, t = s[order], t[order]
    first = np.ones(len(s), bool)
    first[1:] = (s[1:] != s[:-1]) | (t[1:] != t[:-1])   # parallel edges: one entry
    s, t = s[first], t[first]
    lo, hi = np.searchsorted(s, v, "left"), np.searchsorted(s, v, "right")
    offsets = np.zeros(len(v) + 1, np.int64)
    np.cumsum(hi - lo, out=offsets[1:])
    ids = t[np.repeat(lo - offsets[:-1], hi - lo) + np.arange(offsets[-1])]
    return offsets, np.ascontiguousarray(ids, np.int64)


class SgGraph:
    """Owner of a locrec_sg_graph handle."""

    def __init__(self, source_ids, target_ids, balanced_weights, shard_index=0, shard_count=1, by_target=False):
        """shard_count > 1: this handle keeps the edges of the source vertices ("rows of P") that
        fall into shard shard_index of the SAME global edge list; iterate it with ShardedSgRecommender."""
        self._h = C.c_void_p()
        s, t, w = L.as_i64(source_ids), L.as_i64(target_ids), L.as_f64(balanced_weights)
        if not (len(s) == len(t) == len(w)):
            raise L.IllegalArgumentException("edge columns of different lengths")
        if shard_count == 1 and shard_index == 0:
            L.check(L.lib().locrec_sg_create(len(s), L.ptr(s, C.c_int64), L.ptr(t, C.c_int64),
                                             L.ptr(w, C.c_double), C.byref(self._h)))
        else:
            create = L.lib().locrec_sg_create_target_sharded if by_target else L.lib().locrec_sg_create_sharded
            L.check(create(len(s), L.ptr(s, C.c_int64), L.ptr(t, C.c_int64), L.ptr(w, C.c_double),
                           int(shard_index), int(shard_count), C.byref(self._h)))

    @classmethod
    def from_device(cls, source_ids, target_ids, balanced_weights):
        """The same graph from an edge list that already lives in DEVICE memory (torch CUDA tensors on the current
        GPU: int64, int64, float64): the layout is built by kernels (locrec_sg_create_from_device) and equals the
        host-built one element for element, so every request answers the same bits.  The tensors are only read."""
        import torch
        cols = (source_ids, target_ids, balanced_weights)
        for t, dtype, name in zip(cols, (torch.int64, torch.int64, torch.float64),
                                  ("source_ids", "target_ids", "balanced_weights")):
            if not isinstance(t, torch.Tensor):
                raise L.IllegalArgumentException(f"requirement failed: {name} must be a torch tensor, got {type(t).__name__}")
            if t.dtype != dtype or t.dim() != 1:
                raise L.IllegalArgumentException(f"requirement failed: {name} must be a 1-d {dtype} tensor, got "
                                                 f"{t.dim()}-d {t.dtype}")
        if not (len(cols[0]) == len(cols[1]) == len(cols[2])):
            raise L.IllegalArgumentException("edge columns of different lengths")
        if not all(t.is_cuda for t in cols):
            if not torch.cuda.is_available():
                raise L.LocrecRuntimeError("no usable GPU: SgGraph.from_device has no CPU fallback")
            raise L.IllegalArgumentException("requirement failed: the edge columns must be CUDA tensors")
        L.require_current_device(cols)
        cols = [t.contiguous() for t in cols]
        torch.cuda.current_stream().synchronize()  # the library reads the arrays on its own stream
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        n = int(cols[0].numel())
        ptr = [C.c_void_p(t.data_ptr()) if n else None for t in cols]
        L.check(L.lib().locrec_sg_create_from_device(n, ptr[0], ptr[1], ptr[2], C.byref(self._h)))
        return self

    @staticmethod
    def device_build_stats():
        """HIP-event milliseconds of the phases of this thread's last from_device (locrec_sg_create_from_device_stats)."""
        ms = [C.c_double() for _ in range(4)]
        L.check(L.lib().locrec_sg_create_from_device_stats(*[C.byref(x) for x in ms]))
        return dict(zip(("ranking_ms", "plan_ms", "scatter_ms", "dictionary_ms"), (x.value for x in ms)))

    @classmethod
    def through_cache(cls, key, build):
        """The process-wide cached graph for `key` (include/locrec.h, "Handle cache"); build() -> SgGraph runs
        on a miss only.  close() / garbage collection drop a reference, the device graph stays."""
        h = _cache.acquire(L.CACHE_SG, key)
        if h is None:
            before = L.device_bytes_in_use()
            built = build()
            h = _cache.publish(L.CACHE_SG, key, built._h, L.device_bytes_in_use() - before)
            built._h = None
        self = cls.__new__(cls)
        self._h, self._cached = h, True
        self.lock = _cache.handle_lock(h)
        return self

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_cached", False):
                _cache.release(L.CACHE_SG, self._h)
            else:
                L.lib().locrec_sg_destroy(self._h)
            self._h = None

    __del__ = close

    def info(self):
        v, e, b = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib().locrec_sg_info(self._h, C.byref(v), C.byref(e), C.byref(b)))
        db = C.c_int64()
        L.check(L.lib().locrec_sg_device_bytes(self._h, C.byref(db)))
        nd = C.c_int32()
        L.check(L.lib().locrec_sg_weight_dictionary(self._h, C.byref(nd)))
        return {"vertices": v.value, "edges": e.value, "sweep_bytes": b.value, "device_sweep_bytes": db.value,
                "weight_dictionary": nd.value}

    def recommend(self, vertex_id, alpha, epsilon, max_iterations):
        self.iterate_async(vertex_id, alpha, epsilon, max_iterations)
        return self.fetch()

    def recommend_batch(self, vertex_ids, alpha, epsilon, max_iterations):
        """makeRecommendations for many vertices of this graph (locrec_sg_recommend_batch):
        (offsets[n + 1], ids, probabilities, iterations[n], converged[n]); rows of vertex i are
        offsets[i]:offsets[i + 1], each exactly what recommend() returns for that vertex."""
        v = L.as_i64(vertex_ids)
        off = np.zeros(len(v) + 1, np.int64)
        its, conv = np.zeros(len(v), np.int64), np.zeros(len(v), np.int32)
        # room for what one call can return (a target has at most its live vertices once a sweep ran, all vertices
        # before), up to a bound: the retry below sizes anything larger
        per = self.info()["vertices"] if int(max_iterations) == 0 else self.live_count()
        room = min(len(v) * max(1, per), 1 << 24)
        cap = C.c_int64(room)
        ids, probs = np.empty(room, np.int64), np.empty(room, np.float64)
        for _ in range(2):  # a call whose room is too small sizes the result, the second fills it
            L.check(L.lib().locrec_sg_recommend_batch(self._h, len(v), L.ptr(v, C.c_int64), float(alpha), float(epsilon),
                                                      int(max_iterations), L.ptr(off, C.c_int64), L.ptr(ids, C.c_int64),
                                                      L.ptr(probs, C.c_double), C.byref(cap), L.ptr(its, C.c_int64),
                                                      L.ptr(conv, C.c_int32)))
            if cap.value <= len(ids):
                break
            ids, probs = np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)
            cap = C.c_int64(len(ids))
        return off, ids[:off[-1]], probs[:off[-1]], its, conv.astype(bool)

    RANKED_BATCH_STATS = ("tiles", "groups", "emitted_rows", "readback_bytes", "host_syncs")

    def recommend_ranked_batch(self, vertex_ids, alpha, epsilon, max_iterations, place_ids, place_region_ids,
                               target_region_ids, max_recommendations, on_device=True, excluded=None):
        """The batched request to its end: per vertex the places of its target region, top max_recommendations by
        probability.  on_device=True (locrec_sg_recommend_ranked_batch): the rows are emitted into per-request
        segments and ranked on the device, x never leaves it and max_recommendations rows a request come back.
        on_device=False: recommend_batch's host rows through prep.rank_recommendations_batch (the same result; the
        A/B partner).
        excluded=(offsets[n + 1], ids): position i leaves out ids[offsets[i]:offsets[i + 1]] - the places a person has
        been to, from out_neighbours - (locrec_sg_recommend_ranked_batch_excluding; on the host path
        prep.rank_recommendations_batch_excluding).
        -> (ids[n, W], probabilities[n, W], counts[n], iterations[n], converged[n]), rows padded with -1 / 0.0;
        W = max_recommendations cut to the longest row count of a vertex."""
        if excluded is not None:
            xoff, xids = L.as_i64(excluded[0]), L.as_i64(excluded[1])
            if len(xoff) != len(vertex_ids) + 1:
                raise L.IllegalArgumentException("one exclusion list per vertex is required: offsets of n + 1 entries")
        if not on_device:
            from . import prep
            off, ids, probs, its, conv = self.recommend_batch(vertex_ids, alpha, epsilon, max_iterations)
            if excluded is not None:
                oi, op, cnt = prep.rank_recommendations_batch_excluding(off, ids, probs, place_ids, place_region_ids,
                                                                        target_region_ids, max_recommendations, xoff, xids)
            else:
                oi, op, cnt = prep.rank_recommendations_batch(off, ids, probs, place_ids, place_region_ids, target_region_ids,
                                                              max_recommendations)
            return oi, op, cnt, its, conv
        v, pl, reg, tgt = L.as_i64(vertex_ids), L.as_i64(place_ids), L.as_i64(place_region_ids), L.as_i64(target_region_ids)
        n = len(v)
        if len(reg) != len(pl) or len(tgt) != n:
            raise L.IllegalArgumentException("one region per place and one target region per vertex are required")
        # no vertex has more rows than the graph has vertices: the stride of the call, cut to W afterwards
        stride = max(0, min(int(max_recommendations), self.info()["vertices"]))
        oi, op = np.full((n, stride), -1, np.int64), np.zeros((n, stride), np.float64)
        cnt, rows, its, conv = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32))
        head = (self._h, n, L.ptr(v, C.c_int64), float(alpha), float(epsilon), int(max_iterations), len(pl), L.ptr(pl, C.c_int64),
                L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), stride)
        outs = (L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64),
                L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32))
        if excluded is not None:
            L.check(L.lib().locrec_sg_recommend_ranked_batch_excluding(*head, L.ptr(xoff, C.c_int64), len(xids),
                                                                       L.ptr(xids, C.c_int64), *outs))
        else:
            L.check(L.lib().locrec_sg_recommend_ranked_batch(*head, *outs))
        width = max(0, min(stride, int(rows.max()) if n else 0))
        return (np.ascontiguousarray(oi[:, :width]), np.ascontiguousarray(op[:, :width]), cnt, its, conv.astype(bool))

    def recommend_ranked_batch_near(self, vertex_ids, alpha, epsilon, max_iterations, place_ids, place_region_ids,
                                    place_latitudes, place_longitudes, target_region_ids, center_latitudes, center_longitudes,
                                    radius_meters, max_recommendations, excluded=None, on_device=True):
        """recommend_ranked_batch within reach (locrec_sg_recommend_ranked_batch_near): position i keeps only the places
        of its target region with a listing no further than radius_meters[i] (>= 0 or +inf) from (center_latitudes[i],
        center_longitudes[i]) - prep.rank_recommendations_batch_near's rule - and, with excluded=(offsets, ids), none of
        its list.  on_device=False: recommend_batch's host rows through prep.rank_recommendations_batch_near (the same
        result; the A/B partner).
        -> (ids[n, W], probabilities[n, W], meters[n, W], counts[n], iterations[n], converged[n])."""
        xoff = xids = None
        if excluded is not None:
            xoff, xids = L.as_i64(excluded[0]), L.as_i64(excluded[1])
            if len(xoff) != len(vertex_ids) + 1:
                raise L.IllegalArgumentException("one exclusion list per vertex is required: offsets of n + 1 entries")
        if not on_device:
            from . import prep
            off, ids, probs, its, conv = self.recommend_batch(vertex_ids, alpha, epsilon, max_iterations)
            oi, op, om, cnt = prep.rank_recommendations_batch_near(off, ids, probs, place_ids, place_region_ids, place_latitudes,
                                                                   place_longitudes, target_region_ids, center_latitudes,
                                                                   center_longitudes, radius_meters, max_recommendations, xoff, xids)
            return oi, op, om, cnt, its, conv
        v, pl, reg, tgt = L.as_i64(vertex_ids), L.as_i64(place_ids), L.as_i64(place_region_ids), L.as_i64(target_region_ids)
        plat, plon = L.as_f64(place_latitudes), L.as_f64(place_longitudes)
        clat, clon, rad = L.as_f64(center_latitudes), L.as_f64(center_longitudes), L.as_f64(radius_meters)
        n = len(v)
        if len(reg) != len(pl) or len(tgt) != n:
            raise L.IllegalArgumentException("one region per place and one target region per vertex are required")
        if len(plat) != len(pl) or len(plon) != len(pl) or not len(clat) == len(clon) == len(rad) == n:
            raise L.IllegalArgumentException("one coordinate pair per place and one centre and radius per vertex are required")
        stride = max(0, min(int(max_recommendations), self.info()["vertices"]))
        oi, op, om = np.full((n, stride), -1, np.int64), np.zeros((n, stride), np.float64), np.zeros((n, stride), np.float64)
        cnt, rows, its, conv = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32))
        L.check(L.lib().locrec_sg_recommend_ranked_batch_near(
            self._h, n, L.ptr(v, C.c_int64), float(alpha), float(epsilon), int(max_iterations), len(pl), L.ptr(pl, C.c_int64),
            L.ptr(reg, C.c_int64), L.ptr(plat, C.c_double), L.ptr(plon, C.c_double), L.ptr(tgt, C.c_int64),
            L.ptr(clat, C.c_double), L.ptr(clon, C.c_double), L.ptr(rad, C.c_double), stride,
            L.ptr(xoff, C.c_int64), 0 if xids is None else len(xids), L.ptr(xids, C.c_int64),
            L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(om, C.c_double), L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64),
            L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32)))
        width = max(0, min(stride, int(rows.max()) if n else 0))
        return (np.ascontiguousarray(oi[:, :width]), np.ascontiguousarray(op[:, :width]), np.ascontiguousarray(om[:, :width]),
                cnt, its, conv.astype(bool))

    def recommend_ranked_batch_by_category(self, vertex_ids, alpha, epsilon, max_iterations, place_ids, place_region_ids,
                                           target_region_ids, max_recommendations, place_category_ids, allowed=None,
                                           max_per_category=None, circles=None, excluded=None, on_device=True):
        """recommend_ranked_batch by category (locrec_sg_recommend_ranked_batch_by_category): place_category_ids gives the
        category of every row of the place table, allowed=(offsets[n + 1], category_ids) one allow-list per position (an
        empty list allows every category), max_per_category[i] >= 1 caps the rows of one category in position i's ranking
        - prep.rank_recommendations_batch_by_category's rules.  circles=(place_latitudes, place_longitudes,
        center_latitudes, center_longitudes, radius_meters) and excluded=(offsets, ids) as in recommend_ranked_batch_near.
        on_device=False: recommend_batch's host rows through prep.rank_recommendations_batch_by_category (the same result;
        the A/B partner).
        -> (ids[n, W], probabilities[n, W], meters[n, W] or None without circles, counts[n], iterations[n], converged[n])."""
        n = len(vertex_ids)
        xoff = xids = aoff = aids = caps = None
        if excluded is not None:
            xoff, xids = L.as_i64(excluded[0]), L.as_i64(excluded[1])
            if len(xoff) != n + 1:
                raise L.IllegalArgumentException("one exclusion list per vertex is required: offsets of n + 1 entries")
        if allowed is not None:
            aoff, aids = L.as_i64(allowed[0]), L.as_i64(allowed[1])
            if len(aoff) != n + 1:
                raise L.IllegalArgumentException("one allow-list per vertex is required: offsets of n + 1 entries")
        if max_per_category is not None:
            caps = L.as_i64(max_per_category)
            if len(caps) != n:
                raise L.IllegalArgumentException("one cap per vertex is required")
        if not on_device:
            from . import prep
            off, ids, probs, its, conv = self.recommend_batch(vertex_ids, alpha, epsilon, max_iterations)
            oi, op, om, cnt = prep.rank_recommendations_batch_by_category(
                off, ids, probs, place_ids, place_region_ids, target_region_ids, max_recommendations, place_category_ids,
                allowed=None if aoff is None else (aoff, aids), max_per_category=caps, circles=circles,
                excluded=None if xoff is None else (xoff, xids))
            return oi, op, om, cnt, its, conv
        v, pl, reg, tgt = L.as_i64(vertex_ids), L.as_i64(place_ids), L.as_i64(place_region_ids), L.as_i64(target_region_ids)
        pcat = L.as_i64(place_category_ids)
        if len(reg) != len(pl) or len(tgt) != n or len(pcat) != len(pl):
            raise L.IllegalArgumentException("one region and one category per place and one target region per vertex are required")
        c = [None] * 5
        stride = max(0, min(int(max_recommendations), self.info()["vertices"]))
        oi, op, om = np.full((n, stride), -1, np.int64), np.zeros((n, stride), np.float64), None
        if circles is not None:
            c = [L.as_f64(x) for x in circles]
            if len(c[0]) != len(pl) or len(c[1]) != len(pl) or not len(c[2]) == len(c[3]) == len(c[4]) == n:
                raise L.IllegalArgumentException("one coordinate pair per place and one centre and radius per vertex are required")
            om = np.zeros((n, stride), np.float64)
        cnt, rows, its, conv = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32))
        L.check(L.lib().locrec_sg_recommend_ranked_batch_by_category(
            self._h, n, L.ptr(v, C.c_int64), float(alpha), float(epsilon), int(max_iterations), len(pl), L.ptr(pl, C.c_int64),
            L.ptr(reg, C.c_int64), L.ptr(c[0], C.c_double), L.ptr(c[1], C.c_double), L.ptr(pcat, C.c_int64), L.ptr(tgt, C.c_int64),
            L.ptr(c[2], C.c_double), L.ptr(c[3], C.c_double), L.ptr(c[4], C.c_double), stride,
            L.ptr(xoff, C.c_int64), 0 if xids is None else len(xids), L.ptr(xids, C.c_int64),
            L.ptr(aoff, C.c_int64), 0 if aids is None else len(aids), L.ptr(aids, C.c_int64), L.ptr(caps, C.c_int64),
            L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(om, C.c_double), L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64),
            L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32)))
        width = max(0, min(stride, int(rows.max()) if n else 0))
        return (np.ascontiguousarray(oi[:, :width]), np.ascontiguousarray(op[:, :width]),
                None if om is None else np.ascontiguousarray(om[:, :width]), cnt, its, conv.astype(bool))

    @classmethod
    def ranked_batch_stats(cls):
        """What this thread's last on-device recommend_ranked_batch did (locrec_sg_recommend_ranked_batch_stats)."""
        x = [C.c_int64() for _ in cls.RANKED_BATCH_STATS]
        L.check(L.lib().locrec_sg_recommend_ranked_batch_stats(*[C.byref(i) for i in x]))
        return dict(zip(cls.RANKED_BATCH_STATS, (i.value for i in x)))

    # ---- visitors: persons this graph has no vertex for (include/locrec.h, "SG for visitors") ----
    VISITORS_STATS = ("tiles", "visitors", "staged_edges", "table_slots", "set_up_launches", "finalize_launches", "polls",
                      "waits")

    @staticmethod
    def _visitor_edges(edge_offsets, target_ids, weights):
        off, t, w = L.as_i64(edge_offsets), L.as_i64(target_ids), L.as_f64(weights)
        if len(off) < 1 or len(t) != len(w) or (len(off) > 1 and off[-1] > len(t)):
            raise L.IllegalArgumentException("visitor edges: offsets of nv + 1 entries into target ids and weights of one length")
        return off, t, w

    def visitors_recommend_batch(self, edge_offsets, target_ids, weights, alpha, epsilon, max_iterations):
        """makeRecommendations for visitors (locrec_sg_visitors_recommend_batch): visitor v is the out-edges
        (target_ids[e], weights[e]), e in edge_offsets[v]:edge_offsets[v + 1] - prep.visitor_edges builds them - and gets
        what recommend(V) returns on this graph's edge list followed by those edges under a new id V.
        -> (offsets[nv + 1], ids, probabilities, iterations[nv], converged[nv]).  A refused call raises with `bad_visitor`
        set on the exception: the first offending visitor, or -1."""
        off, t, w = self._visitor_edges(edge_offsets, target_ids, weights)
        nv = len(off) - 1
        out_off = np.zeros(nv + 1, np.int64)
        its, conv = np.zeros(nv, np.int64), np.zeros(nv, np.int32)
        per = self.info()["vertices"] if int(max_iterations) == 0 else self.live_count()
        room = min(nv * max(1, per), 1 << 24)
        cap = C.c_int64(room)
        ids, probs = np.empty(room, np.int64), np.empty(room, np.float64)
        bad = C.c_int64(-1)
        for _ in range(2):  # a call whose room is too small sizes the result, the second fills it
            try:
                L.check(L.lib().locrec_sg_visitors_recommend_batch(
                    self._h, nv, L.ptr(off, C.c_int64), L.ptr(t, C.c_int64), L.ptr(w, C.c_double), float(alpha), float(epsilon),
                    int(max_iterations), L.ptr(out_off, C.c_int64), L.ptr(ids, C.c_int64), L.ptr(probs, C.c_double),
                    C.byref(cap), L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32), C.byref(bad)))
            except L.IllegalArgumentException as e:
                e.bad_visitor = bad.value
                raise
            if cap.value <= len(ids):
                break
            ids, probs = np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)
            cap = C.c_int64(len(ids))
        return out_off, ids[:out_off[-1]], probs[:out_off[-1]], its, conv.astype(bool)

    def visitors_recommend_ranked_batch(self, edge_offsets, target_ids, weights, alpha, epsilon, max_iterations, place_ids,
                                        place_region_ids, target_region_ids, max_recommendations, exclude=None):
        """The visitors call to its end (locrec_sg_visitors_recommend_ranked_batch): per visitor the places of its target
        region, top max_recommendations by probability, emitted and ranked on the device.
        exclude=(offsets[nv + 1], ids): visitor i leaves out ids[offsets[i]:offsets[i + 1]].
        -> (ids[nv, W], probabilities[nv, W], counts[nv], iterations[nv], converged[nv]) as recommend_ranked_batch returns
        them.  A refused call raises with `bad_visitor` set, as visitors_recommend_batch does."""
        off, t, w = self._visitor_edges(edge_offsets, target_ids, weights)
        nv = len(off) - 1
        pl, reg, tgt = L.as_i64(place_ids), L.as_i64(place_region_ids), L.as_i64(target_region_ids)
        if len(reg) != len(pl) or len(tgt) != nv:
            raise L.IllegalArgumentException("one region per place and one target region per visitor are required")
        xoff = xids = None
        if exclude is not None:
            xoff, xids = L.as_i64(exclude[0]), L.as_i64(exclude[1])
            if len(xoff) != nv + 1:
                raise L.IllegalArgumentException("one exclusion list per visitor is required: offsets of nv + 1 entries")
        stride = max(0, min(int(max_recommendations), self.info()["vertices"]))
        oi, op = np.full((nv, stride), -1, np.int64), np.zeros((nv, stride), np.float64)
        cnt, rows, its, conv = (np.zeros(nv, np.int64), np.zeros(nv, np.int64), np.zeros(nv, np.int64), np.zeros(nv, np.int32))
        bad = C.c_int64(-1)
        try:
            L.check(L.lib().locrec_sg_visitors_recommend_ranked_batch(
                self._h, nv, L.ptr(off, C.c_int64), L.ptr(t, C.c_int64), L.ptr(w, C.c_double), float(alpha), float(epsilon),
                int(max_iterations), len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), stride,
                L.ptr(xoff, C.c_int64), 0 if xids is None else len(xids), L.ptr(xids, C.c_int64), L.ptr(oi, C.c_int64),
                L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64), L.ptr(its, C.c_int64),
                L.ptr(conv, C.c_int32), C.byref(bad)))
        except L.IllegalArgumentException as e:
            e.bad_visitor = bad.value
            raise
        width = max(0, min(stride, int(rows.max()) if nv else 0))
        return (np.ascontiguousarray(oi[:, :width]), np.ascontiguousarray(op[:, :width]), cnt, its, conv.astype(bool))

    @classmethod
    def visitors_stats(cls):
        """What this thread's last visitors call did (locrec_sg_visitors_stats)."""
        x = (C.c_int64 * 8)()
        L.check(L.lib().locrec_sg_visitors_stats(x))
        return dict(zip(cls.VISITORS_STATS, (int(i) for i in x)))

    def vertex_kinds(self, vertex_ids):
        """Per id: 0 = no vertex of this graph, 1 = a source-only vertex, 2 = a live vertex (locrec_sg_vertex_kinds)."""
        v = L.as_i64(vertex_ids)
        out = np.zeros(len(v), np.int32)
        L.check(L.lib().locrec_sg_vertex_kinds(self._h, len(v), L.ptr(v, C.c_int64), L.ptr(out, C.c_int32)))
        return out

    def iterate_async(self, vertex_id, alpha, epsilon, max_iterations):
        L.check(L.lib().locrec_sg_iterate_async(self._h, int(vertex_id), float(alpha), float(epsilon),
                                                int(max_iterations)))

    def sweeps_async(self, vertex_id, alpha, sweeps):
        L.check(L.lib().locrec_sg_sweeps_async(self._h, int(vertex_id), float(alpha), int(sweeps)))

    def fetch(self):
        cap = max(1, self.info()["vertices"])
        ids = np.empty(cap, np.int64)
        probs = np.empty(cap, np.float64)
        cnt, it, conv = C.c_int64(cap), C.c_int64(), C.c_int32()
        L.check(L.lib().locrec_sg_fetch(self._h, L.ptr(ids, C.c_int64), L.ptr(probs, C.c_double), C.byref(cnt),
                                        C.byref(it), C.byref(conv)))
        return ids[:cnt.value], probs[:cnt.value], it.value, bool(conv.value)

    # ---- row-sharded iteration (include/locrec.h, "Row-sharded form") ----
    def live_count(self):
        n = C.c_int64()
        L.check(L.lib().locrec_sg_live_count(self._h, C.byref(n)))
        return n.value

    def shard_begin(self, vertex_id):
        L.check(L.lib().locrec_sg_shard_begin(self._h, int(vertex_id)))

    def shard_sigma(self, sigma_device_ptr):
        L.check(L.lib().locrec_sg_shard_sigma(self._h, C.c_void_p(sigma_device_ptr)))

    def shard_apply(self, sigma_device_ptr, alpha):
        L.check(L.lib().locrec_sg_shard_apply(self._h, C.c_void_p(sigma_device_ptr), float(alpha)))

    def shard_d2(self):
        d2 = C.c_double()
        L.check(L.lib().locrec_sg_shard_d2(self._h, C.byref(d2)))
        return d2.value

    def shard_finish(self, iterations, converged):
        L.check(L.lib().locrec_sg_shard_finish(self._h, int(iterations), 1 if converged else 0))

    def set_stream(self, hip_stream):
        L.check(L.lib().locrec_sg_set_stream(self._h, C.c_void_p(hip_stream)))

    def synchronize(self):
        L.check(L.lib().locrec_sg_synchronize(self._h))

    def profile_enable(self, on=True):
        L.check(L.lib().locrec_sg_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        ms, n = C.c_double(), C.c_int64()
        L.check(L.lib().locrec_sg_profile_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class SgGroup:
    """Independent graphs iterated together (locrec_sg_group_*): one sweep and one combine launch per
    round for all of them.  The graphs stay owned by the caller and are read with SgGraph.fetch()."""

    def __init__(self, graphs):
        self.graphs = list(graphs)
        arr = (C.c_void_p * len(self.graphs))(*[g._h for g in self.graphs])
        self._h = C.c_void_p()
        L.check(L.lib().locrec_sg_group_create(arr, len(self.graphs), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.lib().locrec_sg_group_destroy(self._h)
            self._h = None

    __del__ = close

    def sweeps_async(self, vertex_ids, alpha, sweeps):
        v = L.as_i64(vertex_ids)
        assert len(v) == len(self.graphs)
        L.check(L.lib().locrec_sg_group_sweeps_async(self._h, L.ptr(v, C.c_int64), float(alpha), int(sweeps)))

    def iterate_async(self, vertex_ids, alpha, epsilon, max_iterations):
        """makeRecommendations' iteration for every graph (each stops at its own isConverged)."""
        v = L.as_i64(vertex_ids)
        assert len(v) == len(self.graphs)
        L.check(L.lib().locrec_sg_group_iterate_async(self._h, L.ptr(v, C.c_int64), float(alpha), float(epsilon),
                                                      int(max_iterations)))

    def synchronize(self):
        L.check(L.lib().locrec_sg_group_synchronize(self._h))


class SgPool:
    """Resident graphs that serve one mixed batch of (graph, vertex) requests (locrec_sg_pool_*): every graph's
    current tile of up to 16 targets shares the launches of a round.  The graphs stay owned by the caller."""

    STATS = ("tile_waves", "rounds", "sweep_launches", "finalize_launches", "polls", "readback_bytes")

    def __init__(self, graphs):
        self.graphs = list(graphs)
        arr = (C.c_void_p * len(self.graphs))(*[g._h for g in self.graphs])
        self._h = C.c_void_p()
        L.check(L.lib().locrec_sg_pool_create(arr, len(self.graphs), C.byref(self._h)))
        self._sizes = None
        self.row_counts = None  # of the last recommend_ranked_batch

    def close(self):
        if getattr(self, "_h", None):
            L.lib().locrec_sg_pool_destroy(self._h)
            self._h = None

    __del__ = close

    def recommend_batch(self, graph_index, vertex_ids, alpha, epsilon, max_iterations):
        """makeRecommendations of graphs[graph_index[i]] for vertex_ids[i], every i in one call:
        (offsets[n + 1], ids, probabilities, iterations[n], converged[n]), request i's rows exactly what
        graphs[graph_index[i]].recommend() returns for that vertex.  A failed call raises with `bad_request` set on the
        exception: the position of the first request that names no graph of the pool or no vertex of its graph."""
        import contextlib
        gi, v = L.as_i32(graph_index), L.as_i64(vertex_ids)
        if len(gi) != len(v):
            raise L.IllegalArgumentException("one graph index per vertex is required")
        n = len(v)
        off = np.zeros(n + 1, np.int64)
        its, conv = np.zeros(n, np.int64), np.zeros(n, np.int32)
        with contextlib.ExitStack() as held:
            for g in self.graphs:  # every member's lock, in member order
                if getattr(g, "lock", None) is not None:
                    held.enter_context(g.lock)
            # room for what one call can return, as SgGraph.recommend_batch sizes it, up to a bound: the retry below
            # sizes anything larger
            known = (gi >= 0) & (gi < len(self.graphs))
            counts = np.bincount(gi[known], minlength=len(self.graphs))
            if self._sizes is None:  # (a handle's vertex and live counts never change)
                self._sizes = (np.array([g.info()["vertices"] for g in self.graphs], np.int64),
                               np.array([g.live_count() for g in self.graphs], np.int64))
            per = self._sizes[0 if int(max_iterations) == 0 else 1]
            room = min(max(int(np.dot(counts, np.maximum(per, 1))), 1), 1 << 24)
            cap = C.c_int64(room)
            ids, probs = np.empty(room, np.int64), np.empty(room, np.float64)
            bad = C.c_int64(-1)
            for _ in range(2):  # a call whose room is too small sizes the result, the second fills it
                try:
                    L.check(L.lib().locrec_sg_pool_recommend_batch(
                        self._h, n, L.ptr(gi, C.c_int32), L.ptr(v, C.c_int64), float(alpha), float(epsilon), int(max_iterations),
                        L.ptr(off, C.c_int64), L.ptr(ids, C.c_int64), L.ptr(probs, C.c_double), C.byref(cap),
                        L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32), C.byref(bad)))
                except L.IllegalArgumentException as e:
                    e.bad_request = bad.value
                    raise
                if cap.value <= len(ids):
                    break
                ids, probs = np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)
                cap = C.c_int64(len(ids))
        return off, ids[:off[-1]], probs[:off[-1]], its, conv.astype(bool)

    @classmethod
    def stats(cls):
        """What this thread's last recommend_batch did (locrec_sg_pool_stats)."""
        x = [C.c_int64() for _ in cls.STATS]
        L.check(L.lib().locrec_sg_pool_stats(*[C.byref(i) for i in x]))
        return dict(zip(cls.STATS, (i.value for i in x)))

    RANKED_STATS = ("tile_waves", "tiles", "rounds", "groups", "emit_launches", "emitted_rows", "readback_bytes", "host_syncs")

    def recommend_ranked_batch(self, graph_index, vertex_ids, alpha, epsilon, max_iterations, place_ids, place_region_ids,
                               target_region_ids, max_recommendations):
        """The pool's batch to its end (locrec_sg_pool_recommend_ranked_batch): request i gets the places of
        target_region_ids[i] that graphs[graph_index[i]] reaches from vertex_ids[i], top max_recommendations by
        probability; every member's tile is emitted and ranked on the device, no x leaves it.
        -> (ids[n, W], probabilities[n, W], counts[n], iterations[n], converged[n] bool), rows padded with -1 / 0.0 and
        W = max_recommendations cut to the longest row count of a request, as SgGraph.recommend_ranked_batch returns
        them; request i equals that call on its member alone.  self.row_counts holds makeRecommendations' own row count
        per request of the last call.  A failed call raises with `bad_request` set, as recommend_batch does."""
        import contextlib
        gi, v = L.as_i32(graph_index), L.as_i64(vertex_ids)
        pl, reg, tgt = L.as_i64(place_ids), L.as_i64(place_region_ids), L.as_i64(target_region_ids)
        n = len(v)
        if len(gi) != n:
            raise L.IllegalArgumentException("one graph index per vertex is required")
        if len(reg) != len(pl) or len(tgt) != n:
            raise L.IllegalArgumentException("one region per place and one target region per vertex are required")
        with contextlib.ExitStack() as held:
            for g in self.graphs:  # every member's lock, in member order
                if getattr(g, "lock", None) is not None:
                    held.enter_context(g.lock)
            if self._sizes is None:  # (a handle's vertex and live counts never change)
                self._sizes = (np.array([g.info()["vertices"] for g in self.graphs], np.int64),
                               np.array([g.live_count() for g in self.graphs], np.int64))
            # no request has more rows than its graph has vertices: the stride of the call, cut to W afterwards
            stride = max(0, min(int(max_recommendations), int(self._sizes[0].max())))
            oi, op = np.full((n, stride), -1, np.int64), np.zeros((n, stride), np.float64)
            cnt, rows, its, conv = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32))
            bad = C.c_int64(-1)
            try:
                L.check(L.lib().locrec_sg_pool_recommend_ranked_batch(
                    self._h, n, L.ptr(gi, C.c_int32), L.ptr(v, C.c_int64), float(alpha), float(epsilon), int(max_iterations),
                    len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64), L.ptr(tgt, C.c_int64), stride, L.ptr(oi, C.c_int64),
                    L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64), L.ptr(its, C.c_int64),
                    L.ptr(conv, C.c_int32), C.byref(bad)))
            except L.IllegalArgumentException as e:
                e.bad_request = bad.value
                raise
        self.row_counts = rows
        width = max(0, min(stride, int(rows.max()) if n else 0))
        return (np.ascontiguousarray(oi[:, :width]), np.ascontiguousarray(op[:, :width]), cnt, its, conv.astype(bool))

    @classmethod
    def ranked_stats(cls):
        """What this thread's last recommend_ranked_batch did (locrec_sg_pool_recommend_ranked_batch_stats)."""
        x = [C.c_int64() for _ in cls.RANKED_STATS]
        L.check(L.lib().locrec_sg_pool_recommend_ranked_batch_stats(*[C.byref(i) for i in x]))
        return dict(zip(cls.RANKED_STATS, (i.value for i in x)))

    # ---- visitors across the pool (include/locrec.h, "Visitors across a pool") ----
    VISITORS_STATS = ("tile_waves", "member_tiles", "visitors", "staged_edges", "stagings", "begin_launches", "set_up_launches",
                      "rounds", "sweep_launches", "finalize_launches", "polls", "consumes")

    def _sizes_of_members(self):
        if self._sizes is None:  # (a handle's vertex and live counts never change)
            self._sizes = (np.array([g.info()["vertices"] for g in self.graphs], np.int64),
                           np.array([g.live_count() for g in self.graphs], np.int64))
        return self._sizes

    def _visitors(self, graph_index, edge_offsets, target_ids, weights):
        gi = L.as_i32(graph_index)
        off, t, w = SgGraph._visitor_edges(edge_offsets, target_ids, weights)
        if len(gi) != len(off) - 1:
            raise L.IllegalArgumentException("one graph index per visitor is required")
        return gi, off, t, w

    def _member_locks(self, held):
        for g in self.graphs:  # every member's lock, in member order
            if getattr(g, "lock", None) is not None:
                held.enter_context(g.lock)

    def visitors_recommend_batch(self, graph_index, edge_offsets, target_ids, weights, alpha, epsilon, max_iterations):
        """makeRecommendations for visitors of many graphs in one call (locrec_sg_pool_visitors_recommend_batch): visitor v,
        given as in SgGraph.visitors_recommend_batch, is asked of graphs[graph_index[v]] and gets exactly what that member's
        own visitors_recommend_batch returns for it.
        -> (offsets[nv + 1], ids, probabilities, iterations[nv], converged[nv]).  A refused call raises with `bad_visitor`
        set on the exception: the position of the first offending visitor, or -1."""
        import contextlib
        gi, off, t, w = self._visitors(graph_index, edge_offsets, target_ids, weights)
        nv = len(gi)
        out_off = np.zeros(nv + 1, np.int64)
        its, conv = np.zeros(nv, np.int64), np.zeros(nv, np.int32)
        with contextlib.ExitStack() as held:
            self._member_locks(held)
            known = (gi >= 0) & (gi < len(self.graphs))
            counts = np.bincount(gi[known], minlength=len(self.graphs))
            per = self._sizes_of_members()[0 if int(max_iterations) == 0 else 1]
            room = min(max(int(np.dot(counts, np.maximum(per, 1))), 1), 1 << 24)
            cap = C.c_int64(room)
            ids, probs = np.empty(room, np.int64), np.empty(room, np.float64)
            bad = C.c_int64(-1)
            for _ in range(2):  # a call whose room is too small sizes the result, the second fills it
                try:
                    L.check(L.lib().locrec_sg_pool_visitors_recommend_batch(
                        self._h, nv, L.ptr(gi, C.c_int32), L.ptr(off, C.c_int64), L.ptr(t, C.c_int64), L.ptr(w, C.c_double),
                        float(alpha), float(epsilon), int(max_iterations), L.ptr(out_off, C.c_int64), L.ptr(ids, C.c_int64),
                        L.ptr(probs, C.c_double), C.byref(cap), L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32), C.byref(bad)))
                except L.IllegalArgumentException as e:
                    e.bad_visitor = bad.value
                    raise
                if cap.value <= len(ids):
                    break
                ids, probs = np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)
                cap = C.c_int64(len(ids))
        return out_off, ids[:out_off[-1]], probs[:out_off[-1]], its, conv.astype(bool)

    def visitors_recommend_ranked_batch(self, graph_index, edge_offsets, target_ids, weights, alpha, epsilon, max_iterations,
                                        place_ids, place_region_ids, target_region_ids, max_recommendations, exclude=None):
        """The pool's visitors call to its end (locrec_sg_pool_visitors_recommend_ranked_batch): per visitor the places of
        its target region that its member reaches, top max_recommendations by probability, emitted and ranked on the device.
        exclude=(offsets[nv + 1], ids): visitor i leaves out ids[offsets[i]:offsets[i + 1]].
        -> (ids[nv, W], probabilities[nv, W], counts[nv], iterations[nv], converged[nv]) as SgGraph's
        visitors_recommend_ranked_batch returns them; visitor i equals that call on its member alone.  self.row_counts holds
        makeRecommendations' own row count per visitor.  A refused call raises with `bad_visitor` set."""
        import contextlib
        gi, off, t, w = self._visitors(graph_index, edge_offsets, target_ids, weights)
        nv = len(gi)
        pl, reg, tgt = L.as_i64(place_ids), L.as_i64(place_region_ids), L.as_i64(target_region_ids)
        if len(reg) != len(pl) or len(tgt) != nv:
            raise L.IllegalArgumentException("one region per place and one target region per visitor are required")
        xoff = xids = None
        if exclude is not None:
            xoff, xids = L.as_i64(exclude[0]), L.as_i64(exclude[1])
            if len(xoff) != nv + 1:
                raise L.IllegalArgumentException("one exclusion list per visitor is required: offsets of nv + 1 entries")
        with contextlib.ExitStack() as held:
            self._member_locks(held)
            # no visitor has more rows than its graph has vertices: the stride of the call, cut to W afterwards
            stride = max(0, min(int(max_recommendations), int(self._sizes_of_members()[0].max())))
            oi, op = np.full((nv, stride), -1, np.int64), np.zeros((nv, stride), np.float64)
            cnt, rows, its, conv = (np.zeros(nv, np.int64), np.zeros(nv, np.int64), np.zeros(nv, np.int64), np.zeros(nv, np.int32))
            bad = C.c_int64(-1)
            try:
                L.check(L.lib().locrec_sg_pool_visitors_recommend_ranked_batch(
                    self._h, nv, L.ptr(gi, C.c_int32), L.ptr(off, C.c_int64), L.ptr(t, C.c_int64), L.ptr(w, C.c_double),
                    float(alpha), float(epsilon), int(max_iterations), len(pl), L.ptr(pl, C.c_int64), L.ptr(reg, C.c_int64),
                    L.ptr(tgt, C.c_int64), stride, L.ptr(xoff, C.c_int64), 0 if xids is None else len(xids),
                    L.ptr(xids, C.c_int64), L.ptr(oi, C.c_int64), L.ptr(op, C.c_double), L.ptr(cnt, C.c_int64),
                    L.ptr(rows, C.c_int64), L.ptr(its, C.c_int64), L.ptr(conv, C.c_int32), C.byref(bad)))
            except L.IllegalArgumentException as e:
                e.bad_visitor = bad.value
                raise
        self.row_counts = rows
        width = max(0, min(stride, int(rows.max()) if nv else 0))
        return (np.ascontiguousarray(oi[:, :width]), np.ascontiguousarray(op[:, :width]), cnt, its, conv.astype(bool))

    @classmethod
    def visitors_stats(cls):
        """What this thread's last visitors call on a pool did (locrec_sg_pool_visitors_stats)."""
        x = (C.c_int64 * 12)()
        L.check(L.lib().locrec_sg_pool_visitors_stats(x))
        return dict(zip(cls.VISITORS_STATS, (int(i) for i in x)))


class StochasticRecommender:
    """new StochasticRecommender(stochasticEdges, epsilon, maxIterations).makeRecommendations(vertexId)

    stochasticEdges: frame with columns source_id, target_id, balanced_weight
    (StochasticGraphBuilder.scala:12-16); ids may be ints of any width."""

    def __init__(self, stochasticEdges, epsilon, maxIterations, quiet=False):
        if not (epsilon >= 0):
            raise L.IllegalArgumentException("requirement failed: epsilon must be non-negative")
        if not (maxIterations >= 0):
            raise L.IllegalArgumentException("requirement failed: max iterations number must be non-negative")
        self.epsilon, self.maxIterations, self.quiet = float(epsilon), int(maxIterations), quiet
        _cache.require_gpu_backend("StochasticRecommender")
        # the edge list alone identifies the graph; epsilon and maxIterations are per-request arguments
        key = _cache.frame_key(stochasticEdges, ("source_id", "target_id", "balanced_weight"))
        self._graph = SgGraph.through_cache(key, lambda: SgGraph(
            np.asarray(stochasticEdges["source_id"]), np.asarray(stochasticEdges["target_id"]),
            np.asarray(stochasticEdges["balanced_weight"])))

    def close(self):
        """Drops this object's reference; the device graph stays cached for the next constructor."""
        self._graph.close()

    def makeRecommendations(self, vertexId):
        import pandas as pd
        with self._graph.lock:
            ids, probs, iterations, converged = self._graph.recommend(vertexId, ALPHA, self.epsilon, self.maxIterations)
        if not self.quiet:  # the two println()s of step(), StochasticRecommender.scala:94,100
            if converged:
                print(f"Converged in {iterations} iterations")
            else:
                print(f"Number of iterations {iterations} reached the maximum {self.maxIterations}")
        return pd.DataFrame({"id": ids, "probability": probs})

    def makeRecommendationsForVisitor(self, edges):
        """Additive: makeRecommendations for a person the graph has no vertex for.  edges: frame with columns target_id,
        balanced_weight - the person's out-edges (prep.visitor_edges).  -> (id, probability): what makeRecommendations
        returns for a new vertex on stochasticEdges followed by those edges."""
        import pandas as pd
        t, w = np.asarray(edges["target_id"]), np.asarray(edges["balanced_weight"])
        with self._graph.lock:
            off, ids, probs, iterations, converged = self._graph.visitors_recommend_batch(
                [0, len(t)], t, w, ALPHA, self.epsilon, self.maxIterations)
        if not self.quiet:  # the two println()s of step(), StochasticRecommender.scala:94,100
            if converged[0]:
                print(f"Converged in {iterations[0]} iterations")
            else:
                print(f"Number of iterations {iterations[0]} reached the maximum {self.maxIterations}")
        return pd.DataFrame({"id": ids, "probability": probs})

    def makeRecommendationsBatch(self, vertexIds):
        """Additive: makeRecommendations for many vertices of this graph in shared sweeps ->
        (vertex_id, id, probability); the rows of each vertex are exactly makeRecommendations' rows."""
        import pandas as pd
        v = L.as_i64(vertexIds)
        with self._graph.lock:
            off, ids, probs, iterations, converged = self._graph.recommend_batch(v, ALPHA, self.epsilon, self.maxIterations)
        if not self.quiet:  # step()'s line (:94,100) for every vertex, in input order
            for it, conv in zip(iterations, converged):
                if conv:
                    print(f"Converged in {it} iterations")
                else:
                    print(f"Number of iterations {it} reached the maximum {self.maxIterations}")
        return pd.DataFrame({"vertex_id": np.repeat(v, np.diff(off)), "id": ids, "probability": probs})

    def makeRecommendationsRankedBatch(self, vertexIds, places, targetRegionIds, maxRecommendations):
        """Additive: makeRecommendationsBatch and printRecommendations' query (StochasticRecommenderMain.scala:64-75)
        in one call on the device.  places: frame with columns id, region_id; targetRegionIds: one per vertex.
        -> (vertex_id, id, probability): per vertex, in input order, the places of its target region, at most
        maxRecommendations of them, by probability descending (ties: id ascending)."""
        import pandas as pd
        v = L.as_i64(vertexIds)
        with self._graph.lock:
            oi, op, cnt, iterations, converged = self._graph.recommend_ranked_batch(
                v, ALPHA, self.epsilon, self.maxIterations, np.asarray(places["id"]), np.asarray(places["region_id"]),
                targetRegionIds, maxRecommendations)
        if not self.quiet:  # step()'s line (:94,100) for every vertex, in input order
            for it, conv in zip(iterations, converged):
                if conv:
                    print(f"Converged in {it} iterations")
                else:
                    print(f"Number of iterations {it} reached the maximum {self.maxIterations}")
        keep = np.arange(oi.shape[1])[None, :] < cnt[:, None]
        return pd.DataFrame({"vertex_id": np.repeat(v, cnt), "id": oi[keep], "probability": op[keep]})
