// knn_batch.hip -- the KNN translation unit: knn.hip whole, then the six batch entry points - findSimilarPersons /
// makeRecommendations for many persons - at any K, e.g. the shipped --k-nearest 2000000 (bin/knn_recommender.sh:35)
// below N - 1; then the ranked forms, the pools and the visitors' calls.
//
// Each entry point is defined once, here: it checks its arguments and then dispatches on K.  Up to
// LOCREC_KNN_BATCH_MAX_K (the per-query LDS lists) a call takes knn.hip's body of its name with _lds (behind the checks);
// any larger K takes the tiled top-K of knn_large.hip (knn_anyk.h) - in the recommend calls K >= N - 1 ("every positive
// neighbour") takes knn.hip's body too, which needs no top-K at all.
//
// The tiled path keeps its device buffers in the handle:
//   lkb_S                     a tile's similarities, transposed, and the masked row-major tile of the aggregation
//   lk_keys / lk_vals (+ _out) the tile's segments, ping-pong of the merge passes
//   tile_hist / tile_sel      one histogram and one selection record per column (shared with enqueue_topk)
//   out_*                     the neighbour lists, as every batch leaves them for locrec_knn_fetch_topk
//   lkb_*                     the place-major aggregation and its resident result (locrec_knn_fetch_recommend)
// They are grow-only and freed with the handle.

#include "knn.hip"

namespace {

// queries per chunk of the synchronous forms: the device result arrays (ids, similarities, rows: 20 bytes an entry)
// stay within 2 GiB at any K
int64_t any_k_chunk(int64_t k)
{
    const int64_t c = std::max<int64_t>(1, ((int64_t)2 << 30) / (k * 20));
    return c >= 16 ? c / 16 * 16 : c;
}

// the tiled top-K of rows[0 .. nq) into the device result arrays, left as enqueue_topk leaves a batch for
// locrec_knn_fetch_topk
int32_t enqueue_any_k(locrec_knn_index *ix, const int32_t *rows, int64_t nq, double pw, double cw, int64_t k, bool mark_absent)
{
    ix->have_result = false;
    ix->single_pending = false;
    ix->single_direct = false;
    ix->last_scan_fast = false;
    ix->have_agg = false;
    ix->have_lkb = false;
    LOCREC_TRY(knn_topk_tiled(ix, rows, nq, pw, cw, k, mark_absent));
    ix->last_nq = nq;
    ix->last_k = k;
    ix->have_result = true;
    return LOCREC_OK;
}

// a synchronous form: rows[i] -> output row i (the tiled path keeps no order of its own), chunk by chunk straight into
// the caller's arrays
int32_t any_k_rows(locrec_knn_index *ix, const std::vector<int32_t> &rows, double pw, double cw, int64_t k, bool mark_absent,
                   int64_t *out_ids, double *out_sims, int64_t *out_counts)
{
    hipStream_t s = ix->stream;
    const int64_t nq = (int64_t)rows.size(), chunk = any_k_chunk(k);
    for (int64_t i0 = 0; i0 < nq; i0 += chunk) {
        const int64_t cn = std::min(chunk, nq - i0);
        LOCREC_TRY(enqueue_any_k(ix, rows.data() + i0, cn, pw, cw, k, mark_absent));
        if (out_ids) LOCREC_HIP_TRY(hipMemcpyAsync(out_ids + i0 * k, ix->out_ids.p, (size_t)(cn * k) * 8, hipMemcpyDeviceToHost, s));
        if (out_sims) LOCREC_HIP_TRY(hipMemcpyAsync(out_sims + i0 * k, ix->out_sims.p, (size_t)(cn * k) * 8, hipMemcpyDeviceToHost, s));
        if (out_counts) LOCREC_HIP_TRY(hipMemcpyAsync(out_counts + i0, ix->out_cnt.p, (size_t)cn * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
    }
    return LOCREC_OK;
}

// the recommend calls take the tiled top-K for LOCREC_KNN_BATCH_MAX_K < K < N - 1
bool any_k_recommend(const locrec_knn_index *ix, int64_t k) { return k > LOCREC_KNN_BATCH_MAX_K && k < ix->n - 1; }

}  // namespace

extern "C" int32_t locrec_knn_query_batch(locrec_knn_index *ix, int64_t nq, const int64_t *person_ids, double pw, double cw,
                                          int64_t k, int64_t *out_ids, double *out_sims, int64_t *out_counts) try
{
    if (!ix) return fail(LOCREC_E_INVALID_ARG, "index is NULL");
    ix->have_result = false;
    LOCREC_TRY(check_params(pw, cw, k));
    if (nq < 0 || (nq > 0 && !person_ids)) return fail(LOCREC_E_INVALID_ARG, "bad query list");
    if (nq == 0) return LOCREC_OK;
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    std::vector<int32_t> rows((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) LOCREC_TRY(find_query_row(ix, person_ids[i], &rows[(size_t)i]));
    if (k <= LOCREC_KNN_BATCH_MAX_K) return query_batch_lds(ix, rows, pw, cw, k, out_ids, out_sims, out_counts);
    return any_k_rows(ix, rows, pw, cw, k, false, out_ids, out_sims, out_counts);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_topk_range_async(locrec_knn_index *ix, int64_t first, int64_t nq, double pw, double cw,
                                               int64_t k) try
{
    if (!ix) return fail(LOCREC_E_INVALID_ARG, "index is NULL");
    ix->have_result = false;
    LOCREC_TRY(check_params(pw, cw, k));
    if (first < 0 || nq <= 0 || first + nq > ix->n) return fail(LOCREC_E_INVALID_ARG, "row range out of bounds");
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    if (k <= LOCREC_KNN_BATCH_MAX_K) return topk_range_lds(ix, first, nq, pw, cw, k);
    // (the whole range stays resident until locrec_knn_fetch_topk: nq x k entries)
    std::vector<int32_t> rows((size_t)nq);
    std::iota(rows.begin(), rows.end(), (int32_t)first);
    return enqueue_any_k(ix, rows.data(), nq, pw, cw, k, true);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_all_pairs_topk(locrec_knn_index *ix, double pw, double cw, int64_t k, int64_t *out_ids,
                                             double *out_sims, int64_t *out_counts) try
{
    if (!ix) return fail(LOCREC_E_INVALID_ARG, "index is NULL");
    LOCREC_TRY(check_params(pw, cw, k));
    if (k <= LOCREC_KNN_BATCH_MAX_K) return all_pairs_topk_lds(ix, pw, cw, k, out_ids, out_sims, out_counts);
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    // every person as the query, in the order of person_ids[] given at create
    std::vector<int32_t> rows(ix->row_of_input.begin(), ix->row_of_input.end());
    return any_k_rows(ix, rows, pw, cw, k, true, out_ids, out_sims, out_counts);
} LOCREC_CATCH_ALL

// findSimilarPersons (:27-49) restricted to one shard of the candidates: the local top-K of a request whose candidate
// scan is split over several GPUs (every GPU holds the whole index).
extern "C" int32_t locrec_knn_query_shard(locrec_knn_index *ix, int64_t person_id, double pw, double cw, int64_t k,
                                          int32_t shard_index, int32_t shard_count, int64_t *out_ids, double *out_sims,
                                          int64_t *inout_count) try
{
    if (!ix) return fail(LOCREC_E_INVALID_ARG, "index is NULL");
    if (!inout_count) return fail(LOCREC_E_INVALID_ARG, "inout_count is NULL");
    LOCREC_TRY(check_params(pw, cw, k));
    if (shard_count < 1 || shard_index < 0 || shard_index >= shard_count)
        return fail(LOCREC_E_INVALID_ARG, "shard %d of %d", shard_index, shard_count);
    int32_t row = 0;
    LOCREC_TRY(find_query_row(ix, person_id, &row));
    const int64_t keff = std::min<int64_t>(k, std::max<int64_t>(1, ix->n - 1));
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    int32_t s0 = 0, s1 = 0;
    shard_slice_range(ix, shard_index, shard_count, &s0, &s1);
    if (s0 >= s1) {  // more shards than slices: this one is empty
        *inout_count = 0;
        return LOCREC_OK;
    }
    CandRangeGuard guard(ix, s0, s1);  // also covers the reruns inside locrec_knn_fetch_topk
    if (keff <= LOCREC_KNN_BATCH_MAX_K) return query_one_lds(ix, row, pw, cw, keff, out_ids, out_sims, inout_count);
    // the single request's full sort over this shard's candidates (lk_gather_keys honours the slice range)
    return knn_large_topk(ix, row, pw, cw, keff, out_ids, out_sims, inout_count);
} LOCREC_CATCH_ALL

// Batched makeRecommendations (the additive surface of SURVEY.md 8b) for the persons at internal rows [first, first + nq);
// everything stays on the device until locrec_knn_fetch_recommend.
extern "C" int32_t locrec_knn_recommend_range_async(locrec_knn_index *ix, int64_t first, int64_t nq, double pw, double cw,
                                                    int64_t k) try
{
    if (!ix) return fail(LOCREC_E_INVALID_ARG, "index is NULL");
    ix->have_agg = false;
    ix->have_lkb = false;
    if (k <= LOCREC_KNN_BATCH_MAX_K) ix->have_result = false;  // (a larger K forgets the lists once its checks have passed)
    LOCREC_TRY(check_params(pw, cw, k));
    if (first < 0 || nq <= 0 || first + nq > ix->n) return fail(LOCREC_E_INVALID_ARG, "row range out of bounds");
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    if (k <= LOCREC_KNN_BATCH_MAX_K) return recommend_range_lds(ix, first, nq, pw, cw, k);
    std::vector<int32_t> rows((size_t)nq);
    std::iota(rows.begin(), rows.end(), (int32_t)first);
    return enqueue_large_k_batch(ix, rows, pw, cw, k);  // (K >= N - 1 or the tiled top-K: any_k_recommend)
} LOCREC_CATCH_ALL

// makeRecommendations for a list of persons; rows of person i are [out_offsets[i], out_offsets[i + 1]) of out_places /
// out_ratings, ordered by place id.
extern "C" int32_t locrec_knn_recommend_batch(locrec_knn_index *ix, int64_t nq, const int64_t *person_ids, double pw,
                                              double cw, int64_t k, int64_t *out_offsets, int64_t *out_places,
                                              double *out_ratings, int64_t *inout_capacity) try
{
    if (!ix) return fail(LOCREC_E_INVALID_ARG, "index is NULL");
    ix->have_result = false;
    ix->have_agg = false;
    ix->have_lkb = false;
    LOCREC_TRY(check_params(pw, cw, k));
    if (nq < 0 || (nq > 0 && !person_ids) || !out_offsets || !inout_capacity) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    if (nq == 0) {
        out_offsets[0] = 0;
        *inout_capacity = 0;
        return LOCREC_OK;
    }
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    std::vector<int32_t> rows((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) LOCREC_TRY(find_query_row(ix, person_ids[i], &rows[(size_t)i]));
    if (!any_k_recommend(ix, k))
        return recommend_batch_lds(ix, rows, pw, cw, k, out_offsets, out_places, out_ratings, inout_capacity);
    // in input order (the tiled path keeps no order of its own): the resident rows go straight to the caller's arrays, or
    // only the offsets and the total when they do not fit
    LOCREC_TRY(enqueue_large_k_batch(ix, rows, pw, cw, k));
    return locrec_knn_fetch_recommend(ix, nq, out_offsets, out_places, out_ratings, inout_capacity);
} LOCREC_CATCH_ALL

// the ranked forms of the two recommend calls above (and locrec_knn_fetch_ranked for the range form)
#include "knn_ranked.h"

// =====================================================================================================
// A pool of resident indexes that serves ONE mixed batch of (index, person[, target region]) requests
// (locrec_knn_pool_*).  A member in the "every positive neighbour" regime (K > LOCREC_KNN_BATCH_MAX_K and
// K >= n - 1: the shipped --k-nearest 2000000) takes the shared launches of knn_pool.h; every other member's sub-batch
// is handed to its own public call.  The pool keeps all its state here.
#include "knn_pool_api.h"
#include "knn_pool_visitors_api.h"

struct locrec_knn_pool {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<locrec_knn_index *> members;  // not owned
    locrec::KnnPoolShared *shared = nullptr;
    locrec::KnnPoolVisitors *visitors = nullptr;  // the visitors' stage (locrec_knn_pool_visitors_*), made at the first such call
    DevBuf<int64_t> rk_in, rk_out;  // the ranked form's inputs (places table, targets, segments) and outputs
    ~locrec_knn_pool()
    {
        locrec::knn_pool_visitors_destroy(visitors);
        locrec::knn_pool_shared_destroy(shared);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// One pool call: its requests sorted out (knn_pool_plan.h), the sharing members' batches and their rows in the pool's buffers
struct KnnPoolCall : locrec::KnnPoolRequests {
    std::vector<locrec::KnnPoolBatch> batches;
    std::vector<int64_t> base, len;  // per distinct request: its rows in d_place / d_est
    const int64_t *d_place = nullptr;
    const double *d_est = nullptr;
};

bool knn_pool_shares(const locrec_knn_index *ix, int64_t k) { return k > LOCREC_KNN_BATCH_MAX_K && k >= ix->n - 1; }

// The beginning of both pool entries, before any device work: the arguments they share (outputs_ok: the entry's own),
// the stats, then the checks in this order - every index position, check_params' requires, every person - and the plan.
int32_t knn_pool_begin(locrec_knn_pool *pool, int64_t n, const int32_t *index_of, const int64_t *persons, double pw, double cw,
                       int64_t k, bool outputs_ok, int64_t *out_bad, KnnPoolCall &call)
{
    if (!pool) return fail(LOCREC_E_INVALID_ARG, "pool is NULL");
    if (out_bad) *out_bad = -1;
    locrec::knn_pool_stats() = locrec::KnnPoolStats();
    if (n < 0 || (n > 0 && (!index_of || !persons)) || !outputs_ok) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    const int32_t nm = (int32_t)pool->members.size();
    for (int64_t i = 0; i < n; ++i)
        if (index_of[i] < 0 || index_of[i] >= nm) {
            if (out_bad) *out_bad = i;
            return fail(LOCREC_E_INVALID_ARG, "request %lld names index %d of a pool of %d", (long long)i, index_of[i], nm);
        }
    LOCREC_TRY(check_params(pw, cw, k));
    std::vector<int32_t> row((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t st = find_query_row(pool->members[(size_t)index_of[i]], persons[i], &row[(size_t)i]);
        if (st != LOCREC_OK) {
            if (out_bad) *out_bad = i;
            return st;
        }
    }
    std::vector<char> shares((size_t)nm);
    for (int32_t m = 0; m < nm; ++m) shares[(size_t)m] = knn_pool_shares(pool->members[(size_t)m], k);
    locrec::knn_pool_requests(n, index_of, row.data(), shares, call);
    for (const auto &c : call.cuts) call.batches.push_back({pool->members[(size_t)c.member], call.rows.data() + c.first, c.n, c.first});
    return LOCREC_OK;
}

// the shared members' part of a call: rows resident in the pool's buffers
int32_t knn_pool_run_shared(locrec_knn_pool *pool, KnnPoolCall &call, double pw, double cw)
{
    LOCREC_HIP_TRY(hipSetDevice(pool->device));
    call.base.assign(call.rows.size(), 0);
    call.len.assign(call.rows.size(), 0);
    if (call.batches.empty()) return LOCREC_OK;
    return locrec::knn_pool_shared_run(pool->shared, pool->stream, call.batches, pw, cw, call.base.data(), call.len.data(),
                                       &call.d_place, &call.d_est);
}

// nothing stays resident in a member for locrec_knn_fetch_*
void knn_pool_forget(locrec_knn_index *ix)
{
    ix->have_result = false;
    ix->have_agg = false;
    ix->have_lkb = false;
}

// the other members: f(d, member, its requests in input order, their persons) = its own public call and the scatter
template <class F>
int32_t knn_pool_each_delegated(locrec_knn_pool *pool, const KnnPoolCall &call, const int64_t *person_ids, F f)
{
    locrec::knn_pool_stats().delegated_members = (int64_t)call.delegated.size();
    for (size_t d = 0; d < call.delegated.size(); ++d) {
        locrec_knn_index *ix = pool->members[(size_t)call.delegated[d]];
        std::vector<int64_t> ids;
        for (int64_t i : call.requests_of[d]) ids.push_back(person_ids[i]);
        const int32_t rc = f(d, ix, call.requests_of[d], ids);
        knn_pool_forget(ix);
        if (rc != LOCREC_OK) return rc;
    }
    return LOCREC_OK;
}

}  // namespace

extern "C" int32_t locrec_knn_pool_create(locrec_knn_index *const *indexes, int32_t n_indexes, locrec_knn_pool **out_pool) try
{
    if (!out_pool) return fail(LOCREC_E_INVALID_ARG, "out_pool is NULL");
    *out_pool = nullptr;
    if (!indexes || n_indexes < 1 || n_indexes > 65535) return fail(LOCREC_E_INVALID_ARG, "a pool holds 1 .. 65535 indexes");
    std::vector<std::pair<const locrec_knn_index *, int32_t>> seen;
    for (int32_t i = 0; i < n_indexes; ++i) {
        if (!indexes[i]) return fail(LOCREC_E_INVALID_ARG, "index %d is NULL", i);
        if (indexes[i]->device != indexes[0]->device)
            return fail(LOCREC_E_INVALID_ARG, "index %d is on device %d, index 0 on device %d: a pool lives on one device", i,
                        indexes[i]->device, indexes[0]->device);
        seen.push_back({indexes[i], i});
    }
    std::sort(seen.begin(), seen.end());
    for (size_t i = 1; i < seen.size(); ++i)
        if (seen[i].first == seen[i - 1].first)
            return fail(LOCREC_E_INVALID_ARG, "index %d is listed twice (also as index %d)", seen[i].second, seen[i - 1].second);
    std::unique_ptr<locrec_knn_pool> pool(new locrec_knn_pool());
    pool->device = indexes[0]->device;
    pool->members.assign(indexes, indexes + n_indexes);
    LOCREC_HIP_TRY(hipSetDevice(pool->device));
    LOCREC_HIP_TRY(hipStreamCreateWithFlags(&pool->stream, hipStreamNonBlocking));
    pool->shared = locrec::knn_pool_shared_create();
    *out_pool = pool.release();
    return LOCREC_OK;
} LOCREC_CATCH_ALL

extern "C" void locrec_knn_pool_destroy(locrec_knn_pool *pool)
{
    if (!pool) return;
    (void)hipSetDevice(pool->device);
    delete pool;
}

extern "C" int32_t locrec_knn_pool_recommend_batch(locrec_knn_pool *pool, int64_t n_requests, const int32_t *index_of_request,
                                                   const int64_t *person_ids, double pw, double cw, int64_t k,
                                                   int64_t *out_offsets, int64_t *out_places, double *out_ratings,
                                                   int64_t *inout_capacity, int64_t *out_bad_request) try
{
    const int64_t n = n_requests;
    KnnPoolCall call;
    LOCREC_TRY(knn_pool_begin(pool, n, index_of_request, person_ids, pw, cw, k, out_offsets && inout_capacity, out_bad_request, call));
    if (n == 0) {
        out_offsets[0] = 0;
        *inout_capacity = 0;
        return LOCREC_OK;
    }
    LOCREC_TRY(knn_pool_run_shared(pool, call, pw, cw));
    locrec::KnnPoolStats &st = locrec::knn_pool_stats();
    hipStream_t s = pool->stream;
    const std::vector<int64_t> &base = call.base, &len = call.len;
    std::vector<int64_t> rlen((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i)
        if (call.distinct_of[(size_t)i] >= 0) rlen[(size_t)i] = len[(size_t)call.distinct_of[(size_t)i]];
    // the other members: their own call on their own persons, sizes first
    std::vector<std::vector<int64_t>> d_off(call.delegated.size());
    const auto sizes = [&](size_t d, locrec_knn_index *ix, const auto &rq, const auto &ids) -> int32_t {
        d_off[d].assign(rq.size() + 1, 0);
        int64_t cap = 0;
        LOCREC_TRY(locrec_knn_recommend_batch(ix, (int64_t)rq.size(), ids.data(), pw, cw, k, d_off[d].data(), nullptr, nullptr, &cap));
        for (size_t j = 0; j < rq.size(); ++j) rlen[(size_t)rq[j]] = d_off[d][j + 1] - d_off[d][j];
        return LOCREC_OK;
    };
    LOCREC_TRY(knn_pool_each_delegated(pool, call, person_ids, sizes));
    const int64_t total = std::accumulate(rlen.begin(), rlen.end(), (int64_t)0);
    const bool sizes_only = total > *inout_capacity || total == 0;  // (nothing but the offsets and the total)
    if (!sizes_only && (!out_places || !out_ratings)) return fail(LOCREC_E_INVALID_ARG, "NULL output buffer");
    out_offsets[0] = 0;
    for (int64_t i = 0; i < n; ++i) out_offsets[i + 1] = out_offsets[i] + rlen[(size_t)i];
    *inout_capacity = total;
    if (sizes_only) return LOCREC_OK;
    // the shared rows: one copy of the pool's row buffer, handed out in input order
    int64_t resident = 0;
    for (size_t u = 0; u < len.size(); ++u) resident = std::max(resident, base[u] + len[u]);
    std::vector<int64_t> hp((size_t)resident);
    std::vector<double> he((size_t)resident);
    if (resident > 0) {
        LOCREC_HIP_TRY(hipMemcpyAsync(hp.data(), call.d_place, (size_t)resident * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(he.data(), call.d_est, (size_t)resident * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        st.readback_bytes += resident * 16;
        ++st.host_syncs;
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t u = call.distinct_of[(size_t)i];
        if (u < 0 || len[(size_t)u] == 0) continue;
        std::copy(hp.begin() + base[(size_t)u], hp.begin() + base[(size_t)u] + len[(size_t)u], out_places + out_offsets[i]);
        std::copy(he.begin() + base[(size_t)u], he.begin() + base[(size_t)u] + len[(size_t)u], out_ratings + out_offsets[i]);
    }
    const auto rows = [&](size_t d, locrec_knn_index *ix, const auto &rq, const auto &ids) -> int32_t {
        int64_t mcap = d_off[d].back();
        if (mcap == 0) return LOCREC_OK;
        std::vector<int64_t> mp((size_t)mcap);
        std::vector<double> me((size_t)mcap);
        LOCREC_TRY(locrec_knn_recommend_batch(ix, (int64_t)rq.size(), ids.data(), pw, cw, k, d_off[d].data(), mp.data(), me.data(), &mcap));
        for (size_t j = 0; j < rq.size(); ++j) {
            std::copy(mp.begin() + d_off[d][j], mp.begin() + d_off[d][j + 1], out_places + out_offsets[rq[j]]);
            std::copy(me.begin() + d_off[d][j], me.begin() + d_off[d][j + 1], out_ratings + out_offsets[rq[j]]);
        }
        return LOCREC_OK;
    };
    return knn_pool_each_delegated(pool, call, person_ids, rows);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_pool_recommend_ranked_batch(locrec_knn_pool *pool, int64_t n_requests, const int32_t *index_of_request,
                                                          const int64_t *person_ids, double pw, double cw, int64_t k,
                                                          int64_t n_places, const int64_t *place_ids,
                                                          const int64_t *place_region_ids, const int64_t *target_region_ids,
                                                          int64_t max_recommendations, int64_t *out_place_ids,
                                                          double *out_estimated_ratings, int64_t *out_counts,
                                                          int64_t *out_bad_request) try
{
    const int64_t n = n_requests, N = std::max<int64_t>(0, max_recommendations);
    KnnPoolCall call;
    LOCREC_TRY(knn_pool_begin(pool, n, index_of_request, person_ids, pw, cw, k, true, out_bad_request, call));
    if (n == 0) return LOCREC_OK;
    LOCREC_TRY(knn_rank_check_args(n_places, place_ids, place_region_ids, target_region_ids, N, out_place_ids, out_estimated_ratings,
                                   out_counts));
    LOCREC_TRY(knn_pool_run_shared(pool, call, pw, cw));
    locrec::KnnPoolStats &st = locrec::knn_pool_stats();
    hipStream_t s = pool->stream;
    // one segment per request of a shared member: duplicates share a row range and keep their own targets
    std::vector<int64_t> seg_req, hin;
    for (int64_t i = 0; i < n; ++i)
        if (call.distinct_of[(size_t)i] >= 0) seg_req.push_back(i);
    const int64_t nseg = (int64_t)seg_req.size();
    if (nseg > 0) {
        // ONE upload of the places table, the targets and the segments; one ranker call over the pool's row buffer
        hin.resize(RankIo::in_words(n_places, nseg));
        if (n_places > 0) {
            std::copy(place_ids, place_ids + n_places, hin.begin());
            std::copy(place_region_ids, place_region_ids + n_places, hin.begin() + n_places);
        }
        for (int64_t c = 0; c < nseg; ++c) {
            const int64_t u = call.distinct_of[(size_t)seg_req[(size_t)c]];
            hin[(size_t)(2 * n_places + c)] = target_region_ids[seg_req[(size_t)c]];
            hin[(size_t)(2 * n_places + nseg + c)] = call.base[(size_t)u];
            hin[(size_t)(2 * n_places + 2 * nseg + c)] = call.len[(size_t)u];
        }
        LOCREC_TRY(pool->rk_in.reserve(hin.size()));
        LOCREC_TRY(pool->rk_out.reserve(RankIo::out_words(nseg, N)));
        const RankIo io(pool->rk_in.p, pool->rk_out.p, n_places, nseg, N);
        LOCREC_HIP_TRY(hipMemcpyAsync(pool->rk_in.p, hin.data(), hin.size() * 8, hipMemcpyHostToDevice, s));
        const int32_t rc = io.rank(call.d_place, call.d_est, 0, s);
        if (rc != LOCREC_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        LOCREC_TRY(io.read_back_to(seg_req, out_place_ids, out_estimated_ratings, out_counts, s));
        st.readback_bytes += nseg * N * 16 + nseg * 8;
        st.host_syncs += rank_batch_stats().host_syncs + 1;
    }
    // the other members: their own ranked call on their own requests
    const auto ranked = [&](size_t, locrec_knn_index *ix, const auto &rq, const auto &ids) -> int32_t {
        const int64_t nq = (int64_t)rq.size();
        std::vector<int64_t> tgt((size_t)nq), oid((size_t)(nq * N)), ocnt((size_t)nq);
        std::vector<double> osc((size_t)(nq * N));
        for (int64_t j = 0; j < nq; ++j) tgt[(size_t)j] = target_region_ids[rq[(size_t)j]];
        LOCREC_TRY(locrec_knn_recommend_ranked_batch(ix, nq, ids.data(), pw, cw, k, n_places, place_ids, place_region_ids, tgt.data(),
                                                     max_recommendations, oid.data(), osc.data(), ocnt.data()));
        for (int64_t j = 0; j < nq; ++j) {
            std::copy(oid.begin() + j * N, oid.begin() + (j + 1) * N, out_place_ids + rq[(size_t)j] * N);
            std::copy(osc.begin() + j * N, osc.begin() + (j + 1) * N, out_estimated_ratings + rq[(size_t)j] * N);
            out_counts[rq[(size_t)j]] = ocnt[(size_t)j];
        }
        return LOCREC_OK;
    };
    return knn_pool_each_delegated(pool, call, person_ids, ranked);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_pool_stats(int64_t *out_waves, int64_t *out_member_tiles, int64_t *out_fill_launches,
                                         int64_t *out_scan_launches, int64_t *out_aggregate_launches, int64_t *out_finish_launches,
                                         int64_t *out_delegated_members, int64_t *out_emitted_rows, int64_t *out_readback_bytes,
                                         int64_t *out_host_syncs)
{
    const locrec::KnnPoolStats &st = locrec::knn_pool_stats();
    if (out_waves) *out_waves = st.waves;
    if (out_member_tiles) *out_member_tiles = st.member_tiles;
    if (out_fill_launches) *out_fill_launches = st.fill_launches;
    if (out_scan_launches) *out_scan_launches = st.scan_launches;
    if (out_aggregate_launches) *out_aggregate_launches = st.aggregate_launches;
    if (out_finish_launches) *out_finish_launches = st.finish_launches;
    if (out_delegated_members) *out_delegated_members = st.delegated_members;
    if (out_emitted_rows) *out_emitted_rows = st.emitted_rows;
    if (out_readback_bytes) *out_readback_bytes = st.readback_bytes;
    if (out_host_syncs) *out_host_syncs = st.host_syncs;
    return LOCREC_OK;
}

// =====================================================================================================
// Visitors: rating vectors that are no rows of the index (locrec_knn_visitors_*), over the handle's visitor state.
#include "knn_visitors_api.h"

// One mixed batch of visitors over a pool of indexes (locrec_knn_pool_visitors_*): the pool's waves with the visitors' front.
#include "knn_pool_visitors_entry.h"

// Measurement and tests only (include/locrec.h): what the hit pre-pass of the last batched head / tail scan left in the
// handle's workspaces (knn_ht_prepass.h).  enqueue_ht_prepass records nothing of its own: the shape is what the handle already says about its last scan - the
// plan (kernel 2 or 3: the batch took the head / tail form, so its pre-pass ran), the number of queries, the query tile
// and the candidate slices - and the caller names the batch by its size, as it does for locrec_knn_fetch_topk.  Those
// workspaces are written by the pre-pass alone, so what is copied is always a pre-pass's own output.
extern "C" int32_t locrec_knn_ht_last_hits(locrec_knn_index *ix, int64_t nq, int64_t tile_capacity, int64_t off_capacity,
                                           int64_t hit_capacity, int32_t *out_query_tile, int64_t *out_tiles, int32_t *out_slice0,
                                           int32_t *out_nslices, int64_t *out_tile_base, uint32_t *out_off, uint32_t *out_hits,
                                           int64_t *out_total) try
{
    if (!ix || !out_tiles || !out_total || tile_capacity < 0 || off_capacity < 0 || hit_capacity < 0 ||
        (tile_capacity > 0 && !out_tile_base) || (off_capacity > 0 && !out_off) || (hit_capacity > 0 && !out_hits))
        return fail(LOCREC_E_INVALID_ARG, "NULL argument");
    const locrec::HtIndex &ht = ix->ht;
    const int qt = ix->last_plan_qt;
    const bool ran = ht.ready && !ix->no_ht && ix->have_result && !ix->single_pending && nq > 0 && ix->last_nq == nq &&
                     (ix->last_plan_kernel == 2 || ix->last_plan_kernel == 3) && qt > 0 && ht.tile_base.p && ht.off.p;
    const int64_t ntiles = ran ? (nq + qt - 1) / qt : 0;
    const int64_t off_stride = (int64_t)ix->cand_slice1 - ix->cand_slice0 + 1;
    if (!ran || (size_t)ntiles + 1 > ht.tile_base.n || (size_t)(ntiles * off_stride) > ht.off.n)
        return fail(LOCREC_E_INVALID_ARG, "no matching hit pre-pass to read");
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = ix->stream;
    int64_t total = 0;
    LOCREC_HIP_TRY(hipMemcpyAsync(&total, ht.tile_base.p + ntiles, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    if (total < 0 || (size_t)total > ht.hits.n) return fail(LOCREC_E_INVALID_ARG, "no matching hit pre-pass to read");
    if (out_query_tile) *out_query_tile = qt;
    if (out_slice0) *out_slice0 = ix->cand_slice0;
    if (out_nslices) *out_nslices = ix->cand_slice1;
    *out_tiles = ntiles;
    *out_total = total;
    const int64_t nb = std::min(tile_capacity, ntiles + 1), no = std::min(off_capacity, ntiles * off_stride),
                  nh = std::min(hit_capacity, total);
    if (nb > 0) LOCREC_HIP_TRY(hipMemcpyAsync(out_tile_base, ht.tile_base.p, (size_t)nb * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (no > 0) LOCREC_HIP_TRY(hipMemcpyAsync(out_off, ht.off.p, (size_t)no * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (nh > 0) LOCREC_HIP_TRY(hipMemcpyAsync(out_hits, ht.hits.p, (size_t)nh * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
} LOCREC_CATCH_ALL
