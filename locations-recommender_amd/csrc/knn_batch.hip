// knn_batch.hip -- the batched KNN entry points at any K: findSimilarPersons / makeRecommendations for many persons
// when k_nearest exceeds the per-query LDS lists (LOCREC_KNN_BATCH_MAX_K), e.g. the shipped --k-nearest 2000000
// (bin/knn_recommender.sh:35) below N - 1.
//
// This file is the KNN translation unit: it includes knn.hip whole and defines the six batch entry points that carried
// the limit (or served 1024 < K < N - 1 one query at a time) in front of it.  knn.hip itself stays as it is: its bytes
// are part of the hash that ties the committed rocprofv3 counter record to the kernels it measured (bench.py
// PMC_SOURCES).  So knn.hip's definitions are renamed on the way in (the macros below) to internal names outside the
// locrec_ prefix, and the public names defined here forward to them for K <= LOCREC_KNN_BATCH_MAX_K (and, in the
// recommend calls, for K >= N - 1): those calls run exactly the code they ran before.  Calls between these functions
// inside knn.hip stay on the originals, which is right: the functions here serve K > LOCREC_KNN_BATCH_MAX_K themselves.
// Any other K takes the tiled top-K of knn_large.hip (knn_anyk.h).
//
// The tiled path keeps its device buffers in handle members that already exist (the handle's layout is hashed too):
//   lkb_S                     a tile's similarities, transposed, and the masked row-major tile of the aggregation
//   lk_keys / lk_vals (+ _out) the tile's segments, ping-pong of the merge passes
//   tile_hist / tile_sel      one histogram and one selection record per column (shared with enqueue_topk)
//   out_*                     the neighbour lists, as every batch leaves them for locrec_knn_fetch_topk
//   lkb_*                     the place-major aggregation and its resident result (locrec_knn_fetch_recommend)
// They are grow-only and freed with the handle.  The deferred one-by-one branch of fetch_large_k_batch (knn.hip) is
// no longer reachable - no call here sets lkb_deferred - and stays only because knn.hip's bytes are hashed.

#define locrec_knn_query_batch knn_query_batch_lds
#define locrec_knn_topk_range_async knn_topk_range_async_lds
#define locrec_knn_all_pairs_topk knn_all_pairs_topk_lds
#define locrec_knn_query_shard knn_query_shard_lds
#define locrec_knn_recommend_batch knn_recommend_batch_lds
#define locrec_knn_recommend_range_async knn_recommend_range_async_lds

#include "knn.hip"

#undef locrec_knn_query_batch
#undef locrec_knn_topk_range_async
#undef locrec_knn_all_pairs_topk
#undef locrec_knn_query_shard
#undef locrec_knn_recommend_batch
#undef locrec_knn_recommend_range_async

#include "knn_anyk.h"

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

// makeRecommendations with 1024 < K < N - 1 for rows (processing order), resident on the device like
// enqueue_large_k_batch leaves the K >= N - 1 batch
int32_t enqueue_any_k_recommend(locrec_knn_index *ix, const std::vector<int32_t> &rows, double pw, double cw, int64_t k)
{
    const int64_t nq = (int64_t)rows.size();
    ix->agg_rows = rows;
    ix->agg_first = -1;
    ix->agg_pw = pw;
    ix->agg_cw = cw;
    ix->last_nq = nq;
    ix->last_k = k;
    ix->single_pending = false;
    ix->have_result = false;  // (no neighbour lists are left for locrec_knn_fetch_topk)
    ix->have_agg = false;
    const int64_t worst = nq * (int64_t)std::max<size_t>(1, ix->cplace_ids.size()) * 16;
    if (worst > ((int64_t)48 << 30))
        return fail(LOCREC_E_INVALID_ARG, "a batch of %lld queries at K = %lld may return %lld GB of rows: split it",
                    (long long)nq, (long long)k, (long long)(worst >> 30));
    ix->lkb_deferred = false;
    return knn_topk_recommend_batch(ix, rows.data(), nq, pw, cw, k);
}

// the recommend calls take the tiled top-K for LOCREC_KNN_BATCH_MAX_K < K < N - 1
bool any_k_recommend(const locrec_knn_index *ix, int64_t k) { return k > LOCREC_KNN_BATCH_MAX_K && k < ix->n - 1; }

}  // namespace

extern "C" int32_t locrec_knn_query_batch(locrec_knn_index *ix, int64_t nq, const int64_t *person_ids, double pw, double cw,
                                          int64_t k, int64_t *out_ids, double *out_sims, int64_t *out_counts) try
{
    if (!ix || k <= LOCREC_KNN_BATCH_MAX_K)
        return knn_query_batch_lds(ix, nq, person_ids, pw, cw, k, out_ids, out_sims, out_counts);
    ix->have_result = false;
    LOCREC_TRY(check_params(pw, cw, k));
    if (nq < 0 || (nq > 0 && !person_ids)) return fail(LOCREC_E_INVALID_ARG, "bad query list");
    if (nq == 0) return LOCREC_OK;
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    std::vector<int32_t> rows((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) LOCREC_TRY(find_query_row(ix, person_ids[i], &rows[(size_t)i]));
    return any_k_rows(ix, rows, pw, cw, k, false, out_ids, out_sims, out_counts);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_topk_range_async(locrec_knn_index *ix, int64_t first, int64_t nq, double pw, double cw,
                                               int64_t k) try
{
    if (!ix || k <= LOCREC_KNN_BATCH_MAX_K) return knn_topk_range_async_lds(ix, first, nq, pw, cw, k);
    ix->have_result = false;
    LOCREC_TRY(check_params(pw, cw, k));
    if (first < 0 || nq <= 0 || first + nq > ix->n) return fail(LOCREC_E_INVALID_ARG, "row range out of bounds");
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    // (the whole range stays resident until locrec_knn_fetch_topk: nq x k entries)
    std::vector<int32_t> rows((size_t)nq);
    std::iota(rows.begin(), rows.end(), (int32_t)first);
    return enqueue_any_k(ix, rows.data(), nq, pw, cw, k, true);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_all_pairs_topk(locrec_knn_index *ix, double pw, double cw, int64_t k, int64_t *out_ids,
                                             double *out_sims, int64_t *out_counts) try
{
    if (!ix || k <= LOCREC_KNN_BATCH_MAX_K) return knn_all_pairs_topk_lds(ix, pw, cw, k, out_ids, out_sims, out_counts);
    LOCREC_TRY(check_params(pw, cw, k));
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    // every person as the query, in the order of person_ids[] given at create
    std::vector<int32_t> rows(ix->row_of_input.begin(), ix->row_of_input.end());
    return any_k_rows(ix, rows, pw, cw, k, true, out_ids, out_sims, out_counts);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_query_shard(locrec_knn_index *ix, int64_t person_id, double pw, double cw, int64_t k,
                                          int32_t shard_index, int32_t shard_count, int64_t *out_ids, double *out_sims,
                                          int64_t *inout_count) try
{
    if (!ix || !inout_count || std::min<int64_t>(k, std::max<int64_t>(1, ix->n - 1)) <= LOCREC_KNN_BATCH_MAX_K)
        return knn_query_shard_lds(ix, person_id, pw, cw, k, shard_index, shard_count, out_ids, out_sims, inout_count);
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
    // the single request's full sort over this shard's candidates (lk_gather_keys honours the slice range)
    CandRangeGuard guard(ix, s0, s1);
    return knn_large_topk(ix, row, pw, cw, keff, out_ids, out_sims, inout_count);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_recommend_range_async(locrec_knn_index *ix, int64_t first, int64_t nq, double pw, double cw,
                                                    int64_t k) try
{
    if (!ix || !any_k_recommend(ix, k)) return knn_recommend_range_async_lds(ix, first, nq, pw, cw, k);
    ix->have_agg = false;
    ix->have_lkb = false;
    LOCREC_TRY(check_params(pw, cw, k));
    if (first < 0 || nq <= 0 || first + nq > ix->n) return fail(LOCREC_E_INVALID_ARG, "row range out of bounds");
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    std::vector<int32_t> rows((size_t)nq);
    std::iota(rows.begin(), rows.end(), (int32_t)first);
    return enqueue_any_k_recommend(ix, rows, pw, cw, k);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_recommend_batch(locrec_knn_index *ix, int64_t nq, const int64_t *person_ids, double pw,
                                              double cw, int64_t k, int64_t *out_offsets, int64_t *out_places,
                                              double *out_ratings, int64_t *inout_capacity) try
{
    if (!ix || !any_k_recommend(ix, k) || nq <= 0 || !person_ids || !out_offsets || !inout_capacity)
        return knn_recommend_batch_lds(ix, nq, person_ids, pw, cw, k, out_offsets, out_places, out_ratings, inout_capacity);
    ix->have_result = false;
    ix->have_agg = false;
    ix->have_lkb = false;
    LOCREC_TRY(check_params(pw, cw, k));
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    std::vector<int32_t> rows((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) LOCREC_TRY(find_query_row(ix, person_ids[i], &rows[(size_t)i]));
    // in input order (the tiled path keeps no order of its own): the resident rows go straight to the caller's arrays, or
    // only the offsets and the total when they do not fit
    LOCREC_TRY(enqueue_any_k_recommend(ix, rows, pw, cw, k));
    return locrec_knn_fetch_recommend(ix, nq, out_offsets, out_places, out_ratings, inout_capacity);
} LOCREC_CATCH_ALL

// the ranked forms of the two recommend calls above (and locrec_knn_fetch_ranked for the range form)
#include "knn_ranked.h"
