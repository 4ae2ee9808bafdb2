// knn_visitors_api.h -- the entry points for visitors (locrec_knn_visitors_*); a fragment of
// knn_batch.hip's translation unit (behind knn.hip, knn_ranked.h).  The kernels and the tile drivers are knn_visitors.h's
// (compiled with knn_large.hip), every size and regime decision knn_visitors_plan.h's.
//
// A call checks its arguments, then check_params' requires, then stages the vectors (one kernel that also validates every
// visitor: the first offending one goes to *out_bad_visitor), and only then touches a result.  Afterwards nothing is
// resident for locrec_knn_fetch_*: a stray fetch is refused instead of returning a visitor's rows as a person's.
#pragma once

#include "knn_visitors_side.h"
#include "rank_batch.h"

namespace {

// nothing of a visitors call stays resident in the handle
void knn_visitors_forget(locrec_knn_index *ix)
{
    ix->have_result = false;
    ix->single_pending = false;
    ix->single_direct = false;
    ix->last_scan_fast = false;
    ix->have_agg = false;
    ix->have_lkb = false;
}

// The beginning of every visitors call: the arguments (outputs_ok: the entry's own; more_args: further argument checks of
// the entry, before the requires), check_params, then the stage with its per-visitor refusals into the handle's visitor state
// (ix->visitors).
template <class F>
int32_t knn_visitors_begin(locrec_knn_index *ix, const locrec::KnnVisitorVectors &v, double pw, double cw, int64_t k, bool outputs_ok,
                           int64_t *out_bad, F more_args)
{
    if (out_bad) *out_bad = -1;
    locrec::knn_visitors_stats() = locrec::KnnVisitorsStats();
    if (!ix) return fail(LOCREC_E_INVALID_ARG, "index is NULL");
    knn_visitors_forget(ix);
    if (v.nv < 0 || v.nv > locrec::kVisitorsMax || (v.nv > 0 && (!v.p_ptr || !v.c_ptr)) || !outputs_ok)
        return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    if (v.mem != LOCREC_MEM_HOST && v.mem != LOCREC_MEM_DEVICE)
        return fail(LOCREC_E_INVALID_ARG, "mem must be LOCREC_MEM_HOST or LOCREC_MEM_DEVICE");
    LOCREC_TRY(more_args());
    LOCREC_TRY(check_params(pw, cw, k));
    if (v.nv == 0) return LOCREC_OK;
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    return locrec::knn_visitors_stage(ix, ix->visitors, v, out_bad);
}

int32_t knn_visitors_no_more_args() { return LOCREC_OK; }

// the recommendation rows of the staged visitors, resident in lkb_place / lkb_est / lkb_off (an index without persons: none)
int32_t knn_visitors_rows(locrec_knn_index *ix, int64_t nv, double pw, double cw, int64_t k)
{
    const int64_t worst = locrec::knn_visitors_worst_row_bytes(nv, (int64_t)ix->cplace_ids.size());
    if (worst > locrec::kVisitorsMaxRowBytes)
        return fail(LOCREC_E_INVALID_ARG, "a batch of %lld visitors may return %lld GB of rows: split it", (long long)nv,
                    (long long)(worst >> 30));
    if (ix->n == 0) {
        ix->lkb_off.assign((size_t)nv + 1, 0);
        return LOCREC_OK;
    }
    return locrec::knn_visitors_recommend(ix, ix->visitors, nv, pw, cw, k);
}

}  // namespace

extern "C" int32_t locrec_knn_visitors_query_batch(locrec_knn_index *ix, int64_t nv, const int64_t *p_rowptr, const int32_t *p_idx,
                                                   const double *p_val, const int64_t *c_rowptr, const int32_t *c_idx,
                                                   const double *c_val, int32_t mem, double pw, double cw, int64_t k,
                                                   int64_t *out_ids, double *out_sims, int64_t *out_counts,
                                                   int64_t *out_bad_visitor) try
{
    const locrec::KnnVisitorVectors v{nv, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, mem};
    LOCREC_TRY(knn_visitors_begin(ix, v, pw, cw, k, nv <= 0 || (out_ids && out_sims && out_counts), out_bad_visitor,
                                  knn_visitors_no_more_args));
    if (nv == 0) return LOCREC_OK;
    if (ix->n == 0) {  // nobody to be similar to
        std::fill(out_ids, out_ids + nv * k, (int64_t)-1);
        std::fill(out_sims, out_sims + nv * k, 0.0);
        std::fill(out_counts, out_counts + nv, (int64_t)0);
        return LOCREC_OK;
    }
    hipStream_t s = ix->stream;
    // (the switch is read at every call: tests run chunks of a few visitors beside the default in one process)
    const int64_t chunk = locrec::knn_visitors_chunk(k, locrec::knn_visitors_chunk_budget(std::getenv("LOCREC_KNN_VISITORS_CHUNK_BYTES")));
    int32_t rc = LOCREC_OK;
    for (int64_t v0 = 0; v0 < nv && rc == LOCREC_OK; v0 += chunk) {
        const int64_t cn = std::min(chunk, nv - v0);
        rc = locrec::knn_visitors_topk(ix, ix->visitors, v0, cn, pw, cw, k);
        if (rc != LOCREC_OK) break;
        LOCREC_HIP_TRY(hipMemcpyAsync(out_ids + v0 * k, ix->out_ids.p, (size_t)(cn * k) * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(out_sims + v0 * k, ix->out_sims.p, (size_t)(cn * k) * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(out_counts + v0, ix->out_cnt.p, (size_t)cn * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        ++locrec::knn_visitors_stats().host_syncs;
    }
    return rc;
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_visitors_recommend_batch(locrec_knn_index *ix, int64_t nv, const int64_t *p_rowptr,
                                                       const int32_t *p_idx, const double *p_val, const int64_t *c_rowptr,
                                                       const int32_t *c_idx, const double *c_val, int32_t mem, double pw, double cw,
                                                       int64_t k, int64_t *out_offsets, int64_t *out_places, double *out_ratings,
                                                       int64_t *inout_capacity, int64_t *out_bad_visitor) try
{
    const locrec::KnnVisitorVectors v{nv, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, mem};
    LOCREC_TRY(knn_visitors_begin(ix, v, pw, cw, k, out_offsets && inout_capacity, out_bad_visitor, knn_visitors_no_more_args));
    if (nv == 0) {
        out_offsets[0] = 0;
        *inout_capacity = 0;
        return LOCREC_OK;
    }
    LOCREC_TRY(knn_visitors_rows(ix, nv, pw, cw, k));
    hipStream_t s = ix->stream;
    std::copy(ix->lkb_off.begin(), ix->lkb_off.begin() + nv + 1, out_offsets);
    const int64_t total = out_offsets[nv], cap = *inout_capacity;
    *inout_capacity = total;
    if (total > cap || total == 0) return LOCREC_OK;  // (the caller looks at the returned total and calls again)
    if (!out_places || !out_ratings) return fail(LOCREC_E_INVALID_ARG, "NULL output buffer");
    LOCREC_HIP_TRY(hipMemcpyAsync(out_places, ix->lkb_place.p, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(out_ratings, ix->lkb_est.p, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    ++locrec::knn_visitors_stats().host_syncs;
    return LOCREC_OK;
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_visitors_recommend_ranked_batch(
    locrec_knn_index *ix, int64_t nv, const int64_t *p_rowptr, const int32_t *p_idx, const double *p_val, const int64_t *c_rowptr,
    const int32_t *c_idx, const double *c_val, int32_t mem, double pw, double cw, int64_t k, int64_t n_places,
    const int64_t *place_ids, const int64_t *place_region_ids, const int64_t *target_region_ids, int64_t max_recommendations,
    const int64_t *exclude_offsets, const int64_t *exclude_place_ids, int64_t *out_place_ids, double *out_estimated_ratings,
    int64_t *out_counts, int64_t *out_bad_visitor) try
{
    const int64_t N = std::max<int64_t>(0, max_recommendations);
    const locrec::KnnVisitorVectors v{nv, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, mem};
    int64_t n_ex = 0;
    const auto rank_args = [&]() -> int32_t {
        if (nv == 0) return LOCREC_OK;
        LOCREC_TRY(knn_rank_check_args(n_places, place_ids, place_region_ids, target_region_ids, N, out_place_ids,
                                       out_estimated_ratings, out_counts));
        if (!exclude_offsets) {
            if (exclude_place_ids) return fail(LOCREC_E_INVALID_ARG, "exclude_place_ids without exclude_offsets");
            return LOCREC_OK;
        }
        n_ex = exclude_offsets[nv];
        bool ok = exclude_offsets[0] >= 0 && n_ex < ((int64_t)1 << 31);
        for (int64_t i = 0; i < nv && ok; ++i) ok = exclude_offsets[i] <= exclude_offsets[i + 1];
        if (!ok) return fail(LOCREC_E_INVALID_ARG, "exclude_offsets must be non-decreasing inside [0, 2^31)");
        if (n_ex > 0 && !exclude_place_ids) return fail(LOCREC_E_INVALID_ARG, "NULL argument");
        return LOCREC_OK;
    };
    LOCREC_TRY(knn_visitors_begin(ix, v, pw, cw, k, true, out_bad_visitor, rank_args));
    if (nv == 0) return LOCREC_OK;
    LOCREC_TRY(knn_visitors_rows(ix, nv, pw, cw, k));
    hipStream_t s = ix->stream;
    if (ix->lkb_off[(size_t)nv] == 0) {  // no rows at all (an index without persons or ratings has no row buffer either)
        std::fill(out_place_ids, out_place_ids + nv * N, (int64_t)-1);
        std::fill(out_estimated_ratings, out_estimated_ratings + nv * N, 0.0);
        std::fill(out_counts, out_counts + nv, (int64_t)0);
        return LOCREC_OK;
    }
    // ONE upload of the places table, the targets, the segments and the caller's lists; the ranker over the resident rows
    const size_t io_words = RankIo::in_words(n_places, nv);
    std::vector<int64_t> hin(io_words + (exclude_offsets ? 2 * (size_t)nv + (size_t)n_ex : 0) + 1);
    if (n_places > 0) {
        std::copy(place_ids, place_ids + n_places, hin.begin());
        std::copy(place_region_ids, place_region_ids + n_places, hin.begin() + n_places);
    }
    for (int64_t i = 0; i < nv; ++i) {
        hin[(size_t)(2 * n_places + i)] = target_region_ids[i];
        hin[(size_t)(2 * n_places + nv + i)] = ix->lkb_off[(size_t)i];
        hin[(size_t)(2 * n_places + 2 * nv + i)] = ix->lkb_off[(size_t)i + 1] - ix->lkb_off[(size_t)i];
        if (exclude_offsets) {
            hin[io_words + (size_t)i] = exclude_offsets[i];
            hin[io_words + (size_t)(nv + i)] = exclude_offsets[i + 1] - exclude_offsets[i];
        }
    }
    if (n_ex > 0) std::copy(exclude_place_ids, exclude_place_ids + n_ex, hin.begin() + (ptrdiff_t)(io_words + 2 * (size_t)nv));
    locrec::KnnVisitorSide *side = &ix->visitors;
    LOCREC_TRY(side->rk_in.reserve(hin.size()));
    LOCREC_TRY(side->rk_out.reserve(RankIo::out_words(nv, N)));
    const RankIo io(side->rk_in.p, side->rk_out.p, n_places, nv, N);
    LOCREC_HIP_TRY(hipMemcpyAsync(side->rk_in.p, hin.data(), hin.size() * 8, hipMemcpyHostToDevice, s));
    RankExclude ex;
    if (exclude_offsets) {
        ex.begin = side->rk_in.p + io_words;
        ex.len = ex.begin + nv;
        ex.ids = ex.len + nv;
        ex.n = n_ex;
    }
    const int32_t rc = io.rank(ix->lkb_place.p, ix->lkb_est.p, 0, s, ex);
    if (rc != LOCREC_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    LOCREC_TRY(io.read_back(out_place_ids, out_estimated_ratings, out_counts, s));
    locrec::knn_visitors_stats().host_syncs += rank_batch_stats().host_syncs + 1;
    return LOCREC_OK;
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_visitors_stats(int64_t out[8])
{
    if (!out) return fail(LOCREC_E_INVALID_ARG, "NULL argument");
    const locrec::KnnVisitorsStats &st = locrec::knn_visitors_stats();
    out[0] = st.tiles;
    out[1] = st.tiles_all;
    out[2] = st.tiles_topk;
    out[3] = st.beyond;
    out[4] = st.renumbered;
    out[5] = st.stage_launches;
    out[6] = st.scan_launches;
    out[7] = st.host_syncs;
    return LOCREC_OK;
}
