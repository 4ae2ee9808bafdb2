// knn_pool_visitors_entry.h -- the entry points for one mixed batch of visitors over a pool of indexes
// (locrec_knn_pool_visitors_*); a fragment of knn_batch.hip's translation unit (behind the pool's and the visitors' entry
// points).  The kernels and the wave driver are knn_pool_visitors.h's (compiled with knn_large.hip), every decision
// knn_pool_visitors_plan.h's.
//
// A call checks, in this order and before any result is written: its arguments; every index position; check_params'
// requires; that every asked member has a record for visitors; then every visitor, in ONE stage launch for all members
// (the first offender in call order goes to *out_bad_visitor).  A sharing member's visitors take the pool's waves, a member
// without persons has no rows, any other member's visitors are gathered into a CSR of their own and handed to its own
// locrec_knn_visitors_* call.  Afterwards nothing is resident in any asked member for locrec_knn_fetch_*.
#pragma once

#include "knn_pool_visitors_api.h"

static_assert(locrec::kPoolVisitorsBatchMaxK == LOCREC_KNN_BATCH_MAX_K, "knn_pool_visitors_plan.h restates LOCREC_KNN_BATCH_MAX_K");

namespace {

// One pool-visitors call: its visitors sorted out (knn_pool_visitors_plan.h), the asked members marked, the sharing members' batches and every visitor's rows in the pool's buffers
struct KnnPoolVisitorsCall : locrec::KnnPoolVisitorsPlan {
    std::vector<locrec::KnnPoolVisitorsMember> members;
    std::vector<locrec::KnnPoolVisitorsBatch> batches;
    std::vector<int64_t> base, len;   // per visitor (a delegated member's: 0, 0)
    std::vector<char> is_delegated;   // per visitor
    const int64_t *d_place = nullptr;
    const double *d_est = nullptr;
};

// The beginning of both entries (outputs_ok: the entry's own; more_args: further argument checks of the entry, before the
// index positions), through the stage and the plan.  nv == 0: nothing but the checks.
template <class F>
int32_t knn_pool_visitors_begin(locrec_knn_pool *pool, const locrec::KnnVisitorVectors &v, const int32_t *index_of, double pw, double cw,
                                int64_t k, bool outputs_ok, int64_t *out_bad, F more_args, KnnPoolVisitorsCall &call)
{
    if (!pool) return fail(LOCREC_E_INVALID_ARG, "pool is NULL");
    if (out_bad) *out_bad = -1;
    locrec::knn_pool_visitors_stats() = locrec::KnnPoolVisitorsStats();
    const int64_t nv = v.nv;
    if (nv < 0 || nv > locrec::kVisitorsMax || (nv > 0 && (!index_of || !v.p_ptr || !v.c_ptr)) || !outputs_ok)
        return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    if (v.mem != LOCREC_MEM_HOST && v.mem != LOCREC_MEM_DEVICE)
        return fail(LOCREC_E_INVALID_ARG, "mem must be LOCREC_MEM_HOST or LOCREC_MEM_DEVICE");
    LOCREC_TRY(more_args());
    const int32_t nm = (int32_t)pool->members.size();
    for (int64_t i = 0; i < nv; ++i)
        if (index_of[i] < 0 || index_of[i] >= nm) {
            if (out_bad) *out_bad = i;
            return fail(LOCREC_E_INVALID_ARG, "visitor %lld names index %d of a pool of %d", (long long)i, index_of[i], nm);
        }
    LOCREC_TRY(check_params(pw, cw, k));
    if (nv == 0) return LOCREC_OK;
    call.members.resize((size_t)nm);
    for (int32_t m = 0; m < nm; ++m) call.members[(size_t)m].ix = pool->members[(size_t)m];
    for (int64_t i = 0; i < nv; ++i) call.members[(size_t)index_of[i]].asked = true;
    LOCREC_HIP_TRY(hipSetDevice(pool->device));
    if (!pool->visitors) pool->visitors = locrec::knn_pool_visitors_create();
    for (const auto &m : call.members)
        if (m.asked) knn_visitors_forget(m.ix);
    LOCREC_TRY(locrec::knn_pool_visitors_stage(pool->visitors, pool->device, pool->stream, call.members, index_of, v, out_bad));
    std::vector<locrec::KnnPoolVisitorsWay> way((size_t)nm);
    for (int32_t m = 0; m < nm; ++m) way[(size_t)m] = locrec::knn_pool_visitors_way(k, pool->members[(size_t)m]->n);
    locrec::knn_pool_visitors_plan(nv, index_of, way, call);
    // the refusal of a batch whose rows cannot be held, on the call's total
    std::vector<int64_t> asked_n, asked_places;
    for (const auto *cuts : {&call.shared, &call.delegated, &call.empty})
        for (const auto &c : *cuts) {
            asked_n.push_back(c.n);
            asked_places.push_back((int64_t)pool->members[(size_t)c.member]->cplace_ids.size());
        }
    const int64_t worst = locrec::knn_pool_visitors_worst_row_bytes(asked_n.size(), asked_n.data(), asked_places.data());
    if (worst > locrec::kVisitorsMaxRowBytes)
        return fail(LOCREC_E_INVALID_ARG, "a pool batch of %lld visitors may return %lld GB of rows: split it", (long long)nv,
                    (long long)(worst >> 30));
    call.is_delegated.assign((size_t)nv, 0);
    for (const auto &c : call.delegated)
        for (int64_t j = 0; j < c.n; ++j) call.is_delegated[(size_t)call.order[(size_t)(c.first + j)]] = 1;
    for (const auto &c : call.shared)
        call.batches.push_back({pool->members[(size_t)c.member], call.order.data() + c.first, c.n});
    return LOCREC_OK;
}

// the sharing members' part of a call: rows resident in the pool's buffers
int32_t knn_pool_visitors_run_shared(locrec_knn_pool *pool, KnnPoolVisitorsCall &call, int64_t nv, double pw, double cw)
{
    call.base.assign((size_t)nv, 0);
    call.len.assign((size_t)nv, 0);
    if (call.batches.empty()) return LOCREC_OK;
    return locrec::knn_pool_visitors_run(pool->shared, pool->visitors, pool->stream, call.batches, pw, cw, call.base.data(),
                                         call.len.data(), &call.d_place, &call.d_est);
}

// the delegated members: f(d, member, its visitors (call positions, ascending), their number, their vectors as a CSR of
// their own) = its own public call and the scatter
template <class F>
int32_t knn_pool_visitors_each_delegated(locrec_knn_pool *pool, const KnnPoolVisitorsCall &call, const locrec::KnnVisitorVectors &v, F f)
{
    locrec::knn_pool_visitors_stats().delegated_members = (int64_t)call.delegated.size();
    for (size_t d = 0; d < call.delegated.size(); ++d) {
        const auto &c = call.delegated[d];
        locrec_knn_index *ix = pool->members[(size_t)c.member];
        const int64_t *vis = call.order.data() + c.first;
        locrec::KnnVisitorVectors g{};
        LOCREC_TRY(locrec::knn_pool_visitors_gather(pool->visitors, pool->stream, v, vis, c.n, &g));
        const int32_t rc = f(d, ix, vis, c.n, g);
        knn_visitors_forget(ix);
        if (rc != LOCREC_OK) return rc;
    }
    return LOCREC_OK;
}

}  // namespace

extern "C" int32_t locrec_knn_pool_visitors_recommend_batch(
    locrec_knn_pool *pool, int64_t nv, const int32_t *index_of_visitor, const int64_t *p_rowptr, const int32_t *p_idx,
    const double *p_val, const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t mem, double pw, double cw,
    int64_t k, int64_t *out_offsets, int64_t *out_places, double *out_ratings, int64_t *inout_capacity, int64_t *out_bad_visitor) try
{
    KnnPoolVisitorsCall call;
    const locrec::KnnVisitorVectors v{nv, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, mem};
    LOCREC_TRY(knn_pool_visitors_begin(pool, v, index_of_visitor, pw, cw, k, out_offsets && inout_capacity, out_bad_visitor,
                                       knn_visitors_no_more_args, call));
    if (nv == 0) {
        out_offsets[0] = 0;
        *inout_capacity = 0;
        return LOCREC_OK;
    }
    LOCREC_TRY(knn_pool_visitors_run_shared(pool, call, nv, pw, cw));
    locrec::KnnPoolVisitorsStats &st = locrec::knn_pool_visitors_stats();
    hipStream_t s = pool->stream;
    std::vector<int64_t> rlen(call.len);
    // the delegated members: their own call on their own visitors, sizes first
    std::vector<std::vector<int64_t>> d_off(call.delegated.size());
    const auto sizes = [&](size_t d, locrec_knn_index *ix, const int64_t *vis, int64_t n, const locrec::KnnVisitorVectors &g) -> int32_t {
        d_off[d].assign((size_t)n + 1, 0);
        int64_t cap = 0;
        LOCREC_TRY(locrec_knn_visitors_recommend_batch(ix, n, g.p_ptr, g.p_idx, g.p_val, g.c_ptr, g.c_idx, g.c_val, g.mem, pw, cw, k,
                                                       d_off[d].data(), nullptr, nullptr, &cap, nullptr));
        for (int64_t j = 0; j < n; ++j) rlen[(size_t)vis[j]] = d_off[d][(size_t)j + 1] - d_off[d][(size_t)j];
        return LOCREC_OK;
    };
    LOCREC_TRY(knn_pool_visitors_each_delegated(pool, call, v, sizes));
    const int64_t total = std::accumulate(rlen.begin(), rlen.end(), (int64_t)0);
    const bool sizes_only = total > *inout_capacity || total == 0;  // (nothing but the offsets and the total)
    if (!sizes_only && (!out_places || !out_ratings)) return fail(LOCREC_E_INVALID_ARG, "NULL output buffer");
    out_offsets[0] = 0;
    for (int64_t i = 0; i < nv; ++i) out_offsets[i + 1] = out_offsets[i] + rlen[(size_t)i];
    *inout_capacity = total;
    if (sizes_only) return LOCREC_OK;
    // the shared rows: one copy of the pool's row buffer, handed out in call order
    int64_t resident = 0;
    for (int64_t i = 0; i < nv; ++i) resident = std::max(resident, call.base[(size_t)i] + call.len[(size_t)i]);
    std::vector<int64_t> hp((size_t)resident);
    std::vector<double> he((size_t)resident);
    if (resident > 0) {
        LOCREC_HIP_TRY(hipMemcpyAsync(hp.data(), call.d_place, (size_t)resident * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(he.data(), call.d_est, (size_t)resident * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        st.readback_bytes += resident * 16;
        ++st.host_syncs;
    }
    for (int64_t i = 0; i < nv; ++i) {
        const int64_t b = call.base[(size_t)i], n = call.len[(size_t)i];
        if (call.is_delegated[(size_t)i] || n == 0) continue;
        std::copy(hp.begin() + b, hp.begin() + b + n, out_places + out_offsets[i]);
        std::copy(he.begin() + b, he.begin() + b + n, out_ratings + out_offsets[i]);
    }
    const auto rows = [&](size_t d, locrec_knn_index *ix, const int64_t *vis, int64_t n, const locrec::KnnVisitorVectors &g) -> int32_t {
        int64_t mcap = d_off[d].back();
        if (mcap == 0) return LOCREC_OK;
        std::vector<int64_t> mp((size_t)mcap);
        std::vector<double> me((size_t)mcap);
        LOCREC_TRY(locrec_knn_visitors_recommend_batch(ix, n, g.p_ptr, g.p_idx, g.p_val, g.c_ptr, g.c_idx, g.c_val, g.mem, pw, cw, k,
                                                       d_off[d].data(), mp.data(), me.data(), &mcap, nullptr));
        for (int64_t j = 0; j < n; ++j) {
            std::copy(mp.begin() + d_off[d][(size_t)j], mp.begin() + d_off[d][(size_t)j + 1], out_places + out_offsets[vis[j]]);
            std::copy(me.begin() + d_off[d][(size_t)j], me.begin() + d_off[d][(size_t)j + 1], out_ratings + out_offsets[vis[j]]);
        }
        return LOCREC_OK;
    };
    return knn_pool_visitors_each_delegated(pool, call, v, rows);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_pool_visitors_recommend_ranked_batch(
    locrec_knn_pool *pool, int64_t nv, const int32_t *index_of_visitor, const int64_t *p_rowptr, const int32_t *p_idx,
    const double *p_val, const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t mem, double pw, double cw,
    int64_t k, int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids, const int64_t *target_region_ids,
    int64_t max_recommendations, const int64_t *exclude_offsets, const int64_t *exclude_place_ids, int64_t *out_place_ids,
    double *out_estimated_ratings, int64_t *out_counts, int64_t *out_bad_visitor) try
{
    const int64_t N = std::max<int64_t>(0, max_recommendations);
    KnnPoolVisitorsCall call;
    const locrec::KnnVisitorVectors v{nv, p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val, mem};
    int64_t n_ex = 0;
    const auto rank_args = [&]() -> int32_t {  // (locrec_knn_visitors_recommend_ranked_batch's checks and texts)
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
    LOCREC_TRY(knn_pool_visitors_begin(pool, v, index_of_visitor, pw, cw, k, true, out_bad_visitor, rank_args, call));
    if (nv == 0) return LOCREC_OK;
    LOCREC_TRY(knn_pool_visitors_run_shared(pool, call, nv, pw, cw));
    locrec::KnnPoolVisitorsStats &st = locrec::knn_pool_visitors_stats();
    hipStream_t s = pool->stream;
    // one segment per visitor of a sharing member or of a member without persons, in call order
    std::vector<int64_t> seg_req;
    int64_t resident = 0;
    for (int64_t i = 0; i < nv; ++i)
        if (!call.is_delegated[(size_t)i]) {
            seg_req.push_back(i);
            resident = std::max(resident, call.base[(size_t)i] + call.len[(size_t)i]);
        }
    const int64_t nseg = (int64_t)seg_req.size();
    if (nseg > 0 && resident == 0) {  // no rows at all (the pool may have no row buffer either)
        for (int64_t i : seg_req) {
            std::fill(out_place_ids + i * N, out_place_ids + (i + 1) * N, (int64_t)-1);
            std::fill(out_estimated_ratings + i * N, out_estimated_ratings + (i + 1) * N, 0.0);
            out_counts[i] = 0;
        }
    } else if (nseg > 0) {
        // ONE upload of the places table, the targets, the segments and the caller's lists; one ranker call over the pool's rows
        const size_t io_words = RankIo::in_words(n_places, nseg);
        std::vector<int64_t> hin(io_words + (exclude_offsets ? 2 * (size_t)nseg + (size_t)n_ex : 0) + 1);
        if (n_places > 0) {
            std::copy(place_ids, place_ids + n_places, hin.begin());
            std::copy(place_region_ids, place_region_ids + n_places, hin.begin() + n_places);
        }
        for (int64_t c = 0; c < nseg; ++c) {
            const int64_t i = seg_req[(size_t)c];
            hin[(size_t)(2 * n_places + c)] = target_region_ids[i];
            hin[(size_t)(2 * n_places + nseg + c)] = call.base[(size_t)i];
            hin[(size_t)(2 * n_places + 2 * nseg + c)] = call.len[(size_t)i];
            if (exclude_offsets) {
                hin[io_words + (size_t)c] = exclude_offsets[i];
                hin[io_words + (size_t)(nseg + c)] = exclude_offsets[i + 1] - exclude_offsets[i];
            }
        }
        if (n_ex > 0) std::copy(exclude_place_ids, exclude_place_ids + n_ex, hin.begin() + (ptrdiff_t)(io_words + 2 * (size_t)nseg));
        LOCREC_TRY(pool->rk_in.reserve(hin.size()));
        LOCREC_TRY(pool->rk_out.reserve(RankIo::out_words(nseg, N)));
        const RankIo io(pool->rk_in.p, pool->rk_out.p, n_places, nseg, N);
        LOCREC_HIP_TRY(hipMemcpyAsync(pool->rk_in.p, hin.data(), hin.size() * 8, hipMemcpyHostToDevice, s));
        RankExclude ex;
        if (exclude_offsets) {
            ex.begin = pool->rk_in.p + io_words;
            ex.len = ex.begin + nseg;
            ex.ids = ex.len + nseg;
            ex.n = n_ex;
        }
        const int32_t rc = io.rank(call.d_place, call.d_est, 0, s, ex);
        if (rc != LOCREC_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        LOCREC_TRY(io.read_back_to(seg_req, out_place_ids, out_estimated_ratings, out_counts, s));
        st.readback_bytes += nseg * N * 16 + nseg * 8;
        st.host_syncs += rank_batch_stats().host_syncs + 1;
    }
    // the delegated members: their own ranked call on their own visitors, targets and lists
    const auto ranked = [&](size_t, locrec_knn_index *ix, const int64_t *vis, int64_t n, const locrec::KnnVisitorVectors &g) -> int32_t {
        std::vector<int64_t> tgt((size_t)n), oid((size_t)(n * N)), ocnt((size_t)n), ex_off, ex_ids;
        std::vector<double> osc((size_t)(n * N));
        for (int64_t j = 0; j < n; ++j) tgt[(size_t)j] = target_region_ids[vis[j]];
        if (exclude_offsets) {
            ex_off.assign((size_t)n + 1, 0);
            for (int64_t j = 0; j < n; ++j) {
                const int64_t a = exclude_offsets[vis[j]], b = exclude_offsets[vis[j] + 1];
                ex_ids.insert(ex_ids.end(), exclude_place_ids + a, exclude_place_ids + b);
                ex_off[(size_t)j + 1] = (int64_t)ex_ids.size();
            }
            if (ex_ids.empty()) ex_ids.push_back(0);  // (never read: a non-null pointer for the lists' checks)
        }
        LOCREC_TRY(locrec_knn_visitors_recommend_ranked_batch(
            ix, n, g.p_ptr, g.p_idx, g.p_val, g.c_ptr, g.c_idx, g.c_val, g.mem, pw, cw, k, n_places, place_ids, place_region_ids,
            tgt.data(), max_recommendations, exclude_offsets ? ex_off.data() : nullptr, exclude_offsets ? ex_ids.data() : nullptr,
            oid.data(), osc.data(), ocnt.data(), nullptr));
        for (int64_t j = 0; j < n; ++j) {
            std::copy(oid.begin() + j * N, oid.begin() + (j + 1) * N, out_place_ids + vis[j] * N);
            std::copy(osc.begin() + j * N, osc.begin() + (j + 1) * N, out_estimated_ratings + vis[j] * N);
            out_counts[vis[j]] = ocnt[(size_t)j];
        }
        return LOCREC_OK;
    };
    return knn_pool_visitors_each_delegated(pool, call, v, ranked);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_pool_visitors_stats(int64_t out[12])
{
    if (!out) return fail(LOCREC_E_INVALID_ARG, "NULL argument");
    const locrec::KnnPoolVisitorsStats &st = locrec::knn_pool_visitors_stats();
    out[0] = st.waves;
    out[1] = st.member_tiles;
    out[2] = st.stage_launches;
    out[3] = st.fill_launches;
    out[4] = st.scan_launches;
    out[5] = st.aggregate_launches;
    out[6] = st.finish_launches;
    out[7] = st.delegated_members;
    out[8] = st.beyond;
    out[9] = st.emitted_rows;
    out[10] = st.readback_bytes;
    out[11] = st.host_syncs;
    return LOCREC_OK;
}
