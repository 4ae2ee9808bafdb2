// knn_ranked.h -- the ranked KNN batches (included by knn_batch.hip behind knn.hip): the rows a batched
// makeRecommendations left on the device are ranked where they are by the segmented ranker (rank_batch.h), and only
// max_recommendations rows a person travel to the host.  Two resident forms:
//   [nq x agg_M] agg_place / agg_est with agg_n    K <= LOCREC_KNN_BATCH_MAX_K (enqueue_aggregate)
//   lkb_place / lkb_est with lkb_off               every other K (knn_large.hip)
// The sizes come from locrec_knn_fetch_recommend itself, called for the offsets only (by locrec_knn_recommend_batch in
// the batch form, here in the range form): that call carries the redo after a survivor-queue overflow, so the rows are
// settled when it returns.  Queries whose aggregation overflowed its block (agg_overflow) have no resident rows:
// knn_large_recommend assembles them on the host, as the row fetch does - in one pass, their row counts being known
// from the fetch - and they are uploaded and ranked as segments of a second ranker call (counted as host-assembled in
// the stats).  (The fetch's own count-and-discard passes over those queries stay as they are: locrec_knn_fetch_recommend.)
// The unvisited forms (locrec_knn_recommend_ranked_batch_unvisited, locrec_knn_fetch_ranked_unvisited) recommend only new
// places: both ranker calls get, per segment, the place ids of the person's rating rows as an exclusion list - begins and
// lengths into ix->r_place, filled on the device from ix->r_ptr (knn_rk_rated_ranges, 8 VGPRs, no LDS, no scratch).
// The near form (locrec_knn_recommend_ranked_batch_near) recommends within reach: per position a centre and a radius, per
// place row its coordinates, uploaded behind the RankIo's other inputs; both ranker calls are the near ranker's
// (rank_segments_device_near), the hosted segments taking their positions' circles, and out_meters comes back with the
// rows.  Its host arrays are checked before the index is looked at.
// The by-category form (locrec_knn_recommend_ranked_batch_by_category) adds an allow-list of categories and a cap per
// category to every position, with the circles optional: the place categories, the lists and the caps are uploaded
// behind the other inputs (RankCatHost), both ranker calls are rank_segments_device_by_category, and the hosted
// segments take their positions' lists and caps.
#pragma once

#include "rank_batch.h"

namespace {

// the ranked calls' own arguments (the pool's entry checks them before any device work)
int32_t knn_rank_check_args(int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids, const int64_t *targets,
                            int64_t N, const int64_t *out_ids, const double *out_scores, const int64_t *out_counts)
{
    if (n_places < 0 || n_places >= ((int64_t)1 << 31)) return fail(LOCREC_E_INVALID_ARG, "place count out of range [0, 2^31)");
    if (!out_counts || !targets || (N > 0 && (!out_ids || !out_scores)) || (n_places > 0 && (!place_ids || !place_region_ids)))
        return fail(LOCREC_E_INVALID_ARG, "NULL argument");
    return LOCREC_OK;
}

// The unvisited forms' exclusion lists, read where they lie: segment c's list is the place ids of the rating rows the
// index holds for internal row rows[c] - r_place[r_ptr[row] .. r_ptr[row + 1]) - so the ranker gets begins and lengths
// into r_place itself.  No gather, no length travels to the host.
__global__ void knn_rk_rated_ranges(int64_t nseg, const int32_t *__restrict__ rows, const int64_t *__restrict__ r_ptr,
                                    int64_t *__restrict__ ex_begin, int64_t *__restrict__ ex_len)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nseg) return;
    const int64_t b = r_ptr[rows[c]];
    ex_begin[c] = b;
    ex_len[c] = r_ptr[rows[c] + 1] - b;
}

// words behind a RankIo's inputs for the lists of nseg segments: begins, lengths, the rows (int32)
inline size_t knn_rk_ex_words(int64_t nseg) { return 2 * (size_t)nseg + ((size_t)nseg + 1) / 2; }

// fills them at `at` for the segments' internal rows (all < ix->n) -> the ranker's lists
int32_t knn_rk_rated_lists(locrec_knn_index *ix, const std::vector<int32_t> &rows, int64_t *at, hipStream_t s, RankExclude &ex)
{
    const int64_t nseg = (int64_t)rows.size();
    int32_t *d_rows = reinterpret_cast<int32_t *>(at + 2 * nseg);
    LOCREC_HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), (size_t)nseg * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(knn_rk_rated_ranges, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, s, nseg, d_rows, ix->r_ptr.p, at,
                       at + nseg);
    LOCREC_HIP_TRY(hipGetLastError());
    ex.begin = at;
    ex.len = at + nseg;
    ex.ids = ix->r_place.p;
    ex.n = (int64_t)ix->r_place.n;
    return LOCREC_OK;
}

// The circles of a near call (host arrays): per row of the place table its coordinates, per segment a centre and a
// radius; meters: the output rows' distances (NULL: not wanted).  The near entry has checked them.
struct KnnRankNear {
    const double *place_lat, *place_lon, *center_lat, *center_lon, *radius;
    double *meters;
};

// segment c of the result = the resident rows of processing slot slots[c], ranked for targets[c] (host arrays).
// known_len: the segments' row counts where the caller has them from a fetch that already settled the rows (the batch
// form: locrec_knn_recommend_batch sizes its result through locrec_knn_fetch_recommend); NULL: that fetch is made here.
// unvisited: every segment leaves out the places its person has rated (both ranker calls get the lists).
// near: every segment keeps only the places inside its circle (both ranker calls are the near ranker's).
int32_t knn_rank_resident(locrec_knn_index *ix, const std::vector<int64_t> &slots, const int64_t *known_len, bool unvisited,
                          int64_t n_places,
                          const int64_t *place_ids, const int64_t *place_region_ids, const int64_t *targets,
                          int64_t max_recommendations, int64_t *out_ids, double *out_scores, int64_t *out_counts,
                          const KnnRankNear *near = nullptr, const RankCatHost *catq = nullptr)
{
    const int64_t nseg = (int64_t)slots.size(), nq = ix->last_nq;
    const int64_t N = std::max<int64_t>(0, max_recommendations);
    LOCREC_TRY(knn_rank_check_args(n_places, place_ids, place_region_ids, targets, N, out_ids, out_scores, out_counts));
    std::vector<int64_t> off((size_t)nq + 1, 0);
    if (!known_len) {
        int64_t cap = 0;
        LOCREC_TRY(locrec_knn_fetch_recommend(ix, nq, off.data(), nullptr, nullptr, &cap));  // sizes only; settles the rows
    }
    LOCREC_HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = ix->stream;
    const bool lkb = ix->have_lkb;
    std::vector<int32_t> ovf((size_t)nq, 0);
    if (!lkb) {
        LOCREC_HIP_TRY(hipMemcpyAsync(ovf.data(), ix->agg_overflow.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
    }
    std::vector<int64_t> hb((size_t)nseg), hl((size_t)nseg), hosted;
    for (int64_t c = 0; c < nseg; ++c) {
        const int64_t q = slots[(size_t)c];
        const int64_t len = known_len ? known_len[c] : off[(size_t)q + 1] - off[(size_t)q];
        hl[(size_t)c] = len;
        if (ovf[(size_t)q]) {
            hb[(size_t)c] = 0;
            hosted.push_back(c);
        } else {
            hb[(size_t)c] = lkb ? ix->lkb_off[(size_t)q] : q * (int64_t)ix->agg_M;
        }
    }
    std::vector<int64_t> host_len;  // of the host-assembled segments, known from the fetch
    for (int64_t c : hosted) {
        host_len.push_back(hl[(size_t)c]);
        hl[(size_t)c] = 0;
    }
    std::fill(out_counts, out_counts + nseg, 0);
    if (nseg == 0) return LOCREC_OK;
    // one allocation for the call's inputs and one for its outputs (every hipMalloc / hipFree costs a wait)
    DevBuf<int64_t> d_in, d_out;
    const bool circ = near != nullptr;
    const RankCatHost none;
    const RankCatHost &cth = catq ? *catq : none;
    const size_t ex_at = RankIo::in_words(n_places, nseg, circ), cat_at = ex_at + (unvisited ? knn_rk_ex_words(nseg) : 0);
    LOCREC_TRY(d_in.alloc(cat_at + cth.words(n_places, nseg, true)));
    LOCREC_TRY(d_out.alloc(RankIo::out_words(nseg, N, circ)));
    RankIo io(d_in.p, d_out.p, n_places, nseg, N, nullptr, circ);
    std::vector<int64_t> cat_stage, hcat_stage;
    LOCREC_TRY(cth.upload(n_places, nseg, nullptr, d_in.p + cat_at, nullptr, s, cat_stage, io.cat));
    if (circ) {
        if (n_places > 0) {
            LOCREC_HIP_TRY(hipMemcpyAsync(io.plat, near->place_lat, (size_t)n_places * 8, hipMemcpyHostToDevice, s));
            LOCREC_HIP_TRY(hipMemcpyAsync(io.plon, near->place_lon, (size_t)n_places * 8, hipMemcpyHostToDevice, s));
        }
        LOCREC_HIP_TRY(hipMemcpyAsync(io.clat, near->center_lat, (size_t)nseg * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(io.clon, near->center_lon, (size_t)nseg * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(io.rad, near->radius, (size_t)nseg * 8, hipMemcpyHostToDevice, s));
    }
    if (n_places > 0) {
        LOCREC_HIP_TRY(hipMemcpyAsync(io.pid, place_ids, (size_t)n_places * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(io.preg, place_region_ids, (size_t)n_places * 8, hipMemcpyHostToDevice, s));
    }
    LOCREC_HIP_TRY(hipMemcpyAsync(io.tgt, targets, (size_t)nseg * 8, hipMemcpyHostToDevice, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(io.base, hb.data(), (size_t)nseg * 8, hipMemcpyHostToDevice, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(io.len, hl.data(), (size_t)nseg * 8, hipMemcpyHostToDevice, s));
    auto row_of_slot = [&](int64_t q) { return ix->agg_rows.empty() ? ix->agg_first + (int32_t)q : ix->agg_rows[(size_t)q]; };
    RankExclude ex;
    if (unvisited) {
        std::vector<int32_t> rows((size_t)nseg);
        for (int64_t c = 0; c < nseg; ++c) rows[(size_t)c] = row_of_slot(slots[(size_t)c]);
        LOCREC_TRY(knn_rk_rated_lists(ix, rows, d_in.p + ex_at, s, ex));
    }
    LOCREC_TRY(io.rank(lkb ? ix->lkb_place.p : ix->agg_place.p, lkb ? ix->lkb_est.p : ix->agg_est.p, 0, s, ex));
    LOCREC_TRY(io.read_back(out_ids, out_scores, out_counts, s, circ ? near->meters : nullptr));
    RankBatchStats total = rank_batch_stats();
    ++total.host_syncs;
    if (!hosted.empty()) {
        // rows of the overflow queries: assembled on the host once per slot, uploaded, ranked as their own segments
        const int64_t nh = (int64_t)hosted.size();
        std::vector<int64_t> rp, tb((size_t)nh), tl((size_t)nh), tt((size_t)nh);
        std::vector<double> re, tc(circ ? 3 * (size_t)nh : 0);  // tc: the circles of the hosted segments
        std::vector<int64_t> slot_begin((size_t)nq, -1), slot_len((size_t)nq, 0);
        for (int64_t i = 0; i < nh; ++i) {
            const int64_t q = slots[(size_t)hosted[(size_t)i]];
            if (slot_begin[(size_t)q] < 0) {
                const int32_t row = row_of_slot(q);
                int64_t c = host_len[(size_t)i];  // one pass: the fetch has counted the rows
                const size_t at = rp.size();
                rp.resize(at + (size_t)c);
                re.resize(at + (size_t)c);
                LOCREC_TRY(knn_large_recommend(ix, row, ix->agg_pw, ix->agg_cw, ix->last_k, rp.data() + at, re.data() + at, &c));
                if (c != host_len[(size_t)i]) return fail(LOCREC_E_DEVICE, "internal: an overflow query changed its row count");
                slot_begin[(size_t)q] = (int64_t)at;
                slot_len[(size_t)q] = c;
            }
            tb[(size_t)i] = slot_begin[(size_t)q];
            tl[(size_t)i] = slot_len[(size_t)q];
            tt[(size_t)i] = targets[hosted[(size_t)i]];
            if (circ) {
                tc[(size_t)i] = near->center_lat[hosted[(size_t)i]];
                tc[(size_t)(nh + i)] = near->center_lon[hosted[(size_t)i]];
                tc[(size_t)(2 * nh + i)] = near->radius[hosted[(size_t)i]];
            }
        }
        DevBuf<int64_t> d_rp, d_hin, d_hout;
        DevBuf<double> d_re;
        LOCREC_TRY(d_rp.upload(rp, s));
        LOCREC_TRY(d_re.upload(re, s));
        const size_t hex_at = RankIo::in_words(0, nh, circ), hcat_at = hex_at + (unvisited ? knn_rk_ex_words(nh) : 0);
        LOCREC_TRY(d_hin.alloc(hcat_at + cth.words(n_places, nh, false)));
        LOCREC_TRY(d_hout.alloc(RankIo::out_words(nh, N, circ)));
        RankIo hio(d_hin.p, d_hout.p, n_places, nh, N, &io, circ);  // (the places table is already there)
        LOCREC_TRY(cth.upload(n_places, nh, hosted.data(), d_hin.p + hcat_at, &io.cat, s, hcat_stage, hio.cat));
        if (circ) LOCREC_HIP_TRY(hipMemcpyAsync(hio.clat, tc.data(), 3 * (size_t)nh * 8, hipMemcpyHostToDevice, s));  // (lat | lon | radius)
        LOCREC_HIP_TRY(hipMemcpyAsync(hio.tgt, tt.data(), (size_t)nh * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(hio.base, tb.data(), (size_t)nh * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(hio.len, tl.data(), (size_t)nh * 8, hipMemcpyHostToDevice, s));
        RankExclude hex;
        if (unvisited) {
            std::vector<int32_t> rows((size_t)nh);
            for (int64_t i = 0; i < nh; ++i) rows[(size_t)i] = row_of_slot(slots[(size_t)hosted[(size_t)i]]);
            LOCREC_TRY(knn_rk_rated_lists(ix, rows, d_hin.p + hex_at, s, hex));
        }
        LOCREC_TRY(hio.rank(d_rp.p, d_re.p, nh, s, hex));
        LOCREC_TRY(hio.read_back_to(hosted, out_ids, out_scores, out_counts, s, circ ? near->meters : nullptr));
        const RankBatchStats &h = rank_batch_stats();
        // (the overflow queries were empty one-block segments of the first call: counted where their rows were ranked)
        if (!h.sorted) {
            total.one_block += h.one_block - nh;
            total.split += h.split;
            total.chunks += h.chunks;
        }
        total.host_assembled = nh;
        total.host_syncs += h.host_syncs + 1;
    }
    rank_batch_stats() = total;
    return LOCREC_OK;
}

}  // namespace

namespace {

int32_t knn_fetch_ranked(locrec_knn_index *ix, int64_t nq, bool unvisited, int64_t n_places, const int64_t *place_ids,
                         const int64_t *place_region_ids, const int64_t *target_region_ids, int64_t max_recommendations,
                         int64_t *out_place_ids, double *out_estimated_ratings, int64_t *out_counts)
{
    if (!ix) return fail(LOCREC_E_INVALID_ARG, "index is NULL");
    if (nq != ix->last_nq || nq <= 0 || !(ix->have_lkb || (ix->have_agg && ix->have_result)))
        return fail(LOCREC_E_INVALID_ARG, "no matching batched recommendation to fetch");
    std::vector<int64_t> slots((size_t)nq);
    std::iota(slots.begin(), slots.end(), (int64_t)0);
    return knn_rank_resident(ix, slots, nullptr, unvisited, n_places, place_ids, place_region_ids, target_region_ids,
                             max_recommendations, out_place_ids, out_estimated_ratings, out_counts);
}

int32_t knn_recommend_ranked_batch(locrec_knn_index *ix, int64_t nq, const int64_t *person_ids, double pw, double cw, int64_t k,
                                   bool unvisited, int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
                                   const int64_t *target_region_ids, int64_t max_recommendations, int64_t *out_place_ids,
                                   double *out_estimated_ratings, int64_t *out_counts, const KnnRankNear *near = nullptr,
                                   const RankCatHost *catq = nullptr)
{
    // the batch itself, with its requires and "No such person": the rows stay on the device (capacity 0: sizes only)
    std::vector<int64_t> off((size_t)std::max<int64_t>(nq, 0) + 1, 0);
    int64_t cap = 0;
    LOCREC_TRY(locrec_knn_recommend_batch(ix, nq, person_ids, pw, cw, k, off.data(), nullptr, nullptr, &cap));
    if (nq == 0) return LOCREC_OK;
    // the caller's order: every person's segment is the processing slot that holds its row (a repeated person: the same)
    std::vector<std::pair<int32_t, int64_t>> by_row((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) by_row[(size_t)i] = {ix->agg_rows[(size_t)i], i};
    std::sort(by_row.begin(), by_row.end());
    std::vector<int64_t> slots((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) {
        int32_t row = 0;
        LOCREC_TRY(find_query_row(ix, person_ids[i], &row));
        slots[(size_t)i] = std::lower_bound(by_row.begin(), by_row.end(), std::make_pair(row, (int64_t)-1))->second;
    }
    std::vector<int64_t> len((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) len[(size_t)i] = off[(size_t)i + 1] - off[(size_t)i];
    return knn_rank_resident(ix, slots, len.data(), unvisited, n_places, place_ids, place_region_ids, target_region_ids,
                             max_recommendations, out_place_ids, out_estimated_ratings, out_counts, near, catq);
}

}  // namespace

extern "C" int32_t locrec_knn_fetch_ranked(locrec_knn_index *ix, int64_t nq, int64_t n_places, const int64_t *place_ids,
                                           const int64_t *place_region_ids, const int64_t *target_region_ids,
                                           int64_t max_recommendations, int64_t *out_place_ids, double *out_estimated_ratings,
                                           int64_t *out_counts) try
{
    return knn_fetch_ranked(ix, nq, false, n_places, place_ids, place_region_ids, target_region_ids, max_recommendations,
                            out_place_ids, out_estimated_ratings, out_counts);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_fetch_ranked_unvisited(locrec_knn_index *ix, int64_t nq, int64_t n_places, const int64_t *place_ids,
                                                     const int64_t *place_region_ids, const int64_t *target_region_ids,
                                                     int64_t max_recommendations, int64_t *out_place_ids,
                                                     double *out_estimated_ratings, int64_t *out_counts) try
{
    return knn_fetch_ranked(ix, nq, true, n_places, place_ids, place_region_ids, target_region_ids, max_recommendations,
                            out_place_ids, out_estimated_ratings, out_counts);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_recommend_ranked_batch(locrec_knn_index *ix, int64_t nq, const int64_t *person_ids, double pw,
                                                     double cw, int64_t k, int64_t n_places, const int64_t *place_ids,
                                                     const int64_t *place_region_ids, const int64_t *target_region_ids,
                                                     int64_t max_recommendations, int64_t *out_place_ids,
                                                     double *out_estimated_ratings, int64_t *out_counts) try
{
    return knn_recommend_ranked_batch(ix, nq, person_ids, pw, cw, k, false, n_places, place_ids, place_region_ids,
                                      target_region_ids, max_recommendations, out_place_ids, out_estimated_ratings, out_counts);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_recommend_ranked_batch_unvisited(locrec_knn_index *ix, int64_t nq, const int64_t *person_ids,
                                                               double pw, double cw, int64_t k, int64_t n_places,
                                                               const int64_t *place_ids, const int64_t *place_region_ids,
                                                               const int64_t *target_region_ids, int64_t max_recommendations,
                                                               int64_t *out_place_ids, double *out_estimated_ratings,
                                                               int64_t *out_counts) try
{
    return knn_recommend_ranked_batch(ix, nq, person_ids, pw, cw, k, true, n_places, place_ids, place_region_ids,
                                      target_region_ids, max_recommendations, out_place_ids, out_estimated_ratings, out_counts);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_recommend_ranked_batch_near(
    locrec_knn_index *ix, int64_t nq, const int64_t *person_ids, double pw, double cw, int64_t k, int64_t n_places,
    const int64_t *place_ids, const int64_t *place_region_ids, const double *place_latitudes, const double *place_longitudes,
    const int64_t *target_region_ids, const double *center_latitudes, const double *center_longitudes, const double *radius_meters,
    int64_t max_recommendations, int32_t unvisited, int64_t *out_place_ids, double *out_estimated_ratings, double *out_meters,
    int64_t *out_counts) try
{
    // the circles' requires first: before the index is looked at
    if (nq < 0 || n_places < 0 || n_places >= ((int64_t)1 << 31)) return fail(LOCREC_E_INVALID_ARG, "query or place count out of range");
    if ((nq > 0 && (!center_latitudes || !center_longitudes || !radius_meters)) || (n_places > 0 && (!place_latitudes || !place_longitudes)))
        return fail(LOCREC_E_INVALID_ARG, "null coordinate or radius array");
    LOCREC_TRY(rank_near_check_host(nq, center_latitudes, center_longitudes, radius_meters, n_places, place_latitudes, place_longitudes));
    const KnnRankNear near = {place_latitudes, place_longitudes, center_latitudes, center_longitudes, radius_meters, out_meters};
    return knn_recommend_ranked_batch(ix, nq, person_ids, pw, cw, k, unvisited != 0, n_places, place_ids, place_region_ids,
                                      target_region_ids, max_recommendations, out_place_ids, out_estimated_ratings, out_counts, &near);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_knn_recommend_ranked_batch_by_category(
    locrec_knn_index *ix, int64_t nq, const int64_t *person_ids, double pw, double cw, int64_t k, int64_t n_places,
    const int64_t *place_ids, const int64_t *place_region_ids, const double *place_latitudes, const double *place_longitudes,
    const int64_t *place_category_ids, const int64_t *target_region_ids, const double *center_latitudes,
    const double *center_longitudes, const double *radius_meters, int64_t max_recommendations, int32_t unvisited,
    const int64_t *allowed_offsets, int64_t n_allowed, const int64_t *allowed_category_ids, const int64_t *max_per_category,
    int64_t *out_place_ids, double *out_estimated_ratings, double *out_meters, int64_t *out_counts) try
{
    // the circles', the lists' and the caps' requires first: before the index is looked at
    if (nq < 0 || n_places < 0 || n_places >= ((int64_t)1 << 31)) return fail(LOCREC_E_INVALID_ARG, "query or place count out of range");
    const bool circles = place_latitudes || place_longitudes || center_latitudes || center_longitudes || radius_meters;
    if (circles) {
        if ((nq > 0 && (!center_latitudes || !center_longitudes || !radius_meters)) || (n_places > 0 && (!place_latitudes || !place_longitudes)))
            return fail(LOCREC_E_INVALID_ARG, "null coordinate or radius array");
        LOCREC_TRY(rank_near_check_host(nq, center_latitudes, center_longitudes, radius_meters, n_places, place_latitudes, place_longitudes));
    }
    RankCatHost cat;
    cat.place_cat = place_category_ids;
    cat.allowed_offsets = allowed_offsets;
    cat.n_allowed = allowed_offsets ? n_allowed : 0;
    cat.allowed_ids = allowed_category_ids;
    cat.caps = max_per_category;
    LOCREC_TRY(cat.check(nq, n_places));
    const KnnRankNear near = {place_latitudes, place_longitudes, center_latitudes, center_longitudes, radius_meters, out_meters};
    return knn_recommend_ranked_batch(ix, nq, person_ids, pw, cw, k, unvisited != 0, n_places, place_ids, place_region_ids,
                                      target_region_ids, max_recommendations, out_place_ids, out_estimated_ratings, out_counts,
                                      circles ? &near : nullptr, &cat);
} LOCREC_CATCH_ALL
