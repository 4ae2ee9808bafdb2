// rank_batch.h -- the segmented ranker's internal entry (rank_batch.hip): "places of the target region, top N by
// score" for many row ranges of one device-resident (ids, scores) pair at once.  locrec_rank_recommendations_batch
// and the ranked KNN batches call it; every pointer is a device pointer of the current device.
#pragma once

#include <algorithm>
#include <vector>

#include "common.h"

namespace locrec {

// what the last ranking of this thread did (locrec_rank_recommendations_batch_stats)
struct RankBatchStats {
    int64_t one_block = 0;        // segments one block served from its LDS list
    int64_t split = 0;            // segments cut into chunks and merged
    int64_t chunks = 0;           // chunks of the split segments
    int64_t sorted = 0;           // segments the global radix sort served
    int64_t membership_form = 0;  // 0: binary search in the (region, place id) table (the only form)
    int64_t host_assembled = 0;   // segments whose rows the host assembled and uploaded
    int64_t host_syncs = 0;       // explicit stream synchronisations of the call (the hipFree of a work buffer waits too)
};
RankBatchStats &rank_batch_stats();

// Segment s is rows [seg_begin[s], seg_begin[s] + seg_len[s]) of ids / scores (0 <= seg_len[s] < 2^31; checked on the
// device before any row is read, with *invalid_flag - when given - as one more reason to refuse: LOCREC_E_INVALID_ARG
// and nothing written).  Row s of out_ids / out_scores (stride max_recommendations > 0) gets the segment's ranking,
// padded with id -1 and score 0.0; out_counts[s] the rows written.  The call waits for the stream twice at the most
// (host_syncs) and frees its call-local work buffers at the end, each hipFree a wait of its own.
int32_t rank_segments_device(int64_t n_segments, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                             const double *scores, int64_t n_places, const int64_t *place_ids,
                             const int64_t *place_region_ids, const int64_t *target_region_ids, int64_t max_recommendations,
                             int64_t *out_ids, double *out_scores, int64_t *out_counts,
                             const unsigned long long *invalid_flag, int64_t host_assembled, hipStream_t s);

// The same with a list of ids per segment to leave out: segment s ranks its rows whose id is none of
// ex_ids[ex_begin[s] .. ex_begin[s] + ex_len[s]) (int64 equality; a list may be unsorted, repeat an id and name ids the
// segment lacks; lists may overlap or be one range for several segments).  Begin / length and not offsets, so that a
// caller can point into an array that is already resident: the KNN calls into the index's rating rows, an SG group into
// the sub-range of its segments.  0 <= ex_len[s], 0 <= ex_begin[s], ex_begin[s] + ex_len[s] <= n_excluded < 2^31, checked
// on the device with the segments, before anything reads through them.  The kept rows stay in their input order, so
// the ties fall as in the plain entry; with every list empty the result and the stats are the plain entry's, and the
// waits are no more in any case.
int32_t rank_segments_device_excluding(int64_t n_segments, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                                       const double *scores, int64_t n_places, const int64_t *place_ids,
                                       const int64_t *place_region_ids, const int64_t *target_region_ids,
                                       int64_t max_recommendations, const int64_t *ex_begin, const int64_t *ex_len,
                                       int64_t n_excluded, const int64_t *ex_ids, int64_t *out_ids, double *out_scores,
                                       int64_t *out_counts, const unsigned long long *invalid_flag, int64_t host_assembled,
                                       hipStream_t s);

// the exclusion lists of one ranker call (begin NULL: none, the plain entry)
struct RankExclude {
    const int64_t *begin = nullptr, *len = nullptr, *ids = nullptr;
    int64_t n = 0;
};

// the circles of one ranker call (center_lat NULL: none): per segment a centre in degrees and a radius in metres, per
// row of the place table its coordinates
struct RankNear {
    const double *center_lat = nullptr, *center_lon = nullptr, *radius = nullptr, *place_lat = nullptr, *place_lon = nullptr;
};

// "Within reach": the same with a circle per segment, and lists only when ex.begin is given.  Segment s keeps a row iff
// its id is a place of the target region and some listing of that place in that region lies within radius[s] metres of
// the centre - distance_meters (place_grid.h) <= radius, +inf keeping every place.  out_meters (NULL: not wanted; the
// shape of out_scores) gets the distance of the first such listing in the table's input order, padding 0.0.  A radius
// that is NaN or negative, or a centre or a place row outside Location's ranges, is refused with the segments in the
// plan step, before any row is read.  With near.center_lat NULL this is the plain / excluding entry.
int32_t rank_segments_device_near(int64_t n_segments, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                                  const double *scores, int64_t n_places, const int64_t *place_ids,
                                  const int64_t *place_region_ids, const int64_t *target_region_ids, int64_t max_recommendations,
                                  const RankExclude &ex, const RankNear &near, int64_t *out_ids, double *out_scores,
                                  double *out_meters, int64_t *out_counts, const unsigned long long *invalid_flag,
                                  int64_t host_assembled, hipStream_t s);

// the same requires for host arrays, before any device work (the public entries and the KNN / SG near calls)
int32_t rank_near_check_host(int64_t n_segments, const double *center_lat, const double *center_lon, const double *radius,
                             int64_t n_places, const double *place_lat, const double *place_lon);

// the categories of one ranker call (place_cat NULL: none): per row of the place table its category, per segment an
// allow-list allow_ids[allow_begin[s] .. + allow_len[s]) in the mould of the exclusion lists (allow_begin NULL: no
// lists; an empty list allows every category) and a cap on the rows of one category (caps NULL: no caps)
struct RankCategory {
    const int64_t *place_cat = nullptr, *allow_begin = nullptr, *allow_len = nullptr, *allow_ids = nullptr;
    int64_t n_allowed = 0;
    const int64_t *caps = nullptr;
    // (the public entry's second validity word: its allowed_offsets broke the offset rules)
    const unsigned long long *allow_invalid = nullptr;
};

// "By category": the same with an allow-list and a cap per segment, circles only when near.center_lat is given and
// exclusion lists only when ex.begin is.  A listing of a place in the target region passes if its category is in the
// segment's list (no list, or an empty one: any) and it lies inside the circle; the first passing listing in the
// table's input order is the one that counts: its category is the row's for the cap, its distance the row's
// out_meters.  A row is eligible iff fewer than caps[s] kept rows of its category precede it in the order (score desc,
// id asc, input row asc); the output is the first max_recommendations eligible rows.  caps[s] >= 1, checked with the
// lists' ranges in the plan step.  With no list entry and every cap >= max_recommendations the existing kernels run
// and the result and the stats are the plain / excluding / near entry's.
int32_t rank_segments_device_by_category(int64_t n_segments, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                                         const double *scores, int64_t n_places, const int64_t *place_ids,
                                         const int64_t *place_region_ids, const int64_t *target_region_ids,
                                         int64_t max_recommendations, const RankExclude &ex, const RankNear &near,
                                         const RankCategory &cat, int64_t *out_ids, double *out_scores, double *out_meters,
                                         int64_t *out_counts, const unsigned long long *invalid_flag, int64_t host_assembled,
                                         hipStream_t s);

// the lists' and caps' requires for host arrays, before any device work: allow_offsets NULL: no lists, caps NULL: none
int32_t rank_category_check_host(int64_t n_segments, const int64_t *allowed_offsets, int64_t n_allowed, const int64_t *caps);

// The categories of a KNN / SG call, host arrays as the public entry takes them (allowed_offsets NULL: no lists, caps NULL:
// no caps, both NULL: none).  Its words lie behind a RankIo's inputs:
//   [place categories | begins | lengths | caps | listed categories]   (a second call of the same request - the KNN calls'
// host-assembled segments, an SG group - shares the first one's place categories and listed categories: table_of)
struct RankCatHost {
    const int64_t *place_cat = nullptr, *allowed_offsets = nullptr;
    int64_t n_allowed = 0;
    const int64_t *allowed_ids = nullptr, *caps = nullptr;
    bool given() const { return allowed_offsets || caps; }
    // the requires of the public entry, before any device work
    int32_t check(int64_t n_segments, int64_t n_places) const
    {
        if (!given()) return LOCREC_OK;
        if (allowed_offsets && (n_allowed < 0 || n_allowed >= ((int64_t)1 << 31)))
            return fail(LOCREC_E_INVALID_ARG, "n_allowed out of range [0, 2^31)");
        if (allowed_offsets && n_allowed > 0 && !allowed_ids) return fail(LOCREC_E_INVALID_ARG, "allowed_category_ids is NULL with n_allowed > 0");
        if (n_places > 0 && !place_cat) return fail(LOCREC_E_INVALID_ARG, "place_category_ids is NULL with allow-lists or caps given");
        return rank_category_check_host(n_segments, allowed_offsets, n_allowed, caps);
    }
    size_t words(int64_t n_places, int64_t nseg, bool with_tables) const
    {
        if (!given()) return 0;
        return 3 * (size_t)nseg + (with_tables ? (size_t)n_places + (size_t)(allowed_offsets ? n_allowed : 0) : 0);
    }
    // Fills the words at `at` for the call's segments seg[0 .. nseg) of the request (seg NULL: 0 .. nseg) -> the ranker's
    // block.  stage: host staging of the copies, the caller's until the stream has been waited for.
    int32_t upload(int64_t n_places, int64_t nseg, const int64_t *seg, int64_t *at, const RankCategory *table_of, hipStream_t s,
                   std::vector<int64_t> &stage, RankCategory &out) const
    {
        out = RankCategory();
        if (!given()) return LOCREC_OK;
        int64_t *begin = at, *len = at + nseg, *cap = at + 2 * nseg, *tables = at + 3 * nseg;
        stage.assign(3 * (size_t)nseg, 0);
        for (int64_t c = 0; c < nseg; ++c) {
            const int64_t g = seg ? seg[c] : c;
            stage[(size_t)c] = allowed_offsets ? allowed_offsets[g] : 0;
            stage[(size_t)(nseg + c)] = allowed_offsets ? allowed_offsets[g + 1] - allowed_offsets[g] : 0;
            stage[(size_t)(2 * nseg + c)] = caps ? caps[g] : 0;
        }
        LOCREC_HIP_TRY(hipMemcpyAsync(at, stage.data(), 3 * (size_t)nseg * 8, hipMemcpyHostToDevice, s));
        if (table_of) {
            out.place_cat = table_of->place_cat;
            out.allow_ids = table_of->allow_ids;
        } else {
            if (n_places > 0) LOCREC_HIP_TRY(hipMemcpyAsync(tables, place_cat, (size_t)n_places * 8, hipMemcpyHostToDevice, s));
            if (allowed_offsets && n_allowed > 0)
                LOCREC_HIP_TRY(hipMemcpyAsync(tables + n_places, allowed_ids, (size_t)n_allowed * 8, hipMemcpyHostToDevice, s));
            out.place_cat = tables;
            out.allow_ids = tables + n_places;
        }
        if (allowed_offsets) {
            out.allow_begin = begin;
            out.allow_len = len;
            out.n_allowed = n_allowed;
        }
        if (caps) out.caps = cap;
        return LOCREC_OK;
    }
};

// One ranker call's device arrays, carved out of one input and one output allocation of 8-byte words:
//   in   [place ids | place regions | targets | bases | lengths]   (without the places table when it is places_of's)
//   out  [ids | scores | counts]
// The caller fills `in` (in one copy or several) and brings the rows; the ranking, its read-back and the scatter are here.
struct RankIo {
    int64_t n_places, nseg, N;
    int64_t *pid, *preg, *tgt, *base, *len, *oid, *ocnt;
    double *osc;
    // with circles (near): [... | lengths | centre lat | centre lon | radius | place lat | place lon] (again without the
    // places' words when they are places_of's) and [ids | scores | counts | meters]
    bool near = false;
    double *clat = nullptr, *clon = nullptr, *rad = nullptr, *plat = nullptr, *plon = nullptr, *omet = nullptr;
    static size_t in_words(int64_t n_places, int64_t nseg, bool near = false)
    {
        return (near ? 4 : 2) * (size_t)n_places + (near ? 6 : 3) * (size_t)nseg;
    }
    static size_t out_words(int64_t nseg, int64_t N, bool near = false) { return (near ? 3 : 2) * (size_t)(nseg * N) + (size_t)nseg; }
    RankIo(int64_t *in, int64_t *out, int64_t n_places_, int64_t nseg_, int64_t N_, const RankIo *places_of = nullptr,
           bool near_ = false)
        : n_places(n_places_), nseg(nseg_), N(N_), pid(places_of ? places_of->pid : in), preg(places_of ? places_of->preg : in + n_places),
          tgt(places_of ? in : in + 2 * n_places), base(tgt + nseg), len(base + nseg), oid(out), ocnt(out + 2 * nseg * N),
          osc(reinterpret_cast<double *>(out + nseg * N)), near(near_)
    {
        if (!near) return;
        clat = reinterpret_cast<double *>(len + nseg);
        clon = clat + nseg;
        rad = clon + nseg;
        plat = places_of ? places_of->plat : rad + nseg;
        plon = places_of ? places_of->plon : plat + n_places;
        omet = reinterpret_cast<double *>(ocnt + nseg);
    }
    // by category: the block RankCatHost::upload made of the words behind the inputs (nothing given: none)
    RankCategory cat;
    int32_t rank(const int64_t *ids, const double *scores, int64_t host_assembled, hipStream_t s, const RankExclude &ex = {}) const
    {
        if (cat.allow_begin || cat.caps)
            return rank_segments_device_by_category(nseg, base, len, ids, scores, n_places, pid, preg, tgt, N, ex,
                                                    near ? RankNear{clat, clon, rad, plat, plon} : RankNear{}, cat, oid, osc, omet, ocnt,
                                                    nullptr, host_assembled, s);
        if (near)
            return rank_segments_device_near(nseg, base, len, ids, scores, n_places, pid, preg, tgt, N, ex, {clat, clon, rad, plat, plon},
                                             oid, osc, omet, ocnt, nullptr, host_assembled, s);
        if (ex.begin)
            return rank_segments_device_excluding(nseg, base, len, ids, scores, n_places, pid, preg, tgt, N, ex.begin, ex.len, ex.n,
                                                  ex.ids, oid, osc, ocnt, nullptr, host_assembled, s);
        return rank_segments_device(nseg, base, len, ids, scores, n_places, pid, preg, tgt, N, oid, osc, ocnt, nullptr, host_assembled, s);
    }
    // nseg x N ids and scores and nseg counts to host arrays of that shape, then the call's one wait
    int32_t read_back(int64_t *ids, double *scores, int64_t *counts, hipStream_t s, double *meters = nullptr) const
    {
        if (N > 0 && meters) LOCREC_HIP_TRY(hipMemcpyAsync(meters, omet, (size_t)(nseg * N) * 8, hipMemcpyDeviceToHost, s));
        if (N > 0) {
            LOCREC_HIP_TRY(hipMemcpyAsync(ids, oid, (size_t)(nseg * N) * 8, hipMemcpyDeviceToHost, s));
            LOCREC_HIP_TRY(hipMemcpyAsync(scores, osc, (size_t)(nseg * N) * 8, hipMemcpyDeviceToHost, s));
        }
        LOCREC_HIP_TRY(hipMemcpyAsync(counts, ocnt, (size_t)nseg * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        return LOCREC_OK;
    }
    // the same, segment c's N rows and count going to position to[c] of the caller's arrays
    int32_t read_back_to(const std::vector<int64_t> &to, int64_t *ids, double *scores, int64_t *counts, hipStream_t s,
                         double *meters = nullptr) const
    {
        std::vector<int64_t> hid((size_t)(nseg * N)), hcnt((size_t)nseg);
        std::vector<double> hsc((size_t)(nseg * N)), hmet(meters ? (size_t)(nseg * N) : 0);
        LOCREC_TRY(read_back(hid.data(), hsc.data(), hcnt.data(), s, meters ? hmet.data() : nullptr));
        for (int64_t c = 0; c < nseg; ++c) {
            if (meters) std::copy(hmet.begin() + c * N, hmet.begin() + (c + 1) * N, meters + to[(size_t)c] * N);
            std::copy(hid.begin() + c * N, hid.begin() + (c + 1) * N, ids + to[(size_t)c] * N);
            std::copy(hsc.begin() + c * N, hsc.begin() + (c + 1) * N, scores + to[(size_t)c] * N);
            counts[to[(size_t)c]] = hcnt[(size_t)c];
        }
        return LOCREC_OK;
    }
};

}  // namespace locrec
