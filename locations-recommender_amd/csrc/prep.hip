// prep.hip -- the producers of the two hot paths' inputs, on the device (SURVEY.md 8f "next" rows):
//
//   f-2  RatingsBuilder.calcRatings              knn/RatingsBuilder.scala:32-48
//        RatingVectorsBuilder.calcRatingVectors  knn/RatingVectorsBuilder.scala:10-25,52-84
//        StochasticGraphBuilder.buildWithBalancedWeights   stochastic/StochasticGraphBuilder.scala:8-28
//   f-4  PlaceVisits.calcPlaceVisits             PlaceVisits.scala:11-46 (+ Location.scala:7-8,30-43)
//   between them, StochasticGraphBuilderMain.generateStochasticGraph's four edge families (:47-66):
//        PersonLikesPlace / PersonLikesCategory / CategorySelectedPlace   stochastic/PersonLikesPlace.scala:12-37
//        PlaceSimilarPlace.calcPlaceSimilarPlaceEdges                      stochastic/PlaceSimilarPlace.scala:18-63
//
// Every function takes either host arrays (copied in and out) or device arrays of the current
// device (mem = LOCREC_MEM_DEVICE): the device form lets visits -> ratings -> rating vectors ->
// locrec_knn_create_from_device run without a host hop.  These are offline, once-per-dataset
// steps: grouping and ranking are keyed rocPRIM radix sorts / scans with small kernels between them
// (as in knn_build.hip); the spatial join replaces the reference's "very inefficient almost
// cross-join" (PlaceVisits.scala:30) with a band / cell grid whose cells are at least one search
// radius wide, so a visit meets only the places of at most 3 x 3 cells, each with the exact
// fp64 haversine of Location.scala.

#include "dev_prims.h"

#include <algorithm>
#include <cmath>
#include <limits>

#include "common.h"
#include "place_grid.h"

namespace {

using namespace locrec;

// ---- sort rows by (person, entity), stable in the input order ------------------------------------

struct SortedRows {
    DevBuf<uint64_t> k0, k1;
    DevBuf<uint32_t> r0, r1;
    const uint32_t *rows = nullptr;  // input row of sorted position i
};

// two stable LSD passes: by entity, then by person
int32_t sort_person_entity(int64_t n, const int64_t *person, const int64_t *entity, SortedRows &S, Temp &tmp, hipStream_t s)
{
    LOCREC_TRY(alloc_each((size_t)n, S.k0, S.k1, S.r0, S.r1));
    LOCREC_LAUNCH(iota_keys, grid_for(n), dim3(256), 0, s, n, entity, S.k0.p, S.r0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, S.k0.p, S.k1.p, S.r0.p, S.r1.p, (int)n, 0, 64, s));
    LOCREC_LAUNCH(gather_id_keys, grid_for(n), dim3(256), 0, s, n, person, S.r1.p, S.k0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, S.k0.p, S.k1.p, S.r1.p, S.r0.p, (int)n, 0, 64, s));
    S.rows = S.r0.p;
    return LOCREC_OK;
}

// ---- calcRatings and the counted edge families -----------------------------------------------------

// flags of the sorted rows: a new (person, entity) group / a new person
__global__ void pr_group_flags(int64_t n, const int64_t *person, const int64_t *entity, const uint32_t *rows,
                               unsigned char *gfirst, uint32_t *pfirst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t p = person[rows[i]], e = entity[rows[i]];
    bool np = true, ng = true;
    if (i > 0) {
        const int64_t pp = person[rows[i - 1]], pe = entity[rows[i - 1]];
        np = pp != p;
        ng = np || pe != e;
    }
    gfirst[i] = ng ? 1 : 0;
    pfirst[i] = np ? 1u : 0u;
}

// per group: its visit count and the dense rank of its person (the "source" of the rank step)
__global__ void pr_group_counts(int64_t g, int64_t n, const uint32_t *gstart, const uint32_t *prank_of_pos, uint64_t *cnt,
                                uint32_t *srank)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g) return;
    const uint32_t b = gstart[i];
    const uint32_t e = i + 1 < g ? gstart[i + 1] : (uint32_t)n;
    cnt[i] = e - b;
    srank[i] = prank_of_pos[b] - 1u;
}

// ---- the rank step every counted family shares: rank() over (partition by source order by count desc) <= topN ----
// Groups arrive ordered by (source, target) with the source as a non-decreasing u32 rank.  Counts below 2^32 (visit
// counts: at most n) sort with the source in one 64-bit key; co-visit counts are 64-bit and take two stable passes.

__global__ void pr_rank_keys(int64_t g, const uint32_t *srank, const uint64_t *cnt, uint64_t *keys, uint32_t *gid)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g) return;
    keys[i] = ((uint64_t)srank[i] << 32) | (uint32_t)(~(uint32_t)cnt[i]);
    gid[i] = (uint32_t)i;
}

__global__ void pr_rank_keys_wide(int64_t g, const uint64_t *cnt, uint64_t *keys, uint32_t *gid)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g) return;
    keys[i] = ~cnt[i];
    gid[i] = (uint32_t)i;
}

__global__ void pr_rank_source_keys(int64_t g, const uint32_t *srank, const uint32_t *gid, uint32_t *keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < g) keys[i] = srank[gid[i]];
}

// over the groups sorted by (source, count desc): position of the source's first group and of the
// first group of the run of equal counts (as values for two running maxima); from the packed keys ...
__global__ void pr_run_marks_packed(int64_t g, const uint64_t *keys, uint32_t *pmark, uint32_t *rmark)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g) return;
    const bool np = i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32);
    const bool nr = i == 0 || keys[i] != keys[i - 1];
    pmark[i] = np ? (uint32_t)i : 0u;
    rmark[i] = nr ? (uint32_t)i : 0u;
}

// ... or, where source and 64-bit count do not fit one key, from the groups themselves
__global__ void pr_run_marks(int64_t g, const uint32_t *gid, const uint32_t *srank, const uint64_t *cnt, uint32_t *pmark,
                             uint32_t *rmark)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g) return;
    bool np = true, nr = true;
    if (i > 0) {
        const uint32_t a = gid[i], b = gid[i - 1];
        np = srank[a] != srank[b];
        nr = np || cnt[a] != cnt[b];
    }
    pmark[i] = np ? (uint32_t)i : 0u;
    rmark[i] = nr ? (uint32_t)i : 0u;
}

// SQL rank() = 1 + rows of the partition sorting strictly before = 1 + (first of the run - first of
// the source); where(rank <= topN)
__global__ void pr_keep_top(int64_t g, const uint32_t *pstart, const uint32_t *rstart, const uint32_t *gid, int64_t top_n,
                            uint32_t *keep)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g) return;
    const int64_t rank = 1 + (int64_t)(rstart[i] - pstart[i]);
    keep[gid[i]] = rank <= top_n ? 1u : 0u;
}

// keep[i] = group i survives the rank filter; pos[i] = its output row; *out_count = rows kept
int32_t rank_keep(int64_t g, const uint32_t *srank, const uint64_t *cnt, int64_t top_n, bool wide_counts, uint32_t *keep,
                  uint32_t *pos, int64_t *out_count, Temp &tmp, hipStream_t s)
{
    DevBuf<uint32_t> gid0, gid1, pmark, rmark, pstart, rstart;
    DevBuf<uint64_t> key0, key1;
    LOCREC_TRY(alloc_each((size_t)g, gid0, gid1, key0, key1, pmark, rmark, pstart, rstart));
    const uint32_t *sorted = gid1.p;
    if (!wide_counts) {
        LOCREC_LAUNCH(pr_rank_keys, grid_for(g), dim3(256), 0, s, g, srank, cnt, key0.p, gid0.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, key0.p, key1.p, gid0.p, gid1.p, (int)g, 0, 64, s));
    } else {  // stable LSD: by count descending, then by source (pmark / rmark serve as the 32-bit key buffers)
        LOCREC_LAUNCH(pr_rank_keys_wide, grid_for(g), dim3(256), 0, s, g, cnt, key0.p, gid0.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, key0.p, key1.p, gid0.p, gid1.p, (int)g, 0, 64, s));
        LOCREC_LAUNCH(pr_rank_source_keys, grid_for(g), dim3(256), 0, s, g, srank, gid1.p, pmark.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, pmark.p, rmark.p, gid1.p, gid0.p, (int)g, 0, 32, s));
        sorted = gid0.p;
    }
    if (!wide_counts)
        LOCREC_LAUNCH(pr_run_marks_packed, grid_for(g), dim3(256), 0, s, g, key1.p, pmark.p, rmark.p);
    else
        LOCREC_LAUNCH(pr_run_marks, grid_for(g), dim3(256), 0, s, g, sorted, srank, cnt, pmark.p, rmark.p);
    LOCREC_PRIM(tmp, prim::inclusive_max(p_, bytes_, pmark.p, pstart.p, (int)g, s));
    LOCREC_PRIM(tmp, prim::inclusive_max(p_, bytes_, rmark.p, rstart.p, (int)g, s));
    LOCREC_LAUNCH(pr_keep_top, grid_for(g), dim3(256), 0, s, g, pstart.p, rstart.p, sorted, top_n, keep);
    LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, keep, pos, (int)g, s));
    uint32_t last_pos = 0, last_keep = 0;
    LOCREC_HIP_TRY(hipMemcpyAsync(&last_pos, pos + (g - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&last_keep, keep + (g - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    *out_count = (int64_t)last_pos + last_keep;
    return LOCREC_OK;
}

// groupBy(source).agg(sum(count)) over the KEPT groups (PersonLikesPlace.scala:25-27): totals[source rank]
__global__ void pr_kept_counts(int64_t g, const uint32_t *keep, const uint64_t *cnt, uint64_t *kept)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < g) kept[i] = keep[i] ? cnt[i] : 0ull;
}

int32_t kept_totals(int64_t g, const uint32_t *srank, const uint64_t *cnt, const uint32_t *keep, DevBuf<uint64_t> &totals,
                    Temp &tmp, hipStream_t s)
{
    DevBuf<uint64_t> kept;
    DevBuf<uint32_t> sources, nsources;
    LOCREC_TRY(alloc_each((size_t)g, kept, sources));
    LOCREC_TRY(nsources.alloc(1));
    LOCREC_TRY(totals.alloc((size_t)g));
    LOCREC_LAUNCH(pr_kept_counts, grid_for(g), dim3(256), 0, s, g, keep, cnt, kept.p);
    LOCREC_PRIM(tmp, prim::sum_by_key(p_, bytes_, srank, kept.p, (size_t)g, sources.p, totals.p, nsources.p, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (kept / sources are released on return)
    return LOCREC_OK;
}

// a kept group's row: calcRatings writes the count (out_rating), the edge families the count over the
// source's total of kept counts, as double / double (out_weight)
__global__ void pr_emit_ratings(int64_t g, const uint32_t *keep, const uint32_t *pos, const uint32_t *gstart,
                                const uint32_t *rows, const int64_t *person, const int64_t *entity, const uint64_t *cnt,
                                const uint32_t *srank, const uint64_t *totals, int64_t *out_person, int64_t *out_entity,
                                int64_t *out_rating, double *out_weight)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g || !keep[i]) return;
    const uint32_t r = rows[gstart[i]], at = pos[i];
    out_person[at] = person[r];
    out_entity[at] = entity[r];
    if (out_rating) out_rating[at] = (int64_t)cnt[i];
    if (out_weight) out_weight[at] = (double)cnt[i] / (double)totals[srank[i]];
}

// calcRatings (out_rating) and calcPersonLikesPlaceEdges and its two siblings (out_weight): one body
int32_t calc_ratings(int64_t n, const int64_t *person, const int64_t *entity, int64_t top_n, int64_t *out_person,
                     int64_t *out_entity, int64_t *out_rating, double *out_weight, int64_t *out_count, hipStream_t s)
{
    Temp tmp;
    SortedRows S;
    LOCREC_TRY(sort_person_entity(n, person, entity, S, tmp, s));
    DevBuf<unsigned char> gfirst;
    DevBuf<uint32_t> pfirst, prank, gstart, ng_dev;
    LOCREC_TRY(alloc_each((size_t)n, gfirst, pfirst, prank, gstart));
    LOCREC_TRY(ng_dev.alloc(1));
    LOCREC_LAUNCH(pr_group_flags, grid_for(n), dim3(256), 0, s, n, person, entity, S.rows, gfirst.p, pfirst.p);
    LOCREC_PRIM(tmp, prim::inclusive_sum(p_, bytes_, pfirst.p, prank.p, (int)n, s));
    prim::counting_iterator<uint32_t> iota(0u);
    LOCREC_PRIM(tmp, prim::select_flagged(p_, bytes_, iota, gfirst.p, gstart.p, ng_dev.p, (int)n, s));
    uint32_t g32 = 0;
    LOCREC_READ_BACK(g32, ng_dev.p, s);
    const int64_t g = g32;

    DevBuf<uint32_t> srank, keep, pos;
    DevBuf<uint64_t> cnt, totals;
    LOCREC_TRY(alloc_each((size_t)g, cnt, srank, keep, pos));
    LOCREC_LAUNCH(pr_group_counts, grid_for(g), dim3(256), 0, s, g, n, gstart.p, prank.p, cnt.p, srank.p);
    LOCREC_TRY(rank_keep(g, srank.p, cnt.p, top_n, false, keep.p, pos.p, out_count, tmp, s));
    if (out_weight) LOCREC_TRY(kept_totals(g, srank.p, cnt.p, keep.p, totals, tmp, s));
    LOCREC_LAUNCH(pr_emit_ratings, grid_for(g), dim3(256), 0, s, g, keep.p, pos.p, gstart.p, S.rows, person, entity,
                  cnt.p, srank.p, totals.p, out_person, out_entity, out_rating, out_weight);
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}

// ---- calcRatingVectors ---------------------------------------------------------------------------

struct RangeOut {
    unsigned long long max_key, min_key;  // ordered_key() of the largest / smallest entity id
};

__global__ void pr_entity_range(int64_t n, const int64_t *entity, RangeOut *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long k = i < n ? ordered_key(entity[i]) : ordered_key(entity[0]);
    unsigned long long mx = k, mn = k;
    for (int off = 32; off > 0; off >>= 1) {
        mx = max(mx, (unsigned long long)__shfl_xor((long long)mx, off));
        mn = min(mn, (unsigned long long)__shfl_xor((long long)mn, off));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&out->max_key, mx);
        atomicMin(&out->min_key, mn);
    }
}

// flags of the sorted rows: first row of a person / a row that the person's TreeSet keeps (the first
// of equal indices, in input order: the sort is stable)
__global__ void pr_vector_flags(int64_t n, const int64_t *person, const int64_t *entity, const uint32_t *rows,
                                uint32_t *pfirst, uint32_t *keep)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool np = true, dup = false;
    if (i > 0) {
        np = person[rows[i - 1]] != person[rows[i]];
        dup = !np && entity[rows[i - 1]] == entity[rows[i]];
    }
    pfirst[i] = np ? 1u : 0u;
    keep[i] = dup ? 0u : 1u;
}

__global__ void pr_emit_vectors(int64_t n, const uint32_t *rows, const uint32_t *pfirst, const uint32_t *keep,
                                const uint32_t *prank, const uint32_t *pos, const int64_t *person, const int64_t *entity,
                                const int64_t *rating, int64_t *out_ids, int64_t *out_rowptr, int32_t *out_idx, double *out_val)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const uint32_t r = rows[i], at = pos[i];
    out_idx[at] = (int32_t)entity[r];
    out_val[at] = (double)rating[r];  // rating.toDouble (RatingVectorsBuilder.scala:69)
    if (pfirst[i]) {
        out_ids[prank[i] - 1u] = person[r];
        out_rowptr[prank[i] - 1u] = (int64_t)at;
    }
}

__global__ void pr_set_i64(int64_t *p, int64_t v) { *p = v; }

int32_t calc_rating_vectors(int64_t n, const int64_t *person, const int64_t *entity, const int64_t *rating, int64_t *out_ids,
                            int64_t *out_rowptr, int32_t *out_idx, double *out_val, int64_t *out_npersons, int64_t *out_nnz,
                            int64_t *out_size, hipStream_t s)
{
    Temp tmp;
    DevBuf<RangeOut> range;
    LOCREC_TRY(range.alloc(1));
    const RangeOut init{0ull, ~0ull};
    LOCREC_HIP_TRY(hipMemcpyAsync(range.p, &init, sizeof init, hipMemcpyHostToDevice, s));
    LOCREC_LAUNCH(pr_entity_range, grid_for(n), dim3(256), 0, s, n, entity, range.p);
    RangeOut got;
    LOCREC_READ_BACK(got, range.p, s);
    const int64_t max_id = id_of_key(got.max_key), min_id = id_of_key(got.min_key);
    // checkedCast (RatingVectorsBuilder.scala:36-41): of max(id) first (:27-34), then of every id (:69)
    if (max_id > std::numeric_limits<int32_t>::max() || max_id < std::numeric_limits<int32_t>::min())
        return fail(LOCREC_E_ARITHMETIC, "Index out of Int range: %lld", (long long)max_id);
    if (min_id < std::numeric_limits<int32_t>::min())
        return fail(LOCREC_E_ARITHMETIC, "Index out of Int range: %lld", (long long)min_id);
    // the SparseVector constructor's own require()s (third party: spark-mllib-local_2.12 3.1.2, ml/linalg/Vectors.scala)
    if (min_id < 0) return fail(LOCREC_E_INVALID_ARG, "requirement failed: Found negative index: %lld.", (long long)min_id);
    if (max_id == std::numeric_limits<int32_t>::max())  // checkedCast(maxId) + 1 wraps to Int.MinValue (:34)
        return fail(LOCREC_E_INVALID_ARG, "requirement failed: The size of the requested sparse vector must be no less than 0.");

    SortedRows S;
    LOCREC_TRY(sort_person_entity(n, person, entity, S, tmp, s));
    DevBuf<uint32_t> pfirst, keep, prank, pos;
    LOCREC_TRY(alloc_each((size_t)n, pfirst, keep, prank, pos));
    LOCREC_LAUNCH(pr_vector_flags, grid_for(n), dim3(256), 0, s, n, person, entity, S.rows, pfirst.p, keep.p);
    LOCREC_PRIM(tmp, prim::inclusive_sum(p_, bytes_, pfirst.p, prank.p, (int)n, s));
    LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, keep.p, pos.p, (int)n, s));
    LOCREC_LAUNCH(pr_emit_vectors, grid_for(n), dim3(256), 0, s, n, S.rows, pfirst.p, keep.p, prank.p, pos.p, person,
                  entity, rating, out_ids, out_rowptr, out_idx, out_val);
    uint32_t tail[3] = {0, 0, 0};
    LOCREC_HIP_TRY(hipMemcpyAsync(&tail[0], prank.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&tail[1], pos.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&tail[2], keep.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    *out_npersons = tail[0];
    *out_nnz = (int64_t)tail[1] + tail[2];
    *out_size = max_id + 1;
    LOCREC_LAUNCH(pr_set_i64, dim3(1), dim3(1), 0, s, out_rowptr + *out_npersons, *out_nnz);
    return LOCREC_OK;
}

// ---- buildWithBalancedWeights --------------------------------------------------------------------

__global__ void pr_balance(int64_t n, const int64_t *src, const int64_t *dst, const double *w, double beta, int64_t *out_src,
                           int64_t *out_dst, double *out_w)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_src[i] = src[i];
    out_dst[i] = dst[i];
    out_w[i] = w[i] * beta;  // col("weight") * beta (StochasticGraphBuilder.scala:14,23)
}

// ---- calcPlaceVisits -----------------------------------------------------------------------------

// One thread per visit: the places of the (at most) 3 bands x 3 cells around it, exact distance each.
// WRITE = false counts the matches; WRITE = true stores the place rows at the visit's offset (ascending
// place row) and fills the columns.
// The matches arrive in scan order (band, then cell), so a visit that the capacity cuts stores ALL of
// them, sorts, and only then writes the first `cap - base`: the rows written are the prefix of the
// full result.  scratch_rows has room to the end of that one visit (pr_cut_end).
template <bool WRITE>
__global__ void pr_join(int64_t nv, const int64_t *v_person, const int64_t *v_ts, const double *v_lat, const double *v_lon,
                        const int64_t *v_region, int64_t visits_from, const int64_t *regions, int32_t nr, Grid g,
                        double max_meters, int64_t np, const uint64_t *keys, const uint32_t *place_rows, const int64_t *p_id,
                        const double *p_lat, const double *p_lon, const int64_t *p_category, unsigned long long *counts,
                        const unsigned long long *offsets, int64_t cap, uint32_t *scratch_rows, int64_t *out_person,
                        int64_t *out_ts, int64_t *out_place, int64_t *out_region, int64_t *out_category)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    unsigned long long found = 0;
    const unsigned long long base = WRITE ? offsets[i] : 0ull;
    if (v_ts[i] >= visits_from) {  // locationVisits.where(timestamp >= visitsFrom) (PlaceVisits.scala:24)
        const int64_t r = rank_of_region(regions, nr, v_region[i]);  // join(places, "region_id") (:31)
        const double lat = v_lat[i], lon = v_lon[i];
        if (r >= 0 && location_ok(lat, lon)) {
            for_each_grid_candidate(g, r, lat, lon, keys, np, place_rows, [&](uint32_t j) {
                if (distance_meters(lat, lon, p_lat[j], p_lon[j]) <= max_meters) {  // (:15-21,127)
                    if (WRITE && base < (unsigned long long)cap) scratch_rows[base + found] = j;
                    ++found;
                }
            });
        }
    }
    if (!WRITE) {
        counts[i] = found;
        return;
    }
    const unsigned long long room = base < (unsigned long long)cap ? (unsigned long long)cap - base : 0ull;
    const unsigned long long m = min(found, room);
    const unsigned long long stored = room ? found : 0ull;
    uint32_t *mine = scratch_rows + base;
    sort_ascending(mine, stored);
    for (unsigned long long a = 0; a < m; ++a) {  // select(person_id, timestamp, id as place_id, region_id, category_id) (:40-46)
        const uint32_t j = mine[a];
        out_person[base + a] = v_person[i];
        out_ts[base + a] = v_ts[i];
        out_place[base + a] = p_id[j];
        out_region[base + a] = v_region[i];
        out_category[base + a] = p_category[j];
    }
}

// where the visit that the capacity cuts ends: offsets[i] + counts[i] of the last visit that starts below cap
// (cap >= 1; offsets[0] = 0, non-decreasing).  Every other visit that starts below cap ends at or below it.
__global__ void pr_cut_end(int64_t nv, const unsigned long long *offsets, const unsigned long long *counts, int64_t cap,
                           unsigned long long *out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t a = 0, b = nv - 1;
    while (a < b) {
        const int64_t mid = (a + b + 1) >> 1;
        if (offsets[mid] < (unsigned long long)cap) a = mid; else b = mid - 1;
    }
    out[0] = offsets[a] + counts[a];
}

}  // namespace

extern "C" int32_t locrec_calc_ratings(int64_t n, const int64_t *person_ids, const int64_t *entity_ids, int64_t top_n,
                                       int32_t mem, int64_t *out_person_ids, int64_t *out_entity_ids, int64_t *out_ratings,
                                       int64_t *out_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!out_count) return fail(LOCREC_E_INVALID_ARG, "out_count is required");
    *out_count = 0;
    if (n < 0 || n >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "visit count %lld out of range [0, 2^31)", (long long)n);
    if (n == 0) return LOCREC_OK;
    if (!person_ids || !entity_ids || !out_person_ids || !out_entity_ids || !out_ratings)
        return fail(LOCREC_E_INVALID_ARG, "null array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    In<int64_t> p, e;
    Out<int64_t> op, oe, orat;
    LOCREC_TRY(p.bind(person_ids, n, mem, s));
    LOCREC_TRY(e.bind(entity_ids, n, mem, s));
    LOCREC_TRY(op.bind(out_person_ids, n, mem));
    LOCREC_TRY(oe.bind(out_entity_ids, n, mem));
    LOCREC_TRY(orat.bind(out_ratings, n, mem));
    LOCREC_TRY(calc_ratings(n, p.p, e.p, top_n, op.p, oe.p, orat.p, nullptr, out_count, s));
    LOCREC_TRY(op.deliver(*out_count, s));
    LOCREC_TRY(oe.deliver(*out_count, s));
    LOCREC_TRY(orat.deliver(*out_count, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_calc_rating_vectors(int64_t n, const int64_t *person_ids, const int64_t *entity_ids,
                                              const int64_t *ratings, int32_t mem, int64_t *out_person_ids,
                                              int64_t *out_rowptr, int32_t *out_idx, double *out_val, int64_t *out_npersons,
                                              int64_t *out_nnz, int64_t *out_size)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!out_npersons || !out_nnz || !out_size) return fail(LOCREC_E_INVALID_ARG, "count outputs are required");
    *out_npersons = *out_nnz = *out_size = 0;
    if (n < 0 || n >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "rating count %lld out of range [0, 2^31)", (long long)n);
    if (!out_rowptr) return fail(LOCREC_E_INVALID_ARG, "null array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    if (n == 0) {
        if (mem == LOCREC_MEM_DEVICE) {
            LOCREC_LAUNCH(pr_set_i64, dim3(1), dim3(1), 0, s, out_rowptr, (int64_t)0);
            LOCREC_HIP_TRY(hipStreamSynchronize(s));
        } else {
            out_rowptr[0] = 0;
        }
        return LOCREC_OK;
    }
    if (!person_ids || !entity_ids || !ratings || !out_person_ids || !out_idx || !out_val)
        return fail(LOCREC_E_INVALID_ARG, "null array");
    In<int64_t> p, e, r;
    Out<int64_t> oid, optr;
    Out<int32_t> oidx;
    Out<double> oval;
    LOCREC_TRY(p.bind(person_ids, n, mem, s));
    LOCREC_TRY(e.bind(entity_ids, n, mem, s));
    LOCREC_TRY(r.bind(ratings, n, mem, s));
    LOCREC_TRY(oid.bind(out_person_ids, n, mem));
    LOCREC_TRY(optr.bind(out_rowptr, n + 1, mem));
    LOCREC_TRY(oidx.bind(out_idx, n, mem));
    LOCREC_TRY(oval.bind(out_val, n, mem));
    LOCREC_TRY(calc_rating_vectors(n, p.p, e.p, r.p, oid.p, optr.p, oidx.p, oval.p, out_npersons, out_nnz, out_size, s));
    LOCREC_TRY(oid.deliver(*out_npersons, s));
    LOCREC_TRY(optr.deliver(*out_npersons + 1, s));
    LOCREC_TRY(oidx.deliver(*out_nnz, s));
    LOCREC_TRY(oval.deliver(*out_nnz, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_build_balanced_edges(int32_t n_families, const double *betas, const int64_t *counts,
                                               const int64_t *const *source_ids, const int64_t *const *target_ids,
                                               const double *const *weights, int32_t mem, int64_t *out_source_ids,
                                               int64_t *out_target_ids, double *out_balanced_weights)
try {
    LOCREC_TRY(mem_ok(mem));
    // betas.head / allEdges.head of an empty Seq throw (StochasticGraphBuilder.scala:9-10)
    if (n_families <= 0 || !betas || !counts || !source_ids || !target_ids || !weights)
        return fail(LOCREC_E_INVALID_ARG, "one beta per edge family is required");
    int64_t total = 0;
    for (int32_t f = 0; f < n_families; ++f) {
        if (counts[f] < 0) return fail(LOCREC_E_INVALID_ARG, "negative edge count in family %d", f);
        total += counts[f];
    }
    if (total == 0) return LOCREC_OK;
    if (!out_source_ids || !out_target_ids || !out_balanced_weights) return fail(LOCREC_E_INVALID_ARG, "null array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Out<int64_t> os, ot;
    Out<double> ow;
    LOCREC_TRY(os.bind(out_source_ids, total, mem));
    LOCREC_TRY(ot.bind(out_target_ids, total, mem));
    LOCREC_TRY(ow.bind(out_balanced_weights, total, mem));
    int64_t at = 0;
    for (int32_t f = 0; f < n_families; ++f) {
        const int64_t m = counts[f];
        if (m == 0) continue;
        if (!source_ids[f] || !target_ids[f] || !weights[f]) return fail(LOCREC_E_INVALID_ARG, "null array in family %d", f);
        In<int64_t> a, b;
        In<double> w;
        LOCREC_TRY(a.bind(source_ids[f], m, mem, s));
        LOCREC_TRY(b.bind(target_ids[f], m, mem, s));
        LOCREC_TRY(w.bind(weights[f], m, mem, s));
        LOCREC_LAUNCH(pr_balance, grid_for(m), dim3(256), 0, s, m, a.p, b.p, w.p, betas[f], os.p + at, ot.p + at, ow.p + at);
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (the family's staging buffers are released at the end of this iteration)
        at += m;
    }
    LOCREC_TRY(os.deliver(total, s));
    LOCREC_TRY(ot.deliver(total, s));
    LOCREC_TRY(ow.deliver(total, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_calc_place_visits(int64_t n_visits, const int64_t *v_person_ids, const int64_t *v_timestamps,
                                            const double *v_latitudes, const double *v_longitudes, const int64_t *v_region_ids,
                                            int64_t n_places, const int64_t *p_ids, const double *p_latitudes,
                                            const double *p_longitudes, const int64_t *p_region_ids,
                                            const int64_t *p_category_ids, int64_t visits_from, double max_meters, int32_t mem,
                                            int64_t *out_person_ids, int64_t *out_timestamps, int64_t *out_place_ids,
                                            int64_t *out_region_ids, int64_t *out_category_ids, int64_t *inout_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!inout_count) return fail(LOCREC_E_INVALID_ARG, "inout_count is required");
    const int64_t cap = *inout_count;
    *inout_count = 0;
    if (cap < 0) return fail(LOCREC_E_INVALID_ARG, "negative capacity");
    if (n_visits < 0 || n_visits >= kMaxRows || n_places < 0 || n_places >= kMaxRows)
        return fail(LOCREC_E_INVALID_ARG, "row count out of range [0, 2^31)");
    if (!(max_meters >= 0.0) || !(max_meters < kEarthRadiusMeters))
        return fail(LOCREC_E_INVALID_ARG, "the search radius %g m must be within [0, earth radius)", max_meters);
    if (n_visits == 0 || n_places == 0) return LOCREC_OK;
    if (!v_person_ids || !v_timestamps || !v_latitudes || !v_longitudes || !v_region_ids || !p_ids || !p_latitudes ||
        !p_longitudes || !p_region_ids || !p_category_ids)
        return fail(LOCREC_E_INVALID_ARG, "null array");
    if (cap > 0 && (!out_person_ids || !out_timestamps || !out_place_ids || !out_region_ids || !out_category_ids))
        return fail(LOCREC_E_INVALID_ARG, "null output array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Temp tmp;
    In<int64_t> vp, vt, vr, pi, pr, pc;
    In<double> vlat, vlon, plat, plon;
    LOCREC_TRY(vp.bind(v_person_ids, n_visits, mem, s));
    LOCREC_TRY(vt.bind(v_timestamps, n_visits, mem, s));
    LOCREC_TRY(vlat.bind(v_latitudes, n_visits, mem, s));
    LOCREC_TRY(vlon.bind(v_longitudes, n_visits, mem, s));
    LOCREC_TRY(vr.bind(v_region_ids, n_visits, mem, s));
    LOCREC_TRY(pi.bind(p_ids, n_places, mem, s));
    LOCREC_TRY(plat.bind(p_latitudes, n_places, mem, s));
    LOCREC_TRY(plon.bind(p_longitudes, n_places, mem, s));
    LOCREC_TRY(pr.bind(p_region_ids, n_places, mem, s));
    LOCREC_TRY(pc.bind(p_category_ids, n_places, mem, s));

    // distinct place regions, ascending
    DevBuf<int64_t> regions;
    int32_t nr = 0;
    LOCREC_TRY(distinct_ids(pr.p, n_places, tmp, s, regions, &nr));
    if (nr >= (1 << 24)) return fail(LOCREC_E_INVALID_ARG, "%d distinct regions: at most 2^24 - 1 are supported", nr);

    const Grid g = make_grid(max_meters);

    DevBuf<uint32_t> visited;
    DevBuf<LocationError> err;
    LOCREC_TRY(visited.alloc((size_t)nr));
    LOCREC_TRY(err.alloc(1));
    LOCREC_HIP_TRY(hipMemsetAsync(visited.p, 0, (size_t)nr * 4, s));
    LOCREC_HIP_TRY(hipMemsetAsync(err.p, 0xFF, sizeof(LocationError), s));
    LOCREC_LAUNCH(check_side_a, grid_for(n_visits), dim3(256), 0, s, n_visits, vt.p, visits_from, vlat.p, vlon.p, vr.p,
                  regions.p, nr, visited.p, err.p);
    LOCREC_LAUNCH(check_side_b, grid_for(n_places), dim3(256), 0, s, n_places, plat.p, plon.p, pr.p, regions.p, nr,
                  visited.p, err.p);
    LocationError le;
    LOCREC_READ_BACK(le, err.p, s);
    LOCREC_TRY(location_error(le, vlat.p, vlon.p, "location visit", n_visits, plat.p, plon.p, "place", inout_count));

    DevBuf<uint64_t> k0, k1;
    DevBuf<uint32_t> r0, r1;
    LOCREC_TRY(alloc_each((size_t)n_places, k0, k1, r0, r1));
    LOCREC_LAUNCH(pr_place_keys, grid_for(n_places), dim3(256), 0, s, n_places, plat.p, plon.p, pr.p, regions.p, nr, g, k0.p,
                  r0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r0.p, r1.p, (int)n_places, 0, 64, s));

    DevBuf<unsigned long long> counts, offsets;
    LOCREC_TRY(alloc_each((size_t)n_visits, counts, offsets));
    LOCREC_LAUNCH((pr_join<false>), grid_for(n_visits), dim3(256), 0, s, n_visits, vp.p, vt.p, vlat.p, vlon.p, vr.p,
                  visits_from, regions.p, nr, g, max_meters, n_places, k1.p, r1.p, pi.p, plat.p, plon.p, pc.p, counts.p,
                  nullptr, (int64_t)0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, counts.p, offsets.p, (int)n_visits, s));
    unsigned long long last_off = 0, last_cnt = 0;
    LOCREC_HIP_TRY(hipMemcpyAsync(&last_off, offsets.p + (n_visits - 1), 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&last_cnt, counts.p + (n_visits - 1), 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    const int64_t total = (int64_t)(last_off + last_cnt);
    *inout_count = total;
    const int64_t rows = std::min(total, cap);
    if (rows == 0) return LOCREC_OK;

    Out<int64_t> op, ots, opl, org, oca;
    DevBuf<uint32_t> scratch;
    LOCREC_TRY(op.bind(out_person_ids, rows, mem));
    LOCREC_TRY(ots.bind(out_timestamps, rows, mem));
    LOCREC_TRY(opl.bind(out_place_ids, rows, mem));
    LOCREC_TRY(org.bind(out_region_ids, rows, mem));
    LOCREC_TRY(oca.bind(out_category_ids, rows, mem));
    int64_t scratch_rows = rows;
    if (total > cap) {  // the one visit that the capacity cuts keeps all its matches until they are sorted
        DevBuf<unsigned long long> cut_dev;
        unsigned long long cut_end = 0;
        LOCREC_TRY(cut_dev.alloc(1));
        LOCREC_LAUNCH(pr_cut_end, dim3(1), dim3(64), 0, s, n_visits, offsets.p, counts.p, cap, cut_dev.p);
        LOCREC_READ_BACK(cut_end, cut_dev.p, s);
        scratch_rows = std::max(rows, (int64_t)cut_end);
    }
    LOCREC_TRY(scratch.alloc((size_t)scratch_rows));
    LOCREC_LAUNCH((pr_join<true>), grid_for(n_visits), dim3(256), 0, s, n_visits, vp.p, vt.p, vlat.p, vlon.p, vr.p,
                  visits_from, regions.p, nr, g, max_meters, n_places, k1.p, r1.p, pi.p, plat.p, plon.p, pc.p, nullptr,
                  offsets.p, rows, scratch.p, op.p, ots.p, opl.p, org.p, oca.p);
    LOCREC_TRY(op.deliver(rows, s));
    LOCREC_TRY(ots.deliver(rows, s));
    LOCREC_TRY(opl.deliver(rows, s));
    LOCREC_TRY(org.deliver(rows, s));
    LOCREC_TRY(oca.deliver(rows, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

// Location.distanceMeters (Location.scala:30-38) of n pairs, computed by the device code the join uses.
__global__ void pr_distances(int64_t n, const double *lat1, const double *lon1, const double *lat2, const double *lon2, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = location_ok(lat1[i], lon1[i]) && location_ok(lat2[i], lon2[i])
                            ? distance_meters(lat1[i], lon1[i], lat2[i], lon2[i])
                            : __longlong_as_double(0x7FF8000000000000ll);
}

extern "C" int32_t locrec_distance_meters(int64_t n, const double *lat1, const double *lon1, const double *lat2,
                                          const double *lon2, int32_t mem, double *out_meters)
try {
    LOCREC_TRY(mem_ok(mem));
    if (n < 0 || n >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "pair count out of range [0, 2^31)");
    if (n == 0) return LOCREC_OK;
    if (!lat1 || !lon1 || !lat2 || !lon2 || !out_meters) return fail(LOCREC_E_INVALID_ARG, "null array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    In<double> a, b, c, d;
    Out<double> o;
    LOCREC_TRY(a.bind(lat1, n, mem, s));
    LOCREC_TRY(b.bind(lon1, n, mem, s));
    LOCREC_TRY(c.bind(lat2, n, mem, s));
    LOCREC_TRY(d.bind(lon2, n, mem, s));
    LOCREC_TRY(o.bind(out_meters, n, mem));
    LOCREC_LAUNCH(pr_distances, grid_for(n), dim3(256), 0, s, n, a.p, b.p, c.p, d.p, o.p);
    LOCREC_TRY(o.deliver(n, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

// ---- the mains' final ranking ----------------------------------------------------
// printRecommendations of both mains (KnnRecommenderMain.scala:90-101, StochasticRecommenderMain.scala:64-75):
// places.where(region_id === target) JOIN recommendations ON id, ORDER BY score DESC, LIMIT n.  Rows whose id
// is not a place of the target region (persons, categories, places elsewhere) drop out in the join.

__global__ void pr_region_place_keys(int64_t np, const int64_t *place_ids, const int64_t *place_regions, int64_t target,
                                     uint64_t *keys, unsigned char *in_region)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= np) return;
    keys[j] = ordered_key(place_ids[j]);
    in_region[j] = place_regions[j] == target ? 1 : 0;
}

// key of a kept row: score descending (bit pattern of a double made monotone, then inverted), id ascending is
// the second, earlier sort pass; rows that are not places of the region get the flag 0
__global__ void pr_rank_flags(int64_t n, const int64_t *ids, const uint64_t *allowed, int32_t nallowed, unsigned char *keep)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = ordered_key(ids[i]);
    const int64_t lo = lower_bound_key(allowed, nallowed, k);
    keep[i] = lo < nallowed && allowed[lo] == k ? 1 : 0;
}

__global__ void pr_rank_keys_by_score(int64_t m, const uint32_t *rows, const double *scores, uint64_t *keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) keys[i] = score_desc_key(scores[rows[i]]);
}

__global__ void pr_rank_emit(int64_t w, const uint32_t *rows, const int64_t *ids, const double *scores, int64_t *out_ids,
                             double *out_scores)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w) return;
    out_ids[i] = ids[rows[i]];
    out_scores[i] = scores[rows[i]];
}

extern "C" int32_t locrec_rank_recommendations(int64_t n, const int64_t *ids, const double *scores, int64_t n_places,
                                               const int64_t *place_ids, const int64_t *place_region_ids,
                                               int64_t target_region_id, int64_t max_recommendations, int32_t mem,
                                               int64_t *out_ids, double *out_scores, int64_t *out_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!out_count) return fail(LOCREC_E_INVALID_ARG, "out_count is required");
    *out_count = 0;
    if (n < 0 || n >= kMaxRows || n_places < 0 || n_places >= kMaxRows)
        return fail(LOCREC_E_INVALID_ARG, "row count out of range [0, 2^31)");
    const int64_t limit = std::max<int64_t>(0, max_recommendations);  // limit(n <= 0) is empty
    if (n == 0 || n_places == 0 || limit == 0) return LOCREC_OK;
    if (!ids || !scores || !place_ids || !place_region_ids || !out_ids || !out_scores) return fail(LOCREC_E_INVALID_ARG, "null array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Temp tmp;
    In<int64_t> rid, pid, preg;
    In<double> rsc;
    LOCREC_TRY(rid.bind(ids, n, mem, s));
    LOCREC_TRY(rsc.bind(scores, n, mem, s));
    LOCREC_TRY(pid.bind(place_ids, n_places, mem, s));
    LOCREC_TRY(preg.bind(place_region_ids, n_places, mem, s));
    // the target region's place ids: selected, sorted, distinct
    DevBuf<uint64_t> a0, a1;
    DevBuf<unsigned char> in_region;
    DevBuf<int32_t> cnt_dev;
    LOCREC_TRY(alloc_each((size_t)n_places, a0, a1, in_region));
    LOCREC_TRY(cnt_dev.alloc(1));
    LOCREC_LAUNCH(pr_region_place_keys, grid_for(n_places), dim3(256), 0, s, n_places, pid.p, preg.p, target_region_id, a0.p,
                  in_region.p);
    LOCREC_PRIM(tmp, prim::select_flagged(p_, bytes_, a0.p, in_region.p, a1.p, cnt_dev.p, (int)n_places, s));
    int32_t nallowed = 0;
    LOCREC_READ_BACK(nallowed, cnt_dev.p, s);
    if (nallowed > 0) {
        LOCREC_PRIM(tmp, prim::sort_keys(p_, bytes_, a1.p, a0.p, nallowed, 0, 64, s));
        LOCREC_PRIM(tmp, prim::unique(p_, bytes_, a0.p, a1.p, cnt_dev.p, nallowed, s));
        LOCREC_READ_BACK(nallowed, cnt_dev.p, s);
        std::swap(a0.p, a1.p);  // a0 = the distinct sorted keys
        std::swap(a0.n, a1.n);
    }
    if (nallowed == 0) return LOCREC_OK;
    // rows of the recommendations that are places of the region
    DevBuf<unsigned char> keep;
    DevBuf<uint32_t> r0, r1;
    DevBuf<uint64_t> k0, k1;
    LOCREC_TRY(alloc_each((size_t)n, keep, r0, r1));
    LOCREC_LAUNCH(pr_rank_flags, grid_for(n), dim3(256), 0, s, n, rid.p, a0.p, nallowed, keep.p);
    prim::counting_iterator<uint32_t> iota(0u);
    LOCREC_PRIM(tmp, prim::select_flagged(p_, bytes_, iota, keep.p, r0.p, cnt_dev.p, (int)n, s));
    int32_t m = 0;
    LOCREC_READ_BACK(m, cnt_dev.p, s);
    if (m == 0) return LOCREC_OK;
    // order by (score desc, id asc): stable LSD - by id, then by score
    LOCREC_TRY(alloc_each((size_t)m, k0, k1));
    LOCREC_LAUNCH(gather_id_keys, grid_for(m), dim3(256), 0, s, (int64_t)m, rid.p, r0.p, k0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r0.p, r1.p, m, 0, 64, s));
    LOCREC_LAUNCH(pr_rank_keys_by_score, grid_for(m), dim3(256), 0, s, (int64_t)m, r1.p, rsc.p, k0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r1.p, r0.p, m, 0, 64, s));
    const int64_t w = std::min<int64_t>(m, limit);
    Out<int64_t> oid;
    Out<double> osc;
    LOCREC_TRY(oid.bind(out_ids, w, mem));
    LOCREC_TRY(osc.bind(out_scores, w, mem));
    LOCREC_LAUNCH(pr_rank_emit, grid_for(w), dim3(256), 0, s, w, r0.p, rid.p, rsc.p, oid.p, osc.p);
    LOCREC_TRY(oid.deliver(w, s));
    LOCREC_TRY(osc.deliver(w, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    *out_count = w;
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

// ---- the stochastic graph's edge families (StochasticGraphBuilderMain.scala:47-66) ----------------
// PersonLikesPlace / PersonLikesCategory / CategorySelectedPlace are calcRatings' body with a weight;
// PlaceSimilarPlace is a per-person self-join of the visits within a time interval, counted per ordered
// place pair and then ranked and normalised per source place in the same way.

extern "C" int32_t locrec_calc_count_edges(int64_t n, const int64_t *source_ids, const int64_t *target_ids, int64_t top_n,
                                           int32_t mem, int64_t *out_source_ids, int64_t *out_target_ids, double *out_weights,
                                           int64_t *out_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!out_count) return fail(LOCREC_E_INVALID_ARG, "out_count is required");
    *out_count = 0;
    if (n < 0 || n >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "visit count %lld out of range [0, 2^31)", (long long)n);
    if (n == 0) return LOCREC_OK;
    if (!source_ids || !target_ids || !out_source_ids || !out_target_ids || !out_weights)
        return fail(LOCREC_E_INVALID_ARG, "null array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    In<int64_t> a, b;
    Out<int64_t> oa, ob;
    Out<double> ow;
    LOCREC_TRY(a.bind(source_ids, n, mem, s));
    LOCREC_TRY(b.bind(target_ids, n, mem, s));
    LOCREC_TRY(oa.bind(out_source_ids, n, mem));
    LOCREC_TRY(ob.bind(out_target_ids, n, mem));
    LOCREC_TRY(ow.bind(out_weights, n, mem));
    LOCREC_TRY(calc_ratings(n, a.p, b.p, top_n, oa.p, ob.p, nullptr, ow.p, out_count, s));
    LOCREC_TRY(oa.deliver(*out_count, s));
    LOCREC_TRY(ob.deliver(*out_count, s));
    LOCREC_TRY(ow.deliver(*out_count, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

namespace {

constexpr int kPairTile = 2048;                       // pair keys one block of pr_covisit_emit writes
constexpr int64_t kDefaultPairBudget = (int64_t)1 << 28;  // candidate pairs per chunk: 2 GiB of keys
constexpr int64_t kMaxPairBudget = (int64_t)1 << 30;      // (a chunk's pair count travels as a 32-bit size)

// LOCREC_PREP_PAIR_BUDGET: candidate pairs per chunk of the co-visit join (read once; the result does not depend on it)
int64_t pair_budget()
{
    static const int64_t budget = [] {
        int64_t b = kDefaultPairBudget;
        if (const char *e = std::getenv("LOCREC_PREP_PAIR_BUDGET")) b = atoll(e);
        return std::min(std::max<int64_t>(b, 1), kMaxPairBudget);
    }();
    return budget;
}

// what the last locrec_calc_similar_place_edges of this thread did (locrec_similar_place_edges_stats)
struct CovisitStats {
    int64_t pairs = 0, chunks = 0;
    double ms[3] = {0, 0, 0};  // sort, emit, merge
};
thread_local CovisitStats g_covisit_stats;

enum { kPhaseSort = 0, kPhaseEmit = 1, kPhaseMerge = 2, kPhaseEnd = -1 };

// the rows in (person, timestamp) order: timestamp and dense place rank of sorted position i
__global__ void pr_covisit_gather(int64_t n, const uint32_t *rows, const int64_t *place, const int64_t *ts, const uint64_t *uniq,
                                  int64_t np, int64_t *sorted_ts, uint32_t *sorted_rank)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rows[i];
    sorted_ts[i] = ts[r];
    sorted_rank[i] = (uint32_t)lower_bound_key(uniq, np, ordered_key(place[r]));
}

// The window of sorted row i: the rows [lo, hi] of the same person whose timestamp is within `interval` of row i's
// (isInPlaceSimilarityIntervalUdf, PlaceSimilarPlace.scala:26-28).  Rows are ordered by (person, timestamp), so both
// ends are binary searches over a monotone predicate; a difference of two timestamps fits in int64 (locrec.h), so
// neither subtraction overflows.  width = hi - lo: the partners of row i, itself excluded, same-place rows included.
__global__ void pr_covisit_windows(int64_t n, const uint64_t *person_keys, const int64_t *ts, int64_t interval, uint32_t *lo_out,
                                   unsigned long long *width)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t p = person_keys[i];
    const int64_t t = ts[i];
    int64_t a = 0, b = i;  // first j in [0, i] that is in the window (i itself is)
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (person_keys[mid] == p && t - ts[mid] <= interval) b = mid; else a = mid + 1;
    }
    const int64_t lo = a;
    a = i;
    b = n - 1;             // last j in [i, n) that is in the window
    while (a < b) {
        const int64_t mid = (a + b + 1) >> 1;
        if (person_keys[mid] == p && ts[mid] - t <= interval) a = mid; else b = mid - 1;
    }
    lo_out[i] = (uint32_t)lo;
    width[i] = (unsigned long long)(a - lo);
}

// the last row of the chunk that starts at row r0: the largest r1 in (r0, n] with off[r1] - off[r0] <= budget, and at
// least r0 + 1 (a row whose own window exceeds the budget is a chunk of its own)
__global__ void pr_chunk_end(int64_t n, const unsigned long long *off, int64_t r0, unsigned long long budget,
                             unsigned long long *out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long base = off[r0];
    int64_t a = r0 + 1, b = n;
    while (a < b) {
        const int64_t mid = (a + b + 1) >> 1;
        if (off[mid] - base <= budget) a = mid; else b = mid - 1;
    }
    out[0] = (unsigned long long)a;
    out[1] = off[a] - base;
}

// The self-join of the rows [r0, r1): pair q of the chunk belongs to the row a with off[a] <= off[r0] + q < off[a + 1]
// and is that row's (q - off[a])-th partner.  The PAIR index space is what is split evenly: a block writes kPairTile
// consecutive keys (coalesced 8-byte stores, partners read from consecutive positions), whatever the lengths of the
// windows; two lanes find the rows of the tile's ends, every thread then searches only between them.
__global__ __launch_bounds__(256) void pr_covisit_emit(int64_t r0, int64_t r1, const unsigned long long *off, const uint32_t *lo,
                                                       const uint32_t *rank, int nb, unsigned long long npairs, uint64_t *keys)
{
    __shared__ int64_t ends[2];
    const unsigned long long base = off[r0];
    const unsigned long long t0 = (unsigned long long)blockIdx.x * kPairTile;
    const unsigned long long t1 = min(t0 + (unsigned long long)kPairTile, npairs);
    if (t0 >= t1) return;
    if (threadIdx.x < 2) {
        const unsigned long long p = base + (threadIdx.x == 0 ? t0 : t1 - 1);
        int64_t a = r0, b = r1;  // off[a] <= p < off[b]
        while (b - a > 1) {
            const int64_t mid = (a + b) >> 1;
            if (off[mid] <= p) a = mid; else b = mid;
        }
        ends[threadIdx.x] = a;
    }
    __syncthreads();
    const int64_t first = ends[0], last = ends[1];
    for (unsigned long long q = t0 + threadIdx.x; q < t1; q += blockDim.x) {
        const unsigned long long p = base + q;
        int64_t a = first, b = last + 1;
        while (b - a > 1) {
            const int64_t mid = (a + b) >> 1;
            if (off[mid] <= p) a = mid; else b = mid;
        }
        int64_t j = (int64_t)lo[a] + (int64_t)(p - off[a]);
        if (j >= a) ++j;  // the row itself is no partner
        keys[q] = ((uint64_t)rank[a] << nb) | (uint64_t)rank[j];
    }
}

// runs of the chunk's sorted keys: a pair of two different places stays (col("place_id") =!= col("that_place_id"))
__global__ void pr_pair_flags(int64_t c, const uint64_t *keys, int nb, uint32_t *flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < c) flag[i] = (keys[i] >> nb) != (keys[i] & ((1ull << nb) - 1)) ? 1u : 0u;
}

__global__ void pr_pair_append(int64_t c, const uint64_t *keys, const uint32_t *counts, const uint32_t *flag, const uint32_t *pos,
                               uint64_t *out_keys, uint64_t *out_counts)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c || !flag[i]) return;
    out_keys[pos[i]] = keys[i];
    out_counts[pos[i]] = counts[i];
}

// 0 for the first pair of every source place but the first, so that the inclusive sum is the dense source rank
__global__ void pr_pair_source_steps(int64_t m, const uint64_t *keys, int nb, uint32_t *step)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) step[i] = i > 0 && (keys[i] >> nb) != (keys[i - 1] >> nb) ? 1u : 0u;
}

__global__ void pr_emit_similar(int64_t m, const uint32_t *keep, const uint32_t *pos, const uint64_t *keys, int nb,
                                const uint64_t *uniq, const uint64_t *cnt, const uint32_t *srank, const uint64_t *totals,
                                int64_t cap, int64_t *out_source, int64_t *out_target, double *out_weight)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || !keep[i] || (int64_t)pos[i] >= cap) return;
    const uint32_t at = pos[i];
    out_source[at] = id_of_key(uniq[keys[i] >> nb]);
    out_target[at] = id_of_key(uniq[keys[i] & ((1ull << nb) - 1)]);
    out_weight[at] = (double)cnt[i] / (double)totals[srank[i]];
}

// (pair key, count) of every ordered pair of different places co-visited within the interval, keys ascending
struct PairCounts {
    DevBuf<uint64_t> keys, counts;
    int64_t m = 0;
};

int32_t covisit_counts(int64_t n, const int64_t *person, const int64_t *place, const int64_t *ts, int64_t interval,
                       DevBuf<uint64_t> &uniq, int *nb_out, PairCounts &R, PhaseClock &clock, CovisitStats &stats, Temp &tmp,
                       hipStream_t s)
{
    LOCREC_TRY(clock.mark(kPhaseSort));
    // distinct places, ascending: a place's rank is order-preserving, so rank order is id order
    DevBuf<uint64_t> pk;
    DevBuf<int32_t> np_dev;
    LOCREC_TRY(alloc_each((size_t)n, pk, uniq));
    LOCREC_TRY(np_dev.alloc(1));
    LOCREC_LAUNCH(iota_keys, grid_for(n), dim3(256), 0, s, n, place, uniq.p, (uint32_t *)nullptr);
    LOCREC_PRIM(tmp, prim::sort_keys(p_, bytes_, uniq.p, pk.p, (int)n, 0, 64, s));
    LOCREC_PRIM(tmp, prim::unique(p_, bytes_, pk.p, uniq.p, np_dev.p, (int)n, s));
    int32_t np = 0;
    LOCREC_READ_BACK(np, np_dev.p, s);
    pk.release();
    if (np < 2) return LOCREC_OK;  // one place: every pair is a same-place pair
    int nb = 1;
    while (((int64_t)1 << nb) < np) ++nb;
    *nb_out = nb;

    SortedRows S;
    LOCREC_TRY(sort_person_entity(n, person, ts, S, tmp, s));  // S.k1 = the persons' keys in sorted order
    DevBuf<int64_t> sts;
    DevBuf<uint32_t> srk, lo;
    DevBuf<unsigned long long> width, off, chunk_dev;
    LOCREC_TRY(alloc_each((size_t)n, sts, srk, lo));
    LOCREC_TRY(alloc_each((size_t)n + 1, width, off));
    LOCREC_TRY(chunk_dev.alloc(2));
    LOCREC_LAUNCH(pr_covisit_gather, grid_for(n), dim3(256), 0, s, n, S.rows, place, ts, uniq.p, (int64_t)np, sts.p, srk.p);
    LOCREC_TRY(clock.mark(kPhaseEmit));
    LOCREC_HIP_TRY(hipMemsetAsync(width.p + n, 0, sizeof(unsigned long long), s));
    LOCREC_LAUNCH(pr_covisit_windows, grid_for(n), dim3(256), 0, s, n, S.k1.p, sts.p, interval, lo.p, width.p);
    LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, width.p, off.p, (size_t)n + 1, s));  // off[n] = all candidate pairs
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
    S.k0.release();
    S.r0.release();
    S.r1.release();
    width.release();

    const int64_t budget = pair_budget();
    DevBuf<uint64_t> ka, kb;
    DevBuf<uint32_t> run_counts, flag, pos, nruns_dev;
    LOCREC_TRY(nruns_dev.alloc(1));
    for (int64_t r0 = 0; r0 < n;) {
        LOCREC_TRY(clock.mark(kPhaseEmit));
        LOCREC_LAUNCH(pr_chunk_end, dim3(1), dim3(64), 0, s, n, off.p, r0, (unsigned long long)budget, chunk_dev.p);
        unsigned long long ce[2] = {0, 0};
        LOCREC_READ_BACK(ce, chunk_dev.p, s);
        const int64_t r1 = (int64_t)ce[0], npairs = (int64_t)ce[1];
        if (npairs == 0) {
            r0 = r1;
            continue;
        }
        if (npairs >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "a chunk of %lld candidate pairs: at most 2^31 - 1", (long long)npairs);
        stats.pairs += npairs;
        stats.chunks += 1;
        LOCREC_TRY(ka.reserve((size_t)npairs));
        LOCREC_TRY(kb.reserve((size_t)npairs));
        LOCREC_TRY(run_counts.reserve((size_t)npairs));
        LOCREC_LAUNCH(pr_covisit_emit, grid_for(npairs, kPairTile), dim3(256), 0, s, r0, r1, off.p, lo.p, srk.p, nb,
                      (unsigned long long)npairs, ka.p);
        LOCREC_TRY(clock.mark(kPhaseSort));
        LOCREC_PRIM(tmp, prim::sort_keys(p_, bytes_, ka.p, kb.p, (size_t)npairs, 0, (unsigned)(2 * nb), s));
        LOCREC_PRIM(tmp, prim::run_length_encode(p_, bytes_, kb.p, (size_t)npairs, ka.p, run_counts.p, nruns_dev.p, s));
        uint32_t c32 = 0;
        LOCREC_READ_BACK(c32, nruns_dev.p, s);
        const int64_t c = c32;

        // the runs of two different places, appended to the result so far; sorted and summed per pair if there was one
        LOCREC_TRY(clock.mark(kPhaseMerge));
        LOCREC_TRY(flag.reserve((size_t)c));
        LOCREC_TRY(pos.reserve((size_t)c));
        LOCREC_LAUNCH(pr_pair_flags, grid_for(c), dim3(256), 0, s, c, ka.p, nb, flag.p);
        LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, flag.p, pos.p, (size_t)c, s));
        uint32_t last_pos = 0, last_flag = 0;
        LOCREC_HIP_TRY(hipMemcpyAsync(&last_pos, pos.p + (c - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(&last_flag, flag.p + (c - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        const int64_t add = (int64_t)last_pos + last_flag;
        r0 = r1;
        if (add == 0) continue;
        const int64_t cat = R.m + add;
        if (cat >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "%lld distinct place pairs: at most 2^31 - 1", (long long)cat);
        DevBuf<uint64_t> ck, cc;
        LOCREC_TRY(alloc_each((size_t)cat, ck, cc));
        if (R.m > 0) {
            LOCREC_HIP_TRY(hipMemcpyAsync(ck.p, R.keys.p, (size_t)R.m * 8, hipMemcpyDeviceToDevice, s));
            LOCREC_HIP_TRY(hipMemcpyAsync(cc.p, R.counts.p, (size_t)R.m * 8, hipMemcpyDeviceToDevice, s));
        }
        LOCREC_LAUNCH(pr_pair_append, grid_for(c), dim3(256), 0, s, c, ka.p, run_counts.p, flag.p, pos.p, ck.p + R.m,
                      cc.p + R.m);
        if (R.m == 0) {
            LOCREC_HIP_TRY(hipStreamSynchronize(s));
            std::swap(R.keys.p, ck.p);
            std::swap(R.keys.n, ck.n);
            std::swap(R.counts.p, cc.p);
            std::swap(R.counts.n, cc.n);
            R.m = cat;
            continue;
        }
        DevBuf<uint64_t> sk, sc;
        LOCREC_TRY(alloc_each((size_t)cat, sk, sc));
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, ck.p, sk.p, cc.p, sc.p, (size_t)cat, 0, (unsigned)(2 * nb), s));
        LOCREC_PRIM(tmp, prim::sum_by_key(p_, bytes_, sk.p, sc.p, (size_t)cat, ck.p, cc.p, nruns_dev.p, s));
        LOCREC_READ_BACK(c32, nruns_dev.p, s);
        std::swap(R.keys.p, ck.p);
        std::swap(R.keys.n, ck.n);
        std::swap(R.counts.p, cc.p);
        std::swap(R.counts.n, cc.n);
        R.m = c32;
    }
    return LOCREC_OK;
}

}  // namespace

extern "C" int32_t locrec_calc_similar_place_edges(int64_t n, const int64_t *person_ids, const int64_t *place_ids,
                                                   const int64_t *timestamps, int64_t interval, int64_t top_n, int32_t mem,
                                                   int64_t *out_source_ids, int64_t *out_target_ids, double *out_weights,
                                                   int64_t *inout_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!inout_count) return fail(LOCREC_E_INVALID_ARG, "inout_count is required");
    const int64_t cap = *inout_count;
    *inout_count = 0;
    g_covisit_stats = CovisitStats();
    if (cap < 0) return fail(LOCREC_E_INVALID_ARG, "negative capacity");
    if (n < 0 || n >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "visit count %lld out of range [0, 2^31)", (long long)n);
    if (n == 0 || interval < 0 || top_n <= 0) return LOCREC_OK;  // |dt| <= a negative interval never holds; rank >= 1
    if (!person_ids || !place_ids || !timestamps) return fail(LOCREC_E_INVALID_ARG, "null array");
    if (cap > 0 && (!out_source_ids || !out_target_ids || !out_weights)) return fail(LOCREC_E_INVALID_ARG, "null output array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Temp tmp;
    In<int64_t> pe, pl, ts;
    LOCREC_TRY(pe.bind(person_ids, n, mem, s));
    LOCREC_TRY(pl.bind(place_ids, n, mem, s));
    LOCREC_TRY(ts.bind(timestamps, n, mem, s));

    PhaseClock clock;
    clock.s = s;
    CovisitStats stats;
    DevBuf<uint64_t> uniq;
    PairCounts R;
    int nb = 0;
    LOCREC_TRY(covisit_counts(n, pe.p, pl.p, ts.p, interval, uniq, &nb, R, clock, stats, tmp, s));
    const int64_t m = R.m;
    int64_t total = 0;
    if (m > 0) {
        LOCREC_TRY(clock.mark(kPhaseMerge));
        DevBuf<uint32_t> step, srank, keep, pos;
        DevBuf<uint64_t> totals;
        LOCREC_TRY(alloc_each((size_t)m, step, srank, keep, pos));
        LOCREC_LAUNCH(pr_pair_source_steps, grid_for(m), dim3(256), 0, s, m, R.keys.p, nb, step.p);
        LOCREC_PRIM(tmp, prim::inclusive_sum(p_, bytes_, step.p, srank.p, (size_t)m, s));
        LOCREC_TRY(rank_keep(m, srank.p, R.counts.p, top_n, true, keep.p, pos.p, &total, tmp, s));
        const int64_t rows = std::min(total, cap);
        if (rows > 0) {
            LOCREC_TRY(kept_totals(m, srank.p, R.counts.p, keep.p, totals, tmp, s));
            Out<int64_t> oa, ob;
            Out<double> ow;
            LOCREC_TRY(oa.bind(out_source_ids, rows, mem));
            LOCREC_TRY(ob.bind(out_target_ids, rows, mem));
            LOCREC_TRY(ow.bind(out_weights, rows, mem));
            LOCREC_LAUNCH(pr_emit_similar, grid_for(m), dim3(256), 0, s, m, keep.p, pos.p, R.keys.p, nb, uniq.p, R.counts.p,
                          srank.p, totals.p, rows, oa.p, ob.p, ow.p);
            LOCREC_TRY(oa.deliver(rows, s));
            LOCREC_TRY(ob.deliver(rows, s));
            LOCREC_TRY(ow.deliver(rows, s));
            LOCREC_HIP_TRY(hipStreamSynchronize(s));
        }
    }
    LOCREC_TRY(clock.mark(kPhaseEnd));
    LOCREC_TRY(clock.read(stats.ms));
    g_covisit_stats = stats;
    *inout_count = total;
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_similar_place_edges_stats(int64_t *out_pairs, int64_t *out_chunks, double *out_sort_ms,
                                                    double *out_emit_ms, double *out_merge_ms)
{
    if (out_pairs) *out_pairs = g_covisit_stats.pairs;
    if (out_chunks) *out_chunks = g_covisit_stats.chunks;
    if (out_sort_ms) *out_sort_ms = g_covisit_stats.ms[kPhaseSort];
    if (out_emit_ms) *out_emit_ms = g_covisit_stats.ms[kPhaseEmit];
    if (out_merge_ms) *out_merge_ms = g_covisit_stats.ms[kPhaseMerge];
    return LOCREC_OK;
}
