// rank_batch.hip -- the last stage of a batched request, where the rows already are: per segment of one (ids, scores)
// pair, "places of the target region JOIN rows ON id, ORDER BY score DESC, LIMIT N" (printRecommendations of both mains,
// knn/KnnRecommenderMain.scala:90-101, stochastic/StochasticRecommenderMain.scala:64-75) - exactly what
// locrec_rank_recommendations (prep.hip) returns for each segment on its own, at 16 N bytes a segment.
//
//   region table, once per call   the (region, place id) pairs sorted by two stable radix passes; a segment finds its
//                                 region's range once (rb_plan), a row's membership test is a binary search inside it.
//                                 Duplicates stay in the table: a search finds a place listed twice once.
//   rb_select                     one block per (segment, chunk of LOCREC_RANK_BATCH_CHUNK rows): streams the rows
//                                 coalesced, drops non-members and rows not below the threshold, appends the rest to an
//                                 LDS buffer of 1024 entries; a full buffer is compacted by a block-wide bitonic sort
//                                 that keeps the best N and raises the threshold (the pattern of the KNN lists,
//                                 knn_device.h).  The order is the 3-part key (score_desc_key, id, row in the segment):
//                                 unique per row, so the result does not depend on the arrival order in the buffer.
//                                 A segment of one chunk writes its output row; a chunk of a split segment its partial.
//   rb_merge                      launched only when a segment was split, one block per segment (a block of an unsplit
//                                 segment returns at once): the chunks' partial lists through the same list.
//   N > LOCREC_RANK_BATCH_MAX_N   (or LOCREC_RANK_BATCH_SORT=1) the global path: the kept rows of all segments are
//                                 compacted in order (rb_count, scan, rb_scatter), sorted by three stable radix passes
//                                 (id, score key, segment) and the first N of every segment emitted (rb_emit_sorted).
//   exclusion lists               (rank_segments_device_excluding, locrec_rank_recommendations_batch_excluding) per
//                                 segment a list of ids to leave out, in the mould of the region table: rb_plan checks
//                                 the lists' ranges with the segments' and adds their lengths into one more header
//                                 word; rb_expand_excluded writes the (segment, id key) pairs, two stable radix passes
//                                 order them by id and then segment, and segment s's range is the exclusive sum of the
//                                 lengths.  rb_select_ex / rb_count_ex / rb_scatter_ex drop a row whose key a binary
//                                 search finds in its segment's range - after the membership test, so only a row that
//                                 would be kept pays it.  The table is global memory: a list has no length limit.  With
//                                 every list empty the plain kernels run.
//
//   circles                       (rank_segments_device_near, locrec_rank_recommendations_batch_near) per segment a
//                                 centre and a radius in metres, per place row its coordinates: a row is kept only if
//                                 some listing of its place in the target region lies within the radius by
//                                 distance_meters (place_grid.h).  The region table's sorts carry the input row of
//                                 every table position, so a search's lower bound leads to the listings' coordinates in
//                                 input order.  rb_check_near refuses bad radii and coordinates in the plan step;
//                                 rb_select_near / rb_count_near / rb_scatter_near test a row after the membership (and
//                                 the list, read at run time: a NULL table is none), rb_merge_near and
//                                 rb_emit_sorted_near write out_meters for the rows they emit - evaluated again for
//                                 those N rows, not carried through the list.
//
//   categories                    (rank_segments_device_by_category, locrec_rank_recommendations_batch_by_category) per
//                                 place row a category, per segment an allow-list of categories and a cap on the rows
//                                 of one category.  Only a call with a list entry or a cap below N pays for the tables:
//                                 the place rows' categories become dense ranks (one stable sort, run heads, their sum,
//                                 a scatter back), the lists (segment << 32 | rank) keys in the exclusion table's mould -
//                                 rb_check_cat checks ranges and caps in the plan step, into the same header read-back.
//                                 rb_select_cat / rb_count_cat / rb_scatter_cat (and their _near forms) test a listing's
//                                 category before its distance; the first listing that passes list and circle gives the
//                                 row its category and its out_meters.  With a cap below N the list's entries carry the
//                                 category (rb_select_cap, rb_merge_cap and their _near forms, RbCapList): a compaction
//                                 orders the buffer by (category, key), kills every entry with `cap` entries of its
//                                 category in front of it, then keeps the best N of the rest - exact, because the
//                                 eligible rows in front of a row can only grow; the partial lists of a split segment
//                                 carry the category too and the merge is the same compaction.  On the global path one
//                                 more stable pass orders the sorted positions by (segment, category), rb_cap_flags
//                                 marks the positions under their cap, and rb_emit_capped writes the marked rows whose
//                                 flag sum inside the segment is below N (rb_pad_capped the padding and the counts).
//
// A call waits for the stream once (the plan's totals and the validity of the segments, before any kernel reads a row)
// and, on the global path, once more for the number of kept rows - whatever the number of segments.  Its work buffers
// are local to the call: each hipFree at the end waits for the device as well (about twenty a call, again whatever the
// number of segments; the partial lists of the split segments live until theirs).
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (VGPRs / LDS bytes / scratch / waves per SIMD):
//   rb_select       27 / 20512 / 0 / 7
//   rb_merge        27 / 20512 / 0 / 7
//   rb_count        12 / 4 / 0 / 8
//   rb_scatter      24 / 16 / 0 / 8
//   rb_emit_sorted  14 / 16 / 0 / 8
//   rb_select_ex    27 / 20512 / 0 / 7        rb_expand_excluded  11 / 0 / 0 / 8
//   rb_count_ex     12 / 4 / 0 / 8
//   rb_scatter_ex   24 / 16 / 0 / 8
//   rb_select_near  113 / 20512 / 0 / 4       rb_merge_near        115 / 20512 / 0 / 4
//   rb_count_near   91 / 4 / 0 / 5            rb_emit_sorted_near  94 / 16 / 0 / 5
//   rb_scatter_near 96 / 16 / 0 / 5           rb_check_near        12 / 0 / 0 / 8
//   rb_select_cat   28 / 20512 / 0 / 7        rb_select_cat_near   113 / 20512 / 0 / 4
//   rb_select_cap   37 / 24616 / 0 / 6        rb_select_cap_near   115 / 24616 / 0 / 4
//   rb_merge_cap    37 / 24616 / 0 / 6        rb_merge_cap_near    117 / 24616 / 0 / 4
//   rb_count_cat    16 / 4 / 0 / 8            rb_merge_cat_near    115 / 20512 / 0 / 4
//   rb_scatter_cat  24 / 16 / 0 / 8           rb_count_cat_near    87 / 4 / 0 / 5
//   rb_emit_capped  96 / 0 / 0 / 5            rb_scatter_cat_near  95 / 16 / 0 / 5
//   rb_pad_capped   14 / 16 / 0 / 8           rb_emit_sorted_cat_near  94 / 16 / 0 / 5
//   rb_check_cat    10 / 0 / 0 / 8            rb_expand_allowed    16 / 0 / 0 / 8
//   rb_cat_heads    8 / 0 / 0 / 8             rb_cat_scatter       7 / 0 / 0 / 8
//   rb_cap_keys     10 / 0 / 0 / 8            rb_cap_flags         8 / 0 / 0 / 8
// The capped list is 24 bytes an entry: 24.6 KB of LDS a block, six blocks a CU instead of seven; no new kernel has
// scratch.  (rb_emit_capped reads the circle at run time and so carries the distance's registers in every call.)
// The list is 20 bytes an entry: 20.5 KB of LDS a block, seven blocks of 256 threads a CU by LDS.  The _near kernels are
// bound by registers instead: the fp64 sin / cos / asin of distance_meters take the select body from 27 to 113 VGPRs
// (4 waves a SIMD, no scratch).  The fused form is kept all the same ("Within reach"): a separate pass
// that marks the kept rows would read every id again, write and read a flag per row and add two launches to a call
// that is made of launch latency, while only a row that passed the region join - and the latitude reject - evaluates.

#include "dev_prims.h"

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "place_grid.h"
#include "prep_cols.h"
#include "rank_batch.h"

namespace locrec {

RankBatchStats &rank_batch_stats()
{
    thread_local RankBatchStats st;
    return st;
}

}  // namespace locrec

namespace {

using namespace locrec;

constexpr int kRbThreads = 256;
constexpr int kRbCap = 1024;               // entries of the LDS buffer
constexpr int64_t kRbDefaultChunk = 4096;  // rows per chunk of a split segment
static_assert(LOCREC_RANK_BATCH_MAX_N <= kRbCap - kRbThreads, "a compacted list plus one tile must fit the buffer");

// LOCREC_RANK_BATCH_CHUNK: rows per chunk; LOCREC_RANK_BATCH_SORT=1: the global path for every N (both read per call)
int64_t rb_chunk_rows()
{
    int64_t c = kRbDefaultChunk;
    if (const char *e = std::getenv("LOCREC_RANK_BATCH_CHUNK")) c = atoll(e);
    return std::min<int64_t>(std::max<int64_t>(c, 1), (int64_t)1 << 30);
}

bool rb_force_sort()
{
    const char *e = std::getenv("LOCREC_RANK_BATCH_SORT");
    return e && atoi(e) != 0;
}

// offsets -> (begin, length) per segment; flag: a negative or decreasing offset, or one beyond n.  Reads the offsets
// only, never through them.
__global__ void rb_prepare(int64_t n_seg, const int64_t *offsets, int64_t n, int64_t *seg_begin, int64_t *seg_len,
                           unsigned long long *invalid)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t b = offsets[s], e = offsets[s + 1];
    const bool ok = b >= 0 && e >= b && e <= n;
    seg_begin[s] = ok ? b : 0;
    seg_len[s] = ok ? e - b : 0;
    if (!ok) atomicOr(invalid, 1ull);
}

// hdr: [0] invalid, [1] work items, [2] split segments, [3] their chunks, [4] entries of the exclusion lists.
// ex_begin (NULL: no lists): segment s leaves out the ids ex_ids[ex_begin[s] .. + ex_len[s]), a range inside [0, n_ex];
// xlen gets the lengths as the pair table's scan wants them.  Reads the ranges only, never through them.
__global__ void rb_plan(int64_t n_seg, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *targets, int64_t np,
                        const uint64_t *table_regions, int64_t chunk, const unsigned long long *invalid_in, uint32_t *nch,
                        uint32_t *split_nch, int32_t *lo, int32_t *hi, unsigned long long *hdr, const int64_t *ex_begin,
                        const int64_t *ex_len, int64_t n_ex, uint32_t *xlen)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0 && invalid_in && *invalid_in) atomicOr(&hdr[0], 1ull);
    if (s > n_seg) return;
    if (s == n_seg) {  // the scans' last element
        nch[s] = 0;
        split_nch[s] = 0;
        if (ex_begin) xlen[s] = 0;
        return;
    }
    const int64_t len = seg_len[s];
    bool ok = len >= 0 && len < kMaxRows && seg_begin[s] >= 0;
    if (ex_begin) {
        const int64_t xb = ex_begin[s], xl = ex_len[s];
        const bool xok = xb >= 0 && xl >= 0 && xl <= n_ex && xb <= n_ex - xl;
        xlen[s] = xok ? (uint32_t)xl : 0u;  // (n_ex < 2^31)
        if (xok && xl > 0) atomicAdd(&hdr[4], (unsigned long long)xl);
        ok = ok && xok;
    }
    if (!ok) atomicOr(&hdr[0], 1ull);
    const uint64_t rk = ordered_key(targets[s]);
    const int64_t a = lower_bound_key(table_regions, np, rk);
    const int64_t b = rk == ~0ull ? np : lower_bound_key(table_regions, np, rk + 1);
    lo[s] = (int32_t)a;
    hi[s] = (int32_t)b;
    uint32_t c = 1;
    if (ok && b > a && len > chunk) c = (uint32_t)((len + chunk - 1) / chunk);
    nch[s] = c;
    split_nch[s] = c > 1 ? c : 0;
    atomicAdd(&hdr[1], (unsigned long long)c);
    if (c > 1) {
        atomicAdd(&hdr[2], 1ull);
        atomicAdd(&hdr[3], (unsigned long long)c);
    }
}

// ---- the list of one block -------------------------------------------------------------------------------------------

struct RbList {
    uint64_t k[kRbCap];    // score_desc_key
    uint64_t id[kRbCap];   // ordered_key of the id
    uint32_t row[kRbCap];  // row inside the segment
    uint64_t thr_k, thr_id;
    uint32_t thr_row;
    int count, have_thr;
};

__device__ __forceinline__ bool rb_less(uint64_t ka, uint64_t ia, uint32_t ra, uint64_t kb, uint64_t ib, uint32_t rb)
{
    if (ka != kb) return ka < kb;
    if (ia != ib) return ia < ib;
    return ra < rb;
}

// ascending bitonic sort of entries [0, P), P a power of two <= kRbCap; every thread of the block
__device__ void rb_sort(RbList &L, int P)
{
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += kRbThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const uint64_t ka = L.k[i], kb = L.k[p], ia = L.id[i], ib = L.id[p];
                const uint32_t ra = L.row[i], rb = L.row[p];
                const bool up = (i & k) == 0;
                const bool sw = up ? rb_less(kb, ib, rb, ka, ia, ra) : rb_less(ka, ia, ra, kb, ib, rb);
                if (sw) {
                    L.k[i] = kb; L.k[p] = ka;
                    L.id[i] = ib; L.id[p] = ia;
                    L.row[i] = rb; L.row[p] = ra;
                }
            }
            __syncthreads();
        }
    }
}

// sorts the buffer; with at least N entries keeps the best N and makes the N-th the threshold.  -> entries kept.
// Every thread of the block, after a barrier behind the last append.
__device__ int rb_compact(RbList &L, int N)
{
    const int cnt = L.count;
    int P = 2;
    while (P < cnt) P <<= 1;
    for (int i = cnt + threadIdx.x; i < P; i += kRbThreads) {  // above every real entry (no score has the key ~0)
        L.k[i] = ~0ull;
        L.id[i] = ~0ull;
        L.row[i] = ~0u;
    }
    __syncthreads();
    rb_sort(L, P);
    const int w = min(cnt, N);
    if (threadIdx.x == 0 && cnt >= N) {
        L.count = N;
        L.thr_k = L.k[N - 1];
        L.thr_id = L.id[N - 1];
        L.thr_row = L.row[N - 1];
        L.have_thr = 1;
    }
    __syncthreads();
    return w;
}

__device__ __forceinline__ void rb_push(RbList &L, uint64_t k, uint64_t id, uint32_t row)
{
    if (L.have_thr && !rb_less(k, id, row, L.thr_k, L.thr_id, L.thr_row)) return;
    const int slot = atomicAdd(&L.count, 1);  // < kRbCap: at most kRbCap - kRbThreads before a tile
    L.k[slot] = k;
    L.id[slot] = id;
    L.row[slot] = row;
}

// before a tile's appends: the count is read by all between two barriers, so the decision to compact is uniform
__device__ __forceinline__ void rb_make_room(RbList &L, int N)
{
    __syncthreads();
    const int cnt = L.count;
    __syncthreads();
    if (cnt > kRbCap - kRbThreads) rb_compact(L, N);
}

// ---- the capped list ---------------------------------------------------------------------------------------------------
// The list of a segment with a cap per category: an entry carries the dense rank of its category as well.  "The N-th best
// so far" is no threshold here - a category that fills up must not push out the rows of the next one - so a compaction
// first orders the buffer by (category, 3-part key) and kills every entry with `cap` entries of its category in front of
// it, then orders the survivors by the 3-part key, keeps the best N and makes the N-th the threshold.  Both steps are
// final whatever arrives later: the eligible rows in front of a row, sum over the categories of min(cap, kept rows of
// the category in front of it), can only grow.
struct RbCapList : RbList {
    uint32_t cat[kRbCap];
    int killed;
};

// rb_sort with the category travelling; BYCAT: the category is the first part of the key
template <bool BYCAT>
__device__ void rb_sort_cap(RbCapList &L, int P)
{
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += kRbThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const uint64_t ka = L.k[i], kb = L.k[p], ia = L.id[i], ib = L.id[p];
                const uint32_t ra = L.row[i], rb = L.row[p], ca = L.cat[i], cb = L.cat[p];
                bool a_b = rb_less(ka, ia, ra, kb, ib, rb), b_a = rb_less(kb, ib, rb, ka, ia, ra);
                if constexpr (BYCAT) {
                    if (ca != cb) {
                        a_b = ca < cb;
                        b_a = cb < ca;
                    }
                }
                const bool up = (i & k) == 0;
                if (up ? b_a : a_b) {
                    L.k[i] = kb; L.k[p] = ka;
                    L.id[i] = ib; L.id[p] = ia;
                    L.row[i] = rb; L.row[p] = ra;
                    L.cat[i] = cb; L.cat[p] = ca;
                }
            }
            __syncthreads();
        }
    }
}

// rb_compact for the capped list; cap: the segment's, already cut to N (cap == N: no cap, the plain compaction)
__device__ int rb_compact(RbCapList &L, int N, int cap)
{
    const int cnt = L.count;
    int P = 2;
    while (P < cnt) P <<= 1;
    for (int i = cnt + threadIdx.x; i < P; i += kRbThreads) {  // above every real entry (a place's rank is < 2^31)
        L.k[i] = ~0ull;
        L.id[i] = ~0ull;
        L.row[i] = ~0u;
        L.cat[i] = ~0u;
    }
    if (threadIdx.x == 0) L.killed = 0;
    __syncthreads();
    if (cap < N) {
        rb_sort_cap<true>(L, P);
        // entry i has `cap` entries of its category in front of it iff entry i - cap is of its category: the kill reads
        // categories only and writes keys only, so it needs no barrier of its own
        int mine = 0;
        for (int i = cap + threadIdx.x; i < cnt; i += kRbThreads) {
            if (L.cat[i - cap] == L.cat[i]) {
                L.k[i] = ~0ull;
                L.id[i] = ~0ull;
                L.row[i] = ~0u;
                ++mine;
            }
        }
        if (mine) atomicAdd(&L.killed, mine);
        __syncthreads();
    }
    rb_sort_cap<false>(L, P);
    const int live = cnt - L.killed, w = min(live, N);
    __syncthreads();  // every thread has read the count of the killed
    if (threadIdx.x == 0) {
        L.count = w;
        if (live >= N) {
            L.thr_k = L.k[N - 1];
            L.thr_id = L.id[N - 1];
            L.thr_row = L.row[N - 1];
            L.have_thr = 1;
        }
    }
    __syncthreads();
    return w;
}

__device__ __forceinline__ void rb_push(RbCapList &L, uint64_t k, uint64_t id, uint32_t row, uint32_t cat)
{
    if (L.have_thr && !rb_less(k, id, row, L.thr_k, L.thr_id, L.thr_row)) return;
    const int slot = atomicAdd(&L.count, 1);
    L.k[slot] = k;
    L.id[slot] = id;
    L.row[slot] = row;
    L.cat[slot] = cat;
}

__device__ __forceinline__ void rb_make_room(RbCapList &L, int N, int cap)
{
    __syncthreads();
    const int cnt = L.count;
    __syncthreads();
    if (cnt > kRbCap - kRbThreads) rb_compact(L, N, cap);
}

// the segment of work item w: the last s with first[s] <= w (first[] strictly increasing, first[0] = 0)
__device__ __forceinline__ int64_t rb_segment_of(const uint32_t *first, int64_t n_seg, uint32_t w)
{
    int64_t a = 0, b = n_seg;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (first[mid] <= w) a = mid + 1; else b = mid;
    }
    return a - 1;
}

// ---- the circle --------------------------------------------------------------------------------------------------------
// What a _near kernel knows beside its siblings' arguments: segment s keeps a row only if some listing of its place in the
// target region lies within rad[s] metres of (clat[s], clon[s]).  Table position t is input row trow[t] of the place
// table (the value the region table's two sorts carry), so the listings of one (region, id) stand in input order and
// the first one inside the circle is the one that counts.  meters (NULL: not wanted): the output rows' distances.
struct RbNear {
    const double *clat, *clon, *rad, *plat, *plon;
    const uint32_t *trow;
    const int32_t *lo, *hi;
    const uint64_t *table_ids;
    double *meters;
};

// The circle of one segment.  band: the radius as degrees of latitude with make_grid's margins - a listing further
// north or south than that is outside whatever its longitude (distance >= R |dlat|; the margin of 1e-9 relative and
// 1e-12 degrees is far above distance_meters' rounding), so the reject is on the safe side and the exact test decides
// everything else.  An infinite radius keeps every listing without evaluating anything.
struct RbCircle {
    double lat, lon, rad, band;
    bool all;
};

__device__ __forceinline__ RbCircle rb_circle_of(const RbNear &nr, int64_t s)
{
    RbCircle c;
    c.lat = nr.clat[s];
    c.lon = nr.clon[s];
    c.rad = nr.rad[s];
    c.all = c.rad == INFINITY;
    c.band = c.rad / kEarthRadiusMeters * (180.0 / kPi) * (1.0 + 1e-9) + 1e-12;
    return c;
}

// table position a is the first listing of `key` (a < thi): is one of its listings inside the circle?  *meters: the
// distance of the first that is - bit for bit distance_meters of (centre, listing), as locrec_distance_meters has it.
// (flatten: distance_meters stays inlined here however many kernels call it - a unit with more callers would otherwise
// turn it into a function call and change the _near kernels' registers)
__device__ __forceinline__ __attribute__((flatten)) bool rb_within(const RbNear &nr, const RbCircle &c, int32_t a, int32_t thi,
                                                                   uint64_t key, double *meters)
{
    for (; a < thi && nr.table_ids[a] == key; ++a) {
        const uint32_t j = nr.trow[a];
        const double plat = nr.plat[j];
        if (!c.all && fabs(plat - c.lat) > c.band) continue;
        const double d = distance_meters(c.lat, c.lon, plat, nr.plon[j]);
        if (d <= c.rad || c.all) {
            *meters = d;
            return true;
        }
    }
    return false;
}

// the distance an output row of segment s reports for the kept id `key`
__device__ __forceinline__ double rb_meters_of(const RbNear &nr, const RbCircle &c, int64_t s, uint64_t key)
{
    const int32_t thi = nr.hi[s];
    int32_t a = nr.lo[s], b = thi;
    while (a < b) {
        const int32_t mid = (int32_t)(((uint32_t)a + (uint32_t)b) >> 1);
        if (nr.table_ids[mid] < key) a = mid + 1; else b = mid;
    }
    double d = 0.0;
    rb_within(nr, c, a, thi, key, &d);
    return d;
}

// ---- the categories ----------------------------------------------------------------------------------------------------
// What a _cat kernel knows beside a _near kernel's arguments (its RbNear always carries trow, lo, hi and table_ids, the
// coordinates only in the _cat_near kernels): input row j of the place table has the category of dense rank crank[j];
// segment s allows the ranks in the low words of akeys[afirst[s] .. afirst[s + 1]) - (segment << 32 | rank), ascending;
// an empty range: any - and keeps caps[s] rows of one category.  afirst NULL: no lists; caps NULL: no caps.
struct RbCat {
    const uint32_t *crank, *afirst;
    const uint64_t *akeys;
    const int64_t *caps;
};

__device__ __forceinline__ bool rb_excluded(const uint64_t *xkeys, uint32_t a, uint32_t b, uint64_t key);  // (below)

// the range of segment s's allow-list (empty: every category)
__device__ __forceinline__ void rb_allow_range(const RbCat &ct, int64_t s, uint32_t *aa, uint32_t *ab)
{
    *aa = ct.afirst ? ct.afirst[s] : 0u;
    *ab = ct.afirst ? ct.afirst[s + 1] : 0u;
}

// rb_within with the listing's category tested first (a search is cheaper than fp64 trig): table position a is the first
// listing of `key`; the first listing whose category segment s allows and which lies inside the circle counts.  *cat: its
// category's rank; *meters (NULL: not wanted, and an infinite radius evaluates nothing): its distance.
template <bool NEAR>
__device__ __forceinline__ __attribute__((flatten)) bool rb_within_cat(const RbNear &nr, const RbCircle &c, const RbCat &ct, uint32_t aa, uint32_t ab,
                                              int64_t s, int32_t a, int32_t thi, uint64_t key, double *meters, uint32_t *cat)
{
    for (; a < thi && nr.table_ids[a] == key; ++a) {
        const uint32_t j = nr.trow[a];
        const uint32_t cr = ct.crank[j];
        if (aa < ab && !rb_excluded(ct.akeys, aa, ab, ((uint64_t)s << 32) | cr)) continue;
        if constexpr (NEAR) {
            if (!c.all || meters) {
                const double plat = nr.plat[j];
                if (!c.all && fabs(plat - c.lat) > c.band) continue;
                const double d = distance_meters(c.lat, c.lon, plat, nr.plon[j]);
                if (!(d <= c.rad || c.all)) continue;
                if (meters) *meters = d;
            }
        }
        *cat = cr;
        return true;
    }
    return false;
}

// rb_meters_of under the categories' rule: the distance of the listing that counts
__device__ __forceinline__ double rb_meters_of_cat(const RbNear &nr, const RbCircle &c, const RbCat &ct, int64_t s, uint64_t key)
{
    const int32_t thi = nr.hi[s];
    int32_t a = nr.lo[s], b = thi;
    while (a < b) {
        const int32_t mid = (int32_t)(((uint32_t)a + (uint32_t)b) >> 1);
        if (nr.table_ids[mid] < key) a = mid + 1; else b = mid;
    }
    uint32_t aa, ab, cr;
    rb_allow_range(ct, s, &aa, &ab);
    double d = 0.0;
    rb_within_cat<true>(nr, c, ct, aa, ab, s, a, thi, key, &d, &cr);
    return d;
}

// the sorted list's first w entries -> output row s (padded to N)
template <bool NEAR, bool CAT = false>
__device__ __forceinline__ void rb_emit_row(const RbList &L, int w, int N, int64_t s, int64_t begin, const double *scores,
                                            int64_t *out_ids, double *out_scores, int64_t *out_counts, const RbNear &nr,
                                            const RbCat &ct = RbCat{})
{
    for (int j = threadIdx.x; j < N; j += kRbThreads) {
        const int64_t o = s * (int64_t)N + j;
        out_ids[o] = j < w ? id_of_key(L.id[j]) : -1;
        out_scores[o] = j < w ? scores[begin + L.row[j]] : 0.0;
        if constexpr (NEAR && CAT) {
            if (nr.meters) nr.meters[o] = j < w ? rb_meters_of_cat(nr, rb_circle_of(nr, s), ct, s, L.id[j]) : 0.0;
        } else if constexpr (NEAR) {
            if (nr.meters) nr.meters[o] = j < w ? rb_meters_of(nr, rb_circle_of(nr, s), s, L.id[j]) : 0.0;
        }
    }
    if (threadIdx.x == 0) out_counts[s] = w;
}

// ---- the exclusion lists: the pair table -----------------------------------------------------------------------------
// (segment, id key) for every entry of every list, sorted by segment and then id: segment s's ids are
// xkeys[xfirst[s] .. xfirst[s + 1]), ascending, duplicates kept (a search finds an id listed twice once).  The table is
// global memory whatever a list's length: nothing here assumes a list fits in LDS.

// pair p of the unsorted table: the segment whose range of the lengths' scan holds p (an empty list holds none)
__global__ void rb_expand_excluded(int64_t n_seg, int64_t total, const uint32_t *xfirst, const int64_t *ex_begin,
                                   const int64_t *ex_ids, uint64_t *keys, uint32_t *segs)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const int64_t s = rb_segment_of(xfirst, n_seg, (uint32_t)p);
    keys[p] = ordered_key(ex_ids[ex_begin[s] + (p - (int64_t)xfirst[s])]);
    segs[p] = (uint32_t)s;
}

// is key in xkeys[a, b)?
__device__ __forceinline__ bool rb_excluded(const uint64_t *xkeys, uint32_t a, uint32_t b, uint64_t key)
{
    const uint32_t end = b;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (xkeys[mid] < key) a = mid + 1; else b = mid;
    }
    return a < end && xkeys[a] == key;
}

// The three kernels that test a row are bodies with the exclusion and the circle as template parameters: the plain
// kernels keep their signatures and, with EX and NEAR false, their code; the _ex kernels take the pair table as well;
// the _near kernels take the circle and read the lists at run time (xkeys NULL: none), so they are three and not six.
// CAT (0: none; 1: the categories' test; 2: the capped list as well - the select and the merge only): the _cat and
// _cat_near kernels, which read the exclusion lists at run time like the _near kernels.
template <bool EX, bool NEAR, int CAT = 0>
__device__ __forceinline__ void rb_select_body(int64_t n_seg, const uint32_t *first, const uint32_t *pfirst,
                                               const int64_t *seg_begin, const int64_t *seg_len, const int32_t *lo,
                                               const int32_t *hi, const uint64_t *table_ids, const int64_t *ids,
                                               const double *scores, int64_t chunk, int N, uint64_t *pk, uint64_t *pid,
                                               uint32_t *prow, int32_t *pcount, int64_t *out_ids, double *out_scores,
                                               int64_t *out_counts, const uint32_t *xfirst, const uint64_t *xkeys,
                                               const RbNear &nr, const RbCat &ct = RbCat{}, uint32_t *pcat = nullptr)
{
    __shared__ std::conditional_t<CAT == 2, RbCapList, RbList> L;
    const uint32_t w = blockIdx.x;
    const int64_t s = rb_segment_of(first, n_seg, w);
    const uint32_t nch = first[s + 1] - first[s], c = w - first[s];
    const int64_t begin = seg_begin[s], len = seg_len[s];
    const int32_t tlo = lo[s], thi = hi[s];
    uint32_t xa = 0, xb = 0;
    if constexpr (EX) {
        if (!(NEAR || CAT) || xkeys) {
            xa = xfirst[s];
            xb = xfirst[s + 1];
        }
    }
    const int64_t r0 = (int64_t)c * chunk;
    const int64_t r1 = thi > tlo ? min(len, nch == 1 ? len : r0 + chunk) : 0;  // no place in the region: nothing to read
    RbCircle cir = {};
    if constexpr (NEAR) cir = rb_circle_of(nr, s);
    uint32_t aa = 0, ab = 0;
    if constexpr (CAT != 0) rb_allow_range(ct, s, &aa, &ab);
    int cap = N;  // (a cap of N or more is none: each of the first N rows has fewer than N in front of it)
    if constexpr (CAT == 2) cap = (int)min((int64_t)N, ct.caps[s]);
    if (threadIdx.x == 0) {
        L.count = 0;
        L.have_thr = 0;
    }
    for (int64_t t0 = r0; t0 < r1; t0 += kRbThreads) {
        if constexpr (CAT == 2) rb_make_room(L, N, cap); else rb_make_room(L, N);
        const int64_t r = t0 + threadIdx.x;
        if (r < r1) {
            const uint64_t key = ordered_key(ids[begin + r]);
            int32_t a = tlo, b = thi;
            while (a < b) {
                const int32_t mid = (int32_t)(((uint32_t)a + (uint32_t)b) >> 1);
                if (table_ids[mid] < key) a = mid + 1; else b = mid;
            }
            bool keep = a < thi && table_ids[a] == key;
            if constexpr (EX) keep = keep && !rb_excluded(xkeys, xa, xb, key);
            uint32_t cr = 0;
            if constexpr (CAT != 0) {
                keep = keep && rb_within_cat<NEAR>(nr, cir, ct, aa, ab, s, a, thi, key, nullptr, &cr);
            } else if constexpr (NEAR) {
                double d;
                keep = keep && (cir.all || rb_within(nr, cir, a, thi, key, &d));
            }
            if constexpr (CAT == 2) {
                if (keep) rb_push(L, score_desc_key(scores[begin + r]), key, (uint32_t)r, cr);
            } else {
                if (keep) rb_push(L, score_desc_key(scores[begin + r]), key, (uint32_t)r);
            }
        }
    }
    __syncthreads();
    int wn;
    if constexpr (CAT == 2) wn = rb_compact(L, N, cap); else wn = rb_compact(L, N);
    if (nch == 1) {
        rb_emit_row<NEAR, CAT != 0>(L, wn, N, s, begin, scores, out_ids, out_scores, out_counts, nr, ct);
        return;
    }
    const int64_t slot = (int64_t)pfirst[s] + c;
    for (int j = threadIdx.x; j < wn; j += kRbThreads) {
        pk[slot * N + j] = L.k[j];
        pid[slot * N + j] = L.id[j];
        prow[slot * N + j] = L.row[j];
        if constexpr (CAT == 2) pcat[slot * N + j] = L.cat[j];
    }
    if (threadIdx.x == 0) pcount[slot] = wn;
}

__global__ __launch_bounds__(kRbThreads) void rb_select(int64_t n_seg, const uint32_t *first, const uint32_t *pfirst,
                                                        const int64_t *seg_begin, const int64_t *seg_len, const int32_t *lo,
                                                        const int32_t *hi, const uint64_t *table_ids, const int64_t *ids,
                                                        const double *scores, int64_t chunk, int N, uint64_t *pk,
                                                        uint64_t *pid, uint32_t *prow, int32_t *pcount, int64_t *out_ids,
                                                        double *out_scores, int64_t *out_counts)
{
    rb_select_body<false, false>(n_seg, first, pfirst, seg_begin, seg_len, lo, hi, table_ids, ids, scores, chunk, N, pk, pid, prow,
                                 pcount, out_ids, out_scores, out_counts, nullptr, nullptr, RbNear{});
}

__global__ __launch_bounds__(kRbThreads) void rb_select_ex(int64_t n_seg, const uint32_t *first, const uint32_t *pfirst,
                                                           const int64_t *seg_begin, const int64_t *seg_len, const int32_t *lo,
                                                           const int32_t *hi, const uint64_t *table_ids, const int64_t *ids,
                                                           const double *scores, int64_t chunk, int N, uint64_t *pk,
                                                           uint64_t *pid, uint32_t *prow, int32_t *pcount, int64_t *out_ids,
                                                           double *out_scores, int64_t *out_counts, const uint32_t *xfirst,
                                                           const uint64_t *xkeys)
{
    rb_select_body<true, false>(n_seg, first, pfirst, seg_begin, seg_len, lo, hi, table_ids, ids, scores, chunk, N, pk, pid, prow,
                                pcount, out_ids, out_scores, out_counts, xfirst, xkeys, RbNear{});
}

__global__ __launch_bounds__(kRbThreads) void rb_select_near(int64_t n_seg, const uint32_t *first, const uint32_t *pfirst,
                                                             const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                                                             const double *scores, int64_t chunk, int N, uint64_t *pk,
                                                             uint64_t *pid, uint32_t *prow, int32_t *pcount, int64_t *out_ids,
                                                             double *out_scores, int64_t *out_counts, const uint32_t *xfirst,
                                                             const uint64_t *xkeys, RbNear nr)
{
    rb_select_body<true, true>(n_seg, first, pfirst, seg_begin, seg_len, nr.lo, nr.hi, nr.table_ids, ids, scores, chunk, N, pk, pid,
                               prow, pcount, out_ids, out_scores, out_counts, xfirst, xkeys, nr);
}

// the _cat kernels: NEAR with the circle; CAT 1: today's list plus the categories' test, 2: the capped list
template <bool NEAR, int CAT>
__device__ __forceinline__ void rb_select_cat_any(int64_t n_seg, const uint32_t *first, const uint32_t *pfirst,
                                                  const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                                                  const double *scores, int64_t chunk, int N, uint64_t *pk, uint64_t *pid,
                                                  uint32_t *prow, uint32_t *pcat, int32_t *pcount, int64_t *out_ids,
                                                  double *out_scores, int64_t *out_counts, const uint32_t *xfirst,
                                                  const uint64_t *xkeys, const RbNear &nr, const RbCat &ct)
{
    rb_select_body<true, NEAR, CAT>(n_seg, first, pfirst, seg_begin, seg_len, nr.lo, nr.hi, nr.table_ids, ids, scores, chunk, N, pk,
                                    pid, prow, pcount, out_ids, out_scores, out_counts, xfirst, xkeys, nr, ct, pcat);
}

#define RB_SELECT_CAT_KERNEL(name, NEAR, CAT)                                                                                   \
    __global__ __launch_bounds__(kRbThreads) void name(                                                                         \
        int64_t n_seg, const uint32_t *first, const uint32_t *pfirst, const int64_t *seg_begin, const int64_t *seg_len,         \
        const int64_t *ids, const double *scores, int64_t chunk, int N, uint64_t *pk, uint64_t *pid, uint32_t *prow,            \
        uint32_t *pcat, int32_t *pcount, int64_t *out_ids, double *out_scores, int64_t *out_counts, const uint32_t *xfirst,     \
        const uint64_t *xkeys, RbNear nr, RbCat ct)                                                                             \
    {                                                                                                                           \
        rb_select_cat_any<NEAR, CAT>(n_seg, first, pfirst, seg_begin, seg_len, ids, scores, chunk, N, pk, pid, prow, pcat,      \
                                     pcount, out_ids, out_scores, out_counts, xfirst, xkeys, nr, ct);                           \
    }
RB_SELECT_CAT_KERNEL(rb_select_cat, false, 1)
RB_SELECT_CAT_KERNEL(rb_select_cat_near, true, 1)
RB_SELECT_CAT_KERNEL(rb_select_cap, false, 2)
RB_SELECT_CAT_KERNEL(rb_select_cap_near, true, 2)
#undef RB_SELECT_CAT_KERNEL

template <bool NEAR, int CAT = 0>
__device__ __forceinline__ void rb_merge_body(const uint32_t *first, const uint32_t *pfirst, const int64_t *seg_begin,
                                              const double *scores, int N, const uint64_t *pk, const uint64_t *pid,
                                              const uint32_t *prow, const int32_t *pcount, int64_t *out_ids, double *out_scores,
                                              int64_t *out_counts, const RbNear &nr, const RbCat &ct = RbCat{},
                                              const uint32_t *pcat = nullptr)
{
    __shared__ std::conditional_t<CAT == 2, RbCapList, RbList> L;
    const int64_t s = blockIdx.x;
    const uint32_t nch = first[s + 1] - first[s];
    if (nch <= 1) return;
    const int64_t slot0 = pfirst[s], total = (int64_t)nch * N;
    int cap = N;
    if constexpr (CAT == 2) cap = (int)min((int64_t)N, ct.caps[s]);
    if (threadIdx.x == 0) {
        L.count = 0;
        L.have_thr = 0;
    }
    for (int64_t t0 = 0; t0 < total; t0 += kRbThreads) {
        if constexpr (CAT == 2) rb_make_room(L, N, cap); else rb_make_room(L, N);
        const int64_t t = t0 + threadIdx.x;
        if (t < total) {
            const int64_t c = t / N;
            const int j = (int)(t - c * N);
            if constexpr (CAT == 2) {
                if (j < pcount[slot0 + c]) rb_push(L, pk[slot0 * N + t], pid[slot0 * N + t], prow[slot0 * N + t], pcat[slot0 * N + t]);
            } else {
                if (j < pcount[slot0 + c]) rb_push(L, pk[slot0 * N + t], pid[slot0 * N + t], prow[slot0 * N + t]);
            }
        }
    }
    __syncthreads();
    int wn;
    if constexpr (CAT == 2) wn = rb_compact(L, N, cap); else wn = rb_compact(L, N);
    rb_emit_row<NEAR, CAT != 0>(L, wn, N, s, seg_begin[s], scores, out_ids, out_scores, out_counts, nr, ct);
}

__global__ __launch_bounds__(kRbThreads) void rb_merge(const uint32_t *first, const uint32_t *pfirst, const int64_t *seg_begin,
                                                       const double *scores, int N, const uint64_t *pk, const uint64_t *pid,
                                                       const uint32_t *prow, const int32_t *pcount, int64_t *out_ids,
                                                       double *out_scores, int64_t *out_counts)
{
    rb_merge_body<false>(first, pfirst, seg_begin, scores, N, pk, pid, prow, pcount, out_ids, out_scores, out_counts, RbNear{});
}

__global__ __launch_bounds__(kRbThreads) void rb_merge_near(const uint32_t *first, const uint32_t *pfirst, const int64_t *seg_begin,
                                                            const double *scores, int N, const uint64_t *pk, const uint64_t *pid,
                                                            const uint32_t *prow, const int32_t *pcount, int64_t *out_ids,
                                                            double *out_scores, int64_t *out_counts, RbNear nr)
{
    rb_merge_body<true>(first, pfirst, seg_begin, scores, N, pk, pid, prow, pcount, out_ids, out_scores, out_counts, nr);
}

// the merges of the _cat kernels' partial lists: with the circle (out_meters under the categories' rule) and / or capped -
// a chunk's partial list holds every row of the answer that lies in the chunk and every row that counts against one,
// so the same compaction over the union gives the whole segment's answer.  (No circle, no cap: rb_merge.)
#define RB_MERGE_CAT_KERNEL(name, NEAR, CAT)                                                                                   \
    __global__ __launch_bounds__(kRbThreads) void name(                                                                        \
        const uint32_t *first, const uint32_t *pfirst, const int64_t *seg_begin, const double *scores, int N,                  \
        const uint64_t *pk, const uint64_t *pid, const uint32_t *prow, const uint32_t *pcat, const int32_t *pcount,            \
        int64_t *out_ids, double *out_scores, int64_t *out_counts, RbNear nr, RbCat ct)                                        \
    {                                                                                                                          \
        rb_merge_body<NEAR, CAT>(first, pfirst, seg_begin, scores, N, pk, pid, prow, pcount, out_ids, out_scores, out_counts,  \
                                 nr, ct, pcat);                                                                                \
    }
RB_MERGE_CAT_KERNEL(rb_merge_cat_near, true, 1)
RB_MERGE_CAT_KERNEL(rb_merge_cap, false, 2)
RB_MERGE_CAT_KERNEL(rb_merge_cap_near, true, 2)
#undef RB_MERGE_CAT_KERNEL

// ---- the global path --------------------------------------------------------------------------------------------------

// kept rows of one work item
template <bool EX, bool NEAR, bool CAT = false>
__device__ __forceinline__ void rb_count_body(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                              const int64_t *seg_len, const int32_t *lo, const int32_t *hi,
                                              const uint64_t *table_ids, const int64_t *ids, int64_t chunk, uint32_t *cnt,
                                              uint32_t n_items, const uint32_t *xfirst, const uint64_t *xkeys, const RbNear &nr,
                                              const RbCat &ct = RbCat{})
{
    __shared__ uint32_t total;
    const uint32_t w = blockIdx.x;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    if (w == n_items) {  // the scan's last element
        if (threadIdx.x == 0) cnt[w] = 0;
        return;
    }
    const int64_t s = rb_segment_of(first, n_seg, w);
    const uint32_t nch = first[s + 1] - first[s], c = w - first[s];
    const int64_t begin = seg_begin[s], len = seg_len[s];
    const int32_t tlo = lo[s], thi = hi[s];
    const int64_t r0 = (int64_t)c * chunk;
    const int64_t r1 = thi > tlo ? min(len, nch == 1 ? len : r0 + chunk) : 0;
    uint32_t xa = 0, xb = 0;
    if constexpr (EX) {
        if (!(NEAR || CAT) || xkeys) {
            xa = xfirst[s];
            xb = xfirst[s + 1];
        }
    }
    RbCircle cir = {};
    if constexpr (NEAR) cir = rb_circle_of(nr, s);
    uint32_t aa = 0, ab = 0;
    if constexpr (CAT) rb_allow_range(ct, s, &aa, &ab);
    uint32_t mine = 0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kRbThreads) {
        const uint64_t key = ordered_key(ids[begin + r]);
        int32_t a = tlo, b = thi;
        while (a < b) {
            const int32_t mid = (int32_t)(((uint32_t)a + (uint32_t)b) >> 1);
            if (table_ids[mid] < key) a = mid + 1; else b = mid;
        }
        bool keep = a < thi && table_ids[a] == key;
        if constexpr (EX) keep = keep && !rb_excluded(xkeys, xa, xb, key);
        if constexpr (CAT) {
            uint32_t cr;
            keep = keep && rb_within_cat<NEAR>(nr, cir, ct, aa, ab, s, a, thi, key, nullptr, &cr);
        } else if constexpr (NEAR) {
            double d;
            keep = keep && (cir.all || rb_within(nr, cir, a, thi, key, &d));
        }
        if (keep) ++mine;
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) cnt[w] = total;
}

__global__ __launch_bounds__(kRbThreads) void rb_count(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                       const int64_t *seg_len, const int32_t *lo, const int32_t *hi,
                                                       const uint64_t *table_ids, const int64_t *ids, int64_t chunk,
                                                       uint32_t *cnt, uint32_t n_items)
{
    rb_count_body<false, false>(n_seg, first, seg_begin, seg_len, lo, hi, table_ids, ids, chunk, cnt, n_items, nullptr, nullptr,
                                RbNear{});
}

__global__ __launch_bounds__(kRbThreads) void rb_count_ex(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                          const int64_t *seg_len, const int32_t *lo, const int32_t *hi,
                                                          const uint64_t *table_ids, const int64_t *ids, int64_t chunk,
                                                          uint32_t *cnt, uint32_t n_items, const uint32_t *xfirst,
                                                          const uint64_t *xkeys)
{
    rb_count_body<true, false>(n_seg, first, seg_begin, seg_len, lo, hi, table_ids, ids, chunk, cnt, n_items, xfirst, xkeys, RbNear{});
}

__global__ __launch_bounds__(kRbThreads) void rb_count_near(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                            const int64_t *seg_len, const int64_t *ids, int64_t chunk,
                                                            uint32_t *cnt, uint32_t n_items, const uint32_t *xfirst,
                                                            const uint64_t *xkeys, RbNear nr)
{
    rb_count_body<true, true>(n_seg, first, seg_begin, seg_len, nr.lo, nr.hi, nr.table_ids, ids, chunk, cnt, n_items, xfirst, xkeys, nr);
}

__global__ __launch_bounds__(kRbThreads) void rb_count_cat(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                           const int64_t *seg_len, const int64_t *ids, int64_t chunk,
                                                           uint32_t *cnt, uint32_t n_items, const uint32_t *xfirst,
                                                           const uint64_t *xkeys, RbNear nr, RbCat ct)
{
    rb_count_body<true, false, true>(n_seg, first, seg_begin, seg_len, nr.lo, nr.hi, nr.table_ids, ids, chunk, cnt, n_items, xfirst,
                                     xkeys, nr, ct);
}

__global__ __launch_bounds__(kRbThreads) void rb_count_cat_near(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                                const int64_t *seg_len, const int64_t *ids, int64_t chunk,
                                                                uint32_t *cnt, uint32_t n_items, const uint32_t *xfirst,
                                                                const uint64_t *xkeys, RbNear nr, RbCat ct)
{
    rb_count_body<true, true, true>(n_seg, first, seg_begin, seg_len, nr.lo, nr.hi, nr.table_ids, ids, chunk, cnt, n_items, xfirst,
                                    xkeys, nr, ct);
}

// the kept rows of one work item, in row order, at base[w] ..: segment, row, id key, and the row's own position as the
// payload of the first sort (CAT, where kcat is given: the category's rank as well, for the caps)
template <bool EX, bool NEAR, bool CAT = false>
__device__ __forceinline__ void rb_scatter_body(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                const int64_t *seg_len, const int32_t *lo, const int32_t *hi,
                                                const uint64_t *table_ids, const int64_t *ids, int64_t chunk,
                                                const uint32_t *base, uint32_t *kseg, uint32_t *krow, uint64_t *keys,
                                                uint32_t *vals, const uint32_t *xfirst, const uint64_t *xkeys, const RbNear &nr,
                                                const RbCat &ct = RbCat{}, uint32_t *kcat = nullptr)
{
    __shared__ uint32_t wave_cnt[kRbThreads / 64];
    const uint32_t w = blockIdx.x;
    const int64_t s = rb_segment_of(first, n_seg, w);
    const uint32_t nch = first[s + 1] - first[s], c = w - first[s];
    const int64_t begin = seg_begin[s], len = seg_len[s];
    const int32_t tlo = lo[s], thi = hi[s];
    const int64_t r0 = (int64_t)c * chunk;
    const int64_t r1 = thi > tlo ? min(len, nch == 1 ? len : r0 + chunk) : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t xa = 0, xb = 0;
    if constexpr (EX) {
        if (!(NEAR || CAT) || xkeys) {
            xa = xfirst[s];
            xb = xfirst[s + 1];
        }
    }
    RbCircle cir = {};
    if constexpr (NEAR) cir = rb_circle_of(nr, s);
    uint32_t aa = 0, ab = 0;
    if constexpr (CAT) rb_allow_range(ct, s, &aa, &ab);
    uint32_t pos = base[w];
    for (int64_t t0 = r0; t0 < r1; t0 += kRbThreads) {
        const int64_t r = t0 + threadIdx.x;
        bool keep = false;
        uint64_t key = 0;
        [[maybe_unused]] uint32_t cr = 0;
        if (r < r1) {
            key = ordered_key(ids[begin + r]);
            int32_t a = tlo, b = thi;
            while (a < b) {
                const int32_t mid = (int32_t)(((uint32_t)a + (uint32_t)b) >> 1);
                if (table_ids[mid] < key) a = mid + 1; else b = mid;
            }
            keep = a < thi && table_ids[a] == key;
            if constexpr (EX) keep = keep && !rb_excluded(xkeys, xa, xb, key);
            if constexpr (CAT) {
                keep = keep && rb_within_cat<NEAR>(nr, cir, ct, aa, ab, s, a, thi, key, nullptr, &cr);
            } else if constexpr (NEAR) {
                double d;
                keep = keep && (cir.all || rb_within(nr, cir, a, thi, key, &d));
            }
        }
        const unsigned long long m = __ballot(keep);
        __syncthreads();  // the previous tile's wave_cnt has been read
        if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int v = 0; v < kRbThreads / 64; ++v) {
            if (v < wave) before += wave_cnt[v];
            all += wave_cnt[v];
        }
        if (keep) {
            const uint32_t p = pos + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            kseg[p] = (uint32_t)s;
            krow[p] = (uint32_t)r;
            keys[p] = key;
            vals[p] = p;
            if constexpr (CAT) {
                if (kcat) kcat[p] = cr;
            }
        }
        pos += all;
    }
}

__global__ __launch_bounds__(kRbThreads) void rb_scatter(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                         const int64_t *seg_len, const int32_t *lo, const int32_t *hi,
                                                         const uint64_t *table_ids, const int64_t *ids, int64_t chunk,
                                                         const uint32_t *base, uint32_t *kseg, uint32_t *krow,
                                                         uint64_t *keys, uint32_t *vals)
{
    rb_scatter_body<false, false>(n_seg, first, seg_begin, seg_len, lo, hi, table_ids, ids, chunk, base, kseg, krow, keys, vals,
                                  nullptr, nullptr, RbNear{});
}

__global__ __launch_bounds__(kRbThreads) void rb_scatter_ex(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                            const int64_t *seg_len, const int32_t *lo, const int32_t *hi,
                                                            const uint64_t *table_ids, const int64_t *ids, int64_t chunk,
                                                            const uint32_t *base, uint32_t *kseg, uint32_t *krow,
                                                            uint64_t *keys, uint32_t *vals, const uint32_t *xfirst,
                                                            const uint64_t *xkeys)
{
    rb_scatter_body<true, false>(n_seg, first, seg_begin, seg_len, lo, hi, table_ids, ids, chunk, base, kseg, krow, keys, vals, xfirst,
                                 xkeys, RbNear{});
}

__global__ __launch_bounds__(kRbThreads) void rb_scatter_near(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                              const int64_t *seg_len, const int64_t *ids, int64_t chunk,
                                                              const uint32_t *base, uint32_t *kseg, uint32_t *krow,
                                                              uint64_t *keys, uint32_t *vals, const uint32_t *xfirst,
                                                              const uint64_t *xkeys, RbNear nr)
{
    rb_scatter_body<true, true>(n_seg, first, seg_begin, seg_len, nr.lo, nr.hi, nr.table_ids, ids, chunk, base, kseg, krow, keys, vals,
                                xfirst, xkeys, nr);
}

__global__ __launch_bounds__(kRbThreads) void rb_scatter_cat(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                             const int64_t *seg_len, const int64_t *ids, int64_t chunk,
                                                             const uint32_t *base, uint32_t *kseg, uint32_t *krow,
                                                             uint64_t *keys, uint32_t *vals, uint32_t *kcat,
                                                             const uint32_t *xfirst, const uint64_t *xkeys, RbNear nr, RbCat ct)
{
    rb_scatter_body<true, false, true>(n_seg, first, seg_begin, seg_len, nr.lo, nr.hi, nr.table_ids, ids, chunk, base, kseg, krow, keys,
                                       vals, xfirst, xkeys, nr, ct, kcat);
}

__global__ __launch_bounds__(kRbThreads) void rb_scatter_cat_near(int64_t n_seg, const uint32_t *first, const int64_t *seg_begin,
                                                                  const int64_t *seg_len, const int64_t *ids, int64_t chunk,
                                                                  const uint32_t *base, uint32_t *kseg, uint32_t *krow,
                                                                  uint64_t *keys, uint32_t *vals, uint32_t *kcat,
                                                                  const uint32_t *xfirst, const uint64_t *xkeys, RbNear nr,
                                                                  RbCat ct)
{
    rb_scatter_body<true, true, true>(n_seg, first, seg_begin, seg_len, nr.lo, nr.hi, nr.table_ids, ids, chunk, base, kseg, krow, keys,
                                      vals, xfirst, xkeys, nr, ct, kcat);
}

__global__ void rb_score_keys(int64_t m, const uint32_t *vals, const uint32_t *kseg, const uint32_t *krow,
                              const int64_t *seg_begin, const double *scores, uint64_t *keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t v = vals[i];
    keys[i] = score_desc_key(scores[seg_begin[kseg[v]] + krow[v]]);
}

__global__ void rb_segment_keys(int64_t m, const uint32_t *vals, const uint32_t *kseg, uint32_t *keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) keys[i] = kseg[vals[i]];
}

// output row s, slots [256 jt, 256 jt + 256): the first N of the segment's run in the sorted rows, then the padding
template <bool NEAR, bool CAT = false>
__device__ __forceinline__ void rb_emit_sorted_body(int64_t tiles, int64_t N, int64_t m, const uint32_t *seg_sorted,
                                                    const uint32_t *vals, const uint32_t *krow, const int64_t *seg_begin,
                                                    const int64_t *ids, const double *scores, int64_t *out_ids,
                                                    double *out_scores, int64_t *out_counts, const RbNear &nr,
                                                    const RbCat &ct = RbCat{})
{
    __shared__ int64_t range[2];
    const int64_t s = blockIdx.x / tiles, jt = blockIdx.x % tiles;
    if (threadIdx.x < 2) {  // lower bound of s and of s + 1
        const uint64_t want = (uint64_t)s + threadIdx.x;
        int64_t a = 0, b = m;
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if ((uint64_t)seg_sorted[mid] < want) a = mid + 1; else b = mid;
        }
        range[threadIdx.x] = a;
    }
    __syncthreads();
    const int64_t lb = range[0], have = range[1] - range[0];
    const int64_t j = jt * kRbThreads + threadIdx.x;
    if (j < N) {
        const int64_t o = s * N + j;
        if (j < have) {
            const int64_t r = seg_begin[s] + krow[vals[lb + j]];
            out_ids[o] = ids[r];
            out_scores[o] = scores[r];
            if constexpr (NEAR && CAT) {
                if (nr.meters) nr.meters[o] = rb_meters_of_cat(nr, rb_circle_of(nr, s), ct, s, ordered_key(ids[r]));
            } else if constexpr (NEAR) {
                if (nr.meters) nr.meters[o] = rb_meters_of(nr, rb_circle_of(nr, s), s, ordered_key(ids[r]));
            }
        } else {
            out_ids[o] = -1;
            out_scores[o] = 0.0;
            if constexpr (NEAR) {
                if (nr.meters) nr.meters[o] = 0.0;
            }
        }
    }
    if (jt == 0 && threadIdx.x == 0) out_counts[s] = min(have, N);
}

__global__ __launch_bounds__(kRbThreads) void rb_emit_sorted(int64_t tiles, int64_t N, int64_t m, const uint32_t *seg_sorted,
                                                             const uint32_t *vals, const uint32_t *krow,
                                                             const int64_t *seg_begin, const int64_t *ids,
                                                             const double *scores, int64_t *out_ids, double *out_scores,
                                                             int64_t *out_counts)
{
    rb_emit_sorted_body<false>(tiles, N, m, seg_sorted, vals, krow, seg_begin, ids, scores, out_ids, out_scores, out_counts, RbNear{});
}

__global__ __launch_bounds__(kRbThreads) void rb_emit_sorted_near(int64_t tiles, int64_t N, int64_t m, const uint32_t *seg_sorted,
                                                                  const uint32_t *vals, const uint32_t *krow,
                                                                  const int64_t *seg_begin, const int64_t *ids,
                                                                  const double *scores, int64_t *out_ids, double *out_scores,
                                                                  int64_t *out_counts, RbNear nr)
{
    rb_emit_sorted_body<true>(tiles, N, m, seg_sorted, vals, krow, seg_begin, ids, scores, out_ids, out_scores, out_counts, nr);
}

__global__ __launch_bounds__(kRbThreads) void rb_emit_sorted_cat_near(int64_t tiles, int64_t N, int64_t m, const uint32_t *seg_sorted,
                                                                      const uint32_t *vals, const uint32_t *krow,
                                                                      const int64_t *seg_begin, const int64_t *ids,
                                                                      const double *scores, int64_t *out_ids, double *out_scores,
                                                                      int64_t *out_counts, RbNear nr, RbCat ct)
{
    rb_emit_sorted_body<true, true>(tiles, N, m, seg_sorted, vals, krow, seg_begin, ids, scores, out_ids, out_scores, out_counts, nr, ct);
}

// ---- the global path with caps -----------------------------------------------------------------------------------------
// After the three passes position i of the sorted rows is row vals[i] of the scatter, in the output order of its segment.
// One more stable pass orders the positions by (segment, category): a position with `cap` positions of its run in front
// of it is over the cap; the others are flagged, the flags summed in sorted order, and a flagged row whose sum minus
// its segment's is below N is output row that number.

// keys[i] = (segment << 32 | category rank) of sorted position i, pos[i] = i
__global__ void rb_cap_keys(int64_t m, const uint32_t *seg_sorted, const uint32_t *vals, const uint32_t *kcat, uint64_t *keys,
                            uint32_t *pos)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    keys[i] = ((uint64_t)seg_sorted[i] << 32) | kcat[vals[i]];
    pos[i] = (uint32_t)i;
}

// flag[pos[t]] = entry t of the (segment, category) order has fewer than its segment's cap entries of its run in front
// of it (entry t - cap is of another run); flag[m] = 0, the scan's last element
__global__ void rb_cap_flags(int64_t m, const uint64_t *keys, const uint32_t *pos, const int64_t *caps, int64_t N, uint32_t *flag)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) flag[m] = 0;
    if (t >= m) return;
    const uint64_t key = keys[t];
    const int64_t cap = min(N, caps[key >> 32]);
    flag[pos[t]] = t >= cap && keys[t - cap] == key ? 0u : 1u;
}

// the first sorted position of segment s (m: none)
__device__ __forceinline__ int64_t rb_segment_lower(const uint32_t *seg_sorted, int64_t m, uint64_t s)
{
    int64_t a = 0, b = m;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if ((uint64_t)seg_sorted[mid] < s) a = mid + 1; else b = mid;
    }
    return a;
}

// the flagged rows to their output rows; the circle is read at run time (nr.meters NULL: no out_meters)
__global__ __launch_bounds__(kRbThreads) void rb_emit_capped(int64_t N, int64_t m, const uint32_t *seg_sorted, const uint32_t *vals,
                                                             const uint32_t *krow, const uint32_t *flag, const uint32_t *fsum,
                                                             const int64_t *seg_begin, const int64_t *ids, const double *scores,
                                                             int64_t *out_ids, double *out_scores, RbNear nr, RbCat ct)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || !flag[i]) return;
    const int64_t s = seg_sorted[i];
    const int64_t j = (int64_t)(fsum[i] - fsum[rb_segment_lower(seg_sorted, m, (uint64_t)s)]);
    if (j >= N) return;
    const int64_t o = s * N + j, r = seg_begin[s] + krow[vals[i]];
    out_ids[o] = ids[r];
    out_scores[o] = scores[r];
    if (nr.meters) nr.meters[o] = rb_meters_of_cat(nr, rb_circle_of(nr, s), ct, s, ordered_key(ids[r]));
}

// output row s, slots [256 jt, 256 jt + 256): the padding behind the segment's flagged rows, and the count
__global__ __launch_bounds__(kRbThreads) void rb_pad_capped(int64_t tiles, int64_t N, int64_t m, const uint32_t *seg_sorted,
                                                            const uint32_t *fsum, int64_t *out_ids, double *out_scores,
                                                            double *out_meters, int64_t *out_counts)
{
    __shared__ int64_t range[2];
    const int64_t s = blockIdx.x / tiles, jt = blockIdx.x % tiles;
    if (threadIdx.x < 2) range[threadIdx.x] = rb_segment_lower(seg_sorted, m, (uint64_t)s + threadIdx.x);
    __syncthreads();
    const int64_t have = (int64_t)(fsum[range[1]] - fsum[range[0]]);
    const int64_t j = jt * kRbThreads + threadIdx.x;
    if (j < N && j >= have) {
        out_ids[s * N + j] = -1;
        out_scores[s * N + j] = 0.0;
        if (out_meters) out_meters[s * N + j] = 0.0;
    }
    if (jt == 0 && threadIdx.x == 0) out_counts[s] = min(have, N);
}

// ---- the categories' tables --------------------------------------------------------------------------------------------
// The place table's categories as dense ranks: one stable sort of the category keys with the input rows as values, run
// heads, their inclusive sum (the rank of every sorted position) and a scatter back through the sort's values.

__global__ void rb_cat_heads(int64_t np, const uint64_t *sorted, uint32_t *heads)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < np) heads[i] = i > 0 && sorted[i] != sorted[i - 1] ? 1u : 0u;
}

__global__ void rb_cat_scatter(int64_t np, const uint32_t *ranks, const uint32_t *rows, uint32_t *crank)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < np) crank[rows[i]] = ranks[i];
}

// The lists' and the caps' requires, in the plan step: hdr[0] gets bit 4 for a cap below 1 and bit 5 for a list outside
// [0, n_allowed] (or *allow_invalid, the verdict on the public entry's offsets); hdr[5] the lists' entries, hdr[6] whether
// some cap is below N; alen (NULL: not wanted) the lengths as the pair table's scan wants them.  Reads the ranges only.
__global__ void rb_check_cat(int64_t n_seg, const int64_t *allow_begin, const int64_t *allow_len, int64_t n_allowed,
                             const int64_t *caps, int64_t N, const unsigned long long *allow_invalid, uint32_t *alen,
                             unsigned long long *hdr)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0 && allow_invalid && *allow_invalid) atomicOr(&hdr[0], 32ull);
    if (s > n_seg) return;
    if (s == n_seg) {
        if (allow_begin && alen) alen[s] = 0;
        return;
    }
    if (allow_begin) {
        const int64_t b = allow_begin[s], l = allow_len[s];
        const bool ok = b >= 0 && l >= 0 && l <= n_allowed && b <= n_allowed - l;
        if (alen) alen[s] = ok ? (uint32_t)l : 0u;  // (n_allowed < 2^31)
        if (ok && l > 0) atomicAdd(&hdr[5], (unsigned long long)l);
        if (!ok) atomicOr(&hdr[0], 32ull);
    }
    if (caps) {
        if (caps[s] < 1) atomicOr(&hdr[0], 16ull);
        else if (caps[s] < N) atomicOr(&hdr[6], 1ull);
    }
}

// pair p of the unsorted allow table, as rb_expand_excluded: (segment << 32 | the listed category's rank); a category
// that no place has gets the rank ~0, which no place row carries
__global__ void rb_expand_allowed(int64_t n_seg, int64_t total, const uint32_t *afirst, const int64_t *allow_begin,
                                  const int64_t *allow_ids, int64_t np, const uint64_t *cat_sorted, const uint32_t *cat_ranks,
                                  uint64_t *keys)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const int64_t s = rb_segment_of(afirst, n_seg, (uint32_t)p);
    const uint64_t key = ordered_key(allow_ids[allow_begin[s] + (p - (int64_t)afirst[s])]);
    const int64_t at = lower_bound_key(cat_sorted, np, key);
    const uint32_t rank = at < np && cat_sorted[at] == key ? cat_ranks[at] : ~0u;
    keys[p] = ((uint64_t)s << 32) | rank;
}

// the refusal of rb_check_cat's bits, naming the argument
int32_t rb_cat_refusal(unsigned long long bits)
{
    if (bits & 16ull) return fail(LOCREC_E_INVALID_ARG, "max_per_category must be >= 1 for every segment");
    return fail(LOCREC_E_INVALID_ARG, "allowed_offsets must be non-decreasing inside [0, n_allowed]");
}

// The circles' and the place table's requires, in the plan step before any row is read: a radius that is NaN or below 0
// (bit 1 of *flags), a centre (bit 2) or a place row (bit 3) that fails Location's require.
__global__ void rb_check_near(int64_t n_seg, const double *clat, const double *clon, const double *rad, int64_t np,
                              const double *plat, const double *plon, unsigned long long *flags)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bad = 0;
    if (i < n_seg) {
        if (!(rad[i] >= 0.0)) bad |= 2ull;
        if (!location_ok(clat[i], clon[i])) bad |= 4ull;
    }
    if (i < np && !location_ok(plat[i], plon[i])) bad |= 8ull;
    if (bad) atomicOr(flags, bad);
}

// the refusal of rb_check_near's bits, naming the argument
int32_t rb_near_refusal(unsigned long long bits)
{
    if (bits & 2ull) return fail(LOCREC_E_INVALID_ARG, "radius_meters must be >= 0 (or +inf) and not NaN");
    if (bits & 4ull)
        return fail(LOCREC_E_INVALID_ARG, "center_latitudes must be within [-90.0, 90.0] and center_longitudes within [-180.0, 180.0]");
    return fail(LOCREC_E_INVALID_ARG, "place_latitudes must be within [-90.0, 90.0] and place_longitudes within [-180.0, 180.0]");
}

// the internal entries; ex_begin NULL: no lists; nq NULL: no circle (out_meters unused)
int32_t rank_segments(int64_t n_seg, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids, const double *scores,
                      int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
                      const int64_t *target_region_ids, int64_t max_recommendations, const int64_t *ex_begin,
                      const int64_t *ex_len, int64_t n_excluded, const int64_t *ex_ids, int64_t *out_ids, double *out_scores,
                      int64_t *out_counts, const unsigned long long *invalid_flag, int64_t host_assembled, hipStream_t s,
                      const RankNear *nq = nullptr, double *out_meters = nullptr, const RankCategory *cq = nullptr)
{
    RankBatchStats &st = rank_batch_stats();
    st = RankBatchStats();
    st.host_assembled = host_assembled;
    if (n_seg < 0 || n_seg >= kMaxRows || n_places < 0 || n_places >= kMaxRows)
        return fail(LOCREC_E_INVALID_ARG, "segment or place count out of range [0, 2^31)");
    if (ex_begin && (n_excluded < 0 || n_excluded >= kMaxRows))
        return fail(LOCREC_E_INVALID_ARG, "excluded id count out of range [0, 2^31)");
    if (cq && cq->allow_begin && (cq->n_allowed < 0 || cq->n_allowed >= kMaxRows))
        return fail(LOCREC_E_INVALID_ARG, "n_allowed out of range [0, 2^31)");
    if (n_seg == 0) return LOCREC_OK;
    const int64_t N = std::max<int64_t>(0, max_recommendations);
    if (N > 0 && n_seg > ((int64_t)1 << 60) / N) return fail(LOCREC_E_INVALID_ARG, "n_segments * max_recommendations overflows");
    if (N == 0) {  // limit(n <= 0) is empty: the caller's verdict on the offsets, the counts, nothing else
        unsigned long long bad = 0;
        if (invalid_flag) {
            LOCREC_READ_BACK(bad, invalid_flag, s);
            ++st.host_syncs;
        }
        if ((nq || cq) && !bad) {  // ... and the circles', the lists' and the caps' requires, in one read-back
            DevBuf<unsigned long long> flags;
            LOCREC_TRY(flags.alloc(7));
            LOCREC_HIP_TRY(hipMemsetAsync(flags.p, 0, 7 * sizeof(unsigned long long), s));
            if (nq)
                LOCREC_LAUNCH(rb_check_near, grid_for(std::max(n_seg, n_places)), dim3(256), 0, s, n_seg, nq->center_lat,
                              nq->center_lon, nq->radius, n_places, nq->place_lat, nq->place_lon, flags.p);
            if (cq)
                LOCREC_LAUNCH(rb_check_cat, grid_for(n_seg + 1), dim3(256), 0, s, n_seg, cq->allow_begin, cq->allow_len,
                              cq->n_allowed, cq->caps, N, cq->allow_invalid, (uint32_t *)nullptr, flags.p);
            unsigned long long bits = 0;
            LOCREC_READ_BACK(bits, flags.p, s);
            ++st.host_syncs;
            if (bits & 48ull) return rb_cat_refusal(bits);
            if (bits) return rb_near_refusal(bits);
        }
        if (bad) return fail(LOCREC_E_INVALID_ARG, "segments must be non-decreasing offsets inside [0, n]");
        LOCREC_HIP_TRY(hipMemsetAsync(out_counts, 0, (size_t)n_seg * sizeof(int64_t), s));
        return LOCREC_OK;
    }
    const int64_t chunk = rb_chunk_rows();
    const bool global = N > LOCREC_RANK_BATCH_MAX_N || rb_force_sort();
    Temp tmp;
    // the region table: (region, place id) sorted - two stable passes, by id and then by region
    // (one allocation each for the table and the plan: every hipMalloc / hipFree of a call costs a wait)
    DevBuf<uint64_t> table, plan;
    uint64_t *k0 = nullptr, *k1 = nullptr;
    if (n_places > 0) {
        const size_t np8 = ((size_t)n_places + 1) / 2;  // u32[n_places] in 8-byte units
        LOCREC_TRY(table.alloc(2 * (size_t)n_places + 2 * np8));
        k0 = table.p;
        k1 = k0 + n_places;
        uint32_t *r0 = reinterpret_cast<uint32_t *>(k1 + n_places), *r1 = r0 + 2 * np8;
        LOCREC_LAUNCH(iota_keys, grid_for(n_places), dim3(256), 0, s, n_places, place_ids, k0, r0);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0, k1, r0, r1, (int)n_places, 0, 64, s));
        LOCREC_LAUNCH(gather_id_keys, grid_for(n_places), dim3(256), 0, s, n_places, place_region_ids, r1, k0);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0, k1, r1, r0, (int)n_places, 0, 64, s));
        LOCREC_LAUNCH(gather_id_keys, grid_for(n_places), dim3(256), 0, s, n_places, place_ids, r0, k0);
    }
    const uint64_t *table_regions = k1, *table_ids = k0;
    // (table position t is input row trow[t]: the second pass's values, in r0 - what leads a listing to its coordinates)
    const uint32_t *trow = n_places > 0 ? reinterpret_cast<const uint32_t *>(k1 + n_places) : nullptr;
    // the plan: every segment's range of the table and its chunks
    const size_t seg8 = ((size_t)n_seg + 2) / 2;  // u32[n_seg + 1] in 8-byte units
    const size_t hw = cq ? 8 : 5;  // header words: with categories [5] the allow-lists' entries, [6] some cap below N
    LOCREC_TRY(plan.alloc(hw + (cq ? 10 : ex_begin ? 8 : 6) * seg8));
    struct {
        unsigned long long *p;
    } hdr = {reinterpret_cast<unsigned long long *>(plan.p)};
    struct U32 {
        uint32_t *p;
    } nch = {reinterpret_cast<uint32_t *>(plan.p + hw)}, split_nch = {nch.p + 2 * seg8}, first = {nch.p + 4 * seg8},
      pfirst = {nch.p + 6 * seg8}, xlen = {nch.p + 12 * seg8}, xfirst = {nch.p + 14 * seg8},  // x*: only with lists
      alen = {nch.p + 16 * seg8}, afirst = {nch.p + 18 * seg8};                               // a*: only with categories
    struct {
        int32_t *p;
    } lo = {reinterpret_cast<int32_t *>(nch.p + 8 * seg8)}, hi = {lo.p + 2 * seg8};
    LOCREC_HIP_TRY(hipMemsetAsync(hdr.p, 0, hw * sizeof(unsigned long long), s));
    LOCREC_LAUNCH(rb_plan, grid_for(n_seg + 1), dim3(256), 0, s, n_seg, seg_begin, seg_len, target_region_ids, n_places,
                  table_regions, chunk, invalid_flag, nch.p, split_nch.p, lo.p, hi.p, hdr.p, ex_begin, ex_len, n_excluded,
                  xlen.p);
    if (nq)
        LOCREC_LAUNCH(rb_check_near, grid_for(std::max(n_seg, n_places)), dim3(256), 0, s, n_seg, nq->center_lat, nq->center_lon,
                      nq->radius, n_places, nq->place_lat, nq->place_lon, hdr.p);
    if (cq)
        LOCREC_LAUNCH(rb_check_cat, grid_for(n_seg + 1), dim3(256), 0, s, n_seg, cq->allow_begin, cq->allow_len, cq->n_allowed,
                      cq->caps, N, cq->allow_invalid, alen.p, hdr.p);
    unsigned long long h[7] = {0, 0, 0, 0, 0, 0, 0};  // (the fifth word travels only when there are lists, two more with categories)
    LOCREC_HIP_TRY(hipMemcpyAsync(h, hdr.p, (cq ? 7 : ex_begin ? 5 : 4) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    ++st.host_syncs;
    if (h[0] & 48ull) return rb_cat_refusal(h[0]);
    if (h[0] & ~1ull) return rb_near_refusal(h[0]);
    if (h[0])
        return fail(LOCREC_E_INVALID_ARG, ex_begin ? "segments and exclusion lists must be non-decreasing offsets inside their "
                                                     "arrays, each segment shorter than 2^31 rows"
                                                   : "segments must be non-decreasing offsets inside [0, n], each shorter than 2^31 rows");
    if (h[1] >= (unsigned long long)kMaxRows - 1)
        return fail(LOCREC_E_INVALID_ARG, "%llu chunks: raise LOCREC_RANK_BATCH_CHUNK or split the batch", h[1]);
    if (h[4] >= (unsigned long long)kMaxRows) return fail(LOCREC_E_INVALID_ARG, "2^31 excluded ids or more in all: split the batch");
    if (h[5] >= (unsigned long long)kMaxRows) return fail(LOCREC_E_INVALID_ARG, "2^31 allowed categories or more in all: split the batch");
    const uint32_t items = (uint32_t)h[1];
    // no list entry and every cap N or more: the existing kernels, and the plain / excluding / near call's result and stats
    const bool capped = cq && h[6] != 0, cat = cq && (h[5] > 0 || capped);
    RbNear nr = {};
    if (nq) nr = {nq->center_lat, nq->center_lon, nq->radius, nq->place_lat, nq->place_lon, trow, lo.p, hi.p, table_ids, out_meters};
    else if (cat) nr = {nullptr, nullptr, nullptr, nullptr, nullptr, trow, lo.p, hi.p, table_ids, nullptr};
    LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, nch.p, first.p, (size_t)n_seg + 1, s));
    // the pair table of the exclusion lists (every list empty: the plain kernels, and the plain call's result and stats)
    const int64_t n_pairs = (int64_t)h[4];
    DevBuf<uint64_t> pairs;
    const uint64_t *xkeys = nullptr;
    if (n_pairs > 0) {
        // one allocation for the two sorts' temporary storage (in front: aligned) and the pairs: the table costs the call
        // one hipMalloc and one hipFree, and `tmp`, sized by the region table, is not grown for it
        const size_t xp8 = ((size_t)n_pairs + 1) / 2;  // u32[n_pairs] in 8-byte units
        int seg_bits = 1;
        while (seg_bits < 32 && ((int64_t)1 << seg_bits) < n_seg) ++seg_bits;
        uint64_t *x0 = nullptr, *x1 = nullptr;
        uint32_t *g0 = nullptr, *g1 = nullptr;
        size_t bytes_id = 0, bytes_seg = 0;
        LOCREC_HIP_TRY(prim::sort_pairs(nullptr, bytes_id, x0, x1, g0, g1, (size_t)n_pairs, 0, 64, s));
        LOCREC_HIP_TRY(prim::sort_pairs(nullptr, bytes_seg, g1, g0, x1, x0, (size_t)n_pairs, 0, seg_bits, s));
        const size_t temp8 = (std::max(bytes_id, bytes_seg) + 256) / 256 * 32;  // whole 256-byte lines, at least one
        LOCREC_TRY(pairs.alloc(temp8 + 2 * (size_t)n_pairs + 2 * xp8));
        x0 = pairs.p + temp8;
        x1 = x0 + n_pairs;
        g0 = reinterpret_cast<uint32_t *>(x1 + n_pairs);
        g1 = g0 + 2 * xp8;
        LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, xlen.p, xfirst.p, (size_t)n_seg + 1, s));
        LOCREC_LAUNCH(rb_expand_excluded, grid_for(n_pairs), dim3(256), 0, s, n_seg, n_pairs, xfirst.p, ex_begin, ex_ids, x0, g0);
        // two stable passes: id, segment
        LOCREC_HIP_TRY(prim::sort_pairs(pairs.p, bytes_id, x0, x1, g0, g1, (size_t)n_pairs, 0, 64, s));
        LOCREC_HIP_TRY(prim::sort_pairs(pairs.p, bytes_seg, g1, g0, x1, x0, (size_t)n_pairs, 0, seg_bits, s));
        xkeys = x0;
    }
    // the categories' tables, only for a call that takes this path: the place rows' dense ranks, then the allow-lists as
    // (segment, rank) keys - the exclusion table's mould with one key and one sort, sharing its allocation trick
    DevBuf<uint64_t> ctab, apairs;
    RbCat ct = {};
    if (cat) {
        const size_t npz = (size_t)n_places, np8 = (npz + 1) / 2;
        LOCREC_TRY(ctab.alloc(std::max<size_t>(1, 2 * npz + 5 * np8)));
        uint64_t *c0 = ctab.p, *c1 = c0 + npz;
        uint32_t *v0 = reinterpret_cast<uint32_t *>(c1 + npz), *v1 = v0 + 2 * np8, *heads = v1 + 2 * np8, *ranks = heads + 2 * np8,
                 *crank = ranks + 2 * np8;
        if (n_places > 0) {
            LOCREC_LAUNCH(iota_keys, grid_for(n_places), dim3(256), 0, s, n_places, cq->place_cat, c0, v0);
            LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, c0, c1, v0, v1, (int)n_places, 0, 64, s));
            LOCREC_LAUNCH(rb_cat_heads, grid_for(n_places), dim3(256), 0, s, n_places, c1, heads);
            LOCREC_PRIM(tmp, prim::inclusive_sum(p_, bytes_, heads, ranks, npz, s));
            LOCREC_LAUNCH(rb_cat_scatter, grid_for(n_places), dim3(256), 0, s, n_places, ranks, v1, crank);
        }
        ct = {crank, nullptr, nullptr, capped ? cq->caps : nullptr};
        const int64_t n_allow = (int64_t)h[5];
        if (n_allow > 0) {
            int key_bits = 33;
            while (key_bits < 64 && ((int64_t)1 << (key_bits - 32)) < n_seg) ++key_bits;
            uint64_t *a0 = nullptr, *a1 = nullptr;
            size_t bytes_a = 0;
            LOCREC_HIP_TRY(prim::sort_keys(nullptr, bytes_a, a0, a1, (size_t)n_allow, 0, key_bits, s));
            const size_t temp8 = (bytes_a + 256) / 256 * 32;
            LOCREC_TRY(apairs.alloc(temp8 + 2 * (size_t)n_allow));
            a0 = apairs.p + temp8;
            a1 = a0 + n_allow;
            LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, alen.p, afirst.p, (size_t)n_seg + 1, s));
            LOCREC_LAUNCH(rb_expand_allowed, grid_for(n_allow), dim3(256), 0, s, n_seg, n_allow, afirst.p, cq->allow_begin,
                          cq->allow_ids, n_places, c1, ranks, a0);
            LOCREC_HIP_TRY(prim::sort_keys(apairs.p, bytes_a, a0, a1, (size_t)n_allow, 0, key_bits, s));
            ct.afirst = afirst.p;
            ct.akeys = a1;
        }
    }
    if (!global) {
        st.split = (int64_t)h[2];
        st.chunks = (int64_t)h[3];
        st.one_block = n_seg - st.split;
        DevBuf<uint64_t> partial;  // the split segments' lists: keys, ids, rows, counts
        struct {
            uint64_t *p = nullptr;
        } pk, pid;
        struct {
            uint32_t *p = nullptr;
        } prow;
        struct {
            int32_t *p = nullptr;
        } pcount;
        uint32_t *pcat = nullptr;  // (the capped lists' categories)
        if (h[3] > 0) {
            LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, split_nch.p, pfirst.p, (size_t)n_seg + 1, s));
            const size_t pn = (size_t)h[3] * (size_t)N, pn8 = (pn + 1) / 2, pc8 = ((size_t)h[3] + 1) / 2;
            LOCREC_TRY(partial.alloc(2 * pn + pn8 + pc8 + (capped ? pn8 : 0)));
            pk.p = partial.p;
            pid.p = pk.p + pn;
            prow.p = reinterpret_cast<uint32_t *>(pid.p + pn);
            pcount.p = reinterpret_cast<int32_t *>(pid.p + pn + pn8);
            if (capped) pcat = reinterpret_cast<uint32_t *>(pid.p + pn + pn8 + pc8);
        }
        if (cat) {
            const uint32_t *xf = xkeys ? xfirst.p : nullptr;
            if (capped && nq)
                LOCREC_LAUNCH(rb_select_cap_near, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, pfirst.p, seg_begin, seg_len,
                              ids, scores, chunk, (int)N, pk.p, pid.p, prow.p, pcat, pcount.p, out_ids, out_scores, out_counts, xf,
                              xkeys, nr, ct);
            else if (capped)
                LOCREC_LAUNCH(rb_select_cap, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, pfirst.p, seg_begin, seg_len, ids,
                              scores, chunk, (int)N, pk.p, pid.p, prow.p, pcat, pcount.p, out_ids, out_scores, out_counts, xf, xkeys,
                              nr, ct);
            else if (nq)
                LOCREC_LAUNCH(rb_select_cat_near, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, pfirst.p, seg_begin, seg_len,
                              ids, scores, chunk, (int)N, pk.p, pid.p, prow.p, pcat, pcount.p, out_ids, out_scores, out_counts, xf,
                              xkeys, nr, ct);
            else
                LOCREC_LAUNCH(rb_select_cat, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, pfirst.p, seg_begin, seg_len, ids,
                              scores, chunk, (int)N, pk.p, pid.p, prow.p, pcat, pcount.p, out_ids, out_scores, out_counts, xf, xkeys,
                              nr, ct);
            if (h[3] > 0 && capped && nq)
                LOCREC_LAUNCH(rb_merge_cap_near, dim3((unsigned)n_seg), dim3(kRbThreads), 0, s, first.p, pfirst.p, seg_begin, scores,
                              (int)N, pk.p, pid.p, prow.p, pcat, pcount.p, out_ids, out_scores, out_counts, nr, ct);
            else if (h[3] > 0 && capped)
                LOCREC_LAUNCH(rb_merge_cap, dim3((unsigned)n_seg), dim3(kRbThreads), 0, s, first.p, pfirst.p, seg_begin, scores,
                              (int)N, pk.p, pid.p, prow.p, pcat, pcount.p, out_ids, out_scores, out_counts, nr, ct);
            else if (h[3] > 0 && nq)
                LOCREC_LAUNCH(rb_merge_cat_near, dim3((unsigned)n_seg), dim3(kRbThreads), 0, s, first.p, pfirst.p, seg_begin, scores,
                              (int)N, pk.p, pid.p, prow.p, pcat, pcount.p, out_ids, out_scores, out_counts, nr, ct);
            else if (h[3] > 0)
                LOCREC_LAUNCH(rb_merge, dim3((unsigned)n_seg), dim3(kRbThreads), 0, s, first.p, pfirst.p, seg_begin, scores,
                              (int)N, pk.p, pid.p, prow.p, pcount.p, out_ids, out_scores, out_counts);
            return LOCREC_OK;
        }
        if (nq)
            LOCREC_LAUNCH(rb_select_near, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, pfirst.p, seg_begin, seg_len, ids,
                          scores, chunk, (int)N, pk.p, pid.p, prow.p, pcount.p, out_ids, out_scores, out_counts,
                          xkeys ? xfirst.p : nullptr, xkeys, nr);
        else if (xkeys)
            LOCREC_LAUNCH(rb_select_ex, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, pfirst.p, seg_begin, seg_len, lo.p,
                          hi.p, table_ids, ids, scores, chunk, (int)N, pk.p, pid.p, prow.p, pcount.p, out_ids, out_scores,
                          out_counts, xfirst.p, xkeys);
        else
            LOCREC_LAUNCH(rb_select, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, pfirst.p, seg_begin, seg_len, lo.p,
                          hi.p, table_ids, ids, scores, chunk, (int)N, pk.p, pid.p, prow.p, pcount.p, out_ids, out_scores,
                          out_counts);
        if (h[3] > 0 && nq)
            LOCREC_LAUNCH(rb_merge_near, dim3((unsigned)n_seg), dim3(kRbThreads), 0, s, first.p, pfirst.p, seg_begin, scores,
                          (int)N, pk.p, pid.p, prow.p, pcount.p, out_ids, out_scores, out_counts, nr);
        else if (h[3] > 0)
            LOCREC_LAUNCH(rb_merge, dim3((unsigned)n_seg), dim3(kRbThreads), 0, s, first.p, pfirst.p, seg_begin, scores,
                          (int)N, pk.p, pid.p, prow.p, pcount.p, out_ids, out_scores, out_counts);
        // (the partial lists are freed below: hipFree waits for the kernels that read them)
        return LOCREC_OK;
    }
    // the global path
    st.sorted = n_seg;
    const int64_t tiles = (N + kRbThreads - 1) / kRbThreads;
    if (n_seg * tiles >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "n_segments * max_recommendations too large for one call");
    DevBuf<uint32_t> cnt, base;
    LOCREC_TRY(cnt.alloc((size_t)items + 1));
    LOCREC_TRY(base.alloc((size_t)items + 1));
    if (cat && nq)
        LOCREC_LAUNCH(rb_count_cat_near, dim3(items + 1), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, ids, chunk,
                      cnt.p, items, xkeys ? xfirst.p : nullptr, xkeys, nr, ct);
    else if (cat)
        LOCREC_LAUNCH(rb_count_cat, dim3(items + 1), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, ids, chunk, cnt.p,
                      items, xkeys ? xfirst.p : nullptr, xkeys, nr, ct);
    else if (nq)
        LOCREC_LAUNCH(rb_count_near, dim3(items + 1), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, ids, chunk, cnt.p,
                      items, xkeys ? xfirst.p : nullptr, xkeys, nr);
    else if (xkeys)
        LOCREC_LAUNCH(rb_count_ex, dim3(items + 1), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, lo.p, hi.p,
                      table_ids, ids, chunk, cnt.p, items, xfirst.p, xkeys);
    else
        LOCREC_LAUNCH(rb_count, dim3(items + 1), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, lo.p, hi.p,
                      table_ids, ids, chunk, cnt.p, items);
    // (kept rows in all: a u32 sum; more than 2^31 - 1 are refused below, and 2^32 or more cannot come from segments that
    // the callers cut out of fewer than 2^31 rows)
    LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, cnt.p, base.p, (size_t)items + 1, s));
    uint32_t m32 = 0;
    LOCREC_READ_BACK(m32, base.p + items, s);
    ++st.host_syncs;
    const int64_t m = m32;
    if (m >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "more than 2^31 rows to sort: split the batch");
    DevBuf<uint32_t> kseg, krow, v0, v1, s0, s1, kcat, flag, fsum;
    DevBuf<uint64_t> q0, q1;
    const size_t mm = (size_t)std::max<int64_t>(m, 1);
    LOCREC_TRY(kseg.alloc(mm));
    LOCREC_TRY(krow.alloc(mm));
    LOCREC_TRY(v0.alloc(mm));
    LOCREC_TRY(v1.alloc(mm));
    LOCREC_TRY(s0.alloc(mm));
    LOCREC_TRY(s1.alloc(mm));
    LOCREC_TRY(q0.alloc(mm));
    LOCREC_TRY(q1.alloc(mm));
    if (capped && m > 0) {
        LOCREC_TRY(kcat.alloc(mm));
        LOCREC_TRY(flag.alloc(mm + 1));
        LOCREC_TRY(fsum.alloc(mm + 1));
    }
    if (m > 0) {
        if (cat && nq)
            LOCREC_LAUNCH(rb_scatter_cat_near, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, ids, chunk,
                          base.p, kseg.p, krow.p, q0.p, v0.p, kcat.p, xkeys ? xfirst.p : nullptr, xkeys, nr, ct);
        else if (cat)
            LOCREC_LAUNCH(rb_scatter_cat, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, ids, chunk,
                          base.p, kseg.p, krow.p, q0.p, v0.p, kcat.p, xkeys ? xfirst.p : nullptr, xkeys, nr, ct);
        else if (nq)
            LOCREC_LAUNCH(rb_scatter_near, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, ids, chunk,
                          base.p, kseg.p, krow.p, q0.p, v0.p, xkeys ? xfirst.p : nullptr, xkeys, nr);
        else if (xkeys)
            LOCREC_LAUNCH(rb_scatter_ex, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, lo.p, hi.p,
                          table_ids, ids, chunk, base.p, kseg.p, krow.p, q0.p, v0.p, xfirst.p, xkeys);
        else
            LOCREC_LAUNCH(rb_scatter, dim3(items), dim3(kRbThreads), 0, s, n_seg, first.p, seg_begin, seg_len, lo.p, hi.p,
                          table_ids, ids, chunk, base.p, kseg.p, krow.p, q0.p, v0.p);
        // three stable passes: id, score key, segment
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, q0.p, q1.p, v0.p, v1.p, (int)m, 0, 64, s));
        LOCREC_LAUNCH(rb_score_keys, grid_for(m), dim3(256), 0, s, m, v1.p, kseg.p, krow.p, seg_begin, scores, q0.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, q0.p, q1.p, v1.p, v0.p, (int)m, 0, 64, s));
        LOCREC_LAUNCH(rb_segment_keys, grid_for(m), dim3(256), 0, s, m, v0.p, kseg.p, s0.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, s0.p, s1.p, v0.p, v1.p, (int)m, 0, 32, s));
    }
    if (capped && m > 0) {
        // one more stable pass, of the sorted positions by (segment, category); then the flags, their sum and the emit
        int key_bits = 33;
        while (key_bits < 64 && ((int64_t)1 << (key_bits - 32)) < n_seg) ++key_bits;
        LOCREC_LAUNCH(rb_cap_keys, grid_for(m), dim3(256), 0, s, m, s1.p, v1.p, kcat.p, q0.p, s0.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, q0.p, q1.p, s0.p, v0.p, (int)m, 0, key_bits, s));
        LOCREC_LAUNCH(rb_cap_flags, grid_for(m), dim3(256), 0, s, m, q1.p, v0.p, cq->caps, N, flag.p);
        LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, flag.p, fsum.p, (size_t)m + 1, s));
        LOCREC_LAUNCH(rb_pad_capped, dim3((unsigned)(n_seg * tiles)), dim3(kRbThreads), 0, s, tiles, N, m, s1.p, fsum.p, out_ids,
                      out_scores, nq ? out_meters : nullptr, out_counts);
        LOCREC_LAUNCH(rb_emit_capped, grid_for(m, kRbThreads), dim3(kRbThreads), 0, s, N, m, s1.p, v1.p, krow.p, flag.p, fsum.p,
                      seg_begin, ids, scores, out_ids, out_scores, nr, ct);
        return LOCREC_OK;
    }
    if (cat && nq)
        LOCREC_LAUNCH(rb_emit_sorted_cat_near, dim3((unsigned)(n_seg * tiles)), dim3(kRbThreads), 0, s, tiles, N, m, s1.p, v1.p,
                      krow.p, seg_begin, ids, scores, out_ids, out_scores, out_counts, nr, ct);
    else if (nq)
        LOCREC_LAUNCH(rb_emit_sorted_near, dim3((unsigned)(n_seg * tiles)), dim3(kRbThreads), 0, s, tiles, N, m, s1.p, v1.p, krow.p,
                      seg_begin, ids, scores, out_ids, out_scores, out_counts, nr);
    else
        LOCREC_LAUNCH(rb_emit_sorted, dim3((unsigned)(n_seg * tiles)), dim3(kRbThreads), 0, s, tiles, N, m, s1.p, v1.p, krow.p,
                      seg_begin, ids, scores, out_ids, out_scores, out_counts);
    return LOCREC_OK;
}

// host offsets: non-decreasing inside [0, n]
bool rb_host_offsets_ok(const int64_t *offsets, int64_t n_segments, int64_t n)
{
    bool ok = offsets[0] >= 0 && offsets[n_segments] <= n;
    for (int64_t i = 0; ok && i < n_segments; ++i) ok = offsets[i] <= offsets[i + 1];
    return ok;
}

// The circles of a public call (host or device arrays like the rest); NULL: the plain and the excluding entry.
struct RbPublicNear {
    const double *place_lat, *place_lon, *center_lat, *center_lon, *radius;
    double *out_meters;
};

// The categories of a public call; allowed_offsets NULL: no lists, max_per_category NULL: no caps; both NULL: the call
// without categories.
struct RbPublicCat {
    const int64_t *place_cat, *allowed_offsets;
    int64_t n_allowed;
    const int64_t *allowed_ids, *caps;
};

// the public entries; with_lists false: no lists (excluded_* unused); pn NULL: no circle; pc NULL: no categories
int32_t rb_public_call(int64_t n_segments, const int64_t *offsets, int64_t n, const int64_t *ids, const double *scores,
                       int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
                       const int64_t *target_region_ids, int64_t max_recommendations, bool with_lists,
                       const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids, int32_t mem,
                       int64_t *out_ids, double *out_scores, int64_t *out_counts, const RbPublicNear *pn = nullptr,
                       const RbPublicCat *pc = nullptr)
{
    rank_batch_stats() = RankBatchStats();
    LOCREC_TRY(mem_ok(mem));
    if (n < 0 || n >= kMaxRows || n_places < 0 || n_places >= kMaxRows || n_segments < 0 || n_segments >= kMaxRows)
        return fail(LOCREC_E_INVALID_ARG, "row, place or segment count out of range [0, 2^31)");
    if (with_lists && (n_excluded < 0 || n_excluded >= kMaxRows))
        return fail(LOCREC_E_INVALID_ARG, "excluded id count out of range [0, 2^31)");
    if (n_segments == 0) return LOCREC_OK;
    const int64_t N = std::max<int64_t>(0, max_recommendations);  // limit(n <= 0) is empty
    if (N > 0 && n_segments > ((int64_t)1 << 60) / N) return fail(LOCREC_E_INVALID_ARG, "n_segments * max_recommendations overflows");
    if (!offsets || !target_region_ids || !out_counts || (n > 0 && (!ids || !scores)) ||
        (n_places > 0 && (!place_ids || !place_region_ids)) || (N > 0 && (!out_ids || !out_scores)) ||
        (with_lists && (!excluded_offsets || (n_excluded > 0 && !excluded_ids))))
        return fail(LOCREC_E_INVALID_ARG, "null array");
    if (pn && (!pn->center_lat || !pn->center_lon || !pn->radius || (n_places > 0 && (!pn->place_lat || !pn->place_lon))))
        return fail(LOCREC_E_INVALID_ARG, "null coordinate or radius array");
    if (pc && pc->allowed_offsets && (pc->n_allowed < 0 || pc->n_allowed >= kMaxRows))
        return fail(LOCREC_E_INVALID_ARG, "n_allowed out of range [0, 2^31)");
    if (pc && pc->allowed_offsets && pc->n_allowed > 0 && !pc->allowed_ids)
        return fail(LOCREC_E_INVALID_ARG, "allowed_category_ids is NULL with n_allowed > 0");
    if (pc && n_places > 0 && !pc->place_cat)
        return fail(LOCREC_E_INVALID_ARG, "place_category_ids is NULL with allow-lists or caps given");
    if (mem == LOCREC_MEM_HOST) {
        if (!rb_host_offsets_ok(offsets, n_segments, n)) return fail(LOCREC_E_INVALID_ARG, "offsets must be non-decreasing inside [0, n]");
        if (with_lists && !rb_host_offsets_ok(excluded_offsets, n_segments, n_excluded))
            return fail(LOCREC_E_INVALID_ARG, "excluded_offsets must be non-decreasing inside [0, n_excluded]");
        if (pn) LOCREC_TRY(rank_near_check_host(n_segments, pn->center_lat, pn->center_lon, pn->radius, n_places, pn->place_lat, pn->place_lon));
        if (pc) LOCREC_TRY(rank_category_check_host(n_segments, pc->allowed_offsets, pc->n_allowed, pc->caps));
    }
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    In<int64_t> off, tgt, rid, pid, preg, xoff, xid;
    In<double> rsc;
    LOCREC_TRY(off.bind(offsets, n_segments + 1, mem, s));
    LOCREC_TRY(tgt.bind(target_region_ids, n_segments, mem, s));
    LOCREC_TRY(rid.bind(ids, n, mem, s));
    LOCREC_TRY(rsc.bind(scores, n, mem, s));
    LOCREC_TRY(pid.bind(place_ids, n_places, mem, s));
    LOCREC_TRY(preg.bind(place_region_ids, n_places, mem, s));
    Out<int64_t> oid, ocnt;
    Out<double> osc;
    LOCREC_TRY(oid.bind(out_ids, n_segments * N, mem));
    LOCREC_TRY(osc.bind(out_scores, n_segments * N, mem));
    LOCREC_TRY(ocnt.bind(out_counts, n_segments, mem));
    In<double> plat, plon, clat, clon, rad;
    Out<double> omet;
    RankNear nq;
    if (pn) {
        LOCREC_TRY(plat.bind(pn->place_lat, n_places, mem, s));
        LOCREC_TRY(plon.bind(pn->place_lon, n_places, mem, s));
        LOCREC_TRY(clat.bind(pn->center_lat, n_segments, mem, s));
        LOCREC_TRY(clon.bind(pn->center_lon, n_segments, mem, s));
        LOCREC_TRY(rad.bind(pn->radius, n_segments, mem, s));
        if (pn->out_meters) LOCREC_TRY(omet.bind(pn->out_meters, n_segments * N, mem));
        nq = {clat.p, clon.p, rad.p, plat.p, plon.p};
    }
    DevBuf<int64_t> seg_begin, seg_len, ex_begin, ex_len, al_begin, al_len;
    DevBuf<unsigned long long> invalid;  // [0] the offsets' and the excluded offsets' verdict, [1] the allowed offsets'
    LOCREC_TRY(seg_begin.alloc((size_t)n_segments));
    LOCREC_TRY(seg_len.alloc((size_t)n_segments));
    LOCREC_TRY(invalid.alloc(2));
    LOCREC_HIP_TRY(hipMemsetAsync(invalid.p, 0, 2 * sizeof(unsigned long long), s));
    LOCREC_LAUNCH(rb_prepare, grid_for(n_segments), dim3(256), 0, s, n_segments, off.p, n, seg_begin.p, seg_len.p, invalid.p);
    if (with_lists) {
        LOCREC_TRY(xoff.bind(excluded_offsets, n_segments + 1, mem, s));
        LOCREC_TRY(xid.bind(excluded_ids, n_excluded, mem, s));
        LOCREC_TRY(ex_begin.alloc((size_t)n_segments));
        LOCREC_TRY(ex_len.alloc((size_t)n_segments));
        LOCREC_LAUNCH(rb_prepare, grid_for(n_segments), dim3(256), 0, s, n_segments, xoff.p, n_excluded, ex_begin.p, ex_len.p,
                      invalid.p);
    }
    In<int64_t> pcat, aoff, aid, caps;
    RankCategory cq;
    if (pc) {
        LOCREC_TRY(pcat.bind(pc->place_cat, n_places, mem, s));
        cq.place_cat = pcat.p;
        if (pc->caps) {
            LOCREC_TRY(caps.bind(pc->caps, n_segments, mem, s));
            cq.caps = caps.p;
        }
        if (pc->allowed_offsets) {
            LOCREC_TRY(aoff.bind(pc->allowed_offsets, n_segments + 1, mem, s));
            LOCREC_TRY(aid.bind(pc->allowed_ids, pc->n_allowed, mem, s));
            LOCREC_TRY(al_begin.alloc((size_t)n_segments));
            LOCREC_TRY(al_len.alloc((size_t)n_segments));
            LOCREC_LAUNCH(rb_prepare, grid_for(n_segments), dim3(256), 0, s, n_segments, aoff.p, pc->n_allowed, al_begin.p, al_len.p,
                          invalid.p + 1);
            cq.allow_begin = al_begin.p;
            cq.allow_len = al_len.p;
            cq.allow_ids = aid.p;
            cq.n_allowed = pc->n_allowed;
            cq.allow_invalid = invalid.p + 1;
        }
    }
    LOCREC_TRY(rank_segments(n_segments, seg_begin.p, seg_len.p, rid.p, rsc.p, n_places, pid.p, preg.p, tgt.p, N, ex_begin.p,
                             ex_len.p, n_excluded, xid.p, oid.p, osc.p, ocnt.p, invalid.p, 0, s, pn ? &nq : nullptr, omet.p,
                             pc ? &cq : nullptr));
    if (pn && pn->out_meters) LOCREC_TRY(omet.deliver(n_segments * N, s));
    LOCREC_TRY(oid.deliver(n_segments * N, s));
    LOCREC_TRY(osc.deliver(n_segments * N, s));
    LOCREC_TRY(ocnt.deliver(n_segments, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    ++rank_batch_stats().host_syncs;
    return LOCREC_OK;
}

}  // namespace

namespace locrec {

int32_t rank_segments_device(int64_t n_seg, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                             const double *scores, int64_t n_places, const int64_t *place_ids,
                             const int64_t *place_region_ids, const int64_t *target_region_ids, int64_t max_recommendations,
                             int64_t *out_ids, double *out_scores, int64_t *out_counts,
                             const unsigned long long *invalid_flag, int64_t host_assembled, hipStream_t s)
{
    return rank_segments(n_seg, seg_begin, seg_len, ids, scores, n_places, place_ids, place_region_ids, target_region_ids,
                         max_recommendations, nullptr, nullptr, 0, nullptr, out_ids, out_scores, out_counts, invalid_flag,
                         host_assembled, s);
}

int32_t rank_segments_device_excluding(int64_t n_seg, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                                       const double *scores, int64_t n_places, const int64_t *place_ids,
                                       const int64_t *place_region_ids, const int64_t *target_region_ids,
                                       int64_t max_recommendations, const int64_t *ex_begin, const int64_t *ex_len,
                                       int64_t n_excluded, const int64_t *ex_ids, int64_t *out_ids, double *out_scores,
                                       int64_t *out_counts, const unsigned long long *invalid_flag, int64_t host_assembled,
                                       hipStream_t s)
{
    if (n_seg > 0 && (!ex_begin || !ex_len || (n_excluded > 0 && !ex_ids))) return fail(LOCREC_E_INVALID_ARG, "null exclusion array");
    return rank_segments(n_seg, seg_begin, seg_len, ids, scores, n_places, place_ids, place_region_ids, target_region_ids,
                         max_recommendations, ex_begin, ex_len, n_excluded, ex_ids, out_ids, out_scores, out_counts, invalid_flag,
                         host_assembled, s);
}

int32_t rank_near_check_host(int64_t n_seg, const double *center_lat, const double *center_lon, const double *radius,
                             int64_t n_places, const double *place_lat, const double *place_lon)
{
    auto ok = [](double lat, double lon) { return lat >= -90.0 && lat <= 90.0 && lon >= -180.0 && lon <= 180.0; };
    unsigned long long bits = 0;
    for (int64_t i = 0; i < n_seg; ++i) {
        if (!(radius[i] >= 0.0)) bits |= 2ull;
        if (!ok(center_lat[i], center_lon[i])) bits |= 4ull;
    }
    for (int64_t j = 0; j < n_places; ++j)
        if (!ok(place_lat[j], place_lon[j])) bits |= 8ull;
    return bits ? rb_near_refusal(bits) : LOCREC_OK;
}

int32_t rank_segments_device_near(int64_t n_seg, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                                  const double *scores, int64_t n_places, const int64_t *place_ids,
                                  const int64_t *place_region_ids, const int64_t *target_region_ids, int64_t max_recommendations,
                                  const RankExclude &ex, const RankNear &near, int64_t *out_ids, double *out_scores,
                                  double *out_meters, int64_t *out_counts, const unsigned long long *invalid_flag,
                                  int64_t host_assembled, hipStream_t s)
{
    if (n_seg > 0 && ex.begin && (!ex.len || (ex.n > 0 && !ex.ids))) return fail(LOCREC_E_INVALID_ARG, "null exclusion array");
    if (n_seg > 0 && near.center_lat &&
        (!near.center_lon || !near.radius || (n_places > 0 && (!near.place_lat || !near.place_lon))))
        return fail(LOCREC_E_INVALID_ARG, "null coordinate or radius array");
    return rank_segments(n_seg, seg_begin, seg_len, ids, scores, n_places, place_ids, place_region_ids, target_region_ids,
                         max_recommendations, ex.begin, ex.len, ex.n, ex.ids, out_ids, out_scores, out_counts, invalid_flag,
                         host_assembled, s, near.center_lat ? &near : nullptr, out_meters);
}

int32_t rank_segments_device_by_category(int64_t n_seg, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                                         const double *scores, int64_t n_places, const int64_t *place_ids,
                                         const int64_t *place_region_ids, const int64_t *target_region_ids,
                                         int64_t max_recommendations, const RankExclude &ex, const RankNear &near,
                                         const RankCategory &cat, int64_t *out_ids, double *out_scores, double *out_meters,
                                         int64_t *out_counts, const unsigned long long *invalid_flag, int64_t host_assembled,
                                         hipStream_t s)
{
    if (n_seg > 0 && ex.begin && (!ex.len || (ex.n > 0 && !ex.ids))) return fail(LOCREC_E_INVALID_ARG, "null exclusion array");
    if (n_seg > 0 && near.center_lat &&
        (!near.center_lon || !near.radius || (n_places > 0 && (!near.place_lat || !near.place_lon))))
        return fail(LOCREC_E_INVALID_ARG, "null coordinate or radius array");
    const bool with_cat = cat.allow_begin || cat.caps;
    if (n_seg > 0 && cat.allow_begin && (!cat.allow_len || (cat.n_allowed > 0 && !cat.allow_ids)))
        return fail(LOCREC_E_INVALID_ARG, "null allowed category array");
    if (n_seg > 0 && with_cat && n_places > 0 && !cat.place_cat)
        return fail(LOCREC_E_INVALID_ARG, "place_category_ids is NULL with allow-lists or caps given");
    return rank_segments(n_seg, seg_begin, seg_len, ids, scores, n_places, place_ids, place_region_ids, target_region_ids,
                         max_recommendations, ex.begin, ex.len, ex.n, ex.ids, out_ids, out_scores, out_counts, invalid_flag,
                         host_assembled, s, near.center_lat ? &near : nullptr, out_meters, with_cat ? &cat : nullptr);
}

int32_t rank_category_check_host(int64_t n_seg, const int64_t *allowed_offsets, int64_t n_allowed, const int64_t *caps)
{
    if (allowed_offsets && !rb_host_offsets_ok(allowed_offsets, n_seg, n_allowed)) return rb_cat_refusal(32ull);
    for (int64_t i = 0; caps && i < n_seg; ++i)
        if (caps[i] < 1) return rb_cat_refusal(16ull);
    return LOCREC_OK;
}

}  // namespace locrec

// (the circles: all five coordinate arrays NULL is none, and out_meters is then unused; the categories: no lists and no
// caps is the call without them)
extern "C" int32_t locrec_rank_recommendations_batch_by_category(
    int64_t n_segments, const int64_t *offsets, int64_t n, const int64_t *ids, const double *scores, int64_t n_places,
    const int64_t *place_ids, const int64_t *place_region_ids, const double *place_latitudes, const double *place_longitudes,
    const int64_t *place_category_ids, const int64_t *target_region_ids, const double *center_latitudes,
    const double *center_longitudes, const double *radius_meters, int64_t max_recommendations, const int64_t *excluded_offsets,
    int64_t n_excluded, const int64_t *excluded_ids, const int64_t *allowed_offsets, int64_t n_allowed,
    const int64_t *allowed_category_ids, const int64_t *max_per_category, int32_t mem, int64_t *out_ids, double *out_scores,
    double *out_meters, int64_t *out_counts)
try {
    const bool circles = place_latitudes || place_longitudes || center_latitudes || center_longitudes || radius_meters;
    const RbPublicNear pn = {place_latitudes, place_longitudes, center_latitudes, center_longitudes, radius_meters, out_meters};
    const RbPublicCat pc = {place_category_ids, allowed_offsets, allowed_offsets ? n_allowed : 0, allowed_category_ids, max_per_category};
    return rb_public_call(n_segments, offsets, n, ids, scores, n_places, place_ids, place_region_ids, target_region_ids,
                          max_recommendations, excluded_offsets != nullptr, excluded_offsets, excluded_offsets ? n_excluded : 0,
                          excluded_ids, mem, out_ids, out_scores, out_counts, circles ? &pn : nullptr,
                          allowed_offsets || max_per_category ? &pc : nullptr);
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_rank_recommendations_batch_near(
    int64_t n_segments, const int64_t *offsets, int64_t n, const int64_t *ids, const double *scores, int64_t n_places,
    const int64_t *place_ids, const int64_t *place_region_ids, const double *place_latitudes, const double *place_longitudes,
    const int64_t *target_region_ids, const double *center_latitudes, const double *center_longitudes, const double *radius_meters,
    int64_t max_recommendations, const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids, int32_t mem,
    int64_t *out_ids, double *out_scores, double *out_meters, int64_t *out_counts)
try {
    const RbPublicNear pn = {place_latitudes, place_longitudes, center_latitudes, center_longitudes, radius_meters, out_meters};
    return rb_public_call(n_segments, offsets, n, ids, scores, n_places, place_ids, place_region_ids, target_region_ids,
                          max_recommendations, excluded_offsets != nullptr, excluded_offsets, excluded_offsets ? n_excluded : 0,
                          excluded_ids, mem, out_ids, out_scores, out_counts, &pn);
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_rank_recommendations_batch(int64_t n_segments, const int64_t *offsets, int64_t n, const int64_t *ids,
                                                     const double *scores, int64_t n_places, const int64_t *place_ids,
                                                     const int64_t *place_region_ids, const int64_t *target_region_ids,
                                                     int64_t max_recommendations, int32_t mem, int64_t *out_ids,
                                                     double *out_scores, int64_t *out_counts)
try {
    return rb_public_call(n_segments, offsets, n, ids, scores, n_places, place_ids, place_region_ids, target_region_ids,
                          max_recommendations, false, nullptr, 0, nullptr, mem, out_ids, out_scores, out_counts);
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_rank_recommendations_batch_excluding(int64_t n_segments, const int64_t *offsets, int64_t n,
                                                               const int64_t *ids, const double *scores, int64_t n_places,
                                                               const int64_t *place_ids, const int64_t *place_region_ids,
                                                               const int64_t *target_region_ids, int64_t max_recommendations,
                                                               const int64_t *excluded_offsets, int64_t n_excluded,
                                                               const int64_t *excluded_ids, int32_t mem, int64_t *out_ids,
                                                               double *out_scores, int64_t *out_counts)
try {
    return rb_public_call(n_segments, offsets, n, ids, scores, n_places, place_ids, place_region_ids, target_region_ids,
                          max_recommendations, true, excluded_offsets, n_excluded, excluded_ids, mem, out_ids, out_scores,
                          out_counts);
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_rank_recommendations_batch_stats(int64_t *out_one_block, int64_t *out_split, int64_t *out_chunks,
                                                           int64_t *out_sorted, int64_t *out_membership_form,
                                                           int64_t *out_host_assembled, int64_t *out_host_syncs)
try {
    const RankBatchStats &st = rank_batch_stats();
    if (out_one_block) *out_one_block = st.one_block;
    if (out_split) *out_split = st.split;
    if (out_chunks) *out_chunks = st.chunks;
    if (out_sorted) *out_sorted = st.sorted;
    if (out_membership_form) *out_membership_form = st.membership_form;
    if (out_host_assembled) *out_host_assembled = st.host_assembled;
    if (out_host_syncs) *out_host_syncs = st.host_syncs;
    return LOCREC_OK;
}
LOCREC_CATCH_ALL
