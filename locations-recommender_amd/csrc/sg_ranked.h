// sg_ranked.h -- the ranked SG batch (included at the end of sg_batch.hip, behind sg.hip): the batched makeRecommendations
// to its end, printRecommendations of StochasticRecommenderMain.scala:64-75, without x ever leaving the device
// (locrec_sg_recommend_ranked_batch).  The handle gets no new member (sg.hip stays as it is): every buffer here is local to
// the call, and their number does not depend on the number of targets.
//
//   emit rows       what a request can return, numbered once per call: rows 0 .. T-1 are x's live rows; when D can still
//                   be positive (no sweep ran) the source-only vertices follow in ascending vertex order.  eid[e] is the
//                   vertex id of emit row e.
//   membership      once per (distinct target region, vertex): a bitmap over the emit rows per region.  sg_rk_members, one
//                   thread per row of the places table: its region among the distinct target regions, its id among the
//                   sorted vertex ids (two binary searches), one 64-bit atomic OR.  A place listed twice sets one bit, a
//                   place listed in two regions one bit in each - as the ranker's join counts them.  The popcount of a
//                   region's bitmap (sg_rk_popcount) is the exact room a request for that region needs.
//   sg_rk_emit      per tile, after its last round: one lane per emit row, a wave reads its 64 rows of x as whole 128-byte
//                   lines (all 16 columns, each from the parity of its own last sweep; a source-only vertex reads D's
//                   row) and parks them in LDS.  Then per request of the tile: the region's bitmap word of these 64 rows
//                   (wave-uniform; zero for most waves), p > 0, not the request's own target; a ballot, ONE atomic add per
//                   wave and request on the segment's length, the lane prefix, and (id, p) goes to the request's segment.
//                   The same pass counts per column the rows makeRecommendations has (p > 0, not the target).
//   sg_rk_state     the tile's read-back: its SgBatchState and per column the sum of the last sweep's block sums, added
//                   by the butterfly the finalize itself decides with - 384 bytes a tile.
//   ranking         rank_segments_device (rank_batch.hip) once per group of requests; a group ends where the room of its
//                   segments would pass LOCREC_SG_RANKED_ROW_BUDGET rows (a tile's requests may straddle groups: the
//                   emit runs once per part).  The group's N rows a request then travel to the host.
//   exclusion lists locrec_sg_recommend_ranked_batch_excluding: a caller-given list of ids per position (the places a
//                   person has been to), uploaded once in emit order; a group's ranker call is the excluding entry with
//                   the sub-range of its segments.  The emit and the segments' room do not see the lists.
//   categories      locrec_sg_recommend_ranked_batch_by_category: an allow-list and a cap per position and the place rows'
//                   categories, uploaded once (lists and caps in emit order, RankCatHost); a group's ranker call is
//                   rank_segments_device_by_category with the sub-range of its segments, the circles optional.
//   circles         locrec_sg_recommend_ranked_batch_near: a centre and a radius per position and the place rows'
//                   coordinates, uploaded once (the circles in emit order); a group's ranker call is the near entry with
//                   the sub-range of its segments, and out_meters comes back with the group's rows.  As with the lists,
//                   the emit and the segments' room see only the region.
//   host            the pool's entry (sg_pool_ranked.h) shares sg_rk_check_args, sg_rk_verdicts, SgRkCall (groups, ranker
//                   call, read-backs, scatter) and sg_rk_plan.h's order and groups: this entry is a pool of one member
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (VGPRs / LDS bytes / scratch):
//   sg_rk_emit      82 / 32832 / 0
//   sg_rk_members   14 / 0 / 0
//   sg_rk_popcount  8 / 4 / 0
//   sg_rk_row_ids   4 / 0 / 0
//   sg_rk_state     14 / 0 / 0
#pragma once

#include "rank_batch.h"
#include "sg_rk_plan.h"

namespace {

constexpr int kRkThreads = 256;
constexpr size_t kRkStateBytes = kBatchPackHead + kBatchB * sizeof(double);  // SgBatchState at 0, the columns' totals behind
constexpr int64_t kRkDefaultBudget = (int64_t)1 << 24;
static_assert(sizeof(SgBatchState) <= kBatchPackHead, "the state sits in front of the totals");

// what this thread's last ranked batch did (locrec_sg_recommend_ranked_batch_stats)
struct SgRankedStats {
    int64_t tiles = 0, groups = 0, emitted_rows = 0, readback_bytes = 0, host_syncs = 0;
};

SgRankedStats &sg_ranked_stats()
{
    thread_local SgRankedStats st;
    return st;
}

// LOCREC_SG_RANKED_ROW_BUDGET: rows of segment room one ranker call takes (read per call; a group has at least one request)
int64_t sg_ranked_row_budget()
{
    int64_t b = kRkDefaultBudget;
    if (const char *e = std::getenv("LOCREC_SG_RANKED_ROW_BUDGET")) b = atoll(e);
    return std::min<int64_t>(std::max<int64_t>(b, 1), (int64_t)1 << 30);
}

inline dim3 rk_grid(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + kRkThreads - 1) / kRkThreads)); }

// eid[srow[i]] = sid[i]: the vertex id of every emit row
__global__ __launch_bounds__(kRkThreads) void sg_rk_row_ids(int64_t m, const int64_t *__restrict__ sid,
                                                           const int32_t *__restrict__ srow, int64_t *__restrict__ eid)
{
    const int64_t i = (int64_t)blockIdx.x * kRkThreads + threadIdx.x;
    if (i < m) eid[srow[i]] = sid[i];
}

// first index of a[0 .. n) that is not below key (a ascending)
__device__ __forceinline__ int64_t rk_lower_bound(const int64_t *__restrict__ a, int64_t n, int64_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one thread per row of the places table: the bit (its region, its emit row), when it has both.  The bodies of this
// file's kernels are __device__ functions that the pool's kernels (sg_pool_ranked.h) call too.
__device__ __forceinline__ void sg_rk_members_body(int64_t n_places, const int64_t *__restrict__ place_ids,
                                                   const int64_t *__restrict__ place_regions, int64_t n_regions,
                                                   const int64_t *__restrict__ regions, int64_t m,
                                                   const int64_t *__restrict__ sid, const int32_t *__restrict__ srow,
                                                   int64_t words, unsigned long long *bits)
{
    const int64_t i = (int64_t)blockIdx.x * kRkThreads + threadIdx.x;
    if (i >= n_places) return;
    const int64_t reg = place_regions[i], id = place_ids[i];
    const int64_t r = rk_lower_bound(regions, n_regions, reg);
    if (r >= n_regions || regions[r] != reg) return;
    const int64_t j = rk_lower_bound(sid, m, id);
    if (j >= m || sid[j] != id) return;
    const int32_t e = srow[j];  // < 64 * words
    atomicOr(&bits[r * words + (e >> 6)], 1ull << (e & 63));
}

__global__ __launch_bounds__(kRkThreads) void sg_rk_members(int64_t n_places, const int64_t *__restrict__ place_ids,
                                                           const int64_t *__restrict__ place_regions, int64_t n_regions,
                                                           const int64_t *__restrict__ regions, int64_t m,
                                                           const int64_t *__restrict__ sid, const int32_t *__restrict__ srow,
                                                           int64_t words, unsigned long long *bits)
{
    sg_rk_members_body(n_places, place_ids, place_regions, n_regions, regions, m, sid, srow, words, bits);
}

// *cap = bits set in row[0 .. words): one block
__device__ __forceinline__ void sg_rk_popcount_body(int64_t words, const unsigned long long *__restrict__ row,
                                                    unsigned long long *__restrict__ cap)
{
    __shared__ unsigned int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    unsigned int mine = 0;
    for (int64_t w = threadIdx.x; w < words; w += kRkThreads) mine += (unsigned int)__popcll(row[w]);
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) *cap = total;
}

// caps[r] = bits set in region r's bitmap; one block per region
__global__ __launch_bounds__(kRkThreads) void sg_rk_popcount(int64_t words, const unsigned long long *__restrict__ bits,
                                                            unsigned long long *__restrict__ caps)
{
    sg_rk_popcount_body(words, bits + (int64_t)blockIdx.x * words, caps + blockIdx.x);
}

// The tile's read-back: the state, and per column the total of its last executed sweep's block sums (the butterfly of
// sg_finalize_batch's own decision; host_total_d2 is the same sum).  One wave per column.
__device__ __forceinline__ void sg_rk_state_body(const SgBatchState *__restrict__ st, const double *__restrict__ parts,
                                                 unsigned char *out)
{
    const int lane = threadIdx.x & 63, b = threadIdx.x >> 6;
    const int sweeps = st->sweeps[b];
    double tot = 0.0;
    if (sweeps > 0) tot = wave_butterfly_sum(parts[(size_t)((sweeps - 1) & 1) * kParts * kBatchB + (size_t)lane * kBatchB + b]);
    if (lane == 0) reinterpret_cast<double *>(out + kBatchPackHead)[b] = tot;
    if (threadIdx.x < sizeof(SgBatchState) / 4)
        reinterpret_cast<int32_t *>(out)[threadIdx.x] = reinterpret_cast<const int32_t *>(st)[threadIdx.x];
}

__global__ __launch_bounds__(64 * kBatchB) void sg_rk_state(const SgBatchState *__restrict__ st, const double *__restrict__ parts,
                                                           unsigned char *out)
{
    sg_rk_state_body(st, parts, out);
}
static_assert(kParts == 64, "one lane per block sum");

// The emit rows of a graph: m searchable ids, ascending (sid), and the emit row of each (srow).  With dead_rows the
// source-only vertices follow the T live rows in ascending vertex order, and sid is the handle's own vertex list.
struct SgRkRows {
    std::vector<int64_t> sid_own;
    std::vector<int32_t> srow;
    const int64_t *sid = nullptr;
    int64_t m = 0;
    bool dead_rows = false;
};

void sg_rk_rows(locrec_sg_graph *g, bool dead_rows, SgRkRows &r)
{
    const int32_t T = g->nlive;
    if (g->live_sorted.size() != (size_t)T) {
        g->live_sorted.clear();
        for (int64_t v = 0; v < g->nv; ++v)
            if (g->live_of[v] >= 0) g->live_sorted.push_back((int32_t)v);
    }
    r.dead_rows = dead_rows;
    r.m = dead_rows ? g->nv : (int64_t)T;  // emit rows = searchable ids
    r.sid_own.clear();
    r.srow.assign((size_t)r.m, 0);
    r.sid = g->vid.data();
    if (dead_rows) {
        int32_t next_dead = T;
        for (int64_t v = 0; v < r.m; ++v) r.srow[(size_t)v] = g->live_of[v] >= 0 ? g->live_of[v] : next_dead++;
    } else {
        r.sid_own.resize((size_t)r.m);
        for (int64_t i = 0; i < r.m; ++i) {
            r.sid_own[(size_t)i] = g->vid[g->live_sorted[(size_t)i]];
            r.srow[(size_t)i] = g->live_of[g->live_sorted[(size_t)i]];
        }
        r.sid = r.sid_own.data();
    }
}

// the emit row of vertex tv (-1: it has none)
inline int32_t sg_rk_row_of(const locrec_sg_graph *g, const SgRkRows &r, int32_t tv)
{
    if (g->live_of[tv] >= 0) return g->live_of[tv];
    return r.dead_rows ? r.srow[(size_t)tv] : -1;
}

// D's value after a sweep is sg_next_x(0, false): never positive; before the first it is 1/V
inline bool sg_rk_dead_rows(double alpha, int64_t max_iterations)
{
    const double xd = 0.0 * alpha + 0.0 * (1 - alpha);
    return max_iterations == 0 || xd > 0;
}

struct SgEmitTile {
    int32_t col_trow[kBatchB];  // emit row of column b's target (-1: it has none), never a row of that column's result
    int32_t nb, T, ne;          // ne: emit rows
    int32_t count_cols;         // this launch also counts the columns' rows (the first launch of a tile)
    int64_t xstride;
};

// bx: the block's position among the emit blocks of its graph
__device__ __forceinline__ void sg_rk_emit_body(
    const SgEmitTile &tl, const SgBatchState *__restrict__ st, const double *__restrict__ xbuf, const int64_t *__restrict__ eid,
    const unsigned long long *__restrict__ bits, const int64_t words, const int32_t k0, const int32_t k1,
    const int32_t *__restrict__ req_col, const int32_t *__restrict__ req_trow, const int32_t *__restrict__ req_bm,
    const int64_t *__restrict__ seg_begin, unsigned long long *seg_len, const int64_t rows_cap, int64_t *__restrict__ seg_ids,
    double *__restrict__ seg_probs, unsigned long long *col_rows, const int bx)
{
    __shared__ double xs[kRkThreads / 64][kBatchB][64];  // [wave][column][lane]: each lane reads back only what it wrote
    __shared__ unsigned int colcnt[kBatchB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e0 = (bx * (kRkThreads / 64) + wave) * 64;  // (a multiple of 64: one bitmap word per wave)
    const int e = e0 + lane;
    if (threadIdx.x < kBatchB) colcnt[threadIdx.x] = 0;
    __syncthreads();
    if (e0 < tl.ne) {
        uint32_t pm = 0;  // the columns whose x is in the second buffer
#pragma unroll
        for (int b = 0; b < kBatchB; ++b) pm |= (uint32_t)(st->sweeps[b] & 1) << b;
        pm = (uint32_t)__builtin_amdgcn_readfirstlane((int)pm);
        const bool in = e < tl.ne;
        // a source-only vertex holds D's value in every column but its own, where it is the target
        const v2d *r0 = reinterpret_cast<const v2d *>(xbuf + (size_t)(e < tl.T ? e : tl.T) * kBatchB);
        const v2d *r1 = reinterpret_cast<const v2d *>(xbuf + tl.xstride + (size_t)(e < tl.T ? e : tl.T) * kBatchB);
        double v[kBatchB];
        if (pm == 0u || pm == 0xFFFFu) {
            const v2d *r = pm ? r1 : r0;
#pragma unroll
            for (int k = 0; k < kBatchB / 2; ++k) {
                const v2d a = r[k];
                v[2 * k] = a.x;
                v[2 * k + 1] = a.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kBatchB / 2; ++k) {
                const v2d a = r0[k], c = r1[k];
                v[2 * k] = ((pm >> (2 * k)) & 1u) ? c.x : a.x;
                v[2 * k + 1] = ((pm >> (2 * k + 1)) & 1u) ? c.y : a.y;
            }
        }
#pragma unroll
        for (int b = 0; b < kBatchB; ++b) xs[wave][b][lane] = v[b];
        if (tl.count_cols) {
            // :84-88 per column: id != vertexId and probability > 0
#pragma unroll
            for (int b = 0; b < kBatchB; ++b) {
                const unsigned long long m = __ballot(in && b < tl.nb && v[b] > 0 && e != tl.col_trow[b]);
                if (lane == 0 && m) atomicAdd(&colcnt[b], (unsigned int)__popcll(m));
            }
        }
        for (int k = k0; k < k1; ++k) {
            const unsigned long long word = bits[(int64_t)req_bm[k] * words + (e0 >> 6)];  // (wave-uniform)
            if (word == 0) continue;
            const double p = xs[wave][req_col[k]][lane];
            const bool ok = ((word >> lane) & 1ull) && p > 0 && e != req_trow[k];  // (a set bit is an emit row)
            const unsigned long long m = __ballot(ok);
            if (m == 0) continue;
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(&seg_len[k], (unsigned long long)__popcll(m));
            const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
            const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
            if (ok) {
                const int64_t pos = seg_begin[k] + (int64_t)(((unsigned long long)bhi << 32) | blo) +
                                    __popcll(m & ((1ull << lane) - 1ull));
                if (pos < rows_cap) {  // (the popcount of the bitmap is the room: always)
                    seg_ids[pos] = eid[e];
                    seg_probs[pos] = p;
                }
            }
        }
    }
    __syncthreads();
    if (tl.count_cols && threadIdx.x < kBatchB && colcnt[threadIdx.x])
        atomicAdd(&col_rows[threadIdx.x], (unsigned long long)colcnt[threadIdx.x]);
}

__global__ __launch_bounds__(kRkThreads) void sg_rk_emit(
    const SgEmitTile tl, const SgBatchState *__restrict__ st, const double *__restrict__ xbuf, const int64_t *__restrict__ eid,
    const unsigned long long *__restrict__ bits, const int64_t words, const int32_t k0, const int32_t k1,
    const int32_t *__restrict__ req_col, const int32_t *__restrict__ req_trow, const int32_t *__restrict__ req_bm,
    const int64_t *__restrict__ seg_begin, unsigned long long *seg_len, const int64_t rows_cap, int64_t *__restrict__ seg_ids,
    double *__restrict__ seg_probs, unsigned long long *col_rows)
{
    sg_rk_emit_body(tl, st, xbuf, eid, bits, words, k0, k1, req_col, req_trow, req_bm, seg_begin, seg_len, rows_cap, seg_ids,
                    seg_probs, col_rows, (int)blockIdx.x);
}

// The ranker surface's argument checks (locrec_rank_recommendations_batch's), the same for both entries.  N: the row limit
int32_t sg_rk_check_args(int64_t n, int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
                         const int64_t *target_region_ids, int64_t max_recommendations, const int64_t *out_ids,
                         const double *out_probabilities, const int64_t *out_counts, int64_t &N)
{
    if (n_places < 0 || n_places >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31))
        return fail(LOCREC_E_INVALID_ARG, "place or target count out of range [0, 2^31)");
    N = std::max<int64_t>(0, max_recommendations);  // limit(n <= 0) is empty
    if (N > 0 && n > ((int64_t)1 << 60) / N) return fail(LOCREC_E_INVALID_ARG, "n_targets * max_recommendations overflows");
    if (n > 0 && (!target_region_ids || !out_counts || (N > 0 && (!out_ids || !out_probabilities)) ||
                  (n_places > 0 && (!place_ids || !place_region_ids))))
        return fail(LOCREC_E_INVALID_ARG, "null array");
    return LOCREC_OK;
}

// A tile's verdicts from its state image (sg_rk_state's 384 bytes): column j of nb -> res_it[j], res_conv[j]
int32_t sg_rk_verdicts(const unsigned char *image, int nb, double eps2, int64_t max_iterations, int64_t *res_it, int32_t *res_conv)
{
    SgBatchState hs;
    std::memcpy(&hs, image, sizeof hs);
    const double *totals = reinterpret_cast<const double *>(image + kBatchPackHead);
    for (int j = 0; j < nb; ++j)
        LOCREC_TRY(sg_batch_verdict(hs.sweeps[j], [&]() { return totals[j]; }, eps2, max_iterations, &res_it[j], &res_conv[j]));
    return LOCREC_OK;
}

// The circles of a near call (host arrays, checked by the entry): per row of the place table its coordinates, per input
// position a centre and a radius; meters: the output rows' distances (NULL: not wanted).
struct SgRkNear {
    const double *place_lat, *place_lon, *center_lat, *center_lon, *radius;
    double *meters;
};

// What both ranked entries hold from the caps' read-back to the call's end.  The first members are the entry's: its
// stream and, in its own buffer, the places table, the targets, the segments' begins and lengths (the columns' row
// counts lie behind the lengths).
struct SgRkCall {
    SgRankedStats &stats;
    hipStream_t s;
    int64_t n, N, n_places;
    const int64_t *d_pid, *d_preg, *d_tgt;
    int64_t *d_seg_begin, *d_seg_len;
    // per-request exclusion lists in emit order (d_ex_begin NULL: none - the pool's entry, the plain batch): request k
    // leaves out d_ex_ids[d_ex_begin[k] .. + d_ex_len[k]); a group's ranker call gets the sub-range of its segments
    const int64_t *d_ex_begin = nullptr, *d_ex_len = nullptr, *d_ex_ids = nullptr;
    int64_t n_ex = 0;
    // per-request circles in emit order and the place rows' coordinates (near.center_lat NULL: none): like the lists,
    // only the group's ranker call sees them
    RankNear near;
    std::vector<double> h_near, h_omet;  // the centres and radii as uploaded; the ranked rows' distances in emit order
    int64_t Nd = 0;
    SgRkGroups groups;
    size_t group = 0;               // the group that is being filled
    DevBuf<int64_t> d_rows, d_out;  // ids, then probabilities: the emitted rows of a group; its ranked rows and counts
    int64_t *d_row_ids = nullptr;
    double *d_row_probs = nullptr;
    std::vector<int64_t> h_oid, h_cnt, res_it;  // the ranked rows in emit order; res_*: per distinct target, flat
    std::vector<double> h_osc;
    std::vector<int32_t> res_conv;
    std::vector<int64_t> h_ex;  // the lists' begins and lengths in emit order, as uploaded
    // per-request allow-lists and caps in emit order and the place rows' categories (nothing given: none): like the
    // circles, uploaded once, and only the group's ranker call sees them
    RankCategory cat;
    std::vector<int64_t> h_cat;

    // Reads the n_caps caps back and forms the groups: request k's segment has room caps[cap_of[k]], a group's segments
    // share the row buffer.  nu: distinct targets.
    int32_t plan(const int64_t *d_caps, size_t n_caps, const int32_t *cap_of, size_t nu)
    {
        std::vector<int64_t> caps(n_caps), cap_k((size_t)n);
        LOCREC_HIP_TRY(hipMemcpyAsync(caps.data(), d_caps, n_caps * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        LOCREC_HIP_TRY(hipGetLastError());
        ++stats.host_syncs;
        stats.readback_bytes += (int64_t)n_caps * 8;
        for (int64_t k = 0; k < n; ++k) cap_k[(size_t)k] = caps[(size_t)cap_of[k]];
        sg_rk_form_groups(cap_k, sg_ranked_row_budget(), groups);
        if (groups.max_rows >= ((int64_t)1 << 31)) return fail(LOCREC_E_INVALID_ARG, "a request's region has 2^31 places or more");
        Nd = std::min(N, groups.max_cap);  // no request has more rows than the largest region: the rest is padding
        LOCREC_HIP_TRY(hipMemcpyAsync(d_seg_begin, groups.seg_begin.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
        LOCREC_TRY(d_rows.alloc(2 * (size_t)groups.max_rows));
        LOCREC_TRY(d_out.alloc((size_t)((near.center_lat ? 3 : 2) * groups.max_req * Nd + groups.max_req)));
        if (near.center_lat) h_omet.resize((size_t)(n * Nd));
        d_row_ids = d_rows.p;
        d_row_probs = reinterpret_cast<double *>(d_rows.p + groups.max_rows);
        h_oid.resize((size_t)(n * Nd));
        h_osc.resize((size_t)(n * Nd));
        h_cnt.assign((size_t)n, 0);
        res_it.resize(nu);
        res_conv.resize(nu);
        return LOCREC_OK;
    }

    // The exclusion lists, uploaded once into d_ex (which outlives the call's launches): begins and lengths in emit order
    // (ord: emit position -> input position), then the ids
    int32_t upload_lists(const std::vector<int64_t> &ord, const int64_t *excluded_offsets, int64_t n_excluded,
                         const int64_t *excluded_ids, DevBuf<int64_t> &d_ex)
    {
        std::vector<int64_t> &xr = h_ex;  // (lives as long as the call: the copy below may read it later)
        xr.resize((size_t)(2 * n));
        for (int64_t k = 0; k < n; ++k) {
            const int64_t i = ord[(size_t)k];
            xr[(size_t)k] = excluded_offsets[i];
            xr[(size_t)(n + k)] = excluded_offsets[i + 1] - excluded_offsets[i];
        }
        LOCREC_TRY(d_ex.alloc((size_t)(2 * n + n_excluded)));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_ex.p, xr.data(), (size_t)(2 * n) * 8, hipMemcpyHostToDevice, s));
        if (n_excluded > 0)
            LOCREC_HIP_TRY(hipMemcpyAsync(d_ex.p + 2 * n, excluded_ids, (size_t)n_excluded * 8, hipMemcpyHostToDevice, s));
        d_ex_begin = d_ex.p;
        d_ex_len = d_ex.p + n;
        d_ex_ids = d_ex.p + 2 * n;
        n_ex = n_excluded;
        return LOCREC_OK;
    }

    // The circles, uploaded once into d_nr (which outlives the call's launches): the place rows' coordinates, then the
    // centres and radii in emit order.  Before plan(): the output buffer's size depends on it.
    int32_t upload_circles(const std::vector<int64_t> &ord, const SgRkNear &nr, DevBuf<double> &d_nr)
    {
        h_near.resize((size_t)(3 * n));
        for (int64_t k = 0; k < n; ++k) {
            const int64_t i = ord[(size_t)k];
            h_near[(size_t)k] = nr.center_lat[i];
            h_near[(size_t)(n + k)] = nr.center_lon[i];
            h_near[(size_t)(2 * n + k)] = nr.radius[i];
        }
        LOCREC_TRY(d_nr.alloc((size_t)(2 * n_places + 3 * n)));
        if (n_places > 0) {
            LOCREC_HIP_TRY(hipMemcpyAsync(d_nr.p, nr.place_lat, (size_t)n_places * 8, hipMemcpyHostToDevice, s));
            LOCREC_HIP_TRY(hipMemcpyAsync(d_nr.p + n_places, nr.place_lon, (size_t)n_places * 8, hipMemcpyHostToDevice, s));
        }
        LOCREC_HIP_TRY(hipMemcpyAsync(d_nr.p + 2 * n_places, h_near.data(), (size_t)(3 * n) * 8, hipMemcpyHostToDevice, s));
        near.place_lat = d_nr.p;
        near.place_lon = d_nr.p + n_places;
        near.center_lat = d_nr.p + 2 * n_places;
        near.center_lon = near.center_lat + n;
        near.radius = near.center_lon + n;
        return LOCREC_OK;
    }

    // The categories, uploaded once into d_cat (which outlives the call's launches): begins, lengths and caps in emit
    // order, then the place rows' categories and the listed categories
    int32_t upload_categories(const std::vector<int64_t> &ord, const RankCatHost &ch, DevBuf<int64_t> &d_cat)
    {
        LOCREC_TRY(d_cat.alloc(std::max<size_t>(1, ch.words(n_places, n, true))));
        return ch.upload(n_places, n, ord.data(), d_cat.p, nullptr, s, h_cat, cat);
    }

    // ranks the filled group and brings its rows to the host
    int32_t flush_group()
    {
        const int64_t ka = group == 0 ? (int64_t)0 : groups.group_end[group - 1], nseg = groups.group_end[group] - ka;
        ++group;
        ++stats.groups;
        if (Nd == 0) return LOCREC_OK;  // every count is 0
        int64_t *d_oid = d_out.p, *d_ocnt = d_out.p + 2 * groups.max_req * Nd;
        double *d_osc = reinterpret_cast<double *>(d_out.p + groups.max_req * Nd);
        double *d_omet = reinterpret_cast<double *>(d_ocnt + groups.max_req);
        if (cat.allow_begin || cat.caps) {
            RankExclude ex;
            if (d_ex_begin) ex = {d_ex_begin + ka, d_ex_len + ka, d_ex_ids, n_ex};
            RankNear nr;
            if (near.center_lat) nr = {near.center_lat + ka, near.center_lon + ka, near.radius + ka, near.place_lat, near.place_lon};
            RankCategory ct = cat;  // the group's sub-range of the lists and caps
            if (ct.allow_begin) {
                ct.allow_begin += ka;
                ct.allow_len += ka;
            }
            if (ct.caps) ct.caps += ka;
            LOCREC_TRY(rank_segments_device_by_category(nseg, d_seg_begin + ka, d_seg_len + ka, d_row_ids, d_row_probs, n_places, d_pid,
                                                        d_preg, d_tgt + ka, Nd, ex, nr, ct, d_oid, d_osc,
                                                        near.center_lat ? d_omet : nullptr, d_ocnt, nullptr, 0, s));
        } else if (near.center_lat) {
            RankExclude ex;
            if (d_ex_begin) ex = {d_ex_begin + ka, d_ex_len + ka, d_ex_ids, n_ex};
            const RankNear nr = {near.center_lat + ka, near.center_lon + ka, near.radius + ka, near.place_lat, near.place_lon};
            LOCREC_TRY(rank_segments_device_near(nseg, d_seg_begin + ka, d_seg_len + ka, d_row_ids, d_row_probs, n_places, d_pid, d_preg,
                                                 d_tgt + ka, Nd, ex, nr, d_oid, d_osc, d_omet, d_ocnt, nullptr, 0, s));
        } else if (d_ex_begin)
            LOCREC_TRY(rank_segments_device_excluding(nseg, d_seg_begin + ka, d_seg_len + ka, d_row_ids, d_row_probs, n_places, d_pid,
                                                      d_preg, d_tgt + ka, Nd, d_ex_begin + ka, d_ex_len + ka, n_ex, d_ex_ids, d_oid,
                                                      d_osc, d_ocnt, nullptr, 0, s));
        else
            LOCREC_TRY(rank_segments_device(nseg, d_seg_begin + ka, d_seg_len + ka, d_row_ids, d_row_probs, n_places, d_pid, d_preg,
                                            d_tgt + ka, Nd, d_oid, d_osc, d_ocnt, nullptr, 0, s));
        const RankBatchStats &rs = rank_batch_stats();
        stats.host_syncs += rs.host_syncs;
        // the ranker's plan header (one word more with lists), the global path's row count
        stats.readback_bytes += (cat.allow_begin || cat.caps ? 56 : d_ex_begin ? 40 : 32) + (rs.sorted ? 4 : 0);
        LOCREC_HIP_TRY(hipMemcpyAsync(h_oid.data() + ka * Nd, d_oid, (size_t)(nseg * Nd) * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(h_osc.data() + ka * Nd, d_osc, (size_t)(nseg * Nd) * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(h_cnt.data() + ka, d_ocnt, (size_t)nseg * 8, hipMemcpyDeviceToHost, s));
        if (near.center_lat)
            LOCREC_HIP_TRY(hipMemcpyAsync(h_omet.data() + ka * Nd, d_omet, (size_t)(nseg * Nd) * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (the next group's rows overwrite these)
        ++stats.host_syncs;
        stats.readback_bytes += nseg * ((near.center_lat ? 24 : 16) * Nd + 8);
        return LOCREC_OK;
    }

    // After the tile loop (its status, its polls of 4 bytes each): the columns' row counts and what the segments took,
    // then the caller's order and stride.  Input position i asks member member_of[i] for its distinct target uniq_of[i].
    int32_t finish(int32_t status, int64_t polls, const SgRkPoolOrder &order, const std::vector<int32_t> &member_of,
                   const std::vector<int32_t> &uniq_of, int64_t *out_ids, double *out_probabilities, int64_t *out_counts,
                   int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged, double *out_meters = nullptr)
    {
        stats.readback_bytes += polls * 4;
        stats.host_syncs += polls;
        LOCREC_TRY(status);
        std::vector<int64_t> tail((size_t)n + res_it.size());  // seg_len, col_rows
        LOCREC_HIP_TRY(hipMemcpyAsync(tail.data(), d_seg_len, tail.size() * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        ++stats.host_syncs;
        stats.readback_bytes += (int64_t)tail.size() * 8;
        for (int64_t k = 0; k < n; ++k) {
            stats.emitted_rows += tail[(size_t)k];
            const int64_t i = order.ord[(size_t)k];
            const size_t f = order.ubase[(size_t)member_of[(size_t)i]] + (size_t)uniq_of[(size_t)i];
            const int64_t c = Nd > 0 ? h_cnt[(size_t)k] : 0;
            out_counts[i] = c;
            if (N > 0) {
                std::copy(h_oid.begin() + k * Nd, h_oid.begin() + k * Nd + c, out_ids + i * N);
                std::copy(h_osc.begin() + k * Nd, h_osc.begin() + k * Nd + c, out_probabilities + i * N);
                std::fill(out_ids + i * N + c, out_ids + (i + 1) * N, (int64_t)-1);
                std::fill(out_probabilities + i * N + c, out_probabilities + (i + 1) * N, 0.0);
                if (out_meters) {
                    std::copy(h_omet.begin() + k * Nd, h_omet.begin() + k * Nd + c, out_meters + i * N);
                    std::fill(out_meters + i * N + c, out_meters + (i + 1) * N, 0.0);
                }
            }
            if (out_row_counts) out_row_counts[i] = tail[(size_t)n + f];
            if (out_iterations) out_iterations[i] = res_it[f];
            if (out_converged) out_converged[i] = res_conv[f];
        }
        return LOCREC_OK;
    }
};

template <class Tiles>
int32_t sg_ranked_batch_columns(locrec_sg_graph *g, SgRankedStats &stats, int64_t n, const std::vector<int32_t> &uniq,
                                const std::vector<int32_t> &uniq_of, Tiles &&tiles, double alpha, double epsilon,
                                int64_t max_iterations, int64_t N, int64_t n_places, const int64_t *place_ids,
                                const int64_t *place_region_ids, const int64_t *target_region_ids, bool with_lists,
                                const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids, int64_t *out_ids,
                                double *out_probabilities, int64_t *out_counts, int64_t *out_row_counts, int64_t *out_iterations,
                                int32_t *out_converged, const SgRkNear *near = nullptr, const RankCatHost *cat = nullptr);

// The exclusion lists' checks (host arrays), before any device work
int32_t sg_rk_check_lists(int64_t n_targets, const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids)
{
    if (n_excluded < 0 || n_excluded >= ((int64_t)1 << 31)) return fail(LOCREC_E_INVALID_ARG, "excluded id count out of range [0, 2^31)");
    if (n_targets > 0 && (!excluded_offsets || (n_excluded > 0 && !excluded_ids))) return fail(LOCREC_E_INVALID_ARG, "null array");
    bool ok = n_targets == 0 || (excluded_offsets[0] >= 0 && excluded_offsets[n_targets] <= n_excluded);
    for (int64_t i = 0; ok && i < n_targets; ++i) ok = excluded_offsets[i] <= excluded_offsets[i + 1];
    if (!ok) return fail(LOCREC_E_INVALID_ARG, "excluded_offsets must be non-decreasing inside [0, n_excluded]");
    return LOCREC_OK;
}

// both entries of the ranked batch; with_lists: position i leaves out excluded_ids[excluded_offsets[i] ..
// excluded_offsets[i + 1]) (host arrays, refused before any device work when they are not offsets into n_excluded ids)
int32_t sg_recommend_ranked_batch(locrec_sg_graph *g, int64_t n_targets, const int64_t *vertex_ids, double alpha, double epsilon,
                                  int64_t max_iterations, int64_t n_places, const int64_t *place_ids,
                                  const int64_t *place_region_ids, const int64_t *target_region_ids, int64_t max_recommendations,
                                  bool with_lists, const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids,
                                  int64_t *out_ids, double *out_probabilities, int64_t *out_counts, int64_t *out_row_counts,
                                  int64_t *out_iterations, int32_t *out_converged, const SgRkNear *near = nullptr,
                                  const RankCatHost *cat = nullptr)
{
    SgRankedStats &stats = sg_ranked_stats();
    stats = SgRankedStats();
    if (!g) return fail(LOCREC_E_INVALID_ARG, "graph is NULL");
    if (n_targets < 0 || (n_targets > 0 && !vertex_ids)) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    int64_t N = 0;
    LOCREC_TRY(sg_rk_check_args(n_targets, n_places, place_ids, place_region_ids, target_region_ids, max_recommendations, out_ids,
                                out_probabilities, out_counts, N));
    if (with_lists) LOCREC_TRY(sg_rk_check_lists(n_targets, excluded_offsets, n_excluded, excluded_ids));
    std::vector<int32_t> uniq, uniq_of;
    LOCREC_TRY(sg_batch_targets(g, n_targets, vertex_ids, epsilon, max_iterations, uniq, uniq_of));
    if (n_targets == 0) return LOCREC_OK;
    return sg_ranked_batch_columns(g, stats, n_targets, uniq, uniq_of, SgPersonTiles{uniq}, alpha, epsilon, max_iterations, N, n_places,
                                   place_ids, place_region_ids, target_region_ids, with_lists, excluded_offsets, n_excluded,
                                   excluded_ids, out_ids, out_probabilities, out_counts, out_row_counts, out_iterations,
                                   out_converged, near, cat);
}

// The ranked batch behind its checks, for n >= 1 positions over the columns `tiles` runs: position i asks column uniq_of[i],
// whose target vertex is uniq[...] (-1: a visitor, which is no vertex and so never a row of its own result)
template <class Tiles>
int32_t sg_ranked_batch_columns(locrec_sg_graph *g, SgRankedStats &stats, int64_t n, const std::vector<int32_t> &uniq,
                                const std::vector<int32_t> &uniq_of, Tiles &&tiles, double alpha, double epsilon,
                                int64_t max_iterations, int64_t N, int64_t n_places, const int64_t *place_ids,
                                const int64_t *place_region_ids, const int64_t *target_region_ids, bool with_lists,
                                const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids, int64_t *out_ids,
                                double *out_probabilities, int64_t *out_counts, int64_t *out_row_counts, int64_t *out_iterations,
                                int32_t *out_converged, const SgRkNear *near, const RankCatHost *cat)
{
    LOCREC_HIP_TRY(hipSetDevice(g->device));
    hipStream_t s = g->stream;
    const size_t nu = uniq.size();
    const int32_t T = g->nlive;
    const int tile_max = tiles.tile_max(g);

    // ---- the emit rows
    SgRkRows er;
    sg_rk_rows(g, sg_rk_dead_rows(alpha, max_iterations), er);
    const int64_t m = er.m;
    const int64_t *sid = er.sid;
    const std::vector<int32_t> &srow = er.srow;
    auto emit_row_of = [&](int32_t tv) -> int32_t { return tv < 0 ? -1 : sg_rk_row_of(g, er, tv); };
    const int64_t words = std::max<int64_t>(1, (m + 63) / 64);

    // ---- the requests in emit order (by tile, then input position: a pool's with one member), the distinct target regions
    std::vector<int64_t> regions(target_region_ids, target_region_ids + n);
    std::sort(regions.begin(), regions.end());
    regions.erase(std::unique(regions.begin(), regions.end()), regions.end());
    const int64_t R = (int64_t)regions.size();
    const std::vector<int32_t> member_of((size_t)n, 0);
    SgRkPoolOrder order;
    sg_rk_pool_order({nu}, {tile_max}, member_of, uniq_of, order);
    const std::vector<int64_t> &ord = order.ord;
    std::vector<int32_t> req((size_t)(3 * n));  // column, target's emit row, bitmap
    std::vector<int64_t> tgt_k((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = ord[(size_t)k];
        const int32_t u = uniq_of[(size_t)i];
        req[(size_t)k] = u % tile_max;
        req[(size_t)(n + k)] = emit_row_of(uniq[(size_t)u]);
        req[(size_t)(2 * n + k)] = (int32_t)(std::lower_bound(regions.begin(), regions.end(), target_region_ids[i]) - regions.begin());
        tgt_k[(size_t)k] = target_region_ids[i];
    }

    // ---- device buffers: the 8-byte inputs and counters, the 4-byte inputs, the bitmaps
    //   d64: place ids, place regions | distinct regions | sid | eid | targets | seg_begin | seg_len | col_rows | caps
    DevBuf<int64_t> d64;
    DevBuf<int32_t> d32;
    DevBuf<unsigned long long> d_bits;
    LOCREC_TRY(d64.alloc((size_t)(2 * n_places + 2 * R + 2 * m + 3 * n) + nu));
    LOCREC_TRY(d32.alloc((size_t)(m + 3 * n)));
    LOCREC_TRY(d_bits.alloc((size_t)(R * words)));
    int64_t *d_pid = d64.p, *d_preg = d_pid + n_places, *d_regions = d_preg + n_places, *d_sid = d_regions + R, *d_eid = d_sid + m,
            *d_tgt = d_eid + m, *d_seg_begin = d_tgt + n, *d_seg_len = d_seg_begin + n, *d_col_rows = d_seg_len + n,
            *d_caps = d_col_rows + nu;
    int32_t *d_srow = d32.p, *d_req = d_srow + m;
    if (n_places > 0) {
        LOCREC_HIP_TRY(hipMemcpyAsync(d_pid, place_ids, (size_t)n_places * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_preg, place_region_ids, (size_t)n_places * 8, hipMemcpyHostToDevice, s));
    }
    LOCREC_HIP_TRY(hipMemcpyAsync(d_regions, regions.data(), (size_t)R * 8, hipMemcpyHostToDevice, s));
    if (m > 0) {
        LOCREC_HIP_TRY(hipMemcpyAsync(d_sid, sid, (size_t)m * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_srow, srow.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
    }
    LOCREC_HIP_TRY(hipMemcpyAsync(d_tgt, tgt_k.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(d_req, req.data(), (size_t)(3 * n) * 4, hipMemcpyHostToDevice, s));
    LOCREC_HIP_TRY(hipMemsetAsync(d_seg_len, 0, ((size_t)n + nu) * 8, s));  // the segments' lengths and the columns' rows
    LOCREC_HIP_TRY(hipMemsetAsync(d_bits.p, 0, (size_t)(R * words) * 8, s));
    if (m > 0) hipLaunchKernelGGL(sg_rk_row_ids, rk_grid(m), dim3(kRkThreads), 0, s, m, d_sid, d_srow, d_eid);
    if (n_places > 0 && m > 0)
        hipLaunchKernelGGL(sg_rk_members, rk_grid(n_places), dim3(kRkThreads), 0, s, n_places, d_pid, d_preg, R, d_regions, m, d_sid,
                           d_srow, words, d_bits.p);
    hipLaunchKernelGGL(sg_rk_popcount, dim3((unsigned)R), dim3(kRkThreads), 0, s, words, d_bits.p,
                       reinterpret_cast<unsigned long long *>(d_caps));

    // ---- the groups (request k's room: its region's cap), the group's buffers
    SgRkCall rc{.stats = stats, .s = s, .n = n, .N = N, .n_places = n_places, .d_pid = d_pid, .d_preg = d_preg, .d_tgt = d_tgt,
                .d_seg_begin = d_seg_begin, .d_seg_len = d_seg_len};
    DevBuf<double> d_nr;  // the circles
    if (near) LOCREC_TRY(rc.upload_circles(ord, *near, d_nr));
    LOCREC_TRY(rc.plan(d_caps, (size_t)R, req.data() + 2 * n, nu));
    DevBuf<int64_t> d_ex, d_cat;  // the lists; the categories
    if (with_lists) LOCREC_TRY(rc.upload_lists(ord, excluded_offsets, n_excluded, excluded_ids, d_ex));
    if (cat && cat->given()) LOCREC_TRY(rc.upload_categories(ord, *cat, d_cat));
    DevBuf<unsigned char> d_state;
    LOCREC_TRY(d_state.alloc(kRkStateBytes));

    const unsigned emit_blocks = (unsigned)std::max<int64_t>(1, (m + kRkThreads - 1) / kRkThreads);
    auto after_tile = [&](SgBatchCtx &ctx, size_t t0, int nb) -> int32_t {
        ++stats.tiles;
        // the state first: it does not wait for the emit
        unsigned char *stg = g->no_pack ? nullptr : g->stage(kRkStateBytes);
        void *stg_dev = nullptr;
        const bool pinned = stg && hipHostGetDevicePointer(&stg_dev, stg, 0) == hipSuccess;
        if (!pinned) (void)hipGetLastError();
        hipLaunchKernelGGL(sg_rk_state, dim3(1), dim3(64 * kBatchB), 0, s, ctx.bstate, g->D2W.p,
                           pinned ? static_cast<unsigned char *>(stg_dev) : d_state.p);
        unsigned char own[kRkStateBytes];
        if (!pinned) LOCREC_HIP_TRY(hipMemcpyAsync(own, d_state.p, kRkStateBytes, hipMemcpyDeviceToHost, s));
        SgEmitTile tl{};
        tl.nb = nb;
        tl.T = T;
        tl.ne = (int32_t)m;
        tl.xstride = ctx.xstride;
        tl.count_cols = 1;
        for (int j = 0; j < kBatchB; ++j) tl.col_trow[j] = j < nb ? emit_row_of(uniq[t0 + (size_t)j]) : -1;
        // the tile's requests, group by group
        int64_t k = order.first[t0];
        const int64_t kb = order.tile_end(0, t0 / (size_t)tile_max, tile_max);
        while (k < kb) {
            const int64_t ke = std::min(kb, rc.groups.group_end[rc.group]);
            hipLaunchKernelGGL(sg_rk_emit, dim3(emit_blocks), dim3(kRkThreads), 0, s, tl, ctx.bstate, g->PA4.p, d_eid, d_bits.p,
                               words, (int32_t)k, (int32_t)ke, d_req, d_req + n, d_req + 2 * n, d_seg_begin,
                               reinterpret_cast<unsigned long long *>(d_seg_len), rc.groups.max_rows, rc.d_row_ids, rc.d_row_probs,
                               reinterpret_cast<unsigned long long *>(d_col_rows) + t0);
            tl.count_cols = 0;
            k = ke;
            if (k == rc.groups.group_end[rc.group]) LOCREC_TRY(rc.flush_group());
        }
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        LOCREC_HIP_TRY(hipGetLastError());
        ++stats.host_syncs;
        stats.readback_bytes += (int64_t)kRkStateBytes;
        return sg_rk_verdicts(pinned ? stg : own, nb, ctx.eps2, ctx.max_iterations, &rc.res_it[t0], &rc.res_conv[t0]);
    };
    SgBatchCtx ctx;
    const int32_t status = sg_batch_tiles_of(g, tiles, alpha, epsilon, max_iterations, ctx, after_tile);
    return rc.finish(status, ctx.polls, order, member_of, uniq_of, out_ids, out_probabilities, out_counts, out_row_counts,
                     out_iterations, out_converged, near ? near->meters : nullptr);
}

}  // namespace

extern "C" int32_t locrec_sg_recommend_ranked_batch_near(
    locrec_sg_graph *g, int64_t n_targets, const int64_t *vertex_ids, double alpha, double epsilon, int64_t max_iterations,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids, const double *place_latitudes,
    const double *place_longitudes, const int64_t *target_region_ids, const double *center_latitudes,
    const double *center_longitudes, const double *radius_meters, int64_t max_recommendations, const int64_t *excluded_offsets,
    int64_t n_excluded, const int64_t *excluded_ids, int64_t *out_ids, double *out_probabilities, double *out_meters,
    int64_t *out_counts, int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged) try
{
    // the circles' and the lists' requires first: before the graph is looked at
    if (n_targets < 0 || n_places < 0 || n_places >= ((int64_t)1 << 31)) return fail(LOCREC_E_INVALID_ARG, "target or place count out of range");
    if ((n_targets > 0 && (!center_latitudes || !center_longitudes || !radius_meters)) ||
        (n_places > 0 && (!place_latitudes || !place_longitudes)))
        return fail(LOCREC_E_INVALID_ARG, "null coordinate or radius array");
    LOCREC_TRY(rank_near_check_host(n_targets, center_latitudes, center_longitudes, radius_meters, n_places, place_latitudes,
                                    place_longitudes));
    const bool with_lists = excluded_offsets != nullptr;
    if (with_lists) LOCREC_TRY(sg_rk_check_lists(n_targets, excluded_offsets, n_excluded, excluded_ids));
    const SgRkNear near = {place_latitudes, place_longitudes, center_latitudes, center_longitudes, radius_meters, out_meters};
    return sg_recommend_ranked_batch(g, n_targets, vertex_ids, alpha, epsilon, max_iterations, n_places, place_ids, place_region_ids,
                                     target_region_ids, max_recommendations, with_lists, excluded_offsets, with_lists ? n_excluded : 0,
                                     excluded_ids, out_ids, out_probabilities, out_counts, out_row_counts, out_iterations,
                                     out_converged, &near);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_recommend_ranked_batch_by_category(
    locrec_sg_graph *g, int64_t n_targets, const int64_t *vertex_ids, double alpha, double epsilon, int64_t max_iterations,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids, const double *place_latitudes,
    const double *place_longitudes, const int64_t *place_category_ids, const int64_t *target_region_ids,
    const double *center_latitudes, const double *center_longitudes, const double *radius_meters, int64_t max_recommendations,
    const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids, const int64_t *allowed_offsets,
    int64_t n_allowed, const int64_t *allowed_category_ids, const int64_t *max_per_category, int64_t *out_ids,
    double *out_probabilities, double *out_meters, int64_t *out_counts, int64_t *out_row_counts, int64_t *out_iterations,
    int32_t *out_converged) try
{
    // the circles', the lists' and the caps' requires first: before the graph is looked at
    if (n_targets < 0 || n_places < 0 || n_places >= ((int64_t)1 << 31)) return fail(LOCREC_E_INVALID_ARG, "target or place count out of range");
    const bool circles = place_latitudes || place_longitudes || center_latitudes || center_longitudes || radius_meters;
    if (circles) {
        if ((n_targets > 0 && (!center_latitudes || !center_longitudes || !radius_meters)) ||
            (n_places > 0 && (!place_latitudes || !place_longitudes)))
            return fail(LOCREC_E_INVALID_ARG, "null coordinate or radius array");
        LOCREC_TRY(rank_near_check_host(n_targets, center_latitudes, center_longitudes, radius_meters, n_places, place_latitudes,
                                        place_longitudes));
    }
    const bool with_lists = excluded_offsets != nullptr;
    if (with_lists) LOCREC_TRY(sg_rk_check_lists(n_targets, excluded_offsets, n_excluded, excluded_ids));
    RankCatHost cat;
    cat.place_cat = place_category_ids;
    cat.allowed_offsets = allowed_offsets;
    cat.n_allowed = allowed_offsets ? n_allowed : 0;
    cat.allowed_ids = allowed_category_ids;
    cat.caps = max_per_category;
    LOCREC_TRY(cat.check(n_targets, n_places));
    const SgRkNear near = {place_latitudes, place_longitudes, center_latitudes, center_longitudes, radius_meters, out_meters};
    return sg_recommend_ranked_batch(g, n_targets, vertex_ids, alpha, epsilon, max_iterations, n_places, place_ids, place_region_ids,
                                     target_region_ids, max_recommendations, with_lists, excluded_offsets, with_lists ? n_excluded : 0,
                                     excluded_ids, out_ids, out_probabilities, out_counts, out_row_counts, out_iterations,
                                     out_converged, circles ? &near : nullptr, &cat);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_recommend_ranked_batch(locrec_sg_graph *g, int64_t n_targets, const int64_t *vertex_ids, double alpha,
                                                    double epsilon, int64_t max_iterations, int64_t n_places,
                                                    const int64_t *place_ids, const int64_t *place_region_ids,
                                                    const int64_t *target_region_ids, int64_t max_recommendations,
                                                    int64_t *out_ids, double *out_probabilities, int64_t *out_counts,
                                                    int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged) try
{
    return sg_recommend_ranked_batch(g, n_targets, vertex_ids, alpha, epsilon, max_iterations, n_places, place_ids, place_region_ids,
                                     target_region_ids, max_recommendations, false, nullptr, 0, nullptr, out_ids, out_probabilities,
                                     out_counts, out_row_counts, out_iterations, out_converged);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_recommend_ranked_batch_excluding(locrec_sg_graph *g, int64_t n_targets, const int64_t *vertex_ids,
                                                              double alpha, double epsilon, int64_t max_iterations,
                                                              int64_t n_places, const int64_t *place_ids,
                                                              const int64_t *place_region_ids, const int64_t *target_region_ids,
                                                              int64_t max_recommendations, const int64_t *excluded_offsets,
                                                              int64_t n_excluded, const int64_t *excluded_ids, int64_t *out_ids,
                                                              double *out_probabilities, int64_t *out_counts,
                                                              int64_t *out_row_counts, int64_t *out_iterations,
                                                              int32_t *out_converged) try
{
    return sg_recommend_ranked_batch(g, n_targets, vertex_ids, alpha, epsilon, max_iterations, n_places, place_ids, place_region_ids,
                                     target_region_ids, max_recommendations, true, excluded_offsets, n_excluded, excluded_ids,
                                     out_ids, out_probabilities, out_counts, out_row_counts, out_iterations, out_converged);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_recommend_ranked_batch_stats(int64_t *out_tiles, int64_t *out_groups, int64_t *out_emitted_rows,
                                                          int64_t *out_readback_bytes, int64_t *out_host_syncs) try
{
    const SgRankedStats &st = sg_ranked_stats();
    if (out_tiles) *out_tiles = st.tiles;
    if (out_groups) *out_groups = st.groups;
    if (out_emitted_rows) *out_emitted_rows = st.emitted_rows;
    if (out_readback_bytes) *out_readback_bytes = st.readback_bytes;
    if (out_host_syncs) *out_host_syncs = st.host_syncs;
    return LOCREC_OK;
} LOCREC_CATCH_ALL
