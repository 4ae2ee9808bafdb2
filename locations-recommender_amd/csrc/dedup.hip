// dedup.hip -- the place deduplicator on the device:
//
//   PlaceDeduplicator.dropDuplicates   deduplicator/PlaceDeduplicator.scala:13-54
//   Levenshtein.lev                    deduplicator/Levenshtein.scala:18-57
//
// The reference joins places with the confirmed places of the same region (a per-region cross join, :38-40) and
// runs a UDF per pair: two Locations, one haversine, two toLowerCase and an O(len1 * len2) Levenshtein with a freshly
// allocated matrix (:25-36).  A pair can only be "the same place" when it is within the radius, so here the band /
// cell grid of the visit join (place_grid.h) prunes by distance first, with the same exact fp64 haversine, and the
// edit distance runs on the survivors only - and only as far as "is it <= maxNameDifference, and if so what is it"
// needs: a thresholded (Ukkonen) band of 2k + 1 cells per row that lives in registers.
//
// Names arrive as CSR (offsets + UTF-16 code units), already lower-cased by the caller: toLowerCase is the host
// language's own, locale rules included.  Levenshtein.lev compares Java chars, i.e. code units.

#include "dev_prims.h"

#include <algorithm>
#include <cmath>
#include <limits>

#include "common.h"
#include "place_grid.h"

namespace {

using namespace locrec;

constexpr int32_t kInf = 1 << 29;              // "no path": larger than any distance, small enough to add 1 to
constexpr int64_t kDefaultPairBudget = (int64_t)1 << 26;  // candidate pairs per chunk of places
constexpr int64_t kMaxPairBudget = (int64_t)1 << 30;
constexpr int32_t kLdsCells = 1280;            // DP row cells of 64 lanes x u16 that fit the 160 KiB of a CU
constexpr int64_t kLdsMaxLong = 65535;         // ... whose values (<= the longer name's length) fit u16
constexpr int64_t kScratchBytes = (int64_t)256 << 20;  // global DP rows of the names beyond that, per launch
constexpr int32_t kMaxThreshold = std::numeric_limits<int32_t>::max() - 1;  // every kernel computes k + 1 in int32

// LOCREC_DEDUP_PAIR_BUDGET: candidate pairs per chunk (the result does not depend on it; read at every call so that a
// test can force many chunks).  LOCREC_DEDUP_FULL_DP=1: every candidate goes through the full matrix of
// Levenshtein.scala - no length pre-test, no band, no early exit - the A/B partner of the banded kernel.
// LOCREC_DEDUP_SCRATCH_BYTES: bytes of global DP rows per launch of tier (c), 4 .. 256 MiB (the default); one pair at
// least per launch.  The result does not depend on it; read at every call so that a test can force many launches.
int64_t pair_budget()
{
    int64_t b = kDefaultPairBudget;
    if (const char *e = std::getenv("LOCREC_DEDUP_PAIR_BUDGET")) b = atoll(e);
    return std::min(std::max<int64_t>(b, 1), kMaxPairBudget);
}

int64_t scratch_bytes()
{
    int64_t b = kScratchBytes;
    if (const char *e = std::getenv("LOCREC_DEDUP_SCRATCH_BYTES")) b = atoll(e);
    return std::min(std::max<int64_t>(b, 4), kScratchBytes);
}

// A threshold of INT32_MAX ("names do not matter") is served as INT32_MAX - 1: no name has that many units, so no
// result changes, and k + 1 stays an int32.
int32_t clamp_threshold(int32_t k) { return std::min(k, kMaxThreshold); }

bool full_dp_forced()
{
    const char *e = std::getenv("LOCREC_DEDUP_FULL_DP");
    return e && e[0] && e[0] != '0';
}

struct DedupStats {
    int64_t candidates = 0, same = 0, chunks = 0;
    double ms[3] = {0, 0, 0};  // grid (keys, sorts, walks), Levenshtein, compaction
};
thread_local DedupStats g_dedup_stats;

enum { kPhaseGrid = 0, kPhaseLev = 1, kPhaseCompact = 2, kPhaseEnd = -1 };

// ---- names ------------------------------------------------------------------------------------------------------------

// CSR offsets must start at or above 0 and never decrease: every kernel below trusts them as array bounds
__global__ void dd_check_offsets(int64_t n, const int64_t *off, uint32_t *bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (off[i] < 0 || (i < n && off[i + 1] < off[i])) *bad = 1u;
}

struct Names {
    In<int64_t> off;
    In<uint16_t> units;
};

// bind the CSR of n names: the offsets first, then offsets[n] code units
int32_t bind_names(Names &N, int64_t n, const int64_t *offsets, const uint16_t *units, int32_t mem, const char *what,
                   hipStream_t s)
{
    LOCREC_TRY(N.off.bind(offsets, n + 1, mem, s));
    DevBuf<uint32_t> bad;
    LOCREC_TRY(bad.alloc(1));
    LOCREC_HIP_TRY(hipMemsetAsync(bad.p, 0, 4, s));
    LOCREC_LAUNCH(dd_check_offsets, grid_for(n + 1), dim3(256), 0, s, n, N.off.p, bad.p);
    uint32_t is_bad = 0;
    int64_t total = 0;
    LOCREC_HIP_TRY(hipMemcpyAsync(&is_bad, bad.p, 4, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&total, N.off.p + n, 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    if (is_bad) return fail(LOCREC_E_INVALID_ARG, "%s name offsets must start at or above 0 and never decrease", what);
    if (total > 0 && !units) return fail(LOCREC_E_INVALID_ARG, "null array (%s name units)", what);
    LOCREC_TRY(N.units.bind(units, total, mem, s));
    return LOCREC_OK;
}

// ---- Levenshtein.lev (Levenshtein.scala:18-57) ---------------------------------------------------------------------------

struct PairNames {
    const uint16_t *a, *b;
    int64_t la, lb;
};

// pair t of the list: rows (pa[t], pb[t]) of the two CSRs, or (t, t) without a list
__device__ __forceinline__ PairNames names_of(int64_t t, const uint32_t *pa, const uint32_t *pb, const int64_t *a_off,
                                              const uint16_t *a_units, const int64_t *b_off, const uint16_t *b_units)
{
    const int64_t ra = pa ? (int64_t)pa[t] : t, rb = pb ? (int64_t)pb[t] : t;
    PairNames n;
    n.a = a_units + a_off[ra];
    n.la = a_off[ra + 1] - a_off[ra];
    n.b = b_units + b_off[rb];
    n.lb = b_off[rb + 1] - b_off[rb];
    return n;
}

// Tier (a): min(lev, k + 1) for k <= K, one lane per pair, the band of 2K + 1 cells in registers.
// Row i of the matrix d(i, j) (:21) is kept for j = i - K .. i + K only: d(i, j) >= |i - j|, so a cell outside the band
// exceeds K >= k and cannot lie on a path of cost <= k; the banded value is exact wherever lev <= K and above K
// otherwise.  band[c] is d(i, i - K + c); going from row i - 1 to row i the cell above is band[c + 1], the diagonal one
// band[c] itself, the left one the new band[c - 1] - so the row is updated in place, left to right.  bw[c] is the unit
// str2(j - 1) of that cell and shifts by one per row.  Every index is a compile-time constant after unrolling: no
// scratch.  A row whose band is above k everywhere ends the pair (:50 only ever adds).
template <int K>
__global__ __launch_bounds__(256) void dd_lev_band(int64_t m, const uint32_t *pa, const uint32_t *pb, const int64_t *a_off,
                                                   const uint16_t *a_units, const int64_t *b_off, const uint16_t *b_units,
                                                   int32_t k, int32_t *out)
{
    constexpr int W = 2 * K + 1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const PairNames n = names_of(t, pa, pb, a_off, a_units, b_off, b_units);
    const int64_t la = n.la, lb = n.lb;
    if (la - lb > k || lb - la > k) {  // |len1 - len2| insertions at least
        out[t] = k + 1;
        return;
    }
    int32_t band[W];
    uint32_t bw[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        const int j = c - K;  // row 0: d(0, j) = j (:32-36); row 1's units str2(j) at the same c
        band[c] = (j >= 0 && j <= lb) ? j : kInf;
        bw[c] = (j >= 0 && j < lb) ? (uint32_t)n.b[j] : 0xFFFFFFFFu;
    }
    for (int64_t i = 1; i <= la; ++i) {
        const uint32_t ai = n.a[i - 1];
        const int64_t j_lo = i - K;  // the column of band[0]
        int32_t left = kInf, row_min = kInf;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int64_t j = j_lo + c;
            const int32_t up = c + 1 < W ? band[c + 1] + 1 : kInf;        // d(i - 1, j) + 1     (:47)
            const int32_t diag = band[c] + (bw[c] != ai ? 1 : 0);         // d(i - 1, j - 1) + replaceCost (:42-49)
            int32_t v = min(min(diag, up), left + 1);                     // d(i, j - 1) + 1     (:48,50)
            if (j == 0) v = (int32_t)i;                                   // d(i, 0) = i         (:26-30)
            if (j < 0 || j > lb) v = kInf;
            band[c] = v;
            left = v;
            row_min = min(row_min, v);
        }
        if (row_min > k) {
            out[t] = k + 1;
            return;
        }
        const int64_t jn = i + K;  // str2 index of the unit entering on the right for row i + 1
        const uint32_t next = jn < lb ? (uint32_t)n.b[jn] : 0xFFFFFFFFu;
#pragma unroll
        for (int c = 0; c + 1 < W; ++c) bw[c] = bw[c + 1];
        bw[W - 1] = next;
    }
    const int at = (int)(lb - la) + K;  // d(len1, len2) (:56)
    int32_t res = kInf;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (c == at) res = band[c];
    out[t] = min(res, k + 1);
}

// which pairs the LDS row cannot hold (the shorter name + 1 cells, values up to the longer name's length in u16)
struct LevPlan {
    unsigned long long max_short;   // largest shorter-name length among the pairs the LDS row serves
    unsigned long long long_pairs;  // pairs it does not serve ...
    unsigned long long long_cells;  // ... and the largest shorter-name length + 1 among those
};

__device__ __forceinline__ bool lds_serves(int64_t shorter, int64_t longer) { return shorter + 1 <= kLdsCells && longer <= kLdsMaxLong; }

__global__ void dd_lev_plan(int64_t m, const uint32_t *pa, const uint32_t *pb, const int64_t *a_off, const int64_t *b_off,
                            LevPlan *plan, uint32_t *long_list)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const int64_t ra = pa ? (int64_t)pa[t] : t, rb = pb ? (int64_t)pb[t] : t;
    const int64_t la = a_off[ra + 1] - a_off[ra], lb = b_off[rb + 1] - b_off[rb];
    const int64_t shorter = min(la, lb), longer = max(la, lb);
    if (lds_serves(shorter, longer)) {
        atomicMax(&plan->max_short, (unsigned long long)shorter);
    } else {
        const unsigned long long at = atomicAdd(&plan->long_pairs, 1ull);
        long_list[at] = (uint32_t)t;
        atomicMax(&plan->long_cells, (unsigned long long)shorter + 1ull);
    }
}

// The matrix of Levenshtein.scala:22-56 kept as ONE row, d(i - 1, .) overwritten by d(i, .) left to right, the shorter
// name along the row (the distance is symmetric).  limit < 0: the full matrix.  limit >= 0: only the columns
// |i - j| <= limit of every row (a cell outside exceeds the limit, see dd_lev_band; it is read as kInf, never stored),
// and limit + 1 as soon as |len1 - len2| or a whole row exceeds the limit.  `cell(j)` addresses the lane's column of
// cells.  The row is walked in blocks of 8 columns: all loads of a block are issued before its first store, so their
// latencies overlap (the compiler cannot move a load across a store to the same array by itself).
template <class Cell, class Row>
__device__ __forceinline__ int32_t lev_one_row(const PairNames &n, int32_t limit, Row cell)
{
    constexpr int B = 8;
    const bool swap = n.lb > n.la;
    const uint16_t *rows = swap ? n.b : n.a, *cols = swap ? n.a : n.b;
    const int64_t nr = swap ? n.lb : n.la, nc = swap ? n.la : n.lb;
    if (limit >= 0 && nr - nc > limit) return limit + 1;
    const int64_t half = limit >= 0 ? (int64_t)limit : nr;  // columns i - half .. i + half of row i
    for (int64_t j = 0; j <= min(nc, half); ++j) cell(j) = (Cell)j;  // d(0, j) = j (:32-36)
    for (int64_t i = 1; i <= nr; ++i) {
        const uint16_t ri = rows[i - 1];
        const int64_t j_lo = max((int64_t)1, i - half), j_hi = min(nc, i + half);
        const int64_t up_max = i - 1 + half;  // the last column row i - 1 holds
        int32_t diag = (int32_t)cell(j_lo - 1), left = kInf, row_min = kInf;
        if (j_lo == 1) {  // d(i, 0) = i (:26-30)
            cell(0) = (Cell)i;
            left = row_min = (int32_t)i;
        }
        for (int64_t j0 = j_lo; j0 <= j_hi; j0 += B) {
            int32_t up[B], v[B];
            uint16_t cu[B];
#pragma unroll
            for (int t = 0; t < B; ++t)
                if (j0 + t <= j_hi) {
                    up[t] = j0 + t <= up_max ? (int32_t)cell(j0 + t) : kInf;
                    cu[t] = cols[j0 + t - 1];
                }
#pragma unroll
            for (int t = 0; t < B; ++t)
                if (j0 + t <= j_hi) {
                    v[t] = min(min(diag + (cu[t] != ri ? 1 : 0), up[t] + 1), left + 1);  // (:42-50)
                    diag = up[t];
                    left = v[t];
                    row_min = min(row_min, v[t]);
                }
#pragma unroll
            for (int t = 0; t < B; ++t)
                if (j0 + t <= j_hi) cell(j0 + t) = (Cell)v[t];
        }
        if (limit >= 0 && row_min > limit) return limit + 1;
    }
    return (int32_t)cell(nc);
}

// Tier (b): one lane per pair, the row in LDS as [cell][lane]: the 64 lanes of a wave touch one cell index at a time
// (their own j may differ, but each lane owns one column), so a wave's access to a cell is 64 consecutive u16 = 32
// dwords on 32 different banks.  No lane reads another lane's cells: no barrier.
__global__ __launch_bounds__(64) void dd_lev_lds(int64_t m, const uint32_t *pa, const uint32_t *pb, const int64_t *a_off,
                                                 const uint16_t *a_units, const int64_t *b_off, const uint16_t *b_units,
                                                 int32_t limit, int32_t k, int32_t cells, int32_t *out)
{
    extern __shared__ uint16_t dd_row[];
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    if (t >= m) return;
    const PairNames n = names_of(t, pa, pb, a_off, a_units, b_off, b_units);
    const int64_t shorter = min(n.la, n.lb), longer = max(n.la, n.lb);
    if (!lds_serves(shorter, longer) || shorter + 1 > cells) return;  // tier (c)'s pair
    const int32_t d = lev_one_row<uint16_t>(n, limit, [&](int64_t j) -> uint16_t & { return dd_row[j * 64 + lane]; });
    out[t] = k >= 0 ? min(d, k + 1) : d;
}

// Tier (c): the pairs of long_list[first .. first + count) with the row in global memory, [cell][pair of the launch]
__global__ void dd_lev_global(int64_t first, int64_t count, const uint32_t *long_list, const uint32_t *pa, const uint32_t *pb,
                              const int64_t *a_off, const uint16_t *a_units, const int64_t *b_off, const uint16_t *b_units,
                              int32_t limit, int32_t k, int32_t *scratch, int32_t *out)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= count) return;
    const int64_t t = long_list[first + u];
    const PairNames n = names_of(t, pa, pb, a_off, a_units, b_off, b_units);
    const int32_t d = lev_one_row<int32_t>(n, limit, [&](int64_t j) -> int32_t & { return scratch[j * count + u]; });
    out[t] = k >= 0 ? min(d, k + 1) : d;
}

// out[t] = lev of pair t (k < 0), or min(lev, k + 1)
int32_t lev_pairs(int64_t m, const uint32_t *pa, const uint32_t *pb, const int64_t *a_off, const uint16_t *a_units,
                  const int64_t *b_off, const uint16_t *b_units, int32_t k, bool full_dp, int32_t *out, hipStream_t s)
{
    if (m == 0) return LOCREC_OK;
    if (k >= 0 && !full_dp && k <= 15) {
        if (k <= 3)
            LOCREC_LAUNCH((dd_lev_band<3>), grid_for(m), dim3(256), 0, s, m, pa, pb, a_off, a_units, b_off, b_units, k, out);
        else if (k <= 7)
            LOCREC_LAUNCH((dd_lev_band<7>), grid_for(m), dim3(256), 0, s, m, pa, pb, a_off, a_units, b_off, b_units, k, out);
        else
            LOCREC_LAUNCH((dd_lev_band<15>), grid_for(m), dim3(256), 0, s, m, pa, pb, a_off, a_units, b_off, b_units, k, out);
        return LOCREC_OK;
    }
    const int32_t limit = full_dp ? -1 : k;
    DevBuf<LevPlan> plan;
    DevBuf<uint32_t> long_list;
    LOCREC_TRY(plan.alloc(1));
    LOCREC_TRY(long_list.alloc((size_t)m));
    LOCREC_HIP_TRY(hipMemsetAsync(plan.p, 0, sizeof(LevPlan), s));
    LOCREC_LAUNCH(dd_lev_plan, grid_for(m), dim3(256), 0, s, m, pa, pb, a_off, b_off, plan.p, long_list.p);
    LevPlan lp;
    LOCREC_READ_BACK(lp, plan.p, s);
    if ((int64_t)lp.long_pairs < m) {
        const int32_t cells = (int32_t)lp.max_short + 1;
        const size_t lds = (size_t)cells * 64 * sizeof(uint16_t);
        if (lds > 64 * 1024)
            LOCREC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(dd_lev_lds), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(kLdsCells * 64 * sizeof(uint16_t))));
        LOCREC_LAUNCH(dd_lev_lds, grid_for(m, 64), dim3(64), lds, s, m, pa, pb, a_off, a_units, b_off, b_units, limit, k, cells,
                      out);
    }
    if (lp.long_pairs) {
        const int64_t row_bytes = (int64_t)lp.long_cells * 4;
        const int64_t per_launch = std::max<int64_t>(1, std::min<int64_t>((int64_t)lp.long_pairs, scratch_bytes() / row_bytes));
        DevBuf<int32_t> scratch;
        LOCREC_TRY(scratch.alloc((size_t)(per_launch * (int64_t)lp.long_cells)));
        for (int64_t first = 0; first < (int64_t)lp.long_pairs; first += per_launch) {
            const int64_t count = std::min<int64_t>(per_launch, (int64_t)lp.long_pairs - first);
            LOCREC_LAUNCH(dd_lev_global, grid_for(count, 64), dim3(64), 0, s, first, count, long_list.p, pa, pb, a_off, a_units,
                          b_off, b_units, limit, k, scratch.p, out);
        }
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (scratch is released on return)
    }
    return LOCREC_OK;
}

// ---- the join of PlaceDeduplicator.scala:38-50 ----------------------------------------------------------------------------

__global__ void dd_region_rank_keys(int64_t nc, const int64_t *region, const uint32_t *rows, const int64_t *regions, int32_t nr,
                                    uint32_t *keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nc) keys[i] = (uint32_t)rank_of_region(regions, nr, region[rows[i]]);
}

// partners of place i: the confirmed rows of its region (:39) minus those with its own id (:40).  The confirmed rows are
// sorted by (region rank, id); the grid walk never sees a far-away row with an equal id, so this is a lookup of its own.
__global__ void dd_partners(int64_t np, const int64_t *p_id, const int64_t *p_region, const int64_t *regions, int32_t nr,
                            int64_t nc, const uint32_t *sorted_rank, const uint64_t *sorted_id, int64_t *partners)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const int64_t r = rank_of_region(regions, nr, p_region[i]);
    int64_t n = 0;
    if (r >= 0) {
        const int64_t lo = lower_bound<uint32_t>(sorted_rank, 0, nc, (uint32_t)r);
        const int64_t hi = lower_bound<uint32_t>(sorted_rank, lo, nc, (uint32_t)r + 1u);
        const uint64_t key = ordered_key(p_id[i]);
        const int64_t a = lower_bound<uint64_t>(sorted_id, lo, hi, key);
        int64_t b = a;
        if (key != ~0ull) b = lower_bound<uint64_t>(sorted_id, a, hi, key + 1ull);
        else b = hi;
        n = (hi - lo) - (b - a);
    }
    partners[i] = n;
}

// One thread per place of [p_begin, p_end): the confirmed places of the (at most) 3 bands x 3 cells around it.  A
// candidate is within max_meters (the first half of :34) and has another id (:40).  WRITE = false counts them;
// WRITE = true stores the confirmed rows at the place's offset, ascending.
template <bool WRITE>
__global__ void dd_walk(int64_t p_begin, int64_t p_end, const int64_t *p_id, const double *p_lat, const double *p_lon,
                        const int64_t *p_region, const int64_t *regions, int32_t nr, Grid g, double max_meters, int64_t nc,
                        const uint64_t *keys, const uint32_t *conf_rows, const int64_t *c_id, const double *c_lat,
                        const double *c_lon, unsigned long long *counts, const unsigned long long *offsets,
                        unsigned long long base, uint32_t *cand_place, uint32_t *cand_conf)
{
    const int64_t i = p_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p_end) return;
    unsigned long long found = 0;
    uint32_t *mine = WRITE ? cand_conf + (offsets[i] - base) : nullptr;
    const int64_t r = rank_of_region(regions, nr, p_region[i]);
    const double lat = p_lat[i], lon = p_lon[i];
    if (r >= 0 && location_ok(lat, lon)) {
        const int64_t id = p_id[i];
        for_each_grid_candidate(g, r, lat, lon, keys, nc, conf_rows, [&](uint32_t j) {
            if (c_id[j] != id && distance_meters(lat, lon, c_lat[j], c_lon[j]) <= max_meters) {
                if (WRITE) mine[found] = j;
                ++found;
            }
        });
    }
    if (!WRITE) {
        counts[i] = found;
        return;
    }
    sort_ascending(mine, found);
    uint32_t *who = cand_place + (offsets[i] - base);
    for (unsigned long long a = 0; a < found; ++a) who[a] = (uint32_t)i;
}

struct ChunkEnd {
    long long end;              // the chunk is the places [begin, end)
    unsigned long long pairs;   // ... and has this many candidates
};

// the longest run of places from `begin` whose candidates fit the budget; one place at least
__global__ void dd_chunk_end(int64_t np, const unsigned long long *offsets, unsigned long long total, int64_t begin,
                             unsigned long long budget, ChunkEnd *out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long base = offsets[begin];
    int64_t a = begin + 1, b = np;  // the answer lies in [a, b]
    while (a < b) {
        const int64_t mid = (a + b + 1) >> 1;
        const unsigned long long end_off = mid < np ? offsets[mid] : total;
        if (end_off - base <= budget) a = mid; else b = mid - 1;
    }
    out->end = a;
    out->pairs = (a < np ? offsets[a] : total) - base;
}

__global__ void dd_same_flags(int64_t m, const int32_t *dist, int32_t k, uint32_t *flags)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) flags[t] = dist[t] <= k ? 1u : 0u;  // the second half of :34-35, negated
}

// the same pairs of a chunk, in (place row, confirmed row) order, behind the `written` of the chunks before
__global__ void dd_emit_same(int64_t m, const uint32_t *flags, const uint32_t *pos, const uint32_t *cand_place,
                             const uint32_t *cand_conf, const int32_t *dist, int64_t written, int64_t cap, int64_t *out_place,
                             int64_t *out_conf, int32_t *out_diff)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m || !flags[t]) return;
    const int64_t w = written + (int64_t)pos[t];
    if (w >= cap) return;
    out_place[w] = (int64_t)cand_place[t];
    out_conf[w] = (int64_t)cand_conf[t];
    out_diff[w] = dist[t];
}

// not same = partners - same: how often the reference's inner join returns the place (:38-53)
__global__ void dd_subtract_same(int64_t p_begin, int64_t p_end, const unsigned long long *offsets,
                                 const unsigned long long *counts, unsigned long long base, const uint32_t *flags,
                                 int64_t *not_same)
{
    const int64_t i = p_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p_end) return;
    const uint32_t *f = flags + (offsets[i] - base);
    int64_t same = 0;
    for (unsigned long long a = 0; a < counts[i]; ++a) same += f[a];
    not_same[i] -= same;
}

}  // namespace

// Levenshtein.lev (deduplicator/Levenshtein.scala:18-57) of n pairs of names
extern "C" int32_t locrec_lev_distances(int64_t n, const int64_t *a_offsets, const uint16_t *a_units, const int64_t *b_offsets,
                                        const uint16_t *b_units, int32_t max_difference, int32_t mem, int32_t *out_distances)
try {
    LOCREC_TRY(mem_ok(mem));
    if (n < 0 || n >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "pair count out of range [0, 2^31)");
    if (n == 0) return LOCREC_OK;
    if (!a_offsets || !b_offsets || !out_distances) return fail(LOCREC_E_INVALID_ARG, "null array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Names A, B;
    Out<int32_t> o;
    LOCREC_TRY(bind_names(A, n, a_offsets, a_units, mem, "first", s));
    LOCREC_TRY(bind_names(B, n, b_offsets, b_units, mem, "second", s));
    LOCREC_TRY(o.bind(out_distances, n, mem));
    const int32_t k = max_difference < 0 ? -1 : clamp_threshold(max_difference);
    LOCREC_TRY(lev_pairs(n, nullptr, nullptr, A.off.p, A.units.p, B.off.p, B.units.p, k, full_dp_forced(), o.p, s));
    LOCREC_TRY(o.deliver(n, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

// PlaceDeduplicator.dropDuplicates (deduplicator/PlaceDeduplicator.scala:13-54): the pairs the UDF of :25-36 calls the
// same place, and per place how many pairs of the join of :38-40 it does not
extern "C" int32_t locrec_find_duplicate_places(
    int64_t n_places, const int64_t *p_ids, const int64_t *p_region_ids, const double *p_latitudes, const double *p_longitudes,
    const int64_t *p_name_offsets, const uint16_t *p_name_units, int64_t n_confirmed, const int64_t *c_ids,
    const int64_t *c_region_ids, const double *c_latitudes, const double *c_longitudes, const int64_t *c_name_offsets,
    const uint16_t *c_name_units, double max_meters, int32_t max_name_difference, int32_t mem, int64_t *out_place_rows,
    int64_t *out_confirmed_rows, int32_t *out_name_differences, int64_t *inout_count, int64_t *out_not_same_counts)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!inout_count) return fail(LOCREC_E_INVALID_ARG, "inout_count is required");
    const int64_t cap = *inout_count;
    *inout_count = 0;
    g_dedup_stats = DedupStats();
    if (cap < 0) return fail(LOCREC_E_INVALID_ARG, "negative capacity");
    if (n_places < 0 || n_places >= kMaxRows || n_confirmed < 0 || n_confirmed >= kMaxRows)
        return fail(LOCREC_E_INVALID_ARG, "row count out of range [0, 2^31)");
    // (a negative radius is legal - no pair is that close - but the grid cannot prune at or beyond the earth radius)
    if (max_meters != max_meters || !(max_meters < kEarthRadiusMeters))
        return fail(LOCREC_E_INVALID_ARG, "the search radius %g m must be below the earth radius", max_meters);
    if (n_places == 0) return LOCREC_OK;
    if (!p_ids || !p_region_ids || !p_latitudes || !p_longitudes || !p_name_offsets) return fail(LOCREC_E_INVALID_ARG, "null array");
    if (n_confirmed > 0 && (!c_ids || !c_region_ids || !c_latitudes || !c_longitudes || !c_name_offsets))
        return fail(LOCREC_E_INVALID_ARG, "null array");
    if (cap > 0 && (!out_place_rows || !out_confirmed_rows || !out_name_differences))
        return fail(LOCREC_E_INVALID_ARG, "null output array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Out<int64_t> ons;
    if (out_not_same_counts) LOCREC_TRY(ons.bind(out_not_same_counts, n_places, mem));
    if (n_confirmed == 0) {  // an empty join: every place disappears
        if (out_not_same_counts) {
            LOCREC_HIP_TRY(hipMemsetAsync(ons.p, 0, (size_t)n_places * 8, s));
            LOCREC_TRY(ons.deliver(n_places, s));
            LOCREC_HIP_TRY(hipStreamSynchronize(s));
        }
        return LOCREC_OK;
    }
    Temp tmp;
    PhaseClock clock;
    clock.s = s;
    In<int64_t> pi, pr, ci, cr;
    In<double> plat, plon, clat, clon;
    Names PN, CN;
    LOCREC_TRY(pi.bind(p_ids, n_places, mem, s));
    LOCREC_TRY(pr.bind(p_region_ids, n_places, mem, s));
    LOCREC_TRY(plat.bind(p_latitudes, n_places, mem, s));
    LOCREC_TRY(plon.bind(p_longitudes, n_places, mem, s));
    LOCREC_TRY(ci.bind(c_ids, n_confirmed, mem, s));
    LOCREC_TRY(cr.bind(c_region_ids, n_confirmed, mem, s));
    LOCREC_TRY(clat.bind(c_latitudes, n_confirmed, mem, s));
    LOCREC_TRY(clon.bind(c_longitudes, n_confirmed, mem, s));
    LOCREC_TRY(bind_names(PN, n_places, p_name_offsets, p_name_units, mem, "place", s));
    LOCREC_TRY(bind_names(CN, n_confirmed, c_name_offsets, c_name_units, mem, "confirmed place", s));
    LOCREC_TRY(clock.mark(kPhaseGrid));

    // distinct regions of the confirmed places, ascending
    DevBuf<int64_t> regions;
    int32_t nr = 0;
    LOCREC_TRY(distinct_ids(cr.p, n_confirmed, tmp, s, regions, &nr));
    if (nr >= (1 << 24)) return fail(LOCREC_E_INVALID_ARG, "%d distinct regions: at most 2^24 - 1 are supported", nr);

    // Location's require (Location.scala:7-8) for every row that meets a row of the other side
    DevBuf<uint32_t> has_place;
    DevBuf<LocationError> err;
    LOCREC_TRY(has_place.alloc((size_t)nr));
    LOCREC_TRY(err.alloc(1));
    LOCREC_HIP_TRY(hipMemsetAsync(has_place.p, 0, (size_t)nr * 4, s));
    LOCREC_HIP_TRY(hipMemsetAsync(err.p, 0xFF, sizeof(LocationError), s));
    LOCREC_LAUNCH(check_side_a, grid_for(n_places), dim3(256), 0, s, n_places, (const int64_t *)nullptr, (int64_t)0, plat.p,
                  plon.p, pr.p, regions.p, nr, has_place.p, err.p);
    LOCREC_LAUNCH(check_side_b, grid_for(n_confirmed), dim3(256), 0, s, n_confirmed, clat.p, clon.p, cr.p, regions.p, nr,
                  has_place.p, err.p);
    LocationError le;
    LOCREC_READ_BACK(le, err.p, s);
    LOCREC_TRY(location_error(le, plat.p, plon.p, "place", n_places, clat.p, clon.p, "confirmed place", inout_count));

    DevBuf<uint64_t> k0, k1;
    DevBuf<uint32_t> r0, r1;
    LOCREC_TRY(k0.alloc((size_t)n_confirmed));
    LOCREC_TRY(k1.alloc((size_t)n_confirmed));
    LOCREC_TRY(r0.alloc((size_t)n_confirmed));
    LOCREC_TRY(r1.alloc((size_t)n_confirmed));
    if (out_not_same_counts) {  // the confirmed rows by (region rank, id): two stable passes
        DevBuf<uint32_t> rk0, rk1;
        LOCREC_TRY(rk0.alloc((size_t)n_confirmed));
        LOCREC_TRY(rk1.alloc((size_t)n_confirmed));
        LOCREC_LAUNCH(iota_keys, grid_for(n_confirmed), dim3(256), 0, s, n_confirmed, ci.p, k0.p, r0.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r0.p, r1.p, (int)n_confirmed, 0, 64, s));
        LOCREC_LAUNCH(dd_region_rank_keys, grid_for(n_confirmed), dim3(256), 0, s, n_confirmed, cr.p, r1.p, regions.p, nr,
                      rk0.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, rk0.p, rk1.p, r1.p, r0.p, (int)n_confirmed, 0, 24, s));
        LOCREC_LAUNCH(gather_id_keys, grid_for(n_confirmed), dim3(256), 0, s, n_confirmed, ci.p, r0.p, k0.p);
        LOCREC_LAUNCH(dd_partners, grid_for(n_places), dim3(256), 0, s, n_places, pi.p, pr.p, regions.p, nr, n_confirmed,
                      rk1.p, k0.p, ons.p);
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (rk0 / rk1 are released here)
    }

    const int32_t k = clamp_threshold(max_name_difference);
    int64_t total_same = 0;
    if (max_meters >= 0.0 && k >= 0) {
        const Grid g = make_grid(max_meters);
        LOCREC_LAUNCH(pr_place_keys, grid_for(n_confirmed), dim3(256), 0, s, n_confirmed, clat.p, clon.p, cr.p, regions.p, nr,
                      g, k0.p, r0.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r0.p, r1.p, (int)n_confirmed, 0, 64, s));

        DevBuf<unsigned long long> counts, offsets;
        LOCREC_TRY(counts.alloc((size_t)n_places));
        LOCREC_TRY(offsets.alloc((size_t)n_places));
        LOCREC_LAUNCH((dd_walk<false>), grid_for(n_places), dim3(256), 0, s, (int64_t)0, n_places, pi.p, plat.p, plon.p, pr.p,
                      regions.p, nr, g, max_meters, n_confirmed, k1.p, r1.p, ci.p, clat.p, clon.p, counts.p, nullptr, 0ull,
                      nullptr, nullptr);
        LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, counts.p, offsets.p, (int)n_places, s));
        unsigned long long last_off = 0, last_cnt = 0;
        LOCREC_HIP_TRY(hipMemcpyAsync(&last_off, offsets.p + (n_places - 1), 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(&last_cnt, counts.p + (n_places - 1), 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        const unsigned long long total_cand = last_off + last_cnt;
        g_dedup_stats.candidates = (int64_t)total_cand;

        Out<int64_t> op, oc;
        Out<int32_t> od;
        LOCREC_TRY(op.bind(out_place_rows, cap, mem));
        LOCREC_TRY(oc.bind(out_confirmed_rows, cap, mem));
        LOCREC_TRY(od.bind(out_name_differences, cap, mem));

        const bool full_dp = full_dp_forced();
        const unsigned long long budget = (unsigned long long)pair_budget();
        DevBuf<uint32_t> cand_place, cand_conf, flags, pos;
        DevBuf<int32_t> dist;
        DevBuf<ChunkEnd> chunk_dev;
        LOCREC_TRY(chunk_dev.alloc(1));
        for (int64_t begin = 0; total_cand > 0 && begin < n_places;) {
            LOCREC_TRY(clock.mark(kPhaseGrid));
            LOCREC_LAUNCH(dd_chunk_end, dim3(1), dim3(64), 0, s, n_places, offsets.p, total_cand, begin, budget, chunk_dev.p);
            ChunkEnd ce;
            unsigned long long base = 0;
            LOCREC_HIP_TRY(hipMemcpyAsync(&ce, chunk_dev.p, sizeof ce, hipMemcpyDeviceToHost, s));
            LOCREC_HIP_TRY(hipMemcpyAsync(&base, offsets.p + begin, 8, hipMemcpyDeviceToHost, s));
            LOCREC_HIP_TRY(hipStreamSynchronize(s));
            const int64_t end = ce.end, m = (int64_t)ce.pairs;
            if (m >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "one place has 2^31 or more candidates");
            ++g_dedup_stats.chunks;
            if (m > 0) {
                LOCREC_TRY(cand_place.reserve((size_t)m));
                LOCREC_TRY(cand_conf.reserve((size_t)m));
                LOCREC_TRY(flags.reserve((size_t)m));
                LOCREC_TRY(pos.reserve((size_t)m));
                LOCREC_TRY(dist.reserve((size_t)m));
                LOCREC_LAUNCH((dd_walk<true>), grid_for(end - begin), dim3(256), 0, s, begin, end, pi.p, plat.p, plon.p, pr.p,
                              regions.p, nr, g, max_meters, n_confirmed, k1.p, r1.p, ci.p, clat.p, clon.p, nullptr, offsets.p,
                              base, cand_place.p, cand_conf.p);
                LOCREC_TRY(clock.mark(kPhaseLev));
                LOCREC_TRY(lev_pairs(m, cand_place.p, cand_conf.p, PN.off.p, PN.units.p, CN.off.p, CN.units.p, k, full_dp, dist.p, s));
                LOCREC_TRY(clock.mark(kPhaseCompact));
                LOCREC_LAUNCH(dd_same_flags, grid_for(m), dim3(256), 0, s, m, dist.p, k, flags.p);
                LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, flags.p, pos.p, (int)m, s));
                LOCREC_LAUNCH(dd_emit_same, grid_for(m), dim3(256), 0, s, m, flags.p, pos.p, cand_place.p, cand_conf.p, dist.p,
                              total_same, cap, op.p, oc.p, od.p);
                if (out_not_same_counts)
                    LOCREC_LAUNCH(dd_subtract_same, grid_for(end - begin), dim3(256), 0, s, begin, end, offsets.p, counts.p, base,
                                  flags.p, ons.p);
                uint32_t last_pos = 0, last_flag = 0;
                LOCREC_HIP_TRY(hipMemcpyAsync(&last_pos, pos.p + (m - 1), 4, hipMemcpyDeviceToHost, s));
                LOCREC_HIP_TRY(hipMemcpyAsync(&last_flag, flags.p + (m - 1), 4, hipMemcpyDeviceToHost, s));
                LOCREC_HIP_TRY(hipStreamSynchronize(s));
                total_same += (int64_t)last_pos + last_flag;
            }
            begin = end;
        }
        LOCREC_TRY(clock.mark(kPhaseEnd));
        const int64_t rows = std::min(total_same, cap);
        LOCREC_TRY(op.deliver(rows, s));
        LOCREC_TRY(oc.deliver(rows, s));
        LOCREC_TRY(od.deliver(rows, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
    } else {
        LOCREC_TRY(clock.mark(kPhaseEnd));
    }
    if (out_not_same_counts) LOCREC_TRY(ons.deliver(n_places, s));
    LOCREC_TRY(clock.read(g_dedup_stats.ms));
    g_dedup_stats.same = total_same;
    *inout_count = total_same;
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_find_duplicate_places_stats(int64_t *out_candidates, int64_t *out_same, int64_t *out_chunks,
                                                      double *out_grid_ms, double *out_lev_ms, double *out_compact_ms)
{
    const DedupStats &st = g_dedup_stats;
    if (out_candidates) *out_candidates = st.candidates;
    if (out_same) *out_same = st.same;
    if (out_chunks) *out_chunks = st.chunks;
    if (out_grid_ms) *out_grid_ms = st.ms[kPhaseGrid];
    if (out_lev_ms) *out_lev_ms = st.ms[kPhaseLev];
    if (out_compact_ms) *out_compact_ms = st.ms[kPhaseCompact];
    return LOCREC_OK;
}
