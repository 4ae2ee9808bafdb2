// region_sets.hip -- from one place-visit table to the rows of every region set, on the device: what the reference's
// two builder mains do around their per-set work (between f-4 and f-2):
//
//   PlaceVisits.calcVisitsFromTimestamp   PlaceVisits.scala:50-61    max(timestamp)          locrec_visits_max_timestamp
//   PlaceVisits.extractRegionIds          PlaceVisits.scala:69-78    distinct region ids     locrec_extract_region_ids
//   PlaceVisits.extractRegionsPlaceVisits PlaceVisits.scala:63-67,80-87
//        placeVisits.where(region_id === a or region_id === b) for every region and every pair of regions:
//                                                                    locrec_region_partition, once per table, and
//                                                                    locrec_region_set_gather, once per set
//
// The partition groups the row numbers by region (rank by binary search, one stable radix sort over the few bits a
// rank has), rows ascending inside a group; a set's rows are then one group, or the stable merge of two, so the
// gathered columns are exactly the where() in input order and a set costs its own rows, not a pass over the table.
// Arrays are host or device memory (`mem`) as for the other producers (prep_cols.h).  No atomics: the only words
// several threads write are validity flags that every writer sets to the same value.

#include "dev_prims.h"

#include <algorithm>
#include <limits>

#include "common.h"
#include "prep_cols.h"

namespace {

using namespace locrec;

constexpr int kRsThreads = 256;
constexpr int kRsTile = 2048;                    // output rows of one block of rs_merge_gather
constexpr int kRsMaxCols = 8;
constexpr int64_t kRsMaxRegions = (int64_t)1 << 24;  // as locrec_calc_place_visits: at most 2^24 - 1 regions

// ---- the partition ----------------------------------------------------------------------------------------------

__global__ void rs_check_ascending(int64_t n, const int64_t *ids, uint32_t *invalid)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 < n && !(ids[i] < ids[i + 1])) *invalid = 1u;
}

// rank of every row's region in the ascending region list; n_regions for a region that is not listed
__global__ void rs_rank_rows(int64_t n, const int64_t *row_regions, int64_t n_regions, const int64_t *regions, uint32_t *rank,
                             uint32_t *rows)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t v = row_regions[i];
    const int64_t lo = lower_bound<int64_t>(regions, 0, n_regions, v);
    rank[i] = (uint32_t)(lo < n_regions && regions[lo] == v ? lo : n_regions);
    rows[i] = (uint32_t)i;
}

// offsets[g] = first sorted position whose rank is >= g, for g in [0, n_regions + 1]; offsets[n_regions + 1] = n
__global__ void rs_group_offsets(int64_t n, const uint32_t *sorted_rank, int64_t n_groups, int64_t *offsets)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n_groups) return;
    if (g == n_groups) {
        offsets[g] = n;
        return;
    }
    offsets[g] = lower_bound<uint32_t>(sorted_rank, 0, n, (uint32_t)g);  // (g < n_groups <= 2^24)
}

// ---- one set's rows: check, then merge and gather ---------------------------------------------------------------

// The entries of the two runs themselves - nothing is read THROUGH them here: each run strictly ascending, every
// entry a row of the table.  (That the two ranges of `rows` do not overlap is a comparison of four host scalars.)
__global__ void rs_check_runs(const int32_t *a, int64_t la, const int32_t *b, int64_t lb, int64_t n_rows, uint32_t *invalid)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= la + lb) return;
    const int32_t *run = i < la ? a : b;
    const int64_t k = i < la ? i : i - la;
    const int32_t v = run[k];
    const bool ok = v >= 0 && (int64_t)v < n_rows && (k == 0 || run[k - 1] < v);
    if (!ok) *invalid = 1u;
}

struct RsCols {
    const int64_t *in[kRsMaxCols];
    int64_t *out[kRsMaxCols];
};

// how many entries of run a stand among the first d rows of the stable merge (a before b where they are equal)
__device__ __forceinline__ int64_t rs_diagonal(const int32_t *a, int64_t la, const int32_t *b, int64_t lb, int64_t d)
{
    int64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;  // lo <= mid < la, 0 <= d - 1 - mid < lb
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The stable merge of two ascending runs of row numbers, every column gathered through it.  The OUTPUT rows are what
// is split evenly (the shape of pr_covisit_emit): a block owns kRsTile consecutive output rows, two lanes find the
// tile's two diagonal splits, the tile's slices of both runs are merged in LDS - an entry's place is its own position
// plus the entries of the other slice that go before it - and after the barrier every column is read through the
// merged row numbers and written with coalesced 8-byte stores.  A failed check (rs_check_runs) leaves at once.
__global__ __launch_bounds__(kRsThreads) void rs_merge_gather(const uint32_t *invalid, const int32_t *a, int64_t la,
                                                              const int32_t *b, int64_t lb, int n_cols, RsCols c)
{
    __shared__ int64_t split[2];
    __shared__ int32_t slice[kRsTile];
    __shared__ int32_t merged[kRsTile];
    if (*invalid) return;
    const int64_t total = la + lb;
    const int64_t t0 = (int64_t)blockIdx.x * kRsTile;
    const int64_t t1 = min(t0 + (int64_t)kRsTile, total);
    if (t0 >= t1) return;
    if (threadIdx.x < 2) split[threadIdx.x] = rs_diagonal(a, la, b, lb, threadIdx.x == 0 ? t0 : t1);
    __syncthreads();
    const int64_t i0 = split[0], j0 = t0 - i0;
    const int na = (int)(split[1] - i0), len = (int)(t1 - t0);
    for (int q = threadIdx.x; q < len; q += kRsThreads) slice[q] = q < na ? a[i0 + q] : b[j0 + (q - na)];
    __syncthreads();
    for (int q = threadIdx.x; q < len; q += kRsThreads) {
        const int32_t v = slice[q];
        const bool from_a = q < na;
        int lo = from_a ? na : 0, hi = from_a ? len : na;  // the other slice
        const int first = lo;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const bool before = from_a ? slice[mid] < v : slice[mid] <= v;
            if (before) lo = mid + 1; else hi = mid;
        }
        merged[(from_a ? q : q - na) + (lo - first)] = v;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < len; q += kRsThreads) {
        const int64_t r = merged[q];
        int64_t v[kRsMaxCols];
#pragma unroll
        for (int k = 0; k < kRsMaxCols; ++k)
            if (k < n_cols) v[k] = c.in[k][r];
#pragma unroll
        for (int k = 0; k < kRsMaxCols; ++k)
            if (k < n_cols) c.out[k][t0 + q] = v[k];
    }
}

int32_t rows_ok(int64_t n, const char *what)
{
    if (n < 0 || n >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "%s %lld out of range [0, 2^31)", what, (long long)n);
    return LOCREC_OK;
}

}  // namespace

extern "C" int32_t locrec_visits_max_timestamp(int64_t n, const int64_t *timestamps, int32_t mem, int64_t *out_max)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!out_max) return fail(LOCREC_E_INVALID_ARG, "out_max is required");
    LOCREC_TRY(rows_ok(n, "visit count"));
    if (n == 0) return fail(LOCREC_E_INVALID_ARG, "the maximum timestamp of no visits is undefined");
    if (!timestamps) return fail(LOCREC_E_INVALID_ARG, "null array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Temp tmp;
    In<int64_t> ts;
    DevBuf<int64_t> out;
    LOCREC_TRY(ts.bind(timestamps, n, mem, s));
    LOCREC_TRY(out.alloc(1));
    LOCREC_PRIM(tmp, prim::reduce(p_, bytes_, ts.p, out.p, (size_t)n, rocprim::maximum<int64_t>(),
                                  std::numeric_limits<int64_t>::min(), s));
    LOCREC_READ_BACK(*out_max, out.p, s);
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_extract_region_ids(int64_t n, const int64_t *region_ids, int32_t mem, int64_t *out_ids,
                                             int64_t *inout_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!inout_count) return fail(LOCREC_E_INVALID_ARG, "inout_count is required");
    const int64_t cap = out_ids ? *inout_count : 0;
    *inout_count = 0;
    if (cap < 0) return fail(LOCREC_E_INVALID_ARG, "negative capacity");
    LOCREC_TRY(rows_ok(n, "row count"));
    if (n == 0) return LOCREC_OK;
    if (!region_ids) return fail(LOCREC_E_INVALID_ARG, "null array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Temp tmp;
    In<int64_t> r;
    DevBuf<int64_t> ids;
    int32_t nr = 0;
    LOCREC_TRY(r.bind(region_ids, n, mem, s));
    LOCREC_TRY(distinct_ids(r.p, n, tmp, s, ids, &nr));
    *inout_count = nr;
    const int64_t m = std::min<int64_t>(nr, cap);
    if (m == 0) return LOCREC_OK;
    const hipMemcpyKind to_caller = mem == LOCREC_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    LOCREC_HIP_TRY(hipMemcpyAsync(out_ids, ids.p, (size_t)m * sizeof(int64_t), to_caller, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_region_partition(int64_t n_rows, const int64_t *row_region_ids, int64_t n_regions,
                                           const int64_t *region_ids, int32_t mem, int32_t *out_rows, int64_t *out_offsets)
try {
    LOCREC_TRY(mem_ok(mem));
    LOCREC_TRY(rows_ok(n_rows, "row count"));
    if (n_regions < 0 || n_regions >= kRsMaxRegions)
        return fail(LOCREC_E_INVALID_ARG, "%lld regions: at most 2^24 - 1 are supported", (long long)n_regions);
    if (!out_offsets) return fail(LOCREC_E_INVALID_ARG, "out_offsets is required");
    if ((n_rows > 0 && (!row_region_ids || !out_rows)) || (n_regions > 0 && !region_ids))
        return fail(LOCREC_E_INVALID_ARG, "null array");
    if (n_rows == 0 && n_regions <= 1) {  // nothing to sort and no order to check
        for (int64_t g = 0; g < n_regions + 2; ++g) out_offsets[g] = 0;
        return LOCREC_OK;
    }
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Temp tmp;
    In<int64_t> rr, regs;
    DevBuf<uint32_t> invalid;
    LOCREC_TRY(rr.bind(row_region_ids, n_rows, mem, s));
    LOCREC_TRY(regs.bind(region_ids, n_regions, mem, s));
    LOCREC_TRY(invalid.alloc(1));
    LOCREC_HIP_TRY(hipMemsetAsync(invalid.p, 0, sizeof(uint32_t), s));
    LOCREC_LAUNCH(rs_check_ascending, grid_for(n_regions), dim3(256), 0, s, n_regions, regs.p, invalid.p);
    uint32_t bad = 0;
    LOCREC_READ_BACK(bad, invalid.p, s);
    if (bad) return fail(LOCREC_E_INVALID_ARG, "region_ids must be strictly ascending");
    if (n_rows == 0) {
        for (int64_t g = 0; g < n_regions + 2; ++g) out_offsets[g] = 0;
        return LOCREC_OK;
    }

    DevBuf<uint32_t> rank0, rank1, rows0;
    DevBuf<int64_t> offsets;
    Out<int32_t> rows;
    LOCREC_TRY(rank0.alloc((size_t)n_rows));
    LOCREC_TRY(rows0.alloc((size_t)n_rows));
    LOCREC_TRY(offsets.alloc((size_t)n_regions + 2));
    LOCREC_TRY(rows.bind(out_rows, n_rows, mem));
    LOCREC_LAUNCH(rs_rank_rows, grid_for(n_rows), dim3(256), 0, s, n_rows, rr.p, n_regions, regs.p, rank0.p, rows0.p);
    unsigned bits = 0;  // ceil(log2(n_regions + 1)): the ranks are 0 .. n_regions
    while (((int64_t)1 << bits) <= n_regions) ++bits;
    const uint32_t *sorted_rank = rank0.p;
    if (bits == 0) {  // no region is listed: one group, the rows as they are
        LOCREC_HIP_TRY(hipMemcpyAsync(rows.p, rows0.p, (size_t)n_rows * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    } else {
        LOCREC_TRY(rank1.alloc((size_t)n_rows));
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, rank0.p, rank1.p, rows0.p, reinterpret_cast<uint32_t *>(rows.p),
                                          (size_t)n_rows, 0, bits, s));
        sorted_rank = rank1.p;
    }
    LOCREC_LAUNCH(rs_group_offsets, grid_for(n_regions + 2), dim3(256), 0, s, n_rows, sorted_rank, n_regions + 1, offsets.p);
    LOCREC_HIP_TRY(hipMemcpyAsync(out_offsets, offsets.p, (size_t)(n_regions + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    LOCREC_TRY(rows.deliver(n_rows, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_region_set_gather(int64_t n_rows, int32_t n_cols, const int64_t *const *cols, const int32_t *rows,
                                            int64_t a_begin, int64_t a_end, int64_t b_begin, int64_t b_end, int32_t mem,
                                            int64_t *const *out_cols)
try {
    LOCREC_TRY(mem_ok(mem));
    LOCREC_TRY(rows_ok(n_rows, "row count"));
    if (n_cols < 1 || n_cols > kRsMaxCols) return fail(LOCREC_E_INVALID_ARG, "%d columns: 1 to %d are supported", n_cols, kRsMaxCols);
    if (!cols || !out_cols) return fail(LOCREC_E_INVALID_ARG, "null column list");
    if (a_begin < 0 || a_begin > a_end || a_end > n_rows || b_begin < 0 || b_begin > b_end || b_end > n_rows)
        return fail(LOCREC_E_INVALID_ARG, "a range of rows must lie inside [0, n_rows]");
    const int64_t la = a_end - a_begin, lb = b_end - b_begin, total = la + lb;
    if (la > 0 && lb > 0 && a_begin < b_end && b_begin < a_end)
        return fail(LOCREC_E_INVALID_ARG, "the two ranges of rows overlap");
    if (total == 0) return LOCREC_OK;
    if (!rows) return fail(LOCREC_E_INVALID_ARG, "null array");
    for (int32_t k = 0; k < n_cols; ++k)
        if (!cols[k] || !out_cols[k]) return fail(LOCREC_E_INVALID_ARG, "null column");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    In<int32_t> ra, rb;
    In<int64_t> in[kRsMaxCols];
    Out<int64_t> out[kRsMaxCols];
    DevBuf<uint32_t> invalid;
    LOCREC_TRY(ra.bind(rows + a_begin, la, mem, s));
    LOCREC_TRY(rb.bind(rows + b_begin, lb, mem, s));
    LOCREC_TRY(invalid.alloc(1));
    LOCREC_HIP_TRY(hipMemsetAsync(invalid.p, 0, sizeof(uint32_t), s));
    LOCREC_LAUNCH(rs_check_runs, grid_for(total), dim3(256), 0, s, ra.p, la, rb.p, lb, n_rows, invalid.p);
    RsCols c = {};
    if (mem == LOCREC_MEM_HOST) {  // the staged columns are uploaded only for rows that passed the check
        uint32_t bad = 0;
        LOCREC_READ_BACK(bad, invalid.p, s);
        if (bad) return fail(LOCREC_E_INVALID_ARG, "rows: a run is not strictly ascending or names a row outside [0, n_rows)");
    }
    for (int32_t k = 0; k < n_cols; ++k) {
        LOCREC_TRY(in[k].bind(cols[k], n_rows, mem, s));
        LOCREC_TRY(out[k].bind(out_cols[k], total, mem));
        c.in[k] = in[k].p;
        c.out[k] = out[k].p;
    }
    // device memory: the kernel itself reads the flag first, so the call waits for its stream once, at the end
    LOCREC_LAUNCH(rs_merge_gather, dim3((unsigned)((total + kRsTile - 1) / kRsTile)), dim3(kRsThreads), 0, s, invalid.p, ra.p,
                  la, rb.p, lb, (int)n_cols, c);
    uint32_t bad = 0;
    LOCREC_HIP_TRY(hipMemcpyAsync(&bad, invalid.p, sizeof bad, hipMemcpyDeviceToHost, s));
    for (int32_t k = 0; k < n_cols; ++k) LOCREC_TRY(out[k].deliver(total, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    if (bad) return fail(LOCREC_E_INVALID_ARG, "rows: a run is not strictly ascending or names a row outside [0, n_rows)");
    return LOCREC_OK;
}
LOCREC_CATCH_ALL
