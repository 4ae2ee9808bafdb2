// knn_large.hip -- K beyond what the per-query LDS lists hold (LOCREC_KNN_BATCH_MAX_K), and
// aggregation over more rating rows than one block sorts in LDS.
//
// The reference ships --k-nearest 2000000 (bin/knn_recommender.sh:35), i.e. "every person with a
// positive similarity is a neighbour" (KnnRecommender.scala:47-48 with K >= the candidate count).
//   knn_large_topk       S (knn_scan1) -> keys in person-id-rank order -> one STABLE descending device
//                        radix sort (rocPRIM, dev_prims.h; ties keep id-ascending order) -> first K
//   knn_large_recommend  the same selection, then makeRecommendations0 (:51-70) as a place-major
//                        pass over the transposed ratings: est[p] = sum r*s / sum s over the selected
//                        raters of p, each place summed by one wave in a fixed order.
// A library sort is used here on purpose: this is the rare large-K corner, not the hot path.
// The place-major pass is ONE set of kernels (lk_aggregate_segments, lk_sum_segments, lk_finish_count, lk_finish_emit)
// templated on the number of query columns of the weights S[row][QT]: QT = 1 is the single request (and the
// host-given weights of knn_large_aggregate), QT = kLkbQt a tile of a batch (below: "Batched large K", "Batched top-K
// at any K") - so a batch's estimates are the single request's bit for bit by construction.

#include "dev_prims.h"

#include <algorithm>

#include "knn_index.h"
#include "knn_pool_plan.h"

namespace {

using namespace locrec;

constexpr int kLkHistBins = 4096;  // kHistBins of knn.hip

// the sum of v over the wave (xor butterfly: every lane ends with the same bits)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d);
    return v;
}

// exclusive prefix of c over the 256 threads of a block: within the wave, then over the four waves, whose totals
// it leaves in wtot[4] (LDS); holds a __syncthreads
__device__ __forceinline__ int block_scan_256(int c, int *wtot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int off = incl - c;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    return off;
}

// keys[r] = bit pattern of the similarity of the person with id-rank r (all similarities are >= +0,
// so the unsigned order of the bits is the numeric order); vals[r] = r
// rows outside [row0, row1) are not candidates of this request (a candidate shard, locrec_knn_query_shard): S holds
// whatever an earlier request left there
__global__ void lk_gather_keys(const double *S, const int32_t *row_of_rid, int32_t n, int32_t row0, int32_t row1, uint64_t *keys,
                               uint32_t *vals)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int32_t row = row_of_rid[r];
    keys[r] = row >= row0 && row < row1 ? (uint64_t)__double_as_longlong(S[row]) : 0ull;
    vals[r] = (uint32_t)r;
}

// pad_to > m: entries [m, pad_to) of a batch slot are reset to "no neighbour" (-1, 0.0, -1) like every other path leaves
// them - the slot may hold a stand-in query's list
__global__ void lk_emit(const uint64_t *keys, const uint32_t *vals, int32_t m, const int64_t *ids_by_rank,
                        int64_t *out_ids, double *out_sims, const int32_t *row_of_rid = nullptr, int32_t *out_rows = nullptr,
                        int64_t *out_cnt = nullptr, int32_t pad_to = 0)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && out_cnt) *out_cnt = m;
    if (i >= m) {
        if (i < pad_to) {
            out_ids[i] = -1;
            out_sims[i] = 0.0;
            if (out_rows) out_rows[i] = -1;
        }
        return;
    }
    out_ids[i] = ids_by_rank[vals[i]];
    out_sims[i] = __longlong_as_double((long long)keys[i]);
    if (out_rows) out_rows[i] = row_of_rid[vals[i]];
}

// w[row] = similarity if the row is among the first m sorted entries, else 0
__global__ void lk_scatter_weights(const uint64_t *keys, const uint32_t *vals, int32_t m, const int32_t *row_of_rid,
                                   double *w)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    w[row_of_rid[vals[i]]] = __longlong_as_double((long long)keys[i]);
}

// Place-major aggregation in two steps.  A popular place has hundreds of thousands of raters (874 k at
// cfg2): one wave walking all of them was the whole cost of a large-K request (~10 ms).  The raters
// of a place are therefore cut into SEGMENTS of at most kSegRaters entries (a table built once per
// index): one wave per segment (lanes stride it, butterfly), then one thread per (place, query) adds its
// segments' sums in segment order - a fixed order, so the result is reproducible.
constexpr int kSegRaters = 4096;

// S[row][QT]: column t = the weights of query t (0 = not a neighbour).  Lane l takes raters l, l + 64, ... of the
// segment in ascending order, U of them in flight: the row loads, then the U dependent gathers of S (one after the
// other this loop was a chain of 64 memory round trips per segment); added in the same order as a plain loop.  With
// QT = 16 a rater's weights are one 128-byte line that serves sixteen queries, and two raters in flight fill the
// registers (150 VGPRs); the single column has room for eight.
// (the bodies of this pass are __device__ functions: the kernels below launch them for one index, knn_pool.h for the
// members of a pool side by side - the same operations in the same order, so the same bits)
template <int QT, int U>
__device__ __forceinline__ void lk_aggregate_segments_body(const int64_t *seg_begin, const int64_t *seg_end, int32_t nsegs,
                                                           const int32_t *cp_row, const double *cp_rating, const double *S,
                                                           double *seg_ws, double *seg_ss, int bx)
{
    const int lane = threadIdx.x & 63;
    const int sg = bx * 4 + (threadIdx.x >> 6);
    if (sg >= nsegs) return;
    double ws[QT], ss[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) ws[t] = ss[t] = 0.0;
    const int64_t end = seg_end[sg];
    for (int64_t e0 = seg_begin[sg] + lane; e0 < end; e0 += 64 * U) {
        int32_t rr[U];
        double rt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t e = e0 + 64 * u;
            rr[u] = e < end ? cp_row[e] : -1;
            rt[u] = e < end ? cp_rating[e] : 0.0;
        }
        double sv[U][QT];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < QT; ++t) sv[u][t] = rr[u] >= 0 ? S[(int64_t)rr[u] * QT + t] : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < QT; ++t)
                if (sv[u][t] > 0) {
                    const double wr = rt[u] * sv[u][t];  // col("rating") * col("similarity") (:59)
                    ws[t] = ws[t] + wr;
                    ss[t] = ss[t] + sv[u][t];
                }
    }
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        ws[t] = wave_sum(ws[t]);
        ss[t] = wave_sum(ss[t]);
    }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            seg_ws[(int64_t)sg * QT + t] = ws[t];
            seg_ss[(int64_t)sg * QT + t] = ss[t];
        }
    }
}

template <int QT, int U>
__global__ __launch_bounds__(256) void lk_aggregate_segments(const int64_t *seg_begin, const int64_t *seg_end, int32_t nsegs,
                                                             const int32_t *cp_row, const double *cp_rating, const double *S,
                                                             double *seg_ws, double *seg_ss)
{
    lk_aggregate_segments_body<QT, U>(seg_begin, seg_end, nsegs, cp_row, cp_rating, S, seg_ws, seg_ss, (int)blockIdx.x);
}

// thread per (place, query): the place's segments in segment order; output query-major [query][place]
template <int QT>
__device__ __forceinline__ void lk_sum_segments_body(const int32_t *place_seg0, int32_t nplaces, const double *seg_ws,
                                                     const double *seg_ss, double *out_ws, double *out_ss, uint32_t bx)
{
    const int64_t i = (int64_t)bx * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nplaces * QT) return;
    const int p = (int)(i / QT), t = (int)(i % QT);
    double ws = 0.0, ss = 0.0;
    for (int sg = place_seg0[p]; sg < place_seg0[p + 1]; ++sg) {
        ws = ws + seg_ws[(int64_t)sg * QT + t];
        ss = ss + seg_ss[(int64_t)sg * QT + t];
    }
    out_ws[(int64_t)t * nplaces + p] = ws;
    out_ss[(int64_t)t * nplaces + p] = ss;
}

template <int QT>
__global__ void lk_sum_segments(const int32_t *place_seg0, int32_t nplaces, const double *seg_ws, const double *seg_ss,
                                double *out_ws, double *out_ss)
{
    lk_sum_segments_body<QT>(place_seg0, nplaces, seg_ws, seg_ss, out_ws, out_ss, blockIdx.x);
}

// The end of the place-major pass on the device: the places somebody among the neighbours rated (ss > 0), in
// ascending place order, with est = ws / ss (:67).  This was a host loop over all places after copying ws and ss
// back - 100 k iterations with a division each, 0.2 ms of a 0.5 ms request at cfg2.  Two small launches on a grid
// (tiles, queries): the rated places of every tile of kFinishTile are counted, then every tile writes its rows behind
// the tiles before it (the prefix over at most a few hundred tile counts is recomputed by each block).
constexpr int kFinishTile = 2048;  // places per block: 256 threads x 8 consecutive places

// tile bx of ntiles, query column q
__device__ __forceinline__ void lk_finish_count_body(const double *ss, int32_t nplaces, int32_t *tile_cnt, int bx, int q, int ntiles)
{
    __shared__ int wsum[4];
    const double *sq = ss + (int64_t)q * nplaces;
    const int p0 = bx * kFinishTile + threadIdx.x * 8;
    int c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) c += (p0 + i < nplaces && sq[p0 + i] > 0) ? 1 : 0;
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[q * ntiles + bx] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void lk_finish_count(const double *ss, int32_t nplaces, int32_t *tile_cnt)
{
    lk_finish_count_body(ss, nplaces, tile_cnt, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x);
}

// where query t's rows begin in the output; < 0: the slot holds no query, nothing is written for it
template <int QT>
struct LkBases {
    int64_t base[QT];
};

// out_n (with host_n, a pinned word the host reads without a copy): the single request's row count, or null
template <int QT>
__device__ __forceinline__ void lk_finish_emit_body(const double *ws, const double *ss, int32_t nplaces, const int32_t *tile_cnt,
                                                    const int64_t *cplace_ids, const LkBases<QT> &bases, int64_t *out_place,
                                                    double *out_est, int64_t *out_n, int64_t *host_n, int bx, int q, int ntiles)
{
    __shared__ int64_t bsum[4];
    __shared__ int wtot[4];
    const int t = threadIdx.x;
    if (bases.base[q] < 0) return;
    const double *wq = ws + (int64_t)q * nplaces, *sq = ss + (int64_t)q * nplaces;
    const int32_t *tc = tile_cnt + q * ntiles;
    // rows of the tiles before this one
    int64_t before = 0;
    for (int i = t; i < bx; i += 256) before += tc[i];
    before = wave_sum(before);
    if ((t & 63) == 0) bsum[t >> 6] = before;
    const int p0 = bx * kFinishTile + t * 8;
    bool keep[8];
    int c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        keep[i] = p0 + i < nplaces && sq[p0 + i] > 0;
        c += keep[i] ? 1 : 0;
    }
    int64_t o = block_scan_256(c, wtot);
    o += bases.base[q] + bsum[0] + bsum[1] + bsum[2] + bsum[3];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (keep[i]) {
            out_place[o] = cplace_ids[p0 + i];
            out_est[o] = wq[p0 + i] / sq[p0 + i];  // :67
            ++o;
        }
    }
    if (out_n && bx == ntiles - 1 && t == 255) {  // the last thread of the last tile knows the total
        *out_n = o;
        if (host_n) *host_n = o;
    }
}

template <int QT>
__global__ __launch_bounds__(256) void lk_finish_emit(const double *ws, const double *ss, int32_t nplaces,
                                                      const int32_t *tile_cnt, const int64_t *cplace_ids,
                                                      const LkBases<QT> bases, int64_t *out_place, double *out_est,
                                                      int64_t *out_n, int64_t *host_n)
{
    lk_finish_emit_body<QT>(ws, ss, nplaces, tile_cnt, cplace_ids, bases, out_place, out_est, out_n, host_n, (int)blockIdx.x,
                            (int)blockIdx.y, (int)gridDim.x);
}

// segment table of the place-major ratings (lazy, once per index)
int32_t ensure_segments(locrec_knn_index *ix)
{
    if (ix->lk_nsegs >= 0) return LOCREC_OK;
    const int64_t np = (int64_t)ix->cplace_ids.size();
    std::vector<int64_t> cptr((size_t)np + 1, 0);
    if (np > 0) LOCREC_HIP_TRY(hipMemcpy(cptr.data(), ix->cp_ptr.p, ((size_t)np + 1) * 8, hipMemcpyDeviceToHost));
    std::vector<int64_t> sb, se;
    std::vector<int32_t> seg0((size_t)np + 1, 0);
    for (int64_t p = 0; p < np; ++p) {
        seg0[(size_t)p] = (int32_t)sb.size();
        for (int64_t b = cptr[(size_t)p]; b < cptr[(size_t)p + 1]; b += kSegRaters) {
            sb.push_back(b);
            se.push_back(std::min(b + kSegRaters, cptr[(size_t)p + 1]));
        }
    }
    seg0[(size_t)np] = (int32_t)sb.size();
    LOCREC_TRY(ix->lk_seg_begin.upload(sb, ix->stream));
    LOCREC_TRY(ix->lk_seg_end.upload(se, ix->stream));
    LOCREC_TRY(ix->lk_place_seg0.upload(seg0, ix->stream));
    LOCREC_TRY(ix->lk_seg_ws.alloc(sb.size()));
    LOCREC_TRY(ix->lk_seg_ss.alloc(sb.size()));
    LOCREC_HIP_TRY(hipStreamSynchronize(ix->stream));
    ix->lk_nsegs = (int32_t)sb.size();
    return LOCREC_OK;
}

// Enqueues aggregate -> sum -> count over the weights S[row][QT] (at least one place, the segment table built): the
// segments' sums [seg][QT], the places' sums [query][place] and the rated places of every finish tile [query][tiles]
template <int QT, int U>
int32_t enqueue_aggregation(locrec_knn_index *ix, const double *S, double *seg_ws, double *seg_ss, double *ws, double *ss,
                            int tiles, int32_t *tile_cnt)
{
    hipStream_t s = ix->stream;
    const int32_t np = (int32_t)ix->cplace_ids.size();
    if (ix->lk_nsegs > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(lk_aggregate_segments<QT, U>), dim3((unsigned)((ix->lk_nsegs + 3) / 4)), dim3(256), 0, s,
                           ix->lk_seg_begin.p, ix->lk_seg_end.p, ix->lk_nsegs, ix->cp_row.p, ix->cp_rating.p, S, seg_ws, seg_ss);
    hipLaunchKernelGGL(lk_sum_segments<QT>, dim3((unsigned)(((int64_t)np * QT + 255) / 256)), dim3(256), 0, s,
                       ix->lk_place_seg0.p, np, seg_ws, seg_ss, ws, ss);
    hipLaunchKernelGGL(lk_finish_count, dim3((unsigned)tiles, QT), dim3(256), 0, s, ss, np, tile_cnt);
    LOCREC_HIP_TRY(hipGetLastError());
    return LOCREC_OK;
}

// number of candidates (similarity > 0) of the scan that was just enqueued: the total of its histogram
int32_t candidate_count(locrec_knn_index *ix, int64_t *m)
{
    std::vector<uint32_t> hist(kLkHistBins);
    LOCREC_HIP_TRY(hipMemcpyAsync(hist.data(), ix->hist1.p, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    LOCREC_HIP_TRY(hipStreamSynchronize(ix->stream));
    int64_t total = 0;
    for (uint32_t h : hist) total += h;
    *m = total;
    return LOCREC_OK;
}

// Sorted (similarity desc, id asc) list of ALL rows in ix->lk_keys_out / lk_vals_out; *m = number of
// candidates (similarity > 0).
int32_t sort_all(locrec_knn_index *ix, int32_t qrow, double pw, double cw, int64_t *m, bool scanned = false)
{
    hipStream_t s = ix->stream;
    const int32_t n = (int32_t)ix->n;
    if (!scanned) LOCREC_TRY(knn_enqueue_dense(ix, qrow, pw, cw));
    LOCREC_TRY(ix->lk_keys.reserve((size_t)n));
    LOCREC_TRY(ix->lk_keys_out.reserve((size_t)n));
    LOCREC_TRY(ix->lk_vals.reserve((size_t)n));
    LOCREC_TRY(ix->lk_vals_out.reserve((size_t)n));
    hipLaunchKernelGGL(lk_gather_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ix->S1.p, ix->row_of_rid.p, n,
                       ix->cand_slice0 * 64, (int32_t)std::min<int64_t>(ix->n, (int64_t)ix->cand_slice1 * 64), ix->lk_keys.p,
                       ix->lk_vals.p);
    size_t temp_bytes = 0;
    LOCREC_HIP_TRY(prim::sort_pairs_desc(nullptr, temp_bytes, ix->lk_keys.p, ix->lk_keys_out.p,
                                                                ix->lk_vals.p, ix->lk_vals_out.p, n, 0, 64, s));
    LOCREC_TRY(ix->lk_temp.reserve(temp_bytes));
    LOCREC_HIP_TRY(prim::sort_pairs_desc(ix->lk_temp.p, temp_bytes, ix->lk_keys.p,
                                                                ix->lk_keys_out.p, ix->lk_vals.p, ix->lk_vals_out.p, n,
                                                                0, 64, s));
    // number of candidates = histogram total = position of the first zero key: binary search on the host
    // would need the keys; count on the device side instead via the histogram the scan already filled
    return candidate_count(ix, m);
}

// =====================================================================================================
// Batched large K.  bin/knn_recommender.sh:35 ships --k-nearest 2000000: with K >= N - 1
// findSimilarPersons (KnnRecommender.scala:47-48) selects EVERY person of positive similarity, so a batch needs no
// top-K at all: the similarities of a TILE of kLkbQt queries against all candidates are computed once
// (lkb_scan: S[row][query], one 128-byte line per candidate) and fed straight into the place-major aggregation
// (makeRecommendations0, :51-70) - the w[row] gather of lk_aggregate_segments, the cost of the single request,
// now serves sixteen queries per cache line.
//
// Dots: every candidate walks its plain CSR row against DENSE query tables qd[index][query] in global memory,
// sum += qd * value left to right in ascending index order - BLAS.dot's order, a product with an absent query
// entry adds +-0.0 - so similarities are the reference's bit for bit in EVERY stored format (the GENERIC fp64
// one included); the aggregation is the single request's kernels with kLkbQt columns, so a batch's estimates equal
// the single request's bit for bit.  (kLkbQt, the tile's queries: knn_pool_plan.h)

struct LkbScan {
    const int64_t *p_ptr, *c_ptr;
    const int32_t *p_idx, *c_idx;
    const double *p_val, *c_val;
    const double *norm_p, *norm_c;
    const double *qd_p, *qd_c;  // [dim][kLkbQt]
    int32_t qrow[kLkbQt];       // -1: no query in this slot
    int32_t nrows;
    double pw, cw;
    double *S;                  // [nrows][kLkbQt], or [kLkbQt][nrows] when transposed
    int32_t *cand;              // [kLkbQt] persons of positive similarity per query
    int32_t transposed;
    const uint32_t *bits;       // which place indices (mod the bitmap size) ANY query of the tile holds
    uint32_t bit_mask;          // bitmap size in bits - 1 (a power of two, <= kLkbBitmapBits)
};

// (the same arithmetic as knn.hip's exact_similarity: one multiply and one divide per family, "> 0", ps*pw + cs*cw)
__device__ __forceinline__ bool lkb_similarity(double dp, double dc, double cnp, double cnc, double qnp, double qnc, double pw,
                                               double cw, double &s)
{
    double ps = 0.0, cs = 0.0;
    bool have = false;
    if (cnp > 0.0) {
        const double den = cnp * qnp;
        const double t = dp / den;
        if (t > 0) { ps = t; have = true; }
    }
    if (cnc > 0.0) {
        const double den = cnc * qnc;
        const double t = dc / den;
        if (t > 0) { cs = t; have = true; }
    }
    const double a = ps * pw;
    const double b = cs * cw;
    s = a + b;
    return have;
}

struct LkbFill {
    const int64_t *ptr;
    const int32_t *idx;
    const double *val;
    double *qd;
    uint32_t *bits;     // presence bitmap of the place table (nullptr for the categories), bit = index & bit_mask
    uint32_t bit_mask;
    int32_t qrow[kLkbQt];
    int32_t set;
};

// element block bx of query t: the vector scattered into (set) or wiped from column t of the dense table
__device__ __forceinline__ void lkb_fill_body(const LkbFill &a, int set, int bx, int t)
{
    const int r = a.qrow[t];
    if (r < 0) return;
    const int64_t e = a.ptr[r] + (int64_t)bx * blockDim.x + threadIdx.x;
    if (e < a.ptr[r + 1]) {
        const int32_t i = a.idx[e];
        a.qd[(int64_t)i * kLkbQt + t] = set ? a.val[e] : 0.0;
        if (a.bits) {
            const uint32_t b = (uint32_t)i & a.bit_mask;
            if (set) atomicOr(&a.bits[b >> 5], 1u << (b & 31u));
            else a.bits[b >> 5] = 0u;  // (wiping: whole words, by whoever comes)
        }
    }
}

// grid (element blocks, kLkbQt)
__global__ void lkb_fill(const LkbFill a) { lkb_fill_body(a, a.set, (int)blockIdx.x, (int)blockIdx.y); }

// The tile's 16 queries hold a few hundred of the place dimensions between them, a candidate row is mostly OTHER places:
// the 128-byte line of the dense table (16 fp64 query values, nearly always all zero) was fetched from L2 for every
// candidate element - 3.2 GB per tile at cfg2, the whole cost of the kernel.  A bitmap of the indices any query of
// the tile holds (one bit per place, folded to at most 32 KB; lkb_fill sets it) sits in LDS: an element whose bit is
// clear adds value * (+0.0) to every dot - nothing, for finite values - and is skipped without touching the table.
constexpr uint32_t kLkbBitmapBits = 1u << 18;

// row block bx of the tile P (cand: the tile's candidate counters)
__device__ __forceinline__ void lkb_scan_body(const LkbScan &P, int32_t *cand, int bx)
{
    __shared__ int s_cand[kLkbQt];
    extern __shared__ uint32_t s_bits[];
    if (threadIdx.x < kLkbQt) s_cand[threadIdx.x] = 0;
    for (uint32_t i = threadIdx.x; i < (P.bit_mask + 1u) / 32u; i += blockDim.x) s_bits[i] = P.bits[i];
    __syncthreads();
    const int row = bx * blockDim.x + threadIdx.x;
    if (row < P.nrows) {
        double dp[kLkbQt], dc[kLkbQt];
#pragma unroll
        for (int t = 0; t < kLkbQt; ++t) dp[t] = dc[t] = 0.0;
        for (int64_t e = P.p_ptr[row]; e < P.p_ptr[row + 1]; ++e) {
            const int32_t i = P.p_idx[e];
            const uint32_t b = (uint32_t)i & P.bit_mask;
            if (!((s_bits[b >> 5] >> (b & 31u)) & 1u)) continue;  // no query of the tile holds this place
            const double v = P.p_val[e];
            const double *q = P.qd_p + (int64_t)i * kLkbQt;
#pragma unroll
            for (int t = 0; t < kLkbQt; ++t) {
                const double x = q[t] * v;  // x(kx) * y(ky), x = the query (Distance.scala:8)
                dp[t] = dp[t] + x;
            }
        }
        for (int64_t e = P.c_ptr[row]; e < P.c_ptr[row + 1]; ++e) {
            const double v = P.c_val[e];
            const double *q = P.qd_c + (int64_t)P.c_idx[e] * kLkbQt;
#pragma unroll
            for (int t = 0; t < kLkbQt; ++t) {
                const double x = q[t] * v;
                dc[t] = dc[t] + x;
            }
        }
        const double cnp = P.norm_p[row], cnc = P.norm_c[row];
#pragma unroll
        for (int t = 0; t < kLkbQt; ++t) {
            const int qr = P.qrow[t];
            double sx = 0.0;
            bool have = false;
            if (qr >= 0 && row != qr)  // person_id =!= personId (KnnRecommender.scala:89)
                have = lkb_similarity(dp[t], dc[t], cnp, cnc, P.norm_p[qr], P.norm_c[qr], P.pw, P.cw, sx);
            if (!have) sx = 0.0;
            // (transposed: one contiguous column per query - what the single request's selection kernels read)
            P.S[P.transposed ? (int64_t)t * P.nrows + row : (int64_t)row * kLkbQt + t] = sx;
            if (have) atomicAdd(&s_cand[t], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < kLkbQt && s_cand[threadIdx.x]) atomicAdd(&cand[threadIdx.x], s_cand[threadIdx.x]);
}

__global__ __launch_bounds__(256) void lkb_scan(const LkbScan P) { lkb_scan_body(P, P.cand, (int)blockIdx.x); }

// the histogram of one query's column of a TRANSPOSED tile (what knn_select1 of knn.hip reads; knn_collect1 then
// reads the column itself): how a batch serves the few queries that cannot ride a packed tile
__global__ __launch_bounds__(256) void lkb_column_hist(const double *col, int32_t nrows, uint32_t *hist)
{
    __shared__ uint32_t s_hist[kLkHistBins];
    col += (size_t)blockIdx.y * (size_t)nrows;   // blockIdx.y = column of the tile
    hist += (size_t)blockIdx.y * kLkHistBins;
    for (int i = threadIdx.x; i < kLkHistBins; i += blockDim.x) s_hist[i] = 0u;
    __syncthreads();
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < nrows; row += gridDim.x * blockDim.x) {
        const double sx = col[row];
        if (sx > 0) {
            const int b = (int)(sx * (double)kLkHistBins);
            atomicAdd(&s_hist[b < kLkHistBins - 1 ? b : kLkHistBins - 1], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kLkHistBins; i += blockDim.x) {
        const uint32_t h = s_hist[i];
        if (h) atomicAdd(&hist[i], h);
    }
}

}  // namespace

namespace locrec {

int32_t knn_large_topk(locrec_knn_index *ix, int32_t qrow, double pw, double cw, int64_t k, int64_t *out_ids,
                       double *out_sims, int64_t *inout_count)
{
    hipStream_t s = ix->stream;
    int64_t cand = 0;
    LOCREC_TRY(sort_all(ix, qrow, pw, cw, &cand));
    const int64_t m = std::min(cand, k);
    const int64_t wr = std::min(m, *inout_count);
    if (wr > 0) {
        LOCREC_TRY(ix->out_ids.reserve((size_t)wr));
        LOCREC_TRY(ix->out_sims.reserve((size_t)wr));
        hipLaunchKernelGGL(lk_emit, dim3((unsigned)((wr + 255) / 256)), dim3(256), 0, s, ix->lk_keys_out.p,
                           ix->lk_vals_out.p, (int32_t)wr, ix->ids_by_rank.p, ix->out_ids.p, ix->out_sims.p);
        if (out_ids) LOCREC_HIP_TRY(hipMemcpyAsync(out_ids, ix->out_ids.p, (size_t)wr * 8, hipMemcpyDeviceToHost, s));
        if (out_sims) LOCREC_HIP_TRY(hipMemcpyAsync(out_sims, ix->out_sims.p, (size_t)wr * 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
    }
    *inout_count = m;
    return LOCREC_OK;
}

// The same top-K, delivered into slot `slot` of the DEVICE result arrays of a batch (ids, similarities,
// neighbour rows, count): how a batch serves a query that is too long for any LDS tile (knn.hip,
// enqueue_topk).  The arrays must already hold (slot + 1) * k entries.
int32_t knn_large_topk_device(locrec_knn_index *ix, int32_t qrow, double pw, double cw, int64_t k, int64_t slot)
{
    hipStream_t s = ix->stream;
    int64_t cand = 0;
    LOCREC_TRY(sort_all(ix, qrow, pw, cw, &cand));
    const int32_t m = (int32_t)std::min(cand, k);
    if ((size_t)((slot + 1) * k) > ix->out_ids.n || (size_t)((slot + 1) * k) > ix->out_rows.n || (size_t)slot >= ix->out_cnt.n)
        return fail(LOCREC_E_DEVICE, "result arrays too small for slot %lld", (long long)slot);
    hipLaunchKernelGGL(lk_emit, dim3((unsigned)std::max<int64_t>(1, (k + 255) / 256)), dim3(256), 0, s, ix->lk_keys_out.p,
                       ix->lk_vals_out.p, m, ix->ids_by_rank.p, ix->out_ids.p + slot * k, ix->out_sims.p + slot * k,
                       ix->row_of_rid.p, ix->out_rows.p + slot * k, ix->out_cnt.p + slot, (int32_t)k);
    LOCREC_HIP_TRY(hipGetLastError());
    return LOCREC_OK;
}

// est[p] = sum r*w / sum w over the raters of p with w > 0 (device weights, one per row)
static int32_t aggregate_places(locrec_knn_index *ix, const double *w, int64_t *out_places, double *out_ratings,
                                int64_t *inout_count)
{
    hipStream_t s = ix->stream;
    const int32_t np = (int32_t)ix->cplace_ids.size();
    LOCREC_TRY(ix->lk_ws.reserve((size_t)np));
    LOCREC_TRY(ix->lk_ss.reserve((size_t)np));
    LOCREC_TRY(ensure_segments(ix));
    const int64_t cap = *inout_count;
    int64_t outn = 0;
    if (np > 0) {
        const int tiles = (np + kFinishTile - 1) / kFinishTile;
        LOCREC_TRY(ix->lk_tile_cnt.reserve((size_t)tiles));
        LOCREC_TRY(ix->lk_out_place.reserve((size_t)np));
        LOCREC_TRY(ix->lk_out_est.reserve((size_t)np));
        LOCREC_TRY(ix->lk_out_n.reserve(1));
        int64_t *pinned_n = nullptr, *pinned_n_dev = nullptr;
        if (knn_stage(ix) && ix->h_stage_dev && !ix->no_pack) {
            pinned_n = reinterpret_cast<int64_t *>(ix->h_stage);
            pinned_n_dev = reinterpret_cast<int64_t *>(ix->h_stage_dev);
        }
        LOCREC_TRY((enqueue_aggregation<1, 8>(ix, w, ix->lk_seg_ws.p, ix->lk_seg_ss.p, ix->lk_ws.p, ix->lk_ss.p, tiles,
                                              ix->lk_tile_cnt.p)));
        // the rated places, compacted in ascending order, with their estimates and their number
        hipLaunchKernelGGL(lk_finish_emit<1>, dim3((unsigned)tiles), dim3(256), 0, s, ix->lk_ws.p, ix->lk_ss.p, np, ix->lk_tile_cnt.p,
                           ix->cplace_dev.p, LkBases<1>{}, ix->lk_out_place.p, ix->lk_out_est.p, ix->lk_out_n.p, pinned_n_dev);
        LOCREC_HIP_TRY(hipGetLastError());
        if (!pinned_n) LOCREC_HIP_TRY(hipMemcpyAsync(&outn, ix->lk_out_n.p, 8, hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        if (pinned_n) outn = *pinned_n;
        const int64_t wr = std::min(cap, outn);
        if (wr > 0 && out_places)
            LOCREC_HIP_TRY(hipMemcpyAsync(out_places, ix->lk_out_place.p, (size_t)wr * 8, hipMemcpyDeviceToHost, s));
        if (wr > 0 && out_ratings)
            LOCREC_HIP_TRY(hipMemcpyAsync(out_ratings, ix->lk_out_est.p, (size_t)wr * 8, hipMemcpyDeviceToHost, s));
        if (wr > 0) LOCREC_HIP_TRY(hipStreamSynchronize(s));
    }
    *inout_count = outn;
    return LOCREC_OK;
}

// the same pass for weights given on the host (one per row, 0 = not a neighbour)
int32_t knn_large_aggregate(locrec_knn_index *ix, const double *w_host, int64_t *out_places, double *out_ratings,
                            int64_t *inout_count)
{
    LOCREC_TRY(ix->lk_w.reserve((size_t)ix->n));
    LOCREC_HIP_TRY(hipMemcpyAsync(ix->lk_w.p, w_host, (size_t)ix->n * sizeof(double), hipMemcpyHostToDevice, ix->stream));
    LOCREC_HIP_TRY(hipStreamSynchronize(ix->stream));  // w_host may be freed by the caller
    return aggregate_places(ix, ix->lk_w.p, out_places, out_ratings, inout_count);
}

int32_t knn_large_recommend(locrec_knn_index *ix, int32_t qrow, double pw, double cw, int64_t k,
                            int64_t *out_places, double *out_ratings, int64_t *inout_count)
{
    hipStream_t s = ix->stream;
    const int32_t n = (int32_t)ix->n;
    // K >= the number of positive-similarity persons - the shipped --k-nearest 2000000 - selects them all:
    // the similarities of the stream scan ARE the weights, nothing needs sorting
    LOCREC_TRY(knn_enqueue_dense(ix, qrow, pw, cw));
    int64_t cand = 0;
    LOCREC_TRY(candidate_count(ix, &cand));
    if (k >= cand) return aggregate_places(ix, ix->S1.p, out_places, out_ratings, inout_count);
    LOCREC_TRY(sort_all(ix, qrow, pw, cw, &cand, true));
    const int64_t m = std::min(cand, k);
    LOCREC_TRY(ix->lk_w.reserve((size_t)n));
    LOCREC_HIP_TRY(hipMemsetAsync(ix->lk_w.p, 0, (size_t)n * sizeof(double), s));
    if (m > 0)
        hipLaunchKernelGGL(lk_scatter_weights, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, ix->lk_keys_out.p,
                           ix->lk_vals_out.p, (int32_t)m, ix->row_of_rid.p, ix->lk_w.p);
    return aggregate_places(ix, ix->lk_w.p, out_places, out_ratings, inout_count);
}

}  // namespace locrec

namespace locrec {

// the presence bitmap of the place table lives behind the table itself (kLkbBitmapBits bits, zero between tiles)
static void lkb_bitmap_of(locrec_knn_index *ix, uint32_t **bits, uint32_t *mask)
{
    uint32_t nbits = 32;
    while (nbits < (uint32_t)std::max(1, ix->fp.dim) && nbits < kLkbBitmapBits) nbits <<= 1;
    *bits = reinterpret_cast<uint32_t *>(ix->lkb_qd_p.p + (size_t)std::max(1, ix->fp.dim) * kLkbQt);
    *mask = nbits - 1u;
}

// the workspaces of a tile scan (lazy, kept with the handle): the tile, the dense query tables (all zero between
// tiles) and the candidate counters
static int32_t lkb_scan_workspaces(locrec_knn_index *ix)
{
    hipStream_t s = ix->stream;
    LOCREC_TRY(ix->lkb_S.reserve((size_t)ix->n * kLkbQt));
    if (!ix->lkb_qd_p.p) {
        LOCREC_TRY(ix->lkb_qd_p.alloc((size_t)std::max(1, ix->fp.dim) * kLkbQt + kLkbBitmapBits / 64));  // (+ the presence bitmap)
        LOCREC_TRY(ix->lkb_qd_c.alloc((size_t)std::max(1, ix->fc.dim) * kLkbQt));
        LOCREC_HIP_TRY(hipMemsetAsync(ix->lkb_qd_p.p, 0, ix->lkb_qd_p.bytes(), s));
        LOCREC_HIP_TRY(hipMemsetAsync(ix->lkb_qd_c.p, 0, ix->lkb_qd_c.bytes(), s));
    }
    LOCREC_TRY(ix->lkb_cand.reserve(kLkbQt));
    return LOCREC_OK;
}

// the workspaces of a batched recommendation (grow-only, kept with the handle)
static int32_t lkb_reserve(locrec_knn_index *ix, int tiles)
{
    const int32_t np = (int32_t)ix->cplace_ids.size();
    LOCREC_TRY(ensure_segments(ix));
    LOCREC_TRY(lkb_scan_workspaces(ix));
    LOCREC_TRY(ix->lkb_seg_ws.reserve((size_t)std::max(1, ix->lk_nsegs) * kLkbQt));
    LOCREC_TRY(ix->lkb_seg_ss.reserve((size_t)std::max(1, ix->lk_nsegs) * kLkbQt));
    LOCREC_TRY(ix->lkb_ws.reserve((size_t)std::max(1, np) * kLkbQt));
    LOCREC_TRY(ix->lkb_ss.reserve((size_t)std::max(1, np) * kLkbQt));
    LOCREC_TRY(ix->lkb_tile_cnt.reserve((size_t)tiles * kLkbQt));
    return LOCREC_OK;
}

// the up to kLkbQt query rows of a tile; a person without a place or category vector is no query (-1)
static int lkt_tile_rows(const locrec_knn_index *ix, const int32_t *rows, int64_t nq, int64_t q0, int32_t *tr, bool *invalid)
{
    const int nt = (int)std::min<int64_t>(kLkbQt, nq - q0);
    for (int t = 0; t < kLkbQt; ++t) {
        const int32_t r = t < nt ? rows[q0 + t] : -1;
        invalid[t] = t < nt && (r < 0 || ix->fp.nnz[(size_t)r] == 0 || ix->fc.nnz[(size_t)r] == 0);
        tr[t] = invalid[t] ? -1 : r;
    }
    return nt;
}

// What the fill and scan kernels get for the tile of the queries rows[0 .. nt) of ix (their `set` is the launch's): the
// dense tables and the bitmap, the CSR rows, the weights, the layout of S, the tile's candidate counters.  maxp / maxc:
// the longest place and category vector among the tile's queries.
static void lkb_describe_tile(locrec_knn_index *ix, const int32_t *rows, int nt, double pw, double cw, bool transposed, int32_t *cand,
                              LkbFill &fp, LkbFill &fc, LkbScan &P, int &maxp, int &maxc)
{
    bool invalid[kLkbQt];
    lkt_tile_rows(ix, rows, nt, 0, P.qrow, invalid);
    for (int t = 0; t < kLkbQt; ++t) {
        const int32_t r = fp.qrow[t] = fc.qrow[t] = P.qrow[t];
        if (r >= 0) {
            maxp = std::max(maxp, ix->fp.nnz[(size_t)r]);
            maxc = std::max(maxc, ix->fc.nnz[(size_t)r]);
        }
    }
    fp.ptr = ix->fp.csr_ptr.p; fp.idx = ix->fp.csr_idx.p; fp.val = ix->fp.csr_val.p; fp.qd = ix->lkb_qd_p.p;
    lkb_bitmap_of(ix, &fp.bits, &fp.bit_mask);
    P.bits = fp.bits;
    P.bit_mask = fp.bit_mask;
    fc.ptr = ix->fc.csr_ptr.p; fc.idx = ix->fc.csr_idx.p; fc.val = ix->fc.csr_val.p; fc.qd = ix->lkb_qd_c.p;
    P.p_ptr = ix->fp.csr_ptr.p; P.p_idx = ix->fp.csr_idx.p; P.p_val = ix->fp.csr_val.p;
    P.c_ptr = ix->fc.csr_ptr.p; P.c_idx = ix->fc.csr_idx.p; P.c_val = ix->fc.csr_val.p;
    P.norm_p = ix->fp.norm.p; P.norm_c = ix->fc.norm.p;
    P.qd_p = ix->lkb_qd_p.p; P.qd_c = ix->lkb_qd_c.p;
    P.nrows = (int32_t)ix->n;
    P.pw = pw; P.cw = cw;
    P.S = ix->lkb_S.p;
    P.cand = cand;
    P.transposed = transposed ? 1 : 0;
}

// One tile of the scan: the similarities of the queries rows[0 .. nt) against every row -> ix->lkb_S, [row][kLkbQt] or
// transposed [kLkbQt][row] (dense fp64 query tables, every candidate walks its plain CSR row: exact in every stored
// format and for every row, wide ones included).  The queries' vectors are scattered into the dense tables, lkb_scan
// runs, the tables are wiped for the next tile.
static int32_t lkb_scan_tile(locrec_knn_index *ix, const int32_t *rows, int nt, double pw, double cw, bool transposed, bool profiled)
{
    hipStream_t s = ix->stream;
    LkbScan P{};
    LkbFill fp{}, fc{};
    int maxp = 1, maxc = 1;
    lkb_describe_tile(ix, rows, nt, pw, cw, transposed, ix->lkb_cand.p, fp, fc, P, maxp, maxc);
    const dim3 gp((unsigned)((maxp + 255) / 256), kLkbQt), gc((unsigned)((maxc + 255) / 256), kLkbQt);
    fp.set = fc.set = 1;
    hipLaunchKernelGGL(lkb_fill, gp, dim3(256), 0, s, fp);
    hipLaunchKernelGGL(lkb_fill, gc, dim3(256), 0, s, fc);
    LOCREC_HIP_TRY(hipMemsetAsync(ix->lkb_cand.p, 0, kLkbQt * sizeof(int32_t), s));
    const dim3 grid((unsigned)((P.nrows + 255) / 256));
    const size_t lds = (P.bit_mask + 1u) / 8u;
    if (profiled) LOCREC_LAUNCH_PROFILED(ix->prof, lkb_scan, grid, dim3(256), lds, s, P);
    else hipLaunchKernelGGL(lkb_scan, grid, dim3(256), lds, s, P);
    fp.set = fc.set = 0;  // the dense tables go back to all zero for the next tile
    hipLaunchKernelGGL(lkb_fill, gp, dim3(256), 0, s, fp);
    hipLaunchKernelGGL(lkb_fill, gc, dim3(256), 0, s, fc);
    LOCREC_HIP_TRY(hipGetLastError());
    return LOCREC_OK;
}

// The first `keep` rows of a grow-only row buffer (place, est) survive its growth to hold `total` rows; the copy is waited
// for (only when keep > 0: the caller counts that wait) before the old pair is freed.
static int32_t lkb_grow_rows(DevBuf<int64_t> &place, DevBuf<double> &est, int64_t total, int64_t keep, hipStream_t s)
{
    DevBuf<int64_t> np_buf;
    DevBuf<double> ne_buf;
    LOCREC_TRY(np_buf.alloc(knn_rows_room(total)));
    LOCREC_TRY(ne_buf.alloc(knn_rows_room(total)));
    if (keep > 0) {
        LOCREC_HIP_TRY(hipMemcpyAsync(np_buf.p, place.p, (size_t)keep * 8, hipMemcpyDeviceToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(ne_buf.p, est.p, (size_t)keep * 8, hipMemcpyDeviceToDevice, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
    }
    std::swap(place.p, np_buf.p); std::swap(place.n, np_buf.n);
    std::swap(est.p, ne_buf.p); std::swap(est.n, ne_buf.n);
    return LOCREC_OK;
}

// The place-major aggregation of one tile: S row-major [row][kLkbQt], column t = the weights of query q0 + t (0 = not a
// neighbour); qrow[t] < 0 marks a slot that is not a valid query.  Appends the tile's rows behind `total` in
// ix->lkb_place / lkb_est and sets their offsets in ix->lkb_off.
static int32_t lkb_aggregate_tile(locrec_knn_index *ix, const double *S, const int32_t *qrow, int64_t q0, int nt, int tiles,
                                  std::vector<int32_t> &tc, int64_t &total)
{
    hipStream_t s = ix->stream;
    const int32_t np = (int32_t)ix->cplace_ids.size();
    if (np > 0) {
        LOCREC_TRY((enqueue_aggregation<kLkbQt, 2>(ix, S, ix->lkb_seg_ws.p, ix->lkb_seg_ss.p, ix->lkb_ws.p, ix->lkb_ss.p, tiles,
                                                   ix->lkb_tile_cnt.p)));
        LOCREC_HIP_TRY(hipMemcpyAsync(tc.data(), ix->lkb_tile_cnt.p, tc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        LkBases<kLkbQt> B{};
        int64_t len[kLkbQt];
        total = knn_tile_bases(tc.data(), tiles, nt, qrow, total, B.base, len);
        for (int t = 0; t < nt; ++t) ix->lkb_off[(size_t)(q0 + t)] = B.base[t];
        // grow-only output with headroom: the rows of the tiles emitted so far (B.base[0] of them) must survive a growth
        if ((size_t)total > ix->lkb_place.n) LOCREC_TRY(lkb_grow_rows(ix->lkb_place, ix->lkb_est, total, B.base[0], s));
        hipLaunchKernelGGL(lk_finish_emit<kLkbQt>, dim3((unsigned)tiles, kLkbQt), dim3(256), 0, s, ix->lkb_ws.p, ix->lkb_ss.p, np,
                           ix->lkb_tile_cnt.p, ix->cplace_dev.p, B, ix->lkb_place.p, ix->lkb_est.p, (int64_t *)nullptr,
                           (int64_t *)nullptr);
        LOCREC_HIP_TRY(hipGetLastError());
    } else {
        for (int t = 0; t < nt; ++t) ix->lkb_off[(size_t)(q0 + t)] = total;
    }
    return LOCREC_OK;
}

// makeRecommendations for the persons at the internal rows rows[0 .. nq) with K >= the number of other persons
// ("every positive-similarity person is a neighbour").  Results stay on the device: ix->lkb_place / lkb_est, rows
// of query i at [lkb_off[i], lkb_off[i + 1]) ordered by place id.  A row that is not a valid query (an empty place
// or category vector: KnnRecommender.scala:77-83 throws for it) gets no rows.
int32_t knn_large_recommend_batch(locrec_knn_index *ix, const int32_t *rows, int64_t nq, double pw, double cw)
{
    const int32_t np = (int32_t)ix->cplace_ids.size();
    ix->have_lkb = false;
    ix->lkb_off.assign((size_t)nq + 1, 0);
    const int tiles = std::max(1, (np + kFinishTile - 1) / kFinishTile);
    LOCREC_TRY(lkb_reserve(ix, tiles));
    std::vector<int32_t> tc((size_t)tiles * kLkbQt);
    int64_t total = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += kLkbQt) {
        int32_t tr[kLkbQt];
        bool invalid[kLkbQt];
        const int nt = lkt_tile_rows(ix, rows, nq, q0, tr, invalid);
        LOCREC_TRY(lkb_scan_tile(ix, tr, nt, pw, cw, false, true));
        LOCREC_TRY(lkb_aggregate_tile(ix, ix->lkb_S.p, tr, q0, nt, tiles, tc, total));
    }
    ix->lkb_off[(size_t)nq] = total;
    ix->have_lkb = true;
    return LOCREC_OK;
}

// The tile scan for the selection kernels: transposed, one contiguous column per query
int32_t knn_large_scan_tile(locrec_knn_index *ix, const int32_t *rows, int nt, double pw, double cw)
{
    if (nt < 1 || nt > kLkbQt) return fail(LOCREC_E_INVALID_ARG, "a tile holds 1 .. %d queries", kLkbQt);
    LOCREC_TRY(lkb_scan_workspaces(ix));
    LOCREC_TRY(lkb_scan_tile(ix, rows, nt, pw, cw, true, false));
    ix->have_lkb = false;  // (a resident large-K batch shares these workspaces)
    return LOCREC_OK;
}

// the histograms of columns 0 .. nt - 1 of the (transposed) tile into hist[t][kLkHistBins] (zeroed by the caller's last
// knn_select1); *cols = the tile itself, columns ix->n similarities apart
int32_t knn_large_tile_hists(locrec_knn_index *ix, int nt, uint32_t *hist, const double **cols)
{
    hipStream_t s = ix->stream;
    const int32_t n = (int32_t)ix->n;
    *cols = ix->lkb_S.p;
    hipLaunchKernelGGL(lkb_column_hist, dim3((unsigned)std::min(512, (n + 255) / 256), (unsigned)nt), dim3(256), 0, s, ix->lkb_S.p, n,
                       hist);
    LOCREC_HIP_TRY(hipGetLastError());
    return LOCREC_OK;
}

}  // namespace locrec

// =====================================================================================================
// Batched top-K at any K (K > LOCREC_KNN_BATCH_MAX_K, beyond the per-query LDS lists; knn_anyk.h).  A tile of up to
// kLkbQt queries:
//   knn_large_scan_tile  S[t][row] (transposed: one contiguous column per query, what the selection reads)
//   lkb_column_hist      one histogram per column, lkt_select the deciding bin b* of each (knn_select1's walk; it also
//                        reports the population of b*, which sizes the column's segment)
//   lkt_collect          every candidate with bin(s) >= b* -> its column's segment as (similarity bits, id rank); the
//                        segments of the tile are laid end to end, sized from the counts read back once per tile
//   lkt_sort_runs        runs of kLktRun entries sorted in LDS (bitonic), cut to K
//   lkt_merge_pass       pairs of runs merged in global memory (merge path: every output finds its own split), cut to K,
//                        until one run per column is left: its first min(K, candidates) entries are the column's top-K
//   lkt_emit             -> the query's result slot (ids, similarities, rows, count), padded with (-1, 0.0, -1)
//   lkt_mask_rows        (recommendations) S masked to each column's selected set, written row-major [row][kLkbQt] for
//                        lk_aggregate_segments<kLkbQt, 2>: one 128-byte line per rater, the single request's kernels
// The order is (similarity desc, id rank asc), a total order: the result does not depend on the order in which the
// collect's atomics fill a segment, and a tie group of any size needs no special case.  No library sort, no host loop
// over queries.  VGPRs (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): lkt_select 12, lkt_collect 16,
// lkt_sort_runs 19 (96 KB dynamic LDS), lkt_merge_pass 32, lkt_emit 14, lkt_mask_rows 40; no scratch.
namespace {

constexpr int kLktRun = 8192;       // entries one block sorts in LDS (12 B each: 96 KB)
constexpr int kLktThreads = 1024;

struct LktTile {
    int64_t off[kLkbQt];    // column t's segment in the ping-pong arrays
    int64_t slot[kLkbQt];   // result slot of column t (lkt_emit), or -1
    int32_t n[kLkbQt];      // entries of the segment: candidates with bin(s) >= bin[t]
    int32_t bin[kLkbQt];    // deciding bin b*
    int32_t m[kLkbQt];      // neighbours: min(K_eff, candidates)
    int32_t all[kLkbQt];    // every candidate is a neighbour (candidates <= K)
    int32_t absent[kLkbQt]; // not a valid query: count -1 (the range forms)
};

// (similarity bits desc, id rank asc): similarities are > 0, so the bit patterns order like the values; the
// knn_device.h better() order
__device__ __forceinline__ bool lkt_better(uint64_t ka, uint32_t ra, uint64_t kb, uint32_t rb)
{
    return ka > kb || (ka == kb && ra < rb);
}

// lkb_column_hist's bin
__device__ __forceinline__ int lkt_bin(double s)
{
    const int b = (int)(s * (double)kLkHistBins);
    return b < kLkHistBins - 1 ? b : kLkHistBins - 1;
}

// knn_select1 for column blockIdx.x (same walk from the top bin down); sel[t * 8 + ...] = b*, above, total, 0 (the
// collect counter), the segment size (above + the population of b*, or total when total <= K).  Leaves the histogram
// zeroed for the next tile.
__global__ __launch_bounds__(1024) void lkt_select(uint32_t *hist, int64_t K, int32_t *sel)
{
    __shared__ uint32_t suf[2][1024];
    const int t = threadIdx.x;
    hist += (size_t)blockIdx.x * kLkHistBins;
    sel += blockIdx.x * 8;
    constexpr int per = kLkHistBins / 1024;
    uint32_t mine = 0;
    for (int i = 0; i < per; ++i) mine += hist[t * per + i];
    suf[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < 1024; d <<= 1) {
        suf[cur ^ 1][t] = suf[cur][t] + (t + d < 1024 ? suf[cur][t + d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t incl = suf[cur][t];
    const uint32_t above_me = incl - mine;
    const uint32_t total = suf[cur][0];
    if ((int64_t)total <= K) {
        if (t == 0) {
            sel[0] = 0;
            sel[1] = (int32_t)(total - hist[0]);
            sel[2] = (int32_t)total;
            sel[4] = (int32_t)total;
        }
    } else if ((int64_t)above_me < K && (int64_t)incl >= K) {  // exactly one thread: the K-th value is in its range
        uint32_t above = above_me;
        int b = t * per + per - 1;
        for (; b > t * per; --b) {
            if ((int64_t)(above + hist[b]) >= K) break;
            above += hist[b];
        }
        sel[0] = b;
        sel[1] = (int32_t)above;
        sel[2] = (int32_t)total;
        sel[4] = (int32_t)(above + hist[b]);
    }
    if (t == 0) sel[3] = 0;
    __syncthreads();
    for (int i = 0; i < per; ++i) hist[t * per + i] = 0u;
}

// grid (row blocks, columns): a block takes `per` rows per thread (strided, coalesced), counts its takers, claims their
// positions with ONE atomic per block and column, then writes them (a second read of its rows); at most a few hundred
// atomics per column (one per wave put every column's counter - one cache line for the tile - at 1.3 ms per tile)
__global__ __launch_bounds__(256) void lkt_collect(const double *S, int32_t nrows, int32_t per, const uint32_t *rid,
                                                   const LktTile T, int32_t *sel, uint64_t *keys, uint32_t *vals)
{
    __shared__ int s_wave[4];
    __shared__ int s_base;
    const int t = blockIdx.y;
    const double *col = S + (size_t)t * nrows;
    const int64_t row0 = (int64_t)blockIdx.x * 256 * per + threadIdx.x;
    const int bin = T.bin[t];
    int c = 0;
    for (int i = 0; i < per; ++i) {
        const int64_t row = row0 + (int64_t)i * 256;
        if (row < nrows) {
            const double s = col[row];
            c += s > 0 && lkt_bin(s) >= bin ? 1 : 0;
        }
    }
    int pos = block_scan_256(c, s_wave);
    if (threadIdx.x == 0) {
        const int tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        s_base = tot ? atomicAdd(&sel[t * 8 + 3], tot) : 0;
    }
    __syncthreads();
    if (c == 0) return;
    pos += s_base;
    for (int i = 0; i < per; ++i) {
        const int64_t row = row0 + (int64_t)i * 256;
        if (row < nrows) {
            const double s = col[row];
            if (s > 0 && lkt_bin(s) >= bin) {
                if (pos < T.n[t]) {
                    keys[T.off[t] + pos] = (uint64_t)__double_as_longlong(s);
                    vals[T.off[t] + pos] = rid[row];
                }
                ++pos;
            }
        }
    }
}

// grid (runs, columns): run blockIdx.x of column t sorted in place, best first; only its first K entries are kept
__global__ __launch_bounds__(kLktThreads) void lkt_sort_runs(const LktTile T, int64_t K, uint64_t *keys, uint32_t *vals)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t *sk = reinterpret_cast<uint64_t *>(smem);
    uint32_t *sr = reinterpret_cast<uint32_t *>(sk + kLktRun);
    const int t = blockIdx.y;
    const int64_t b0 = (int64_t)blockIdx.x * kLktRun;
    const int len = (int)std::min<int64_t>(kLktRun, (int64_t)T.n[t] - b0);
    if (len <= 0) return;  // (block-uniform)
    int n2 = 2;
    while (n2 < len) n2 <<= 1;
    uint64_t *gk = keys + T.off[t] + b0;
    uint32_t *gr = vals + T.off[t] + b0;
    for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        sk[i] = i < len ? gk[i] : 0ull;           // (padding sorts behind every candidate: s > 0)
        sr[i] = i < len ? gr[i] : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int u = threadIdx.x; u < (n2 >> 1); u += blockDim.x) {
                const int i = 2 * u - (u & (j - 1));
                const int l = i + j;
                const bool first_better = (i & k) == 0;
                const uint64_t ki = sk[i], kl = sk[l];
                const uint32_t ri = sr[i], rl = sr[l];
                if (lkt_better(kl, rl, ki, ri) == first_better) {
                    sk[i] = kl; sk[l] = ki;
                    sr[i] = rl; sr[l] = ri;
                }
            }
            __syncthreads();
        }
    }
    const int keep = (int)std::min<int64_t>(len, K);
    for (int i = threadIdx.x; i < keep; i += blockDim.x) {
        gk[i] = sk[i];
        gr[i] = sr[i];
    }
}

// One merge pass: runs of R entries (each holding min(K, its entries) sorted) pairwise into runs of 2R at the first
// run's place, cut to K.  Thread = output position d of a pair: it finds how many of the first d outputs come from the
// first run (binary search along the merge path), then writes the better of the two heads.  grid (outputs, columns).
__global__ __launch_bounds__(256) void lkt_merge_pass(const LktTile T, int64_t K, int64_t R, const uint64_t *ik,
                                                      const uint32_t *ir, uint64_t *ok, uint32_t *orr)
{
    const int t = blockIdx.y;
    const int64_t n = T.n[t];
    const int64_t full = std::min<int64_t>(K, 2 * R);  // outputs of a pair whose runs are both full
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t pair = g / full, d = g - pair * full;
    const int64_t base = pair * 2 * R;
    if (base >= n) return;
    const int64_t na = std::min<int64_t>(K, std::min<int64_t>(R, n - base));
    const int64_t nb = std::min<int64_t>(K, std::max<int64_t>(0, std::min<int64_t>(R, n - base - R)));
    if (d >= std::min<int64_t>(K, na + nb)) return;
    const uint64_t *ak = ik + T.off[t] + base, *bk = ak + R;
    const uint32_t *ar = ir + T.off[t] + base, *br = ar + R;
    int64_t lo = std::max<int64_t>(0, d - nb), hi = std::min<int64_t>(d, na);
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (lkt_better(ak[mid], ar[mid], bk[d - 1 - mid], br[d - 1 - mid])) lo = mid + 1;
        else hi = mid;
    }
    const int64_t a = lo, b = d - lo;
    const bool from_a = a < na && (b >= nb || lkt_better(ak[a], ar[a], bk[b], br[b]));
    ok[T.off[t] + base + d] = from_a ? ak[a] : bk[b];
    orr[T.off[t] + base + d] = from_a ? ar[a] : br[b];
}

// grid (positions of a slot, columns): the column's neighbours into result slot T.slot[t] (stride k), the rest padded
__global__ __launch_bounds__(256) void lkt_emit(const LktTile T, int64_t k, const uint64_t *keys, const uint32_t *vals,
                                                const int64_t *ids_by_rank, const int32_t *row_of_rid, int64_t *out_ids,
                                                double *out_sims, int32_t *out_rows, int64_t *out_cnt)
{
    const int t = blockIdx.y;
    const int64_t slot = T.slot[t];
    if (slot < 0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) out_cnt[slot] = T.absent[t] ? -1 : T.m[t];
    if (i >= k) return;
    const int64_t o = slot * k + i;
    if (i < T.m[t]) {
        const uint32_t rr = vals[T.off[t] + i];
        out_ids[o] = ids_by_rank[rr];
        out_sims[o] = __longlong_as_double((long long)keys[T.off[t] + i]);
        out_rows[o] = row_of_rid[rr];
    } else {
        out_ids[o] = -1;
        out_sims[o] = 0.0;
        out_rows[o] = -1;
    }
}

// SR[row][t] = ST[t][row] when (s, rank) is better than or equal to column t's K-th entry (every candidate when the
// column has no more than K), else 0: the weights of the single request's lk_scatter_weights, per column
__global__ __launch_bounds__(256) void lkt_mask_rows(const double *ST, int32_t nrows, const uint32_t *rid, const LktTile T,
                                                     int64_t K, const uint64_t *keys, const uint32_t *vals, double *SR)
{
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= nrows) return;
    const uint32_t r = rid[row];
    double w[kLkbQt];
#pragma unroll
    for (int t = 0; t < kLkbQt; ++t) {
        const double s = ST[(size_t)t * nrows + row];
        bool keep = s > 0;
        if (keep && !T.all[t]) {
            const int64_t c = T.off[t] + K - 1;  // the K-th entry of the column's sorted run
            keep = !lkt_better(keys[c], vals[c], (uint64_t)__double_as_longlong(s), r);
        }
        w[t] = keep ? s : 0.0;
    }
#pragma unroll
    for (int t = 0; t < kLkbQt; ++t) SR[(size_t)row * kLkbQt + t] = w[t];
}

}  // namespace

namespace locrec {

// the per-column workspaces of a tile (knn_index.h: shared with enqueue_topk's special queries), and lkt_sort_runs' LDS
static_assert(kLkHistBins == cfg::kHistBins, "knn_large.hip restates cfg::kHistBins");
static int32_t lkt_tile_workspaces(locrec_knn_index *ix)
{
    LOCREC_TRY(knn_tile_workspaces(ix));
    return knn_raise_lds_limit(lkt_sort_runs, (size_t)kLktRun * 12);
}

// The top-K of the nt columns of the tile knn_large_scan_tile just left in ix->lkb_S: selection, collect, sort, merge.
// On return column t's first min(K, candidates) entries lie sorted at T.off[t] of *keys / *vals.
static int32_t lkt_topk_tile(locrec_knn_index *ix, int nt, int64_t K, LktTile &T, const uint64_t **keys, const uint32_t **vals)
{
    hipStream_t s = ix->stream;
    const int32_t n = (int32_t)ix->n;
    const double *cols = nullptr;
    LOCREC_TRY(knn_large_tile_hists(ix, nt, ix->tile_hist.p, &cols));
    hipLaunchKernelGGL(lkt_select, dim3((unsigned)nt), dim3(1024), 0, s, ix->tile_hist.p, K, ix->tile_sel.p);
    LOCREC_HIP_TRY(hipGetLastError());
    int32_t sel[kLkbQt * 8];
    LOCREC_HIP_TRY(hipMemcpyAsync(sel, ix->tile_sel.p, (size_t)nt * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    int64_t total = 0, most = 0;
    for (int t = 0; t < kLkbQt; ++t) {
        const bool live = t < nt;
        T.off[t] = total;
        T.n[t] = live ? sel[t * 8 + 4] : 0;
        T.bin[t] = live ? sel[t * 8 + 0] : kLkHistBins;
        const int64_t cand = live ? sel[t * 8 + 2] : 0;
        T.m[t] = (int32_t)std::min<int64_t>(K, cand);
        T.all[t] = cand <= K ? 1 : 0;
        total += T.n[t];
        most = std::max<int64_t>(most, T.n[t]);
    }
    LOCREC_TRY(ix->lk_keys.reserve((size_t)std::max<int64_t>(1, total)));
    LOCREC_TRY(ix->lk_vals.reserve((size_t)std::max<int64_t>(1, total)));
    LOCREC_TRY(ix->lk_keys_out.reserve((size_t)std::max<int64_t>(1, total)));
    LOCREC_TRY(ix->lk_vals_out.reserve((size_t)std::max<int64_t>(1, total)));
    uint64_t *k0 = ix->lk_keys.p, *k1 = ix->lk_keys_out.p;
    uint32_t *v0 = ix->lk_vals.p, *v1 = ix->lk_vals_out.p;
    if (most > 0) {
        const int32_t per = std::max<int32_t>(16, (int32_t)(((int64_t)n + 256 * 256 - 1) / (256 * 256)));  // <= ~256 blocks a column
        const int64_t cblocks = ((int64_t)n + 256 * per - 1) / (256 * per);
        hipLaunchKernelGGL(lkt_collect, dim3((unsigned)cblocks, (unsigned)nt), dim3(256), 0, s, cols, n, per, ix->rid.p, T,
                           ix->tile_sel.p, k0, v0);
        hipLaunchKernelGGL(lkt_sort_runs, dim3((unsigned)((most + kLktRun - 1) / kLktRun), (unsigned)nt), dim3(kLktThreads),
                           (size_t)kLktRun * 12, s, T, K, k0, v0);
        for (int64_t R = kLktRun; R < most; R *= 2) {
            const int64_t full = std::min<int64_t>(K, 2 * R);
            const int64_t outs = (most + 2 * R - 1) / (2 * R) * full;
            hipLaunchKernelGGL(lkt_merge_pass, dim3((unsigned)((outs + 255) / 256), (unsigned)nt), dim3(256), 0, s, T, K, R, k0, v0,
                               k1, v1);
            std::swap(k0, k1);
            std::swap(v0, v1);
        }
    }
    LOCREC_HIP_TRY(hipGetLastError());
    *keys = k0;
    *vals = v0;
    return LOCREC_OK;
}

int32_t knn_topk_tiled(locrec_knn_index *ix, const int32_t *rows, int64_t nq, double pw, double cw, int64_t k, bool mark_absent)
{
    hipStream_t s = ix->stream;
    const int64_t keff = std::min<int64_t>(k, std::max<int64_t>(1, ix->n - 1));  // (H4)
    LOCREC_TRY(ix->out_ids.reserve((size_t)(nq * k)));
    LOCREC_TRY(ix->out_sims.reserve((size_t)(nq * k)));
    LOCREC_TRY(ix->out_rows.reserve((size_t)(nq * k)));
    LOCREC_TRY(ix->out_cnt.reserve((size_t)nq));
    LOCREC_TRY(lkt_tile_workspaces(ix));
    for (int64_t q0 = 0; q0 < nq; q0 += kLkbQt) {
        int32_t tr[kLkbQt];
        bool invalid[kLkbQt];
        const int nt = lkt_tile_rows(ix, rows, nq, q0, tr, invalid);
        LOCREC_TRY(knn_large_scan_tile(ix, tr, nt, pw, cw));
        LktTile T{};
        const uint64_t *keys = nullptr;
        const uint32_t *vals = nullptr;
        LOCREC_TRY(lkt_topk_tile(ix, nt, keff, T, &keys, &vals));
        for (int t = 0; t < kLkbQt; ++t) {
            T.slot[t] = t < nt ? q0 + t : -1;
            T.absent[t] = t < nt && invalid[t] && mark_absent ? 1 : 0;
        }
        hipLaunchKernelGGL(lkt_emit, dim3((unsigned)((k + 255) / 256), (unsigned)nt), dim3(256), 0, s, T, k, keys, vals,
                           ix->ids_by_rank.p, ix->row_of_rid.p, ix->out_ids.p, ix->out_sims.p, ix->out_rows.p, ix->out_cnt.p);
        LOCREC_HIP_TRY(hipGetLastError());
    }
    return LOCREC_OK;
}

int32_t knn_topk_recommend_batch(locrec_knn_index *ix, const int32_t *rows, int64_t nq, double pw, double cw, int64_t k)
{
    hipStream_t s = ix->stream;
    const int32_t n = (int32_t)ix->n;
    const int32_t np = (int32_t)ix->cplace_ids.size();
    ix->have_lkb = false;
    ix->lkb_off.assign((size_t)nq + 1, 0);
    const int tiles = std::max(1, (np + kFinishTile - 1) / kFinishTile);
    LOCREC_TRY(lkb_reserve(ix, tiles));
    // lkb_S: the transposed tile of the scan, then the masked row-major tile of the aggregation behind it
    LOCREC_TRY(ix->lkb_S.reserve((size_t)n * kLkbQt * 2));
    LOCREC_TRY(lkt_tile_workspaces(ix));
    std::vector<int32_t> tc((size_t)tiles * kLkbQt);
    int64_t total = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += kLkbQt) {
        int32_t tr[kLkbQt];
        bool invalid[kLkbQt];
        const int nt = lkt_tile_rows(ix, rows, nq, q0, tr, invalid);
        LOCREC_TRY(knn_large_scan_tile(ix, tr, nt, pw, cw));
        LktTile T{};
        const uint64_t *keys = nullptr;
        const uint32_t *vals = nullptr;
        LOCREC_TRY(lkt_topk_tile(ix, nt, k, T, &keys, &vals));
        double *SR = ix->lkb_S.p + (size_t)n * kLkbQt;
        hipLaunchKernelGGL(lkt_mask_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ix->lkb_S.p, n, ix->rid.p, T, k,
                           keys, vals, SR);
        LOCREC_HIP_TRY(hipGetLastError());
        LOCREC_TRY(lkb_aggregate_tile(ix, SR, tr, q0, nt, tiles, tc, total));
    }
    ix->lkb_off[(size_t)nq] = total;
    ix->have_lkb = true;
    return LOCREC_OK;
}

}  // namespace locrec

// a pool of indexes: the kernels above for every member's tile in shared launches (locrec_knn_pool_*, knn_batch.hip)
#include "knn_pool.h"

// visitors: rating vectors that are no rows of the index, through the tile scan above (locrec_knn_visitors_*, knn_batch.hip)
#include "knn_visitors.h"

// a mixed batch of visitors over a pool of indexes: the pool's waves with the visitors' stage and scan
// (locrec_knn_pool_visitors_*, knn_batch.hip)
#include "knn_pool_visitors.h"
