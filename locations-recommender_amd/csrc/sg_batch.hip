// sg_batch.hip -- batched SG requests: makeRecommendations (StochasticRecommender.scala:66-141) for many targets of ONE
// graph, a tile of up to kBatchB of them per sweep (locrec_sg_recommend_batch).
//
// This file is the SG translation unit: it includes sg.hip whole (the handle, its layout and the device helpers the
// batched kernels share with the single request) and adds the batched path behind it.  sg.hip itself stays as it is:
// its bytes are part of the hash that ties the committed rocprofv3 counter record to the kernels it measured
// (bench.py PMC_SOURCES).  For the same reason the batch keeps its device buffers in handle members sg.hip allocates
// only for the fused experiment (LOCREC_SG_FUSED), whose handles the batch refuses:
//   PA4         x of the tile, (T + 1 + kBatchB) rows x kBatchB columns, two parities
//   XL          the partials, pa_stride slots x kBatchB
//   D2W         the block sums, 2 x kParts x kBatchB
//   fused_conv  the tile's SgBatchState
// They are allocated on the first batch and kept, like the other work buffers, and freed with the handle.

#include "sg.hip"

#include <unordered_map>

namespace {

// 16 fp64 columns = one 128-byte line per gathered x row.  VGPRs (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
// sg_sweep_batch 92 / 60 (uint16 columns, dictionary / fp64 weights), 80 / 130 (int32 columns), sg_finalize_batch 153,
// sg_finalize_visitors (sg_visitors.h) 118; no scratch.
constexpr int kBatchB = 16;

struct SgBatchState {
    int32_t done[kBatchB];    // per column, sticky as SgState::done
    int32_t sweeps[kBatchB];  // per column: executed finalize passes (the column's x is at parity sweeps & 1)
    int32_t all_done;         // every column of the tile is done: the sweeps and finalizes left are no-ops
    int32_t pad[3];
};

}  // namespace

// ---------------------------------------------------------------------------------------------------
// A tile of nb <= kBatchB distinct targets shares every sweep.  x is stored as (T + 1 + kBatchB) rows x kBatchB
// columns, row-major, two parities: column b is tile target b's x.  Rows 0 .. T-1 are the live vertices and row T is D,
// as in the single request; row T + 1 + j is the private slot of tile target j when that target is source-only (its
// out-edge slots point there for the length of the tile).  In column b that row holds Q's value if j == b and D's value
// otherwise, so every column sees exactly the x of its single request.  A gathered source row is 16 contiguous fp64
// values (one 128-byte line), and the column and weight (index) loads of a piece are issued once for all columns.
// Per column the arithmetic is the single request's: the four products added left to right, the segment butterfly of
// the piece's class, one partial per segment; the finalize keeps sg_finalize_body's thread -> row mapping and the order
// of every sum.  Each column has its own sticky `done` flag and sweep count, and its result is read from the parity of
// its last executed sweep.

namespace {

constexpr int kBatchRanges = 2 * kBatchB + 1;  // slot ranges one set-up re-points: the previous tile's, the new tile's
constexpr size_t kBatchPackHead = 256;         // bytes in front of the packed block sums (the SgBatchState)

template <int STEP>
__device__ __forceinline__ void butterfly_step_all(double (&s)[kBatchB])
{
#pragma unroll
    for (int b = 0; b < kBatchB; ++b) s[b] = butterfly_step<STEP>(s[b]);
}

// segment_butterfly_sum for every column (cls wave-uniform): per column the same steps in the same order
__device__ __forceinline__ void segment_butterfly_sum_all(double (&s)[kBatchB], int cls)
{
    if (cls >= 1) butterfly_step_all<0>(s);
    if (cls >= 2) butterfly_step_all<1>(s);
    if (cls >= 3) butterfly_step_all<2>(s);
    if (cls >= 4) butterfly_step_all<3>(s);
    if (cls >= 5) butterfly_step_all<4>(s);
    if (cls >= 6) butterfly_step_all<5>(s);
}

// Batched sg_sweep / sg_sweep_dict: one wave per piece, its column and weight (index) loads once for all columns.
// bx is the block's index among the blocks of ITS graph (sg_sweep_batch: blockIdx.x; sg_sweep_pool, sg_pool.h: behind the
// graph's block base), as sg_sweep_body serves sg_sweep and sg_sweep_group.
template <bool COL16, bool DICT>
__device__ __forceinline__ void sg_sweep_batch_body(
    const void *__restrict__ colv, const v2d *__restrict__ w2, const v4h *__restrict__ widx, const double *__restrict__ dict,
    const int32_t ndict, const int2 *__restrict__ pinfo, const int32_t *__restrict__ seg_out, const double *__restrict__ x_in,
    double *__restrict__ partial, const int32_t npieces, const SgBatchState *__restrict__ st, const int bx)
{
    extern __shared__ double tbl[];
    const int lane = threadIdx.x & 63;
    const int p0 = __builtin_amdgcn_readfirstlane(bx * 4 + (threadIdx.x >> 6));
    const int p = min(p0, npieces - 1);  // (npieces >= 1: the launch has no blocks otherwise)
    int c[4];
    if constexpr (COL16) {
        const v4h cc = __builtin_nontemporal_load(&reinterpret_cast<const v4h *>(colv)[(int64_t)p * 64 + lane]);
        c[0] = cc.x; c[1] = cc.y; c[2] = cc.z; c[3] = cc.w;
    } else {
        const v4i cc = __builtin_nontemporal_load(&reinterpret_cast<const v4i *>(colv)[(int64_t)p * 64 + lane]);
        c[0] = cc.x; c[1] = cc.y; c[2] = cc.z; c[3] = cc.w;
    }
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    v4h wi = {0, 0, 0, 0};
    if constexpr (DICT) {
        wi = __builtin_nontemporal_load(&widx[(int64_t)p * 64 + lane]);
    } else {
        const v2d wa = __builtin_nontemporal_load(&w2[(int64_t)p * 128 + lane]);
        const v2d wb = __builtin_nontemporal_load(&w2[(int64_t)p * 128 + 64 + lane]);
        w[0] = wa.x; w[1] = wa.y; w[2] = wb.x; w[3] = wb.y;
    }
    const int2 info = pinfo[p];
    const int all_done = st->all_done;
    if constexpr (DICT) {
        for (int i = threadIdx.x; i < ndict; i += blockDim.x) tbl[i] = dict[i];
        __syncthreads();
        w[0] = tbl[wi.x]; w[1] = tbl[wi.y]; w[2] = tbl[wi.z]; w[3] = tbl[wi.w];
    }
    if (all_done || p0 >= npieces) return;
    const int cls = __builtin_amdgcn_readfirstlane(info.y);
    const int tgt = seg_out[info.x + (lane >> cls)];
    double s[kBatchB];
    {
        const v2d *xr = reinterpret_cast<const v2d *>(x_in + (size_t)c[0] * kBatchB);
#pragma unroll
        for (int k = 0; k < kBatchB / 2; ++k) {
            const v2d v = xr[k];
            s[2 * k] = v.x * w[0];  // col("probability") * col("balanced_weight") (:112)
            s[2 * k + 1] = v.y * w[0];
        }
    }
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const v2d *xr = reinterpret_cast<const v2d *>(x_in + (size_t)c[j] * kBatchB);
#pragma unroll
        for (int k = 0; k < kBatchB / 2; ++k) {
            const v2d v = xr[k];
            s[2 * k] = s[2 * k] + v.x * w[j];
            s[2 * k + 1] = s[2 * k + 1] + v.y * w[j];
        }
    }
    segment_butterfly_sum_all(s, cls);
    if ((lane & ((1 << cls) - 1)) == 0 && tgt >= 0) {
        v2d *pr = reinterpret_cast<v2d *>(partial + (size_t)tgt * kBatchB);
#pragma unroll
        for (int k = 0; k < kBatchB / 2; ++k) pr[k] = v2d{s[2 * k], s[2 * k + 1]};
    }
}

template <bool COL16, bool DICT>
__global__ __launch_bounds__(256) void sg_sweep_batch(
    const void *__restrict__ colv, const v2d *__restrict__ w2, const v4h *__restrict__ widx, const double *__restrict__ dict,
    const int32_t ndict, const int2 *__restrict__ pinfo, const int32_t *__restrict__ seg_out, const double *__restrict__ x_in,
    double *__restrict__ partial, const int32_t npieces, const SgBatchState *__restrict__ st)
{
    sg_sweep_batch_body<COL16, DICT>(colv, w2, widx, dict, ndict, pinfo, seg_out, x_in, partial, npieces, st, (int)blockIdx.x);
}

// What a tile's finalize needs per column (sg_finalize_batch takes it by value: its launches are issued directly, not
// replayed; sg_finalize_pool reads it from its graph's row of a device table)
struct SgBatchReq {
    int32_t target_x[kBatchB];      // row of column b's target: its live index, or T + 1 + b when it is source-only
    int32_t n_plain_dead[kBatchB];  // source-only vertices other than column b's target (they hold D's value)
    int32_t q_in_use[kBatchB];      // column b's target is source-only
    int32_t nb, T;
    double alpha, oma, eps2;
};

__device__ __forceinline__ void batch_add_row(double (&s)[kBatchB], const double *__restrict__ row)
{
    const v2d *r = reinterpret_cast<const v2d *>(row);
#pragma unroll
    for (int k = 0; k < kBatchB / 2; ++k) {
        const v2d v = r[k];
        s[2 * k] = s[2 * k] + v.x;
        s[2 * k + 1] = s[2 * k + 1] + v.y;
    }
}

// The tables of a visitors tile (sg_visitors.h): slot[r] is live row r's line of w, or -1 when no visitor of the tile
// points at r; w[slot][b] is the weight of column b's visitor's edge to r, +0.0 where it has none
struct SgVisTables {
    const int32_t *slot;
    const double *w;
};

// A visitors tile: sigma'(r) = sigma(r) + x_V(b) * w_{b->r} in every column, the product last (where a fold over the
// graph's edges followed by the visitor's puts it).  x_V(b) is column b's private row.  One 4-byte load a row otherwise.
template <bool VIS>
__device__ __forceinline__ void batch_add_visitors(double (&s)[kBatchB], int row, int T, const SgVisTables &vt,
                                                   const double *__restrict__ x_in)
{
    if constexpr (VIS) {
        const int32_t sl = vt.slot[row];
        if (sl >= 0) {
            const double *w = vt.w + (size_t)sl * kBatchB;
#pragma unroll
            for (int b = 0; b < kBatchB; ++b) s[b] = s[b] + x_in[(size_t)(T + 1 + b) * kBatchB + b] * w[b];
        }
    }
}

// x' of one live row in every column (:115-126), its diff^2 into the column's sum; done columns are not written
__device__ __forceinline__ void batch_combine(const SgBatchReq &rq, uint32_t act, int row, const double (&s)[kBatchB],
                                              const double *__restrict__ x_in, double *__restrict__ x_out, double (&d2)[kBatchB])
{
    const v2d *xo = reinterpret_cast<const v2d *>(x_in + (size_t)row * kBatchB);
    double *xw = x_out + (size_t)row * kBatchB;
#pragma unroll
    for (int k = 0; k < kBatchB / 2; ++k) {
        const v2d o = xo[k];
        const double n0 = sg_next_x(s[2 * k], row == rq.target_x[2 * k], rq.alpha, rq.oma);
        const double n1 = sg_next_x(s[2 * k + 1], row == rq.target_x[2 * k + 1], rq.alpha, rq.oma);
        const double e0 = n0 - o.x, e1 = n1 - o.y;
        d2[2 * k] = d2[2 * k] + e0 * e0;
        d2[2 * k + 1] = d2[2 * k + 1] + e1 * e1;
        if ((act >> (2 * k)) & 3u) {
            if (((act >> (2 * k)) & 3u) == 3u) {
                *reinterpret_cast<v2d *>(xw + 2 * k) = v2d{n0, n1};
            } else if ((act >> (2 * k)) & 1u) {
                xw[2 * k] = n0;
            } else {
                xw[2 * k + 1] = n1;
            }
        }
    }
}

// Batched sg_finalize_body: the same rows per thread / wave, the same order of every sum, per column.  bx is the block's
// index among the kParts blocks of its graph.  VIS: the tile's columns are visitors (vt, batch_add_visitors); every other
// instantiation compiles to what it was.
template <bool VIS = false>
__device__ __forceinline__ void sg_finalize_batch_body(
    const SgBatchReq &rq, const int bx, int32_t n_short, const int4 *__restrict__ lrows, int32_t nlrows, int32_t n_crows,
    const double *__restrict__ partial, const double *__restrict__ x_in, double *__restrict__ x_out,
    const double *__restrict__ parts_prev, double *__restrict__ parts_out, SgBatchState *st, int32_t first,
    const SgVisTables vt = SgVisTables{nullptr, nullptr})
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // the columns this launch advances: isConverged of each column's PREVIOUS sweep (:99), decided by every wave from
    // the same block sums in the same order as sg_finalize; a done column is never written again
    uint32_t act = 0;
    for (int b = 0; b < rq.nb; ++b) {
        bool on = true;
        if (!first) {
            const double tot = wave_butterfly_sum(parts_prev[lane * kBatchB + b]);
            on = !(st->done[b] != 0 || tot <= rq.eps2);
        }
        if (on) act |= 1u << b;
    }
    act = (uint32_t)__builtin_amdgcn_readfirstlane((int)act);
    if (!first && bx == 0 && threadIdx.x == 0) {
        for (int b = 0; b < rq.nb; ++b)
            if (!((act >> b) & 1u)) st->done[b] = 1;
        if (act == 0) st->all_done = 1;
    }
    if (act == 0) return;
    const int T = rq.T;
    const int n_brows = nlrows - n_crows;
    double d2[kBatchB];
#pragma unroll
    for (int b = 0; b < kBatchB; ++b) d2[b] = 0.0;
    // one thread per medium row (3 .. kLongRow full pieces), its partials added in slot order
    for (int bi = bx + kParts * (int)threadIdx.x; bi < n_brows; bi += kParts * 256) {
        const int4 r = lrows[n_crows + bi];
        double s[kBatchB];
#pragma unroll
        for (int b = 0; b < kBatchB; ++b) s[b] = 0.0;
        for (int j = 0; j < r.z; ++j) batch_add_row(s, partial + (size_t)(r.y + j) * kBatchB);
        if (r.w) batch_add_row(s, partial + (size_t)(r.y + r.z) * kBatchB);
        batch_add_visitors<VIS>(s, r.x, T, vt, x_in);
        batch_combine(rq, act, r.x, s, x_in, x_out, d2);
    }
    // one wave per long row: each lane adds its strided partials in ascending order, a butterfly, then the remainder
    for (int i = bx * 4 + wave; i < n_crows; i += kParts * 4) {
        const int4 r = lrows[i];
        double s[kBatchB];
#pragma unroll
        for (int b = 0; b < kBatchB; ++b) s[b] = 0.0;
        for (int j = lane; j < r.z; j += 64) batch_add_row(s, partial + (size_t)(r.y + j) * kBatchB);
#pragma unroll
        for (int b = 0; b < kBatchB; ++b) s[b] = wave_butterfly_sum(s[b]);
        if (r.w) batch_add_row(s, partial + (size_t)(r.y + r.z) * kBatchB);
        if (lane == 0) {
            batch_add_visitors<VIS>(s, r.x, T, vt, x_in);
            batch_combine(rq, act, r.x, s, x_in, x_out, d2);
        }
    }
    // the short rows: three partial slots each
    for (int l = bx * 256 + (int)threadIdx.x; l < n_short; l += kParts * 256) {
        double s[kBatchB];
#pragma unroll
        for (int b = 0; b < kBatchB; ++b) s[b] = 0.0;
        const double *p = partial + (size_t)(3 * l) * kBatchB;
        batch_add_row(s, p);
        batch_add_row(s, p + kBatchB);
        batch_add_row(s, p + 2 * kBatchB);
        batch_add_visitors<VIS>(s, l, T, vt, x_in);
        batch_combine(rq, act, l, s, x_in, x_out, d2);
    }
    if (bx == 0 && threadIdx.x == 0) {
        // D, and the private rows: column b's own is its Q (summed when its target is source-only), the other
        // targets' are copies of D there (written, not summed: those vertices are counted in n_plain_dead)
        const double xd = sg_next_x(0.0, false, rq.alpha, rq.oma);
#pragma unroll
        for (int b = 0; b < kBatchB; ++b) {
            if (!((act >> b) & 1u)) continue;
            const double dd = xd - x_in[(size_t)T * kBatchB + b];
            x_out[(size_t)T * kBatchB + b] = xd;
            d2[b] = d2[b] + (double)rq.n_plain_dead[b] * (dd * dd);
            for (int j = 0; j < rq.nb; ++j) {
                const size_t at = (size_t)(T + 1 + j) * kBatchB + b;
                if (j == b) {
                    const double xq = sg_next_x(0.0, rq.q_in_use[b] != 0, rq.alpha, rq.oma);
                    const double dq = xq - x_in[at];
                    x_out[at] = xq;
                    if (rq.q_in_use[b]) d2[b] = d2[b] + dq * dq;
                } else {
                    x_out[at] = xd;
                }
            }
        }
    }
    __shared__ double wsum[4][kBatchB];
#pragma unroll
    for (int b = 0; b < kBatchB; ++b) {
        const double t = wave_butterfly_sum(d2[b]);
        if (lane == 0) wsum[wave][b] = t;
    }
    __syncthreads();
    if (threadIdx.x < kBatchB) {
        const int b = threadIdx.x;
        if ((act >> b) & 1u) {
            double t = wsum[0][b];
            t = t + wsum[1][b];
            t = t + wsum[2][b];
            t = t + wsum[3][b];
            parts_out[bx * kBatchB + b] = t;
            if (bx == 0) st->sweeps[b] = st->sweeps[b] + 1;  // nobody reads it inside this launch
        }
    }
}

__global__ __launch_bounds__(256) void sg_finalize_batch(
    const SgBatchReq rq, int32_t n_short, const int4 *__restrict__ lrows, int32_t nlrows, int32_t n_crows,
    const double *__restrict__ partial, const double *__restrict__ x_in, double *__restrict__ x_out,
    const double *__restrict__ parts_prev, double *__restrict__ parts_out, SgBatchState *st, int32_t first)
{
    sg_finalize_batch_body(rq, (int)blockIdx.x, n_short, lrows, nlrows, n_crows, partial, x_in, x_out, parts_prev, parts_out, st,
                           first);
}

// A tile's set-up in one launch: x0 (:51-54) in every row and column of the first x buffer, the state and block sums
// reset, and the out-edge slots of listed source-only vertices re-pointed (the previous tile's back at D, this tile's at
// their private rows).  nx = 0: the slot ranges only (the end of a batch).
struct SgBatchBegin {
    double *x;
    double *parts;
    SgBatchState *st;
    void *col;              // uint16 or int32 column indices
    const int32_t *slots;   // dead_slots, resident
    double x0;
    int64_t nx;
    int32_t col16, nb, nranges, pad;
    int32_t off[kBatchRanges], cnt[kBatchRanges], val[kBatchRanges];  // (the ranges belong to different vertices: disjoint)
};

__device__ __forceinline__ void sg_begin_batch_body(const SgBatchBegin &b)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    const int stride = gridDim.x * 256;
    for (int64_t j = i; j < b.nx; j += stride) b.x[j] = b.x0;
    for (int r = 0; r < b.nranges; ++r) {
        const int32_t off = b.off[r], cnt = b.cnt[r], val = b.val[r];
        for (int j = i; j < cnt; j += stride) {
            const int32_t slot = b.slots[off + j];
            if (b.col16) static_cast<unsigned short *>(b.col)[slot] = (unsigned short)val;
            else static_cast<int32_t *>(b.col)[slot] = val;
        }
    }
    if (b.nx > 0 && blockIdx.x == 0) {
        if (threadIdx.x < kBatchB) {
            b.st->done[threadIdx.x] = (int)threadIdx.x < b.nb ? 0 : 1;  // (unused columns count as done)
            b.st->sweeps[threadIdx.x] = 0;
        }
        if (threadIdx.x == 0) b.st->all_done = 0;
        for (int j = threadIdx.x; j < 2 * kParts * kBatchB; j += 256) b.parts[j] = 0.0;
    }
}

__global__ __launch_bounds__(256) void sg_begin_batch(const SgBatchBegin b) { sg_begin_batch_body(b); }

__global__ void sg_poll_batch(const SgBatchState *__restrict__ st, int32_t *host_word)
{
    if (threadIdx.x == 0) *host_word = st->all_done;
}

// The tile's read-back in one launch: the state at 0, both parities' block sums at kBatchPackHead, then rows 0 .. T
// (the live vertices and D) of x, every column from the parity its last executed sweep wrote, row-major.
__device__ __forceinline__ void sg_pack_batch_body(const SgBatchState *__restrict__ st, const double *__restrict__ parts,
                                                   const double *__restrict__ xbuf, int64_t x_parity_stride, int32_t nrows,
                                                   unsigned char *out)
{
    __shared__ int32_t par[kBatchB];
    if (threadIdx.x < kBatchB) par[threadIdx.x] = st->sweeps[threadIdx.x] & 1;
    __syncthreads();
    const int t = blockIdx.x * 256 + (int)threadIdx.x;
    const int stride = gridDim.x * 256;
    if (t < (int)(sizeof(SgBatchState) / 4)) reinterpret_cast<int32_t *>(out)[t] = reinterpret_cast<const int32_t *>(st)[t];
    double *hp = reinterpret_cast<double *>(out + kBatchPackHead);
    for (int i = t; i < 2 * kParts * kBatchB; i += stride) hp[i] = parts[i];
    double *hx = hp + 2 * kParts * kBatchB;
    const int64_t n = (int64_t)nrows * kBatchB;
    for (int64_t i = t; i < n; i += stride) hx[i] = xbuf[par[i & (kBatchB - 1)] * x_parity_stride + i];
}

__global__ __launch_bounds__(256) void sg_pack_batch(const SgBatchState *__restrict__ st, const double *__restrict__ parts,
                                                     const double *__restrict__ xbuf, int64_t x_parity_stride, int32_t nrows,
                                                     unsigned char *out)
{
    sg_pack_batch_body(st, parts, xbuf, x_parity_stride, nrows, out);
}

struct SlotRange {
    int32_t off, cnt, val;
};

// What the batched entries share (locrec_sg_recommend_batch below, locrec_sg_recommend_ranked_batch in sg_ranked.h,
// locrec_sg_pool_recommend_batch in sg_pool.h): the requires and refusals, the distinct targets, a tile's set-up rows, the
// verdict on a column, the tile loop and the host's side of a tile's read-back.
struct SgBatchCtx {
    hipStream_t s = nullptr;
    int32_t T = 0;
    int64_t xstride = 0;             // one parity of x
    SgBatchState *bstate = nullptr;  // the tile's state, on the device
    double eps2 = 0;
    int64_t max_iterations = 0;  // (cut to INT32_MAX)
    int64_t polls = 0;           // convergence words read so far
};

// require()s of the constructor (StochasticRecommender.scala:33-34)
int32_t sg_batch_requires(double epsilon, int64_t max_iterations)
{
    if (!(epsilon >= 0)) return fail(LOCREC_E_INVALID_ARG, "requirement failed: epsilon must be non-negative");
    if (max_iterations < 0)
        return fail(LOCREC_E_INVALID_ARG, "requirement failed: max iterations number must be non-negative");
    return LOCREC_OK;
}

// why a handle serves no batched request (NULL: it does)
const char *sg_batch_refusal(const locrec_sg_graph *g)
{
    if (g->shard_count != 1) return "a sharded graph is iterated with locrec_sg_shard_* (it holds only part of the edges)";
    if (g->env_fused || g->env_persist)  // (other kernels serve their single requests; the fused one's buffers are the batch's)
        return "batched requests are not served on a handle of the fused or persistent experiment";
    return nullptr;
}

// isVertexExist (:70-77): the vertex's index, or -1
inline int32_t sg_vertex_index(const locrec_sg_graph *g, int64_t vertex_id)
{
    auto it = std::lower_bound(g->vid.begin(), g->vid.end(), vertex_id);
    return it == g->vid.end() || *it != vertex_id ? -1 : (int32_t)(it - g->vid.begin());
}

// The requires, the handles a batch refuses, and isVertexExist for every target before any device work; a repeated target
// is computed once
int32_t sg_batch_targets(locrec_sg_graph *g, int64_t n_targets, const int64_t *vertex_ids, double epsilon,
                         int64_t max_iterations, std::vector<int32_t> &uniq, std::vector<int32_t> &uniq_of)
{
    LOCREC_TRY(sg_batch_requires(epsilon, max_iterations));
    if (const char *why = sg_batch_refusal(g)) return fail(LOCREC_E_INVALID_ARG, "%s", why);
    uniq.clear();                          // vertex index of each distinct target, in order of appearance
    uniq_of.assign((size_t)n_targets, 0);  // input position -> its entry of uniq
    std::unordered_map<int32_t, int32_t> seen;
    for (int64_t i = 0; i < n_targets; ++i) {
        const int32_t tv = sg_vertex_index(g, vertex_ids[i]);
        if (tv < 0) return fail(LOCREC_E_NOT_FOUND, "No such vertex in the graph: %lld", (long long)vertex_ids[i]);
        auto ins = seen.emplace(tv, (int32_t)uniq.size());
        if (ins.second) uniq.push_back(tv);
        uniq_of[(size_t)i] = ins.first->second;
    }
    return LOCREC_OK;
}

// targets of a tile: uint16 columns address rows up to 65535, so a graph with T close to that takes fewer private rows
inline int sg_batch_tile_max(const locrec_sg_graph *g) { return g->use16 ? std::min(kBatchB, 65535 - g->nlive) : kBatchB; }

inline int64_t sg_batch_xstride(const locrec_sg_graph *g) { return ((int64_t)g->nlive + 1 + kBatchB) * kBatchB; }  // one parity of x

// The batch's device buffers (the head of this file), allocated at the handle's first batch; s orders the clearing
int32_t sg_batch_buffers(locrec_sg_graph *g, hipStream_t s)
{
    if (g->PA4.p) return LOCREC_OK;
    LOCREC_TRY(g->PA4.alloc((size_t)(2 * sg_batch_xstride(g))));
    LOCREC_TRY(g->XL.alloc((size_t)std::max(1, g->pa_stride) * kBatchB));
    LOCREC_TRY(g->D2W.alloc(2 * kParts * kBatchB));
    LOCREC_TRY(g->fused_conv.alloc(sizeof(SgBatchState) / sizeof(int32_t)));
    // (partial slots no sweep writes - a short row's missing full pieces or remainder - stay 0.0 for good)
    LOCREC_HIP_TRY(hipMemsetAsync(g->XL.p, 0, g->XL.bytes(), s));
    return LOCREC_OK;
}

inline const void *sg_batch_columns(const locrec_sg_graph *g)
{
    return g->use16 ? static_cast<const void *>(g->col16.p) : static_cast<const void *>(g->col4.p);
}

// The slot ranges of a handle that point at the single request's Q and go back to D next: taken over by the batch
inline void sg_batch_take_patched(locrec_sg_graph *g, std::vector<SlotRange> &pointed)
{
    pointed.clear();
    if (g->n_patched > 0) pointed.push_back(SlotRange{(int32_t)g->patched_off, g->n_patched, g->nlive});
    g->patched_off = 0;
    g->n_patched = 0;
}

// The set-up and finalize rows of the tile uniq[t0 .. t0 + nb): `pointed` lists the slot ranges that point at a private
// row (or at the single request's Q) now and leaves as this tile's
void sg_batch_tile_rows(const locrec_sg_graph *g, const std::vector<int32_t> &uniq, size_t t0, int nb, double alpha, double eps2,
                        std::vector<SlotRange> &pointed, SgBatchBegin &b, SgBatchReq &rq)
{
    const int32_t T = g->nlive;
    b = SgBatchBegin{};
    b.x = g->PA4.p;
    b.parts = g->D2W.p;
    b.st = reinterpret_cast<SgBatchState *>(g->fused_conv.p);
    b.col = const_cast<void *>(sg_batch_columns(g));
    b.slots = g->dead_slots_dev.p;
    b.x0 = 1.0 / (double)g->nv;  // :51-54
    b.nx = sg_batch_xstride(g);
    b.col16 = g->use16 ? 1 : 0;
    b.nb = nb;
    rq = SgBatchReq{};
    rq.nb = nb;
    rq.T = T;
    rq.alpha = alpha;
    rq.oma = 1 - alpha;  // :121
    rq.eps2 = eps2;
    std::vector<SlotRange> fresh;
    for (int j = 0; j < nb; ++j) {
        const int32_t tv = uniq[t0 + (size_t)j];
        const bool dead = g->live_of[tv] < 0;
        rq.target_x[j] = dead ? T + 1 + j : g->live_of[tv];
        rq.n_plain_dead[j] = (int32_t)(g->nv - T) - (dead ? 1 : 0);
        rq.q_in_use[j] = dead ? 1 : 0;
        const int32_t n = dead ? (int32_t)(g->dead_ptr[tv + 1] - g->dead_ptr[tv]) : 0;
        if (n > 0) fresh.push_back(SlotRange{(int32_t)g->dead_ptr[tv], n, T + 1 + j});
    }
    for (const SlotRange &r : pointed) {
        bool again = false;  // the same vertex is re-pointed by this tile: one write per slot
        for (const SlotRange &f : fresh) again |= f.off == r.off;
        if (!again) {
            b.off[b.nranges] = r.off;
            b.cnt[b.nranges] = r.cnt;
            b.val[b.nranges++] = T;
        }
    }
    for (const SlotRange &f : fresh) {
        b.off[b.nranges] = f.off;
        b.cnt[b.nranges] = f.cnt;
        b.val[b.nranges++] = f.val;
    }
    pointed = fresh;
}

// The set-up row that only points the last tile's slots back at D: the handle's column array is as a fresh handle's
// (nothing points at Q)
void sg_batch_restore_row(const locrec_sg_graph *g, const std::vector<SlotRange> &pointed, SgBatchBegin &b)
{
    b = SgBatchBegin{};
    b.col = const_cast<void *>(sg_batch_columns(g));
    b.slots = g->dead_slots_dev.p;
    b.col16 = g->use16 ? 1 : 0;
    for (const SlotRange &r : pointed) {
        b.off[b.nranges] = r.off;
        b.cnt[b.nranges] = r.cnt;
        b.val[b.nranges++] = g->nlive;
    }
}

// step(), :92-106: which of the two exits a column took (as locrec_sg_fetch decides it).  total() is the sum of the block
// sums of the column's last executed sweep, added as the finalize adds them; it is asked for only when a sweep ran.
template <class Total>
int32_t sg_batch_verdict(int64_t sweeps, Total &&total, double eps2, int64_t max_iterations, int64_t *iterations,
                         int32_t *converged)
{
    *converged = 0;
    *iterations = max_iterations;
    if (sweeps > 0 && total() <= eps2) {
        *converged = 1;
        *iterations = sweeps - 1;
    }
    if (!*converged && sweeps != max_iterations)
        return fail(LOCREC_E_DEVICE, "internal: %lld sweeps executed, %lld expected", (long long)sweeps,
                    (long long)max_iterations);
    return LOCREC_OK;
}

// What the columns of a batch's tiles are: distinct vertices of the graph (here), or visitors (SgVisitorTiles, sg_visitors.h)
struct SgPersonTiles {
    const std::vector<int32_t> &uniq;
    size_t count() const { return uniq.size(); }
    int tile_max(const locrec_sg_graph *g) const { return sg_batch_tile_max(g); }
    void rows(const locrec_sg_graph *g, size_t t0, int nb, double alpha, double eps2, std::vector<SlotRange> &pointed,
              SgBatchBegin &b, SgBatchReq &rq) const
    {
        sg_batch_tile_rows(g, uniq, t0, nb, alpha, eps2, pointed, b, rq);
    }
    void set_up(const locrec_sg_graph *, hipStream_t, size_t) const {}  // (launches behind the tile's sg_begin_batch: none)
    void polled() const {}                                              // (a convergence word was read: SgBatchCtx counts it)
    void finalize(const locrec_sg_graph *g, hipStream_t s, const SgBatchReq &rq, const double *x_in, double *x_out,
                  const double *parts_prev, double *parts_out, SgBatchState *bstate, int32_t first) const
    {
        hipLaunchKernelGGL(sg_finalize_batch, dim3(kParts), dim3(256), 0, s, rq, g->n_short, g->lrows.p, g->nlrows, g->n_crows,
                           g->XL.p, x_in, x_out, parts_prev, parts_out, bstate, first);
    }
};

// Every tile of the batch's columns: its set-up, its rounds and polls, then consume(ctx, t0, nb) - after the tile's last
// round and before the next tile's set-up overwrites x.  At the end the last tile's slots go back to D.
template <class Tiles, class Consume>
int32_t sg_batch_tiles_of(locrec_sg_graph *g, Tiles &&tiles, double alpha, double epsilon, int64_t max_iterations,
                          SgBatchCtx &ctx, Consume &&consume)
{
    if (max_iterations > INT32_MAX) max_iterations = INT32_MAX;
    LOCREC_HIP_TRY(hipSetDevice(g->device));
    hipStream_t s = g->stream;
    const int32_t T = g->nlive;
    const int64_t xstride = sg_batch_xstride(g);
    const int tile_max = tiles.tile_max(g);
    LOCREC_TRY(sg_batch_buffers(g, s));
    SgBatchState *bstate = reinterpret_cast<SgBatchState *>(g->fused_conv.p);
    const double eps2 = epsilon * epsilon;  // :40
    const bool poll = epsilon > 0 && max_iterations > 4;
    const bool poll_by_kernel = g->h_poll_dev != nullptr && !g->no_pack;
    const int sweep_blocks = (g->npieces + 3) / 4;
    const void *colv = sg_batch_columns(g);
    const v2d *wv2 = reinterpret_cast<const v2d *>(g->w2.p);
    const v4h *wi = reinterpret_cast<const v4h *>(g->widx.p);
    const size_t lds = g->ndict > 0 ? (size_t)g->ndict * sizeof(double) : 0;
    const size_t nu = tiles.count();
    ctx.s = s;
    ctx.T = T;
    ctx.xstride = xstride;
    ctx.bstate = bstate;
    ctx.eps2 = eps2;
    ctx.max_iterations = max_iterations;
    // slot ranges that point at a private row (or at the single request's Q) and go back to D next
    std::vector<SlotRange> pointed;
    sg_batch_take_patched(g, pointed);

    auto run_tile = [&](size_t t0, int nb) -> int32_t {
        SgBatchBegin b;
        SgBatchReq rq;
        tiles.rows(g, t0, nb, alpha, eps2, pointed, b, rq);
        hipLaunchKernelGGL(sg_begin_batch, dim3(kBeginBlocks), dim3(256), 0, s, b);
        tiles.set_up(g, s, t0);
        // step() (:92-106) for every column; the host looks at "all columns done" on the single request's schedule
        auto launch_round = [&](int64_t i) {
            const int par = (int)(i & 1);
            const double *x_in = g->PA4.p + (size_t)par * xstride;
            double *x_out = g->PA4.p + (size_t)(par ^ 1) * xstride;
            if (sweep_blocks > 0) {
#define LOCREC_SWEEP_BATCH(C16, DICT)                                                                                   \
    hipLaunchKernelGGL((sg_sweep_batch<C16, DICT>), dim3(sweep_blocks), dim3(256), DICT ? lds : 0, s, colv, wv2, wi,    \
                       g->dict.p, g->ndict, g->pinfo.p, g->seg_out.p, x_in, g->XL.p, g->npieces, bstate)
                if (g->use16) {
                    if (g->ndict > 0) LOCREC_SWEEP_BATCH(true, true); else LOCREC_SWEEP_BATCH(true, false);
                } else {
                    if (g->ndict > 0) LOCREC_SWEEP_BATCH(false, true); else LOCREC_SWEEP_BATCH(false, false);
                }
#undef LOCREC_SWEEP_BATCH
            }
            tiles.finalize(g, s, rq, x_in, x_out, g->D2W.p + (size_t)(par ^ 1) * kParts * kBatchB,
                           g->D2W.p + (size_t)par * kParts * kBatchB, bstate, i == 0 ? 1 : 0);
        };
        int64_t next_check = 4;
        for (int64_t i = 0; i < max_iterations;) {
            const int64_t stop = poll ? std::min(max_iterations, next_check) : max_iterations;
            for (int64_t k = i; k < stop; ++k) launch_round(k);
            i = stop;
            if (poll && stop == next_check && stop < max_iterations) {
                int32_t all_done = 0;
                if (poll_by_kernel) {
                    hipLaunchKernelGGL(sg_poll_batch, dim3(1), dim3(64), 0, s, bstate, g->h_poll_dev);
                    LOCREC_HIP_TRY(hipStreamSynchronize(s));
                    all_done = *g->h_poll;
                } else {
                    LOCREC_HIP_TRY(hipMemcpyAsync(&all_done, &bstate->all_done, sizeof all_done, hipMemcpyDeviceToHost, s));
                    LOCREC_HIP_TRY(hipStreamSynchronize(s));
                }
                ++ctx.polls;
                tiles.polled();
                if (all_done) break;
                next_check += next_check < 8 ? 2 : (next_check < 16 ? 4 : kCheckEvery);
            }
        }
        return consume(ctx, t0, nb);
    };
    int32_t status = LOCREC_OK;
    for (size_t t0 = 0; t0 < nu && status == LOCREC_OK; t0 += (size_t)tile_max)
        status = run_tile(t0, (int)std::min<size_t>((size_t)tile_max, nu - t0));
    if (!pointed.empty()) {
        SgBatchBegin b;
        sg_batch_restore_row(g, pointed, b);
        hipLaunchKernelGGL(sg_begin_batch, dim3(kBeginBlocks), dim3(256), 0, s, b);
        LOCREC_HIP_TRY(hipGetLastError());
    }
    return status;
}

// ... of the distinct targets uniq
template <class Consume>
int32_t sg_batch_tiles(locrec_sg_graph *g, const std::vector<int32_t> &uniq, double alpha, double epsilon,
                       int64_t max_iterations, SgBatchCtx &ctx, Consume &&consume)
{
    return sg_batch_tiles_of(g, SgPersonTiles{uniq}, alpha, epsilon, max_iterations, ctx, consume);
}

// ---- the host's side of a tile's read-back: the packed image (the state at 0, the block sums at kBatchPackHead, then
// rows 0 .. T of x, every column from the parity of its last executed sweep), the verdicts and the rows ----

inline size_t sg_batch_pack_bytes(int32_t T) { return kBatchPackHead + (size_t)2 * kParts * kBatchB * 8 + (size_t)(T + 1) * kBatchB * 8; }

inline unsigned sg_batch_pack_blocks(int32_t T) { return (unsigned)std::min<int64_t>(64, ((int64_t)(T + 1) * kBatchB + 2047) / 2048); }

// (no pinned staging, or LOCREC_SG_NO_PACK) the same image from plain copies: enqueued here, assembled by
// sg_batch_copy_assemble once the stream has been synchronised.  dst and both stay where they are until then.
int32_t sg_batch_copy_enqueue(const locrec_sg_graph *g, hipStream_t s, unsigned char *dst, std::vector<double> &both)
{
    const int64_t xstride = sg_batch_xstride(g);
    const size_t nxc = (size_t)(g->nlive + 1) * kBatchB;
    both.resize(2 * nxc);
    LOCREC_HIP_TRY(hipMemcpyAsync(dst, g->fused_conv.p, sizeof(SgBatchState), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(dst + kBatchPackHead, g->D2W.p, (size_t)2 * kParts * kBatchB * sizeof(double),
                                  hipMemcpyDeviceToHost, s));
    for (int par = 0; par < 2; ++par)
        LOCREC_HIP_TRY(hipMemcpyAsync(both.data() + par * nxc, g->PA4.p + (size_t)par * xstride, nxc * sizeof(double),
                                      hipMemcpyDeviceToHost, s));
    return LOCREC_OK;
}

void sg_batch_copy_assemble(int32_t T, unsigned char *dst, const std::vector<double> &both)
{
    const size_t nxc = (size_t)(T + 1) * kBatchB;
    SgBatchState st0;
    std::memcpy(&st0, dst, sizeof st0);
    double *hx0 = reinterpret_cast<double *>(dst + kBatchPackHead) + 2 * kParts * kBatchB;
    for (size_t i = 0; i < nxc; ++i) hx0[i] = both[(size_t)(st0.sweeps[i % kBatchB] & 1) * nxc + i];
}

// What a batch collects per distinct target
struct SgBatchRows {
    std::vector<std::vector<int64_t>> ids;
    std::vector<std::vector<double>> probs;
    std::vector<int64_t> it;
    std::vector<int32_t> conv;
    void resize(size_t nu)
    {
        ids.assign(nu, {});
        probs.assign(nu, {});
        it.assign(nu, 0);
        conv.assign(nu, 0);
    }
};

// The verdicts and rows (:84-88) of the tile uniq[t0 .. t0 + nb) from its packed image
int32_t sg_batch_host_rows(locrec_sg_graph *g, const unsigned char *host, const std::vector<int32_t> &uniq, size_t t0, int nb,
                           double eps2, int64_t max_iterations, SgBatchRows &res)
{
    const int32_t T = g->nlive;
    SgBatchState hs;
    std::memcpy(&hs, host, sizeof hs);
    const double *hparts = reinterpret_cast<const double *>(host + kBatchPackHead);
    const double *hx = hparts + 2 * kParts * kBatchB;
    if (g->live_sorted.size() != (size_t)T) {
        g->live_sorted.clear();
        for (int64_t v = 0; v < g->nv; ++v)
            if (g->live_of[v] >= 0) g->live_sorted.push_back((int32_t)v);
    }
    // step(), :92-106: which of the two exits each column took (as locrec_sg_fetch decides it)
    for (int j = 0; j < nb; ++j) {
        const size_t u = t0 + (size_t)j;
        const int64_t sweeps = hs.sweeps[j];
        auto total = [&]() {
            double parts[kParts];
            for (int q = 0; q < kParts; ++q) parts[q] = hparts[(size_t)((sweeps - 1) & 1) * kParts * kBatchB + (size_t)q * kBatchB + j];
            return host_total_d2(parts);
        };
        LOCREC_TRY(sg_batch_verdict(sweeps, total, eps2, max_iterations, &res.it[u], &res.conv[u]));
    }
    // :84-88  id != vertexId and probability > 0, ascending id.  A source-only vertex holds D's value: 1/V before the
    // first sweep (then every vertex is walked, column by column), 0 after it (then only the live ones can appear,
    // and one pass over them serves every column: each x row is one contiguous line)
    int swept[kBatchB];
    int nswept = 0;
    for (int j = 0; j < nb; ++j) {
        const size_t u = t0 + (size_t)j;
        const int32_t tv = uniq[u];
        const double xdead = hx[(size_t)T * kBatchB + j];
        if (!(xdead > 0)) {
            swept[nswept++] = j;
            res.ids[u].reserve((size_t)T);
            res.probs[u].reserve((size_t)T);
            continue;
        }
        for (int64_t v = 0; v < g->nv; ++v) {
            const int32_t l = g->live_of[v];
            const double xv = l >= 0 ? hx[(size_t)l * kBatchB + j] : xdead;
            if (v == tv || !(xv > 0)) continue;
            res.ids[u].push_back(g->vid[v]);
            res.probs[u].push_back(xv);
        }
    }
    if (nswept > 0) {
        for (const int32_t v : g->live_sorted) {
            const double *row = hx + (size_t)g->live_of[v] * kBatchB;
            for (int k = 0; k < nswept; ++k) {
                const int j = swept[k];
                const size_t u = t0 + (size_t)j;
                if (v == uniq[u] || !(row[j] > 0)) continue;
                res.ids[u].push_back(g->vid[v]);
                res.probs[u].push_back(row[j]);
            }
        }
    }
    return LOCREC_OK;
}

// One request's share of what a batch collected
struct SgBatchRowRef {
    const SgBatchRows *res;
    size_t u;
};

// The rows in input order (a repeated target's rows are copies) under the capacity protocol: offsets and counters always,
// *inout_capacity = the need, the rows when the room suffices.  at(i) -> request i's SgBatchRowRef.
template <class At>
int32_t sg_batch_output(int64_t n_targets, At &&at, int64_t *out_offsets, int64_t *out_ids, double *out_probs,
                        int64_t *inout_capacity, int64_t *out_iterations, int32_t *out_converged)
{
    int64_t total = 0;
    out_offsets[0] = 0;
    for (int64_t i = 0; i < n_targets; ++i) {
        const SgBatchRowRef r = at(i);
        total += (int64_t)r.res->ids[r.u].size();
        out_offsets[i + 1] = total;
        if (out_iterations) out_iterations[i] = r.res->it[r.u];
        if (out_converged) out_converged[i] = r.res->conv[r.u];
    }
    const int64_t cap = *inout_capacity;
    *inout_capacity = total;
    if (total > cap || total == 0) return LOCREC_OK;
    if (!out_ids || !out_probs) return fail(LOCREC_E_INVALID_ARG, "NULL output buffer");
    for (int64_t i = 0; i < n_targets; ++i) {
        const SgBatchRowRef r = at(i);
        std::copy(r.res->ids[r.u].begin(), r.res->ids[r.u].end(), out_ids + out_offsets[i]);
        std::copy(r.res->probs[r.u].begin(), r.res->probs[r.u].end(), out_probs + out_offsets[i]);
    }
    return LOCREC_OK;
}

// A tile's read-back for the unranked entries: one pack launch into pinned memory, then the rows of every column (:84-88)
int32_t sg_batch_read_back(locrec_sg_graph *g, SgBatchCtx &ctx, const std::vector<int32_t> &uniq, size_t t0, int nb, SgBatchRows &res)
{
    hipStream_t s = ctx.s;
    const int32_t T = ctx.T;
    const size_t pack_bytes = sg_batch_pack_bytes(T);
    unsigned char *stg = g->no_pack ? nullptr : g->stage(pack_bytes);
    void *stg_dev = nullptr;
    std::vector<unsigned char> own;
    const unsigned char *host = nullptr;
    if (stg && hipHostGetDevicePointer(&stg_dev, stg, 0) == hipSuccess) {
        hipLaunchKernelGGL(sg_pack_batch, dim3(sg_batch_pack_blocks(T)), dim3(256), 0, s, ctx.bstate, g->D2W.p, g->PA4.p,
                           ctx.xstride, T + 1, static_cast<unsigned char *>(stg_dev));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        host = stg;
    } else {
        (void)hipGetLastError();
        own.resize(pack_bytes);
        std::vector<double> both;
        LOCREC_TRY(sg_batch_copy_enqueue(g, s, own.data(), both));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        sg_batch_copy_assemble(T, own.data(), both);
        host = own.data();
    }
    LOCREC_HIP_TRY(hipGetLastError());
    return sg_batch_host_rows(g, host, uniq, t0, nb, ctx.eps2, ctx.max_iterations, res);
}

}  // namespace

extern "C" int32_t locrec_sg_recommend_batch(locrec_sg_graph *g, int64_t n_targets, const int64_t *vertex_ids, double alpha,
                                             double epsilon, int64_t max_iterations, int64_t *out_offsets, int64_t *out_ids,
                                             double *out_probs, int64_t *inout_capacity, int64_t *out_iterations,
                                             int32_t *out_converged) try
{
    if (!g) return fail(LOCREC_E_INVALID_ARG, "graph is NULL");
    if (n_targets < 0 || (n_targets > 0 && !vertex_ids) || !out_offsets || !inout_capacity)
        return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    std::vector<int32_t> uniq, uniq_of;
    LOCREC_TRY(sg_batch_targets(g, n_targets, vertex_ids, epsilon, max_iterations, uniq, uniq_of));
    if (n_targets == 0) {
        out_offsets[0] = 0;
        *inout_capacity = 0;
        return LOCREC_OK;
    }
    SgBatchRows res;
    res.resize(uniq.size());
    auto read_back = [&](SgBatchCtx &ctx, size_t t0, int nb) -> int32_t { return sg_batch_read_back(g, ctx, uniq, t0, nb, res); };
    SgBatchCtx ctx;
    LOCREC_TRY(sg_batch_tiles(g, uniq, alpha, epsilon, max_iterations, ctx, read_back));
    return sg_batch_output(n_targets, [&](int64_t i) { return SgBatchRowRef{&res, (size_t)uniq_of[(size_t)i]}; }, out_offsets,
                           out_ids, out_probs, inout_capacity, out_iterations, out_converged);
} LOCREC_CATCH_ALL

#include "sg_ranked.h"
#include "sg_pool.h"
#include "sg_pool_ranked.h"
#include "sg_visitors.h"
#include "sg_pool_visitors.h"
