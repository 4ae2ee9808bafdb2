// knn_visitors.h -- KNN for visitors: rating vectors that are no rows of the index (locrec_knn_visitors_*,
// knn_visitors_api.h).  Included at the end of knn_large.hip: the kernels and the tile drivers over the handle's
// visitor state (knn_index.h: KnnVisitorSide; knn_visitors_side.h).
//
// For a visitor v and an index built from the persons P every result equals what the person calls return for v on an
// index built from P + {v}: v is a candidate of nobody, nobody is left out as "self", v has no rating rows.  The path is
// the dense-table tile scan of this file with another front:
//
//   lkv_stage     one thread per (visitor, family) walks the vector once: the checks a row gets at create time
//                 (kb_validate) -> one report word, the first refusal; place indices through the index's popularity
//                 renumbering (the identity where it has none); entries at an index beyond the index's dimensions - the
//                 reference's builder would have given every vector the larger size - enter the vector's length and no
//                 dot product: they are squeezed out of the staged vector and counted; the fp64 vector length with
//                 kb_norms' arithmetic (left fold of squares in the given order, sqrt).  The staged vector lies where the
//                 input lies, its bounds two words a visitor, so that lkb_fill reads it as a CSR row; its indices are
//                 not re-sorted: the fill is a scatter.  The walk is serial: right for visitors of a few hundred
//                 entries (the measured shapes: about 100), where the stage is a few microseconds of a call; a batch of
//                 few visitors near the 2^21-entry limit makes it the serial tail of the call - a wave per vector (a
//                 segmented scan for the kept positions and the left fold) is not built
//   lkb_fill     as it stands, on the staged vectors (set, and the wipe after the scan)
//   lkv_scan      lkb_scan_body's loop (bitmap in LDS, dense tables, lkb_similarity) with the queries' norms from the
//                 stage and without the self-exclusion; S row-major or transposed, the candidate counters kept
//   then          K >= n: the row-major tile straight into lkb_aggregate_tile; any smaller K, from 1: lkt_topk_tile, then
//                 lkt_emit (neighbour lists) or lkt_mask_rows and lkb_aggregate_tile - with K_eff = min(K, n)
//
// Bits: a candidate's dots are summed over ITS row in ascending stored index order against the dense tables, as for a
// person's query.  On an index that renumbers its place dimensions the place values are integers (the stage refuses a
// visitor with any other place value, or one of 65536 or more: the squares of 2^21 such entries still add up exactly),
// so every place sum is exact in any order; the categories are never renumbered, and without the renumbering the
// places' order is BLAS.dot's too: any finite value stays bit-exact there.
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950: VGPRs / LDS bytes (static) / scratch / occupancy (waves per SIMD)
//   lkv_stage    26 /  0 / 0 / 8
//   lkv_scan    112 / 64 / 0 / 4   (+ the bitmap, dynamic: at most 32 KB) - lkb_scan's figures
// (unchanged with their bodies as functions - lkv_stage_body, lkv_scan_body - which the pool's kernels call too:
// knn_pool_visitors.h)

#include "knn_visitors_side.h"

namespace {

enum {
    kVisErrPtr = 1, kVisErrLong, kVisErrEmpty, kVisErrNegative, kVisErrOrder, kVisErrFinite, kVisErrFraction, kVisErrZero
};

struct LkvStage {
    int64_t nv;
    const int64_t *ptr[2];     // family 0 = places, 1 = categories
    const int32_t *idx[2];
    const double *val[2];
    int64_t total[2];          // entries of the family's element arrays
    int32_t dim[2];
    const int32_t *new_of_old; // of the place family, or null; given: a place value must be an integer below 65536
    int64_t *bounds[2];
    int32_t *out_idx[2];
    double *out_val[2];
    double *norm[2];
    int32_t *lens;             // [2][nv]
    unsigned long long *report;  // [0] min over refusals of visitor << 8 | family << 4 | code; [1] entries beyond the dimensions
};

// family f of visitor v against an index of `dim` dimensions in that family; map: the renumbering of the family, or null
__device__ __forceinline__ void lkv_stage_body(const LkvStage &a, int64_t v, int f, int32_t dim, const int32_t *map)
{
    const int64_t b = a.ptr[f][v], e = a.ptr[f][v + 1];
    unsigned code = 0;
    int32_t kept = 0, beyond = 0;
    double sum = 0.0;
    if (b < 0 || e < b || e > a.total[f]) {
        code = kVisErrPtr;  // (nothing is read through such a row)
    } else if (e - b >= (1 << 21)) {
        code = kVisErrLong;
    } else if (e == b) {
        code = kVisErrEmpty;
    } else {
        int32_t prev = -1;
        for (int64_t i = b; i < e && !code; ++i) {
            const int32_t ix = a.idx[f][i];
            const double x = a.val[f][i];
            if (ix < 0) code = kVisErrNegative;
            else if (i > b && ix <= prev) code = kVisErrOrder;
            else if (!isfinite(x)) code = kVisErrFinite;
            else if (map && (x != floor(x) || !(fabs(x) < 65536.0))) code = kVisErrFraction;  // (renumbered places only)
            if (code) break;
            prev = ix;
            const double sq = x * x;  // Distance.vectorLength (Distance.scala:11-16), as kb_norms
            sum = sum + sq;
            if (ix >= dim) {
                ++beyond;
            } else {
                a.out_idx[f][b + kept] = map ? map[ix] : ix;
                a.out_val[f][b + kept] = x;
                ++kept;
            }
        }
        if (!code && !(sum > 0)) code = kVisErrZero;
    }
    if (code) atomicMin(&a.report[0], ((unsigned long long)v << 8) | ((unsigned long long)f << 4) | code);
    if (beyond) atomicAdd(&a.report[1], (unsigned long long)beyond);
    a.bounds[f][2 * v] = b;
    a.bounds[f][2 * v + 1] = b + kept;
    a.lens[(int64_t)f * a.nv + v] = kept;
    a.norm[f][v] = sqrt(sum);
}

// grid (visitor blocks, 2 families)
__global__ __launch_bounds__(256) void lkv_stage(const LkvStage a)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y;
    if (v >= a.nv) return;
    lkv_stage_body(a, v, f, a.dim[f], f == 0 ? a.new_of_old : nullptr);
}

struct LkvScan {
    LkbScan P;                    // (its qrow is not read)
    const double *vnorm_p, *vnorm_c;  // the vector lengths of the tile's visitors: slot t's at [t]
    int32_t nt;                   // visitors in the tile
};

// row block bx of the tile P: lkb_scan_body with the queries' norms from the stage; every row is a candidate.  kByStage
// false: slot t's norms at [t], nt slots; true (the pool's form, knn_pool_visitors.h): slot t's norms at [P.qrow[t]], the
// visitor's position in the stage (a wave-uniform load), -1: no visitor in the slot
template <bool kByStage>
__device__ __forceinline__ void lkv_scan_body(const LkbScan &P, int32_t *cand, const double *vnorm_p, const double *vnorm_c, int nt,
                                              int bx)
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
            if (!((s_bits[b >> 5] >> (b & 31u)) & 1u)) continue;  // no visitor of the tile holds this place
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
            double sx = 0.0;
            bool have = false;
            if (kByStage) {
                const int32_t v = P.qrow[t];
                if (v >= 0) have = lkb_similarity(dp[t], dc[t], cnp, cnc, vnorm_p[v], vnorm_c[v], P.pw, P.cw, sx);
            } else {
                if (t < nt) have = lkb_similarity(dp[t], dc[t], cnp, cnc, vnorm_p[t], vnorm_c[t], P.pw, P.cw, sx);
            }
            if (!have) sx = 0.0;
            P.S[P.transposed ? (int64_t)t * P.nrows + row : (int64_t)row * kLkbQt + t] = sx;
            if (have) atomicAdd(&s_cand[t], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < kLkbQt && s_cand[threadIdx.x]) atomicAdd(&cand[threadIdx.x], s_cand[threadIdx.x]);
}

// grid (row blocks of the tile)
__global__ __launch_bounds__(256) void lkv_scan(const LkvScan V)
{
    lkv_scan_body<false>(V.P, V.P.cand, V.vnorm_p, V.vnorm_c, V.nt, (int)blockIdx.x);
}

int32_t lkv_device_array(const void *p, int device, const char *what)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return locrec::fail(LOCREC_E_INVALID_ARG, "%s is not a device array", what);
    }
    if ((a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) || a.device != device)
        return locrec::fail(LOCREC_E_INVALID_ARG, "%s does not live on the index's device", what);
    return LOCREC_OK;
}

}  // namespace

namespace locrec {

KnnVisitorsStats &knn_visitors_stats()
{
    thread_local KnnVisitorsStats st;
    return st;
}

// the refusal the stage's report word stands for (lkv_stage, lkv_stage_pool): *bad = the visitor, the family's message
static int32_t lkv_refuse(unsigned long long word, int64_t *bad)
{
    const char *const fam[2] = {"place", "category"};
    const long long who = (long long)(word >> 8);
    const char *name = fam[(word >> 4) & 1];
    if (bad) *bad = who;
    switch ((int)(word & 0xF)) {
    case kVisErrPtr: return fail(LOCREC_E_INVALID_ARG, "%s rowptr not monotone at visitor %lld", name, who);
    case kVisErrLong: return fail(LOCREC_E_INVALID_ARG, "%s vector of visitor %lld has 2^21 or more entries", name, who);
    case kVisErrEmpty: return fail(LOCREC_E_NOT_FOUND, "No such person: visitor %lld has no %s vector", who, name);
    case kVisErrNegative: return fail(LOCREC_E_INVALID_ARG, "%s index of visitor %lld is negative", name, who);
    case kVisErrOrder: return fail(LOCREC_E_INVALID_ARG, "%s indices of visitor %lld not strictly ascending", name, who);
    case kVisErrFinite: return fail(LOCREC_E_INVALID_ARG, "%s value of visitor %lld is not finite", name, who);
    case kVisErrFraction:
        return fail(LOCREC_E_INVALID_ARG,
                    "%s value of visitor %lld is not an integer count below 65536: the index renumbers its place dimensions",
                    name, who);
    default: return fail(LOCREC_E_INVALID_ARG, "%s vector of visitor %lld has zero norm", name, who);
    }
}

int32_t knn_visitors_stage(locrec_knn_index *ix, KnnVisitorSide &side, const KnnVisitorVectors &v, int64_t *bad)
{
    hipStream_t s = ix->stream;
    KnnVisitorsStats &st = knn_visitors_stats();
    const int64_t nv = v.nv;
    const bool on_device = v.mem == LOCREC_MEM_DEVICE;
    const char *const fam[2] = {"place", "category"};
    const int64_t *in_ptr[2] = {v.p_ptr, v.c_ptr};
    const int32_t *in_idx[2] = {v.p_idx, v.c_idx};
    const double *in_val[2] = {v.p_val, v.c_val};
    int64_t total[2] = {0, 0};
    // the row pointers decide how much is read: their ends first (a device array's: one small copy)
    if (on_device) {
        LOCREC_TRY(lkv_device_array(v.p_ptr, ix->device, "place rowptr"));
        LOCREC_TRY(lkv_device_array(v.c_ptr, ix->device, "category rowptr"));
        int64_t ends[4] = {0, 0, 0, 0};
        for (int f = 0; f < 2; ++f) {
            LOCREC_HIP_TRY(hipMemcpyAsync(&ends[2 * f], in_ptr[f], 8, hipMemcpyDeviceToHost, s));
            LOCREC_HIP_TRY(hipMemcpyAsync(&ends[2 * f + 1], in_ptr[f] + nv, 8, hipMemcpyDeviceToHost, s));
        }
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        ++st.host_syncs;
        for (int f = 0; f < 2; ++f) {
            if (ends[2 * f] != 0) return fail(LOCREC_E_INVALID_ARG, "%s rowptr must start at 0", fam[f]);
            total[f] = ends[2 * f + 1];
        }
    } else {
        for (int f = 0; f < 2; ++f) {
            if (in_ptr[f][0] != 0) return fail(LOCREC_E_INVALID_ARG, "%s rowptr must start at 0", fam[f]);
            total[f] = in_ptr[f][nv];
        }
        // (the first visitor whose row pointers turn back is found on the host: nothing is uploaded past the end)
        for (int64_t i = 0; i < nv; ++i)
            for (int f = 0; f < 2; ++f)
                if (in_ptr[f][i + 1] < in_ptr[f][i] || in_ptr[f][i + 1] > total[f]) {
                    if (bad) *bad = i;
                    return fail(LOCREC_E_INVALID_ARG, "%s rowptr not monotone at visitor %lld", fam[f], (long long)i);
                }
    }
    for (int f = 0; f < 2; ++f) {
        if (total[f] < 0 || total[f] >= ((int64_t)1 << 31))
            return fail(LOCREC_E_INVALID_ARG, "%s element count out of range [0, 2^31)", fam[f]);
        if (total[f] > 0 && (!in_idx[f] || !in_val[f])) return fail(LOCREC_E_INVALID_ARG, "NULL %s array", fam[f]);
        if (on_device && total[f] > 0) {
            LOCREC_TRY(lkv_device_array(in_idx[f], ix->device, f == 0 ? "place indices" : "category indices"));
            LOCREC_TRY(lkv_device_array(in_val[f], ix->device, f == 0 ? "place values" : "category values"));
        }
    }
    const KnnVisitorsStageSizes sz = knn_visitors_stage_sizes(nv, total[0], total[1]);
    if (!on_device) {
        LOCREC_TRY(side.in_ptr_p.reserve((size_t)nv + 1));
        LOCREC_TRY(side.in_ptr_c.reserve((size_t)nv + 1));
        LOCREC_TRY(side.in_idx_p.reserve(sz.p_elems));
        LOCREC_TRY(side.in_val_p.reserve(sz.p_elems));
        LOCREC_TRY(side.in_idx_c.reserve(sz.c_elems));
        LOCREC_TRY(side.in_val_c.reserve(sz.c_elems));
        int64_t *d_ptr[2] = {side.in_ptr_p.p, side.in_ptr_c.p};
        int32_t *d_idx[2] = {side.in_idx_p.p, side.in_idx_c.p};
        double *d_val[2] = {side.in_val_p.p, side.in_val_c.p};
        for (int f = 0; f < 2; ++f) {
            LOCREC_HIP_TRY(hipMemcpyAsync(d_ptr[f], in_ptr[f], ((size_t)nv + 1) * 8, hipMemcpyHostToDevice, s));
            if (total[f] > 0) {
                LOCREC_HIP_TRY(hipMemcpyAsync(d_idx[f], in_idx[f], (size_t)total[f] * 4, hipMemcpyHostToDevice, s));
                LOCREC_HIP_TRY(hipMemcpyAsync(d_val[f], in_val[f], (size_t)total[f] * 8, hipMemcpyHostToDevice, s));
            }
            in_ptr[f] = d_ptr[f];
            in_idx[f] = d_idx[f];
            in_val[f] = d_val[f];
        }
    }
    LOCREC_TRY(side.bounds_p.reserve(sz.bounds));
    LOCREC_TRY(side.bounds_c.reserve(sz.bounds));
    LOCREC_TRY(side.idx_p.reserve(sz.p_elems));
    LOCREC_TRY(side.val_p.reserve(sz.p_elems));
    LOCREC_TRY(side.idx_c.reserve(sz.c_elems));
    LOCREC_TRY(side.val_c.reserve(sz.c_elems));
    LOCREC_TRY(side.norm_p.reserve(sz.norms));
    LOCREC_TRY(side.norm_c.reserve(sz.norms));
    LOCREC_TRY(side.lens.reserve(sz.lens));
    LOCREC_TRY(side.report.reserve(2));
    unsigned long long report[2] = {~0ull, 0ull};
    LOCREC_HIP_TRY(hipMemcpyAsync(side.report.p, report, sizeof report, hipMemcpyHostToDevice, s));
    LkvStage a{};
    a.nv = nv;
    for (int f = 0; f < 2; ++f) {
        a.ptr[f] = in_ptr[f];
        a.idx[f] = in_idx[f];
        a.val[f] = in_val[f];
        a.total[f] = total[f];
    }
    a.dim[0] = ix->fp.dim;
    a.dim[1] = ix->fc.dim;
    a.new_of_old = side.new_of_old.p;
    a.bounds[0] = side.bounds_p.p; a.bounds[1] = side.bounds_c.p;
    a.out_idx[0] = side.idx_p.p; a.out_idx[1] = side.idx_c.p;
    a.out_val[0] = side.val_p.p; a.out_val[1] = side.val_c.p;
    a.norm[0] = side.norm_p.p; a.norm[1] = side.norm_c.p;
    a.lens = side.lens.p;
    a.report = side.report.p;
    hipLaunchKernelGGL(lkv_stage, dim3((unsigned)((nv + 255) / 256), 2), dim3(256), 0, s, a);
    LOCREC_HIP_TRY(hipGetLastError());
    ++st.stage_launches;
    side.h_lens.resize(sz.lens);
    LOCREC_HIP_TRY(hipMemcpyAsync(report, side.report.p, sizeof report, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(side.h_lens.data(), side.lens.p, sz.lens * 4, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    ++st.host_syncs;
    st.renumbered = side.renumbered() ? 1 : 0;
    if (report[0] != ~0ull) return lkv_refuse(report[0], bad);
    st.beyond = (int64_t)report[1];
    return LOCREC_OK;
}

// One tile of the visitor scan: the similarities of the staged visitors [v0, v0 + nt) against every row -> ix->lkb_S,
// [row][kLkbQt] or transposed; lkb_scan_tile with the fill reading the stage and lkv_scan in lkb_scan's place
static int32_t lkv_scan_tile(locrec_knn_index *ix, KnnVisitorSide &side, int64_t v0, int nt, double pw, double cw, bool transposed)
{
    hipStream_t s = ix->stream;
    KnnVisitorsStats &st = knn_visitors_stats();
    const int64_t nv_staged = (int64_t)side.h_lens.size() / 2;
    LkvScan V{};
    LkbScan &P = V.P;
    LkbFill fp{}, fc{};
    for (int t = 0; t < kLkbQt; ++t) P.qrow[t] = fp.qrow[t] = fc.qrow[t] = t < nt ? knn_visitors_stage_row(v0 + t) : -1;
    fp.ptr = side.bounds_p.p; fp.idx = side.idx_p.p; fp.val = side.val_p.p; fp.qd = ix->lkb_qd_p.p;
    lkb_bitmap_of(ix, &fp.bits, &fp.bit_mask);
    fc.ptr = side.bounds_c.p; fc.idx = side.idx_c.p; fc.val = side.val_c.p; fc.qd = ix->lkb_qd_c.p;
    P.bits = fp.bits;
    P.bit_mask = fp.bit_mask;
    P.p_ptr = ix->fp.csr_ptr.p; P.p_idx = ix->fp.csr_idx.p; P.p_val = ix->fp.csr_val.p;
    P.c_ptr = ix->fc.csr_ptr.p; P.c_idx = ix->fc.csr_idx.p; P.c_val = ix->fc.csr_val.p;
    P.norm_p = ix->fp.norm.p; P.norm_c = ix->fc.norm.p;
    P.qd_p = ix->lkb_qd_p.p; P.qd_c = ix->lkb_qd_c.p;
    P.nrows = (int32_t)ix->n;
    P.pw = pw; P.cw = cw;
    P.S = ix->lkb_S.p;
    P.cand = ix->lkb_cand.p;
    P.transposed = transposed ? 1 : 0;
    V.vnorm_p = side.norm_p.p + v0;
    V.vnorm_c = side.norm_c.p + v0;
    V.nt = nt;
    const dim3 gp(knn_visitors_fill_blocks(side.h_lens.data(), v0, nt), kLkbQt);
    const dim3 gc(knn_visitors_fill_blocks(side.h_lens.data() + nv_staged, v0, nt), kLkbQt);
    fp.set = fc.set = 1;
    hipLaunchKernelGGL(lkb_fill, gp, dim3(256), 0, s, fp);
    hipLaunchKernelGGL(lkb_fill, gc, dim3(256), 0, s, fc);
    LOCREC_HIP_TRY(hipMemsetAsync(ix->lkb_cand.p, 0, kLkbQt * sizeof(int32_t), s));
    const dim3 grid((unsigned)((P.nrows + 255) / 256));
    const size_t lds = (P.bit_mask + 1u) / 8u;
    LOCREC_LAUNCH_PROFILED(ix->prof, lkv_scan, grid, dim3(256), lds, s, V);
    ++st.scan_launches;
    fp.set = fc.set = 0;  // the dense tables go back to all zero for the next tile
    hipLaunchKernelGGL(lkb_fill, gp, dim3(256), 0, s, fp);
    hipLaunchKernelGGL(lkb_fill, gc, dim3(256), 0, s, fc);
    LOCREC_HIP_TRY(hipGetLastError());
    return LOCREC_OK;
}

int32_t knn_visitors_topk(locrec_knn_index *ix, KnnVisitorSide &side, int64_t v0, int64_t nv, double pw, double cw, int64_t k)
{
    hipStream_t s = ix->stream;
    KnnVisitorsStats &st = knn_visitors_stats();
    const int64_t keff = knn_visitors_keff(k, ix->n);
    LOCREC_TRY(ix->out_ids.reserve((size_t)(nv * k)));
    LOCREC_TRY(ix->out_sims.reserve((size_t)(nv * k)));
    LOCREC_TRY(ix->out_rows.reserve((size_t)(nv * k)));
    LOCREC_TRY(ix->out_cnt.reserve((size_t)nv));
    LOCREC_TRY(lkt_tile_workspaces(ix));
    LOCREC_TRY(lkb_scan_workspaces(ix));
    for (int64_t q0 = 0; q0 < nv; q0 += kLkbQt) {
        const int nt = (int)std::min<int64_t>(kLkbQt, nv - q0);
        LOCREC_TRY(lkv_scan_tile(ix, side, v0 + q0, nt, pw, cw, true));
        LktTile T{};
        const uint64_t *keys = nullptr;
        const uint32_t *vals = nullptr;
        LOCREC_TRY(lkt_topk_tile(ix, nt, keff, T, &keys, &vals));
        ++st.host_syncs;
        for (int t = 0; t < kLkbQt; ++t) T.slot[t] = t < nt ? q0 + t : -1;
        hipLaunchKernelGGL(lkt_emit, dim3((unsigned)((k + 255) / 256), (unsigned)nt), dim3(256), 0, s, T, k, keys, vals,
                           ix->ids_by_rank.p, ix->row_of_rid.p, ix->out_ids.p, ix->out_sims.p, ix->out_rows.p, ix->out_cnt.p);
        LOCREC_HIP_TRY(hipGetLastError());
        ++st.tiles;
        ++st.tiles_topk;
    }
    return LOCREC_OK;
}

int32_t knn_visitors_recommend(locrec_knn_index *ix, KnnVisitorSide &side, int64_t nv, double pw, double cw, int64_t k)
{
    hipStream_t s = ix->stream;
    KnnVisitorsStats &st = knn_visitors_stats();
    const int32_t n = (int32_t)ix->n;
    const int32_t np = (int32_t)ix->cplace_ids.size();
    const bool all = knn_visitors_all(k, ix->n);
    const int64_t keff = knn_visitors_keff(k, ix->n);
    ix->lkb_off.assign((size_t)nv + 1, 0);
    const int tiles = std::max(1, (np + kFinishTile - 1) / kFinishTile);
    LOCREC_TRY(lkb_reserve(ix, tiles));
    if (!all) {
        // lkb_S: the transposed tile of the scan, then the masked row-major tile of the aggregation behind it
        LOCREC_TRY(ix->lkb_S.reserve((size_t)n * kLkbQt * 2));
        LOCREC_TRY(lkt_tile_workspaces(ix));
    }
    std::vector<int32_t> tc((size_t)tiles * kLkbQt);
    int64_t total = 0;
    for (int64_t q0 = 0; q0 < nv; q0 += kLkbQt) {
        const int nt = (int)std::min<int64_t>(kLkbQt, nv - q0);
        int32_t live[kLkbQt];  // (what lkb_aggregate_tile asks of a slot: does it hold a query)
        for (int t = 0; t < kLkbQt; ++t) live[t] = t < nt ? 0 : -1;
        const double *S = ix->lkb_S.p;
        LOCREC_TRY(lkv_scan_tile(ix, side, q0, nt, pw, cw, !all));
        if (!all) {
            LktTile T{};
            const uint64_t *keys = nullptr;
            const uint32_t *vals = nullptr;
            LOCREC_TRY(lkt_topk_tile(ix, nt, keff, T, &keys, &vals));
            ++st.host_syncs;
            double *SR = ix->lkb_S.p + (size_t)n * kLkbQt;
            hipLaunchKernelGGL(lkt_mask_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ix->lkb_S.p, n, ix->rid.p, T, keff,
                               keys, vals, SR);
            LOCREC_HIP_TRY(hipGetLastError());
            S = SR;
        }
        LOCREC_TRY(lkb_aggregate_tile(ix, S, live, q0, nt, tiles, tc, total));
        if (np > 0) ++st.host_syncs;
        ++st.tiles;
        ++(all ? st.tiles_all : st.tiles_topk);
    }
    ix->lkb_off[(size_t)nv] = total;
    return LOCREC_OK;
}

}  // namespace locrec
