// sg_create_device.hip -- locrec_sg_create_from_device: the layout of an unsharded locrec_sg_graph built by kernels from
// an edge list that already lives in device memory (the SG counterpart of locrec_knn_create_from_device).
//
// This file is the SG translation unit: it includes sg_batch.hip whole (which includes sg.hip whole), so it sees the
// handle and its constants.  The contract is that both builders leave the SAME handle, element for element (DESIGN.md
// 4, "Device build"; tests/test_gpu_sg_device_build.py compares them).  They share every layout rule (sg_layout_plan.h)
// and what happens to the handle once columns and weights are resident: the poll word, the weight dictionary and the
// closing figures are sg_build_shared.h's, called from here and from the host build (sg_host_build.h).
//
// The host side is sg_create_device_impl at the end: named phases over one Build, in the order they run.  What the host
// decides or computes about the layout - the plan from the scan's totals with its two refusals, the id-table and
// 16-bit-column rules, radix bits, byte figures, persist_pw - is sg_layout_plan.h's (plain C++, checked stand-alone by
// tests/host/sg_layout_plan_check.cpp against a row-by-row walk of the layout); no phase keeps an expression of its own
// for any of it, and the kernels take their three per-row rules from the same header.
//
// Nothing here takes a position from an atomic: every position is a stable radix sort's or a scan's, so the layout does
// not depend on scheduling.  The only atomics are the integer min / max of the id range.

#include "sg_batch.hip"

#include "offline.h"
#include "sg_layout_plan.h"

namespace {

constexpr int kDbThreads = 256;

__device__ __forceinline__ unsigned long long db_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long db_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// per-row counters scanned together: c[0..6] = rows of remainder class 0..6 so far, c[7] = full pieces so far
struct DbCnt {
    int32_t c[8];
};
struct DbCntPlus {
    __host__ __device__ DbCnt operator()(const DbCnt &a, const DbCnt &b) const
    {
        DbCnt r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r.c[i] = a.c[i] + b.c[i];
        return r;
    }
};

// what the row, piece and edge kernels need of the plan (SgLayoutPlan's 32-bit part)
struct DbPlan {
    int32_t piece_begin[7], part_begin[7];
    int32_t nfull_total, T, n_short;
    int32_t long_base;  // sg_long_begin
};

// ---- vertex ranking ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kDbThreads) void sg_db_minmax(int64_t ne, const int64_t *src, const int64_t *dst,
                                                           unsigned long long *lohi)
{
    __shared__ unsigned long long slo[kDbThreads], shi[kDbThreads];
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int64_t e = (int64_t)blockIdx.x * kDbThreads + threadIdx.x; e < ne; e += (int64_t)gridDim.x * kDbThreads) {
        const unsigned long long a = ordered_key(src[e]), b = ordered_key(dst[e]);
        lo = db_min(lo, db_min(a, b));
        hi = db_max(hi, db_max(a, b));
    }
    slo[threadIdx.x] = lo;
    shi[threadIdx.x] = hi;
    __syncthreads();
    for (int st = kDbThreads / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            slo[threadIdx.x] = db_min(slo[threadIdx.x], slo[threadIdx.x + st]);
            shi[threadIdx.x] = db_max(shi[threadIdx.x], shi[threadIdx.x + st]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMin(&lohi[0], slo[0]);
        atomicMax(&lohi[1], shi[0]);
    }
}

// table path: mark[id - lo] = 1 (every writer stores the same value)
__global__ __launch_bounds__(kDbThreads) void sg_db_mark(int64_t ne, const int64_t *src, const int64_t *dst, uint64_t lo,
                                                         int32_t *mark)
{
    const int64_t e = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (e >= ne) return;
    mark[(uint64_t)src[e] - lo] = 1;
    mark[(uint64_t)dst[e] - lo] = 1;
}

// r = exclusive scan of the marks over n + 1 entries (the last mark is 0): id lo + i is a vertex iff r[i + 1] > r[i]
__global__ __launch_bounds__(kDbThreads) void sg_db_dense_vid(int64_t n, const int32_t *r, uint64_t lo, int64_t *vid)
{
    const int64_t i = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (i >= n) return;
    if (r[i + 1] != r[i]) vid[r[i]] = (int64_t)(lo + (uint64_t)i);
}

__global__ __launch_bounds__(kDbThreads) void sg_db_dense_rank(int64_t ne, const int64_t *src, const int64_t *dst, uint64_t lo,
                                                               const int32_t *r, int32_t *cs, uint32_t *ct, uint32_t *eidx)
{
    const int64_t e = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (e >= ne) return;
    cs[e] = r[(uint64_t)src[e] - lo];
    ct[e] = (uint32_t)r[(uint64_t)dst[e] - lo];
    eidx[e] = (uint32_t)e;
}

// sort path
__global__ __launch_bounds__(kDbThreads) void sg_db_interleave(int64_t ne, const int64_t *src, const int64_t *dst, int64_t *ids)
{
    const int64_t e = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (e >= ne) return;
    ids[2 * e] = src[e];
    ids[2 * e + 1] = dst[e];
}

__global__ __launch_bounds__(kDbThreads) void sg_db_bisect(int64_t ne, const int64_t *src, const int64_t *dst, const int64_t *vid,
                                                           int64_t nv, int32_t *cs, uint32_t *ct, uint32_t *eidx)
{
    const int64_t e = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (e >= ne) return;
    cs[e] = (int32_t)lower_bound<int64_t>(vid, 0, nv, src[e]);
    ct[e] = (uint32_t)lower_bound<int64_t>(vid, 0, nv, dst[e]);
    eidx[e] = (uint32_t)e;
}

// ---- rows ----------------------------------------------------------------------------------------------------------

// kt = the target vertex of every edge, stably sorted: [vbeg[v], vend[v]) is vertex v's row in edge-list order
// (both arrays zeroed before: a vertex without inbound edges keeps an empty range)
__global__ __launch_bounds__(kDbThreads) void sg_db_row_bounds(int64_t ne, const uint32_t *kt, int32_t *vbeg, int32_t *vend)
{
    const int64_t i = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (i >= ne) return;
    const uint32_t v = kt[i];
    if (i == 0 || kt[i - 1] != v) vbeg[v] = (int32_t)i;
    if (i == ne - 1 || kt[i + 1] != v) vend[v] = (int32_t)(i + 1);
}

// live flags of both classes in one word: low half = at most two full pieces, high half = more; entry nv is 0
__global__ __launch_bounds__(kDbThreads) void sg_db_live_flags(int64_t nv, const int32_t *vbeg, const int32_t *vend,
                                                               unsigned long long *fl)
{
    const int64_t v = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (v > nv) return;
    unsigned long long f = 0;
    if (v < nv) {
        const int d = vend[v] - vbeg[v];
        if (d > 0) f = sg_in_long_area(d) ? 1ull << 32 : 1ull;
    }
    fl[v] = f;
}

// sc = exclusive scan of the flags
__global__ __launch_bounds__(kDbThreads) void sg_db_live(int64_t nv, const int32_t *vbeg, const int32_t *vend,
                                                         const unsigned long long *sc, int32_t n_short, int32_t *live_of,
                                                         int32_t *live_vertex)
{
    const int64_t v = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (v >= nv) return;
    const int d = vend[v] - vbeg[v];
    int32_t l = -1;
    if (d > 0) {
        l = sg_in_long_area(d) ? n_short + (int32_t)(sc[v] >> 32) : (int32_t)(sc[v] & 0xFFFFFFFFull);
        live_vertex[l] = (int32_t)v;
    }
    live_of[v] = l;
}

__global__ __launch_bounds__(kDbThreads) void sg_db_row_counts(int32_t T, const int32_t *live_vertex, const int32_t *vbeg,
                                                               const int32_t *vend, DbCnt *cnt)
{
    const int32_t l = (int32_t)(blockIdx.x * kDbThreads + threadIdx.x);
    if (l > T) return;
    DbCnt c;
#pragma unroll
    for (int i = 0; i < 8; ++i) c.c[i] = 0;
    if (l < T) {
        const int32_t v = live_vertex[l];
        const int d = vend[v] - vbeg[v];
        const int rem = d % kSlots;
        c.c[7] = d / kSlots;
        if (rem > 0) {
            const int k = sg_remainder_class(rem);
#pragma unroll
            for (int i = 0; i < 7; ++i)
                if (i == k) c.c[i] = 1;
        }
    }
    cnt[l] = c;
}

// per live row: where its full pieces and its remainder segment start (rowinfo = first full piece, absolute slot of
// remainder element 0 or -1), its partial slots (seg_out) and, for a row of the long area, its lrows entry in row order
__global__ __launch_bounds__(kDbThreads) void sg_db_row_maps(DbPlan P, const int32_t *live_vertex, const int32_t *vbeg,
                                                             const int32_t *vend, const DbCnt *sc, int2 *rowinfo, int32_t *seg_out,
                                                             int4 *lrows_in_order, int32_t *crow)
{
    const int32_t l = (int32_t)(blockIdx.x * kDbThreads + threadIdx.x);
    if (l >= P.T) return;
    const int32_t v = live_vertex[l];
    const int d = vend[v] - vbeg[v];
    const int nfull = d / kSlots, rem = d % kSlots;
    const DbCnt s = sc[l];
    const int32_t full_begin = s.c[7];
    int32_t rem_part = -1, rem_slot0 = -1;
    if (rem > 0) {
        const int c = sg_remainder_class(rem);
        int32_t k = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i)
            if (i == c) k = s.c[i];
        const int per = 64 >> c;
        rem_part = P.part_begin[c] + k;
        rem_slot0 = (P.piece_begin[c] + k / per) * kSlots + (k % per) * (4 << c);
    }
    rowinfo[l] = make_int2(full_begin, rem_slot0);
    const bool in_long_area = l >= P.n_short;
    const int32_t long_begin = sg_long_begin(P.long_base, full_begin, l);
    for (int j = 0; j < nfull; ++j) seg_out[full_begin + j] = in_long_area ? long_begin + j : 3 * l + j;
    if (rem_part >= 0) seg_out[rem_part] = in_long_area ? long_begin + nfull : 3 * l + 2;
    if (in_long_area) {
        lrows_in_order[l - P.n_short] = make_int4(l, long_begin, nfull, rem_part >= 0 ? 1 : 0);
        crow[l - P.n_short] = sg_wave_row(nfull) ? 1 : 0;
    }
}

// std::stable_partition(lrows, nfull > kLongRow): pos = exclusive scan of crow over n + 1 entries (pos[n] = how many)
__global__ __launch_bounds__(kDbThreads) void sg_db_lrows_partition(int32_t n, const int4 *in, const int32_t *pos, int4 *out)
{
    const int32_t i = (int32_t)(blockIdx.x * kDbThreads + threadIdx.x);
    if (i >= n) return;
    const int4 r = in[i];
    out[sg_wave_row(r.z) ? pos[i] : pos[n] + (i - pos[i])] = r;
}

__global__ __launch_bounds__(kDbThreads) void sg_db_pinfo(int32_t np, DbPlan P, int2 *pinfo)
{
    const int32_t p = (int32_t)(blockIdx.x * kDbThreads + threadIdx.x);
    if (p >= np) return;
    if (p < P.nfull_total) {
        pinfo[p] = make_int2(p, 6);
        return;
    }
    int c = 6;  // the classes follow the full pieces from 6 down to 0: the last one that begins at or before p
#pragma unroll
    for (int k = 5; k >= 0; --k)
        if (p >= P.piece_begin[k]) c = k;
    pinfo[p] = make_int2(P.part_begin[c] + (p - P.piece_begin[c]) * (64 >> c), c);
}

template <class C>
__global__ __launch_bounds__(kDbThreads) void sg_db_fill(int64_t n, C value, C *out)
{
    const int64_t i = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (i < n) out[i] = value;
}

// ---- edges ---------------------------------------------------------------------------------------------------------

// sorted position i holds edge es[i] of target vertex kt[i]: its place in the row is i - vbeg, its slot the host
// build's formula; the slot of an edge whose source is not live is remembered per edge for the dead-slot lists
template <class C>
__global__ __launch_bounds__(kDbThreads) void sg_db_scatter(int64_t ne, const uint32_t *kt, const uint32_t *es, const int32_t *vbeg,
                                                            const int32_t *vend, const int32_t *live_of, const int2 *rowinfo,
                                                            const int32_t *cs, const double *w, int32_t T, int64_t nslots, C *col,
                                                            double *wv, int32_t *slot_of_edge, int32_t *bad)
{
    const int64_t i = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (i >= ne) return;
    const uint32_t v = kt[i], e = es[i];
    const int32_t l = live_of[v];
    const int32_t k = (int32_t)(i - vbeg[v]);
    const int32_t full = (vend[v] - vbeg[v]) / kSlots * kSlots;
    const int2 ri = rowinfo[l];
    const int64_t slot = k < full ? (int64_t)ri.x * kSlots + k : (int64_t)ri.y + (k - full);
    if (slot < 0 || slot >= nslots) {  // (cannot happen with a consistent plan; never write outside the layout)
        *bad = 1;
        return;
    }
    const int32_t sl = live_of[cs[e]];
    col[slot] = (C)(sl >= 0 ? sl : T);
    if (sl < 0) slot_of_edge[e] = (int32_t)slot;
    const int64_t piece = slot / kSlots;
    const int kk = (int)(slot % kSlots), lane = kk >> 2, j = kk & 3;
    wv[piece * kSlots + (j >> 1) * 128 + lane * 2 + (j & 1)] = w[e];
}

__global__ __launch_bounds__(kDbThreads) void sg_db_dead_flag(int64_t ne, const int32_t *cs, const int32_t *live_of,
                                                              unsigned char *flag)
{
    const int64_t e = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (e < ne) flag[e] = live_of[cs[e]] < 0 ? 1 : 0;
}

__global__ __launch_bounds__(kDbThreads) void sg_db_dead_gather(int64_t nd, const uint32_t *didx, const int32_t *cs,
                                                                const int32_t *slot_of_edge, uint32_t *dk, int32_t *dv)
{
    const int64_t i = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (i >= nd) return;
    const uint32_t e = didx[i];
    dk[i] = (uint32_t)cs[e];
    dv[i] = slot_of_edge[e];
}

// dead_ptr[v] = first position of source vertex v in the sorted keys, v = 0 .. nv
__global__ __launch_bounds__(kDbThreads) void sg_db_dead_ptr(int64_t nv, const uint32_t *dk, int64_t nd, int64_t *dead_ptr)
{
    const int64_t v = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
    if (v > nv) return;
    dead_ptr[v] = lower_bound<uint32_t>(dk, 0, nd, (uint32_t)v);  // (v <= nv < 2^31)
}

// ---- host ----------------------------------------------------------------------------------------------------------

enum { kDbRanking = 0, kDbPlan = 1, kDbScatter = 2, kDbDict = 3, kDbPhases = 4 };

// HIP-event milliseconds of the phases of this thread's last device build (locrec_sg_create_from_device_stats)
struct DbStats {
    double ms[kDbPhases] = {0, 0, 0, 0};
};
thread_local DbStats g_db_stats;

int32_t db_device_array(const void *p, int device, const char *what)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LOCREC_E_INVALID_ARG, "%s is not a device array", what);
    }
    if ((a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) || a.device != device)
        return fail(LOCREC_E_INVALID_ARG, "%s does not live on the current device", what);
    return LOCREC_OK;
}

// the experiments keep their host-only extra layouts: one copy of the columns to the host, then the host build
int32_t db_host_build(int64_t ne, const int64_t *src, const int64_t *dst, const double *w, locrec_sg_graph **out)
{
    std::vector<int64_t> hs((size_t)ne), ht((size_t)ne);
    std::vector<double> hw((size_t)ne);
    LOCREC_HIP_TRY(hipMemcpy(hs.data(), src, (size_t)ne * 8, hipMemcpyDeviceToHost));
    LOCREC_HIP_TRY(hipMemcpy(ht.data(), dst, (size_t)ne * 8, hipMemcpyDeviceToHost));
    LOCREC_HIP_TRY(hipMemcpy(hw.data(), w, (size_t)ne * 8, hipMemcpyDeviceToHost));
    return sg_create_impl(ne, hs.data(), ht.data(), hw.data(), 0, 1, false, out);
}

// ---- the build's phases ---------------------------------------------------------------------------------------------
// sg_create_device_impl below runs them in this order as members of one Build: what a phase leaves for later ones is a
// member (released by the last phase that reads it), what only it needs is a local of its own and goes when it returns.

struct Build {
    // the caller's DEVICE columns
    int64_t ne;
    const int64_t *src, *dst;
    const double *w;
    std::unique_ptr<locrec_sg_graph> g;  // the handle under construction (first: its stream outlives every buffer here)
    hipStream_t s = nullptr;
    PhaseClock clock;
    Temp tmp;
    const dim3 B{kDbThreads};
    // rank_vertices: vid (ascending distinct ids), cs / ct (vertex index of every edge's source / target), eidx = 0 .. ne
    DevBuf<int32_t> cs;
    DevBuf<uint32_t> ct, eidx;
    DevBuf<int64_t> vid;
    int64_t nv = 0;
    // sort_rows: the edges stably sorted by target vertex (kt) with their indices (es), every vertex's run in them
    DevBuf<uint32_t> kt, es;
    DevBuf<int32_t> vbeg, vend;
    // live_order
    DevBuf<int32_t> live_of, live_vertex;
    int32_t n_short = 0, T = 0;
    // piece_plan: the scanned row counters, the plan (sg_layout_plan.h) and the kernels' part of it
    DevBuf<DbCnt> sc;
    SgLayoutPlan plan;
    DbPlan P;
    DevBuf<int2> rowinfo;          // row_maps
    DevBuf<int32_t> slot_of_edge;  // scatter_edges: the slot of every edge whose source is not live
    DevBuf<int32_t> bad;           // scatter_edges' verdict (lives as long as the Build)
    DevBuf<int64_t> dead_ptr;      // dead_slots
    int ncu = 0;                   // sg_compute_units_and_grid, for finish_handle

    // the phases, in the order sg_create_device_impl runs them
    int32_t open(locrec_sg_graph **out, bool *built_on_host);
    int32_t rank_vertices(), sort_rows(), live_order(), piece_plan(), alloc_resident(), row_maps(), scatter_edges(), dead_slots();
    int32_t host_tables(), finish_handle();
};

// argument and pointer checks, the handle with its switches and stream.  *built_on_host: the call is already answered
// by the host build (no edge; one of the two experiments), nothing is left to do
int32_t Build::open(locrec_sg_graph **out, bool *built_on_host)
{
    *built_on_host = false;
    if (!out) return fail(LOCREC_E_INVALID_ARG, "out_graph is NULL");
    *out = nullptr;
    if (ne < 0 || ne >= ((int64_t)1 << 31)) return fail(LOCREC_E_INVALID_ARG, "n_edges must be in [0, 2^31)");
    if (ne > 0 && (!src || !dst || !w)) return fail(LOCREC_E_INVALID_ARG, "bad edge arrays");
    if (ne == 0) {  // (no array to read)
        *built_on_host = true;
        return sg_create_impl(0, nullptr, nullptr, nullptr, 0, 1, false, out);
    }
    LOCREC_TRY(ensure_device());
    g.reset(new (std::nothrow) locrec_sg_graph);
    if (!g) return fail(LOCREC_E_OOM, "host allocation failed");
    LOCREC_HIP_TRY(hipGetDevice(&g->device));
    LOCREC_TRY(db_device_array(src, g->device, "source_ids"));
    LOCREC_TRY(db_device_array(dst, g->device, "target_ids"));
    LOCREC_TRY(db_device_array(w, g->device, "balanced_weights"));
    sg_read_env(g.get());
    if (g->env_fused || g->env_persist) {
        g.reset();
        *built_on_host = true;
        return db_host_build(ne, src, dst, w, out);
    }
    LOCREC_HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    g->own_stream = true;
    g->ne = ne;
    s = g->stream;
    g_db_stats = DbStats();
    clock.s = s;
    return LOCREC_OK;
}

// min / max of the ids, then the table over [min, max] or the sort of the 2E ids
int32_t Build::rank_vertices()
{
    LOCREC_TRY(cs.alloc((size_t)ne));
    LOCREC_TRY(ct.alloc((size_t)ne));
    LOCREC_TRY(eidx.alloc((size_t)ne));
    DevBuf<unsigned long long> lohi;
    unsigned long long h[2] = {~0ull, 0ull};
    LOCREC_TRY(lohi.alloc(2));
    LOCREC_HIP_TRY(hipMemcpyAsync(lohi.p, h, sizeof h, hipMemcpyHostToDevice, s));
    LOCREC_LAUNCH(sg_db_minmax, dim3((unsigned)std::min<int64_t>(1024, (ne + kDbThreads - 1) / kDbThreads)), B, 0, s, ne, src,
                  dst, lohi.p);
    LOCREC_READ_BACK(h, lohi.p, s);
    const uint64_t id_lo = (uint64_t)id_of_key(h[0]);  // (the id's bits; differences are exact in unsigned arithmetic)
    const uint64_t id_span = h[1] - h[0];
    if (sg_dense_ids(id_span, ne) && !g->env_no_dense_ids) {
        const int64_t n = (int64_t)id_span + 1;  // table entries; the scan runs over n + 1 (a closing 0)
        DevBuf<int32_t> r;
        LOCREC_TRY(r.alloc((size_t)n + 1));
        LOCREC_HIP_TRY(hipMemsetAsync(r.p, 0, ((size_t)n + 1) * 4, s));
        LOCREC_LAUNCH(sg_db_mark, grid_for(ne), B, 0, s, ne, src, dst, id_lo, r.p);
        LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, r.p, r.p, (size_t)n + 1, s));
        int32_t k = 0;
        LOCREC_READ_BACK(k, r.p + n, s);
        nv = k;
        LOCREC_TRY(vid.alloc((size_t)nv));
        LOCREC_LAUNCH(sg_db_dense_vid, grid_for(n), B, 0, s, n, r.p, id_lo, vid.p);
        LOCREC_LAUNCH(sg_db_dense_rank, grid_for(ne), B, 0, s, ne, src, dst, id_lo, r.p, cs.p, ct.p, eidx.p);
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (r is a local)
    } else {
        DevBuf<int64_t> ids, sorted;
        DevBuf<unsigned long long> nuniq;
        LOCREC_TRY(ids.alloc((size_t)(2 * ne)));
        LOCREC_TRY(sorted.alloc((size_t)(2 * ne)));
        LOCREC_TRY(nuniq.alloc(1));
        LOCREC_LAUNCH(sg_db_interleave, grid_for(ne), B, 0, s, ne, src, dst, ids.p);
        LOCREC_PRIM(tmp, prim::sort_keys(p_, bytes_, ids.p, sorted.p, (size_t)(2 * ne), 0u, 64u, s));
        LOCREC_PRIM(tmp, prim::unique(p_, bytes_, sorted.p, ids.p, nuniq.p, (size_t)(2 * ne), s));
        unsigned long long k = 0;
        LOCREC_READ_BACK(k, nuniq.p, s);
        nv = (int64_t)k;
        sorted.release();
        LOCREC_TRY(vid.alloc((size_t)nv));
        LOCREC_HIP_TRY(hipMemcpyAsync(vid.p, ids.p, (size_t)nv * 8, hipMemcpyDeviceToDevice, s));
        LOCREC_LAUNCH(sg_db_bisect, grid_for(ne), B, 0, s, ne, src, dst, vid.p, nv, cs.p, ct.p, eidx.p);
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (ids is a local)
    }
    if (nv >= ((int64_t)1 << 31) - 2) return fail(LOCREC_E_INVALID_ARG, "too many vertices");
    g->nv = nv;
    return LOCREC_OK;
}

// rows: the edges stably sorted by target vertex; a row's order is the edge-list order
int32_t Build::sort_rows()
{
    LOCREC_TRY(kt.alloc((size_t)ne));
    LOCREC_TRY(es.alloc((size_t)ne));
    LOCREC_TRY(vbeg.alloc((size_t)nv));
    LOCREC_TRY(vend.alloc((size_t)nv));
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, ct.p, kt.p, eidx.p, es.p, (size_t)ne, 0u, (unsigned)sg_radix_bits(nv), s));
    LOCREC_HIP_TRY(hipMemsetAsync(vbeg.p, 0, (size_t)nv * 4, s));
    LOCREC_HIP_TRY(hipMemsetAsync(vend.p, 0, (size_t)nv * 4, s));
    LOCREC_LAUNCH(sg_db_row_bounds, grid_for(ne), B, 0, s, ne, kt.p, vbeg.p, vend.p);
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    ct.release();
    eidx.release();
    return LOCREC_OK;
}

// live order: rows with at most two full pieces first, ascending vertex inside each class
int32_t Build::live_order()
{
    DevBuf<unsigned long long> fl;
    LOCREC_TRY(fl.alloc((size_t)nv + 1));
    LOCREC_TRY(live_of.alloc((size_t)nv));
    LOCREC_LAUNCH(sg_db_live_flags, grid_for(nv + 1), B, 0, s, nv, vbeg.p, vend.p, fl.p);
    LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, fl.p, fl.p, (size_t)nv + 1, s));
    unsigned long long tot = 0;
    LOCREC_READ_BACK(tot, fl.p + nv, s);
    n_short = (int32_t)(tot & 0xFFFFFFFFull);
    T = n_short + (int32_t)(tot >> 32);
    LOCREC_TRY(live_vertex.alloc((size_t)T));
    LOCREC_LAUNCH(sg_db_live, grid_for(nv), B, 0, s, nv, vbeg.p, vend.p, fl.p, n_short, live_of.p, live_vertex.p);
    LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (fl is a local)
    g->nlive = T;
    g->n_short = n_short;
    return LOCREC_OK;
}

// piece plan: full pieces in row order, then remainder pieces by class 6 down to 0.  One scan of the eight per-row
// counters; its totals, and the full pieces in front of row n_short, are all the plan takes
int32_t Build::piece_plan()
{
    DbCnt tot, at_short;
    LOCREC_TRY(sc.alloc((size_t)T + 1));
    LOCREC_LAUNCH(sg_db_row_counts, grid_for((int64_t)T + 1), B, 0, s, T, live_vertex.p, vbeg.p, vend.p, sc.p);
    LOCREC_PRIM(tmp, rocprim::exclusive_scan(p_, bytes_, sc.p, sc.p, DbCnt{{0, 0, 0, 0, 0, 0, 0, 0}}, (size_t)T + 1,
                                             DbCntPlus(), s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&tot, sc.p + T, sizeof tot, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&at_short, sc.p + n_short, sizeof at_short, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    plan = sg_layout_plan(tot.c, tot.c[7], at_short.c[7], T, n_short);
    if (plan.status == SgPlanStatus::too_many_slots) return fail(LOCREC_E_INVALID_ARG, "graph too large for int32 slot ids");
    if (plan.status == SgPlanStatus::too_many_partials)
        return fail(LOCREC_E_INVALID_ARG, "graph too large for int32 partial slots");
    g->npieces = (int32_t)plan.np;
    for (int c = 0; c < 7; ++c) {
        P.piece_begin[c] = plan.piece_begin[c];
        P.part_begin[c] = plan.part_begin[c];
    }
    P.nfull_total = plan.nfull_total;
    P.T = plan.T;
    P.n_short = plan.n_short;
    P.long_base = plan.long_base;
    return LOCREC_OK;
}

// what stays resident, before the temporaries of the steps below
int32_t Build::alloc_resident()
{
    g->use16 = sg_use16(T) && !g->env_no_col16;
    if (g->use16)
        LOCREC_TRY(g->col16.alloc((size_t)plan.nslots()));
    else
        LOCREC_TRY(g->col4.alloc((size_t)plan.np * 64));
    LOCREC_TRY(g->w2.alloc((size_t)plan.np * 128));
    LOCREC_TRY(g->pinfo.alloc((size_t)plan.np));
    LOCREC_TRY(g->seg_out.alloc((size_t)plan.npart));
    LOCREC_TRY(g->lrows.alloc((size_t)plan.long_area_rows()));
    LOCREC_TRY(g->PA.alloc((size_t)(2 * plan.pa)));
    LOCREC_TRY(g->xbuf.alloc((size_t)(2 * (T + 2))));
    LOCREC_TRY(g->parts.alloc(2 * kParts));
    LOCREC_TRY(g->state.alloc(1));
    return LOCREC_OK;
}

// rows, segments, pieces: rowinfo, seg_out, lrows (partitioned: the whole-wave rows first), pinfo
int32_t Build::row_maps()
{
    const int64_t np = plan.np;
    const int32_t nl = plan.long_area_rows();
    DevBuf<int32_t> crow;  // (declared in this order: lrows_in_order goes first)
    DevBuf<int4> lrows_in_order;
    LOCREC_TRY(rowinfo.alloc((size_t)T));
    LOCREC_TRY(lrows_in_order.alloc((size_t)nl));
    LOCREC_TRY(crow.alloc((size_t)nl + 1));
    LOCREC_HIP_TRY(hipMemsetAsync(g->seg_out.p, 0xFF, g->seg_out.bytes(), s));  // -1: a segment no row owns
    LOCREC_HIP_TRY(hipMemsetAsync(crow.p, 0, crow.bytes(), s));
    LOCREC_HIP_TRY(hipMemsetAsync(g->PA.p, 0, (size_t)(2 * plan.pa) * sizeof(double), s));
    if (T > 0) {
        LOCREC_LAUNCH(sg_db_row_maps, grid_for(T), B, 0, s, P, live_vertex.p, vbeg.p, vend.p, sc.p, rowinfo.p, g->seg_out.p,
                      lrows_in_order.p, crow.p);
    }
    int32_t n_crows = 0;
    if (nl > 0) {
        LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, crow.p, crow.p, (size_t)nl + 1, s));
        LOCREC_LAUNCH(sg_db_lrows_partition, grid_for(nl), B, 0, s, nl, lrows_in_order.p, crow.p, g->lrows.p);
        LOCREC_HIP_TRY(hipMemcpyAsync(&n_crows, crow.p + nl, 4, hipMemcpyDeviceToHost, s));
    }
    if (np > 0) {
        LOCREC_LAUNCH(sg_db_pinfo, grid_for(np), B, 0, s, (int32_t)np, P, g->pinfo.p);
    }
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    g->nlong = n_crows;  // (rows with more than kLongRow full pieces: all of them sit in the long area)
    g->n_crows = n_crows;
    g->nlrows = nl;
    g->pa_stride = (int32_t)plan.pa;
    sc.release();
    return LOCREC_OK;
}

// slot of every edge; col and w (through the weight interleave)
int32_t Build::scatter_edges()
{
    const int64_t nslots = plan.nslots();
    LOCREC_TRY(slot_of_edge.alloc((size_t)ne));
    LOCREC_TRY(bad.alloc(1));
    LOCREC_HIP_TRY(hipMemsetAsync(bad.p, 0, 4, s));
    LOCREC_HIP_TRY(hipMemsetAsync(g->w2.p, 0, (size_t)nslots * 8, s));
    if (g->use16) {
        LOCREC_LAUNCH(sg_db_fill<unsigned short>, grid_for(nslots), B, 0, s, nslots, (unsigned short)T, g->col16.p);
        LOCREC_LAUNCH(sg_db_scatter<unsigned short>, grid_for(ne), B, 0, s, ne, kt.p, es.p, vbeg.p, vend.p, live_of.p, rowinfo.p,
                      cs.p, w, T, nslots, g->col16.p, reinterpret_cast<double *>(g->w2.p), slot_of_edge.p, bad.p);
    } else {
        int32_t *col = reinterpret_cast<int32_t *>(g->col4.p);
        LOCREC_LAUNCH(sg_db_fill<int32_t>, grid_for(nslots), B, 0, s, nslots, T, col);
        LOCREC_LAUNCH(sg_db_scatter<int32_t>, grid_for(ne), B, 0, s, ne, kt.p, es.p, vbeg.p, vend.p, live_of.p, rowinfo.p, cs.p, w,
                      T, nslots, col, reinterpret_cast<double *>(g->w2.p), slot_of_edge.p, bad.p);
    }
    int32_t bad_h = 0;
    LOCREC_READ_BACK(bad_h, bad.p, s);
    if (bad_h) return fail(LOCREC_E_DEVICE, "device build: an edge fell outside the piece plan");
    kt.release();
    es.release();
    rowinfo.release();
    vbeg.release();
    vend.release();
    return LOCREC_OK;
}

// dead slots: the out-edges of source-only vertices, by source, edge-list order inside a source
int32_t Build::dead_slots()
{
    LOCREC_TRY(dead_ptr.alloc((size_t)nv + 1));
    {
        DevBuf<unsigned char> flag;
        DevBuf<uint32_t> didx;
        DevBuf<unsigned long long> ndead;
        LOCREC_TRY(flag.alloc((size_t)ne));
        LOCREC_TRY(didx.alloc((size_t)ne));
        LOCREC_TRY(ndead.alloc(1));
        LOCREC_LAUNCH(sg_db_dead_flag, grid_for(ne), B, 0, s, ne, cs.p, live_of.p, flag.p);
        LOCREC_PRIM(tmp, prim::select_flagged(p_, bytes_, prim::counting_iterator<uint32_t>(0), flag.p, didx.p, ndead.p,
                                              (size_t)ne, s));
        unsigned long long k = 0;
        LOCREC_READ_BACK(k, ndead.p, s);
        const int64_t nd = (int64_t)k;
        flag.release();
        LOCREC_TRY(g->dead_slots_dev.alloc((size_t)nd));
        DevBuf<uint32_t> dk, dk2;
        DevBuf<int32_t> dv;
        LOCREC_TRY(dk.alloc((size_t)nd));
        LOCREC_TRY(dk2.alloc((size_t)nd));
        LOCREC_TRY(dv.alloc((size_t)nd));
        if (nd > 0) {
            LOCREC_LAUNCH(sg_db_dead_gather, grid_for(nd), B, 0, s, nd, didx.p, cs.p, slot_of_edge.p, dk.p, dv.p);
            LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, dk.p, dk2.p, dv.p, g->dead_slots_dev.p, (size_t)nd, 0u,
                                              (unsigned)sg_radix_bits(nv), s));
        }
        LOCREC_LAUNCH(sg_db_dead_ptr, grid_for(nv + 1), B, 0, s, nv, dk2.p, nd, dead_ptr.p);
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (locals)
    }
    slot_of_edge.release();
    cs.release();
    tmp.buf.release();
    return LOCREC_OK;
}

// what the handle keeps on the host (V-sized): begin_request and fetch use it
int32_t Build::host_tables()
{
    g->vid.resize((size_t)nv);
    g->live_of.resize((size_t)nv);
    g->live_vertex.resize((size_t)T);
    g->dead_ptr.resize((size_t)nv + 1);
    LOCREC_HIP_TRY(hipMemcpyAsync(g->vid.data(), vid.p, (size_t)nv * 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(g->live_of.data(), live_of.p, (size_t)nv * 4, hipMemcpyDeviceToHost, s));
    if (T > 0) LOCREC_HIP_TRY(hipMemcpyAsync(g->live_vertex.data(), live_vertex.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(g->dead_ptr.data(), dead_ptr.p, ((size_t)nv + 1) * 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    vid.release();
    live_of.release();
    live_vertex.release();
    dead_ptr.release();
    return LOCREC_OK;
}

// the byte figures bench.py reports, persist_pw, the phase times
int32_t Build::finish_handle()
{
    sg_closing_figures(g.get(), plan.np, plan.npart, ncu);
    g->persist_ok = false;  // (LOCREC_SG_PERSIST handles come from the host build)
    return clock.read(g_db_stats.ms);
}

// kDbScatter covers the row sort and the scatter with the dead slots and the host tables, kDbPlan the live order
// through pinfo
int32_t sg_create_device_impl(int64_t ne, const int64_t *src, const int64_t *dst, const double *w, locrec_sg_graph **out)
{
    Build b{ne, src, dst, w};
    bool built_on_host = false;
    LOCREC_TRY(b.open(out, &built_on_host));
    if (built_on_host) return LOCREC_OK;
    LOCREC_TRY(b.clock.mark(kDbRanking));
    LOCREC_TRY(b.rank_vertices());
    LOCREC_TRY(b.clock.mark(kDbScatter));
    LOCREC_TRY(b.sort_rows());
    LOCREC_TRY(b.clock.mark(kDbPlan));
    LOCREC_TRY(b.live_order());
    LOCREC_TRY(b.piece_plan());
    LOCREC_TRY(b.alloc_resident());
    LOCREC_TRY(b.row_maps());
    LOCREC_TRY(b.clock.mark(kDbScatter));
    LOCREC_TRY(b.scatter_edges());
    LOCREC_TRY(b.dead_slots());
    LOCREC_TRY(b.host_tables());
    sg_poll_word(b.g.get());  // from here on what the host build does too, over the resident arrays (sg_build_shared.h)
    b.ncu = sg_compute_units_and_grid(b.g.get());
    LOCREC_TRY(b.clock.mark(kDbDict));
    LOCREC_TRY(sg_weight_dictionary(b.g.get(), b.plan.np));
    LOCREC_TRY(b.clock.mark(-1));
    LOCREC_TRY(b.finish_handle());
    *out = b.g.release();
    return LOCREC_OK;
}

}  // namespace

extern "C" int32_t locrec_sg_create_from_device(int64_t ne, const int64_t *src, const int64_t *dst, const double *w,
                                                locrec_sg_graph **out) try
{
    return sg_create_device_impl(ne, src, dst, w, out);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_create_from_device_stats(double *out_ranking_ms, double *out_plan_ms, double *out_scatter_ms,
                                                      double *out_dictionary_ms) try
{
    if (out_ranking_ms) *out_ranking_ms = g_db_stats.ms[kDbRanking];
    if (out_plan_ms) *out_plan_ms = g_db_stats.ms[kDbPlan];
    if (out_scatter_ms) *out_scatter_ms = g_db_stats.ms[kDbScatter];
    if (out_dictionary_ms) *out_dictionary_ms = g_db_stats.ms[kDbDict];
    return LOCREC_OK;
} LOCREC_CATCH_ALL
