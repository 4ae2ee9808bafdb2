// knn_pool.h -- the shared-launch path of a pool of resident indexes (locrec_knn_pool_*, knn_batch.hip).  Included at the
// end of knn_large.hip.
//
// The reference serves every request from the index of sorted{home region, target region}
// (KnnRecommenderMain.scala:53-67): a queue of request lines fans out over many region-set indexes, most of them a few
// hundred to a few thousand persons.  At the shipped --k-nearest 2000000 each of them goes through
// knn_large_recommend_batch: per member and per tile of kLkbQt queries nine launches, a memset and a host wait, on
// grids of 2 - 12 blocks.  The pool runs the members' tiles side by side:
//
//   wave w        the w-th tile (kLkbQt distinct requests) of every member that still has one.  A query's column does
//                 not depend on its tile-mates, so how a member's requests are cut into tiles is free
//   table         one KpRow per member of the wave: the tile as lkb_describe_tile (knn_large.hip) describes it to the
//                 member's own launches, and the aggregation's arguments; one copy
//   launches      ONE per kernel and wave, the member = a block index:
//                   lkb_fill_pool               (element blocks of the wave's longest query, 2 families x kLkbQt, members)
//                   lkb_scan_pool               (row blocks of the largest member, members); a block past its member's
//                                               rows returns before any barrier or read; dynamic LDS = the largest bitmap
//                   lkb_fill_pool (wipe)        as the set launch: every member's dense tables are all zero again
//                   lk_aggregate_segments_pool  (segment blocks of the largest member, members)
//                   lk_sum_segments_pool        (place blocks of the largest member, members)
//                   lk_finish_count_pool        (finish tiles of the largest member, kLkbQt, members)
//                   lk_finish_emit_pool         as the count launch, rows at per-request bases of the pool's row buffer
//   read-back     ONE tile-count buffer for all members of the wave: one copy, one wait
//
// The bodies are knn_large.hip's (lkb_fill_body, lkb_scan_body, lk_*_body) on each member's own workspaces (lkb_S, the
// dense tables, the segment and place sums): the order of operations per (member, query) is that of the member's own
// batch, so request i's rows are bit for bit what locrec_knn_recommend_batch returns for it.  A member without a rated
// place (or without segments) joins no wave: its requests have no rows.  The host arithmetic is the per-index batch's
// too (knn_pool_plan.h: waves, a tile's bases), and so is the growth of the row buffer (lkb_grow_rows).
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950: VGPRs / LDS bytes (static) / scratch.  The kernels of
// knn_large.hip have the figures they had before their bodies became functions; the pool's kernels have the same.
//   lkb_fill                       6 /  0 / 0     lkb_fill_pool                 7 /  0 / 0
//   lkb_scan                     112 / 64 / 0     lkb_scan_pool               112 / 64 / 0   (+ the bitmap, dynamic)
//   lk_aggregate_segments<16, 2> 150 /  0 / 0     lk_aggregate_segments_pool  150 /  0 / 0
//   lk_sum_segments<16>           18 /  0 / 0     lk_sum_segments_pool         18 /  0 / 0
//   lk_finish_count               12 / 16 / 0     lk_finish_count_pool         12 / 16 / 0
//   lk_finish_emit<16>            20 / 48 / 0     lk_finish_emit_pool          18 / 48 / 0
// (the single request's lk_aggregate_segments<1, 8> 56, lk_sum_segments<1> 18, lk_finish_emit<1> 20: unchanged too)

#include "knn_pool_api.h"

namespace {

// a member's row of the wave's launch table
struct KpRow {
    LkbFill fp, fc;  // (their `set` is the launch's argument)
    LkbScan P;
    const int64_t *seg_begin, *seg_end;
    const int32_t *cp_row;
    const double *cp_rating;
    double *seg_ws, *seg_ss;  // [segment][kLkbQt]
    const int32_t *place_seg0;
    double *ws, *ss;          // [query][place]
    const int64_t *cplace_ids;
    int32_t *cand;            // the tile's candidate counters (the pool's)
    int32_t *tile_cnt;        // the member's part of the wave's tile counts: [kLkbQt][tiles]
    int32_t nsegs, nplaces, tiles, pad;
};

// grid (element blocks, 2 * kLkbQt, members): y = family * kLkbQt + query
__global__ void lkb_fill_pool(const KpRow *__restrict__ tab, const int32_t set)
{
    const KpRow &m = tab[blockIdx.z];
    const int family = (int)blockIdx.y / kLkbQt, t = (int)blockIdx.y % kLkbQt;
    lkb_fill_body(family ? m.fc : m.fp, set, (int)blockIdx.x, t);
}

// grid (row blocks of the largest member, members)
__global__ __launch_bounds__(256) void lkb_scan_pool(const KpRow *__restrict__ tab)
{
    const KpRow &m = tab[blockIdx.y];
    if ((int64_t)blockIdx.x * 256 >= m.P.nrows) return;  // (the whole block: before any barrier or read of the member's data)
    lkb_scan_body(m.P, m.cand, (int)blockIdx.x);
}

// grid (segment blocks of the largest member, members)
__global__ __launch_bounds__(256) void lk_aggregate_segments_pool(const KpRow *__restrict__ tab)
{
    const KpRow &m = tab[blockIdx.y];
    lk_aggregate_segments_body<kLkbQt, 2>(m.seg_begin, m.seg_end, m.nsegs, m.cp_row, m.cp_rating, m.P.S, m.seg_ws, m.seg_ss,
                                          (int)blockIdx.x);
}

// grid (blocks of 256 (place, query) pairs of the largest member, members)
__global__ __launch_bounds__(256) void lk_sum_segments_pool(const KpRow *__restrict__ tab)
{
    const KpRow &m = tab[blockIdx.y];
    lk_sum_segments_body<kLkbQt>(m.place_seg0, m.nplaces, m.seg_ws, m.seg_ss, m.ws, m.ss, blockIdx.x);
}

// grid (finish tiles of the largest member, kLkbQt, members)
__global__ __launch_bounds__(256) void lk_finish_count_pool(const KpRow *__restrict__ tab)
{
    const KpRow &m = tab[blockIdx.z];
    if ((int)blockIdx.x >= m.tiles) return;
    lk_finish_count_body(m.ss, m.nplaces, m.tile_cnt, (int)blockIdx.x, (int)blockIdx.y, m.tiles);
}

__global__ __launch_bounds__(256) void lk_finish_emit_pool(const KpRow *__restrict__ tab, const LkBases<kLkbQt> *__restrict__ bases,
                                                           int64_t *out_place, double *out_est)
{
    const KpRow &m = tab[blockIdx.z];
    if ((int)blockIdx.x >= m.tiles) return;
    lk_finish_emit_body<kLkbQt>(m.ws, m.ss, m.nplaces, m.tile_cnt, m.cplace_ids, bases[blockIdx.z], out_place, out_est,
                                (int64_t *)nullptr, (int64_t *)nullptr, (int)blockIdx.x, (int)blockIdx.y, m.tiles);
}

}  // namespace

namespace locrec {

KnnPoolStats &knn_pool_stats()
{
    thread_local KnnPoolStats st;
    return st;
}

struct KnnPoolShared {
    DevBuf<unsigned char> tab;  // the wave's KpRow rows, then its LkBases rows
    DevBuf<int32_t> cand;       // [members][kLkbQt]
    DevBuf<int32_t> tile_cnt;   // every member's [kLkbQt][tiles], side by side
    DevBuf<int64_t> place;      // the call's result rows, wave after wave
    DevBuf<double> est;
    unsigned char *h = nullptr;  // pinned: the host images of tab and tile_cnt
    size_t h_bytes = 0;
    hipEvent_t ev = nullptr;     // a member's stream as the pool's stream waits for it
    ~KnnPoolShared()
    {
        if (h) (void)hipHostFree(h);
        if (ev) (void)hipEventDestroy(ev);
    }
    int32_t host_room(size_t bytes)
    {
        if (bytes <= h_bytes) return LOCREC_OK;
        if (h) (void)hipHostFree(h);
        h = nullptr;
        h_bytes = 0;
        void *p = nullptr;
        const size_t want = bytes + bytes / 8;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail(LOCREC_E_OOM, "hipHostMalloc(%zu bytes) failed", want);
        }
        h = static_cast<unsigned char *>(p);
        h_bytes = want;
        return LOCREC_OK;
    }
};

KnnPoolShared *knn_pool_shared_create() { return new KnnPoolShared(); }
void knn_pool_shared_destroy(KnnPoolShared *ws) { delete ws; }

namespace {

inline size_t kp_align(size_t b) { return (b + 255) & ~(size_t)255; }

// a member of the shared path during one call
struct KpLive {
    const KnnPoolBatch *b;
    int tiles;           // finish tiles
};

int32_t kp_run(KnnPoolShared *ws, hipStream_t s, const std::vector<KnnPoolBatch> &batches, double pw, double cw, int64_t *row_base,
               int64_t *row_len)
{
    KnnPoolStats &st = knn_pool_stats();
    // the refusal of a batch whose rows cannot be held (enqueue_large_k_batch's, on the call's total)
    int64_t worst = 0, nreq = 0;
    for (const KnnPoolBatch &b : batches) {
        worst += b.n * (int64_t)std::max<size_t>(1, b.ix->cplace_ids.size()) * 16;
        nreq += b.n;
    }
    if (worst > ((int64_t)48 << 30))
        return fail(LOCREC_E_INVALID_ARG, "a pool batch of %lld requests may return %lld GB of rows: split it", (long long)nreq,
                    (long long)(worst >> 30));
    // every member's own workspaces (on its own stream), before the pool's stream waits for the members
    std::vector<KpLive> live;
    size_t tc_words = 0;
    int64_t nwaves = 0;
    for (const KnnPoolBatch &b : batches) {
        locrec_knn_index *ix = b.ix;
        ix->have_result = false;
        ix->have_agg = false;
        ix->have_lkb = false;
        ix->single_pending = false;
        for (int64_t j = 0; j < b.n; ++j) row_base[b.first + j] = row_len[b.first + j] = 0;
        const int32_t np = (int32_t)ix->cplace_ids.size();
        const int tiles = std::max(1, (np + kFinishTile - 1) / kFinishTile);
        LOCREC_TRY(lkb_reserve(ix, tiles));
        if (np == 0 || ix->lk_nsegs <= 0 || b.n == 0) continue;  // nobody rated anything: no rows
        live.push_back({&b, tiles});
        tc_words += (size_t)tiles * kLkbQt;
        nwaves = std::max(nwaves, knn_waves_of(b.n));
    }
    if (live.empty()) return LOCREC_OK;
    const size_t nl = live.size();
    const size_t off_bases = kp_align(nl * sizeof(KpRow)), off_tc = off_bases + kp_align(nl * sizeof(LkBases<kLkbQt>));
    LOCREC_TRY(ws->host_room(off_tc + tc_words * sizeof(int32_t)));
    LOCREC_TRY(ws->tab.reserve(off_tc));
    LOCREC_TRY(ws->cand.reserve(nl * kLkbQt));
    LOCREC_TRY(ws->tile_cnt.reserve(tc_words));
    if (!ws->ev) LOCREC_HIP_TRY(hipEventCreateWithFlags(&ws->ev, hipEventDisableTiming));
    for (const KpLive &m : live) {
        LOCREC_HIP_TRY(hipEventRecord(ws->ev, m.b->ix->stream));
        LOCREC_HIP_TRY(hipStreamWaitEvent(s, ws->ev, 0));
    }
    KpRow *htab = reinterpret_cast<KpRow *>(ws->h);
    LkBases<kLkbQt> *hbases = reinterpret_cast<LkBases<kLkbQt> *>(ws->h + off_bases);
    const int32_t *htc = reinterpret_cast<const int32_t *>(ws->h + off_tc);
    const KpRow *dtab = reinterpret_cast<const KpRow *>(ws->tab.p);
    const LkBases<kLkbQt> *dbases = reinterpret_cast<const LkBases<kLkbQt> *>(ws->tab.p + off_bases);
    int64_t total = 0;
    std::vector<const KpLive *> wave;
    for (int64_t w = 0; w < nwaves; ++w) {
        wave.clear();
        for (const KpLive &m : live)
            if (knn_wave_tile(m.b->n, w) > 0) wave.push_back(&m);
        const size_t nw = wave.size();
        int max_nnz = 1, max_tiles = 1;
        int64_t max_rows = 1, max_segs = 1, max_np = 1;
        size_t lds = 0, tc_used = 0;
        for (size_t i = 0; i < nw; ++i) {
            const KpLive &m = *wave[i];
            locrec_knn_index *ix = m.b->ix;
            const int nt = knn_wave_tile(m.b->n, w);
            KpRow r{};
            int maxp = 1, maxc = 1;
            lkb_describe_tile(ix, m.b->rows + w * kLkbQt, nt, pw, cw, false, ws->cand.p + i * kLkbQt, r.fp, r.fc, r.P, maxp, maxc);
            max_nnz = std::max(max_nnz, std::max(maxp, maxc));
            r.cand = r.P.cand;
            // the aggregation's arguments (enqueue_aggregation<kLkbQt, 2>'s, and the finish kernels')
            r.seg_begin = ix->lk_seg_begin.p; r.seg_end = ix->lk_seg_end.p;
            r.cp_row = ix->cp_row.p; r.cp_rating = ix->cp_rating.p;
            r.seg_ws = ix->lkb_seg_ws.p; r.seg_ss = ix->lkb_seg_ss.p;
            r.place_seg0 = ix->lk_place_seg0.p;
            r.ws = ix->lkb_ws.p; r.ss = ix->lkb_ss.p;
            r.cplace_ids = ix->cplace_dev.p;
            r.tile_cnt = ws->tile_cnt.p + tc_used;
            r.nsegs = ix->lk_nsegs;
            r.nplaces = (int32_t)ix->cplace_ids.size();
            r.tiles = m.tiles;
            htab[i] = r;
            tc_used += (size_t)m.tiles * kLkbQt;
            max_rows = std::max<int64_t>(max_rows, ix->n);
            max_segs = std::max<int64_t>(max_segs, r.nsegs);
            max_np = std::max<int64_t>(max_np, r.nplaces);
            max_tiles = std::max(max_tiles, m.tiles);
            lds = std::max(lds, (size_t)(r.P.bit_mask + 1u) / 8u);
        }
        LOCREC_HIP_TRY(hipMemcpyAsync(ws->tab.p, htab, nw * sizeof(KpRow), hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemsetAsync(ws->cand.p, 0, nw * kLkbQt * sizeof(int32_t), s));
        const dim3 gfill((unsigned)((max_nnz + 255) / 256), 2 * kLkbQt, (unsigned)nw);
        hipLaunchKernelGGL(lkb_fill_pool, gfill, dim3(256), 0, s, dtab, 1);
        hipLaunchKernelGGL(lkb_scan_pool, dim3((unsigned)((max_rows + 255) / 256), (unsigned)nw), dim3(256), lds, s, dtab);
        hipLaunchKernelGGL(lkb_fill_pool, gfill, dim3(256), 0, s, dtab, 0);  // the dense tables go back to all zero
        hipLaunchKernelGGL(lk_aggregate_segments_pool, dim3((unsigned)((max_segs + 3) / 4), (unsigned)nw), dim3(256), 0, s, dtab);
        hipLaunchKernelGGL(lk_sum_segments_pool, dim3((unsigned)((max_np * kLkbQt + 255) / 256), (unsigned)nw), dim3(256), 0, s, dtab);
        const dim3 gfin((unsigned)max_tiles, kLkbQt, (unsigned)nw);
        hipLaunchKernelGGL(lk_finish_count_pool, gfin, dim3(256), 0, s, dtab);
        LOCREC_HIP_TRY(hipGetLastError());
        LOCREC_HIP_TRY(hipMemcpyAsync(ws->h + off_tc, ws->tile_cnt.p, tc_used * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        st.readback_bytes += (int64_t)(tc_used * sizeof(int32_t));
        ++st.host_syncs;
        const int64_t keep = total;
        tc_used = 0;
        for (size_t i = 0; i < nw; ++i) {
            const KpLive &m = *wave[i];
            const int nt = knn_wave_tile(m.b->n, w);
            int64_t len[kLkbQt];
            total = knn_tile_bases(htc + tc_used, m.tiles, nt, htab[i].P.qrow, total, hbases[i].base, len);
            for (int t = 0; t < nt; ++t) {
                const int64_t u = m.b->first + w * kLkbQt + t;
                row_base[u] = hbases[i].base[t];
                row_len[u] = len[t];
            }
            tc_used += (size_t)m.tiles * kLkbQt;
        }
        // grow-only output with headroom: the rows of the waves emitted so far survive a growth
        if ((size_t)total > ws->place.n || !ws->place.p) {
            LOCREC_TRY(lkb_grow_rows(ws->place, ws->est, total, keep, s));
            if (keep > 0) ++st.host_syncs;
        }
        LOCREC_HIP_TRY(hipMemcpyAsync(ws->tab.p + off_bases, hbases, nw * sizeof(LkBases<kLkbQt>), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(lk_finish_emit_pool, gfin, dim3(256), 0, s, dtab, dbases, ws->place.p, ws->est.p);
        LOCREC_HIP_TRY(hipGetLastError());
        ++st.waves;
        st.member_tiles += (int64_t)nw;
        st.fill_launches += 2;
        ++st.scan_launches;
        ++st.aggregate_launches;
        st.finish_launches += 3;
    }
    st.emitted_rows += total;
    return LOCREC_OK;
}

}  // namespace

int32_t knn_pool_shared_run(KnnPoolShared *ws, hipStream_t s, const std::vector<KnnPoolBatch> &batches, double pw, double cw,
                            int64_t *row_base, int64_t *row_len, const int64_t **out_place, const double **out_est)
{
    const int32_t rc = kp_run(ws, s, batches, pw, cw, row_base, row_len);
    // the members' workspaces are theirs again when this returns, whatever happened
    const hipError_t e = hipStreamSynchronize(s);
    ++knn_pool_stats().host_syncs;
    *out_place = ws->place.p;
    *out_est = ws->est.p;
    if (rc != LOCREC_OK) return rc;
    LOCREC_HIP_TRY(e);
    return LOCREC_OK;
}

}  // namespace locrec
