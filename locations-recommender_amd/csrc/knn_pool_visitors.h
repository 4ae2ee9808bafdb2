// knn_pool_visitors.h -- one mixed batch of visitors over a pool of indexes (locrec_knn_pool_visitors_*,
// knn_pool_visitors_entry.h).  Included at the end of knn_large.hip behind knn_pool.h and knn_visitors.h: the pool's
// waves (knn_pool.h) with the visitors' front (knn_visitors.h).
//
//   lkv_stage_pool  ONE launch for every visitor of every member: lkv_stage's walk and checks (lkv_stage_body), the
//                   visitor's member from member_of_visitor[nv], the member's dimensions and renumbering from a small
//                   per-member table.  One report word - the minimum over the refusals, so the first offender in CALL
//                   order whatever the members - and one counter of the entries beyond the dimensions.  The staged
//                   vectors lie where the inputs lie, bounds two words a visitor: visitor v is row 2v of ONE staged CSR
//                   whatever its member, so nothing is sorted or gathered by member - a tile lists its visitors' rows
//   wave w          the w-th tile (kLkbQt visitors, in call order) of every live sharing member; one KpRow per member whose
//                   fills point at the pool's stage and whose P.qrow holds the visitors' stage positions
//   launches        lkb_fill_pool (set), lkv_scan_pool, lkb_fill_pool (wipe), lk_aggregate_segments_pool,
//                   lk_sum_segments_pool, lk_finish_count_pool, lk_finish_emit_pool: seven per wave, plus the ONE stage
//                   launch per call, whatever the number of members; one tile-count read-back and one wait per wave
//
// Bits: per (member, visitor) the order of operations is that of the member's own visitors call at K >= n
// (lkv_scan_body, then the bodies of the large-K aggregation on the member's own workspaces), and a visitor's column does
// not depend on its tile-mates: visitor i's rows are bit for bit what locrec_knn_visitors_recommend_batch returns for
// that vector on its member alone.
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950: VGPRs / LDS bytes (static) / scratch / occupancy (waves per SIMD)
//   lkv_stage_pool   30 /  0 / 0 / 8
//   lkv_scan_pool   112 / 64 / 0 / 4   (+ the bitmap, dynamic: at most 32 KB) - lkv_scan's figures
// (lkv_stage and lkv_scan keep theirs - 26 / 0 / 0 / 8 and 112 / 64 / 0 / 4 - with their bodies as functions)

#include "knn_pool_visitors_api.h"

namespace {

// a member's row of the stage's table
struct KpvMember {
    const int32_t *new_of_old;  // of the place family, or null
    int32_t dim[2];
};

struct LkvStagePool {
    LkvStage a;                 // (its dim and new_of_old are not read)
    const int32_t *member_of;   // [nv] the visitor's member: a row of `members`
    const KpvMember *members;
};

// grid (visitor blocks, 2 families)
__global__ __launch_bounds__(256) void lkv_stage_pool(const LkvStagePool s)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y;
    if (v >= s.a.nv) return;
    const KpvMember &m = s.members[s.member_of[v]];
    lkv_stage_body(s.a, v, f, m.dim[f], f == 0 ? m.new_of_old : nullptr);
}

// grid (row blocks of the largest member, members); P.qrow[t] = the stage position of slot t's visitor, or -1
__global__ __launch_bounds__(256) void lkv_scan_pool(const KpRow *__restrict__ tab, const double *__restrict__ vnorm_p,
                                                     const double *__restrict__ vnorm_c)
{
    const KpRow &m = tab[blockIdx.y];
    if ((int64_t)blockIdx.x * 256 >= m.P.nrows) return;  // (the whole block: before any barrier or read of the member's data)
    lkv_scan_body<true>(m.P, m.cand, vnorm_p, vnorm_c, 0, (int)blockIdx.x);
}

}  // namespace

namespace locrec {

KnnPoolVisitorsStats &knn_pool_visitors_stats()
{
    thread_local KnnPoolVisitorsStats st;
    return st;
}

struct KnnPoolVisitors {
    // the stage (grow-only): knn_visitors_side.h's, for all members at once
    DevBuf<int64_t> bounds_p, bounds_c;
    DevBuf<int32_t> idx_p, idx_c, lens, member_of;
    DevBuf<double> val_p, val_c, norm_p, norm_c;
    DevBuf<unsigned long long> report;
    DevBuf<unsigned char> members;      // KpvMember rows
    DevBuf<int64_t> in_ptr_p, in_ptr_c;  // host arrays on their way in
    DevBuf<int32_t> in_idx_p, in_idx_c;
    DevBuf<double> in_val_p, in_val_c;
    std::vector<int32_t> h_lens;         // host copy of lens: [2][nv]
    int64_t nv = 0;
    // the gather for a delegated member
    DevBuf<int64_t> g_ptr_p, g_ptr_c;
    DevBuf<int32_t> g_idx_p, g_idx_c;
    DevBuf<double> g_val_p, g_val_c;
    std::vector<int64_t> h_ptr[2], hg_ptr[2];  // the call's row pointers (device arrays: read back once); the gathered ones
    std::vector<int32_t> hg_idx[2];
    std::vector<double> hg_val[2];
    bool have_h_ptr = false;
};

KnnPoolVisitors *knn_pool_visitors_create() { return new KnnPoolVisitors(); }
void knn_pool_visitors_destroy(KnnPoolVisitors *pv) { delete pv; }

int32_t knn_pool_visitors_stage(KnnPoolVisitors *pv, int device, hipStream_t s, const std::vector<KnnPoolVisitorsMember> &members,
                                const int32_t *index_of, const KnnVisitorVectors &v, int64_t *bad)
{
    KnnPoolVisitorsStats &st = knn_pool_visitors_stats();
    const int64_t nv = v.nv;
    const bool on_device = v.mem == LOCREC_MEM_DEVICE;
    const char *const fam[2] = {"place", "category"};
    const int64_t *in_ptr[2] = {v.p_ptr, v.c_ptr};
    const int32_t *in_idx[2] = {v.p_idx, v.c_idx};
    const double *in_val[2] = {v.p_val, v.c_val};
    int64_t total[2] = {0, 0};
    pv->have_h_ptr = false;
    pv->nv = nv;
    // the row pointers decide how much is read: their ends first (knn_visitors_stage's checks and texts)
    if (on_device) {
        LOCREC_TRY(lkv_device_array(v.p_ptr, device, "place rowptr"));
        LOCREC_TRY(lkv_device_array(v.c_ptr, device, "category rowptr"));
        int64_t ends[4] = {0, 0, 0, 0};
        for (int f = 0; f < 2; ++f) {
            LOCREC_HIP_TRY(hipMemcpyAsync(&ends[2 * f], in_ptr[f], 8, hipMemcpyDeviceToHost, s));
            LOCREC_HIP_TRY(hipMemcpyAsync(&ends[2 * f + 1], in_ptr[f] + nv, 8, hipMemcpyDeviceToHost, s));
        }
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        ++st.host_syncs;
        st.readback_bytes += 32;
        for (int f = 0; f < 2; ++f) {
            if (ends[2 * f] != 0) return fail(LOCREC_E_INVALID_ARG, "%s rowptr must start at 0", fam[f]);
            total[f] = ends[2 * f + 1];
        }
    } else {
        for (int f = 0; f < 2; ++f) {
            if (in_ptr[f][0] != 0) return fail(LOCREC_E_INVALID_ARG, "%s rowptr must start at 0", fam[f]);
            total[f] = in_ptr[f][nv];
        }
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
            LOCREC_TRY(lkv_device_array(in_idx[f], device, f == 0 ? "place indices" : "category indices"));
            LOCREC_TRY(lkv_device_array(in_val[f], device, f == 0 ? "place values" : "category values"));
        }
    }
    const KnnPoolVisitorsStageSizes psz = knn_pool_visitors_stage_sizes(nv, total[0], total[1], (int64_t)members.size());
    const KnnVisitorsStageSizes &sz = psz.one;
    if (!on_device) {
        LOCREC_TRY(pv->in_ptr_p.reserve((size_t)nv + 1));
        LOCREC_TRY(pv->in_ptr_c.reserve((size_t)nv + 1));
        LOCREC_TRY(pv->in_idx_p.reserve(sz.p_elems));
        LOCREC_TRY(pv->in_val_p.reserve(sz.p_elems));
        LOCREC_TRY(pv->in_idx_c.reserve(sz.c_elems));
        LOCREC_TRY(pv->in_val_c.reserve(sz.c_elems));
        int64_t *d_ptr[2] = {pv->in_ptr_p.p, pv->in_ptr_c.p};
        int32_t *d_idx[2] = {pv->in_idx_p.p, pv->in_idx_c.p};
        double *d_val[2] = {pv->in_val_p.p, pv->in_val_c.p};
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
    LOCREC_TRY(pv->bounds_p.reserve(sz.bounds));
    LOCREC_TRY(pv->bounds_c.reserve(sz.bounds));
    LOCREC_TRY(pv->idx_p.reserve(sz.p_elems));
    LOCREC_TRY(pv->val_p.reserve(sz.p_elems));
    LOCREC_TRY(pv->idx_c.reserve(sz.c_elems));
    LOCREC_TRY(pv->val_c.reserve(sz.c_elems));
    LOCREC_TRY(pv->norm_p.reserve(sz.norms));
    LOCREC_TRY(pv->norm_c.reserve(sz.norms));
    LOCREC_TRY(pv->lens.reserve(sz.lens));
    LOCREC_TRY(pv->report.reserve(2));
    LOCREC_TRY(pv->member_of.reserve(psz.member_of));
    LOCREC_TRY(pv->members.reserve(psz.members * sizeof(KpvMember)));
    // the members' table (the row of a member nobody asks is never read) and the visitors' members
    std::vector<KpvMember> tab(members.size());
    for (size_t m = 0; m < members.size(); ++m) {
        tab[m].new_of_old = members[m].asked ? members[m].ix->visitors.new_of_old.p : nullptr;
        tab[m].dim[0] = members[m].ix->fp.dim;
        tab[m].dim[1] = members[m].ix->fc.dim;
    }
    unsigned long long report[2] = {kVisitorsNoReport, 0ull};
    LOCREC_HIP_TRY(hipMemcpyAsync(pv->report.p, report, sizeof report, hipMemcpyHostToDevice, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(pv->members.p, tab.data(), tab.size() * sizeof(KpvMember), hipMemcpyHostToDevice, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(pv->member_of.p, index_of, (size_t)nv * 4, hipMemcpyHostToDevice, s));
    LkvStagePool P{};
    LkvStage &a = P.a;
    a.nv = nv;
    for (int f = 0; f < 2; ++f) {
        a.ptr[f] = in_ptr[f];
        a.idx[f] = in_idx[f];
        a.val[f] = in_val[f];
        a.total[f] = total[f];
    }
    a.bounds[0] = pv->bounds_p.p; a.bounds[1] = pv->bounds_c.p;
    a.out_idx[0] = pv->idx_p.p; a.out_idx[1] = pv->idx_c.p;
    a.out_val[0] = pv->val_p.p; a.out_val[1] = pv->val_c.p;
    a.norm[0] = pv->norm_p.p; a.norm[1] = pv->norm_c.p;
    a.lens = pv->lens.p;
    a.report = pv->report.p;
    P.member_of = pv->member_of.p;
    P.members = reinterpret_cast<const KpvMember *>(pv->members.p);
    hipLaunchKernelGGL(lkv_stage_pool, dim3((unsigned)((nv + 255) / 256), 2), dim3(256), 0, s, P);
    LOCREC_HIP_TRY(hipGetLastError());
    ++st.stage_launches;
    pv->h_lens.resize(sz.lens);
    LOCREC_HIP_TRY(hipMemcpyAsync(report, pv->report.p, sizeof report, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(pv->h_lens.data(), pv->lens.p, sz.lens * 4, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (the host images of the table and of index_of are free again, too)
    ++st.host_syncs;
    st.readback_bytes += (int64_t)(sizeof report + sz.lens * 4);
    if (report[0] != kVisitorsNoReport) return lkv_refuse(report[0], bad);
    st.beyond = (int64_t)report[1];
    return LOCREC_OK;
}

namespace {

// a member of the shared path during one call
struct KpvLive {
    const KnnPoolVisitorsBatch *b;
    int tiles;  // finish tiles
};

int32_t kpv_run(KnnPoolShared *ws, KnnPoolVisitors *pv, hipStream_t s, const std::vector<KnnPoolVisitorsBatch> &batches, double pw,
                double cw, int64_t *row_base, int64_t *row_len)
{
    KnnPoolVisitorsStats &st = knn_pool_visitors_stats();
    // every member's own workspaces (on its own stream), before the pool's stream waits for the members
    std::vector<KpvLive> live;
    size_t tc_words = 0;
    int64_t nwaves = 0;
    for (const KnnPoolVisitorsBatch &b : batches) {
        locrec_knn_index *ix = b.ix;
        for (int64_t j = 0; j < b.n; ++j) row_base[b.visitors[j]] = row_len[b.visitors[j]] = 0;
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
    for (const KpvLive &m : live) {  // (a first-use memset of the dense tables runs on the member's stream)
        LOCREC_HIP_TRY(hipEventRecord(ws->ev, m.b->ix->stream));
        LOCREC_HIP_TRY(hipStreamWaitEvent(s, ws->ev, 0));
    }
    KpRow *htab = reinterpret_cast<KpRow *>(ws->h);
    LkBases<kLkbQt> *hbases = reinterpret_cast<LkBases<kLkbQt> *>(ws->h + off_bases);
    const int32_t *htc = reinterpret_cast<const int32_t *>(ws->h + off_tc);
    const KpRow *dtab = reinterpret_cast<const KpRow *>(ws->tab.p);
    const LkBases<kLkbQt> *dbases = reinterpret_cast<const LkBases<kLkbQt> *>(ws->tab.p + off_bases);
    int64_t total = 0;
    std::vector<const KpvLive *> wave;
    for (int64_t w = 0; w < nwaves; ++w) {
        wave.clear();
        for (const KpvLive &m : live)
            if (knn_wave_tile(m.b->n, w) > 0) wave.push_back(&m);
        const size_t nw = wave.size();
        unsigned fill_blocks = 1;
        int max_tiles = 1;
        int64_t max_rows = 1, max_segs = 1, max_np = 1;
        size_t lds = 0, tc_used = 0;
        for (size_t i = 0; i < nw; ++i) {
            const KpvLive &m = *wave[i];
            locrec_knn_index *ix = m.b->ix;
            const int nt = knn_wave_tile(m.b->n, w);
            const int64_t *vis = m.b->visitors + w * kLkbQt;
            KpRow r{};
            LkbScan &P = r.P;
            // the tile as lkv_scan_tile describes it to the member's own launches, the fills reading the pool's stage
            for (int t = 0; t < kLkbQt; ++t) {
                P.qrow[t] = t < nt ? (int32_t)vis[t] : -1;
                r.fp.qrow[t] = r.fc.qrow[t] = t < nt ? knn_visitors_stage_row(vis[t]) : -1;
            }
            r.fp.ptr = pv->bounds_p.p; r.fp.idx = pv->idx_p.p; r.fp.val = pv->val_p.p; r.fp.qd = ix->lkb_qd_p.p;
            lkb_bitmap_of(ix, &r.fp.bits, &r.fp.bit_mask);
            r.fc.ptr = pv->bounds_c.p; r.fc.idx = pv->idx_c.p; r.fc.val = pv->val_c.p; r.fc.qd = ix->lkb_qd_c.p;
            P.bits = r.fp.bits;
            P.bit_mask = r.fp.bit_mask;
            P.p_ptr = ix->fp.csr_ptr.p; P.p_idx = ix->fp.csr_idx.p; P.p_val = ix->fp.csr_val.p;
            P.c_ptr = ix->fc.csr_ptr.p; P.c_idx = ix->fc.csr_idx.p; P.c_val = ix->fc.csr_val.p;
            P.norm_p = ix->fp.norm.p; P.norm_c = ix->fc.norm.p;
            P.qd_p = ix->lkb_qd_p.p; P.qd_c = ix->lkb_qd_c.p;
            P.nrows = (int32_t)ix->n;
            P.pw = pw; P.cw = cw;
            P.S = ix->lkb_S.p;
            P.cand = ws->cand.p + i * kLkbQt;
            P.transposed = 0;
            r.cand = P.cand;
            fill_blocks = std::max(fill_blocks, knn_pool_visitors_fill_blocks(pv->h_lens.data(), pv->nv, vis, nt));
            // the aggregation's arguments (kp_run's)
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
            lds = std::max(lds, (size_t)(P.bit_mask + 1u) / 8u);
        }
        LOCREC_HIP_TRY(hipMemcpyAsync(ws->tab.p, htab, nw * sizeof(KpRow), hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemsetAsync(ws->cand.p, 0, nw * kLkbQt * sizeof(int32_t), s));
        const dim3 gfill(fill_blocks, 2 * kLkbQt, (unsigned)nw);
        hipLaunchKernelGGL(lkb_fill_pool, gfill, dim3(256), 0, s, dtab, 1);
        hipLaunchKernelGGL(lkv_scan_pool, dim3((unsigned)((max_rows + 255) / 256), (unsigned)nw), dim3(256), lds, s, dtab,
                           pv->norm_p.p, pv->norm_c.p);
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
            const KpvLive &m = *wave[i];
            const int nt = knn_wave_tile(m.b->n, w);
            int64_t len[kLkbQt];
            total = knn_tile_bases(htc + tc_used, m.tiles, nt, htab[i].P.qrow, total, hbases[i].base, len);
            for (int t = 0; t < nt; ++t) {
                const int64_t u = m.b->visitors[w * kLkbQt + t];
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

int32_t knn_pool_visitors_run(KnnPoolShared *ws, KnnPoolVisitors *pv, hipStream_t s, const std::vector<KnnPoolVisitorsBatch> &batches,
                              double pw, double cw, int64_t *row_base, int64_t *row_len, const int64_t **out_place,
                              const double **out_est)
{
    const int32_t rc = kpv_run(ws, pv, s, batches, pw, cw, row_base, row_len);
    // the members' workspaces are theirs again when this returns, whatever happened
    const hipError_t e = hipStreamSynchronize(s);
    ++knn_pool_visitors_stats().host_syncs;
    *out_place = ws->place.p;
    *out_est = ws->est.p;
    if (rc != LOCREC_OK) return rc;
    LOCREC_HIP_TRY(e);
    return LOCREC_OK;
}

int32_t knn_pool_visitors_gather(KnnPoolVisitors *pv, hipStream_t s, const KnnVisitorVectors &v, const int64_t *visitors, int64_t n,
                                 KnnVisitorVectors *out)
{
    KnnPoolVisitorsStats &st = knn_pool_visitors_stats();
    const bool on_device = v.mem == LOCREC_MEM_DEVICE;
    const int64_t *in_ptr[2] = {v.p_ptr, v.c_ptr};
    const int32_t *in_idx[2] = {v.p_idx, v.c_idx};
    const double *in_val[2] = {v.p_val, v.c_val};
    if (on_device && !pv->have_h_ptr) {  // (the stage has checked them: they ascend inside the element arrays)
        for (int f = 0; f < 2; ++f) {
            pv->h_ptr[f].resize((size_t)v.nv + 1);
            LOCREC_HIP_TRY(hipMemcpyAsync(pv->h_ptr[f].data(), in_ptr[f], ((size_t)v.nv + 1) * 8, hipMemcpyDeviceToHost, s));
        }
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        ++st.host_syncs;
        st.readback_bytes += 2 * ((int64_t)v.nv + 1) * 8;
        pv->have_h_ptr = true;
    }
    for (int f = 0; f < 2; ++f) {
        const int64_t *ptr = on_device ? pv->h_ptr[f].data() : in_ptr[f];
        std::vector<int64_t> &g = pv->hg_ptr[f];
        g.assign((size_t)n + 1, 0);
        for (int64_t j = 0; j < n; ++j) g[(size_t)j + 1] = g[(size_t)j] + (ptr[visitors[j] + 1] - ptr[visitors[j]]);
        const int64_t total = g[(size_t)n];
        if (!on_device) {
            pv->hg_idx[f].resize((size_t)total);
            pv->hg_val[f].resize((size_t)total);
            for (int64_t j = 0; j < n; ++j) {
                const int64_t a = ptr[visitors[j]], b = ptr[visitors[j] + 1];
                std::copy(in_idx[f] + a, in_idx[f] + b, pv->hg_idx[f].begin() + g[(size_t)j]);
                std::copy(in_val[f] + a, in_val[f] + b, pv->hg_val[f].begin() + g[(size_t)j]);
            }
            continue;
        }
        DevBuf<int64_t> &d_ptr = f == 0 ? pv->g_ptr_p : pv->g_ptr_c;
        DevBuf<int32_t> &d_idx = f == 0 ? pv->g_idx_p : pv->g_idx_c;
        DevBuf<double> &d_val = f == 0 ? pv->g_val_p : pv->g_val_c;
        LOCREC_TRY(d_ptr.reserve((size_t)n + 1));
        LOCREC_TRY(d_idx.reserve((size_t)std::max<int64_t>(1, total)));
        LOCREC_TRY(d_val.reserve((size_t)std::max<int64_t>(1, total)));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_ptr.p, g.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
        for (int64_t j = 0; j < n; ++j) {
            const int64_t a = ptr[visitors[j]], len = ptr[visitors[j] + 1] - a;
            if (len <= 0) continue;
            LOCREC_HIP_TRY(hipMemcpyAsync(d_idx.p + g[(size_t)j], in_idx[f] + a, (size_t)len * 4, hipMemcpyDeviceToDevice, s));
            LOCREC_HIP_TRY(hipMemcpyAsync(d_val.p + g[(size_t)j], in_val[f] + a, (size_t)len * 8, hipMemcpyDeviceToDevice, s));
        }
    }
    out->nv = n;
    out->mem = v.mem;
    if (on_device) {
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // the member's own call reads them on its own stream
        ++st.host_syncs;
        out->p_ptr = pv->g_ptr_p.p; out->p_idx = pv->g_idx_p.p; out->p_val = pv->g_val_p.p;
        out->c_ptr = pv->g_ptr_c.p; out->c_idx = pv->g_idx_c.p; out->c_val = pv->g_val_c.p;
    } else {
        out->p_ptr = pv->hg_ptr[0].data(); out->p_idx = pv->hg_idx[0].data(); out->p_val = pv->hg_val[0].data();
        out->c_ptr = pv->hg_ptr[1].data(); out->c_idx = pv->hg_idx[1].data(); out->c_val = pv->hg_val[1].data();
    }
    return LOCREC_OK;
}

}  // namespace locrec
