// knn_topk_host.h -- enqueue_topk: the top-K of a batch of queries (K <= LOCREC_KNN_BATCH_MAX_K) enqueued on the handle's
// stream, as named phases over one TopkCall.  Included by knn.hip behind the scans' plans and launchers (make_plan,
// make_plan_ht, launch_scan, launch_scan_ht, enqueue_ht_prepass, enqueue_single).  The arithmetic - chunks and merge
// levels, the admission to the head / tail form, knn_side_topk's LDS - is knn_topk_plan.h's (plain C++, checked stand-alone
// by tests/host/knn_topk_plan_check.cpp); what is left here is the order of allocations, launches and copies.
//
// A call takes one of three paths: one query as a stream (try_single); a batch with queries no tile can hold - wide rows,
// rows too long for any LDS panel - whose other queries run tiled over a patched row list while the special ones are
// selected 16 columns at a time (split_special, special_tiles); the tiled scan (run_tiled: reserve_lists .. mark_absent).
#pragma once

#include "knn_topk_plan.h"

namespace {

static_assert(kHtMaxEntries == kTopkHtMaxEntries, "knn_ht_prepass.h and knn_topk_plan.h disagree");

// Candidate slices from which ONE request takes the stream path (scan -> select -> collect -> sort).  It used to be
// 64; a region-sized index (the reference builds one recommender per region: ~3 k persons = ~50 slices) then fell
// to the tiled path: 0.092 ms per query at 2,000 persons against ~0.05 ms on the stream path.
constexpr int kSingleMinSlices = 4;

// The batch of one call: a list of rows on the device (dev, with its host image) or the range row0 .. row0 + nq - 1.
// A caller that has the list on the host passes it; nothing about a batch is kept in the handle between calls.
struct QueryRows {
    const int32_t *dev = nullptr;
    int32_t row0 = 0;
    int64_t nq = 0;
    const int32_t *host = nullptr;  // [nq] the list's rows on the host; null for a range (and for a list until it is resolved)
    int32_t row(int64_t i) const { return host ? host[(size_t)i] : row0 + (int32_t)i; }
    static QueryRows range(int32_t first, int64_t nq) { return {nullptr, first, nq, nullptr}; }
    static QueryRows list(const int32_t *dev, const std::vector<int32_t> &host) { return {dev, 0, (int64_t)host.size(), host.data()}; }
};

struct TopkCall {
    locrec_knn_index *ix;
    QueryRows q;
    int max_nnz_p, max_nnz_c;  // the longest vectors among the queries
    double pw, cw;
    int64_t k;
    bool mark_absent;
    // settled by the phases
    Plan pl{};
    bool use_ht = false;     // the head / tail form (knn_ht.h)
    int64_t ht_total = 0;    // ... and the hits of its pre-pass
    KnnTopkChunks ch{};
    ScanParams P{};
    int K() const { return (int)k; }
    int range_slices() const { return ix->cand_slice1 - ix->cand_slice0; }
};

// The only place a batch's rows are brought to the host: a list whose caller passed no host image, one blocking copy.
int32_t resolve_host_rows(QueryRows &q, std::vector<int32_t> &fetched)
{
    if (!q.dev || q.host) return LOCREC_OK;
    fetched.resize((size_t)q.nq);
    LOCREC_HIP_TRY(hipMemcpy(fetched.data(), q.dev, (size_t)q.nq * sizeof(int32_t), hipMemcpyDeviceToHost));
    q.host = fetched.data();
    return LOCREC_OK;
}

// One query over enough slices takes the stream path (enqueue_single); *used = false: the call goes on tiled.
int32_t try_single(TopkCall &c, bool *used)
{
    *used = false;
    if (c.q.nq != 1 || c.ix->no_single || c.range_slices() < kSingleMinSlices || c.mark_absent) return LOCREC_OK;
    return enqueue_single(c.ix, c.q.row(0), c.pw, c.cw, c.k, used);
}

// Head / tail form when the index has it and this batch fits its pre-pass (knn_topk_admit_head_tail); sets c.pl with it.
void admit_head_tail(TopkCall &c)
{
    const locrec::HtIndex &ht = c.ix->ht;
    c.use_ht = false;
    c.ht_total = 0;
    if (!ht.ready || c.ix->no_ht) return;
    const bool ok = knn_topk_admit_head_tail(c.q.host, c.q.row0, c.q.nq, ht.qt, ht.tail_nnz.data(), ht.tail_hits_ps.data(),
                                             kHtMaxEntries, &c.ht_total);
    c.use_ht = ok && ht.desc.p && make_plan_ht(c.ix, c.K(), c.pl);
}

// A WIDE row among the queries (per-row format fallback): its values do not fit the packed panels.
bool has_wide_query(const TopkCall &c)
{
    if (c.ix->wide_rows.empty()) return false;
    for (int64_t i = 0; i < c.q.nq; ++i)
        if (c.ix->row_is_wide(c.q.row(i))) return true;
    return false;
}

// the tile of the scan: the head / tail form's, or the largest row-scan tile that fits the LDS; false: none does
bool plan_tile(TopkCall &c) { return c.use_ht || make_plan(c.ix, c.q.nq, c.max_nnz_p, c.max_nnz_c, c.K(), c.pl); }

// The special queries of a batch - wide rows, rows too long for an LDS tile even on their own (rank()-with-ties can emit
// rows of any length) - and the rest's row list with a stand-in row in their places.
struct Special {
    std::vector<int64_t> slots;    // positions of the special queries in the batch
    std::vector<int32_t> srow;     // their rows
    std::vector<int32_t> patched;  // the batch's rows, the special ones replaced by stand_in (when there is one)
    int32_t stand_in = -1;         // the first ordinary row of the batch
    int mp = 1, mc = 1;            // the longest vectors among the ordinary rows
};
int32_t split_special(const TopkCall &c, Special &sp)
{
    locrec_knn_index *ix = c.ix;
    const int64_t nq = c.q.nq;
    sp.patched.resize((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) {
        const int32_t r = sp.patched[(size_t)i] = c.q.row(i);
        Plan one;
        if (ix->row_is_wide(r) || !make_plan(ix, 1, ix->fp.nnz[r], ix->fc.nnz[r], c.K(), one)) {
            sp.slots.push_back(i);
            sp.srow.push_back(r);
        } else {
            if (sp.stand_in < 0) sp.stand_in = r;
            sp.mp = std::max(sp.mp, ix->fp.nnz[r]);
            sp.mc = std::max(sp.mc, ix->fc.nnz[r]);
        }
    }
    if (sp.slots.empty())
        return fail(LOCREC_E_INVALID_ARG, "query tile does not fit in LDS (k=%d, nnz=%d/%d)", c.K(), c.max_nnz_p, c.max_nnz_c);
    if (sp.stand_in >= 0)
        for (int64_t i : sp.slots) sp.patched[(size_t)i] = sp.stand_in;
    return LOCREC_OK;
}

// The special queries into their slots of the result arrays, 16 at a time: one pass of every candidate's plain CSR row
// against dense tables of the tile's queries (knn_large.hip: exact for every row in every format) gives S[row][16]; each
// column then takes the single request's selection (histogram -> deciding bin -> collect -> sort) straight into its slot.
// One by one through the dense scan + full radix sort this was ~1 ms per query - 16 wide queries doubled a cfg2 step; that
// form remains for a partial candidate range, a K beyond half the collect list and LOCREC_KNN_NO_TILE_SPECIAL.
int32_t special_tiles(const TopkCall &c, const Special &sp)
{
    locrec_knn_index *ix = c.ix;
    hipStream_t s = ix->stream;
    const int K = c.K();
    const std::vector<int64_t> &longq = sp.slots;
    const std::vector<int32_t> &srow = sp.srow;
    const bool whole_range = ix->cand_slice0 == 0 && ix->cand_slice1 == ix->nslices;
    if (!(whole_range && K <= kCollectCap / 2 && !ix->no_tile_special)) {
        for (size_t j = 0; j < longq.size(); ++j) LOCREC_TRY(knn_large_topk_device(ix, srow[j], c.pw, c.cw, c.k, longq[j]));
        return LOCREC_OK;
    }
    LOCREC_TRY(locrec::knn_tile_workspaces(ix));
    const size_t flds = (size_t)kCollectCap * 12;
    LOCREC_TRY(locrec::knn_raise_lds_limit(knn_final1, flds, &ix->final1_attr));
    const int32_t nrows = (int32_t)ix->n;
    for (size_t j0 = 0; j0 < longq.size(); j0 += 16) {
        const int nt = (int)std::min<size_t>(16, longq.size() - j0);
        LOCREC_TRY(knn_large_scan_tile(ix, srow.data() + j0, nt, c.pw, c.cw));
        // all columns of the tile at once: histograms, deciding bins, collect lists, sorted lists into the slots
        // (four launches per tile; one set per column was 64 launches and 0.6 ms of a cfg2 step with 16 wide queries)
        int64_t slots[16] = {0};
        for (int t = 0; t < nt; ++t) slots[t] = longq[j0 + (size_t)t];
        LOCREC_HIP_TRY(hipMemcpyAsync(ix->tile_slots.p, slots, (size_t)nt * sizeof(int64_t), hipMemcpyHostToDevice, s));
        const double *cols = nullptr;
        LOCREC_TRY(knn_large_tile_hists(ix, nt, ix->tile_hist.p, &cols));
        hipLaunchKernelGGL(knn_select1, dim3((unsigned)nt), dim3(1024), 0, s, ix->tile_hist.p, K, ix->tile_sel.p);
        hipLaunchKernelGGL(knn_collect1, dim3((unsigned)std::max(1, (nrows + 255) / 256), (unsigned)nt), dim3(256), 0, s, cols,
                           ix->rid.p, 0, nrows, ix->tile_sel.p, ix->tile_list_s.p, ix->tile_list_r.p, ix->tile_sel.p + 3,
                           (int64_t)nrows);
        hipLaunchKernelGGL(knn_final1, dim3((unsigned)nt), dim3(256), flds, s, ix->tile_list_s.p, ix->tile_list_r.p,
                           ix->tile_sel.p + 3, K, ix->ids_by_rank.p, ix->row_of_rid.p, ix->out_ids.p, ix->out_sims.p,
                           ix->out_rows.p, ix->out_cnt.p, ix->tile_ovf.p, static_cast<unsigned char *>(nullptr),
                           ix->tile_slots.p);
        LOCREC_HIP_TRY(hipGetLastError());
        // a deciding bin with more entries than the collect list holds (a pathological tie mass): that slot
        // takes the full sort instead
        int32_t ovf[16] = {0};
        LOCREC_HIP_TRY(hipMemcpyAsync(ovf, ix->tile_ovf.p, (size_t)nt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        for (int t = 0; t < nt; ++t)
            if (ovf[t]) LOCREC_TRY(knn_large_topk_device(ix, srow[j0 + (size_t)t], c.pw, c.cw, c.k, longq[j0 + (size_t)t]));
    }
    return LOCREC_OK;
}

// the result arrays of nq queries (every path writes them)
int32_t reserve_outputs(locrec_knn_index *ix, int64_t nq, int K)
{
    LOCREC_TRY(ix->out_ids.reserve((size_t)nq * K));
    LOCREC_TRY(ix->out_sims.reserve((size_t)nq * K));
    LOCREC_TRY(ix->out_rows.reserve((size_t)nq * K));
    LOCREC_TRY(ix->out_cnt.reserve((size_t)nq));
    return LOCREC_OK;
}

// The chunks' lists, the second level's when the merge has one, and the result arrays (grow-only, in this order).
int32_t reserve_lists(TopkCall &c)
{
    locrec_knn_index *ix = c.ix;
    const size_t nq = (size_t)c.q.nq, K = (size_t)c.K();
    LOCREC_TRY(ix->part_s.reserve(nq * c.ch.nchunks * K));
    LOCREC_TRY(ix->part_rid.reserve(nq * c.ch.nchunks * K));
    LOCREC_TRY(ix->part_cnt.reserve(nq * c.ch.nchunks));
    if (c.ch.ngroups) {
        LOCREC_TRY(ix->part2_s.reserve(nq * c.ch.ngroups * K));
        LOCREC_TRY(ix->part2_rid.reserve(nq * c.ch.ngroups * K));
        LOCREC_TRY(ix->part2_cnt.reserve(nq * c.ch.ngroups));
    }
    return reserve_outputs(ix, c.q.nq, c.K());
}

// The scan's parameters from the plan and the chunks; the overflow word of the fast insertion path cleared on the stream.
int32_t scan_params(TopkCall &c)
{
    locrec_knn_index *ix = c.ix;
    hipStream_t s = ix->stream;
    const Plan &pl = c.pl;
    ScanParams &P = c.P;
    P = ScanParams{};
    P.fp = pl.fp;
    P.fc = pl.fc;
    P.rid = ix->rid.p;
    P.qrows = c.q.dev;
    P.qrow0 = c.q.row0;
    P.nq = (int32_t)c.q.nq;
    P.nrows = (int32_t)ix->n;
    P.slice0 = ix->cand_slice0;
    P.nslices = ix->cand_slice1;
    P.slices_per_chunk = c.ch.slices_per_chunk;
    P.nchunks = c.ch.nchunks;
    P.K = c.K();
    P.S = pl.S;
    P.pw = c.pw;
    P.cw = c.cw;
    P.part_s = ix->part_s.p;
    P.part_rid = ix->part_rid.p;
    P.part_cnt = ix->part_cnt.p;
    P.off_cand_s = pl.off_cand_s;
    P.off_cand_rid = pl.off_cand_rid;
    P.off_misc = pl.off_misc;
    P.off_queue = pl.off_queue;
    if (!ix->scan_overflow.p) {
        LOCREC_TRY(ix->scan_overflow.alloc(2));  // [0] this launch, [1] cumulative
        LOCREC_HIP_TRY(hipMemsetAsync(ix->scan_overflow.p, 0, 2 * sizeof(int32_t), s));
    }
    LOCREC_HIP_TRY(hipMemsetAsync(ix->scan_overflow.p, 0, sizeof(int32_t), s));
    P.overflow = ix->scan_overflow.p;
    P.fast = (pl.mode != 0 && !ix->no_fast) ? 1 : 0;
    P.flush_mask = kFlushEvery - 1;
    P.enter_threads = kEnterFastThreads;
    if (ix->env_flush > 0) P.flush_mask = ix->env_flush - 1;      // tuning
    if (ix->env_enter >= 0) P.enter_threads = ix->env_enter;
    ix->last_scan_fast = P.fast != 0;
    P.lds_bytes = (int32_t)pl.lds;
    P.poison = (debug_env("LOCREC_DEBUG_POISON") ? 1 : 0) | (debug_env("LOCREC_DEBUG_NOFILTER") ? 2 : 0) |
               (debug_env("LOCREC_DEBUG_NOEPILOGUE") ? 4 : 0);
    if (P.poison) {
        (void)hipMemsetAsync(ix->part_s.p, 0xA5, ix->part_s.bytes(), s);
        (void)hipMemsetAsync(ix->part_rid.p, 0xA5, ix->part_rid.bytes(), s);
        (void)hipMemsetAsync(ix->part_cnt.p, 0xA5, ix->part_cnt.bytes(), s);
    }
    return LOCREC_OK;
}

// The head / tail form's hit pre-pass, then the scan: the threshold-seeding launch and knn_scan_ht (dedicated), or knn_scan.
int32_t launch_scans(TopkCall &c)
{
    locrec_knn_index *ix = c.ix;
    hipStream_t s = ix->stream;
    const Plan &pl = c.pl;
    ScanParams &P = c.P;
    const int range_slices = c.range_slices();
    if (c.use_ht) {
        LOCREC_TRY(enqueue_ht_prepass(ix, c.q.dev, c.q.row0, c.q.nq, pl.qt, c.ht_total));
        P.ht.hits = ix->ht.hits.p;
        P.ht.off = ix->ht.off.p;
        P.ht.tile_base = ix->ht.tile_base.p;
        P.ht.off_stride = ix->cand_slice1 - ix->cand_slice0 + 1;
        P.ht.off_tail = pl.off_tail;
        P.ht.h = ix->ht.h;
        P.ht.c_rows = ix->fc.dim;
    }
    const dim3 grid((unsigned)c.ch.nchunks, (unsigned)c.ch.ntiles);
    const bool dedicated = c.use_ht && !ix->ht.v1 && pl.qt == 16 && ix->ht.h <= cfg::kHtHead;  // (its plane stride is a constant)
    // threshold seeding (knn_ht.h, SEED): worth a launch of its own when the scan is long - ~256 sampled slices
    // per tile cost 1 - 2 % of a cfg2 scan and remove its cold start
    const bool seeded = dedicated && pl.waves == 8 && range_slices >= ix->seed_min_slices && !ix->no_seed;
    if (seeded)
        LOCREC_TRY(launch_scan_ht(ix, pl, P, dim3(1u, (unsigned)c.ch.ntiles), s, true, false,
                                  std::max(1, range_slices / ix->seed_sample_slices)));
    if (dedicated)
        LOCREC_TRY(launch_scan_ht(ix, pl, P, grid, s, false, seeded));
    else
        LOCREC_TRY(launch_scan(ix->prof, pl, P, grid, s));
    ix->last_plan_kernel = !c.use_ht ? 1 : dedicated ? 2 : 3;
    ix->last_plan_mode = pl.mode;
    ix->last_plan_qt = pl.qt;
    ix->last_plan_waves = pl.waves;
    return LOCREC_OK;
}

// The chunks' lists of every query into its result slot: knn_merge, behind knn_merge_partial when there are groups.
int32_t merge_lists(TopkCall &c)
{
    locrec_knn_index *ix = c.ix;
    hipStream_t s = ix->stream;
    const KnnTopkChunks &ch = c.ch;
    const unsigned nq = (unsigned)c.q.nq;
    const double *fs = ix->part_s.p;
    const uint32_t *fr = ix->part_rid.p;
    const int32_t *fc = ix->part_cnt.p;
    int flists = ch.nchunks;
    if (ch.ngroups) {
        LOCREC_TRY(locrec::knn_raise_lds_limit(knn_merge_partial, ch.lds_partial));
        hipLaunchKernelGGL(knn_merge_partial, dim3((unsigned)ch.ngroups, nq), dim3(256), ch.lds_partial, s, ix->part_s.p,
                           ix->part_rid.p, ix->part_cnt.p, ch.nchunks, c.K(), ch.max_chunks, ch.M1, ix->part2_s.p,
                           ix->part2_rid.p, ix->part2_cnt.p, ch.ngroups);
        fs = ix->part2_s.p;
        fr = ix->part2_rid.p;
        fc = ix->part2_cnt.p;
        flists = ch.ngroups;
    }
    LOCREC_TRY(locrec::knn_raise_lds_limit(knn_merge, ch.lds_merge));
    hipLaunchKernelGGL(knn_merge, dim3(nq), dim3(256), ch.lds_merge, s, fs, fr, fc, flists, c.K(), ch.M,
                       ix->ids_by_rank.p, ix->row_of_rid.p, ix->out_ids.p, ix->out_sims.p, ix->out_rows.p,
                       ix->out_cnt.p);
    return LOCREC_OK;
}

// The index's wide rows as candidates (they are padding in the packed images): merged into every K-list (knn_side_topk).
int32_t side_rows(TopkCall &c)
{
    locrec_knn_index *ix = c.ix;
    if (ix->wide_rows.empty()) return LOCREC_OK;
    const int32_t nw = (int32_t)ix->wide_rows.size();
    const int c_dim = std::max(1, ix->fc.dim);
    const KnnSideTopkLds l = knn_side_topk_lds(c.K(), nw, c.max_nnz_p, c_dim);
    LOCREC_TRY(locrec::knn_raise_lds_limit(knn_side_topk, l.slds));
    hipLaunchKernelGGL(knn_side_topk, dim3((unsigned)c.q.nq), dim3(256), l.slds, ix->stream, side_csr_of(ix), ix->wide_rows_dev.p, nw,
                       c.q.dev, c.q.row0, ix->cand_slice0 * 64, (int32_t)std::min<int64_t>(ix->n, (int64_t)ix->cand_slice1 * 64),
                       c.pw, c.cw, c.K(), ix->rid.p, ix->ids_by_rank.p, ix->row_of_rid.p, ix->out_ids.p, ix->out_sims.p,
                       ix->out_rows.p, ix->out_cnt.p, c_dim, l.hash_cap);
    return LOCREC_OK;
}

// Count -1 for the queries of a range that lack a place or a category vector.
void mark_absent(TopkCall &c)
{
    locrec_knn_index *ix = c.ix;
    if (c.mark_absent)
        hipLaunchKernelGGL(knn_mark_absent, dim3((unsigned)c.q.nq), dim3(64), 0, ix->stream, ix->fp.norm.p, ix->fc.norm.p, c.q.dev,
                           c.q.row0, (int32_t)c.q.nq, c.K(), ix->out_ids.p, ix->out_sims.p, ix->out_rows.p, ix->out_cnt.p);
}

// The tiled scan of c's rows over the tile c.pl: chunk plan, workspaces, scan, merge; remembered for rerun_tiled_sync.
int32_t run_tiled(TopkCall &c)
{
    locrec_knn_index *ix = c.ix;
    c.ch = knn_topk_chunks(c.range_slices(), c.q.nq, c.pl.qt, c.pl.waves, c.K(), c.use_ht, ix->env_blocks);
    LOCREC_TRY(reserve_lists(c));
    LOCREC_TRY(scan_params(c));
    LOCREC_TRY(launch_scans(c));
    LOCREC_TRY(merge_lists(c));
    LOCREC_TRY(side_rows(c));
    mark_absent(c);
    LOCREC_HIP_TRY(hipGetLastError());
    ix->last_nq = c.q.nq;
    ix->last_k = c.k;
    ix->have_result = true;
    ix->last_tiled.qrows_dev = c.q.dev;
    ix->last_tiled.qrow0 = c.q.row0;
    ix->last_tiled.nq = c.q.nq;
    if (c.q.host) ix->last_tiled.qrows.assign(c.q.host, c.q.host + c.q.nq);
    else ix->last_tiled.qrows.clear();
    ix->last_tiled.max_p = c.max_nnz_p;
    ix->last_tiled.max_c = c.max_nnz_c;
    ix->last_tiled.pw = c.pw;
    ix->last_tiled.cw = c.cw;
    ix->last_tiled.k = c.k;
    ix->last_tiled.mark_absent = c.mark_absent;
    return LOCREC_OK;
}

// A batch with special queries: the rest tiled with a stand-in row in their places (when there is a rest), then the special
// ones into their slots.
int32_t run_with_special(TopkCall &c)
{
    locrec_knn_index *ix = c.ix;
    hipStream_t s = ix->stream;
    const int64_t nq = c.q.nq;
    Special sp;
    LOCREC_TRY(split_special(c, sp));
    if (sp.stand_in >= 0 && nq > 1) {
        LOCREC_TRY(ix->qrows_patch.reserve((size_t)nq));
        LOCREC_HIP_TRY(hipMemcpyAsync(ix->qrows_patch.p, sp.patched.data(), (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (the device list is read from here on)
        TopkCall t{ix, QueryRows::list(ix->qrows_patch.p, sp.patched), sp.mp, sp.mc, c.pw, c.cw, c.k, c.mark_absent};
        admit_head_tail(t);
        if (!plan_tile(t)) return fail(LOCREC_E_INVALID_ARG, "query tile does not fit in LDS (k=%d, nnz=%d/%d)", t.K(), sp.mp, sp.mc);
        LOCREC_TRY(run_tiled(t));
    } else {
        LOCREC_TRY(reserve_outputs(ix, nq, c.K()));
        ix->last_scan_fast = false;
    }
    LOCREC_TRY(special_tiles(c, sp));
    ix->single_pending = false;
    ix->last_nq = nq;
    ix->last_k = c.k;
    ix->have_result = true;
    return LOCREC_OK;
}

// Enqueue scan + merge for the queries q; max_nnz_p / max_nnz_c: the longest place and category vectors among them.
int32_t enqueue_topk(locrec_knn_index *ix, QueryRows q, int max_nnz_p, int max_nnz_c, double pw, double cw, int64_t k,
                     bool mark_absent = false)
{
    ix->single_pending = false;
    ix->single_direct = false;
    ix->last_scan_fast = false;
    ix->have_agg = false;  // the neighbour lists a resident batched aggregation was built from are overwritten
    ix->have_lkb = false;
    TopkCall c{ix, q, max_nnz_p, max_nnz_c, pw, cw, k, mark_absent};
    std::vector<int32_t> fetched;
    LOCREC_TRY(resolve_host_rows(c.q, fetched));
    bool used = false;
    LOCREC_TRY(try_single(c, &used));
    if (used) return LOCREC_OK;
    admit_head_tail(c);
    if (has_wide_query(c) || !plan_tile(c)) return run_with_special(c);
    return run_tiled(c);
}

}  // namespace
