// sg_pool_ranked.h -- the ranked pool (locrec_sg_pool_recommend_ranked_batch): one mixed batch of (graph, vertex, target
// region) requests over a pool's resident graphs, emitted and ranked on the device.  Included at the end of sg_batch.hip,
// behind sg_ranked.h and sg_pool.h: the sweeps, finalizes, set-up, polls and the restore launch are sg_pool_waves', the
// emit, state, membership and popcount bodies and the host's SgRkCall are sg_ranked.h's - per column and per request the order
// of operations is the ranked batch's, so request i equals locrec_sg_recommend_ranked_batch on its member alone bit for bit.
// The entry's body behind its checks is sg_pool_ranked_columns, which the pool's visitors entry (sg_pool_visitors.h) runs too.
//
//   emit rows       per member with requests its own numbering (sg_rk_rows): sorted ids, their emit rows and eid, kept
//                   resident by the pool per member and numbering (with / without the source-only vertices), built at the
//                   member's first ranked call
//   membership      one bitmap per (member, distinct target region asked of that member); ONE sg_rk_members_pool launch
//                   over (rows of the places table, members with requests), blockIdx.y = the member's table row; ONE
//                   sg_rk_popcount_pool launch over all pairs; one read-back of the caps and one synchronisation
//   requests        in emit order: by tile wave, then member in pool order, then the ranked batch's order within a tile
//                   (sg_rk_pool_order).  Groups are runs of that order within LOCREC_SG_RANKED_ROW_BUDGET
//                   (sg_rk_form_groups): a group may span members and waves, a tile's requests may straddle two groups
//   sg_rk_emit_pool per tile wave and group part ONE launch, grid (emit blocks of the wave's largest member, members of the
//                   wave); the part's table row of a member holds its SgEmitTile, state, x, eid, bitmaps and its range of
//                   the part's requests.  A block past its member's emit rows returns before it reads that member's x.
//                   count_cols is set on the wave's first part only.
//   sg_rk_state_pool  ONE launch per wave, blockIdx.x = the member: 384 bytes a member at its offset of the pool's pinned
//                   buffer (a device buffer and one plain copy where that has no device address or a member was created
//                   under LOCREC_SG_NO_PACK); one synchronisation covers the wave
//   ranking         SgRkCall::flush_group once per full group; its N rows a request come to the host once
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (VGPRs / LDS bytes / scratch):
//   sg_rk_emit_pool      82 / 32832 / 0
//   sg_rk_state_pool     14 / 0 / 0
//   sg_rk_members_pool   14 / 0 / 0
//   sg_rk_popcount_pool  8 / 4 / 0
#pragma once

#include <array>

namespace {

// A member's row of a group part's emit launch and of the wave's state launch
struct SgRkPoolRow {
    SgEmitTile tl;
    const SgBatchState *st;
    const double *xbuf;   // both parities
    const double *parts;  // both parities' block sums
    const int64_t *eid;
    const unsigned long long *bits;  // the member's bitmaps, one per distinct target region asked of it
    unsigned long long *col_rows;    // of the tile's columns
    int64_t words;                   // of one bitmap
    int64_t state_off;               // of the member's state in the wave's state image
    int32_t k0, k1;                  // the member's requests of this part, in emit order
};

// A member's row of the membership launch
struct SgRkPoolMembers {
    const int64_t *sid;
    const int32_t *srow;
    const int64_t *regions;  // the distinct target regions asked of it, ascending
    unsigned long long *bits;
    int64_t m, n_regions, words;
};

// A (member, region) pair's bitmap
struct SgRkPoolPair {
    int64_t off, words;
};

__global__ __launch_bounds__(kRkThreads) void sg_rk_members_pool(int64_t n_places, const int64_t *__restrict__ place_ids,
                                                                const int64_t *__restrict__ place_regions,
                                                                const SgRkPoolMembers *__restrict__ tab)
{
    const SgRkPoolMembers &t = tab[blockIdx.y];
    sg_rk_members_body(n_places, place_ids, place_regions, t.n_regions, t.regions, t.m, t.sid, t.srow, t.words, t.bits);
}

__global__ __launch_bounds__(kRkThreads) void sg_rk_popcount_pool(const SgRkPoolPair *__restrict__ pairs,
                                                                 const unsigned long long *__restrict__ bits,
                                                                 unsigned long long *__restrict__ caps)
{
    const SgRkPoolPair p = pairs[blockIdx.x];
    sg_rk_popcount_body(p.words, bits + p.off, caps + blockIdx.x);
}

__global__ __launch_bounds__(kRkThreads) void sg_rk_emit_pool(
    const SgRkPoolRow *__restrict__ rows, const int32_t *__restrict__ req_col, const int32_t *__restrict__ req_trow,
    const int32_t *__restrict__ req_bm, const int64_t *__restrict__ seg_begin, unsigned long long *seg_len, const int64_t rows_cap,
    int64_t *__restrict__ seg_ids, double *__restrict__ seg_probs)
{
    const SgRkPoolRow &r = rows[blockIdx.y];
    // past this member's emit rows, or nothing to do for it in this part: before any read of its x
    if ((int64_t)blockIdx.x * kRkThreads >= (int64_t)r.tl.ne || (r.k0 >= r.k1 && !r.tl.count_cols)) return;
    sg_rk_emit_body(r.tl, r.st, r.xbuf, r.eid, r.bits, r.words, r.k0, r.k1, req_col, req_trow, req_bm, seg_begin, seg_len, rows_cap,
                    seg_ids, seg_probs, r.col_rows, (int)blockIdx.x);
}

__global__ __launch_bounds__(64 * kBatchB) void sg_rk_state_pool(const SgRkPoolRow *__restrict__ rows, unsigned char *out)
{
    const SgRkPoolRow &r = rows[blockIdx.x];
    sg_rk_state_body(r.st, r.parts, out + r.state_off);
}

constexpr size_t kRkPoolStateStride = 512;  // a member's 384 bytes of state, on a line of their own
static_assert(kRkStateBytes <= kRkPoolStateStride, "a member's state fits its slot");

// the ranked batch's counters (tiles: member tiles), and the pool's own
struct SgRkPoolStats : SgRankedStats {
    int64_t tile_waves = 0, rounds = 0, emit_launches = 0;
};

SgRkPoolStats &sg_rk_pool_stats()
{
    thread_local SgRkPoolStats st;
    return st;
}

// One numbering of a member's emit rows, resident: the host's rows and their device image
struct SgRkImage {
    SgRkRows rows;
    DevBuf<int64_t> ids;  // sid, then eid
    DevBuf<int32_t> srow;
    bool built = false;
};

struct SgRkPoolCache {
    std::vector<std::array<SgRkImage, 2>> images;  // [member][with the source-only vertices]
    explicit SgRkPoolCache(size_t members) : images(members) {}
};

// the member's image of this numbering, built and uploaded at its first use (s orders the upload and sg_rk_row_ids)
int32_t sg_rk_pool_image(locrec_sg_pool *pool, int32_t gi, bool dead_rows, hipStream_t s, SgRkImage *&out)
{
    if (!pool->ranked) pool->ranked = std::make_shared<SgRkPoolCache>(pool->graphs.size());
    SgRkImage &im = static_cast<SgRkPoolCache *>(pool->ranked.get())->images[(size_t)gi][dead_rows ? 1 : 0];
    out = &im;
    if (im.built) return LOCREC_OK;
    sg_rk_rows(pool->graphs[(size_t)gi], dead_rows, im.rows);
    const int64_t m = im.rows.m;
    LOCREC_TRY(im.ids.alloc((size_t)(2 * m)));
    LOCREC_TRY(im.srow.alloc((size_t)m));
    if (m > 0) {
        // (the host arrays live as long as the image: im.rows, or the handle's own vertex list)
        LOCREC_HIP_TRY(hipMemcpyAsync(im.ids.p, im.rows.sid, (size_t)m * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(im.srow.p, im.rows.srow.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(sg_rk_row_ids, rk_grid(m), dim3(kRkThreads), 0, s, m, im.ids.p, im.srow.p, im.ids.p + m);
    }
    im.built = true;
    return LOCREC_OK;
}

// A member with requests, for the length of a call
struct SgRkPoolActive {
    int32_t gi = 0;
    SgRkImage *im = nullptr;
    int tile_max = 0;
    int64_t words = 1;
    std::vector<int64_t> regions;  // the distinct target regions asked of it, ascending
    size_t pair_base = 0;          // its first (member, region) pair
    size_t bits_off = 0;           // its bitmaps in the call's bitmap buffer, in words
};

inline size_t rk_units(size_t bytes) { return (bytes + 7) / 8; }  // 8-byte units

// The ranked pool behind its checks and sg_pool_begin_call, for n >= 1 positions over the columns `tp` runs: position i asks
// member graph_index[i] for its column uniq_of[i], whose target vertex is mem[..].uniq[..] (-1: a visitor, which is no
// vertex and so never a row of its own result).  with_lists: position i leaves out excluded_ids[excluded_offsets[i] ..
// excluded_offsets[i + 1]) (host arrays, checked).  ps: the waves' counters.
template <class Tiles>
int32_t sg_pool_ranked_columns(locrec_sg_pool *pool, SgRkPoolStats &stats, SgPoolStats &ps, const std::vector<int32_t> &act,
                               std::vector<SgPoolMember> &mem, const int64_t n, const int32_t *graph_index,
                               const std::vector<int32_t> &uniq_of, Tiles &&tp, double alpha, double epsilon, int64_t max_iterations,
                               int64_t N, int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
                               const int64_t *target_region_ids, bool with_lists, const int64_t *excluded_offsets, int64_t n_excluded,
                               const int64_t *excluded_ids, int64_t *out_ids, double *out_probabilities, int64_t *out_counts,
                               int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged)
{
    hipStream_t s = pool->stream;
    const size_t na = act.size();
    const double eps2 = epsilon * epsilon;  // :40
    auto row_of = [](const locrec_sg_graph *g, const SgRkRows &rows, int32_t tv) { return tv < 0 ? -1 : sg_rk_row_of(g, rows, tv); };
    // ---- the members with requests: their emit rows, the distinct regions asked of each, the (member, region) pairs
    const bool dead_rows = sg_rk_dead_rows(alpha, max_iterations);
    std::vector<SgRkPoolActive> am(na);
    std::vector<int32_t> act_of(pool->graphs.size(), -1);
    std::vector<size_t> nu(na);
    std::vector<int> tile_max(na);
    for (size_t a = 0; a < na; ++a) {
        SgRkPoolActive &x = am[a];
        x.gi = act[a];
        act_of[(size_t)x.gi] = (int32_t)a;
        LOCREC_TRY(sg_rk_pool_image(pool, x.gi, dead_rows, s, x.im));
        x.words = std::max<int64_t>(1, (x.im->rows.m + 63) / 64);
        x.tile_max = tile_max[a] = tp.tile_max(pool->graphs[(size_t)x.gi]);
        nu[a] = mem[(size_t)x.gi].uniq.size();
    }
    std::vector<int32_t> member_of((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        member_of[(size_t)i] = act_of[(size_t)graph_index[i]];
        am[(size_t)member_of[(size_t)i]].regions.push_back(target_region_ids[i]);
    }
    size_t P = 0, bit_words = 0;
    for (SgRkPoolActive &x : am) {
        std::sort(x.regions.begin(), x.regions.end());
        x.regions.erase(std::unique(x.regions.begin(), x.regions.end()), x.regions.end());
        x.pair_base = P;
        x.bits_off = bit_words;
        P += x.regions.size();
        bit_words += x.regions.size() * (size_t)x.words;
    }

    // ---- the requests in emit order
    SgRkPoolOrder order;
    sg_rk_pool_order(nu, tile_max, member_of, uniq_of, order);
    const size_t NU = order.ubase[na];
    std::vector<int32_t> req((size_t)(3 * n));  // column, target's emit row, bitmap (among its member's)
    std::vector<int32_t> pair_k((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = order.ord[(size_t)k];
        const SgRkPoolActive &x = am[(size_t)member_of[(size_t)i]];
        const int32_t u = uniq_of[(size_t)i];
        const size_t r = (size_t)(std::lower_bound(x.regions.begin(), x.regions.end(), target_region_ids[i]) - x.regions.begin());
        req[(size_t)k] = u % x.tile_max;
        req[(size_t)(n + k)] = row_of(pool->graphs[(size_t)x.gi], x.im->rows, mem[(size_t)x.gi].uniq[(size_t)u]);
        req[(size_t)(2 * n + k)] = (int32_t)r;
        pair_k[(size_t)k] = (int32_t)(x.pair_base + r);
    }

    // ---- device buffers.  d64, in 8-byte units; the head is ONE upload:
    //   place ids, place regions | the members' regions | targets | pairs | member table | requests ||
    //   seg_begin | seg_len | col_rows | caps
    const size_t u_pid = 0, u_preg = u_pid + (size_t)n_places, u_regions = u_preg + (size_t)n_places, u_tgt = u_regions + P,
                 u_pairs = u_tgt + (size_t)n, u_memtab = u_pairs + rk_units(P * sizeof(SgRkPoolPair)),
                 u_req = u_memtab + rk_units(na * sizeof(SgRkPoolMembers)), u_head = u_req + rk_units((size_t)(3 * n) * 4),
                 u_seg_begin = u_head, u_seg_len = u_seg_begin + (size_t)n, u_col_rows = u_seg_len + (size_t)n,
                 u_caps = u_col_rows + NU, u_end = u_caps + P;
    DevBuf<int64_t> d64;
    DevBuf<unsigned long long> d_bits;
    LOCREC_TRY(d64.alloc(u_end));
    LOCREC_TRY(d_bits.alloc(bit_words));
    int64_t *d_pid = d64.p + u_pid, *d_preg = d64.p + u_preg, *d_regions = d64.p + u_regions, *d_tgt = d64.p + u_tgt,
            *d_seg_begin = d64.p + u_seg_begin, *d_seg_len = d64.p + u_seg_len, *d_col_rows = d64.p + u_col_rows,
            *d_caps = d64.p + u_caps;
    const SgRkPoolPair *d_pairs = reinterpret_cast<const SgRkPoolPair *>(d64.p + u_pairs);
    const SgRkPoolMembers *d_memtab = reinterpret_cast<const SgRkPoolMembers *>(d64.p + u_memtab);
    const int32_t *d_req = reinterpret_cast<const int32_t *>(d64.p + u_req);
    std::vector<int64_t> head(u_head, 0);
    if (n_places > 0) {
        std::copy(place_ids, place_ids + n_places, head.begin() + (ptrdiff_t)u_pid);
        std::copy(place_region_ids, place_region_ids + n_places, head.begin() + (ptrdiff_t)u_preg);
    }
    {
        SgRkPoolPair *pairs = reinterpret_cast<SgRkPoolPair *>(head.data() + u_pairs);
        SgRkPoolMembers *memtab = reinterpret_cast<SgRkPoolMembers *>(head.data() + u_memtab);
        for (size_t a = 0; a < na; ++a) {
            const SgRkPoolActive &x = am[a];
            std::copy(x.regions.begin(), x.regions.end(), head.begin() + (ptrdiff_t)(u_regions + x.pair_base));
            for (size_t r = 0; r < x.regions.size(); ++r)
                pairs[x.pair_base + r] = SgRkPoolPair{(int64_t)(x.bits_off + r * (size_t)x.words), x.words};
            memtab[a] = SgRkPoolMembers{x.im->ids.p, x.im->srow.p, d_regions + x.pair_base, d_bits.p + x.bits_off, x.im->rows.m,
                                        (int64_t)x.regions.size(), x.words};
        }
        for (int64_t k = 0; k < n; ++k) head[u_tgt + (size_t)k] = target_region_ids[order.ord[(size_t)k]];
        std::memcpy(head.data() + u_req, req.data(), req.size() * 4);
    }
    LOCREC_HIP_TRY(hipMemcpyAsync(d64.p, head.data(), u_head * 8, hipMemcpyHostToDevice, s));
    LOCREC_HIP_TRY(hipMemsetAsync(d_seg_len, 0, ((size_t)n + NU) * 8, s));  // the segments' lengths and the columns' rows
    LOCREC_HIP_TRY(hipMemsetAsync(d_bits.p, 0, std::max<size_t>(bit_words, 1) * 8, s));
    if (n_places > 0)
        hipLaunchKernelGGL(sg_rk_members_pool, dim3(rk_grid(n_places).x, (unsigned)na), dim3(kRkThreads), 0, s, n_places, d_pid,
                           d_preg, d_memtab);
    hipLaunchKernelGGL(sg_rk_popcount_pool, dim3((unsigned)P), dim3(kRkThreads), 0, s, d_pairs, d_bits.p,
                       reinterpret_cast<unsigned long long *>(d_caps));

    // ---- the groups (request k's room: its pair's cap); a wave's row table has a row per member and group part
    SgRkCall rc{.stats = stats, .s = s, .n = n, .N = N, .n_places = n_places, .d_pid = d_pid, .d_preg = d_preg, .d_tgt = d_tgt,
                .d_seg_begin = d_seg_begin, .d_seg_len = d_seg_len};
    LOCREC_TRY(rc.plan(d_caps, P, pair_k.data(), NU));
    const std::vector<int64_t> &group_end = rc.groups.group_end;
    DevBuf<int64_t> d_ex;
    if (with_lists) LOCREC_TRY(rc.upload_lists(order.ord, excluded_offsets, n_excluded, excluded_ids, d_ex));
    DevBuf<unsigned char> d_state, d_tab;
    LOCREC_TRY(d_tab.alloc(sg_rk_pool_table_rows(nu, tile_max, order, group_end) * sizeof(SgRkPoolRow)));
    const bool pinned = !pool->no_pack && pool->h_pack_dev != nullptr && pool->h_pack_bytes >= na * kRkPoolStateStride;
    if (!pinned) LOCREC_TRY(d_state.alloc(na * kRkPoolStateStride));
    std::vector<unsigned char> own_state(pinned ? 0 : na * kRkPoolStateStride);

    std::vector<SgRkPoolRow> tab;  // the wave's rows: part p's at tab[p * nw ..)
    std::vector<int64_t> cuts;
    std::vector<size_t> present;  // the wave's members, as positions of act
    auto emit_and_rank = [&](const SgPoolWave &w) -> int32_t {
        const unsigned nw = (unsigned)w.members.size();
        stats.tiles += nw;
        // the wave's requests are one run of the emit order; the groups that end inside it cut it into parts
        unsigned emit_blocks = 1;
        present.clear();
        for (const int32_t gi : w.members) {
            present.push_back((size_t)act_of[(size_t)gi]);
            emit_blocks = std::max(emit_blocks, (unsigned)((am[present.back()].im->rows.m + kRkThreads - 1) / kRkThreads));
        }
        sg_rk_wave_cuts(present, w.k, tile_max, order, group_end, cuts);
        const size_t parts = cuts.size() - 1;
        tab.assign(parts * nw, SgRkPoolRow{});
        for (unsigned j = 0; j < nw; ++j) {
            const size_t a = present[j];
            const SgRkPoolActive &x = am[a];
            const locrec_sg_graph *g = pool->graphs[(size_t)x.gi];
            const std::vector<int32_t> &uniq = mem[(size_t)x.gi].uniq;
            const size_t t0 = w.k * (size_t)x.tile_max;
            SgRkPoolRow row{};
            row.tl.nb = w.nb[j];
            row.tl.T = g->nlive;
            row.tl.ne = (int32_t)x.im->rows.m;
            row.tl.xstride = w.tiles[j].xstride;
            for (int c = 0; c < kBatchB; ++c)
                row.tl.col_trow[c] = c < w.nb[j] ? row_of(g, x.im->rows, uniq[t0 + (size_t)c]) : -1;
            row.st = w.tiles[j].st;
            row.xbuf = w.tiles[j].xbuf;
            row.parts = w.tiles[j].parts;
            row.eid = x.im->ids.p + x.im->rows.m;
            row.bits = d_bits.p + x.bits_off;
            row.col_rows = reinterpret_cast<unsigned long long *>(d_col_rows) + order.ubase[a] + t0;
            row.words = x.words;
            row.state_off = (int64_t)(j * kRkPoolStateStride);
            const int64_t tb = order.tile_begin(a, w.k, x.tile_max), te = order.tile_end(a, w.k, x.tile_max);
            for (size_t p = 0; p < parts; ++p) {
                row.tl.count_cols = p == 0 ? 1 : 0;
                row.k0 = (int32_t)std::min(std::max(tb, cuts[p]), te);
                row.k1 = (int32_t)std::max(std::min(te, cuts[p + 1]), (int64_t)row.k0);
                tab[p * nw + j] = row;
            }
        }
        LOCREC_HIP_TRY(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * sizeof(SgRkPoolRow), hipMemcpyHostToDevice, s));
        const SgRkPoolRow *d_rows_tab = reinterpret_cast<const SgRkPoolRow *>(d_tab.p);
        // the states first: they do not wait for the emit
        hipLaunchKernelGGL(sg_rk_state_pool, dim3(nw), dim3(64 * kBatchB), 0, s, d_rows_tab, pinned ? pool->h_pack_dev : d_state.p);
        if (!pinned)
            LOCREC_HIP_TRY(hipMemcpyAsync(own_state.data(), d_state.p, nw * kRkPoolStateStride, hipMemcpyDeviceToHost, s));
        for (size_t p = 0; p < parts; ++p) {
            hipLaunchKernelGGL(sg_rk_emit_pool, dim3(emit_blocks, nw), dim3(kRkThreads), 0, s, d_rows_tab + p * nw, d_req, d_req + n,
                               d_req + 2 * n, d_seg_begin, reinterpret_cast<unsigned long long *>(d_seg_len), rc.groups.max_rows,
                               rc.d_row_ids, rc.d_row_probs);
            ++stats.emit_launches;
            if (cuts[p + 1] == group_end[rc.group]) LOCREC_TRY(rc.flush_group());
        }
        LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (also: nothing reads the wave's tables any more)
        LOCREC_HIP_TRY(hipGetLastError());
        ++stats.host_syncs;
        stats.readback_bytes += (int64_t)(nw * kRkStateBytes);
        const unsigned char *host = pinned ? pool->h_pack : own_state.data();
        for (unsigned j = 0; j < nw; ++j) {
            const size_t f = order.ubase[present[j]] + w.k * (size_t)tile_max[present[j]];  // the tile's first column
            LOCREC_TRY(sg_rk_verdicts(host + j * kRkPoolStateStride, w.nb[j], eps2, max_iterations, &rc.res_it[f], &rc.res_conv[f]));
        }
        return LOCREC_OK;
    };
    const int32_t status = sg_pool_waves_of(pool, act, mem, tp, alpha, epsilon, max_iterations, ps, emit_and_rank);
    stats.tile_waves = ps.tile_waves;
    stats.rounds = ps.rounds;
    return rc.finish(status, ps.polls, order, member_of, uniq_of, out_ids, out_probabilities, out_counts, out_row_counts,
                     out_iterations, out_converged);
}

}  // namespace

extern "C" int32_t locrec_sg_pool_recommend_ranked_batch(
    locrec_sg_pool *pool, int64_t n_requests, const int32_t *graph_index, const int64_t *vertex_ids, double alpha, double epsilon,
    int64_t max_iterations, int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations, int64_t *out_ids, double *out_probabilities,
    int64_t *out_counts, int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged, int64_t *out_bad_request) try
{
    SgRkPoolStats &stats = sg_rk_pool_stats();
    stats = SgRkPoolStats();
    if (!pool) return fail(LOCREC_E_INVALID_ARG, "pool is NULL");
    if (n_requests < 0 || (n_requests > 0 && (!graph_index || !vertex_ids))) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    int64_t N = 0;
    LOCREC_TRY(sg_rk_check_args(n_requests, n_places, place_ids, place_region_ids, target_region_ids, max_recommendations, out_ids,
                                out_probabilities, out_counts, N));
    LOCREC_TRY(sg_batch_requires(epsilon, max_iterations));
    std::vector<SgPoolMember> mem;
    std::vector<int32_t> act, uniq_of;
    LOCREC_TRY(sg_pool_requests(pool, n_requests, graph_index, vertex_ids, mem, act, uniq_of, out_bad_request));
    if (n_requests == 0) return LOCREC_OK;
    if (max_iterations > INT32_MAX) max_iterations = INT32_MAX;
    LOCREC_TRY(sg_pool_begin_call(pool, act, mem));  // (sorts act: member order)
    // from here on the members' slots are the call's: whatever happens, sg_pool_end_call gives them back
    SgPoolStats ps;
    const int32_t status = sg_pool_ranked_columns(pool, stats, ps, act, mem, n_requests, graph_index, uniq_of, SgPoolPersonTiles{}, alpha,
                                                  epsilon, max_iterations, N, n_places, place_ids, place_region_ids, target_region_ids,
                                                  false, nullptr, 0, nullptr, out_ids, out_probabilities, out_counts, out_row_counts,
                                                  out_iterations, out_converged);
    // (a failed run may have left launches in flight that read the call's buffers, freed at run's end by hipFree, which
    // waits for the device)
    return sg_pool_end_call(pool, act, mem, status);
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_pool_recommend_ranked_batch_stats(int64_t *out_tile_waves, int64_t *out_tiles, int64_t *out_rounds,
                                                               int64_t *out_groups, int64_t *out_emit_launches,
                                                               int64_t *out_emitted_rows, int64_t *out_readback_bytes,
                                                               int64_t *out_host_syncs) try
{
    const SgRkPoolStats &st = sg_rk_pool_stats();
    if (out_tile_waves) *out_tile_waves = st.tile_waves;
    if (out_tiles) *out_tiles = st.tiles;
    if (out_rounds) *out_rounds = st.rounds;
    if (out_groups) *out_groups = st.groups;
    if (out_emit_launches) *out_emit_launches = st.emit_launches;
    if (out_emitted_rows) *out_emitted_rows = st.emitted_rows;
    if (out_readback_bytes) *out_readback_bytes = st.readback_bytes;
    if (out_host_syncs) *out_host_syncs = st.host_syncs;
    return LOCREC_OK;
} LOCREC_CATCH_ALL
