// sg_pool_visitors.h -- ONE mixed batch of SG visitors over a pool of resident graphs (locrec_sg_pool_visitors_*).
// Included at the end of sg_batch.hip, behind sg_pool_ranked.h and sg_visitors.h.
//
// Visitors fan out over region sets as persons do (StochasticRecommenderMain.scala:53-62): visitor v is asked of member
// graph_index[v] and is given by its out-edges, as in locrec_sg_visitors_recommend_batch.  The waves, sweeps, polls, packs
// and the restore launch are sg_pool_waves_of's (sg_pool.h); the per-column arithmetic is sg_finalize_batch_body<true> on
// the member's own tables - the single visitors call's - so visitor v's rows, iterations and converged flag are bit for
// bit what locrec_sg_visitors_recommend_batch returns for it on its member alone, whatever shares its call.
//
//   tile          kBatchB = 16 visitors whatever the member's column width; wave k of a member is its visitors
//                 16k .. 16k+15 in call order
//   staging       per call, before any launch (sg_pool_visitors_plan.h): every member's staged edges (row | col | slot | w)
//                 in ONE pair of device buffers with one set of copies; every asked member's slot table (T entries at -1)
//                 and weight table (the lines of its largest tile) carved from the same buffers, freed with the call
//   tables        beside the wave's SgPoolTile rows a row of SgPoolVisRow per member (sg_vis_set_up's arguments and the
//                 member's SgVisTables), in the pool's table buffer (sized at create): the wave's one copy carries them
//   set-up        ONE sg_vis_set_up_pool launch per wave behind sg_begin_pool, blockIdx.y = the member's table row:
//                 sg_vis_set_up's body on that member's tables.  A member whose visitors ran out has no row.
//   finalize      ONE sg_finalize_pool_visitors launch per round, grid (kParts, members of the wave)
//   ranked call   the ranked pool's consumer (sg_pool_ranked_columns) with nobody as every column's own vertex, one
//                 request per visitor, the exclusion lists uploaded in emit order (wave, member, column)
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (VGPRs / LDS bytes / scratch), beside
// sg_finalize_pool's 152 / 512 / 0, sg_finalize_visitors' 118 / 512 / 0 and sg_vis_set_up's 16 / 0 / 0:
//   sg_finalize_pool_visitors  117 / 512 / 0
//   sg_vis_set_up_pool         16 / 0 / 0
#pragma once

#include "sg_pool_visitors_plan.h"

namespace {

// A member's row of a visitors wave, beside its SgPoolTile row
struct SgPoolVisRow {
    SgVisSetUp su;
    SgVisTables vt;
};
static_assert(sizeof(SgPoolVisRow) == kSgPoolVisRowBytes, "the pool sizes its table buffer by this");

__global__ __launch_bounds__(256) void sg_vis_set_up_pool(const SgPoolVisRow *__restrict__ rows) { sg_vis_set_up_body(rows[blockIdx.y].su); }

__global__ __launch_bounds__(256) void sg_finalize_pool_visitors(const SgPoolTile *__restrict__ tiles,
                                                                 const SgPoolVisRow *__restrict__ vis, const int32_t par,
                                                                 const int32_t first)
{
    const SgPoolTile &t = tiles[blockIdx.y];
    sg_finalize_batch_body<true>(t.rq, (int)blockIdx.x, t.n_short, t.lrows, t.nlrows, t.n_crows, t.partial,
                                 t.xbuf + (size_t)par * t.xstride, t.xbuf + (size_t)(par ^ 1) * t.xstride,
                                 t.parts + (size_t)(par ^ 1) * kParts * kBatchB, t.parts + (size_t)par * kParts * kBatchB, t.st, first,
                                 vis[blockIdx.y].vt);
}

// what this thread's last pool visitors call did (locrec_sg_pool_visitors_stats, in this order)
struct SgPoolVisStats {
    int64_t tile_waves = 0, member_tiles = 0, visitors = 0, staged_edges = 0, stagings = 0, begin_launches = 0, set_up_launches = 0,
            rounds = 0, sweep_launches = 0, finalize_launches = 0, polls = 0, consumes = 0;
};

SgPoolVisStats &sg_pool_vis_stats()
{
    thread_local SgPoolVisStats st;
    return st;
}

// A call's visitors: checked, planned, staged
struct SgPoolVisitorsCall {
    SgPoolVisitorsPlan plan;
    std::vector<int32_t> entry_of;  // member of the pool -> its entry of plan.members (-1: nobody asks it)
    DevBuf<int32_t> d_i32;          // row | col | slot | the members' slot tables
    DevBuf<double> d_f64;           // w | the members' weight tables

    // Every graph index, then the visitors in call order, each against its own member: all before any device work.
    // *bad: the first offender's position.  (The CSR's shape and the require()s are checked: sg_visitors_check_shape.)
    int32_t check_and_plan(const locrec_sg_pool *pool, int64_t nv, const int32_t *graph_index, const int64_t *offsets,
                           const int64_t *target_ids, const double *weights, int64_t *bad)
    {
        LOCREC_TRY(sg_pool_graph_indices(pool, nv, graph_index, bad));
        const int64_t ne = nv > 0 ? offsets[nv] : 0;
        std::vector<int32_t> live((size_t)ne);
        for (int64_t v = 0; v < nv; ++v) {
            *bad = v;
            LOCREC_TRY(sg_visitor_check(pool->graphs[(size_t)graph_index[v]], v, offsets, target_ids, weights, live.data()));
        }
        *bad = -1;
        const int32_t ng = (int32_t)pool->graphs.size();
        std::vector<int32_t> nlive((size_t)ng);
        for (int32_t g = 0; g < ng; ++g) nlive[(size_t)g] = pool->graphs[(size_t)g]->nlive;
        sg_pool_visitors_plan(nv, graph_index, offsets, live.data(), weights, ng, nlive.data(), plan);
        entry_of.assign((size_t)ng, -1);
        for (size_t a = 0; a < plan.members.size(); ++a) entry_of[(size_t)plan.members[a].graph] = (int32_t)a;
        return LOCREC_OK;
    }

    // The members asked with their columns (nobody's vertex: -1 each), as sg_pool_requests leaves them for persons
    void members(const locrec_sg_pool *pool, std::vector<SgPoolMember> &mem, std::vector<int32_t> &act) const
    {
        mem = std::vector<SgPoolMember>(pool->graphs.size());
        act.clear();
        for (const SgPoolVisitorsMember &m : plan.members) {
            act.push_back(m.graph);
            mem[(size_t)m.graph].uniq.assign(m.count(), -1);  // a visitor is no vertex: never a row of its own result
        }
    }

    // the one staging of the call: four copies and the slot tables at -1, before the first wave
    int32_t upload(hipStream_t s)
    {
        const size_t ne = (size_t)plan.edges();
        LOCREC_TRY(d_i32.alloc((size_t)plan.words32));
        LOCREC_TRY(d_f64.alloc((size_t)plan.words64));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_i32.p, plan.row.data(), ne * 4, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_i32.p + ne, plan.col.data(), ne * 4, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_i32.p + 2 * ne, plan.slot.data(), ne * 4, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_f64.p, plan.w.data(), ne * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemsetAsync(d_i32.p + 3 * ne, 0xFF, ((size_t)plan.words32 - 3 * ne) * 4, s));
        return LOCREC_OK;
    }
};

// The columns of a pool visitors call's tiles (SgPoolPersonTiles' counterpart for sg_pool_waves_of)
struct SgPoolVisitorTiles {
    const SgPoolVisitorsCall &call;
    SgPoolVisStats &stats;
    int tile_max(const locrec_sg_graph *) const { return kBatchB; }
    void rows(int32_t, const locrec_sg_graph *g, SgPoolMember &m, size_t, size_t, int nb, double alpha, double eps2, SgBatchBegin &b,
              SgBatchReq &rq) const
    {
        sg_vis_tile_rows(g, nb, alpha, eps2, m.pointed, b, rq);
    }
    // row j of the wave's SgPoolVisRow table: member gi's tile k
    void member_row(locrec_sg_pool *pool, unsigned j, int32_t gi, size_t k) const
    {
        const SgPoolVisitorsMember &m = call.plan.members[(size_t)call.entry_of[(size_t)gi]];
        const size_t ne = (size_t)call.plan.edges();
        SgPoolVisRow &r = reinterpret_cast<SgPoolVisRow *>(pool->tab_host.data() + pool->off_vis)[j];
        r = SgPoolVisRow{};
        r.su.slot = call.d_i32.p + m.slot_off;
        r.su.w = call.d_f64.p + m.w_off;
        r.su.e_row = call.d_i32.p;
        r.su.e_col = call.d_i32.p + ne;
        r.su.e_slot = call.d_i32.p + 2 * ne;
        r.su.e_w = call.d_f64.p;
        r.su.p0 = k > 0 ? (int32_t)(m.edge_base + m.st.tile_ptr[k - 1]) : 0;
        r.su.p1 = k > 0 ? (int32_t)(m.edge_base + m.st.tile_ptr[k]) : 0;
        r.su.n0 = (int32_t)(m.edge_base + m.st.tile_ptr[k]);
        r.su.n1 = (int32_t)(m.edge_base + m.st.tile_ptr[k + 1]);
        r.su.lines = m.st.tile_slots[k];
        r.vt = SgVisTables{r.su.slot, r.su.w};
        ++stats.member_tiles;
    }
    size_t table_bytes(const locrec_sg_pool *pool, size_t, unsigned nw) const { return pool->off_vis + nw * sizeof(SgPoolVisRow); }
    void set_up(locrec_sg_pool *pool, hipStream_t s, unsigned nw) const
    {
        hipLaunchKernelGGL(sg_vis_set_up_pool, dim3(1, nw), dim3(256), 0, s,
                           reinterpret_cast<const SgPoolVisRow *>(pool->tab_dev.p + pool->off_vis));
        ++stats.set_up_launches;
    }
    void finalize(locrec_sg_pool *pool, hipStream_t s, unsigned nw, const SgPoolTile *tiles_dev, int par, int32_t first) const
    {
        hipLaunchKernelGGL(sg_finalize_pool_visitors, dim3(kParts, nw), dim3(256), 0, s, tiles_dev,
                           reinterpret_cast<const SgPoolVisRow *>(pool->tab_dev.p + pool->off_vis), par, first);
    }
};

void sg_pool_vis_begin_stats(SgPoolVisStats &stats, const SgPoolVisitorsCall &call, int64_t nv)
{
    stats.visitors = nv;
    stats.staged_edges = call.plan.edges();
    stats.stagings = 1;
}

void sg_pool_vis_end_stats(SgPoolVisStats &stats, const SgPoolStats &ps)
{
    stats.tile_waves = stats.begin_launches = stats.consumes = ps.tile_waves;
    stats.rounds = ps.rounds;
    stats.sweep_launches = ps.sweep_launches;
    stats.finalize_launches = ps.finalize_launches;
    stats.polls = ps.polls;
}

}  // namespace

extern "C" int32_t locrec_sg_pool_visitors_recommend_batch(locrec_sg_pool *pool, int64_t nv, const int32_t *graph_index,
                                                           const int64_t *edge_offsets, const int64_t *target_ids,
                                                           const double *weights, double alpha, double epsilon,
                                                           int64_t max_iterations, int64_t *out_offsets, int64_t *out_ids,
                                                           double *out_probs, int64_t *inout_capacity, int64_t *out_iterations,
                                                           int32_t *out_converged, int64_t *out_bad_visitor) try
{
    int64_t bad = -1;
    SgPoolVisStats &stats = sg_pool_vis_stats();
    stats = SgPoolVisStats();
    auto run = [&]() -> int32_t {
        if (!pool) return fail(LOCREC_E_INVALID_ARG, "pool is NULL");
        if ((nv > 0 && !graph_index) || !out_offsets || !inout_capacity) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
        LOCREC_TRY(sg_visitors_check_shape(nv, edge_offsets, target_ids, weights, epsilon, max_iterations));
        SgPoolVisitorsCall call;
        LOCREC_TRY(call.check_and_plan(pool, nv, graph_index, edge_offsets, target_ids, weights, &bad));
        if (nv == 0) {
            out_offsets[0] = 0;
            *inout_capacity = 0;
            return LOCREC_OK;
        }
        if (max_iterations > INT32_MAX) max_iterations = INT32_MAX;
        std::vector<SgPoolMember> mem;
        std::vector<int32_t> act;
        call.members(pool, mem, act);
        LOCREC_TRY(sg_pool_begin_call(pool, act, mem));
        // from here on the members' slots are the call's: whatever happens, sg_pool_end_call gives them back
        SgPoolStats ps;
        auto waves = [&]() -> int32_t {
            LOCREC_TRY(call.upload(pool->stream));
            sg_pool_vis_begin_stats(stats, call, nv);
            for (const int32_t gi : act) mem[(size_t)gi].res.resize(mem[(size_t)gi].uniq.size());
            const double eps2 = epsilon * epsilon;  // :40
            const SgPoolVisitorTiles tiles{call, stats};
            std::vector<unsigned char> own;  // the plain-copy path's images
            auto read_back = [&](const SgPoolWave &w) -> int32_t {
                return sg_pool_read_back(pool, w, mem, tiles, eps2, max_iterations, ps, own);
            };
            return sg_pool_waves_of(pool, act, mem, tiles, alpha, epsilon, max_iterations, ps, read_back);
        };
        const int32_t status = waves();
        sg_pool_vis_end_stats(stats, ps);
        // (a failed run may have left launches in flight that read the call's buffers, freed at the call's end by hipFree,
        // which waits for the device)
        LOCREC_TRY(sg_pool_end_call(pool, act, mem, status));
        return sg_batch_output(
            nv,
            [&](int64_t i) { return SgBatchRowRef{&mem[(size_t)graph_index[i]].res, (size_t)call.plan.rank_of[(size_t)i]}; },
            out_offsets, out_ids, out_probs, inout_capacity, out_iterations, out_converged);
    };
    const int32_t status = run();
    if (out_bad_visitor) *out_bad_visitor = bad;
    return status;
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_pool_visitors_recommend_ranked_batch(
    locrec_sg_pool *pool, int64_t nv, const int32_t *graph_index, const int64_t *edge_offsets, const int64_t *target_ids,
    const double *weights, double alpha, double epsilon, int64_t max_iterations, int64_t n_places, const int64_t *place_ids,
    const int64_t *place_region_ids, const int64_t *target_region_ids, int64_t max_recommendations, const int64_t *excluded_offsets,
    int64_t n_excluded, const int64_t *excluded_ids, int64_t *out_ids, double *out_probabilities, int64_t *out_counts,
    int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged, int64_t *out_bad_visitor) try
{
    int64_t bad = -1;
    SgPoolVisStats &stats = sg_pool_vis_stats();
    stats = SgPoolVisStats();
    SgRkPoolStats &rstats = sg_rk_pool_stats();
    rstats = SgRkPoolStats();
    auto run = [&]() -> int32_t {
        if (!pool) return fail(LOCREC_E_INVALID_ARG, "pool is NULL");
        if (nv > 0 && !graph_index) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
        LOCREC_TRY(sg_visitors_check_shape(nv, edge_offsets, target_ids, weights, epsilon, max_iterations));
        int64_t N = 0;
        LOCREC_TRY(sg_rk_check_args(nv, n_places, place_ids, place_region_ids, target_region_ids, max_recommendations, out_ids,
                                    out_probabilities, out_counts, N));
        const bool with_lists = excluded_offsets != nullptr;
        if (with_lists) LOCREC_TRY(sg_rk_check_lists(nv, excluded_offsets, n_excluded, excluded_ids));
        SgPoolVisitorsCall call;
        LOCREC_TRY(call.check_and_plan(pool, nv, graph_index, edge_offsets, target_ids, weights, &bad));
        if (nv == 0) return LOCREC_OK;
        if (max_iterations > INT32_MAX) max_iterations = INT32_MAX;
        std::vector<SgPoolMember> mem;
        std::vector<int32_t> act;
        call.members(pool, mem, act);
        LOCREC_TRY(sg_pool_begin_call(pool, act, mem));
        SgPoolStats ps;
        auto waves = [&]() -> int32_t {
            LOCREC_TRY(call.upload(pool->stream));
            sg_pool_vis_begin_stats(stats, call, nv);
            return sg_pool_ranked_columns(pool, rstats, ps, act, mem, nv, graph_index, call.plan.rank_of, SgPoolVisitorTiles{call, stats},
                                          alpha, epsilon, max_iterations, N, n_places, place_ids, place_region_ids, target_region_ids,
                                          with_lists, excluded_offsets, n_excluded, excluded_ids, out_ids, out_probabilities,
                                          out_counts, out_row_counts, out_iterations, out_converged);
        };
        const int32_t status = waves();
        sg_pool_vis_end_stats(stats, ps);
        return sg_pool_end_call(pool, act, mem, status);
    };
    const int32_t status = run();
    if (out_bad_visitor) *out_bad_visitor = bad;
    return status;
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_pool_visitors_stats(int64_t out[12]) try
{
    if (!out) return fail(LOCREC_E_INVALID_ARG, "out is NULL");
    const SgPoolVisStats &st = sg_pool_vis_stats();
    const int64_t v[12] = {st.tile_waves,      st.member_tiles, st.visitors,       st.staged_edges,      st.stagings, st.begin_launches,
                           st.set_up_launches, st.rounds,       st.sweep_launches, st.finalize_launches, st.polls,    st.consumes};
    std::copy(v, v + 12, out);
    return LOCREC_OK;
} LOCREC_CATCH_ALL
