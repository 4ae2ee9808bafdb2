// sg_visitors.h -- SG for visitors (included at the end of sg_batch.hip, behind sg_ranked.h): makeRecommendations for
// persons the resident graph G has no vertex for, each given by its out-edges (target_id, balanced_weight), without a
// rebuild (locrec_sg_visitors_recommend_batch, locrec_sg_visitors_recommend_ranked_batch).  A visitor's result is that of
// makeRecommendations(V) on G + v: G's edge list followed by (V, t_k, w_k), V an id no edge of G has.  A person who is a
// vertex of G and comes back as a visitor keeps that vertex, as the source-only vertex it is.
//
// Nothing points at a person (StochasticGraphBuilderMain.scala:47-66), so V is a source-only target whose out-edges are
// not in the layout: a column of a batch tile with the private row T + 1 + b (q_in_use, n_plain_dead = N - T: every
// source-only vertex of G holds D's value), x0 = 1 / (N + 1), and in the finalize one more product in the sum of every live
// row the visitor points at (batch_add_visitors, sg_batch.hip).  No out-edge slot is re-pointed and sg_sweep_batch runs as
// it is; no column index addresses a private row, so a tile holds kBatchB visitors whatever T and the column width.
//
//   tables    per call: slot[T] (int32, -1: no visitor of the tile points at the row) and w[lines][kBatchB] (fp64), the
//             lines of the call's largest tile.  A row with a slot adds w[slot][b] * x_V(b) in every column: one
//             128-byte line, +0.0 where column b's visitor has no edge to the row (the sum keeps its bits).
//   set-up    sg_vis_set_up, one block a tile behind sg_begin_batch: the previous tile's rows back to -1, the weight
//             lines to +0.0, then this tile's staged edges scattered (a (slot, column) pair is written once: a visitor
//             names a target once).  The tables are freed with the call.
//   staging   on the host before any device work (sg_visitors_plan.h): ids -> live rows, a tile's edges by live row.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (VGPRs / LDS bytes / scratch), beside
// sg_finalize_batch's 153 / 512 / 0:
//   sg_finalize_visitors  118 / 512 / 0
//   sg_vis_set_up         16 / 0 / 0
#pragma once

#include "sg_visitors_plan.h"

namespace {

// what this thread's last visitors call did (locrec_sg_visitors_stats)
struct SgVisitorsStats {
    int64_t tiles = 0, visitors = 0, staged_edges = 0, max_slots = 0, set_up_launches = 0, finalize_launches = 0, polls = 0,
            waits = 0;
};

SgVisitorsStats &sg_visitors_stats()
{
    thread_local SgVisitorsStats st;
    return st;
}

struct SgVisSetUp {
    int32_t *slot;  // [T]
    double *w;      // [lines][kBatchB]
    const int32_t *e_row, *e_col, *e_slot;  // the call's staged edges
    const double *e_w;
    int32_t p0, p1;  // the previous tile's edges (p0 == p1: none)
    int32_t n0, n1;  // this tile's
    int32_t lines;   // this tile's weight lines
};

// one block: the edges of a tile are a few hundred.  sg_vis_set_up_pool (sg_pool_visitors.h) runs the same body per member.
__device__ __forceinline__ void sg_vis_set_up_body(const SgVisSetUp &a)
{
    for (int i = a.p0 + (int)threadIdx.x; i < a.p1; i += 256) a.slot[a.e_row[i]] = -1;
    for (int i = (int)threadIdx.x; i < a.lines * kBatchB; i += 256) a.w[i] = 0.0;
    __syncthreads();  // (a row of both tiles: -1 first)
    for (int i = a.n0 + (int)threadIdx.x; i < a.n1; i += 256) {
        const int32_t sl = a.e_slot[i];
        a.slot[a.e_row[i]] = sl;  // (the edges of one row carry the same slot)
        a.w[(size_t)sl * kBatchB + a.e_col[i]] = a.e_w[i];
    }
}

__global__ __launch_bounds__(256) void sg_vis_set_up(const SgVisSetUp a) { sg_vis_set_up_body(a); }

__global__ __launch_bounds__(256) void sg_finalize_visitors(
    const SgBatchReq rq, int32_t n_short, const int4 *__restrict__ lrows, int32_t nlrows, int32_t n_crows,
    const double *__restrict__ partial, const double *__restrict__ x_in, double *__restrict__ x_out,
    const double *__restrict__ parts_prev, double *__restrict__ parts_out, SgBatchState *st, int32_t first, const SgVisTables vt)
{
    sg_finalize_batch_body<true>(rq, (int)blockIdx.x, n_short, lrows, nlrows, n_crows, partial, x_in, x_out, parts_prev, parts_out,
                                 st, first, vt);
}

// The shape of a visitors call's CSR and the constructor's two require()s (before any per-visitor check)
int32_t sg_visitors_check_shape(int64_t nv, const int64_t *offsets, const int64_t *target_ids, const double *weights, double epsilon,
                                int64_t max_iterations)
{
    if (nv < 0 || (nv > 0 && !offsets)) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    if (nv > 0) {
        bool ok = offsets[0] == 0;
        for (int64_t v = 0; ok && v < nv; ++v) ok = offsets[v] <= offsets[v + 1];
        if (!ok) return fail(LOCREC_E_INVALID_ARG, "edge_offsets must start at 0 and be non-decreasing");
        if (offsets[nv] > kSgVisitorsMaxEdges) return fail(LOCREC_E_INVALID_ARG, "2^31 visitor edges or more");
        if (offsets[nv] > 0 && (!target_ids || !weights)) return fail(LOCREC_E_INVALID_ARG, "null array");
    }
    return sg_batch_requires(epsilon, max_iterations);
}

// Visitor v of a call against the graph it is asked of: it has edges, every weight is finite, every target is a vertex
// with a row of the layout, none is named twice.  live[e] <- the live row of every edge of v.
int32_t sg_visitor_check(const locrec_sg_graph *g, int64_t v, const int64_t *offsets, const int64_t *target_ids, const double *weights,
                         int32_t *live)
{
    if (offsets[v] == offsets[v + 1]) return fail(LOCREC_E_NOT_FOUND, "visitor %lld has no edges", (long long)v);
    for (int64_t e = offsets[v]; e < offsets[v + 1]; ++e) {
        if (!std::isfinite(weights[e]))
            return fail(LOCREC_E_INVALID_ARG, "visitor %lld: the weight of its edge to %lld is not finite", (long long)v,
                        (long long)target_ids[e]);
        const int32_t tv = sg_vertex_index(g, target_ids[e]);
        if (tv < 0) return fail(LOCREC_E_NOT_FOUND, "No such vertex in the graph: %lld", (long long)target_ids[e]);
        if (g->live_of[tv] < 0)
            return fail(LOCREC_E_INVALID_ARG, "visitor %lld: vertex %lld has no inbound edge in the graph (the layout has no row for it)",
                        (long long)v, (long long)target_ids[e]);
        live[(size_t)e] = g->live_of[tv];
    }
    const int64_t rep = sg_visitors_first_repeat(live + offsets[v], offsets[v + 1] - offsets[v]);
    if (rep >= 0)
        return fail(LOCREC_E_INVALID_ARG, "visitor %lld names the target %lld twice", (long long)v,
                    (long long)target_ids[offsets[v] + rep]);
    return LOCREC_OK;
}

// The set-up and finalize rows of a tile of nb visitors on g: every column has its private row, nothing is re-pointed
void sg_vis_tile_rows(const locrec_sg_graph *g, int nb, double alpha, double eps2, std::vector<SlotRange> &pointed, SgBatchBegin &b,
                      SgBatchReq &rq)
{
    const int32_t T = g->nlive;
    sg_batch_restore_row(g, pointed, b);  // what a single request left pointing at its Q: back to D
    pointed.clear();
    b.x = g->PA4.p;
    b.parts = g->D2W.p;
    b.st = reinterpret_cast<SgBatchState *>(g->fused_conv.p);
    b.x0 = 1.0 / (double)(g->nv + 1);  // :51-54 on G + v
    b.nx = sg_batch_xstride(g);
    b.nb = nb;
    rq = SgBatchReq{};
    rq.nb = nb;
    rq.T = T;
    rq.alpha = alpha;
    rq.oma = 1 - alpha;  // :121
    rq.eps2 = eps2;
    for (int j = 0; j < nb; ++j) {
        rq.target_x[j] = T + 1 + j;
        rq.n_plain_dead[j] = (int32_t)(g->nv - T);
        rq.q_in_use[j] = 1;
    }
}

// A call's visitors, checked and staged; the device side of the stage and the tables
struct SgVisitorsCall {
    int64_t nv = 0;
    SgVisitorsStage st;
    DevBuf<int32_t> d_i32;  // e_row | e_col | e_slot | slot table
    DevBuf<double> d_f64;   // e_w | weight table
    int32_t *d_slot = nullptr;
    double *d_w = nullptr;

    // The refusals of a visitors call, all before any device work.  *bad: the first offending visitor.
    int32_t check_and_stage(locrec_sg_graph *g, int64_t n, const int64_t *offsets, const int64_t *target_ids, const double *weights,
                            double epsilon, int64_t max_iterations, int64_t *bad)
    {
        nv = n;
        LOCREC_TRY(sg_visitors_check_shape(nv, offsets, target_ids, weights, epsilon, max_iterations));
        if (const char *why = sg_batch_refusal(g)) return fail(LOCREC_E_INVALID_ARG, "%s", why);
        const int64_t ne = nv > 0 ? offsets[nv] : 0;
        std::vector<int32_t> live((size_t)ne);
        for (int64_t v = 0; v < nv; ++v) {
            *bad = v;
            LOCREC_TRY(sg_visitor_check(g, v, offsets, target_ids, weights, live.data()));
        }
        *bad = -1;
        sg_visitors_stage(nv, offsets, live.data(), weights, st);
        return LOCREC_OK;
    }

    // the stage to the device, the slot table at -1: everything a tile's set-up reads, allocated before the first tile
    int32_t upload(locrec_sg_graph *g)
    {
        LOCREC_HIP_TRY(hipSetDevice(g->device));
        hipStream_t s = g->stream;
        const size_t ne = (size_t)st.edges(), nslot = SgVisitorsStage::slot_table(g->nlive);
        LOCREC_TRY(d_i32.alloc(3 * ne + nslot));
        LOCREC_TRY(d_f64.alloc(ne + st.weight_table()));
        d_slot = d_i32.p + 3 * ne;
        d_w = d_f64.p + ne;
        LOCREC_HIP_TRY(hipMemcpyAsync(d_i32.p, st.row.data(), ne * 4, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_i32.p + ne, st.col.data(), ne * 4, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_i32.p + 2 * ne, st.slot.data(), ne * 4, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemcpyAsync(d_f64.p, st.w.data(), ne * 8, hipMemcpyHostToDevice, s));
        LOCREC_HIP_TRY(hipMemsetAsync(d_slot, 0xFF, nslot * 4, s));
        return LOCREC_OK;
    }
};

// The columns of a visitors call's tiles (SgPersonTiles' counterpart for sg_batch_tiles_of)
struct SgVisitorTiles {
    const SgVisitorsCall &call;
    SgVisitorsStats &stats;
    size_t count() const { return (size_t)call.nv; }
    int tile_max(const locrec_sg_graph *) const { return kBatchB; }
    void rows(const locrec_sg_graph *g, size_t, int nb, double alpha, double eps2, std::vector<SlotRange> &pointed, SgBatchBegin &b,
              SgBatchReq &rq) const
    {
        sg_vis_tile_rows(g, nb, alpha, eps2, pointed, b, rq);
    }
    void set_up(const locrec_sg_graph *, hipStream_t s, size_t t0) const
    {
        const size_t t = t0 / (size_t)kBatchB, ne = (size_t)call.st.edges();
        SgVisSetUp a{};
        a.slot = call.d_slot;
        a.w = call.d_w;
        a.e_row = call.d_i32.p;
        a.e_col = call.d_i32.p + ne;
        a.e_slot = call.d_i32.p + 2 * ne;
        a.e_w = call.d_f64.p;
        a.p0 = t > 0 ? (int32_t)call.st.tile_ptr[t - 1] : 0;
        a.p1 = t > 0 ? (int32_t)call.st.tile_ptr[t] : 0;
        a.n0 = (int32_t)call.st.tile_ptr[t];
        a.n1 = (int32_t)call.st.tile_ptr[t + 1];
        a.lines = call.st.tile_slots[t];
        hipLaunchKernelGGL(sg_vis_set_up, dim3(1), dim3(256), 0, s, a);
        ++stats.set_up_launches;
    }
    void polled() const { ++stats.polls; }
    void finalize(const locrec_sg_graph *g, hipStream_t s, const SgBatchReq &rq, const double *x_in, double *x_out,
                  const double *parts_prev, double *parts_out, SgBatchState *bstate, int32_t first) const
    {
        hipLaunchKernelGGL(sg_finalize_visitors, dim3(kParts), dim3(256), 0, s, rq, g->n_short, g->lrows.p, g->nlrows, g->n_crows,
                           g->XL.p, x_in, x_out, parts_prev, parts_out, bstate, first, SgVisTables{call.d_slot, call.d_w});
        ++stats.finalize_launches;
    }
};

void sg_visitors_begin_stats(SgVisitorsStats &stats, const SgVisitorsCall &call)
{
    stats = SgVisitorsStats();
    stats.visitors = call.nv;
    stats.tiles = call.st.tiles();
    stats.staged_edges = call.st.edges();
    stats.max_slots = call.st.max_slots;
}

}  // namespace

extern "C" int32_t locrec_sg_visitors_recommend_batch(locrec_sg_graph *g, int64_t nv, const int64_t *edge_offsets,
                                                      const int64_t *target_ids, const double *weights, double alpha,
                                                      double epsilon, int64_t max_iterations, int64_t *out_offsets, int64_t *out_ids,
                                                      double *out_probs, int64_t *inout_capacity, int64_t *out_iterations,
                                                      int32_t *out_converged, int64_t *out_bad_visitor) try
{
    int64_t bad = -1;
    SgVisitorsStats &stats = sg_visitors_stats();
    stats = SgVisitorsStats();
    auto run = [&]() -> int32_t {
        if (!g) return fail(LOCREC_E_INVALID_ARG, "graph is NULL");
        if (!out_offsets || !inout_capacity) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
        SgVisitorsCall call;
        LOCREC_TRY(call.check_and_stage(g, nv, edge_offsets, target_ids, weights, epsilon, max_iterations, &bad));
        if (nv == 0) {
            out_offsets[0] = 0;
            *inout_capacity = 0;
            return LOCREC_OK;
        }
        sg_visitors_begin_stats(stats, call);
        LOCREC_TRY(call.upload(g));
        const std::vector<int32_t> nobody((size_t)nv, -1);  // a visitor is no vertex: never a row of its own result
        SgBatchRows res;
        res.resize((size_t)nv);
        auto read_back = [&](SgBatchCtx &ctx, size_t t0, int nb) -> int32_t {
            ++stats.waits;
            return sg_batch_read_back(g, ctx, nobody, t0, nb, res);
        };
        SgBatchCtx ctx;
        const int32_t status = sg_batch_tiles_of(g, SgVisitorTiles{call, stats}, alpha, epsilon, max_iterations, ctx, read_back);
        stats.waits += stats.polls;
        LOCREC_TRY(status);
        return sg_batch_output(nv, [&](int64_t i) { return SgBatchRowRef{&res, (size_t)i}; }, out_offsets, out_ids, out_probs,
                               inout_capacity, out_iterations, out_converged);
    };
    const int32_t status = run();
    if (out_bad_visitor) *out_bad_visitor = bad;
    return status;
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_visitors_recommend_ranked_batch(
    locrec_sg_graph *g, int64_t nv, const int64_t *edge_offsets, const int64_t *target_ids, const double *weights, double alpha,
    double epsilon, int64_t max_iterations, int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations, const int64_t *excluded_offsets, int64_t n_excluded,
    const int64_t *excluded_ids, int64_t *out_ids, double *out_probabilities, int64_t *out_counts, int64_t *out_row_counts,
    int64_t *out_iterations, int32_t *out_converged, int64_t *out_bad_visitor) try
{
    int64_t bad = -1;
    SgVisitorsStats &stats = sg_visitors_stats();
    stats = SgVisitorsStats();
    SgRankedStats &rstats = sg_ranked_stats();
    rstats = SgRankedStats();
    auto run = [&]() -> int32_t {
        if (!g) return fail(LOCREC_E_INVALID_ARG, "graph is NULL");
        if (nv < 0) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
        int64_t N = 0;
        LOCREC_TRY(sg_rk_check_args(nv, n_places, place_ids, place_region_ids, target_region_ids, max_recommendations, out_ids,
                                    out_probabilities, out_counts, N));
        const bool with_lists = excluded_offsets != nullptr;
        if (with_lists) LOCREC_TRY(sg_rk_check_lists(nv, excluded_offsets, n_excluded, excluded_ids));
        SgVisitorsCall call;
        LOCREC_TRY(call.check_and_stage(g, nv, edge_offsets, target_ids, weights, epsilon, max_iterations, &bad));
        if (nv == 0) return LOCREC_OK;
        sg_visitors_begin_stats(stats, call);
        LOCREC_TRY(call.upload(g));
        const std::vector<int32_t> nobody((size_t)nv, -1);
        std::vector<int32_t> column_of((size_t)nv);
        std::iota(column_of.begin(), column_of.end(), 0);
        const int32_t status = sg_ranked_batch_columns(
            g, rstats, nv, nobody, column_of, SgVisitorTiles{call, stats}, alpha, epsilon, max_iterations, N, n_places, place_ids,
            place_region_ids, target_region_ids, with_lists, excluded_offsets, n_excluded, excluded_ids, out_ids, out_probabilities,
            out_counts, out_row_counts, out_iterations, out_converged);
        stats.waits = rstats.host_syncs;
        return status;
    };
    const int32_t status = run();
    if (out_bad_visitor) *out_bad_visitor = bad;
    return status;
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_vertex_kinds(const locrec_sg_graph *g, int64_t n, const int64_t *vertex_ids, int32_t *out_kinds) try
{
    if (!g) return fail(LOCREC_E_INVALID_ARG, "graph is NULL");
    if (n < 0 || (n > 0 && (!vertex_ids || !out_kinds))) return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    for (int64_t i = 0; i < n; ++i) {
        const int32_t tv = sg_vertex_index(g, vertex_ids[i]);
        out_kinds[i] = tv < 0 ? 0 : (g->live_of[tv] < 0 ? 1 : 2);
    }
    return LOCREC_OK;
} LOCREC_CATCH_ALL

extern "C" int32_t locrec_sg_visitors_stats(int64_t out[8]) try
{
    if (!out) return fail(LOCREC_E_INVALID_ARG, "out is NULL");
    const SgVisitorsStats &st = sg_visitors_stats();
    const int64_t v[8] = {st.tiles, st.visitors, st.staged_edges, st.max_slots, st.set_up_launches, st.finalize_launches, st.polls,
                          st.waits};
    std::copy(v, v + 8, out);
    return LOCREC_OK;
} LOCREC_CATCH_ALL
