// sg_host_layout.h -- the layout of a stochastic graph built from HOST arrays (locrec_sg_create and its two sharded
// forms), from the vertex ranking through the partial-slot maps, as plain C++: no HIP, no device call, no look at the
// environment (the two switches the layout depends on arrive as bools).  sg_host_build.h runs the phases below in order and
// uploads what they leave; tests/host/sg_host_layout_check.cpp compiles this header alone and holds every layout against
// a model that knows nothing of pieces, under a host sanitizer.  Every rule sg_layout_plan.h states - remainder class,
// long area, whole-wave rows, the piece plan with its two refusals, the id-table rule - is taken from there.
//
// Sharded handles: a row's AREA (short, or the long area behind 3T) follows its in-degree over ALL edges (gdeg), so the
// vertex set, the live order and n_short are the same on every shard; its full pieces and its remainder class follow
// the shard's own edges (deg).  sg_layout_plan() takes totals, so it serves both.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "sg_layout_plan.h"

namespace locrec {

// as the device sees them: int2, int4 and sg.hip's RowMeta (sg_host_build.h asserts the sizes and uploads through casts)
struct SgInt2 { int32_t x, y; };
struct SgInt4 { int32_t x, y, z, w; };
struct SgRowMeta { int32_t full_begin, nfull, rem; };  // first full piece, their number, the remainder's segment or -1

// A phase that refuses the graph returns the text of the refusal (nullptr: done); this one is the only one that is not
// an invalid argument
constexpr const char *kSgNoHostMemory = "host allocation failed";

// where the weight of an edge slot sits: fp64 [piece][half][lane][2], the slot's lane = k / 4, its element j = k % 4
inline int64_t sg_weight_offset(int64_t slot)
{
    const int k = (int)(slot % kSgPlanSlots), lane = k >> 2, j = k & 3;
    return slot - k + (j >> 1) * 128 + lane * 2 + (j & 1);
}

// The phases in the order they run.  A member is what a later phase (or the caller) reads, a local what one phase needs.
struct SgHostLayout {
    // the caller's arrays and the shard: this handle keeps the edges whose SOURCE vertex index (by_target: whose target's
    // LIVE index - the live rows are sorted by degree, so a stride spreads the heavy ones evenly) is congruent to
    // shard_index modulo shard_count
    int64_t ne;
    const int64_t *src, *dst;
    const double *w;
    int32_t shard_index, shard_count;
    bool by_target, env_no_dense_ids, env_fused;  // ... and the switches LOCREC_SG_NO_DENSE_IDS, LOCREC_SG_FUSED
    // rank_vertices: vertexes = distinct(source_id U target_id), StochasticRecommender.scala:42-49, ascending; the vertex
    // index of every edge's source / target; the in-degree over ALL edges (live set, a row's area)
    std::vector<int64_t> vid;
    int64_t nv = 0;
    std::vector<int32_t> cs, ct, gdeg;
    // live_order: vertex -> live index or -1, and back
    std::vector<int32_t> live_of, live_vertex;
    int32_t T = 0, n_short = 0;
    // piece_plan: the in-degree over this shard's edges; per row the absolute slot of remainder element 0 (or -1); per
    // piece its first segment (old contiguous numbering) and its class
    std::vector<int32_t> deg;
    SgLayoutPlan plan;
    std::vector<SgRowMeta> meta;
    std::vector<int64_t> rem_slot0;
    std::vector<SgInt2> pinfo, pinfo2;
    // scatter_edges: col [piece][lane][4], D = T where no edge sits or the source is not live; the weights through
    // sg_weight_offset; the CSR over all vertices of the slots of the out-edges of source-only vertices
    std::vector<int32_t> col, dead_slots;
    std::vector<double> wv, wv2;
    std::vector<int64_t> dead_ptr;
    // row_maps: segment / leader lane -> partial slot, -1 where no row owns it; the long area's rows (l, first slot,
    // nfull, has remainder), the n_crows whole-wave rows first
    std::vector<int32_t> seg_out, lane_out;
    std::vector<SgInt4> lrows, lrows_f;
    int32_t n_crows = 0;
    // fused_layout (LOCREC_SG_FUSED, one shard)
    bool fused_ok = false;
    std::vector<int32_t> seg_fa, col2, seg2;  // (lrows_f, pinfo2 and wv2 stand beside lrows, pinfo and wv)
    int64_t pa4 = 0, np2 = 0;
    bool owned(int64_t e) const { return (by_target ? live_of[ct[e]] : cs[e]) % shard_count == shard_index; }
    int32_t partial_slot(int32_t l, int j) const  // j-th partial slot of live row l
    {
        return l >= n_short ? sg_long_begin(plan.long_base, meta[l].full_begin, l) + j : 3 * l + j;
    }
    const char *rank_vertices(), *live_order(), *piece_plan();
    void scatter_edges(), row_maps(), fused_layout();
    const char *run()  // every phase; fused_layout only where it applies
    {
        if (const char *refusal = rank_vertices()) return refusal;
        if (const char *refusal = live_order()) return refusal;
        if (const char *refusal = piece_plan()) return refusal;
        scatter_edges();
        row_maps();
        if (shard_count == 1 && env_fused) fused_layout();
        return nullptr;
    }
};

// Ids that sit close together (the generator's and most real id spaces: categories, places, persons numbered one after
// the other) are ranked through a table over [min, max] - three linear passes - instead of sorting 2E ids and bisecting
// twice per edge (0.5 s of the 0.55 s locrec_sg_create took at cfg3); any other id space takes the sort.  Both give the
// same ascending `vid` and the same indices.
inline const char *SgHostLayout::rank_vertices()
{
    int64_t id_lo = INT64_MAX, id_hi = INT64_MIN;
    for (int64_t e = 0; e < ne; ++e) {
        id_lo = std::min(id_lo, std::min(src[e], dst[e]));
        id_hi = std::max(id_hi, std::max(src[e], dst[e]));
    }
    const uint64_t lo = (uint64_t)id_lo, id_span = ne > 0 ? (uint64_t)id_hi - lo : 0;  // (exact in unsigned arithmetic)
    const bool dense_ids = ne > 0 && sg_dense_ids(id_span, ne) && !env_no_dense_ids;
    std::vector<int32_t> rank_of;  // dense_ids: id - id_lo -> vertex index
    try {
        vid.resize((size_t)(2 * ne));
        if (dense_ids) rank_of.assign((size_t)id_span + 1, 0);
    } catch (...) {
        return kSgNoHostMemory;
    }
    if (dense_ids) {
        for (int64_t e = 0; e < ne; ++e) rank_of[(uint64_t)src[e] - lo] = rank_of[(uint64_t)dst[e] - lo] = 1;
        size_t k = 0;
        for (size_t i = 0; i <= (size_t)id_span; ++i)
            if (rank_of[i]) {
                rank_of[i] = (int32_t)k;
                vid[k++] = (int64_t)(lo + i);
            }
        vid.resize(k);
        vid.shrink_to_fit();
    } else {
        std::copy(dst, dst + ne, std::copy(src, src + ne, vid.begin()));
        std::sort(vid.begin(), vid.end());
        vid.erase(std::unique(vid.begin(), vid.end()), vid.end());
    }
    nv = (int64_t)vid.size();
    if (nv >= ((int64_t)1 << 31) - 2) return "too many vertices";
    const auto index_of = [&](int64_t id) {
        return dense_ids ? rank_of[(uint64_t)id - lo] : (int32_t)(std::lower_bound(vid.begin(), vid.end(), id) - vid.begin());
    };
    cs.resize((size_t)ne);
    ct.resize((size_t)ne);
    gdeg.assign((size_t)nv + 1, 0);
    for (int64_t e = 0; e < ne; ++e) {
        cs[e] = index_of(src[e]);
        ct[e] = index_of(dst[e]);
        ++gdeg[ct[e]];
    }
    return nullptr;
}

// live vertices, the rows outside the long area first (ascending id inside each kind): the first n_short rows are then
// treated uniformly (three row-major partial slots each)
inline const char *SgHostLayout::live_order()
{
    if (shard_count < 1 || shard_index < 0 || shard_index >= shard_count) return "bad shard specification";
    live_of.assign((size_t)nv, -1);
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t v = 0; v < nv; ++v)
            if (gdeg[v] > 0 && sg_in_long_area(gdeg[v]) == (pass == 1)) {
                live_of[v] = (int32_t)live_vertex.size();
                live_vertex.push_back((int32_t)v);
            }
        if (pass == 0) n_short = (int32_t)live_vertex.size();
    }
    T = (int32_t)live_vertex.size();
    return nullptr;
}

// piece plan over the live rows: full pieces first (row order), then remainder pieces by class 6 .. 0.  The per-row walk
// only counts; where every class and the long area begin is sg_layout_plan's, from the totals
inline const char *SgHostLayout::piece_plan()
{
    deg.assign((size_t)nv + 1, 0);
    for (int64_t e = 0; e < ne; ++e)
        if (owned(e)) ++deg[ct[e]];
    meta.resize((size_t)T);
    int32_t rows_of_class[kSgPlanClasses] = {};
    int64_t nfull_total = 0, full_before_short = 0;
    for (int32_t l = 0; l < T; ++l) {
        const int d = deg[live_vertex[l]];
        if (l == n_short) full_before_short = nfull_total;
        meta[l] = SgRowMeta{(int32_t)nfull_total, d / kSgPlanSlots, -1};
        nfull_total += d / kSgPlanSlots;
        if (d % kSgPlanSlots > 0) ++rows_of_class[sg_remainder_class(d % kSgPlanSlots)];
    }
    if (n_short == T) full_before_short = nfull_total;
    // (the plan takes 32-bit totals: a count of full pieces past them is refused like any other past 2^31 / 256 pieces)
    plan = sg_layout_plan(rows_of_class, (int32_t)std::min<int64_t>(nfull_total, INT32_MAX),
                          (int32_t)std::min<int64_t>(full_before_short, INT32_MAX), T, n_short);
    if (plan.status == SgPlanStatus::too_many_slots) return "graph too large for int32 slot ids";
    if (plan.status == SgPlanStatus::too_many_partials) return "graph too large for int32 partial slots";
    pinfo.resize((size_t)plan.np);
    for (int32_t p = 0; p < plan.nfull_total; ++p) pinfo[p] = SgInt2{p, 6};
    for (int c = kSgPlanClasses - 1; c >= 0; --c)
        for (int32_t p = plan.piece_begin[c]; p < (c > 0 ? plan.piece_begin[c - 1] : (int32_t)plan.np); ++p)
            pinfo[p] = SgInt2{plan.part_begin[c] + (p - plan.piece_begin[c]) * (64 >> c), c};
    rem_slot0.assign((size_t)T, -1);
    int32_t seg_used[kSgPlanClasses] = {};
    for (int32_t l = 0; l < T; ++l) {
        const int rem = deg[live_vertex[l]] % kSgPlanSlots;
        if (rem == 0) continue;
        const int c = sg_remainder_class(rem), segs_per_piece = 64 >> c;
        const int32_t s = seg_used[c]++;
        meta[l].rem = plan.part_begin[c] + s;
        rem_slot0[l] = (int64_t)(plan.piece_begin[c] + s / segs_per_piece) * kSgPlanSlots + (s % segs_per_piece) * (4 << c);
    }
    return nullptr;
}

// scatter the edges in edge-list order (stable within a row); remember where the out-edges of source-only vertices landed
inline void SgHostLayout::scatter_edges()
{
    col.assign((size_t)plan.nslots(), T);
    wv.assign((size_t)plan.nslots(), 0.0);
    dead_ptr.assign((size_t)nv + 1, 0);
    for (int64_t e = 0; e < ne; ++e)
        if (owned(e) && live_of[cs[e]] < 0) ++dead_ptr[cs[e] + 1];
    for (int64_t v = 0; v < nv; ++v) dead_ptr[v + 1] += dead_ptr[v];
    dead_slots.resize((size_t)dead_ptr[nv]);
    std::vector<int64_t> dcur(dead_ptr.begin(), dead_ptr.end() - 1);
    std::vector<int64_t> cursor((size_t)T, 0);  // edges placed so far in the row
    for (int64_t e = 0; e < ne; ++e) {
        if (!owned(e)) continue;
        const int32_t l = live_of[ct[e]], sl = live_of[cs[e]];
        const int64_t k = cursor[l]++, in_full = (int64_t)meta[l].nfull * kSgPlanSlots;
        const int64_t slot = k < in_full ? (int64_t)meta[l].full_begin * kSgPlanSlots + k : rem_slot0[l] + (k - in_full);
        col[slot] = sl >= 0 ? sl : T;
        if (sl < 0) dead_slots[dcur[cs[e]]++] = (int32_t)slot;
        wv[sg_weight_offset(slot)] = w[e];
    }
}

// row-major partial slots (3l + j for the first n_short rows, a contiguous run behind them for the others); seg_out maps
// a segment (old contiguous numbering: pinfo.x + seg; a full piece is its own segment) to its slot, lane_out does the
// same per leader lane for the persistent kernel
inline void SgHostLayout::row_maps()
{
    seg_out.assign((size_t)plan.npart, -1);
    for (int32_t l = 0; l < T; ++l) {
        const SgRowMeta &m = meta[l];
        for (int j = 0; j < m.nfull; ++j) seg_out[m.full_begin + j] = partial_slot(l, j);
        if (m.rem >= 0) seg_out[m.rem] = partial_slot(l, l >= n_short ? m.nfull : 2);
        if (l >= n_short) lrows.push_back(SgInt4{l, partial_slot(l, 0), m.nfull, m.rem >= 0 ? 1 : 0});
    }
    lane_out.assign((size_t)plan.np * 64, -1);
    for (int64_t p = 0; p < plan.np; ++p) {
        const int c = pinfo[p].y, segs = p < plan.nfull_total ? 1 : 64 >> c;
        for (int sgm = 0; sgm < segs; ++sgm) lane_out[p * 64 + (sgm << c)] = seg_out[pinfo[p].x + sgm];
    }
    // rows summed by a whole wave first, then one thread's (no slot moves: every entry carries its own first slot)
    const auto mid = std::stable_partition(lrows.begin(), lrows.end(), [](const SgInt4 &r) { return sg_wave_row(r.z); });
    n_crows = (int32_t)(mid - lrows.begin());
}

// fused iteration (sg_sweep_fused): its own slot map - four slots per short row, a run per longer row with the X slot at
// its end - and the second piece list: the edges whose SOURCE is a longer row, grouped by target row into one pow2
// segment each (at most 256 of them per row, or the handle keeps the two-launch form: fused_ok stays false).  An
// experiment (LOCREC_SG_FUSED), not the product path.
inline void SgHostLayout::fused_layout()
{
    std::vector<int32_t> xslot((size_t)T, -1), cnt2((size_t)T, 0);
    seg_fa.assign((size_t)plan.npart, -1);
    pa4 = 4 * (int64_t)n_short;
    for (int32_t l = 0; l < T; ++l) {
        const SgRowMeta &m = meta[l];
        const bool is_short = l < n_short;
        const int32_t first = is_short ? 4 * l : (int32_t)pa4;
        for (int j = 0; j < m.nfull; ++j) seg_fa[m.full_begin + j] = first + j;
        if (m.rem >= 0) seg_fa[m.rem] = first + (is_short ? 2 : m.nfull);
        xslot[l] = first + (is_short ? 3 : m.nfull + 1);
        if (is_short) continue;
        lrows_f.push_back(SgInt4{l, first, m.nfull, m.rem >= 0 ? 1 : 0});
        pa4 += m.nfull + 2;
    }
    std::stable_partition(lrows_f.begin(), lrows_f.end(), [](const SgInt4 &r) { return sg_wave_row(r.z); });
    // the second piece list
    for (int64_t e = 0; e < ne; ++e)
        if (live_of[cs[e]] >= n_short) ++cnt2[live_of[ct[e]]];
    if (pa4 >= ((int64_t)1 << 30)) return;
    int64_t seg_n[kSgPlanClasses] = {};
    for (int32_t l = 0; l < T; ++l) {
        if (cnt2[l] > kSgPlanSlots) return;
        if (cnt2[l] > 0) ++seg_n[sg_remainder_class(cnt2[l])];
    }
    fused_ok = true;
    int64_t piece0[kSgPlanClasses], segbase[kSgPlanClasses], nseg2 = 0;
    for (int c = 0; c < kSgPlanClasses; ++c) {  // (this list runs from class 0 up)
        piece0[c] = np2;
        segbase[c] = nseg2;
        const int64_t per = 64 >> c, pcs = (seg_n[c] + per - 1) / per;
        np2 += pcs;
        nseg2 += pcs * per;
    }
    col2.assign((size_t)np2 * kSgPlanSlots, -1);
    seg2.assign((size_t)nseg2, -1);
    wv2.assign((size_t)np2 * kSgPlanSlots, 0.0);
    pinfo2.resize((size_t)np2);
    for (int c = 0; c < kSgPlanClasses; ++c)
        for (int64_t p = piece0[c]; p < (c < 6 ? piece0[c + 1] : np2); ++p)
            pinfo2[p] = SgInt2{(int32_t)(segbase[c] + (p - piece0[c]) * (64 >> c)), c};
    std::vector<int64_t> slot0((size_t)T, -1);
    int64_t used[kSgPlanClasses] = {};
    for (int32_t l = 0; l < T; ++l) {
        if (cnt2[l] == 0) continue;
        const int c = sg_remainder_class(cnt2[l]);
        const int64_t sidx = used[c]++, per = 64 >> c;
        slot0[l] = (piece0[c] + sidx / per) * kSgPlanSlots + (sidx % per) * (4 << c);
        seg2[segbase[c] + sidx] = xslot[l];
    }
    for (int64_t e = 0; e < ne; ++e) {  // edge-list order inside a row, like the main pieces
        const int32_t sl = live_of[cs[e]];
        if (sl < n_short) continue;
        const int64_t slot = slot0[live_of[ct[e]]]++;
        col2[slot] = sl;
        wv2[sg_weight_offset(slot)] = w[e];
    }
}

}  // namespace locrec
