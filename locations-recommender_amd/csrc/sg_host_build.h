// sg_host_build.h -- sg_create_impl: a locrec_sg_graph from HOST arrays (locrec_sg_create and its two sharded forms).
// Included by sg.hip behind the handle.  The layout itself is sg_host_layout.h's (plain C++, checked stand-alone by
// tests/host/sg_host_layout_check.cpp); what is left here is the handle, the uploads in a fixed order - resident buffers
// before temporaries - and the steps shared with the device build (sg_build_shared.h).
#pragma once

#include "sg_build_shared.h"
#include "sg_host_layout.h"

namespace {

static_assert(sizeof(SgInt2) == sizeof(int2) && sizeof(SgInt4) == sizeof(int4) && sizeof(SgRowMeta) == sizeof(RowMeta),
              "sg_host_layout.h's plain structs are uploaded as the device's, through casts like col and wv");

struct HostBuild {  // the phases, in the order sg_create_impl runs them
    std::unique_ptr<locrec_sg_graph> g;  // the handle under construction (first: its stream outlives the vectors it uploads)
    SgHostLayout L;
    int ncu = 0;
    int32_t open(locrec_sg_graph **out), layout(), upload_edges(), upload_tables(), upload_fused(), persistent_form();
};

int32_t HostBuild::open(locrec_sg_graph **out)
{
    if (!out) return fail(LOCREC_E_INVALID_ARG, "out_graph is NULL");
    *out = nullptr;
    if (L.ne < 0 || (L.ne > 0 && (!L.src || !L.dst || !L.w))) return fail(LOCREC_E_INVALID_ARG, "bad edge arrays");
    LOCREC_TRY(ensure_device());
    g.reset(new (std::nothrow) locrec_sg_graph);
    if (!g) return fail(LOCREC_E_OOM, "host allocation failed");
    LOCREC_HIP_TRY(hipGetDevice(&g->device));
    LOCREC_HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    g->own_stream = true;
    g->ne = L.ne;
    sg_read_env(g.get());
    L.env_no_dense_ids = g->env_no_dense_ids;
    L.env_fused = g->env_fused;
    return LOCREC_OK;
}

// the whole layout on the host, and what the handle keeps of it there
int32_t HostBuild::layout()
{
    if (const char *refusal = L.run()) return fail(refusal == kSgNoHostMemory ? LOCREC_E_OOM : LOCREC_E_INVALID_ARG, "%s", refusal);
    g->nv = L.nv;
    g->shard_index = L.shard_index;
    g->shard_count = L.shard_count;
    g->nlive = L.T;
    g->n_short = L.n_short;
    g->npieces = (int32_t)L.plan.np;
    g->nlong = g->n_crows = L.n_crows;  // (rows with more than kLongRow full pieces: all of them sit in the long area)
    g->nlrows = (int32_t)L.lrows.size();
    g->pa_stride = (int32_t)L.plan.pa;
    g->use16 = sg_use16(L.T) && !g->env_no_col16;
    g->vid.swap(L.vid);
    g->live_of.swap(L.live_of);
    g->live_vertex.swap(L.live_vertex);
    g->dead_ptr.swap(L.dead_ptr);
    g->dead_slots.swap(L.dead_slots);
    return LOCREC_OK;
}

int32_t HostBuild::upload_edges()
{
    if (g->use16) {
        std::vector<unsigned short> col16(L.col.size());
        for (size_t i = 0; i < L.col.size(); ++i) col16[i] = (unsigned short)L.col[i];
        LOCREC_TRY(g->col16.upload(col16, g->stream));
        LOCREC_HIP_TRY(hipStreamSynchronize(g->stream));  // (col16 is a local)
    } else {
        LOCREC_TRY(g->col4.upload(reinterpret_cast<const int4 *>(L.col.data()), (size_t)L.plan.np * 64, g->stream));
    }
    return g->w2.upload(reinterpret_cast<const double2 *>(L.wv.data()), (size_t)L.plan.np * 128, g->stream);
}

// pieces, work buffers, dead slots, the fused experiment's tables, the partial-slot maps: in this order
int32_t HostBuild::upload_tables()
{
    LOCREC_TRY(g->pinfo.upload(reinterpret_cast<const int2 *>(L.pinfo.data()), L.pinfo.size(), g->stream));
    LOCREC_TRY(g->xbuf.alloc((size_t)(2 * (L.T + 2))));
    LOCREC_TRY(g->parts.alloc(2 * kParts));
    LOCREC_TRY(g->state.alloc(1));
    if (g->dead_slots.size() > (size_t)INT32_MAX) return fail(LOCREC_E_INVALID_ARG, "too many out-edges of source-only vertices");
    LOCREC_TRY(g->dead_slots_dev.upload(g->dead_slots, g->stream));
    LOCREC_TRY(upload_fused());
    LOCREC_TRY(g->seg_out.upload(L.seg_out, g->stream));
    LOCREC_TRY(g->lrows.upload(reinterpret_cast<const int4 *>(L.lrows.data()), L.lrows.size(), g->stream));
    LOCREC_TRY(g->PA.alloc((size_t)(2 * L.plan.pa)));
    LOCREC_HIP_TRY(hipMemsetAsync(g->PA.p, 0, g->PA.bytes(), g->stream));
    LOCREC_HIP_TRY(hipStreamSynchronize(g->stream));
    return LOCREC_OK;
}

// the second layout of the fused iteration, where the layout took it (one shard, <= 256 long-source edges per row)
int32_t HostBuild::upload_fused()
{
    g->fused_ok = g->use_fused = L.fused_ok;
    if (!L.fused_ok) return LOCREC_OK;
    g->pa4 = (int32_t)std::max<int64_t>(1, L.pa4);
    g->npieces2 = (int32_t)L.np2;
    g->nduty = std::max(1, (L.n_short + 63) / 64);
    LOCREC_TRY(g->seg_fa.upload(L.seg_fa, g->stream));
    LOCREC_TRY(g->lrows_f.upload(reinterpret_cast<const int4 *>(L.lrows_f.data()), L.lrows_f.size(), g->stream));
    LOCREC_TRY(g->col2.upload(L.col2, g->stream));
    LOCREC_TRY(g->seg2.upload(L.seg2, g->stream));
    LOCREC_TRY(g->pinfo2.upload(reinterpret_cast<const int2 *>(L.pinfo2.data()), L.pinfo2.size(), g->stream));
    LOCREC_TRY(g->w2b.upload(reinterpret_cast<const double2 *>(L.wv2.data()), (size_t)L.np2 * 128, g->stream));
    LOCREC_TRY(g->PA4.alloc((size_t)4 * g->pa4));
    LOCREC_TRY(g->XL.alloc((size_t)4 * std::max(1, L.T - L.n_short)));
    LOCREC_TRY(g->D2W.alloc((size_t)4 * (g->nduty + kParts)));
    LOCREC_TRY(g->fused_conv.alloc(2));
    // (slots no kernel writes - a remainder or X slot of a row without one - stay 0.0 for good)
    LOCREC_HIP_TRY(hipMemsetAsync(g->PA4.p, 0, g->PA4.bytes(), g->stream));
    LOCREC_HIP_TRY(hipMemsetAsync(g->XL.p, 0, g->XL.bytes(), g->stream));
    LOCREC_HIP_TRY(hipMemsetAsync(g->D2W.p, 0, g->D2W.bytes(), g->stream));
    LOCREC_HIP_TRY(hipStreamSynchronize(g->stream));
    if (!g->fused_one_stream) LOCREC_HIP_TRY(hipStreamCreateWithFlags(&g->stream2, hipStreamNonBlocking));
    return LOCREC_OK;
}

// the persistent form (LOCREC_SG_PERSIST: opt-in, see the note above sg_persistent): x in LDS, one block per compute unit
int32_t HostBuild::persistent_form()
{
    const size_t lds = (size_t)(L.T + 2) * 8;
    g->persist_ok = L.shard_count == 1 && g->persist_pw > 0 && lds <= 128 * 1024 && ncu > 0 && g->env_persist;
    if (!g->persist_ok) return LOCREC_OK;
    g->persist_blocks = ncu;
    g->persist_lds = lds;
    LOCREC_TRY(g->lane_out.upload(L.lane_out, g->stream));
    LOCREC_TRY(g->barrier.alloc(1));
    if (debug_env("LOCREC_SG_DEBUG_PHASES")) LOCREC_TRY(g->dbg.alloc(4));
    LOCREC_HIP_TRY(hipStreamSynchronize(g->stream));
    return LOCREC_OK;
}

int32_t sg_create_impl(int64_t ne, const int64_t *src, const int64_t *dst, const double *w, int32_t shard_index,
                       int32_t shard_count, bool by_target, locrec_sg_graph **out)
{
    HostBuild b{nullptr, {ne, src, dst, w, shard_index, shard_count, by_target, false, false}};
    LOCREC_TRY(b.open(out));
    LOCREC_TRY(b.layout());
    sg_poll_word(b.g.get());
    b.ncu = sg_compute_units_and_grid(b.g.get());
    LOCREC_TRY(b.upload_edges());
    LOCREC_TRY(sg_weight_dictionary(b.g.get(), b.L.plan.np));
    LOCREC_TRY(b.upload_tables());
    sg_closing_figures(b.g.get(), b.L.plan.np, b.L.plan.npart, b.ncu);
    LOCREC_TRY(b.persistent_form());
    LOCREC_HIP_TRY(hipStreamSynchronize(b.g->stream));
    std::vector<int32_t>().swap(b.g->dead_slots);  // resident on the device now (dead_slots_dev); dead_ptr stays on the host
    *out = b.g.release();
    return LOCREC_OK;
}

}  // namespace
