// sg_build_shared.h -- what both builders of a locrec_sg_graph do to the handle once its columns and weights are
// resident: the host build (sg_host_build.h) and the device build (sg_create_device.hip) call these, so the poll word,
// the weight dictionary and the closing figures exist once.  Included by sg.hip behind the handle and sg_read_env, where
// the host build always stood: the dictionary's rocPRIM kernels are instantiated at this place of the unit.  That is
// also why the one launch and the one read-back below are written out instead of taken from offline.h: that header
// defines kernels, and included here it would move them in front of sg.hip's own in the unit's code object.
#pragma once

#include "sg_layout_plan.h"

namespace {

// the pinned word the packed requests poll; without one the handle polls through copies (as under LOCREC_SG_NO_PACK)
void sg_poll_word(locrec_sg_graph *g)
{
    if (g->no_pack) return;
    void *hp = nullptr, *dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocDefault) == hipSuccess && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
        g->h_poll = static_cast<int32_t *>(hp);
        g->h_poll_dev = static_cast<int32_t *>(dp);
    } else {
        (void)hipGetLastError();
        if (hp) (void)hipHostFree(hp);
        g->no_pack = true;
    }
}

// the compute units of the handle's device (0 where the device does not say: no later launch check must report it)
// and, under LOCREC_SG_GS, the grid of the grid-stride sweep
int sg_compute_units_and_grid(locrec_sg_graph *g)
{
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess) (void)hipGetLastError();
    if (g->env_gs > 0) g->gs_blocks = g->env_gs * std::max(1, ncu);
    return ncu;
}

// The dictionary of the edge weights, built on the device from the resident w2 of np pieces: their bit patterns sorted
// (rocPRIM radix sort) and run-length encoded; when there are at most kDictMax distinct ones the table is ordered by
// FREQUENCY (the lanes of a wave mostly ask for the common values: the 32 most common ones then sit in 32 different
// LDS bank pairs) and every slot's index found by bisection in the sorted values (sg_build_widx).  (A host pass with a
// hash table took 37 ms of a 100 ms create at cfg3; this takes ~2.)
int32_t sg_weight_dictionary(locrec_sg_graph *g, int64_t np)
{
    if (g->env_no_dict || np == 0) return LOCREC_OK;
    const size_t nslots = (size_t)np * kSlots;
    hipStream_t s = g->stream;
    DevBuf<uint64_t> ka, kb;
    DevBuf<unsigned int> counts;
    DevBuf<int32_t> nuniq;
    DevBuf<unsigned char> storage;
    LOCREC_TRY(g->widx.alloc(nslots));  // (before the temporaries: what stays resident is allocated first)
    LOCREC_TRY(g->dict.alloc(kDictMax));
    LOCREC_TRY(ka.alloc(nslots));
    LOCREC_TRY(kb.alloc(nslots));
    LOCREC_TRY(counts.alloc(nslots));
    LOCREC_TRY(nuniq.alloc(1));
    LOCREC_HIP_TRY(hipMemcpyAsync(ka.p, g->w2.p, nslots * 8, hipMemcpyDeviceToDevice, s));
    size_t b1 = 0, b2 = 0;  // (not LOCREC_PRIM: both calls are sized before the one allocation)
    LOCREC_HIP_TRY(prim::sort_keys(nullptr, b1, ka.p, kb.p, nslots, 0u, 64u, s));
    LOCREC_HIP_TRY(prim::run_length_encode(nullptr, b2, kb.p, nslots, ka.p, counts.p, nuniq.p, s));
    LOCREC_TRY(storage.alloc(std::max(b1, b2)));
    LOCREC_HIP_TRY(prim::sort_keys(storage.p, b1, ka.p, kb.p, nslots, 0u, 64u, s));
    LOCREC_HIP_TRY(prim::run_length_encode(storage.p, b2, kb.p, nslots, ka.p, counts.p, nuniq.p, s));
    int32_t nu = 0;
    LOCREC_HIP_TRY(hipMemcpyAsync(&nu, nuniq.p, sizeof(nu), hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    if (!sg_dict_fits(nu)) {
        g->widx.release();
        g->dict.release();
        return LOCREC_OK;
    }
    std::vector<uint64_t> vals((size_t)nu);
    std::vector<unsigned int> cnt((size_t)nu);
    LOCREC_HIP_TRY(hipMemcpyAsync(vals.data(), ka.p, (size_t)nu * 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(cnt.data(), counts.p, (size_t)nu * 4, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    std::vector<int32_t> order((size_t)nu);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return cnt[(size_t)a] > cnt[(size_t)b]; });
    std::vector<double> dict_h((size_t)nu);
    std::vector<unsigned short> rank_h((size_t)nu);  // position in the sorted values -> table index
    for (int32_t r = 0; r < nu; ++r) {
        std::memcpy(&dict_h[(size_t)r], &vals[(size_t)order[(size_t)r]], 8);
        rank_h[(size_t)order[(size_t)r]] = (unsigned short)r;
    }
    DevBuf<unsigned short> rank;
    LOCREC_HIP_TRY(hipMemcpyAsync(g->dict.p, dict_h.data(), (size_t)nu * 8, hipMemcpyHostToDevice, s));
    LOCREC_TRY(rank.upload(rank_h, s));
    hipLaunchKernelGGL(sg_build_widx, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const double *>(g->w2.p), (int64_t)nslots, ka.p, rank.p, nu, g->widx.p);
    LOCREC_HIP_TRY(hipGetLastError());  // (offline.h's LOCREC_LAUNCH written out, see the head)
    LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (locals)
    g->ndict = nu;
    return LOCREC_OK;
}

// the byte figures bench.py reports and the pieces per wave of the persistent form
void sg_closing_figures(locrec_sg_graph *g, int64_t np, int64_t npart, int ncu)
{
    g->layout_bytes = sg_layout_bytes(np, g->nlive);
    g->device_sweep_bytes = sg_device_sweep_bytes(np, npart, g->nlive, g->use16, g->ndict > 0);
    g->persist_pw = sg_persist_pw(np, ncu);  // (8 and 16 pieces per wave spill registers: not built)
}

}  // namespace
