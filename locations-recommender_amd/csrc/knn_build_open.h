// knn_build_open.h -- how both KNN builders begin (knn_build_device, knn_create_host): argument checks, the handle with
// its stream, slices and switches, the handle's part of the format decision's input (knn_format_plan.h), the lap timer.
#pragma once

#include <chrono>
#include <memory>
#include <new>

#include "knn_format_plan.h"
#include "knn_index.h"

namespace locrec {

// LOCREC_DEBUG_TIMING: laps of one build on stderr; the device build waits for its stream first (sync), the host build not
struct KnnBuildLap {
    const char *label;
    hipStream_t sync;
    bool on = debug_env("LOCREC_DEBUG_TIMING") != nullptr;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void operator()(const char *what)
    {
        if (!on) return;
        if (sync && hipStreamSynchronize(sync) != hipSuccess) (void)hipGetLastError();  // (tolerated: cleared)
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[locrec %s] %-30s %.3f s\n", label, what, std::chrono::duration<double>(now - last).count());
        last = now;
    }
};

inline int32_t knn_build_open(int64_t n, const int64_t *ids, const int64_t *p_ptr, const int64_t *c_ptr, int32_t p_dim, int32_t c_dim,
                              locrec_knn_index **out, std::unique_ptr<locrec_knn_index> &ix, KnnFormatInput &in)
{
    if (!out) return fail(LOCREC_E_INVALID_ARG, "out_index is NULL");
    *out = nullptr;
    if (n < 0 || n >= ((int64_t)1 << 31) - 64) return fail(LOCREC_E_INVALID_ARG, "bad person count");
    if (n > 0 && (!ids || !p_ptr || !c_ptr)) return fail(LOCREC_E_INVALID_ARG, "NULL input array");
    if (p_dim <= 0 || c_dim <= 0) return fail(LOCREC_E_INVALID_ARG, "vector sizes must be positive");
    LOCREC_TRY(ensure_device());
    ix.reset(new (std::nothrow) locrec_knn_index);
    if (!ix) return fail(LOCREC_E_OOM, "host allocation failed");
    LOCREC_HIP_TRY(hipGetDevice(&ix->device));
    LOCREC_HIP_TRY(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
    ix->own_stream = true;
    ix->n = n;
    ix->nslices = (int32_t)((n + 63) / 64);
    ix->cand_slice0 = 0;
    ix->cand_slice1 = ix->nslices;
    knn_read_env(ix.get());
    // the format decision's input as far as the handle and the sizes give it; validation adds integral, all, narrow
    in.n = n;
    in.p_dim = p_dim;
    in.c_dim = c_dim;
    in.sw = {ix->force_generic, ix->no_row_fallback, ix->no_pack16, ix->no_ht, ix->no_pop, ix->force_hash, ix->env_ht_h, ix->env_pop_h};
    in.lim = {cfg::kHtHead, cfg::kHtQt, cfg::kHtCatRows, cfg::kPopTable, cfg::kDirectMaxBytes};
    return LOCREC_OK;
}

}  // namespace locrec
