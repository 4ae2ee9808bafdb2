// prep_cols.h -- the column layer of the producers (prep.hip, dedup.hip, rank_batch.hip, region_sets.hip): the columns
// of one call in host or device memory (In, Out, mem_ok), the row limit of a u32 sort payload and the order-preserving
// key of a score.  The plumbing below it (temporary storage, grids, id keys, bisection) is offline.h.  Everything lives
// in an unnamed namespace: the text is shared, each translation unit compiles its own instance.
#pragma once

#include "offline.h"

namespace {

using namespace locrec;

constexpr int64_t kMaxRows = (int64_t)1 << 31;  // row numbers travel as u32 sort payloads

// An input column: the caller's array, on the device.  Host arrays are uploaded into `own`.
template <class T>
struct In {
    DevBuf<T> own;
    const T *p = nullptr;
    int32_t bind(const T *src, int64_t n, int32_t mem, hipStream_t s)
    {
        if (mem == LOCREC_MEM_DEVICE || n == 0) {
            p = src;
            return LOCREC_OK;
        }
        LOCREC_TRY(own.upload(src, (size_t)n, s));
        p = own.p;
        return LOCREC_OK;
    }
};

// An output column: the caller's device array, or a staging buffer copied back to the host array.
template <class T>
struct Out {
    DevBuf<T> own;
    T *p = nullptr;
    T *host = nullptr;
    int32_t bind(T *dst, int64_t cap, int32_t mem)
    {
        if (mem == LOCREC_MEM_DEVICE) {
            p = dst;
            return LOCREC_OK;
        }
        host = dst;
        LOCREC_TRY(own.alloc((size_t)std::max<int64_t>(cap, 1)));
        p = own.p;
        return LOCREC_OK;
    }
    int32_t deliver(int64_t count, hipStream_t s)
    {
        if (host && count > 0) LOCREC_HIP_TRY(hipMemcpyAsync(host, p, (size_t)count * sizeof(T), hipMemcpyDeviceToHost, s));
        return LOCREC_OK;
    }
};

// Spark SQL's order of doubles: every NaN, whatever its sign and payload, is one value above
// +inf, and -0.0 equals 0.0 - so both are made one bit pattern before the usual monotone map
__device__ __forceinline__ uint64_t score_desc_key(double s)
{
    uint64_t b = (uint64_t)__double_as_longlong(s);
    if (s != s) b = 0x7FF8000000000000ull;
    else if (s == 0.0) b = 0ull;
    b = (b >> 63) ? ~b : b | kSignBit;  // ascending order of the doubles
    return ~b;                          // ... descending
}

inline int32_t mem_ok(int32_t mem)
{
    if (mem != LOCREC_MEM_HOST && mem != LOCREC_MEM_DEVICE) return fail(LOCREC_E_INVALID_ARG, "mem must be LOCREC_MEM_HOST or LOCREC_MEM_DEVICE");
    return LOCREC_OK;
}

}  // namespace
