// prep_cols.h -- what every producer translation unit shares (prep.hip, dedup.hip, rank_batch.hip): the columns of
// one call in host or device memory, the temporary storage of the rocPRIM calls, and the order-preserving keys of ids
// and scores.  Everything lives in an unnamed namespace, so each unit gets its own copy.
#pragma once

#include "dev_prims.h"

#include <algorithm>

#include "common.h"

namespace {

using namespace locrec;

struct Temp {
    DevBuf<unsigned char> buf;
};

#define PR_PRIM(tmp, call_with_args)                   \
    do {                                              \
        size_t bytes_ = 0;                            \
        void *p_ = nullptr;                           \
        LOCREC_HIP_TRY((call_with_args));             \
        LOCREC_TRY((tmp).buf.reserve(bytes_ + 256));  \
        p_ = (tmp).buf.p;                             \
        LOCREC_HIP_TRY((call_with_args));             \
    } while (0)

dim3 grid_for(int64_t n, int threads = 256) { return dim3((unsigned)std::max<int64_t>(1, (n + threads - 1) / threads)); }

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

__device__ __forceinline__ uint64_t ordered_key(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }  // signed order

// Spark SQL's order of doubles: every NaN, whatever its sign and payload, is one value above
// +inf, and -0.0 equals 0.0 - so both are made one bit pattern before the usual monotone map
__device__ __forceinline__ uint64_t score_desc_key(double s)
{
    uint64_t b = (uint64_t)__double_as_longlong(s);
    if (s != s) b = 0x7FF8000000000000ull;
    else if (s == 0.0) b = 0ull;
    b = (b >> 63) ? ~b : b | 0x8000000000000000ull;  // ascending order of the doubles
    return ~b;                                       // ... descending
}

__global__ void pr_iota_keys(int64_t n, const int64_t *col, uint64_t *keys, uint32_t *rows)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = ordered_key(col[i]);
    rows[i] = (uint32_t)i;
}

__device__ __forceinline__ int64_t lower_bound_key(const uint64_t *keys, int64_t n, uint64_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

int32_t mem_ok(int32_t mem)
{
    if (mem != LOCREC_MEM_HOST && mem != LOCREC_MEM_DEVICE) return fail(LOCREC_E_INVALID_ARG, "mem must be LOCREC_MEM_HOST or LOCREC_MEM_DEVICE");
    return LOCREC_OK;
}

}  // namespace
