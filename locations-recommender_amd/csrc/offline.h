// offline.h -- what every offline device step shares (knn_build.hip, prep.hip, dedup.hip, rank_batch.hip's host side,
// region_sets.hip, sample.hip, sg_create_device.hip): the checked launch and the one-value read-back, the temporary
// storage of the rocPRIM calls, launch grids, the order-preserving keys of signed ids, the lower-bound bisection, the
// phase clock and the distinct ids of a column.  Nothing here knows about a caller's columns (prep_cols.h) or about
// places (place_grid.h).  Everything lives in an unnamed namespace: the text is shared, each translation unit compiles
// its own instance.  Every launch here AND in the units above goes through LOCREC_LAUNCH: a rejected launch is an
// error of the call that made it, not of whichever HIP call comes next (tests/test_offline_launches.py).
#pragma once

#include "dev_prims.h"

#include <algorithm>
#include <type_traits>

#include "common.h"

namespace {

using namespace locrec;

// rocPRIM temporary storage, grow-only, reused by the calls of one step
struct Temp {
    DevBuf<unsigned char> buf;
};

// rocPRIM's two-phase protocol: `call` names p_ and bytes_ as its first two arguments
#define LOCREC_PRIM(tmp, call_with_args)              \
    do {                                              \
        size_t bytes_ = 0;                            \
        void *p_ = nullptr;                           \
        LOCREC_HIP_TRY((call_with_args));             \
        LOCREC_TRY((tmp).buf.reserve(bytes_ + 256));  \
        p_ = (tmp).buf.p;                             \
        LOCREC_HIP_TRY((call_with_args));             \
    } while (0)

// The one way these units launch a kernel: launch, then return hipGetLastError's verdict with the site's file and line.
// `kern` may be a template instance.  What a unit tolerates to fail it clears on the spot, so nothing stale ends here.
#define LOCREC_LAUNCH(kern, grid, block, lds, stream, ...)                      \
    do {                                                                        \
        hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);        \
        LOCREC_HIP_TRY(hipGetLastError());                                      \
    } while (0)

// one value (or small struct, or array) from the device to the host, and wait for it
#define LOCREC_READ_BACK(dest, dev, stream)                                                                    \
    do {                                                                                                       \
        static_assert(!std::is_pointer_v<std::remove_reference_t<decltype(dest)>>, "the value, not its address"); \
        LOCREC_HIP_TRY(hipMemcpyAsync(&(dest), (dev), sizeof(dest), hipMemcpyDeviceToHost, (stream)));         \
        LOCREC_HIP_TRY(hipStreamSynchronize(stream));                                                          \
    } while (0)

// count elements in each of the buffers, in the order given; stops at the first failure
template <class... Bufs>
int32_t alloc_each(size_t count, Bufs &...bufs)
{
    int32_t st = LOCREC_OK;
    ((st = st == LOCREC_OK ? bufs.alloc(count) : st), ...);
    return st;
}

inline dim3 grid_for(int64_t n, int threads = 256) { return dim3((unsigned)std::max<int64_t>(1, (n + threads - 1) / threads)); }

// signed order as unsigned order: flipping the sign bit keeps the order and is its own inverse
constexpr uint64_t kSignBit = 0x8000000000000000ull;
__host__ __device__ __forceinline__ uint64_t ordered_key(int64_t v) { return (uint64_t)v ^ kSignBit; }
__host__ __device__ __forceinline__ int64_t id_of_key(uint64_t k) { return (int64_t)(k ^ kSignBit); }

// first position in [lo, hi) of the ascending a whose entry is not below key; hi if there is none
template <class T>
__device__ __forceinline__ int64_t lower_bound(const T *a, int64_t lo, int64_t hi, T key)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t lower_bound_key(const uint64_t *keys, int64_t n, uint64_t key)
{
    return lower_bound<uint64_t>(keys, 0, n, key);
}

// The three kernels below are [[maybe_unused]]: not every unit launches each of them.

// keys[i] = ordered_key(col[i]) and, where asked for, rows[i] = i: the first pass of a sort by id
[[maybe_unused]] __global__ void iota_keys(int64_t n, const int64_t *col, uint64_t *keys, uint32_t *rows)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = ordered_key(col[i]);
    if (rows) rows[i] = (uint32_t)i;
}

// keys[i] = ordered_key(col[rows[i]]): a later pass of a stable sort, or the keys of the sorted rows
[[maybe_unused]] __global__ void gather_id_keys(int64_t n, const int64_t *col, const uint32_t *rows, uint64_t *keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = ordered_key(col[rows[i]]);
}

[[maybe_unused]] __global__ void unkey_ids(int64_t n, const uint64_t *keys, int64_t *ids)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = id_of_key(keys[i]);
}

// HIP events at the phase changes of one call; read() adds every interval to the phase that began it (a negative
// phase is not counted)
struct PhaseClock {
    hipStream_t s = nullptr;
    std::vector<hipEvent_t> ev;
    std::vector<int> phase;
    ~PhaseClock()
    {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    int32_t mark(int ph)
    {
        hipEvent_t e;
        LOCREC_HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
        phase.push_back(ph);
        LOCREC_HIP_TRY(hipEventRecord(e, s));
        return LOCREC_OK;
    }
    int32_t read(double *ms)
    {
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        for (size_t i = 0; i + 1 < ev.size(); ++i) {
            float t = 0;
            LOCREC_HIP_TRY(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
            if (phase[i] >= 0) ms[phase[i]] += t;
        }
        return LOCREC_OK;
    }
};

// the distinct values of col[0 .. n), n >= 1, ascending in out[0 .. *count): sort, unique and un-key on the device;
// the only word that travels to the host is the count (the caller's limit on it comes next).  A template over the
// count's type (int32_t at every call) only so that a unit that does not call it instantiates no rocPRIM kernels.
template <class Count>
int32_t distinct_ids(const int64_t *col, int64_t n, Temp &tmp, hipStream_t s, DevBuf<int64_t> &out, Count *count)
{
    DevBuf<uint64_t> k0, k1;
    DevBuf<Count> count_dev;
    LOCREC_TRY(k0.alloc((size_t)n));
    LOCREC_TRY(k1.alloc((size_t)n));
    LOCREC_TRY(count_dev.alloc(1));
    LOCREC_LAUNCH(iota_keys, grid_for(n), dim3(256), 0, s, n, col, k0.p, (uint32_t *)nullptr);
    LOCREC_PRIM(tmp, prim::sort_keys(p_, bytes_, k0.p, k1.p, (size_t)n, 0, 64, s));
    LOCREC_PRIM(tmp, prim::unique(p_, bytes_, k1.p, k0.p, count_dev.p, (size_t)n, s));
    LOCREC_READ_BACK(*count, count_dev.p, s);
    LOCREC_TRY(out.alloc((size_t)*count));
    LOCREC_LAUNCH(unkey_ids, grid_for(*count), dim3(256), 0, s, (int64_t)*count, k0.p, out.p);
    LOCREC_HIP_TRY(hipStreamSynchronize(s));  // (the keys are released on return)
    return LOCREC_OK;
}

}  // namespace
