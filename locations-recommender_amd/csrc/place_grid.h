// place_grid.h -- what the two spatial joins share (prep.hip: calcPlaceVisits; dedup.hip: the place deduplicator):
// the column helpers of the producers, Location.scala's haversine and range check, and the per-region
// band / cell grid whose cells are at least one search radius wide.  Included by both translation units;
// everything lives in an unnamed namespace, so each unit gets its own copy.
#pragma once

#include "dev_prims.h"

#include <algorithm>
#include <cmath>

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

__global__ void pr_iota_keys(int64_t n, const int64_t *col, uint64_t *keys, uint32_t *rows)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = ordered_key(col[i]);
    rows[i] = (uint32_t)i;
}

constexpr double kEarthRadiusMeters = 6371.0 * 1000.0;  // Location.scala:28
constexpr double kPi = 3.14159265358979323846;
constexpr int kCellBits = 20;                            // bands and cells per band: < 2^20 each; regions < 2^24

__device__ __forceinline__ double to_radians(double deg) { return deg / 180.0 * kPi; }

__device__ __forceinline__ double haversine(double theta)  // Location.scala:40-43
{
    const double sn = sin(theta / 2);
    return sn * sn;
}

__device__ double distance_meters(double lat1d, double lon1d, double lat2d, double lon2d)  // Location.scala:30-38
{
    const double lat1 = to_radians(lat1d), lat2 = to_radians(lat2d);
    const double lon1 = to_radians(lon1d), lon2 = to_radians(lon2d);
    const double h1 = haversine(lat2 - lat1);
    const double cc = cos(lat1) * cos(lat2);
    const double h2 = cc * haversine(lon2 - lon1);
    const double hav = h1 + h2;
    return (kEarthRadiusMeters * 2) * asin(sqrt(hav));
}

__device__ __forceinline__ bool location_ok(double lat, double lon)  // Location.scala:7-8 (NaN fails the require)
{
    return lat >= -90.0 && lat <= 90.0 && lon >= -180.0 && lon <= 180.0;
}

// The grid.  Latitude bands of `band_deg` degrees (>= the search radius as an angle, so a match lies in
// the visit's band or a neighbouring one).  Band b is cut into nx(b) longitude cells of 360 / nx(b)
// degrees, at least as wide as the largest longitude difference a match can have when the place is in
// band b and the visit in bands b - 1 .. b + 1:  hav(d / R) >= cos(lat1) cos(lat2) hav(dlon)  =>
// sin(dlon / 2) <= sin(d / 2R) / cos(latmax).  Near the poles that bound exceeds 1: one cell.
struct Grid {
    double band_deg, sin_half;  // sin(d / 2R), with a 1e-9 relative safety margin
    int32_t nbands;
};

// the grid of one search radius, 0 <= max_meters < kEarthRadiusMeters
inline Grid make_grid(double max_meters)
{
    Grid g;
    const double ang = max_meters / kEarthRadiusMeters;                       // the radius as an angle
    g.band_deg = std::max(ang * (180.0 / kPi) * (1.0 + 1e-9) + 1e-12, 180.0 / (double)((1 << kCellBits) - 2));
    g.nbands = (int32_t)std::floor(180.0 / g.band_deg) + 1;
    g.sin_half = std::sin(ang / 2) * (1.0 + 1e-9);
    return g;
}

__device__ __forceinline__ int32_t band_of(const Grid &g, double lat)
{
    const int32_t b = (int32_t)floor((lat + 90.0) / g.band_deg);
    return min(max(b, 0), g.nbands - 1);
}

// longitude half-window (degrees) and cell count of band b
__device__ __forceinline__ void band_cells(const Grid &g, int32_t b, double *half_window_deg, int32_t *nx)
{
    const double lo = -90.0 + (b - 1) * g.band_deg, hi = -90.0 + (b + 2) * g.band_deg;
    const double latmax = fmin(fmax(fabs(lo), fabs(hi)), 90.0);
    const double c = cos(to_radians(latmax));
    double win = 180.0;
    if (c > 0.0) {
        const double ratio = g.sin_half / c;
        if (ratio < 1.0) win = fmin(180.0, 2.0 * asin(ratio) * (180.0 / kPi) * (1.0 + 1e-9) + 1e-12);
    }
    *half_window_deg = win;
    *nx = (int32_t)fmin(fmax(floor(360.0 / win), 1.0), (double)((1 << kCellBits) - 1));
}

__device__ __forceinline__ int64_t rank_of_region(const int64_t *regions, int32_t nr, int64_t region)
{
    int32_t lo = 0, hi = nr;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (regions[mid] < region) lo = mid + 1; else hi = mid;
    }
    return lo < nr && regions[lo] == region ? lo : -1;
}

__global__ void pr_place_keys(int64_t np, const double *lat, const double *lon, const int64_t *region, const int64_t *regions,
                              int32_t nr, Grid g, uint64_t *keys, uint32_t *rows)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= np) return;
    rows[j] = (uint32_t)j;
    const int64_t r = rank_of_region(regions, nr, region[j]);
    if (!location_ok(lat[j], lon[j])) {  // never a match; reported by pr_check_places if a visit would meet it
        keys[j] = ~0ull;
        return;
    }
    const int32_t b = band_of(g, lat[j]);
    double win;
    int32_t nx;
    band_cells(g, b, &win, &nx);
    const double w = 360.0 / nx;
    const int32_t cx = min(max((int32_t)floor((lon[j] + 180.0) / w), 0), nx - 1);
    keys[j] = ((uint64_t)r << (2 * kCellBits)) | ((uint64_t)b << kCellBits) | (uint64_t)cx;
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
