// place_grid.h -- what the two spatial joins share (prep.hip: calcPlaceVisits; dedup.hip: the place deduplicator):
// Location.scala's haversine, its range check and the report of a row that fails it, the per-region band / cell grid
// whose cells are at least one search radius wide, the keys of the gridded side and the walk of the other side over
// the up to 3 x 3 cells around a point.  Everything lives in an unnamed namespace (see offline.h).
#pragma once

#include "dev_prims.h"

#include <algorithm>
#include <cmath>

#include "common.h"
#include "prep_cols.h"

namespace {

using namespace locrec;

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

// rank of a region in the ascending region list, -1 when it is not listed
__device__ __forceinline__ int64_t rank_of_region(const int64_t *regions, int32_t nr, int64_t region)
{
    const int64_t at = lower_bound<int64_t>(regions, 0, nr, region);
    return at < nr && regions[at] == region ? at : -1;
}

__device__ __forceinline__ uint64_t cell_key(int64_t region_rank, int32_t band, int64_t cell)
{
    return ((uint64_t)region_rank << (2 * kCellBits)) | ((uint64_t)band << kCellBits) | (uint64_t)cell;
}

// keys of the gridded side, to be sorted with their rows
[[maybe_unused]] __global__ void pr_place_keys(int64_t np, const double *lat, const double *lon, const int64_t *region, const int64_t *regions,
                              int32_t nr, Grid g, uint64_t *keys, uint32_t *rows)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= np) return;
    rows[j] = (uint32_t)j;
    const int64_t r = rank_of_region(regions, nr, region[j]);
    if (!location_ok(lat[j], lon[j])) {  // never a match; reported by check_side_b if a row of the other side would meet it
        keys[j] = ~0ull;
        return;
    }
    const int32_t b = band_of(g, lat[j]);
    double win;
    int32_t nx;
    band_cells(g, b, &win, &nx);
    const double w = 360.0 / nx;
    const int32_t cx = min(max((int32_t)floor((lon[j] + 180.0) / w), 0), nx - 1);
    keys[j] = cell_key(r, b, cx);
}

// The walk of one point of the other side: f(row) for every keyed row in the (at most) 3 bands x 3 cells around
// (lat, lon) in the region of rank region_rank >= 0 - band by band, cell by cell, then the run of equal sorted keys.
// The caller's f does the exact distance test (and whatever else decides a match).
template <class F>
__device__ __forceinline__ void for_each_grid_candidate(const Grid &g, int64_t region_rank, double lat, double lon,
                                                        const uint64_t *keys, int64_t n, const uint32_t *rows, F f)
{
    const int32_t bv = band_of(g, lat);
    for (int32_t b = max(bv - 1, 0); b <= min(bv + 1, g.nbands - 1); ++b) {
        double win;
        int32_t nx;
        band_cells(g, b, &win, &nx);
        const double w = 360.0 / nx;
        const int64_t c_lo = (int64_t)floor((lon - win + 180.0) / w), c_hi = (int64_t)floor((lon + win + 180.0) / w);
        const int64_t ncell = min(c_hi - c_lo + 1, (int64_t)nx);
        for (int64_t t = 0; t < ncell; ++t) {
            const int64_t cx = ((c_lo + t) % nx + nx) % nx;  // cells wrap around the antimeridian
            const uint64_t key = cell_key(region_rank, b, cx);
            for (int64_t at = lower_bound_key(keys, n, key); at < n && keys[at] == key; ++at) f(rows[at]);
        }
    }
}

// the matches of one point, ascending: a point has few, an insertion sort orders them
__device__ __forceinline__ void sort_ascending(uint32_t *mine, unsigned long long count)
{
    for (unsigned long long a = 1; a < count; ++a) {
        const uint32_t v = mine[a];
        unsigned long long b = a;
        for (; b > 0 && mine[b - 1] > v; --b) mine[b] = mine[b - 1];
        mine[b] = v;
    }
}

// ---- Location's require (Location.scala:7-8) for every row that meets a row of the other side --------------------------

struct LocationError {
    unsigned long long first_bad_a, first_bad_b;  // rows; ~0 = none
};

// Side A: a row that takes part (ts == nullptr, or ts[i] >= from) and whose region is listed - the list is side B's -
// meets a row of side B: it marks its region, and its Location must be valid (the reference's UDF constructs both
// Locations for every joined pair)
[[maybe_unused]] __global__ void check_side_a(int64_t n, const int64_t *ts, int64_t from, const double *lat, const double *lon,
                             const int64_t *region, const int64_t *regions, int32_t nr, uint32_t *marked, LocationError *err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (ts && ts[i] < from)) return;
    const int64_t r = rank_of_region(regions, nr, region[i]);
    if (r < 0) return;
    marked[r] = 1u;
    if (!location_ok(lat[i], lon[i])) atomicMin(&err->first_bad_a, (unsigned long long)i);
}

// Side B: checked where a row of side A marked the region
[[maybe_unused]] __global__ void check_side_b(int64_t n, const double *lat, const double *lon, const int64_t *region, const int64_t *regions,
                             int32_t nr, const uint32_t *marked, LocationError *err)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t r = rank_of_region(regions, nr, region[j]);
    if (r >= 0 && marked[r] && !location_ok(lat[j], lon[j])) atomicMin(&err->first_bad_b, (unsigned long long)j);
}

// LOCREC_OK when no row failed; otherwise the reference's message for the first bad row (side A's before side B's) and
// *inout_count = -(1 + row) with side B's rows counted behind side A's n_a
inline int32_t location_error(const LocationError &e, const double *a_lat, const double *a_lon, const char *a_name, int64_t n_a,
                              const double *b_lat, const double *b_lon, const char *b_name, int64_t *inout_count)
{
    if (e.first_bad_a == ~0ull && e.first_bad_b == ~0ull) return LOCREC_OK;
    const bool a = e.first_bad_a != ~0ull;
    const int64_t row = (int64_t)(a ? e.first_bad_a : e.first_bad_b);
    double lat = 0, lon = 0;
    LOCREC_HIP_TRY(hipMemcpy(&lat, (a ? a_lat : b_lat) + row, 8, hipMemcpyDeviceToHost));
    LOCREC_HIP_TRY(hipMemcpy(&lon, (a ? a_lon : b_lon) + row, 8, hipMemcpyDeviceToHost));
    *inout_count = a ? -(1 + row) : -(1 + n_a + row);
    if (!(lat >= -90.0 && lat <= 90.0))
        return fail(LOCREC_E_INVALID_ARG, "requirement failed: Latitude %.17g must be within range [-90.0, 90.0] (%s %lld)", lat,
                    a ? a_name : b_name, (long long)row);
    return fail(LOCREC_E_INVALID_ARG, "requirement failed: Longitude %.17g must be within range [-180.0, 180.0] (%s %lld)", lon,
                a ? a_name : b_name, (long long)row);
}

}  // namespace
