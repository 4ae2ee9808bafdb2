// place_grid.h -- what the two spatial joins share (prep.hip: calcPlaceVisits; dedup.hip: the place deduplicator):
// Location.scala's haversine and range check, and the per-region
// band / cell grid whose cells are at least one search radius wide.  Included by both translation units;
// everything lives in an unnamed namespace, so each unit gets its own copy.
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

}  // namespace
