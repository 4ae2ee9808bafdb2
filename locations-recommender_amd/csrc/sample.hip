// sample.hip -- the reference's sample generator on the device:
//
//   LocationVisitsSampleGenerator.generatePersons                 sample/LocationVisitsSampleGenerator.scala:55-68
//       locrec_sample_persons
//   ... withVisits / withGeoLocations / withTimestamps            sample/LocationVisitsSampleGenerator.scala:78-133
//       locrec_sample_location_visits (+ _stats)
//   PlacesSampleGenerator.withGeo / withCategories                sample/PlacesSampleGenerator.scala:41-77
//       locrec_sample_places
//   PlacesSampleGenerator.withNames                               sample/PlacesSampleGenerator.scala:79-90
//       locrec_sample_place_names
//
// The random numbers are synth.u01(seed, stream, row, slot) restated in integer arithmetic: a
// splitmix64 chain keyed stream -> row -> slot, the stream key computed on the host, the row key once per person.
// Spark's rand() values cannot be reproduced (parity unpinned); what is kept is the structure of the tables.
//
// The visits are per-person counts, one exclusive scan, and a fill with ONE ROW PER THREAD: the thread finds its person
// by bisection in the scanned offsets, so every column is written by consecutive lanes to consecutive addresses (8 bytes
// a lane, 4 for year_month) whatever the persons' counts are - handing a person's 1 to 365 rows to a wave instead
// would leave most lanes idle for short persons.  Arrays are host or device memory (`mem`) as for the other producers
// (prep_cols.h); region and category tables are always host memory.  Every floating-point step is one IEEE operation
// (the Makefile's -ffp-contract=off keeps them apart).

#include "dev_prims.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>

#include "common.h"
#include "prep_cols.h"

namespace {

using namespace locrec;

constexpr int64_t kSmMaxRegions = (int64_t)1 << 24;  // as the other producers: at most 2^24 - 1 regions
constexpr int64_t kSmMsPerHour = 3'600'000;
constexpr int64_t kSmMsPerDay = 86'400'000;
constexpr int64_t kSmMaxAbsMs = 8'640'000'000'000'000;  // +-100,000,000 days around 1970: the year stays far inside int32
constexpr int kSmStreamVisitCount = 1, kSmStreamVisit = 2, kSmStreamCategory = 3;

// ---- synth.u01 in integer arithmetic ------------------------------------------------------------------------------

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

inline uint64_t stream_key(uint64_t seed, uint64_t stream) { return splitmix64(seed ^ (stream * 0xD1342543DE82EF95ull)); }
__device__ __forceinline__ uint64_t row_key(uint64_t skey, uint64_t row) { return splitmix64(skey ^ row); }
// (k >> 11) has 53 bits: the conversion and the scaling by 2^-53 are exact
__device__ __forceinline__ double u01_of(uint64_t rkey, uint64_t slot)
{
    const uint64_t k = splitmix64(rkey ^ (slot * 0xA24BAED4963EE407ull));
    return (double)(k >> 11) * (1.0 / 9007199254740992.0);
}

// ---- the regions of a call: checked on the host, sorted by id for the device's bisection ---------------------------

struct Regions {
    std::vector<int64_t> sorted_ids;   // ascending
    std::vector<int32_t> order;        // sorted position -> position in the caller's list
};

int32_t check_regions(int32_t n_regions, const int64_t *region_ids, Regions &R)
{
    if (n_regions <= 0 || n_regions >= kSmMaxRegions) return fail(LOCREC_E_INVALID_ARG, "n_regions %d out of range [1, 2^24)", n_regions);
    if (!region_ids) return fail(LOCREC_E_INVALID_ARG, "region_ids is required");
    R.order.resize((size_t)n_regions);
    std::iota(R.order.begin(), R.order.end(), 0);
    std::sort(R.order.begin(), R.order.end(), [&](int32_t a, int32_t b) { return region_ids[a] < region_ids[b]; });
    R.sorted_ids.resize((size_t)n_regions);
    for (int32_t i = 0; i < n_regions; ++i) R.sorted_ids[(size_t)i] = region_ids[R.order[(size_t)i]];
    if (R.sorted_ids[0] < 0) return fail(LOCREC_E_INVALID_ARG, "negative region id %lld", (long long)R.sorted_ids[0]);
    for (int32_t i = 1; i < n_regions; ++i)
        if (R.sorted_ids[(size_t)i] == R.sorted_ids[(size_t)i - 1])
            return fail(LOCREC_E_INVALID_ARG, "region id %lld is listed twice", (long long)R.sorted_ids[(size_t)i]);
    return LOCREC_OK;
}

// boxes: [n_regions][4] = minLat, maxLat, minLon, maxLon
int32_t check_boxes(int32_t n_regions, const double *boxes)
{
    if (!boxes) return fail(LOCREC_E_INVALID_ARG, "region_boxes is required");
    for (int32_t r = 0; r < n_regions; ++r) {
        const double *b = boxes + 4 * (size_t)r;
        const bool ok = std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2]) && std::isfinite(b[3]) && b[0] <= b[1] &&
                        b[2] <= b[3] && b[0] >= -90.0 && b[1] <= 90.0 && b[2] >= -180.0 && b[3] <= 180.0;
        if (!ok)
            return fail(LOCREC_E_INVALID_ARG, "region %d: the box must be finite with min <= max inside [-90, 90] x [-180, 180]", r);
    }
    return LOCREC_OK;
}

// first + (last_index) * step for the largest id of a range, without leaving int64
bool fits_i64(__int128 v) { return v >= (__int128)std::numeric_limits<int64_t>::min() && v <= (__int128)std::numeric_limits<int64_t>::max(); }

// ---- persons ------------------------------------------------------------------------------------------------------

// row i: region i / ppr of the given list, id = min_person_id + region id * ppr + i % ppr
__global__ void sm_persons(int64_t total, int64_t ppr, const int64_t *region_ids, int64_t min_person_id, int64_t *out_ids,
                           int64_t *out_home)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t r = region_ids[i / ppr];
    out_ids[i] = min_person_id + r * ppr + i % ppr;
    out_home[i] = r;
}

// ---- location visits ----------------------------------------------------------------------------------------------

// per person: the rank of its home region in the sorted list, the key of its visit stream and its number of rows,
// (int)(f * max_visits) + 1.  A home region that is not listed: no rows, and the smallest such person row in *bad.
__global__ void sm_visit_counts(int64_t np, const int64_t *home, int64_t index_base, const int64_t *regions, int32_t nr,
                                uint64_t count_skey, uint64_t visit_skey, double max_visits, unsigned long long *counts,
                                uint64_t *visit_keys, int32_t *rank, unsigned long long *bad)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const int64_t h = home[p];
    const int64_t lo = lower_bound<int64_t>(regions, 0, nr, h);
    if (lo >= nr || regions[lo] != h) {
        counts[p] = 0ull;
        rank[p] = -1;
        visit_keys[p] = 0ull;
        atomicMin(bad, (unsigned long long)p);
        return;
    }
    const uint64_t row = (uint64_t)index_base + (uint64_t)p;
    const double f = u01_of(row_key(count_skey, row), 0ull);
    counts[p] = (unsigned long long)((int64_t)(f * max_visits) + 1);
    visit_keys[p] = row_key(visit_skey, row);
    rank[p] = (int32_t)lo;
}

// year * 100 + month of a day number (days since 1970-01-01, any sign) in the proleptic Gregorian calendar: the
// civil-from-days computation over 400-year eras, every division a floor division
__device__ __forceinline__ int32_t year_month_of_days(int64_t z)
{
    z += 719468;  // days from 0000-03-01 to 1970-01-01
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const int64_t doe = z - era * 146097;                                        // [0, 146096]
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;   // [0, 399]
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                 // [0, 365], the year begins in March
    const int64_t mp = (5 * doy + 2) / 153;                                      // [0, 11]
    const int64_t m = mp < 10 ? mp + 3 : mp - 9;
    const int64_t y = yoe + era * 400 + (m <= 2 ? 1 : 0);
    return (int32_t)(y * 100 + m);
}

// one row per thread; offsets[p] = first row of person p (strictly ascending: every person has a row)
__global__ void __launch_bounds__(256)
sm_visit_fill(int64_t rows, int64_t np, const unsigned long long *offsets, const uint64_t *visit_keys, const int32_t *rank,
              const int64_t *person_ids, const int64_t *home, const double *boxes, int64_t from_ms, double interval_hours,
              int32_t shared, int64_t *out_person, int64_t *out_region, double *out_lat, double *out_lon, int64_t *out_ts,
              int32_t *out_ym)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    // the last person whose first row is not beyond i
    const int64_t p = lower_bound<unsigned long long>(offsets, 0, np, (unsigned long long)i + 1ull) - 1;
    const uint64_t k = (uint64_t)i - offsets[p];
    const uint64_t key = visit_keys[p];
    const double *b = boxes + 4 * (int64_t)rank[p];
    const double g_lat = u01_of(key, 3ull * k);
    const double g_lon = shared ? g_lat : u01_of(key, 3ull * k + 1ull);
    const double g_t = shared ? g_lat : u01_of(key, 3ull * k + 2ull);
    const int64_t ts = from_ms + (int64_t)(interval_hours * g_t) * kSmMsPerHour;
    out_person[i] = person_ids[p];
    out_region[i] = home[p];
    out_lat[i] = b[0] + (b[1] - b[0]) * g_lat;
    out_lon[i] = b[2] + (b[3] - b[2]) * g_lon;
    out_ts[i] = ts;
    out_ym[i] = year_month_of_days((ts >= 0 ? ts : ts - (kSmMsPerDay - 1)) / kSmMsPerDay);
}

struct SampleStats {
    int64_t rows = 0, bytes = 0;
    double ms[2] = {0, 0};  // counts and scan, fill
};
thread_local SampleStats g_sample_stats;

constexpr int64_t kSmVisitRowBytes = 5 * 8 + 4;

// ---- places -------------------------------------------------------------------------------------------------------

// geo: [n_regions][4] = minLat, latStep, minLon, lonStep (the steps divided on the host).  Row i: region i / c^2 of the
// given list, grid cell idx = i % c^2 with the latitude index as the outer loop, both indices from 1.
__global__ void sm_places(int64_t total, int64_t c, const int64_t *region_ids, const double *geo, int64_t min_place_id,
                          double n_categories, int64_t min_category_id, uint64_t cat_skey, int64_t *out_ids, double *out_lat,
                          double *out_lon, int64_t *out_region, int64_t *out_category)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t cc = c * c, r = i / cc, idx = i % cc;
    const int64_t lat_idx = idx / c + 1, lon_idx = idx % c + 1;
    const double *g = geo + 4 * r;
    const int64_t region = region_ids[r];
    out_ids[i] = min_place_id + region * cc + idx;
    out_lat[i] = g[0] + g[1] * (double)lat_idx;
    out_lon[i] = g[2] + g[3] * (double)lon_idx;
    out_region[i] = region;
    const double f = u01_of(row_key(cat_skey, (uint64_t)i), 0ull);
    out_category[i] = min_category_id + (int64_t)(f * n_categories);
}

// ---- place names --------------------------------------------------------------------------------------------------

__constant__ uint64_t kSmPow10[20] = {1ull,
                                      10ull,
                                      100ull,
                                      1000ull,
                                      10000ull,
                                      100000ull,
                                      1000000ull,
                                      10000000ull,
                                      100000000ull,
                                      1000000000ull,
                                      10000000000ull,
                                      100000000000ull,
                                      1000000000000ull,
                                      10000000000000ull,
                                      100000000000000ull,
                                      1000000000000000ull,
                                      10000000000000000ull,
                                      100000000000000000ull,
                                      1000000000000000000ull,
                                      10000000000000000000ull};

__device__ __forceinline__ int decimal_digits(uint64_t v)
{
    int d = 1;
    while (d < 20 && v >= kSmPow10[d]) ++d;
    return d;
}

// units of "<category>-<id>" per place; a negative id or a category outside the table: no units, smallest row in *bad
__global__ void sm_name_lengths(int64_t n, const int64_t *place_ids, const int64_t *category_ids, int64_t min_category_id,
                                int64_t n_categories, const int64_t *cat_offsets, int64_t *lengths,
                                unsigned long long *bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t id = place_ids[i], cat = category_ids[i] - min_category_id;
    if (id < 0 || cat < 0 || cat >= n_categories) {
        lengths[i] = 0;
        atomicMin(bad, (unsigned long long)i);
        return;
    }
    lengths[i] = cat_offsets[cat + 1] - cat_offsets[cat] + 1 + decimal_digits((uint64_t)id);
}

// one unit per thread; offsets[j] = first unit of name j (strictly ascending: a name has at least two units)
__global__ void sm_name_fill(int64_t units, int64_t n, const int64_t *offsets, const int64_t *place_ids, const int64_t *category_ids,
                             int64_t min_category_id, const int64_t *cat_offsets, const uint16_t *cat_units, uint16_t *out_units)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= units) return;
    const int64_t j = lower_bound<int64_t>(offsets, 0, n, u + 1) - 1;
    const int64_t pos = u - offsets[j];
    const int64_t cat = category_ids[j] - min_category_id;
    const int64_t cat_len = cat_offsets[cat + 1] - cat_offsets[cat];
    uint16_t unit;
    if (pos < cat_len) {
        unit = cat_units[cat_offsets[cat] + pos];
    } else if (pos == cat_len) {
        unit = (uint16_t)'-';
    } else {
        const uint64_t id = (uint64_t)place_ids[j];
        const int q = (int)(pos - cat_len - 1);  // digit number, from the most significant
        unit = (uint16_t)('0' + (id / kSmPow10[decimal_digits(id) - 1 - q]) % 10ull);
    }
    out_units[u] = unit;
}

__global__ void sm_set_i64(int64_t *p, int64_t v) { *p = v; }

}  // namespace

extern "C" int32_t locrec_sample_persons(int32_t n_regions, const int64_t *region_ids, int64_t person_count,
                                         int64_t min_person_id, int32_t mem, int64_t *out_ids, int64_t *out_home_region_ids,
                                         int64_t *out_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!out_count) return fail(LOCREC_E_INVALID_ARG, "out_count is required");
    *out_count = 0;
    Regions R;
    LOCREC_TRY(check_regions(n_regions, region_ids, R));
    if (person_count < 0) return fail(LOCREC_E_INVALID_ARG, "negative person count");
    const int64_t ppr = person_count / n_regions;  // the remainder is dropped (LocationVisitsSampleGenerator.scala:19)
    const int64_t total = ppr * n_regions;
    if (total == 0) return LOCREC_OK;
    const __int128 last = (__int128)min_person_id + ((__int128)R.sorted_ids.back() + 1) * ppr - 1;
    if (!fits_i64(last) || !fits_i64((__int128)min_person_id + (__int128)R.sorted_ids.front() * ppr))
        return fail(LOCREC_E_INVALID_ARG, "the person ids leave the int64 range");
    if (!out_ids || !out_home_region_ids) return fail(LOCREC_E_INVALID_ARG, "null output array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    DevBuf<int64_t> regs;
    Out<int64_t> oid, ohome;
    LOCREC_TRY(regs.upload(region_ids, (size_t)n_regions, s));
    LOCREC_TRY(oid.bind(out_ids, total, mem));
    LOCREC_TRY(ohome.bind(out_home_region_ids, total, mem));
    LOCREC_LAUNCH(sm_persons, grid_for(total), dim3(256), 0, s, total, ppr, regs.p, min_person_id, oid.p, ohome.p);
    LOCREC_TRY(oid.deliver(total, s));
    LOCREC_TRY(ohome.deliver(total, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    *out_count = total;
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_sample_location_visits(int64_t n_persons, const int64_t *person_ids, const int64_t *home_region_ids,
                                                 int64_t person_index_base, int32_t n_regions, const int64_t *region_ids,
                                                 const double *region_boxes, int64_t from_timestamp_ms, int64_t interval_hours,
                                                 int64_t max_visits_per_person, uint64_t seed, int32_t shared_factor,
                                                 int32_t mem, int64_t *out_person_ids, int64_t *out_region_ids,
                                                 double *out_latitudes, double *out_longitudes, int64_t *out_timestamps,
                                                 int32_t *out_year_months, int64_t *inout_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!inout_count) return fail(LOCREC_E_INVALID_ARG, "inout_count is required");
    const int64_t cap = *inout_count;
    *inout_count = 0;
    g_sample_stats = SampleStats();
    if (cap < 0) return fail(LOCREC_E_INVALID_ARG, "negative capacity");
    if (n_persons < 0) return fail(LOCREC_E_INVALID_ARG, "negative person count");
    if (person_index_base < 0 || person_index_base > std::numeric_limits<int64_t>::max() - n_persons)
        return fail(LOCREC_E_INVALID_ARG, "person_index_base + n_persons must stay inside [0, 2^63)");
    Regions R;
    LOCREC_TRY(check_regions(n_regions, region_ids, R));
    LOCREC_TRY(check_boxes(n_regions, region_boxes));
    if (shared_factor != 0 && shared_factor != 1) return fail(LOCREC_E_INVALID_ARG, "shared_factor must be 0 or 1");
    if (max_visits_per_person < 1 || max_visits_per_person > std::numeric_limits<int32_t>::max())
        return fail(LOCREC_E_INVALID_ARG, "max_visits_per_person %lld out of range [1, 2^31)", (long long)max_visits_per_person);
    if (interval_hours < 0 || interval_hours > kSmMaxAbsMs / kSmMsPerHour || from_timestamp_ms < -kSmMaxAbsMs ||
        from_timestamp_ms > kSmMaxAbsMs - interval_hours * kSmMsPerHour)
        return fail(LOCREC_E_INVALID_ARG, "the interval [from_timestamp_ms, + interval_hours] must lie within 100,000,000 days of 1970");
    if (n_persons == 0) return LOCREC_OK;
    if (!person_ids || !home_region_ids) return fail(LOCREC_E_INVALID_ARG, "null array");
    if (cap > 0 && (!out_person_ids || !out_region_ids || !out_latitudes || !out_longitudes || !out_timestamps || !out_year_months))
        return fail(LOCREC_E_INVALID_ARG, "null output array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Temp tmp;
    PhaseClock clock;
    clock.s = s;
    In<int64_t> pid, home;
    LOCREC_TRY(pid.bind(person_ids, n_persons, mem, s));
    LOCREC_TRY(home.bind(home_region_ids, n_persons, mem, s));
    std::vector<double> sorted_boxes((size_t)n_regions * 4);
    for (int32_t i = 0; i < n_regions; ++i)
        std::copy(region_boxes + 4 * (size_t)R.order[(size_t)i], region_boxes + 4 * (size_t)R.order[(size_t)i] + 4,
                  sorted_boxes.begin() + 4 * (size_t)i);
    DevBuf<int64_t> regs;
    DevBuf<double> boxes;
    DevBuf<unsigned long long> counts, offsets, bad;
    DevBuf<uint64_t> keys;
    DevBuf<int32_t> rank;
    LOCREC_TRY(regs.upload(R.sorted_ids, s));
    LOCREC_TRY(boxes.upload(sorted_boxes, s));
    LOCREC_TRY(counts.alloc((size_t)n_persons));
    LOCREC_TRY(offsets.alloc((size_t)n_persons));
    LOCREC_TRY(keys.alloc((size_t)n_persons));
    LOCREC_TRY(rank.alloc((size_t)n_persons));
    LOCREC_TRY(bad.alloc(1));
    LOCREC_HIP_TRY(hipMemsetAsync(bad.p, 0xFF, sizeof(unsigned long long), s));

    LOCREC_TRY(clock.mark(0));
    LOCREC_LAUNCH(sm_visit_counts, grid_for(n_persons), dim3(256), 0, s, n_persons, home.p, person_index_base, regs.p,
                  n_regions, stream_key(seed, kSmStreamVisitCount), stream_key(seed, kSmStreamVisit),
                  (double)max_visits_per_person, counts.p, keys.p, rank.p, bad.p);
    LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, counts.p, offsets.p, (size_t)n_persons, s));
    unsigned long long last_off = 0, last_cnt = 0, bad_row = 0;
    LOCREC_HIP_TRY(hipMemcpyAsync(&last_off, offsets.p + (n_persons - 1), 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&last_cnt, counts.p + (n_persons - 1), 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&bad_row, bad.p, 8, hipMemcpyDeviceToHost, s));
    LOCREC_TRY(clock.mark(-1));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    if (bad_row != ~0ull) {  // regions.find(_.id == regionId).get of a missing region (LocationVisitsSampleGenerator.scala:33-36)
        int64_t region = 0;
        LOCREC_HIP_TRY(hipMemcpy(&region, home.p + bad_row, sizeof region, hipMemcpyDeviceToHost));
        return fail(LOCREC_E_INVALID_ARG, "person row %llu: home region %lld is not one of the regions", bad_row, (long long)region);
    }
    const int64_t total = (int64_t)(last_off + last_cnt);
    *inout_count = total;
    const int64_t rows = std::min(total, cap);
    if (rows > 0) {
        Out<int64_t> op, org, ots;
        Out<double> olat, olon;
        Out<int32_t> oym;
        LOCREC_TRY(op.bind(out_person_ids, rows, mem));
        LOCREC_TRY(org.bind(out_region_ids, rows, mem));
        LOCREC_TRY(olat.bind(out_latitudes, rows, mem));
        LOCREC_TRY(olon.bind(out_longitudes, rows, mem));
        LOCREC_TRY(ots.bind(out_timestamps, rows, mem));
        LOCREC_TRY(oym.bind(out_year_months, rows, mem));
        LOCREC_TRY(clock.mark(1));
        LOCREC_LAUNCH(sm_visit_fill, grid_for(rows), dim3(256), 0, s, rows, n_persons, offsets.p, keys.p, rank.p, pid.p, home.p,
                      boxes.p, from_timestamp_ms, (double)interval_hours, shared_factor, op.p, org.p, olat.p, olon.p, ots.p,
                      oym.p);
        LOCREC_TRY(clock.mark(-1));
        LOCREC_TRY(op.deliver(rows, s));
        LOCREC_TRY(org.deliver(rows, s));
        LOCREC_TRY(olat.deliver(rows, s));
        LOCREC_TRY(olon.deliver(rows, s));
        LOCREC_TRY(ots.deliver(rows, s));
        LOCREC_TRY(oym.deliver(rows, s));
    }
    LOCREC_TRY(clock.read(g_sample_stats.ms));
    g_sample_stats.rows = rows;
    g_sample_stats.bytes = rows * kSmVisitRowBytes;
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_sample_location_visits_stats(int64_t *out_rows, int64_t *out_bytes, double *out_count_ms,
                                                       double *out_fill_ms)
{
    const SampleStats &st = g_sample_stats;
    if (out_rows) *out_rows = st.rows;
    if (out_bytes) *out_bytes = st.bytes;
    if (out_count_ms) *out_count_ms = st.ms[0];
    if (out_fill_ms) *out_fill_ms = st.ms[1];
    return LOCREC_OK;
}

extern "C" int32_t locrec_sample_places(int32_t n_regions, const int64_t *region_ids, const double *region_boxes,
                                        int64_t place_count, int64_t min_place_id, int64_t n_categories,
                                        int64_t min_category_id, uint64_t seed, int32_t mem, int64_t *out_ids,
                                        double *out_latitudes, double *out_longitudes, int64_t *out_region_ids,
                                        int64_t *out_category_ids, int64_t *out_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!out_count) return fail(LOCREC_E_INVALID_ARG, "out_count is required");
    *out_count = 0;
    Regions R;
    LOCREC_TRY(check_regions(n_regions, region_ids, R));
    LOCREC_TRY(check_boxes(n_regions, region_boxes));
    if (place_count < 0 || place_count > ((int64_t)1 << 52))  // (the conversion to double and its square root stay exact)
        return fail(LOCREC_E_INVALID_ARG, "place_count %lld out of range [0, 2^52]", (long long)place_count);
    if (n_categories < 1 || n_categories > std::numeric_limits<int32_t>::max())
        return fail(LOCREC_E_INVALID_ARG, "n_categories %lld out of range [1, 2^31)", (long long)n_categories);
    if (min_category_id < 0 || min_category_id > std::numeric_limits<int64_t>::max() - n_categories)
        return fail(LOCREC_E_INVALID_ARG, "the category ids leave the non-negative int64 range");
    const int64_t ppr = place_count / n_regions;  // PlacesSampleGenerator.scala:14
    if (ppr == 0) return LOCREC_OK;
    const int64_t c = (int64_t)std::floor(std::sqrt((double)ppr));  // latCount = lonCount (:51)
    const int64_t cc = c * c, total = cc * n_regions;
    if (!fits_i64((__int128)min_place_id + ((__int128)R.sorted_ids.back() + 1) * cc - 1) ||
        !fits_i64((__int128)min_place_id + (__int128)R.sorted_ids.front() * cc))
        return fail(LOCREC_E_INVALID_ARG, "the place ids leave the int64 range");
    if (!out_ids || !out_latitudes || !out_longitudes || !out_region_ids || !out_category_ids)
        return fail(LOCREC_E_INVALID_ARG, "null output array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    std::vector<double> geo((size_t)n_regions * 4);
    for (int32_t r = 0; r < n_regions; ++r) {
        const double *b = region_boxes + 4 * (size_t)r;
        geo[4 * (size_t)r + 0] = b[0];
        geo[4 * (size_t)r + 1] = (b[1] - b[0]) / (double)c;  // latStep (:52)
        geo[4 * (size_t)r + 2] = b[2];
        geo[4 * (size_t)r + 3] = (b[3] - b[2]) / (double)c;  // lonStep (:53)
    }
    DevBuf<int64_t> regs;
    DevBuf<double> geo_dev;
    LOCREC_TRY(regs.upload(region_ids, (size_t)n_regions, s));
    LOCREC_TRY(geo_dev.upload(geo, s));
    Out<int64_t> oid, org, oca;
    Out<double> olat, olon;
    LOCREC_TRY(oid.bind(out_ids, total, mem));
    LOCREC_TRY(olat.bind(out_latitudes, total, mem));
    LOCREC_TRY(olon.bind(out_longitudes, total, mem));
    LOCREC_TRY(org.bind(out_region_ids, total, mem));
    LOCREC_TRY(oca.bind(out_category_ids, total, mem));
    LOCREC_LAUNCH(sm_places, grid_for(total), dim3(256), 0, s, total, c, regs.p, geo_dev.p, min_place_id, (double)n_categories,
                  min_category_id, stream_key(seed, kSmStreamCategory), oid.p, olat.p, olon.p, org.p, oca.p);
    LOCREC_TRY(oid.deliver(total, s));
    LOCREC_TRY(olat.deliver(total, s));
    LOCREC_TRY(olon.deliver(total, s));
    LOCREC_TRY(org.deliver(total, s));
    LOCREC_TRY(oca.deliver(total, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    *out_count = total;
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_sample_place_names(int64_t n, const int64_t *place_ids, const int64_t *category_ids,
                                             int64_t min_category_id, int64_t n_categories,
                                             const int64_t *category_name_offsets, const uint16_t *category_name_units,
                                             int32_t mem, int64_t *out_offsets, uint16_t *out_units, int64_t *inout_units)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!inout_units) return fail(LOCREC_E_INVALID_ARG, "inout_units is required");
    const int64_t cap = *inout_units;
    *inout_units = 0;
    if (cap < 0) return fail(LOCREC_E_INVALID_ARG, "negative capacity");
    if (n < 0) return fail(LOCREC_E_INVALID_ARG, "negative place count");
    if (n_categories < 1 || n_categories > std::numeric_limits<int32_t>::max())
        return fail(LOCREC_E_INVALID_ARG, "n_categories %lld out of range [1, 2^31)", (long long)n_categories);
    if (!category_name_offsets) return fail(LOCREC_E_INVALID_ARG, "category_name_offsets is required");
    if (category_name_offsets[0] < 0) return fail(LOCREC_E_INVALID_ARG, "category_name_offsets must begin at or above 0");
    for (int64_t c = 0; c < n_categories; ++c)
        if (category_name_offsets[c + 1] < category_name_offsets[c])
            return fail(LOCREC_E_INVALID_ARG, "category_name_offsets must never decrease (category %lld)", (long long)c);
    const int64_t cat_units = category_name_offsets[n_categories];
    if (cat_units > 0 && !category_name_units) return fail(LOCREC_E_INVALID_ARG, "category_name_units is required");
    if (n > 0 && (!place_ids || !category_ids)) return fail(LOCREC_E_INVALID_ARG, "null array");
    if (cap > 0 && (!out_offsets || !out_units)) return fail(LOCREC_E_INVALID_ARG, "null output array");
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Temp tmp;
    Out<int64_t> ooff;
    if (out_offsets) LOCREC_TRY(ooff.bind(out_offsets, n + 1, mem));
    if (n == 0) {
        if (out_offsets) {
            LOCREC_LAUNCH(sm_set_i64, dim3(1), dim3(1), 0, s, ooff.p, (int64_t)0);
            LOCREC_TRY(ooff.deliver(1, s));
            LOCREC_HIP_TRY(hipStreamSynchronize(s));
        }
        return LOCREC_OK;
    }
    In<int64_t> pid, cid;
    LOCREC_TRY(pid.bind(place_ids, n, mem, s));
    LOCREC_TRY(cid.bind(category_ids, n, mem, s));
    DevBuf<int64_t> coff, offsets_own, lengths;
    DevBuf<uint16_t> cunits;
    DevBuf<unsigned long long> bad;
    LOCREC_TRY(coff.upload(category_name_offsets, (size_t)n_categories + 1, s));
    LOCREC_TRY(cunits.upload(category_name_units, (size_t)cat_units, s));
    LOCREC_TRY(lengths.alloc((size_t)n));
    LOCREC_TRY(bad.alloc(1));
    LOCREC_HIP_TRY(hipMemsetAsync(bad.p, 0xFF, sizeof(unsigned long long), s));
    int64_t *offsets = ooff.p;
    if (!offsets) {
        LOCREC_TRY(offsets_own.alloc((size_t)n + 1));
        offsets = offsets_own.p;
    }
    LOCREC_LAUNCH(sm_name_lengths, grid_for(n), dim3(256), 0, s, n, pid.p, cid.p, min_category_id, n_categories, coff.p,
                  lengths.p, bad.p);
    LOCREC_PRIM(tmp, prim::exclusive_sum(p_, bytes_, lengths.p, offsets, (size_t)n, s));
    unsigned long long bad_row = 0;
    int64_t last_off = 0, last_len = 0;
    LOCREC_HIP_TRY(hipMemcpyAsync(&last_off, offsets + (n - 1), 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&last_len, lengths.p + (n - 1), 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipMemcpyAsync(&bad_row, bad.p, 8, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    if (bad_row != ~0ull)
        return fail(LOCREC_E_INVALID_ARG, "place row %llu: the id is negative or the category is outside the %lld categories from %lld",
                    bad_row, (long long)n_categories, (long long)min_category_id);
    const int64_t total = last_off + last_len;
    *inout_units = total;
    LOCREC_LAUNCH(sm_set_i64, dim3(1), dim3(1), 0, s, offsets + n, total);
    const int64_t units = std::min(total, cap);
    Out<uint16_t> ounits;
    if (units > 0) {
        LOCREC_TRY(ounits.bind(out_units, units, mem));
        LOCREC_LAUNCH(sm_name_fill, grid_for(units), dim3(256), 0, s, units, n, offsets, pid.p, cid.p, min_category_id, coff.p,
                      cunits.p, ounits.p);
        LOCREC_TRY(ounits.deliver(units, s));
    }
    if (out_offsets) LOCREC_TRY(ooff.deliver(n + 1, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL
