// eval.hip -- offline evaluation on the device: the two ends of the hold-out protocol around the existing builds and
// ranked batches (include/locrec.h, "Offline evaluation").
//
//   locrec_eval_ranked_batch   ranked rows (what every *_ranked_batch call returns) against one list of relevant ids per
//                              segment: hits, precision, recall, reciprocal rank, average precision and NDCG at up to
//                              LOCREC_EVAL_MAX_CUTOFFS cutoffs, their means, the hit rate and the catalogue coverage.
//   locrec_holdout_split       a visit table cut at a time: the train rows, and the distinct (person, region, place)
//                              triples behind the cut of persons that have a train row.
//
// The evaluator, one path for every shape:
//   ev_check      rel_offsets and rec_counts, on the device, before anything reads through them (the call's first wait).
//   pair table    the relevant lists as (segment, id key) pairs: ev_expand, then two stable radix passes (id, segment) -
//                 the exclusion table of rank_batch.hip in shape.  Here the segments' ranges ARE the offsets (minus
//                 offsets[0]), so no scan of lengths is needed, and the duplicates stay in the table: the first pair of
//                 a run of equal (segment, id) is the entry, a lower bound always lands on it, and R is the number of
//                 run heads in a segment's range.  Global memory: a list has no length limit.
//   ev_match      one thread per (segment, position below min(count, largest cutoff)): a binary search in the segment's
//                 range, and atomicMin(first position, position) on the entry it finds - an integer minimum, so a row
//                 that repeats an id gets its hit at the first of them whatever the order of arrival.  The same thread
//                 writes the (id key, position) pair of the coverage sort.
//   ev_walk       one wave64 per segment, 64 positions a step: a position is a hit iff its entry's first position is
//                 itself; ballot, prefix pop-count for h(r), one fixed-shape inclusive wave scan each for the AP and the
//                 DCG terms, and every cutoff reads the scan at its own last position - all cutoffs in one pass, a
//                 cutoff's value independent of the others.  d[r] and the ideal DCG's prefix sums come from tables the
//                 host computes in fp64.  No LDS, so no width limit.
//   ev_means      one block per cutoff: every thread sums its segments (s = t, t + 256, ...) in order, then a fixed LDS
//                 tree - the same bits for the same input, no floating-point atomics anywhere.
//   coverage      one stable radix sort of the (id key, position) pairs, the smallest position of every run
//                 (prim::min_by_key), and per cutoff the runs whose smallest position is below it (integer atomics).
// The call waits for the stream twice whatever the number of segments: after ev_check and for the results.
//
// The split: a stable select of the rows before the cut; the train rows' (person, place) pairs sorted by two radix
// passes; hs_held_flags keeps a row at or behind the cut whose person the table holds (and, for new places only, whose
// (person, place) it does not); the kept rows are sorted by three stable passes (place, region, person), the run heads
// selected and the three columns gathered.  Four waits at the most (train rows, kept rows, distinct triples, results).
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (VGPRs / LDS bytes / scratch / waves per SIMD):
//   ev_check  10 / 0 / 0 / 8    ev_expand  14 / 0 / 0 / 8      ev_match     20 / 0 / 0 / 8
//   ev_walk   98 / 0 / 0 / 4    ev_means   44 / 16384 / 0 / 8  ev_coverage  6 / 0 / 0 / 8
//   hs_train_flags 4 / 0 / 0 / 8   hs_held_flags 16 / 0 / 0 / 8   hs_head_flags 14 / 0 / 0 / 8   hs_gather 10 / 0 / 0 / 8
// ev_walk keeps the running sums of all eight cutoffs in registers (8 x (hits, AP, DCG) = 40 VGPRs, the two scans and
// the search on top): 4 waves a SIMD, no scratch.  It is bound by the latency of its binary searches, one per position,
// and a wave holds one segment - sixteen segments a CU in flight at that occupancy; halving the registers (cutoffs in
// two passes) would double the searches instead.

#include "dev_prims.h"

#include <algorithm>
#include <cmath>

#include "common.h"
#include "prep_cols.h"

namespace {

using namespace locrec;

constexpr int kEvThreads = 256;
constexpr int kEvWaves = kEvThreads / 64;  // segments per block of ev_walk
constexpr int kEvMaxCut = LOCREC_EVAL_MAX_CUTOFFS;
constexpr uint32_t kEvNoPos = 0xFFFFFFFFu;  // no position (positions are below 2^31)
// the result words of one call: [0, 48) the means as doubles (cutoff-major, 6 each), [48, 56) the coverage, [56]
// segments evaluated, [57] table entries
constexpr int kEvResMeans = 0, kEvResCoverage = 6 * kEvMaxCut, kEvResEvaluated = kEvResCoverage + kEvMaxCut,
              kEvResEntries = kEvResEvaluated + 1, kEvResWords = kEvResEntries + 1;

struct EvalStats {
    int64_t table_entries = 0;  // (segment, id) pairs after de-duplication
    int64_t evaluated = 0;      // segments with R > 0
    int64_t host_syncs = 0;     // explicit stream synchronisations of the call
    int64_t path = 0;           // 1: the wave-per-segment walk (the only path); 0: no device work (no segments, or refused)
};

EvalStats &eval_stats()
{
    thread_local EvalStats st;
    return st;
}

struct EvCuts {
    int64_t k[kEvMaxCut];
    int32_t n;
};

// hdr[0]: bit 0 - rel_offsets negative, decreasing or beyond n_rel; bit 1 - a rec_counts entry outside [0, width].
// hdr[1] = rel_offsets[0], hdr[2] = rel_offsets[n_seg].  Reads the offsets and counts only, never through them.
__global__ void ev_check(int64_t n_seg, int64_t width, const int64_t *counts, const int64_t *off, int64_t n_rel,
                         unsigned long long *hdr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_seg) return;
    const int64_t b = off[i], e = off[i + 1], c = counts[i];
    unsigned long long bad = 0;
    if (!(b >= 0 && e >= b && e <= n_rel)) bad |= 1ull;
    if (c < 0 || c > width) bad |= 2ull;
    if (bad) atomicOr(&hdr[0], bad);
    if (i == 0) hdr[1] = (unsigned long long)b;
    if (i == n_seg - 1) hdr[2] = (unsigned long long)e;
}

// pair q of the unsorted table is entry off0 + q of rel_ids: its id key and its segment - the last s with off[s] <= p
// (off0 <= p < off[n_seg], so there is one, and an empty list holds none)
__global__ void ev_expand(int64_t n_seg, int64_t total, const int64_t *off, int64_t off0, const int64_t *rel_ids, uint64_t *keys,
                          uint32_t *segs)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const int64_t p = off0 + q;
    int64_t a = 0, b = n_seg;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (off[mid] <= p) a = mid + 1; else b = mid;
    }
    keys[q] = ordered_key(rel_ids[p]);
    segs[q] = (uint32_t)(a - 1);
}

// Position r = i % weff of segment i / weff, weff = min(width, largest cutoff).  Below the segment's count: the entry
// of its id in the segment's range gets min(first position, r), and the coverage pair is (id key, r).  At or beyond
// the count nothing of the row is read; the pair is (0, no position), which no cutoff counts.
__global__ void ev_match(int64_t n_entries, int64_t width, int64_t weff, const int64_t *rec_ids, const int64_t *counts,
                         const int64_t *off, int64_t off0, const uint64_t *keys, uint32_t *first_pos, uint64_t *ckey,
                         uint32_t *cpos)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries) return;
    const int64_t s = i / weff, r = i - s * weff;
    uint64_t key = 0;
    uint32_t pos = kEvNoPos;
    if (r < counts[s]) {
        key = ordered_key(rec_ids[s * width + r]);
        pos = (uint32_t)r;
        const int64_t tb = off[s] - off0, te = off[s + 1] - off0;
        if (te > tb) {
            const int64_t a = lower_bound<uint64_t>(keys, tb, te, key);
            if (a < te && keys[a] == key) atomicMin(&first_pos[a], pos);
        }
    }
    ckey[i] = key;
    cpos[i] = pos;
}

// inclusive sum over the 64 lanes of a wave, lane order, in the fixed shape of the doubling scan
__device__ __forceinline__ double ev_wave_scan(double x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// One wave per segment.  dtab[r] = 1 / log2(r + 2) for r < weff; idcg[m] = sum of dtab over r < m for m <= min(largest
// cutoff, pairs in the table) - which bounds min(R, k).  hits / metrics are the call's own buffers when the caller wants
// none.
__global__ __launch_bounds__(kEvThreads) void ev_walk(int64_t n_seg, int64_t width, int64_t weff, const int64_t *rec_ids,
                                                      const int64_t *counts, const int64_t *off, int64_t off0,
                                                      const uint64_t *keys, const uint32_t *first_pos, EvCuts cuts,
                                                      const double *dtab, const double *idcg, int64_t *out_relevant,
                                                      int64_t *hits, double *metrics)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kEvWaves + (threadIdx.x >> 6);
    if (s >= n_seg) return;  // (the whole wave)
    const int64_t tb = off[s] - off0, te = off[s + 1] - off0;
    int64_t R = 0;
    for (int64_t p0 = tb; p0 < te; p0 += 64) {
        const int64_t p = p0 + lane;
        const bool head = p < te && (p == tb || keys[p] != keys[p - 1]);
        R += __popcll(__ballot(head));
    }
    const int64_t lmax = R > 0 ? min(counts[s], weff) : 0;
    int64_t hj[kEvMaxCut], before = 0, first = -1;
    double apj[kEvMaxCut], dcgj[kEvMaxCut];
#pragma unroll
    for (int j = 0; j < kEvMaxCut; ++j) {
        hj[j] = 0;
        apj[j] = 0.0;
        dcgj[j] = 0.0;
    }
    for (int64_t t0 = 0; t0 < lmax; t0 += 64) {
        const int64_t r = t0 + lane;
        bool hit = false;
        if (r < lmax) {
            const uint64_t key = ordered_key(rec_ids[s * width + r]);
            const int64_t a = lower_bound<uint64_t>(keys, tb, te, key);
            hit = a < te && keys[a] == key && first_pos[a] == (uint32_t)r;
        }
        const unsigned long long m = __ballot(hit);
        if (m == 0) continue;  // (uniform: a tile without a hit adds nothing)
        const int64_t h = before + __popcll(m & (~0ull >> (63 - lane)));  // hits at positions <= r
        const double ap_scan = ev_wave_scan(hit ? (double)h / (double)(r + 1) : 0.0, lane);
        const double dcg_scan = ev_wave_scan(hit ? dtab[r] : 0.0, lane);
#pragma unroll
        for (int j = 0; j < kEvMaxCut; ++j) {
            if (j < cuts.n) {
                const int64_t lim = min(min(cuts.k[j], lmax) - t0, (int64_t)64);  // positions of this tile below the cutoff
                const int src = lim > 0 ? (int)lim - 1 : 0;
                const double a = __shfl(ap_scan, src, 64), d = __shfl(dcg_scan, src, 64);
                if (lim > 0) {
                    apj[j] += a;
                    dcgj[j] += d;
                    hj[j] += __popcll(m & (~0ull >> (64 - lim)));
                }
            }
        }
        if (first < 0) first = t0 + (__ffsll((long long)m) - 1);
        before += __popcll(m);
    }
    if (lane != 0) return;
    out_relevant[s] = R;
#pragma unroll
    for (int j = 0; j < kEvMaxCut; ++j) {
        if (j < cuts.n) {
            const int64_t k = cuts.k[j], o = s * cuts.n + j;
            double *mt = metrics + o * 5;
            hits[o] = hj[j];
            if (R > 0) {
                const int64_t ideal = min(R, k);
                mt[0] = (double)hj[j] / (double)k;
                mt[1] = (double)hj[j] / (double)R;
                mt[2] = first >= 0 && first < k ? 1.0 / (double)(first + 1) : 0.0;
                mt[3] = apj[j] / (double)ideal;
                mt[4] = dcgj[j] / idcg[ideal];
            } else {
                mt[0] = mt[1] = mt[2] = mt[3] = mt[4] = 0.0;
            }
        }
    }
}

// Block j: the sums of cutoff j's five metrics and of "hits > 0" over the evaluated segments - per thread in segment
// order, then a fixed tree - divided by their number; block 0 also reports that number and the table's entries.
__global__ __launch_bounds__(kEvThreads) void ev_means(int64_t n_seg, int32_t nc, const int64_t *relevant, const int64_t *hits,
                                                       const double *metrics, unsigned long long *res)
{
    __shared__ double sum[6][kEvThreads];
    __shared__ long long cnt[2][kEvThreads];
    const int j = blockIdx.x, t = threadIdx.x;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    long long evaluated = 0, entries = 0;
    for (int64_t s = t; s < n_seg; s += kEvThreads) {
        const int64_t R = relevant[s];
        if (R <= 0) continue;
        ++evaluated;
        entries += R;
        const int64_t o = s * nc + j;
#pragma unroll
        for (int m = 0; m < 5; ++m) a[m] += metrics[o * 5 + m];
        a[5] += hits[o] > 0 ? 1.0 : 0.0;
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) sum[m][t] = a[m];
    cnt[0][t] = evaluated;
    cnt[1][t] = entries;
    __syncthreads();
    for (int stride = kEvThreads / 2; stride > 0; stride >>= 1) {
        if (t < stride) {
#pragma unroll
            for (int m = 0; m < 6; ++m) sum[m][t] += sum[m][t + stride];
            cnt[0][t] += cnt[0][t + stride];
            cnt[1][t] += cnt[1][t + stride];
        }
        __syncthreads();
    }
    if (t < 6) {
        const double v = cnt[0][0] > 0 ? sum[t][0] / (double)cnt[0][0] : 0.0;
        res[kEvResMeans + j * 6 + t] = (unsigned long long)__double_as_longlong(v);
    }
    if (j == 0 && t == 0) {
        res[kEvResEvaluated] = (unsigned long long)cnt[0][0];
        res[kEvResEntries] = (unsigned long long)cnt[1][0];
    }
}

// run u < *n_runs of the sorted coverage pairs: its smallest position is below which cutoffs?
__global__ void ev_coverage(int64_t n_entries, const uint32_t *n_runs, const uint32_t *run_min, EvCuts cuts, unsigned long long *res)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = u < n_entries && u < (int64_t)*n_runs && run_min[u] != kEvNoPos;
    const int64_t pos = live ? (int64_t)run_min[u] : 0;
    for (int j = 0; j < cuts.n; ++j) {
        const unsigned long long m = __ballot(live && pos < cuts.k[j]);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&res[kEvResCoverage + j], (unsigned long long)__popcll(m));
    }
}

bool ev_host_offsets_ok(const int64_t *off, int64_t n_seg, int64_t n)
{
    bool ok = off[0] >= 0 && off[n_seg] <= n;
    for (int64_t i = 0; ok && i < n_seg; ++i) ok = off[i] <= off[i + 1];
    return ok;
}

const char *const kEvBadOffsets = "rel_offsets must be non-decreasing offsets inside [0, n_rel]";
const char *const kEvBadCounts = "every rec_counts entry must be within [0, width]";

// ---- the hold-out split -----------------------------------------------------------------------------------------------

__global__ void hs_train_flags(int64_t n, const int64_t *ts, int64_t cut, unsigned char *flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = ts[i] < cut ? 1 : 0;
}

// first position of the train table (person keys tp, place keys tq, sorted by person and then place) that is not below
// (p, q); nt if there is none
__device__ __forceinline__ int64_t hs_lower_bound(const uint64_t *tp, const uint64_t *tq, int64_t nt, uint64_t p, uint64_t q)
{
    int64_t lo = 0, hi = nt;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const uint64_t a = tp[mid];
        if (a < p || (a == p && tq[mid] < q)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a row at or behind the cut is kept iff its person has a train row - and, for new places only, no train row at its place
__global__ void hs_held_flags(int64_t n, const int64_t *person, const int64_t *ts, const int64_t *place, int64_t cut,
                              int32_t new_only, const uint64_t *tp, const uint64_t *tq, int64_t nt, unsigned char *flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool keep = false;
    if (ts[i] >= cut) {
        const uint64_t p = ordered_key(person[i]), q = ordered_key(place[i]);
        const int64_t a = hs_lower_bound(tp, tq, nt, p, 0);
        keep = a < nt && tp[a] == p;
        if (keep && new_only) {
            const int64_t b = hs_lower_bound(tp, tq, nt, p, q);
            keep = !(b < nt && tp[b] == p && tq[b] == q);
        }
    }
    flag[i] = keep ? 1 : 0;
}

// the first of every run of equal (person, region, place) among the sorted rows
__global__ void hs_head_flags(int64_t m, const uint32_t *rows, const int64_t *person, const int64_t *region, const int64_t *place,
                              unsigned char *flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    bool head = i == 0;
    if (!head) {
        const uint32_t a = rows[i], b = rows[i - 1];
        head = person[a] != person[b] || region[a] != region[b] || place[a] != place[b];
    }
    flag[i] = head ? 1 : 0;
}

__global__ void hs_gather(int64_t m, const uint32_t *rows, const int64_t *person, const int64_t *region, const int64_t *place,
                          int64_t *out_person, int64_t *out_region, int64_t *out_place)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t r = rows[i];
    out_person[i] = person[r];
    out_region[i] = region[r];
    out_place[i] = place[r];
}

}  // namespace

extern "C" int32_t locrec_eval_ranked_batch(int64_t n_segments, int64_t width, const int64_t *rec_ids, const int64_t *rec_counts,
                                            const int64_t *rel_offsets, int64_t n_rel, const int64_t *rel_ids, int32_t n_cutoffs,
                                            const int64_t *cutoffs, int32_t mem, int64_t *out_relevant, int64_t *out_hits,
                                            double *out_metrics, double *out_means, int64_t *out_coverage, int64_t *out_evaluated)
try {
    EvalStats &st = eval_stats();
    st = EvalStats();
    LOCREC_TRY(mem_ok(mem));
    if (!out_means) return fail(LOCREC_E_INVALID_ARG, "out_means is required");
    if (!out_coverage) return fail(LOCREC_E_INVALID_ARG, "out_coverage is required");
    if (!out_evaluated) return fail(LOCREC_E_INVALID_ARG, "out_evaluated is required");
    if (!out_relevant) return fail(LOCREC_E_INVALID_ARG, "out_relevant is required");
    if (n_cutoffs < 1 || n_cutoffs > kEvMaxCut) return fail(LOCREC_E_INVALID_ARG, "n_cutoffs %d outside 1..%d", n_cutoffs, kEvMaxCut);
    if (!cutoffs) return fail(LOCREC_E_INVALID_ARG, "cutoffs is NULL");
    EvCuts cuts = {};
    cuts.n = n_cutoffs;
    int64_t kmax = 0;
    for (int32_t j = 0; j < n_cutoffs; ++j) {
        if (cutoffs[j] <= 0) return fail(LOCREC_E_INVALID_ARG, "cutoffs[%d] = %lld: a cutoff must be > 0", j, (long long)cutoffs[j]);
        cuts.k[j] = cutoffs[j];
        kmax = std::max(kmax, cutoffs[j]);
    }
    if (width < 0) return fail(LOCREC_E_INVALID_ARG, "width %lld must be >= 0", (long long)width);
    if (n_segments < 0 || n_segments >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "n_segments out of range [0, 2^31)");
    if (n_rel < 0 || n_rel >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "n_rel out of range [0, 2^31)");
    if (n_segments > 0 && width > (kMaxRows - 1) / n_segments)
        return fail(LOCREC_E_INVALID_ARG, "n_segments x width must be below 2^31: split the batch");
    if (n_segments > 0 && !rec_counts) return fail(LOCREC_E_INVALID_ARG, "rec_counts is NULL");
    if (n_segments > 0 && !rel_offsets) return fail(LOCREC_E_INVALID_ARG, "rel_offsets is NULL");
    if (n_segments > 0 && width > 0 && !rec_ids) return fail(LOCREC_E_INVALID_ARG, "rec_ids is NULL");
    if (n_segments > 0 && n_rel > 0 && !rel_ids) return fail(LOCREC_E_INVALID_ARG, "rel_ids is NULL");
    if (mem == LOCREC_MEM_HOST && n_segments > 0) {
        if (!ev_host_offsets_ok(rel_offsets, n_segments, n_rel)) return fail(LOCREC_E_INVALID_ARG, kEvBadOffsets);
        for (int64_t i = 0; i < n_segments; ++i)
            if (rec_counts[i] < 0 || rec_counts[i] > width) return fail(LOCREC_E_INVALID_ARG, kEvBadCounts);
    }
    if (n_segments == 0) {
        std::fill(out_means, out_means + 6 * n_cutoffs, 0.0);
        std::fill(out_coverage, out_coverage + n_cutoffs, (int64_t)0);
        *out_evaluated = 0;
        return LOCREC_OK;
    }
    LOCREC_TRY(ensure_device());
    st.path = 1;
    hipStream_t s = nullptr;
    Temp tmp;
    In<int64_t> rid, rcnt, roff, rl;
    LOCREC_TRY(rid.bind(rec_ids, n_segments * width, mem, s));
    LOCREC_TRY(rcnt.bind(rec_counts, n_segments, mem, s));
    LOCREC_TRY(roff.bind(rel_offsets, n_segments + 1, mem, s));
    LOCREC_TRY(rl.bind(rel_ids, n_rel, mem, s));
    DevBuf<unsigned long long> hdr, res;
    LOCREC_TRY(hdr.alloc(3));
    LOCREC_HIP_TRY(hipMemsetAsync(hdr.p, 0, 3 * sizeof(unsigned long long), s));
    LOCREC_LAUNCH(ev_check, grid_for(n_segments), dim3(256), 0, s, n_segments, width, rcnt.p, roff.p, n_rel, hdr.p);
    unsigned long long h[3] = {0, 0, 0};
    LOCREC_HIP_TRY(hipMemcpyAsync(h, hdr.p, sizeof h, hipMemcpyDeviceToHost, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    ++st.host_syncs;
    if (h[0] & 1ull) return fail(LOCREC_E_INVALID_ARG, kEvBadOffsets);
    if (h[0] & 2ull) return fail(LOCREC_E_INVALID_ARG, kEvBadCounts);
    const int64_t off0 = (int64_t)h[1], total = (int64_t)h[2] - off0;  // 0 <= off0 <= off0 + total <= n_rel
    const int64_t weff = std::min(width, kmax), n_entries = n_segments * weff;

    // the pair table
    DevBuf<uint64_t> x0, x1;
    DevBuf<uint32_t> g0, g1, first_pos;
    if (total > 0) {
        LOCREC_TRY(alloc_each((size_t)total, x0, x1));
        LOCREC_TRY(alloc_each((size_t)total, g0, g1, first_pos));
        unsigned seg_bits = 1;
        while (seg_bits < 32 && ((int64_t)1 << seg_bits) < n_segments) ++seg_bits;
        LOCREC_LAUNCH(ev_expand, grid_for(total), dim3(256), 0, s, n_segments, total, roff.p, off0, rl.p, x0.p, g0.p);
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, x0.p, x1.p, g0.p, g1.p, (size_t)total, 0, 64, s));
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, g1.p, g0.p, x1.p, x0.p, (size_t)total, 0, seg_bits, s));
        LOCREC_HIP_TRY(hipMemsetAsync(first_pos.p, 0xFF, (size_t)total * sizeof(uint32_t), s));
    }
    const uint64_t *keys = total > 0 ? x0.p : nullptr;

    // d[r] and the ideal DCG's prefix sums, in fp64 on the host
    const int64_t n_ideal = std::min(kmax, total);
    std::vector<double> dtab((size_t)std::max<int64_t>(weff, 1)), idcg((size_t)n_ideal + 1);
    for (int64_t r = 0; r < weff; ++r) dtab[(size_t)r] = 1.0 / std::log2((double)(r + 2));
    idcg[0] = 0.0;
    for (int64_t r = 0; r < n_ideal; ++r)
        idcg[(size_t)r + 1] = idcg[(size_t)r] + (r < weff ? dtab[(size_t)r] : 1.0 / std::log2((double)(r + 2)));
    DevBuf<double> dtab_dev, idcg_dev;
    LOCREC_TRY(dtab_dev.upload(dtab, s));
    LOCREC_TRY(idcg_dev.upload(idcg, s));

    Out<int64_t> orel, ohit;
    Out<double> omet;
    DevBuf<int64_t> hit_own;
    DevBuf<double> met_own;
    const int64_t n_hits = n_segments * n_cutoffs;
    LOCREC_TRY(orel.bind(out_relevant, n_segments, mem));
    if (out_hits) LOCREC_TRY(ohit.bind(out_hits, n_hits, mem)); else LOCREC_TRY(hit_own.alloc((size_t)n_hits));
    if (out_metrics) LOCREC_TRY(omet.bind(out_metrics, n_hits * 5, mem)); else LOCREC_TRY(met_own.alloc((size_t)n_hits * 5));
    int64_t *hits = out_hits ? ohit.p : hit_own.p;
    double *metrics = out_metrics ? omet.p : met_own.p;

    DevBuf<uint64_t> c0, c1;
    DevBuf<uint32_t> q0, q1, n_runs;
    if (n_entries > 0) {
        LOCREC_TRY(alloc_each((size_t)n_entries, c0, c1));
        LOCREC_TRY(alloc_each((size_t)n_entries, q0, q1));
        LOCREC_TRY(n_runs.alloc(1));
        LOCREC_LAUNCH(ev_match, grid_for(n_entries), dim3(256), 0, s, n_entries, width, weff, rid.p, rcnt.p, roff.p, off0, keys,
                      first_pos.p, c0.p, q0.p);
    }
    LOCREC_LAUNCH(ev_walk, grid_for(n_segments, kEvWaves), dim3(kEvThreads), 0, s, n_segments, width, weff, rid.p, rcnt.p, roff.p,
                  off0, keys, first_pos.p, cuts, dtab_dev.p, idcg_dev.p, orel.p, hits, metrics);
    LOCREC_TRY(res.alloc(kEvResWords));
    LOCREC_HIP_TRY(hipMemsetAsync(res.p, 0, kEvResWords * sizeof(unsigned long long), s));
    LOCREC_LAUNCH(ev_means, dim3((unsigned)n_cutoffs), dim3(kEvThreads), 0, s, n_segments, n_cutoffs, orel.p, hits, metrics, res.p);
    if (n_entries > 0) {
        LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, c0.p, c1.p, q0.p, q1.p, (size_t)n_entries, 0, 64, s));
        LOCREC_PRIM(tmp, prim::min_by_key(p_, bytes_, c1.p, q1.p, (size_t)n_entries, c0.p, q0.p, n_runs.p, s));
        LOCREC_LAUNCH(ev_coverage, grid_for(n_entries), dim3(256), 0, s, n_entries, n_runs.p, q0.p, cuts, res.p);
    }
    unsigned long long r[kEvResWords];
    LOCREC_HIP_TRY(hipMemcpyAsync(r, res.p, sizeof r, hipMemcpyDeviceToHost, s));
    LOCREC_TRY(orel.deliver(n_segments, s));
    if (out_hits) LOCREC_TRY(ohit.deliver(n_hits, s));
    if (out_metrics) LOCREC_TRY(omet.deliver(n_hits * 5, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    ++st.host_syncs;
    for (int32_t j = 0; j < n_cutoffs; ++j) {
        for (int m = 0; m < 6; ++m) memcpy(&out_means[j * 6 + m], &r[kEvResMeans + j * 6 + m], sizeof(double));
        out_coverage[j] = (int64_t)r[kEvResCoverage + j];
    }
    *out_evaluated = (int64_t)r[kEvResEvaluated];
    st.evaluated = (int64_t)r[kEvResEvaluated];
    st.table_entries = (int64_t)r[kEvResEntries];
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_eval_ranked_batch_stats(int64_t *out_table_entries, int64_t *out_evaluated, int64_t *out_host_syncs,
                                                  int64_t *out_path)
try {
    const EvalStats &st = eval_stats();
    if (out_table_entries) *out_table_entries = st.table_entries;
    if (out_evaluated) *out_evaluated = st.evaluated;
    if (out_host_syncs) *out_host_syncs = st.host_syncs;
    if (out_path) *out_path = st.path;
    return LOCREC_OK;
}
LOCREC_CATCH_ALL

extern "C" int32_t locrec_holdout_split(int64_t n, const int64_t *person_ids, const int64_t *timestamps, const int64_t *place_ids,
                                        const int64_t *region_ids, int64_t cut_timestamp, int32_t new_places_only, int32_t mem,
                                        int32_t *out_train_rows, int64_t *out_train_count, int64_t *out_person_ids,
                                        int64_t *out_region_ids, int64_t *out_place_ids, int64_t *inout_held_count)
try {
    LOCREC_TRY(mem_ok(mem));
    if (!out_train_count) return fail(LOCREC_E_INVALID_ARG, "out_train_count is required");
    if (!inout_held_count) return fail(LOCREC_E_INVALID_ARG, "inout_held_count is required");
    const bool fill = out_person_ids && out_region_ids && out_place_ids;  // NULL outputs: count only
    const int64_t cap = fill ? *inout_held_count : 0;
    if (cap < 0) return fail(LOCREC_E_INVALID_ARG, "negative capacity");
    if (n < 0 || n >= kMaxRows) return fail(LOCREC_E_INVALID_ARG, "row count %lld out of range [0, 2^31)", (long long)n);
    if (n > 0 && (!person_ids || !timestamps || !place_ids || !region_ids)) return fail(LOCREC_E_INVALID_ARG, "null array");
    *out_train_count = 0;
    *inout_held_count = 0;
    if (n == 0) return LOCREC_OK;
    LOCREC_TRY(ensure_device());
    hipStream_t s = nullptr;
    Temp tmp;
    In<int64_t> pe, ts, pl, rg;
    LOCREC_TRY(pe.bind(person_ids, n, mem, s));
    LOCREC_TRY(ts.bind(timestamps, n, mem, s));
    LOCREC_TRY(pl.bind(place_ids, n, mem, s));
    LOCREC_TRY(rg.bind(region_ids, n, mem, s));

    // the train rows: a stable selection of the row numbers
    DevBuf<unsigned char> flag;
    DevBuf<uint32_t> r0, r1, cnt_dev;
    LOCREC_TRY(flag.alloc((size_t)n));
    LOCREC_TRY(alloc_each((size_t)n, r0, r1));
    LOCREC_TRY(cnt_dev.alloc(1));
    prim::counting_iterator<uint32_t> iota(0u);
    LOCREC_LAUNCH(hs_train_flags, grid_for(n), dim3(256), 0, s, n, ts.p, cut_timestamp, flag.p);
    LOCREC_PRIM(tmp, prim::select_flagged(p_, bytes_, iota, flag.p, r0.p, cnt_dev.p, (size_t)n, s));
    uint32_t c32 = 0;
    LOCREC_READ_BACK(c32, cnt_dev.p, s);
    const int64_t nt = c32;
    *out_train_count = nt;
    if (out_train_rows && nt > 0) {  // (row numbers are below 2^31: the same bits as int32)
        LOCREC_HIP_TRY(hipMemcpyAsync(out_train_rows, r0.p, (size_t)nt * sizeof(uint32_t),
                                      mem == LOCREC_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
    }
    if (nt == 0 || nt == n) return LOCREC_OK;  // nobody has a train row, or nothing lies behind the cut

    // the train rows' (person, place) pairs, sorted: two stable passes, by place and then by person
    DevBuf<uint64_t> k0, k1, tq;
    LOCREC_TRY(alloc_each((size_t)n, k0, k1));
    LOCREC_TRY(tq.alloc((size_t)nt));
    LOCREC_LAUNCH(gather_id_keys, grid_for(nt), dim3(256), 0, s, nt, pl.p, r0.p, k0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r0.p, r1.p, (size_t)nt, 0, 64, s));
    LOCREC_LAUNCH(gather_id_keys, grid_for(nt), dim3(256), 0, s, nt, pe.p, r1.p, k0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r1.p, r0.p, (size_t)nt, 0, 64, s));
    LOCREC_LAUNCH(gather_id_keys, grid_for(nt), dim3(256), 0, s, nt, pl.p, r0.p, tq.p);
    DevBuf<uint64_t> tp;  // (k1 is needed again below)
    LOCREC_TRY(tp.alloc((size_t)nt));
    LOCREC_HIP_TRY(hipMemcpyAsync(tp.p, k1.p, (size_t)nt * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));

    // the rows behind the cut that count
    LOCREC_LAUNCH(hs_held_flags, grid_for(n), dim3(256), 0, s, n, pe.p, ts.p, pl.p, cut_timestamp, new_places_only, tp.p, tq.p, nt,
                  flag.p);
    LOCREC_PRIM(tmp, prim::select_flagged(p_, bytes_, iota, flag.p, r0.p, cnt_dev.p, (size_t)n, s));
    LOCREC_READ_BACK(c32, cnt_dev.p, s);
    const int64_t m = c32;
    if (m == 0) return LOCREC_OK;

    // sorted by person, region, place: three stable passes, the last key first
    LOCREC_LAUNCH(gather_id_keys, grid_for(m), dim3(256), 0, s, m, pl.p, r0.p, k0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r0.p, r1.p, (size_t)m, 0, 64, s));
    LOCREC_LAUNCH(gather_id_keys, grid_for(m), dim3(256), 0, s, m, rg.p, r1.p, k0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r1.p, r0.p, (size_t)m, 0, 64, s));
    LOCREC_LAUNCH(gather_id_keys, grid_for(m), dim3(256), 0, s, m, pe.p, r0.p, k0.p);
    LOCREC_PRIM(tmp, prim::sort_pairs(p_, bytes_, k0.p, k1.p, r0.p, r1.p, (size_t)m, 0, 64, s));
    LOCREC_LAUNCH(hs_head_flags, grid_for(m), dim3(256), 0, s, m, r1.p, pe.p, rg.p, pl.p, flag.p);
    LOCREC_PRIM(tmp, prim::select_flagged(p_, bytes_, r1.p, flag.p, r0.p, cnt_dev.p, (size_t)m, s));
    LOCREC_READ_BACK(c32, cnt_dev.p, s);
    const int64_t held = c32;
    *inout_held_count = held;
    const int64_t rows = std::min(held, cap);
    if (rows == 0) return LOCREC_OK;
    Out<int64_t> op, org, opl;
    LOCREC_TRY(op.bind(out_person_ids, rows, mem));
    LOCREC_TRY(org.bind(out_region_ids, rows, mem));
    LOCREC_TRY(opl.bind(out_place_ids, rows, mem));
    LOCREC_LAUNCH(hs_gather, grid_for(rows), dim3(256), 0, s, rows, r0.p, pe.p, rg.p, pl.p, op.p, org.p, opl.p);
    LOCREC_TRY(op.deliver(rows, s));
    LOCREC_TRY(org.deliver(rows, s));
    LOCREC_TRY(opl.deliver(rows, s));
    LOCREC_HIP_TRY(hipStreamSynchronize(s));
    return LOCREC_OK;
}
LOCREC_CATCH_ALL
