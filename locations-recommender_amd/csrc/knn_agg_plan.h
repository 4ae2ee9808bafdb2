// knn_agg_plan.h -- the host arithmetic of the LDS aggregation (knn_aggregate.h: knn_aggregate_buckets, knn_aggregate): which
// form pass 1 takes, capacities, threads and LDS bytes of each launch, whether a redo launch follows; and the word / bit /
// slot arithmetic of the bucket form's presence bitmap, which the kernel shares.
// Plain C++ without a device call: tests/host/knn_agg_plan_check.cpp runs it stand-alone, under a host sanitizer too.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LOCREC_AGG_HD __host__ __device__
#else
#define LOCREC_AGG_HD
#endif

namespace locrec {

constexpr int kAggThreads = 1024;      // threads of a full-capacity block: one neighbour per thread (K <= 1024)
constexpr int kAggPass1Cap = 2048;     // rating rows a pass-1 block has room for
constexpr int kAggPer = 4;             // positions a thread of the bucket form keeps in registers
constexpr int kAggBucketMax = 128;     // rows of one place the bucket form orders itself (its cost is their square)
constexpr size_t kAggLdsMax = 160 * 1024;        // LDS of a CU
constexpr size_t kAggBucketLdsMax = 80 * 1024;   // the bucket form's share: two blocks per CU

// ---- presence bitmap over the compact place indices: bit p & 31 of word p >> 5 ----
LOCREC_AGG_HD inline int32_t knn_agg_words(int64_t nplaces) { return (int32_t)((nplaces + 31) >> 5); }
LOCREC_AGG_HD inline int32_t knn_agg_word_of(uint32_t p) { return (int32_t)(p >> 5); }
LOCREC_AGG_HD inline uint32_t knn_agg_bit_of(uint32_t p) { return 1u << (p & 31); }
// set bits of `word` below place p's: p's rank among the places of its word
LOCREC_AGG_HD inline int32_t knn_agg_rank_in_word(uint32_t word, uint32_t p)
{
    return __builtin_popcount(word & (knn_agg_bit_of(p) - 1u));
}
// slot of place p = its rank among all present places; prefix = the exclusive popcount prefix of p's word
LOCREC_AGG_HD inline int32_t knn_agg_slot(int32_t prefix, uint32_t word, uint32_t p) { return prefix + knn_agg_rank_in_word(word, p); }
// thread t of `threads` owns the consecutive words [t * per, min(words, (t + 1) * per))
LOCREC_AGG_HD inline int32_t knn_agg_words_per_thread(int32_t words, int32_t threads) { return (words + threads - 1) / threads; }

// ---- LDS images (knn_aggregate.h lays its arrays out in exactly this order) ----
LOCREC_AGG_HD inline size_t knn_agg_up8(size_t b) { return (b + 7) & ~(size_t)7; }
// [K] first rating row, [K] similarity, [K + 1] offsets of the neighbours: the tail of both forms' images
LOCREC_AGG_HD inline size_t knn_agg_lds_neighbours(int K) { return (size_t)K * 16 + (size_t)(K + 1) * 4; }
// sort form: [cap] keys of 4 or 8 bytes, [cap] products, [cap] neighbour numbers
LOCREC_AGG_HD inline size_t knn_agg_lds_sort(int cap, int K, bool key32)
{
    return (size_t)cap * (key32 ? 14 : 18) + 8 + knn_agg_lds_neighbours(K) + 16;
}
// bucket form: a region that holds the [words] bitmap and its [words] 16-bit popcount prefix until every row knows its
// slot (phases 2-5), and from then on the ordered rows' [cap] products and [cap] neighbour numbers (phases 6-7: a block
// barrier lies between the last read of the one and the first write of the other); behind it [cap + 1] bucket starts,
// [cap] slot places, [cap] bucket entries.  The smaller image is what lets three blocks share a CU at cfg2's 100 k places.
struct KnnAggBucketLds {
    size_t bitmap, prefix, prod, nb, start, place, entry, neighbours, total;
};
LOCREC_AGG_HD inline KnnAggBucketLds knn_agg_bucket_lds(int cap, int K, int64_t nplaces)
{
    const size_t words = (size_t)knn_agg_words(nplaces);
    KnnAggBucketLds l{};
    l.bitmap = 0;
    l.prefix = l.bitmap + knn_agg_up8(words * 4);
    const size_t ranked = l.prefix + knn_agg_up8(words * 2);
    l.prod = 0;
    l.nb = l.prod + (size_t)cap * 8;
    const size_t ordered = l.nb + knn_agg_up8((size_t)cap * 2);
    l.start = ranked > ordered ? ranked : ordered;
    l.place = l.start + knn_agg_up8((size_t)(cap + 1) * 4);
    l.entry = l.place + knn_agg_up8((size_t)cap * 4);
    l.neighbours = l.entry + knn_agg_up8((size_t)cap * 2);
    l.total = l.neighbours + knn_agg_up8(knn_agg_lds_neighbours(K));
    return l;
}

inline int knn_agg_pow2ceil(int64_t v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline int knn_agg_ceil_log2(int64_t v)
{
    int b = 0;
    while (((int64_t)1 << b) < v) ++b;
    return b;
}

enum KnnAggForm : int32_t { kAggNone = 0, kAggBuckets = 1, kAggSort = 2 };

struct KnnAggLaunch {
    int32_t form = kAggNone;
    int32_t cap = 0;      // rating rows of a block (a power of two)
    int32_t threads = 0;
    size_t lds = 0;       // dynamic LDS bytes
    bool key32 = false;   // sort form: 32-bit keys (compact place index and position fit them)
    int32_t fbits = 16;   // sort form: bits of the position inside a key
};

struct KnnAggPlan {
    int32_t M = 0;        // full capacity: the row stride of the result and the capacity of the redo launch
    KnnAggLaunch pass1, redo;
    bool redo_needed = false;
};

inline KnnAggLaunch knn_agg_sort_launch(int cap, int threads, int K, int64_t nplaces)
{
    KnnAggLaunch l;
    l.form = kAggSort;
    l.cap = cap;
    l.threads = threads;
    l.key32 = knn_agg_ceil_log2(nplaces + 2) + knn_agg_ceil_log2(cap) <= 32;
    l.fbits = l.key32 ? knn_agg_ceil_log2(cap) : 16;
    l.lds = knn_agg_lds_sort(cap, K, l.key32);
    return l;
}

// threads of a pass-1 block: half a full block where the capacity and the neighbour count allow it
inline int knn_agg_pass1_threads(int K, int cap1, int M) { return (cap1 < M && K <= 512) ? 512 : kAggThreads; }

// The plan of one aggregation: K neighbours (1 .. 1024) of at most max_r_nnz rating rows each, nplaces compact places.
// Pass 1 runs every query at min(M, kAggPass1Cap) rows: in the bucket form where its LDS lets two blocks share a CU (and the
// switch does not force the sort form), else in the sort form.  A redo launch (sort form, full capacity, flagged queries
// only) follows wherever pass 1 can flag a query: more rows than its capacity, or - bucket form - more than bucket_max
// rows of one place, which no query can have whose rows are bucket_max or fewer in all.
inline KnnAggPlan knn_agg_plan(int K, int64_t max_r_nnz, int64_t nplaces, int agg_cap, bool force_sort,
                               int bucket_max = kAggBucketMax)
{
    KnnAggPlan p;
    const int64_t rows_max = (int64_t)K * std::max<int64_t>(1, max_r_nnz);
    const int64_t tmax = std::min<int64_t>(rows_max, agg_cap);
    p.M = knn_agg_pow2ceil(std::max<int64_t>(2, tmax));
    const int cap1 = std::min(p.M, kAggPass1Cap);
    const int threads1 = knn_agg_pass1_threads(K, cap1, p.M);
    const size_t blds = knn_agg_bucket_lds(cap1, K, nplaces).total;
    const bool buckets = !force_sort && blds <= kAggBucketLdsMax && cap1 <= threads1 * kAggPer;
    if (buckets) {
        p.pass1.form = kAggBuckets;
        p.pass1.cap = cap1;
        p.pass1.threads = threads1;
        p.pass1.lds = blds;
    } else {
        p.pass1 = knn_agg_sort_launch(cap1, threads1, K, nplaces);
    }
    const bool rows_flag = rows_max > cap1 && cap1 < p.M;  // (at cap1 == M a flag is final: the host assembles the query)
    const bool bucket_flag = buckets && rows_max > bucket_max;
    p.redo_needed = rows_flag || bucket_flag;
    if (p.redo_needed) p.redo = knn_agg_sort_launch(p.M, kAggThreads, K, nplaces);
    return p;
}

// the largest place count at which knn_agg_plan still chooses the bucket form (0: never)
inline int64_t knn_agg_place_limit(int K, int64_t max_r_nnz, int agg_cap)
{
    int64_t lo = 0, hi = (int64_t)1 << 32;  // bucket form at lo (or lo == 0), not at hi
    if (knn_agg_plan(K, max_r_nnz, 1, agg_cap, false).pass1.form != kAggBuckets) return 0;
    lo = 1;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (knn_agg_plan(K, max_r_nnz, mid, agg_cap, false).pass1.form == kAggBuckets) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace locrec
