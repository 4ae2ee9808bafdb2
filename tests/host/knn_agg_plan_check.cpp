// knn_agg_plan_check.cpp -- the host arithmetic of the LDS aggregation (csrc/knn_agg_plan.h): the plan over a grid of
// neighbour counts, row counts and place counts against its rules re-stated here, and a scalar model of the bucket form's
// phases 4-7 (rank, bucket, order, sum), built on the word / bit / slot functions the kernel shares, against a brute-force
// "group by place, sum in position order".  Stand-alone, so that it also runs under a host sanitizer:
//   g++ -std=c++17 -fsanitize=address,undefined -I locations-recommender_amd/csrc tests/host/knn_agg_plan_check.cpp
// Prints the number of cases and returns 0, or the first failed check and 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "knn_agg_plan.h"

using namespace locrec;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "%s:%d: %s fails (case %ld)\n", __FILE__, __LINE__, #cond, cases); \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

static long cases = 0;
constexpr int kCap = 4096;  // kAggCap of csrc/knn.hip

static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

static void check_launch(const KnnAggLaunch &l, int K, int64_t nplaces)
{
    CHECK(l.form == kAggBuckets || l.form == kAggSort);
    CHECK(l.lds <= kAggLdsMax);
    CHECK(l.threads >= K && l.threads <= kAggThreads && l.threads % 64 == 0);  // one neighbour per thread, whole waves
    CHECK(pow2(l.cap) && l.cap >= 2 && l.cap <= kCap);
    if (l.form == kAggBuckets) {
        CHECK(l.lds <= kAggBucketLdsMax);
        CHECK(l.cap <= l.threads * kAggPer);
        CHECK(l.cap < 65536);  // positions and the popcount prefix are 16-bit in LDS
        const KnnAggBucketLds b = knn_agg_bucket_lds(l.cap, K, nplaces);
        CHECK(b.total == l.lds);
        // the arrays in their order, none overlapping the next, each aligned for its type
        const size_t words = (size_t)knn_agg_words(nplaces);
        // (bitmap, prefix) and (products, neighbour numbers) share the head of the image, one pair after the other in time
        CHECK(b.bitmap + words * 4 <= b.prefix && b.prefix + words * 2 <= b.start);
        CHECK(b.prod + (size_t)l.cap * 8 <= b.nb && b.nb + (size_t)l.cap * 2 <= b.start);
        CHECK(b.start + (size_t)(l.cap + 1) * 4 <= b.place && b.place + (size_t)l.cap * 4 <= b.entry);
        CHECK(b.entry + (size_t)l.cap * 2 <= b.neighbours && b.neighbours + knn_agg_lds_neighbours(K) <= b.total);
        CHECK(b.start % 8 == 0 && b.place % 8 == 0 && b.prod % 8 == 0 && b.neighbours % 8 == 0);
        CHECK(words * 32 >= (size_t)nplaces);
    } else {
        CHECK(l.lds == knn_agg_lds_sort(l.cap, K, l.key32));
        CHECK(l.fbits >= 1 && ((int64_t)1 << l.fbits) >= l.cap);  // a position fits its field
        if (l.key32) CHECK(nplaces + 2 <= ((int64_t)1 << (32 - l.fbits)));  // place index and the all-ones filler fit above it
        else CHECK(l.fbits == 16);
    }
}

static void check_plan(int K, int64_t r, int64_t nplaces, bool force_sort)
{
    ++cases;
    const KnnAggPlan p = knn_agg_plan(K, r, nplaces, kCap, force_sort);
    const int64_t rows_max = (int64_t)K * (r > 1 ? r : 1);
    CHECK(pow2(p.M) && p.M >= 2 && p.M <= kCap);
    CHECK(p.M >= (rows_max < kCap ? rows_max : kCap));  // every query that fits kAggCap fits the full capacity
    check_launch(p.pass1, K, nplaces);
    CHECK(p.pass1.cap <= p.M && p.pass1.cap <= kAggPass1Cap);
    if (force_sort) CHECK(p.pass1.form == kAggSort);
    // the bucket form wherever its image lets two blocks share a CU
    const bool fits = knn_agg_bucket_lds(p.pass1.cap, K, nplaces).total <= kAggBucketLdsMax;
    CHECK((p.pass1.form == kAggBuckets) == (!force_sort && fits));
    // a flag of pass 1 that a larger capacity or the sort form can clear: more rows than pass 1 holds while the full
    // capacity is larger, or (bucket form) possibly more than kAggBucketMax rows of one place
    const bool rows_flag = rows_max > p.pass1.cap && p.pass1.cap < p.M;
    const bool bucket_flag = p.pass1.form == kAggBuckets && rows_max > kAggBucketMax;
    CHECK(p.redo_needed == (rows_flag || bucket_flag));
    if (rows_max > p.pass1.cap) CHECK(p.pass1.cap < p.M || rows_max > kCap);  // else the flag is final: host assembly
    if (p.redo_needed) {
        check_launch(p.redo, K, nplaces);
        CHECK(p.redo.form == kAggSort && p.redo.cap == p.M && p.redo.threads == kAggThreads);
    } else {
        CHECK(p.redo.form == kAggNone);
    }
}

// ---- phases 4-7 of knn_aggregate_buckets, one row after another; `threads` only decides who owns which bitmap words,
// `order` is the arrival order of the rows at the LDS atomics
struct Summed {
    std::vector<int32_t> place;
    std::vector<double> ws, ss;
};

static Summed model(int64_t nplaces, const std::vector<int32_t> &pidx, const std::vector<double> &prod, const std::vector<int> &nb,
                    const std::vector<double> &sim, int threads, const std::vector<int> &order)
{
    const int T = (int)pidx.size(), words = knn_agg_words(nplaces);
    std::vector<uint32_t> bitmap((size_t)words, 0u);
    for (int f = 0; f < T; ++f) bitmap[(size_t)knn_agg_word_of((uint32_t)pidx[(size_t)f])] |= knn_agg_bit_of((uint32_t)pidx[(size_t)f]);
    // 4. rank
    std::vector<int> prefix((size_t)words, -1);
    const int wpt = knn_agg_words_per_thread(words, threads);
    std::vector<int> pc((size_t)threads, 0);
    for (int t = 0; t < threads; ++t)
        for (int w = std::min(t * wpt, words); w < std::min(std::min(t * wpt, words) + wpt, words); ++w)
            pc[(size_t)t] += __builtin_popcount(bitmap[(size_t)w]);
    int nslots = 0;
    for (int t = 0; t < threads; ++t) {
        int run = nslots;
        for (int w = std::min(t * wpt, words); w < std::min(std::min(t * wpt, words) + wpt, words); ++w) {
            CHECK(prefix[(size_t)w] == -1);  // every word has one owner
            prefix[(size_t)w] = run;
            run += __builtin_popcount(bitmap[(size_t)w]);
        }
        nslots += pc[(size_t)t];
    }
    for (int w = 0; w < words; ++w) CHECK(prefix[(size_t)w] >= 0);
    auto slot_of = [&](int32_t p) {
        const int w = knn_agg_word_of((uint32_t)p);
        return knn_agg_slot(prefix[(size_t)w], bitmap[(size_t)w], (uint32_t)p);
    };
    // 5. bucket
    std::vector<int> start((size_t)nslots + 1, 0), arrival((size_t)T, 0);
    for (int f : order) {
        const int s = slot_of(pidx[(size_t)f]);
        CHECK(s >= 0 && s < nslots);
        arrival[(size_t)f] = start[(size_t)s]++;
    }
    int run = 0;
    for (int s = 0; s < nslots; ++s) {
        const int c = start[(size_t)s];
        CHECK(c > 0);  // a slot exists because a row set its bit
        start[(size_t)s] = run;
        run += c;
    }
    start[(size_t)nslots] = run;
    CHECK(run == T);
    Summed out;
    out.place.assign((size_t)nslots, -1);
    std::vector<int> entry((size_t)T, -1);
    for (int f = 0; f < T; ++f) {
        const int s = slot_of(pidx[(size_t)f]);
        entry[(size_t)(start[(size_t)s] + arrival[(size_t)f])] = f;
        out.place[(size_t)s] = pidx[(size_t)f];
    }
    // 6. order
    std::vector<double> sprod((size_t)T, 0.0);
    std::vector<int> snb((size_t)T, -1);
    for (int f = 0; f < T; ++f) {
        const int s = slot_of(pidx[(size_t)f]);
        int r = start[(size_t)s];
        for (int i = start[(size_t)s]; i < start[(size_t)s + 1]; ++i) r += entry[(size_t)i] < f;
        CHECK(snb[(size_t)r] == -1);
        sprod[(size_t)r] = prod[(size_t)f];
        snb[(size_t)r] = nb[(size_t)f];
    }
    // 7. sum
    for (int s = 0; s < nslots; ++s) {
        double ws = 0.0, ss = 0.0;
        for (int t = start[(size_t)s]; t < start[(size_t)s + 1]; ++t) {
            ws = ws + sprod[(size_t)t];
            ss = ss + sim[(size_t)snb[(size_t)t]];
        }
        out.ws.push_back(ws);
        out.ss.push_back(ss);
    }
    return out;
}

static void check_model(std::mt19937_64 &rng, int64_t nplaces, const std::vector<int32_t> &pidx, int threads)
{
    ++cases;
    const int T = (int)pidx.size();
    const int nnb = 1 + (int)(rng() % 60);
    std::vector<double> sim((size_t)nnb), prod((size_t)T);
    std::vector<int> nb((size_t)T), order((size_t)T);
    // similarities from 1e-17 to 1: a sum in another order has other bits
    for (double &s : sim) s = std::pow(10.0, -17.0 * (double)(rng() % 1000) / 999.0);
    for (int f = 0; f < T; ++f) {
        nb[(size_t)f] = (int)((int64_t)f * nnb / (T > 0 ? T : 1));  // neighbours in rank order, as the flattening has them
        prod[(size_t)f] = (double)(1 + rng() % 5) * sim[(size_t)nb[(size_t)f]];
        order[(size_t)f] = f;
    }
    std::shuffle(order.begin(), order.end(), rng);
    const Summed got = model(nplaces, pidx, prod, nb, sim, threads, order);
    std::map<int32_t, std::vector<int>> by_place;
    for (int f = 0; f < T; ++f) by_place[pidx[(size_t)f]].push_back(f);  // ascending f inside a place
    CHECK(got.place.size() == by_place.size());
    size_t s = 0;
    for (const auto &kv : by_place) {
        double ws = 0.0, ss = 0.0;
        for (int f : kv.second) {
            ws = ws + prod[(size_t)f];
            ss = ss + sim[(size_t)nb[(size_t)f]];
        }
        CHECK(got.place[s] == kv.first);
        CHECK(std::memcmp(&got.ws[s], &ws, 8) == 0 && std::memcmp(&got.ss[s], &ss, 8) == 0);
        ++s;
    }
}

int main()
{
    // ---- the plan over the grid
    const int Ks[] = {1, 50, 512, 1024};
    const int64_t rs[] = {0, 1, 40, 41, 4096};
    int bucket_plans = 0, sort_plans = 0;
    for (int K : Ks)
        for (int64_t r : rs) {
            const int64_t limit = knn_agg_place_limit(K, r, kCap);
            CHECK(limit > 100000 && limit < 1000000);  // cfg2's 100 k places take the bucket form, cfg4's 1 M the sort form
            const int64_t ps[] = {1, 32, 33, 100000, limit, limit + 1, 1000000};
            for (int64_t np : ps)
                for (int force = 0; force < 2; ++force) {
                    check_plan(K, r, np, force != 0);
                    const KnnAggPlan p = knn_agg_plan(K, r, np, kCap, force != 0);
                    (p.pass1.form == kAggBuckets ? bucket_plans : sort_plans)++;
                    if (!force) CHECK((p.pass1.form == kAggBuckets) == (np <= limit));
                }
        }
    CHECK(bucket_plans > 0 && sort_plans > bucket_plans);
    {   // the benchmarked shape: 512-thread bucket blocks of 2,048 rows, three per CU, and a redo launch
        const KnnAggPlan p = knn_agg_plan(50, 60, 100000, kCap, false);
        CHECK(p.M == 4096 && p.pass1.form == kAggBuckets && p.pass1.cap == 2048 && p.pass1.threads == 512 && p.redo_needed);
        CHECK(3 * p.pass1.lds <= kAggLdsMax);
    }
    // ---- the word / bit / slot functions
    CHECK(knn_agg_words(0) == 0 && knn_agg_words(1) == 1 && knn_agg_words(32) == 1 && knn_agg_words(33) == 2);
    CHECK(knn_agg_word_of(31) == 0 && knn_agg_word_of(32) == 1 && knn_agg_bit_of(31) == 0x80000000u && knn_agg_bit_of(32) == 1u);
    CHECK(knn_agg_rank_in_word(0xFFFFFFFFu, 0) == 0 && knn_agg_rank_in_word(0xFFFFFFFFu, 31) == 31);
    CHECK(knn_agg_rank_in_word(0x80000001u, 63) == 1 && knn_agg_slot(7, 0x5u, 34) == 8);
    CHECK(knn_agg_words_per_thread(3125, 512) == 7 && knn_agg_words_per_thread(513, 512) == 2 && knn_agg_words_per_thread(0, 512) == 0);
    // ---- the model against brute force
    std::mt19937_64 rng(20240611);
    const int64_t nps[] = {1, 31, 32, 33, 64, 65, 1000, 16417, 100000};
    const int threads_of[] = {64, 512, 1024};
    for (int64_t np : nps)
        for (int threads : threads_of) {
            // the places of every word boundary and the last place, each several times
            std::vector<int32_t> edge;
            for (int64_t b : {(int64_t)0, (int64_t)31, (int64_t)32, (int64_t)63, (int64_t)64, np - 1})
                if (b >= 0 && b < np)
                    for (int rep = 0; rep < 3; ++rep) edge.push_back((int32_t)b);
            std::shuffle(edge.begin(), edge.end(), rng);
            check_model(rng, np, edge, threads);
            check_model(rng, np, {}, threads);                                   // no rows: every word empty
            check_model(rng, np, {(int32_t)(np - 1)}, threads);                  // one row
            check_model(rng, np, std::vector<int32_t>(200, (int32_t)(np / 2)), threads);  // all rows in one place
            for (int rep = 0; rep < 6; ++rep) {  // random rows: sparse (most words empty) to dense, repeated places
                const int T = 1 + (int)(rng() % 2048);
                const int64_t span = rep < 3 ? np : std::min<int64_t>(np, 1 + (int64_t)(rng() % 300));
                std::vector<int32_t> pidx((size_t)T);
                for (int32_t &p : pidx) p = (int32_t)(np - 1 - (int64_t)(rng() % (uint64_t)span));
                check_model(rng, np, pidx, threads);
            }
        }
    std::printf("knn_agg_plan_check: %ld cases pass\n", cases);
    return 0;
}
