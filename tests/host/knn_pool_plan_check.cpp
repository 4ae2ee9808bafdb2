// knn_pool_plan_check.cpp -- the host arithmetic of the large-K batch and the pool of indexes (csrc/knn_pool_plan.h)
// against brute-force re-computation: the request plan, a tile's bases, the waves, the row buffer's growth.  Stand-alone,
// so that it also runs under a host sanitizer:
//   g++ -std=c++17 -fsanitize=address,undefined -I locations-recommender_amd/csrc tests/host/knn_pool_plan_check.cpp
// Prints the number of cases and returns 0, or the first failed check and 1.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "knn_pool_plan.h"

using namespace locrec;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "%s:%d: %s fails (case %ld)\n", __FILE__, __LINE__, #cond, cases); \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

static long cases = 0;

// ---- the request plan by its definition, request by request and member by member
static void check_requests(const std::vector<int32_t> &index_of, const std::vector<int32_t> &row, const std::vector<char> &shares)
{
    ++cases;
    const int64_t n = (int64_t)index_of.size();
    KnnPoolRequests p;
    knn_pool_requests(n, index_of.data(), row.data(), shares, p);
    CHECK((int64_t)p.distinct_of.size() == n && p.requests_of.size() == p.delegated.size());
    size_t cut = 0, del = 0;
    int64_t at = 0;
    for (int32_t m = 0; m < (int32_t)shares.size(); ++m) {
        std::vector<int64_t> asked;   // the member's requests, in input order
        std::set<int32_t> want;       // its distinct rows
        for (int64_t i = 0; i < n; ++i)
            if (index_of[(size_t)i] == m) {
                asked.push_back(i);
                want.insert(row[(size_t)i]);
            }
        if (asked.empty()) continue;  // a member nobody asks appears nowhere
        if (!shares[(size_t)m]) {
            CHECK(del < p.delegated.size() && p.delegated[del] == m && p.requests_of[del] == asked);
            for (const int64_t i : asked) CHECK(p.distinct_of[(size_t)i] == -1);
            ++del;
            continue;
        }
        CHECK(cut < p.cuts.size() && p.cuts[cut].member == m && p.cuts[cut].first == at && p.cuts[cut].n == (int64_t)want.size());
        CHECK(at + (int64_t)want.size() <= (int64_t)p.rows.size());
        CHECK(std::equal(want.begin(), want.end(), p.rows.begin() + at));   // each distinct row once, ascending
        for (const int64_t i : asked) {
            const int64_t u = p.distinct_of[(size_t)i];
            CHECK(u >= at && u < at + (int64_t)want.size() && p.rows[(size_t)u] == row[(size_t)i]);
        }
        at += (int64_t)want.size();
        ++cut;
    }
    CHECK(cut == p.cuts.size() && del == p.delegated.size() && at == (int64_t)p.rows.size());
}

static void request_cases()
{
    for (const int n : {0, 1, 16, 17, 33})          // sizes: one member, distinct rows in a scrambled order
        for (const char shared : {1, 0}) {
            std::vector<int32_t> idx((size_t)n, 0), row((size_t)n);
            for (int i = 0; i < n; ++i) row[(size_t)i] = (i * 7 + 3) % 40;
            check_requests(idx, row, {shared});
        }
    // member mixes over five members (member 3 is asked by nobody): only shared, only delegated, interleaved
    const std::vector<int32_t> idx = {4, 0, 2, 0, 1, 4, 2, 0, 1, 4, 0, 2}, row = {5, 9, 1, 2, 7, 5, 8, 9, 7, 0, 30, 1};
    check_requests(idx, row, {1, 1, 1, 1, 1});
    check_requests(idx, row, {0, 0, 0, 0, 0});
    check_requests(idx, row, {1, 0, 1, 0, 0});
    check_requests(idx, row, {0, 1, 0, 1, 1});
    // repeats and gaps: a pair repeated side by side and far apart; one row asked of two members; members 1 and 3 unasked
    const std::vector<int32_t> ridx = {2, 2, 0, 4, 0, 0, 4, 2, 0, 2}, rrow = {6, 6, 6, 3, 1, 12, 6, 0, 6, 6};
    check_requests(ridx, rrow, {1, 1, 1, 1, 1});
    check_requests(ridx, rrow, {1, 1, 0, 1, 1});
    check_requests(ridx, rrow, {0, 1, 1, 1, 0});
}

// ---- a tile's bases: slot t's rows lie behind those of the slots before it
static void check_bases(int nt, int tiles, int invalid_at, bool all_invalid, int64_t total0)
{
    ++cases;
    int32_t qrow[kLkbQt];
    std::vector<int32_t> cnt((size_t)kLkbQt * tiles);
    for (int t = 0; t < kLkbQt; ++t) {
        qrow[t] = t < nt && !all_invalid && t != invalid_at ? 100 + t : -1;
        // what the device leaves: an invalid slot's column of S is all zero, so are its counts; past nt: anything
        for (int i = 0; i < tiles; ++i) cnt[(size_t)t * tiles + i] = t >= nt ? 77 : qrow[t] < 0 ? 0 : (t * 5 + i * 3 + nt) % 11;
    }
    int64_t base[kLkbQt], len[kLkbQt];
    const int64_t total = knn_tile_bases(cnt.data(), tiles, nt, qrow, total0, base, len);
    int64_t at = total0;
    for (int t = 0; t < kLkbQt; ++t) {
        int64_t c = 0;
        for (int i = 0; i < tiles; ++i) c += t < nt ? cnt[(size_t)t * tiles + i] : 0;   // (the rule without the qrow test)
        CHECK(base[t] == (t < nt ? at : -1) && len[t] == c);
        if (qrow[t] < 0) CHECK(len[t] == 0);
        at += c;
    }
    CHECK(total == at);
}

static void base_cases()
{
    for (const int nt : {1, 15, 16})
        for (const int tiles : {1, 3})
            for (const int64_t total0 : {(int64_t)0, ((int64_t)1 << 31) + 5}) {
                check_bases(nt, tiles, -1, false, total0);
                for (const int at : {0, nt / 2, nt - 1}) check_bases(nt, tiles, at, false, total0);
                check_bases(nt, tiles, -1, true, total0);
            }
}

// ---- waves: request j of a batch belongs to the batch's tile j / kLkbQt, and wave w is every batch's w-th tile
static void wave_cases()
{
    ++cases;
    const std::vector<int64_t> batches = {0, 1, 16, 17, 32, 37};
    int64_t waves = 0;
    for (const int64_t n : batches) waves = std::max(waves, knn_waves_of(n));
    std::vector<std::vector<int>> in((size_t)waves + 1, std::vector<int>(batches.size(), 0));
    int64_t last = -1;
    for (size_t b = 0; b < batches.size(); ++b)
        for (int64_t j = 0; j < batches[b]; ++j) {
            CHECK(j / kLkbQt < waves);
            ++in[(size_t)(j / kLkbQt)][b];
            last = std::max(last, j / kLkbQt);
        }
    CHECK(waves == last + 1 && waves == 3);
    for (int64_t w = 0; w <= waves; ++w)   // (one past the last wave: nobody)
        for (size_t b = 0; b < batches.size(); ++b) CHECK(knn_wave_tile(batches[b], w) == in[(size_t)w][b]);
    CHECK(knn_waves_of(0) == 0 && knn_waves_of(1) == 1 && knn_waves_of(16) == 1 && knn_waves_of(17) == 2 && knn_waves_of(32) == 2);
}

static void growth_cases()
{
    for (const int64_t total : {(int64_t)0, (int64_t)1, (int64_t)1023, (int64_t)2049, ((int64_t)1 << 32) + 1}) {
        ++cases;
        CHECK(knn_rows_room(total) == (size_t)(total + total / 2 + 1024) && knn_rows_room(total) > (size_t)total);
    }
}

int main()
{
    request_cases();
    base_cases();
    wave_cases();
    growth_cases();
    std::printf("knn_pool_plan_check: %ld cases pass\n", cases);
    return 0;
}
