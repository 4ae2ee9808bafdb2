// knn_topk_plan_check.cpp -- the host arithmetic of the batched top-K (csrc/knn_topk_plan.h): the chunk plan of a tiled
// scan and its merge levels against their invariants over a sweep and against tuples recorded from the arithmetic as it
// stood inside enqueue_topk before it moved; the admission to the head / tail form against a brute-force recomputation;
// knn_side_topk's LDS against the formula evaluated by hand.  Stand-alone, so that it also runs under a host sanitizer:
//   g++ -std=c++17 -fsanitize=address,undefined -I locations-recommender_amd/csrc tests/host/knn_topk_plan_check.cpp
// Prints the number of cases and returns 0, or the first failed check and 1.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "knn_topk_plan.h"

using namespace locrec;

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "%s:%d: %s fails (case %ld)\n", __FILE__, __LINE__, #cond, cases); \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

static long cases = 0;

static bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// ---- the chunk plan: every slice in exactly one chunk, no chunk empty, the merge holds its lists and fits the LDS
static void check_chunks(int range_slices, int64_t nq, int qt, int waves, int K, bool use_ht, int env_blocks)
{
    ++cases;
    const KnnTopkChunks c = knn_topk_chunks(range_slices, nq, qt, waves, K, use_ht, env_blocks);
    const int64_t spc = c.slices_per_chunk, nch = c.nchunks, mc = c.max_chunks;
    CHECK(c.ntiles == (int)((nq + qt - 1) / qt) && mc == std::max(1, 8192 / K));
    CHECK(spc > 0 && spc % waves == 0);
    CHECK((nch - 1) * spc < range_slices && range_slices <= nch * spc);
    CHECK(nch <= mc * mc);
    CHECK((c.ngroups == 0) == (nch <= mc));
    if (c.ngroups) CHECK(((int64_t)c.ngroups - 1) * mc < nch && nch <= (int64_t)c.ngroups * mc);
    const int64_t flists = c.ngroups ? c.ngroups : nch;
    CHECK(pow2(c.M) && c.M >= 2 && c.M >= flists * K);
    if (c.ngroups) CHECK(pow2(c.M1) && c.M1 >= mc * K);
    else CHECK(c.M1 == 0);
    CHECK(c.lds_merge == (size_t)c.M * 12 && c.lds_partial == (size_t)c.M1 * 12);
    CHECK(c.lds_merge <= 163840 && c.lds_partial <= 163840 && kTopkLdsMax == 163840);
}

static void chunk_sweep()
{
    for (const int64_t nq : {(int64_t)1, (int64_t)2, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)16384})
        for (const int qt : {1, 8, 16, 32})
            for (const int waves : {4, 8, 16})
                for (const int K : {1, 2, 50, 1023, 1024})
                    for (const bool use_ht : {false, true})
                        for (const int env_blocks : {0, 1, 100000}) {
                            std::set<int64_t> ranges;
                            for (int r = 1; r <= 40; ++r) ranges.insert(r);
                            // around every multiple of the block's waves, as far as 1,024 slices: where slices_per_chunk's
                            // rounding to whole blocks changes the chunk count
                            for (int m = waves; m <= 1024; m += waves)
                                for (int d = -1; d <= 1; ++d) ranges.insert(m + d);
                            // around 8 x each bound of the chunk count (range_slices / 8 caps it): the block target per
                            // tile, the lists of one merge block (where the second level begins), their square
                            const int64_t ntiles = (nq + qt - 1) / qt, mc = std::max(1, 8192 / K);
                            int64_t want = std::max<int64_t>(1, ((use_ht ? 1024 : 2048) + ntiles - 1) / ntiles);
                            if (env_blocks > 0) want = std::max<int64_t>(1, (env_blocks + ntiles - 1) / ntiles);
                            for (const int64_t b : {want, mc, mc * mc})
                                for (int d = -1; d <= 1; ++d) ranges.insert(8 * b + d);
                            ranges.insert(4096);
                            ranges.insert(15625);  // cfg2: 1,000,000 persons
                            ranges.insert(200000);
                            for (const int64_t r : ranges)
                                if (r >= 1 && r < ((int64_t)1 << 30)) check_chunks((int)r, nq, qt, waves, K, use_ht, env_blocks);
                        }
}

// (range_slices, nq, qt, waves, K, use_ht, env_blocks) -> (ntiles, nchunks, slices_per_chunk, ngroups, M1, M, the two LDS
// sizes) as enqueue_topk computed them in place before the arithmetic moved into the header (M1 and its LDS: 0 without groups)
static void parent_cases()
{
    static const long long T[][15] = {
        {1, 1, 1, 4, 1, 0, 0, /* -> */ 1, 1, 4, 0, 0, 2, 0, 24},
        {7, 2, 8, 8, 50, 1, 0, /* -> */ 1, 1, 8, 0, 0, 64, 0, 768},
        {40, 15, 16, 16, 2, 0, 1, /* -> */ 1, 1, 48, 0, 0, 2, 0, 24},
        {33, 16, 16, 8, 50, 1, 0, /* -> */ 1, 3, 16, 0, 0, 256, 0, 3072},
        {63, 17, 32, 4, 1023, 0, 0, /* -> */ 1, 6, 12, 0, 0, 8192, 0, 98304},
        {64, 1, 1, 8, 1024, 0, 0, /* -> */ 1, 8, 8, 0, 0, 8192, 0, 98304},
        {65, 1, 8, 8, 50, 0, 0, /* -> */ 1, 5, 16, 0, 0, 256, 0, 3072},
        {4096, 1, 16, 8, 50, 0, 0, /* -> */ 1, 512, 8, 4, 8192, 256, 98304, 3072},
        {4096, 16384, 16, 8, 50, 1, 0, /* -> */ 1024, 1, 4096, 0, 0, 64, 0, 768},
        {15625, 16384, 16, 8, 50, 1, 0, /* -> */ 1024, 1, 15632, 0, 0, 64, 0, 768},
        {15625, 16384, 32, 4, 50, 0, 0, /* -> */ 512, 4, 3908, 0, 0, 256, 0, 3072},
        {15625, 1, 1, 4, 50, 0, 0, /* -> */ 1, 1303, 12, 8, 8192, 512, 98304, 6144},
        {15625, 1, 1, 4, 1, 0, 100000, /* -> */ 1, 1303, 12, 0, 0, 2048, 0, 24576},
        {15625, 17, 16, 16, 1024, 0, 100000, /* -> */ 2, 62, 256, 8, 8192, 8192, 98304, 98304},
        {200000, 1, 1, 4, 2, 0, 0, /* -> */ 1, 2000, 100, 0, 0, 4096, 0, 49152},
        {200000, 1, 1, 4, 1, 0, 100000, /* -> */ 1, 25000, 8, 4, 8192, 4, 98304, 48},
        {200000, 2, 8, 8, 1023, 1, 0, /* -> */ 1, 64, 3128, 8, 8192, 8192, 98304, 98304},
        {200000, 16384, 16, 8, 1024, 1, 100000, /* -> */ 1024, 64, 3128, 8, 8192, 8192, 98304, 98304},
        {1311, 15, 8, 16, 50, 0, 0, /* -> */ 2, 82, 16, 0, 0, 8192, 0, 98304},
        {1304, 16, 16, 8, 2, 0, 100000, /* -> */ 1, 163, 8, 0, 0, 512, 0, 6144},
        {1311, 1, 1, 4, 50, 0, 0, /* -> */ 1, 110, 12, 0, 0, 8192, 0, 98304},
        {1312, 1, 1, 4, 50, 0, 0, /* -> */ 1, 164, 8, 2, 8192, 128, 98304, 1536},
    };
    for (const auto &t : T) {
        ++cases;
        const KnnTopkChunks c = knn_topk_chunks((int)t[0], t[1], (int)t[2], (int)t[3], (int)t[4], t[5] != 0, (int)t[6]);
        CHECK(c.ntiles == t[7] && c.nchunks == t[8] && c.slices_per_chunk == t[9] && c.ngroups == t[10] && c.M1 == t[11] &&
              c.M == t[12] && (long long)c.lds_partial == t[13] && (long long)c.lds_merge == t[14]);
    }
}

// ---- admission to the head / tail form: every tile's sums, recomputed tile by tile from a map of the batch
static void check_admit(const std::vector<int32_t> *rows, int32_t row0, int64_t nq, int qt, const std::vector<int32_t> &tail_nnz,
                        const std::vector<int64_t> &hits, int64_t max_entries)
{
    ++cases;
    std::vector<int64_t> ps(hits.size() + 1, 0);
    for (size_t r = 0; r < hits.size(); ++r) ps[r + 1] = ps[r] + hits[r];
    std::map<int64_t, std::pair<int64_t, int64_t>> tile;  // tile -> (entries, hits)
    int64_t all = 0;
    for (int64_t i = 0; i < nq; ++i) {
        const int32_t r = rows ? (*rows)[(size_t)i] : row0 + (int32_t)i;
        tile[i / qt].first += tail_nnz[(size_t)r];
        tile[i / qt].second += hits[(size_t)r];
        all += hits[(size_t)r];
    }
    bool want = true;
    for (const auto &t : tile) want = want && t.second.first <= max_entries && t.second.second < ((int64_t)1 << 32);
    int64_t total = -1;
    const bool got = knn_topk_admit_head_tail(rows ? rows->data() : nullptr, row0, nq, qt, tail_nnz.data(), ps.data(), max_entries, &total);
    CHECK(got == want);
    if (got) CHECK(total == all);
}

static void admit_cases()
{
    std::mt19937_64 rng(20240521);
    for (int round = 0; round < 400; ++round) {
        const int n = 1 + (int)(rng() % 300);
        const int nnz_scale = round % 4 == 0 ? 200 : 40;                       // some tiles beyond kHtMaxEntries, most within
        const int64_t hit_scale = round % 5 == 0 ? (int64_t)1 << 29 : 100000;   // some tiles at 2^32 hits and beyond
        std::vector<int32_t> tail_nnz((size_t)n);
        std::vector<int64_t> hits((size_t)n);
        for (int r = 0; r < n; ++r) {
            tail_nnz[(size_t)r] = (int32_t)(rng() % (uint64_t)nnz_scale);
            hits[(size_t)r] = (int64_t)(rng() % (uint64_t)hit_scale);
        }
        for (const int qt : {1, 8, 16, 32}) {
            const int32_t row0 = (int32_t)(rng() % (uint64_t)n);
            check_admit(nullptr, row0, 1 + (int64_t)(rng() % (uint64_t)(n - row0)), qt, tail_nnz, hits, kTopkHtMaxEntries);
            std::vector<int32_t> rows(1 + (size_t)(rng() % 100));
            for (auto &r : rows) r = (int32_t)(rng() % (uint64_t)n);
            check_admit(&rows, 0, (int64_t)rows.size(), qt, tail_nnz, hits, kTopkHtMaxEntries);
        }
    }
    // a tile exactly at the limit of the pre-pass's LDS entries, and one entry over; the second tile decides
    std::vector<int32_t> tail_nnz(32, 0);
    std::vector<int64_t> hits(32, 1);
    for (int r = 16; r < 32; ++r) tail_nnz[(size_t)r] = kTopkHtMaxEntries / 16;
    std::vector<int64_t> ps(33, 0);
    for (int r = 0; r < 32; ++r) ps[(size_t)r + 1] = ps[(size_t)r] + hits[(size_t)r];
    int64_t total = 0;
    ++cases;
    CHECK(knn_topk_admit_head_tail(nullptr, 0, 32, 16, tail_nnz.data(), ps.data(), kTopkHtMaxEntries, &total) && total == 32);
    check_admit(nullptr, 0, 32, 16, tail_nnz, hits, kTopkHtMaxEntries);
    tail_nnz[31] += 1;
    ++cases;
    CHECK(!knn_topk_admit_head_tail(nullptr, 0, 32, 16, tail_nnz.data(), ps.data(), kTopkHtMaxEntries, &total));
    CHECK(knn_topk_admit_head_tail(nullptr, 0, 16, 16, tail_nnz.data(), ps.data(), kTopkHtMaxEntries, &total));  // the first tile alone
    check_admit(nullptr, 0, 32, 16, tail_nnz, hits, kTopkHtMaxEntries);
    // ... and a tile one hit short of a 32-bit offset, and exactly at 2^32
    tail_nnz.assign(32, 1);
    hits.assign(32, 0);
    hits[3] = ((int64_t)1 << 32) - 1;
    check_admit(nullptr, 0, 32, 16, tail_nnz, hits, kTopkHtMaxEntries);
    for (int r = 0; r < 32; ++r) ps[(size_t)r + 1] = ps[(size_t)r] + hits[(size_t)r];
    ++cases;
    CHECK(knn_topk_admit_head_tail(nullptr, 0, 32, 16, tail_nnz.data(), ps.data(), kTopkHtMaxEntries, &total));
    hits[4] = 1;
    for (int r = 0; r < 32; ++r) ps[(size_t)r + 1] = ps[(size_t)r] + hits[(size_t)r];
    ++cases;
    CHECK(!knn_topk_admit_head_tail(nullptr, 0, 32, 16, tail_nnz.data(), ps.data(), kTopkHtMaxEntries, &total));
    check_admit(nullptr, 0, 32, 16, tail_nnz, hits, kTopkHtMaxEntries);
}

// ---- knn_side_topk's LDS: cap * 12 + c_dim * 8 + hash_cap * 12, by hand
static void side_cases()
{
    ++cases;
    KnnSideTopkLds l = knn_side_topk_lds(50, 0, 10, 20);  // cap 64 (>= 50), hash 64 (>= 20): 768 + 160 + 768
    CHECK(l.cap == 64 && l.hash_cap == 64 && l.slds == 1696);
    ++cases;
    l = knn_side_topk_lds(50, 1000, 3000, 64);  // cap 2048 (>= 1050), hash 8192 (>= 6000): 24576 + 512 + 98304
    CHECK(l.cap == 2048 && l.hash_cap == 8192 && l.slds == 123392);
    ++cases;
    l = knn_side_topk_lds(1024, 1, 5000, 1);  // cap 2048 (>= 1025), hash 8192 (its most): 24576 + 8 + 98304
    CHECK(l.cap == 2048 && l.hash_cap == 8192 && l.slds == 122888);
}

int main()
{
    chunk_sweep();
    parent_cases();
    admit_cases();
    side_cases();
    std::printf("knn_topk_plan_check: %ld cases pass\n", cases);
    return 0;
}
