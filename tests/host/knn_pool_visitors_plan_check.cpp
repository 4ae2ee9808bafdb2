// The host decisions of a pool-visitors call (csrc/knn_pool_visitors_plan.h) against brute force and literals: who shares
// on both sides of k = 1024 | 1025 and n - 1 | n; the members' cuts, waves and tiles for member sizes 0, 1, 15, 16, 17 and
// 37 in interleaved call orders; the fill grid at staged lengths 0, 256 and 257; the first offender across members; the
// 48 GiB refusal at its two sides; the stage's buffers.
// Stand-alone: c++ -std=c++17 -I locations-recommender_amd/csrc tests/host/knn_pool_visitors_plan_check.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knn_pool_visitors_plan.h"

using namespace locrec;

static int cases = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        ++cases;                                                        \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
            return 1;                                                   \
        }                                                               \
    } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int main()
{
    using Way = KnnPoolVisitorsWay;
    // who shares: k > 1024 and k >= n and n > 0; a member without persons has no rows whatever K; the rest is delegated
    for (int64_t n : {1, 2, 200, 1024, 1025, 1026, 3000, 4200, 2000000}) {
        for (int64_t k : {(int64_t)1, (int64_t)1024, (int64_t)1025, n - 1, n, n + 1, (int64_t)2000000}) {
            if (k < 1) continue;
            const bool brute = k >= 1025 && k >= n;
            CHECK(knn_pool_visitors_way(k, n) == (brute ? Way::Shared : Way::Delegated));
        }
        CHECK(knn_pool_visitors_way(1024, n) == Way::Delegated);
        CHECK(knn_pool_visitors_way(1025, n) == (n <= 1025 ? Way::Shared : Way::Delegated));
    }
    CHECK(knn_pool_visitors_way(2999, 3000) == Way::Delegated && knn_pool_visitors_way(3000, 3000) == Way::Shared);
    CHECK(knn_pool_visitors_way(1024, 200) == Way::Delegated && knn_pool_visitors_way(1025, 200) == Way::Shared);
    for (int64_t k : {1, 50, 1024, 1025, 2000000}) CHECK(knn_pool_visitors_way(k, 0) == Way::Empty);
    CHECK(kPoolVisitorsBatchMaxK == 1024);

    // cuts, waves and tiles: member sizes 0, 1, 15, 16, 17 and 37 in three call orders (member after member, round robin,
    // shuffled), members 1 and 4 delegated, member 6 without persons
    const std::vector<int64_t> sizes = {0, 1, 15, 16, 17, 37, 3};
    const std::vector<Way> way = {Way::Shared, Way::Delegated, Way::Shared, Way::Shared, Way::Delegated, Way::Shared, Way::Empty};
    for (int order = 0; order < 3; ++order) {
        std::vector<int32_t> index_of;
        if (order == 1) {
            std::vector<int64_t> left(sizes);
            for (bool any = true; any;) {
                any = false;
                for (size_t m = 0; m < sizes.size(); ++m)
                    if (left[m] > 0) {
                        --left[m];
                        index_of.push_back((int32_t)m);
                        any = true;
                    }
            }
        } else {
            for (size_t m = 0; m < sizes.size(); ++m) index_of.insert(index_of.end(), (size_t)sizes[m], (int32_t)m);
            if (order == 2)
                for (size_t i = index_of.size(); i > 1; --i) std::swap(index_of[i - 1], index_of[rnd() % i]);
        }
        const int64_t nv = (int64_t)index_of.size();
        CHECK(nv == 89);
        KnnPoolVisitorsPlan plan;
        knn_pool_visitors_plan(nv, index_of.data(), way, plan);
        CHECK((int64_t)plan.order.size() == nv);
        CHECK(plan.shared.size() == 3 && plan.delegated.size() == 2 && plan.empty.size() == 1);  // (member 0: nobody asks)
        CHECK(plan.shared[0].member == 2 && plan.shared[1].member == 3 && plan.shared[2].member == 5);
        CHECK(plan.delegated[0].member == 1 && plan.delegated[1].member == 4 && plan.empty[0].member == 6);
        std::vector<char> seen((size_t)nv, 0);
        for (const auto *cuts : {&plan.shared, &plan.delegated, &plan.empty})
            for (const auto &c : *cuts) {
                CHECK(c.n == sizes[(size_t)c.member]);
                // brute force: the member's visitors are the positions that name it, ascending
                std::vector<int64_t> want;
                for (int64_t i = 0; i < nv; ++i)
                    if (index_of[(size_t)i] == c.member) want.push_back(i);
                CHECK((int64_t)want.size() == c.n);
                for (int64_t j = 0; j < c.n; ++j) {
                    CHECK(plan.order[(size_t)(c.first + j)] == want[(size_t)j]);
                    CHECK(!seen[(size_t)want[(size_t)j]]);
                    seen[(size_t)want[(size_t)j]] = 1;
                }
            }
        for (char s : seen) CHECK(s);
        // waves: 37 visitors make three, the last tile holds 5; every visitor of a sharing member is in exactly one tile
        CHECK(knn_pool_visitors_waves(plan.shared) == 3);
        const int want_tiles[3][3] = {{15, 16, 16}, {0, 0, 16}, {0, 0, 5}};
        int64_t tiles = 0;
        for (int64_t w = 0; w < 3; ++w)
            for (size_t i = 0; i < 3; ++i) {
                CHECK(knn_wave_tile(plan.shared[i].n, w) == want_tiles[w][i]);
                tiles += want_tiles[w][i] > 0;
            }
        CHECK(tiles == 5);
        CHECK(knn_wave_tile(plan.shared[2].n, 3) == 0);
    }
    CHECK(knn_waves_of(0) == 0 && knn_waves_of(1) == 1 && knn_waves_of(15) == 1 && knn_waves_of(16) == 1 && knn_waves_of(17) == 2 &&
          knn_waves_of(37) == 3);
    CHECK(knn_wave_tile(17, 1) == 1 && knn_wave_tile(16, 1) == 0 && knn_wave_tile(1, 0) == 1 && knn_wave_tile(0, 0) == 0);
    {
        KnnPoolVisitorsPlan plan;
        knn_pool_visitors_plan(0, nullptr, way, plan);
        CHECK(plan.order.empty() && plan.shared.empty() && plan.delegated.empty() && plan.empty.empty());
        CHECK(knn_pool_visitors_waves(plan.shared) == 0);
    }

    // the fill grid of a tile: the longest staged vector of either family among the listed visitors; 0 entries still one block
    {
        const int64_t nv = 6;
        //                         places                     categories
        const int32_t lens[12] = {0, 256, 257, 3, 0, 100, /**/ 0, 1, 2, 600, 0, 256};
        const int64_t a[] = {0, 4}, b[] = {0, 1}, c[] = {1, 2}, d[] = {4, 3, 0}, e[] = {5};
        CHECK(knn_pool_visitors_fill_blocks(lens, nv, a, 2) == 1);   // 0 entries
        CHECK(knn_pool_visitors_fill_blocks(lens, nv, b, 2) == 1);   // 256
        CHECK(knn_pool_visitors_fill_blocks(lens, nv, c, 2) == 2);   // 257
        CHECK(knn_pool_visitors_fill_blocks(lens, nv, d, 3) == 3);   // the category family decides: 600
        CHECK(knn_pool_visitors_fill_blocks(lens, nv, e, 1) == 1);   // 256 categories
        CHECK(knn_pool_visitors_fill_blocks(lens, nv, a, 0) == 1);
        for (int trial = 0; trial < 200; ++trial) {
            int64_t vis[16];
            const int nt = 1 + (int)(rnd() % 16);
            int32_t longest = 1;
            for (int t = 0; t < nt; ++t) {
                vis[t] = (int64_t)(rnd() % nv);
                longest = std::max(longest, std::max(lens[vis[t]], lens[nv + vis[t]]));
            }
            CHECK(knn_pool_visitors_fill_blocks(lens, nv, vis, nt) == (unsigned)((longest + 255) / 256));
        }
    }

    // the first offender: the minimum report word = the smallest position in call order whatever the members, within it the
    // place family first
    {
        struct R { int64_t v; int f; unsigned code; };
        const R reports[] = {{9, 0, 7}, {3, 1, 3}, {3, 0, 8}, {200, 0, 1}, {4, 0, 2}};  // (member 0's visitor 9, member 1's visitor 3, ...)
        unsigned long long word = kVisitorsNoReport;
        for (const R &r : reports) word = std::min(word, knn_visitors_report_word(r.v, r.f, r.code));
        const KnnVisitorsOffender o = knn_visitors_first_offender(word);
        CHECK(o.visitor == 3 && o.family == 0 && o.code == 8);
        for (int trial = 0; trial < 200; ++trial) {
            unsigned long long w = kVisitorsNoReport;
            int64_t bv = -1;
            int bf = 2;
            unsigned bc = 0;
            const int n = 1 + (int)(rnd() % 6);
            for (int i = 0; i < n; ++i) {
                const int64_t v = (int64_t)(rnd() % ((uint64_t)1 << 30));
                const int f = (int)(rnd() % 2);
                const unsigned code = 1 + (unsigned)(rnd() % 8);
                if (bv < 0 || v < bv || (v == bv && f < bf)) {
                    bv = v; bf = f; bc = code;
                } else if (v == bv && f == bf) {
                    bc = std::min(bc, code);  // (one (visitor, family) reports once on the device: a tie never arises there)
                }
                w = std::min(w, knn_visitors_report_word(v, f, code));
            }
            const KnnVisitorsOffender g = knn_visitors_first_offender(w);
            CHECK(g.visitor == bv && g.family == bf && g.code == bc);
        }
        CHECK(knn_visitors_report_word(kVisitorsMax, 1, 8) < kVisitorsNoReport);
    }

    // the refusal: the call's total of max(1, rated places of the member) x 16 bytes a visitor, beyond 48 GiB
    {
        const int64_t lim = (int64_t)48 << 30;
        CHECK(kVisitorsMaxRowBytes == lim);
        const int64_t nvs[] = {1 << 20, 1 << 20, 5}, places[] = {2048, 1024, 0};
        CHECK(knn_pool_visitors_worst_row_bytes(2, nvs, places) == lim);       // 32 GiB + 16 GiB: just held
        CHECK(knn_pool_visitors_worst_row_bytes(3, nvs, places) > lim);        // and five visitors of a member without rated places
        const int64_t one = 1, p = 3000;
        CHECK(knn_pool_visitors_worst_row_bytes(1, &one, &p) == 48000);
        CHECK(knn_pool_visitors_worst_row_bytes(0, nullptr, nullptr) == 0);
        const int64_t huge_n[] = {(int64_t)1 << 30, (int64_t)1 << 30}, huge_p[] = {(int64_t)1 << 27, (int64_t)1 << 27};
        CHECK(knn_pool_visitors_worst_row_bytes(2, huge_n, huge_p) > lim);      // (2^62 bytes a member: no overflow)
        for (int trial = 0; trial < 200; ++trial) {
            int64_t n[4], q[4];
            __int128 brute = 0;
            for (int j = 0; j < 4; ++j) {
                n[j] = (int64_t)(rnd() % 100000);
                q[j] = (int64_t)(rnd() % 20000);
                brute += (__int128)n[j] * (q[j] > 1 ? q[j] : 1) * 16;
            }
            const int64_t got = knn_pool_visitors_worst_row_bytes(4, n, q);
            CHECK((brute > lim) == (got > lim));
            if (brute <= lim) CHECK(got == (int64_t)brute);
        }
    }

    // the stage's buffers: the per-index stage's for ONE CSR over all visitors, a member per visitor, a row per member
    {
        const KnnPoolVisitorsStageSizes s = knn_pool_visitors_stage_sizes(37, 1000, 0, 7);
        CHECK(s.one.bounds == 74 && s.one.p_elems == 1000 && s.one.c_elems == 1 && s.one.norms == 37 && s.one.lens == 74);
        CHECK(s.member_of == 37 && s.members == 7);
        CHECK(knn_visitors_stage_row(36) == 72);
    }
    printf("%d cases pass\n", cases);
    return 0;
}
