// The host decisions of a visitors call (csrc/knn_visitors_plan.h) against brute force and literals: the regime and K_eff on
// both sides of k = n - 1, n; the chunks of the neighbour lists on both sides of 2 GiB; the fill grid; the stage's buffers.
// Stand-alone: c++ -std=c++17 -I locations-recommender_amd/csrc tests/host/knn_visitors_plan_check.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knn_visitors_plan.h"

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

int main()
{
    // the regime: a visitor is no candidate, so all n persons are - "every positive neighbour" begins at k = n, not n - 1
    for (int64_t n : {1, 2, 255, 256, 2960, 1000000}) {
        CHECK(knn_visitors_all(n, n) && knn_visitors_all(n + 1, n) && knn_visitors_all(2000000000, n));
        if (n > 1) CHECK(!knn_visitors_all(n - 1, n));
        CHECK(knn_visitors_keff(n - 1 > 0 ? n - 1 : 1, n) == (n - 1 > 0 ? n - 1 : 1));
        CHECK(knn_visitors_keff(n, n) == n && knn_visitors_keff(n + 1, n) == n && knn_visitors_keff(2000000, n) == (n < 2000000 ? n : 2000000));
        CHECK(knn_visitors_keff(1, n) == 1);
    }
    CHECK(!knn_visitors_all(2959, 2960) && knn_visitors_all(2960, 2960));
    CHECK(knn_visitors_keff(5, 0) == 1);  // (an index without persons: the selection kernels still divide by K_eff)
    // chunks: the largest number of visitors whose nv x k entries of 20 bytes stay within 2 GiB, whole tiles from 16 on
    for (int64_t k : {1, 50, 1024, 1025, 2959, 2960, 2000000, 6710886, 6710887, 107374182, 107374183, 2000000000}) {
        const int64_t c = knn_visitors_chunk(k);
        int64_t brute = 1;
        while ((brute + 1) * k * 20 <= ((int64_t)2 << 30)) {
            ++brute;
            if (brute > 4096 && k < 1000) break;  // (small K: checked by the formula below)
        }
        CHECK(c >= 1);
        CHECK(c * k * 20 <= ((int64_t)2 << 30) || c == 1);
        if (k >= 1000) CHECK(c == (brute >= 16 ? brute / 16 * 16 : brute));
        CHECK(c < 16 || c % 16 == 0);
    }
    CHECK(knn_visitors_chunk(2000000) == 48);           // 53 fit: three whole tiles
    CHECK(knn_visitors_chunk(6710886) == 16);           // 16 x 6,710,886 x 20 = 2 GiB - 32 bytes: one tile still fits ...
    CHECK(knn_visitors_chunk(6710887) == 15);           // ... and no longer
    CHECK(knn_visitors_chunk(107374182) == 1 && knn_visitors_chunk(107374183) == 1);   // one list beyond 2 GiB: still served
    CHECK(knn_visitors_chunk(1) == ((int64_t)2 << 30) / 20 / 16 * 16);
    // the budget as an argument (LOCREC_KNN_VISITORS_CHUNK_BYTES): brute force at 100 bytes, at 320 x K (one tile, to the
    // byte) and at the default, which is what the one-argument form takes
    for (int64_t k : {1, 2, 5, 50, 304, 305, 2960, 2965, 2000000, 6710886, 6710887}) {
        for (int64_t budget : {(int64_t)100, 320 * k - 1, 320 * k, 320 * k + 19, 2 * 320 * k - 1, 2 * 320 * k, (int64_t)2 << 30}) {
            int64_t brute = 0;  // the most visitors whose lists fit, by counting
            while ((brute + 1) * k * 20 <= budget && brute < 70000) ++brute;
            const int64_t c = knn_visitors_chunk(k, budget);
            CHECK(c >= 1 && (c < 16 || c % 16 == 0));
            if (brute < 70000) CHECK(c == (brute >= 16 ? brute / 16 * 16 : brute >= 1 ? brute : 1));
            CHECK(c == 1 || c * k * 20 <= budget);
        }
        CHECK(knn_visitors_chunk(k, 320 * k) == 16 && knn_visitors_chunk(k, 320 * k - 1) == 15);
        CHECK(knn_visitors_chunk(k, 100 * k) == 5 && knn_visitors_chunk(k, 640 * k) == 32 && knn_visitors_chunk(k, 640 * k - 1) == 16);
        CHECK(knn_visitors_chunk(k, (int64_t)2 << 30) == knn_visitors_chunk(k));
    }
    CHECK(knn_visitors_chunk(1, 100) == 5 && knn_visitors_chunk(5, 100) == 1 && knn_visitors_chunk(6, 100) == 1);
    // the switch's text: unset, empty and no number are the default; clamped to [1, 2 GiB]
    CHECK(knn_visitors_chunk_budget(nullptr) == kVisitorsChunkBytes && knn_visitors_chunk_budget("") == kVisitorsChunkBytes);
    CHECK(knn_visitors_chunk_budget("x") == kVisitorsChunkBytes && knn_visitors_chunk_budget("100") == 100);
    CHECK(knn_visitors_chunk_budget("0") == 1 && knn_visitors_chunk_budget("-5") == 1);
    CHECK(knn_visitors_chunk_budget("2147483648") == kVisitorsChunkBytes && knn_visitors_chunk_budget("2147483647") == 2147483647);
    CHECK(knn_visitors_chunk_budget("99999999999999999999999") == kVisitorsChunkBytes);
    // rows a recommendation call may leave: refused beyond 48 GB
    CHECK(knn_visitors_worst_row_bytes(49152, 65536) == kVisitorsMaxRowBytes);          // 3 x 2^30 rows: served ...
    CHECK(knn_visitors_worst_row_bytes(49153, 65536) > kVisitorsMaxRowBytes);           // ... one visitor more: refused
    CHECK(knn_visitors_worst_row_bytes(1024, 100000) == (int64_t)1024 * 100000 * 16);
    CHECK(knn_visitors_worst_row_bytes(33, 0) == 33 * 16);
    CHECK(knn_visitors_worst_row_bytes(32212, 100000) <= kVisitorsMaxRowBytes && knn_visitors_worst_row_bytes(32212, 100001) > kVisitorsMaxRowBytes);
    // the fill grid: blocks of 256 over the longest staged vector of the tile's visitors, at least one
    {
        std::vector<int32_t> len = {0, 255, 256, 257, 1, 512, 513, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2097151};
        CHECK(knn_visitors_fill_blocks(len.data(), 0, 1) == 1);
        CHECK(knn_visitors_fill_blocks(len.data(), 0, 2) == 1);
        CHECK(knn_visitors_fill_blocks(len.data(), 0, 3) == 1);
        CHECK(knn_visitors_fill_blocks(len.data(), 0, 4) == 2);
        CHECK(knn_visitors_fill_blocks(len.data(), 4, 1) == 1);
        CHECK(knn_visitors_fill_blocks(len.data(), 4, 2) == 2);
        CHECK(knn_visitors_fill_blocks(len.data(), 0, 16) == 3);
        CHECK(knn_visitors_fill_blocks(len.data(), 16, 2) == 8192);
        for (int64_t v0 = 0; v0 < (int64_t)len.size(); ++v0)
            for (int nt = 1; nt <= 16 && v0 + nt <= (int64_t)len.size(); ++nt) {
                int32_t m = 0;
                for (int t = 0; t < nt; ++t) m = std::max(m, len[(size_t)(v0 + t)]);
                const unsigned b = knn_visitors_fill_blocks(len.data(), v0, nt);
                CHECK(b >= 1 && (int64_t)b * 256 >= m && ((int64_t)b - 1) * 256 < std::max(1, m));
            }
    }
    // the stage: a staged vector lies where the input lies; two bounds a visitor; never an empty allocation's size 0 for
    // the element arrays (a family may hold no entry at all)
    {
        const KnnVisitorsStageSizes s = knn_visitors_stage_sizes(33, 1000, 0);
        CHECK(s.bounds == 66 && s.p_elems == 1000 && s.c_elems == 1 && s.norms == 33 && s.lens == 66);
        for (int64_t v : {0, 1, 32, 1 << 20}) CHECK(knn_visitors_stage_row(v) == 2 * v && knn_visitors_stage_row(v) + 1 < 2 * (v + 1) + 1);
        CHECK(knn_visitors_stage_row(kVisitorsMax) == 2147483646);   // the last stage row still is an int32
    }
    printf("%d cases pass\n", cases);
    return 0;
}
