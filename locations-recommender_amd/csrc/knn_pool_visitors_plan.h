// knn_pool_visitors_plan.h -- what the host decides for one mixed batch of visitors over a pool of indexes
// (locrec_knn_pool_visitors_*; knn_pool_visitors.h, knn_pool_visitors_entry.h): which members share the pool's launches,
// the members' cuts, waves and tiles, the fill grid of a wave, the refusal of a result that cannot be held, the stage's
// buffers, the first offender.  Plain C++ without a device call: tests/host/knn_pool_visitors_plan_check.cpp runs it
// stand-alone, under a host sanitizer too.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "knn_visitors_plan.h"

namespace locrec {

// the largest K of the per-query LDS lists (LOCREC_KNN_BATCH_MAX_K of include/locrec.h; knn_batch.hip asserts the equality)
constexpr int64_t kPoolVisitorsBatchMaxK = 1024;

// How a member of n persons is served at k_nearest = k:
//   Shared     its own visitors call would serve every tile without a top-K and at the shipped regime: the pool's launches
//   Empty      nobody to be similar to: its visitors have no rows, whatever K (what its own call returns without a launch)
//   Delegated  any other member: its own locrec_knn_visitors_* call on its own visitors
enum class KnnPoolVisitorsWay { Shared, Empty, Delegated };
inline KnnPoolVisitorsWay knn_pool_visitors_way(int64_t k, int64_t n)
{
    if (n <= 0) return KnnPoolVisitorsWay::Empty;
    return k > kPoolVisitorsBatchMaxK && knn_visitors_all(k, n) ? KnnPoolVisitorsWay::Shared : KnnPoolVisitorsWay::Delegated;
}

// One call sorted out.  A visitor carries no id: a vector given twice is two visitors.
struct KnnPoolVisitorsPlan {
    struct Cut {
        int32_t member;
        int64_t first, n;  // its visitors are order[first .. first + n): positions of the call, ascending
    };
    std::vector<int64_t> order;   // the visitors member after member, each member's in call order
    std::vector<Cut> shared;      // the asked sharing members, ascending (a member that joins no wave included)
    std::vector<Cut> delegated;   // the asked delegated members, ascending
    std::vector<Cut> empty;       // the asked members without persons, ascending
};

// visitor i asks member index_of[i] (every position checked before); way[m]: how member m is served
inline void knn_pool_visitors_plan(int64_t nv, const int32_t *index_of, const std::vector<KnnPoolVisitorsWay> &way,
                                   KnnPoolVisitorsPlan &out)
{
    out = KnnPoolVisitorsPlan();
    const size_t nm = way.size();
    std::vector<int64_t> count(nm + 1, 0);
    for (int64_t i = 0; i < nv; ++i) ++count[(size_t)index_of[i] + 1];
    for (size_t m = 0; m < nm; ++m) count[m + 1] += count[m];
    out.order.resize((size_t)nv);
    std::vector<int64_t> at(count.begin(), count.end() - 1);
    for (int64_t i = 0; i < nv; ++i) out.order[(size_t)at[(size_t)index_of[i]]++] = i;  // (a counting sort: stable)
    for (size_t m = 0; m < nm; ++m) {
        const int64_t n = count[m + 1] - count[m];
        if (n == 0) continue;
        const KnnPoolVisitorsPlan::Cut c{(int32_t)m, count[m], n};
        (way[m] == KnnPoolVisitorsWay::Shared ? out.shared : way[m] == KnnPoolVisitorsWay::Empty ? out.empty : out.delegated)
            .push_back(c);
    }
}

// waves of a set of live cuts: the w-th tile of kLkbQt visitors of each that has one (knn_waves_of / knn_wave_tile)
inline int64_t knn_pool_visitors_waves(const std::vector<KnnPoolVisitorsPlan::Cut> &live)
{
    int64_t w = 0;
    for (const auto &c : live) w = std::max(w, knn_waves_of(c.n));
    return w;
}

// element blocks (of 256 threads) of a wave's fill and wipe launches, as far as one tile asks: the longest staged vector,
// of either family, among its visitors (staged_len: [2][nv], as the stage leaves it; visitors: positions of the call)
inline unsigned knn_pool_visitors_fill_blocks(const int32_t *staged_len, int64_t nv, const int64_t *visitors, int nt)
{
    int32_t longest = 1;
    for (int t = 0; t < nt; ++t)
        longest = std::max(longest, std::max(staged_len[visitors[t]], staged_len[nv + visitors[t]]));
    return (unsigned)((longest + 255) / 256);
}

// the most rows (16 bytes each) the call may leave resident: a visitor's member's rated places each (one at least);
// refused beyond kVisitorsMaxRowBytes (any such total is returned as the limit + 1).  n_visitors[j] visitors ask a member
// of n_places[j] rated places.
inline int64_t knn_pool_visitors_worst_row_bytes(size_t members, const int64_t *n_visitors, const int64_t *n_places)
{
    int64_t worst = 0;
    for (size_t j = 0; j < members; ++j) {
        const int64_t n = n_visitors[j], p = std::max<int64_t>(1, n_places[j]);
        if (n <= 0) continue;
        // worst + n * p * 16 > the limit, without forming a product that may not fit 64 bits
        if (p > (kVisitorsMaxRowBytes - worst) / 16 / n) return kVisitorsMaxRowBytes + 1;
        worst += knn_visitors_worst_row_bytes(n, p);
    }
    return worst;
}

// The stage's buffers: knn_visitors_stage_sizes' (ONE staged CSR for all members: visitor v is row 2v whatever its
// member) and a member position per visitor.
struct KnnPoolVisitorsStageSizes {
    KnnVisitorsStageSizes one;
    size_t member_of;  // int32
    size_t members;    // rows of the per-member table
};
inline KnnPoolVisitorsStageSizes knn_pool_visitors_stage_sizes(int64_t nv, int64_t pe, int64_t ce, int64_t members)
{
    return {knn_visitors_stage_sizes(nv, pe, ce), (size_t)std::max<int64_t>(1, nv), (size_t)std::max<int64_t>(1, members)};
}

// The stage's report word: the MINIMUM over all refusals of visitor << 8 | family << 4 | code.  So the first offender is
// the smallest position in call order, whatever the members; within it the place family (0) comes before the categories
// (1), and a family has one code: the first its walk meets.
inline unsigned long long knn_visitors_report_word(int64_t visitor, int family, unsigned code)
{
    return ((unsigned long long)visitor << 8) | ((unsigned long long)family << 4) | code;
}
constexpr unsigned long long kVisitorsNoReport = ~0ull;
struct KnnVisitorsOffender {
    int64_t visitor;
    int family;
    unsigned code;
};
inline KnnVisitorsOffender knn_visitors_first_offender(unsigned long long word)
{
    return {(int64_t)(word >> 8), (int)((word >> 4) & 1), (unsigned)(word & 0xF)};
}

}  // namespace locrec
