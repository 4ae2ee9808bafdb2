// knn_visitors_plan.h -- what the host decides for a batch of visitors (locrec_knn_visitors_*: rating vectors that are
// no rows of the index; knn_visitors.h, knn_visitors_api.h): the regime, the effective K, the chunks of the neighbour
// lists, the fill grid, the stage's buffers.  Plain C++ without a device call: tests/host/knn_visitors_plan_check.cpp
// runs it stand-alone, under a host sanitizer too.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "knn_pool_plan.h"

namespace locrec {

// A visitor is a candidate of nobody and nobody is left out as "self": all n persons are candidates, so "every
// positive-similarity person is a neighbour" begins at K >= n (a person's own request: n - 1) ...
inline bool knn_visitors_all(int64_t k, int64_t n) { return k >= n; }
// ... and a list holds at most min(K, n) entries (at least 1: the selection kernels divide their work by it)
inline int64_t knn_visitors_keff(int64_t k, int64_t n) { return std::min<int64_t>(k, std::max<int64_t>(1, n)); }

// bytes of one entry of the device result arrays of a neighbour-list call: id, similarity, row
constexpr int64_t kVisitorsEntryBytes = 20;
constexpr int64_t kVisitorsChunkBytes = (int64_t)2 << 30;

// visitors per chunk of a neighbour-list call: nv x K entries stay within the budget (2 GiB); whole tiles where a chunk
// holds one; one visitor at least
inline int64_t knn_visitors_chunk(int64_t k, int64_t budget = kVisitorsChunkBytes)
{
    const int64_t c = std::max<int64_t>(1, budget / (std::max<int64_t>(1, k) * kVisitorsEntryBytes));
    return c >= kLkbQt ? c / kLkbQt * kLkbQt : c;
}
// the budget from the text of LOCREC_KNN_VISITORS_CHUNK_BYTES (tests: chunks of a few visitors without gigabytes of
// results): null, empty or no number: the default; clamped to [1, 2 GiB].  The result does not depend on it.
inline int64_t knn_visitors_chunk_budget(const char *text)
{
    if (!text || !*text) return kVisitorsChunkBytes;
    char *end = nullptr;
    const long long b = std::strtoll(text, &end, 10);
    if (end == text) return kVisitorsChunkBytes;
    return std::min<int64_t>(kVisitorsChunkBytes, std::max<int64_t>(1, (int64_t)b));
}

// the most rows (16 bytes each) a recommendation call may leave resident: one per visitor and place; refused beyond 48 GB
inline int64_t knn_visitors_worst_row_bytes(int64_t nv, int64_t n_places) { return nv * std::max<int64_t>(1, n_places) * 16; }
constexpr int64_t kVisitorsMaxRowBytes = (int64_t)48 << 30;

// element blocks (of 256 threads) of the fill and wipe launches of a tile: the longest staged vector among its visitors
inline unsigned knn_visitors_fill_blocks(const int32_t *staged_len, int64_t v0, int nt)
{
    int32_t longest = 1;
    for (int t = 0; t < nt; ++t) longest = std::max(longest, staged_len[v0 + t]);
    return (unsigned)((longest + 255) / 256);
}

// The stage's buffers for nv visitors holding pe place and ce category entries.  A staged vector lies where its input
// lies (the entries beyond the dimensions are squeezed out inside the row), so the element arrays have the input's size;
// row v of a family is [bounds[2v], bounds[2v + 1]): two words a visitor, so that bounds + 2v serves as the `ptr` of a row.
struct KnnVisitorsStageSizes {
    size_t bounds;    // int64 per family
    size_t p_elems, c_elems;
    size_t norms;     // fp64 per family
    size_t lens;      // int32, both families: [2][nv]
};
inline KnnVisitorsStageSizes knn_visitors_stage_sizes(int64_t nv, int64_t pe, int64_t ce)
{
    return {2 * (size_t)nv, (size_t)std::max<int64_t>(1, pe), (size_t)std::max<int64_t>(1, ce), (size_t)nv, 2 * (size_t)nv};
}
// the visitor's number in the stage as lkb_fill's qrow: its row of `bounds`
inline int32_t knn_visitors_stage_row(int64_t v) { return (int32_t)(2 * v); }
// visitors one call may stage: the stage rows are int32
constexpr int64_t kVisitorsMax = ((int64_t)1 << 30) - 1;

}  // namespace locrec
