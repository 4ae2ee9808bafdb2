// knn_pool_plan.h -- the host arithmetic of the large-K batch (knn_large.hip) and of a pool of indexes (knn_pool.h,
// knn_batch.hip): tiles and waves, where a tile's rows go, how the row buffer grows, which requests a pool call computes.
// Plain C++ without a device call: tests/host/knn_pool_plan_check.cpp runs it stand-alone, under a host sanitizer too.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <tuple>
#include <vector>

namespace locrec {

constexpr int kLkbQt = 16;  // queries per tile of the batched large-K scan and aggregation

// A batch of n queries is cut into tiles of kLkbQt; wave w of a set of batches is the w-th tile of each that has one.
inline int64_t knn_waves_of(int64_t n) { return (n + kLkbQt - 1) / kLkbQt; }
// the queries of such a batch's tile in wave w; 0: it takes no part in the wave
inline int knn_wave_tile(int64_t n, int64_t w) { return (int)std::clamp<int64_t>(n - w * kLkbQt, 0, kLkbQt); }

// The rows of one tile behind `total`: cnt[slot][tiles] are the read-back counts per finish tile.  base[t] = where slot
// t's rows begin (-1 past the tile's nt queries: nothing is written), len[t] = its rows; returns the advanced total.
// (A slot with qrow < 0 has an all-zero column of S, so its counts are zero anyway: the test says what is meant.)
inline int64_t knn_tile_bases(const int32_t *cnt, int tiles, int nt, const int32_t *qrow, int64_t total, int64_t *base, int64_t *len)
{
    for (int t = 0; t < kLkbQt; ++t) {
        base[t] = t < nt ? total : -1;
        len[t] = 0;
        if (t < nt && qrow[t] >= 0)
            for (int i = 0; i < tiles; ++i) len[t] += cnt[(size_t)t * tiles + i];
        total += len[t];
    }
    return total;
}

// the grow-only row buffer's size once `total` rows no longer fit: half as much again
inline size_t knn_rows_room(int64_t total) { return (size_t)total + (size_t)total / 2 + 1024; }

// The requests of one pool call, sorted out: a member either shares the pool's launches or is delegated to its own call.
struct KnnPoolRequests {
    struct Cut {
        int32_t member;
        int64_t first, n;  // its distinct requests are rows[first .. first + n)
    };
    std::vector<int64_t> distinct_of;  // request -> its distinct request, or -1 (a delegated member's)
    std::vector<int32_t> rows;         // the distinct requests' rows, member after member; a repeated pair once
    std::vector<Cut> cuts;             // the sharing members that are asked, ascending
    std::vector<int32_t> delegated;    // the delegated members that are asked, ascending
    std::vector<std::vector<int64_t>> requests_of;  // per delegated member: its requests, in input order
};

// request i asks member index_of[i] for its row row[i]; shares[m]: member m takes the shared path
inline void knn_pool_requests(int64_t n, const int32_t *index_of, const int32_t *row, const std::vector<char> &shares,
                              KnnPoolRequests &out)
{
    out = KnnPoolRequests();
    std::vector<int64_t> ord((size_t)n);
    std::iota(ord.begin(), ord.end(), (int64_t)0);
    const auto key = [&](int64_t a) { return std::make_tuple(index_of[a], row[a], a); };
    std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return key(a) < key(b); });
    out.distinct_of.assign((size_t)n, -1);
    for (int64_t j = 0; j < n; ++j) {
        const int64_t i = ord[(size_t)j], before = j > 0 ? ord[(size_t)j - 1] : -1;
        const int32_t m = index_of[i];
        const bool new_member = before < 0 || index_of[before] != m;
        if (!shares[(size_t)m]) {
            if (new_member) {
                out.delegated.push_back(m);
                out.requests_of.emplace_back();
            }
            out.requests_of.back().push_back(i);
            continue;
        }
        if (new_member) out.cuts.push_back({m, (int64_t)out.rows.size(), 0});
        if (new_member || row[before] != row[i]) {
            out.rows.push_back(row[i]);
            ++out.cuts.back().n;
        }
        out.distinct_of[(size_t)i] = (int64_t)out.rows.size() - 1;
    }
    for (std::vector<int64_t> &r : out.requests_of) std::sort(r.begin(), r.end());
}

}  // namespace locrec
