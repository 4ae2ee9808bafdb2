// knn_topk_plan.h -- the host arithmetic of the batched top-K (enqueue_topk, knn_topk_host.h): how a tiled scan cuts its
// candidate slices into chunks and how many levels merge the chunks' lists; whether a batch is admitted to the head / tail
// form's hit pre-pass; the LDS image of knn_side_topk.
// Plain C++ without a device call: tests/host/knn_topk_plan_check.cpp runs it stand-alone, under a host sanitizer too.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace locrec {

constexpr int kTopkMergeCap = 8192;          // entries one merge block sorts in LDS (12 bytes each)
constexpr int kTopkBlocksRowScan = 2048;     // blocks a tiled row scan aims at: 4 rounds of 512 resident blocks
constexpr int kTopkBlocksHeadTail = 1024;    // ... and the head / tail scan: one chunk per tile at the bench batch
constexpr size_t kTopkLdsMax = 160 * 1024;   // LDS of a workgroup
constexpr int kTopkHtMaxEntries = 1024;      // kHtMaxEntries of knn_ht_prepass.h (asserted in knn_topk_host.h)

inline int knn_topk_pow2ceil(int v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// ---- chunks of a tiled scan, and the merge of their lists ----
// The grid is (nchunks, ntiles): a block scans slices_per_chunk candidate slices for one tile of qt queries and leaves one
// K-list per query.  knn_merge sorts M entries in LDS: up to max_chunks lists.  More chunks than that (a single request
// that has to fill the chip by itself) are merged in two levels: knn_merge_partial turns each group of max_chunks lists
// into one (M1 entries), knn_merge the ngroups results.
struct KnnTopkChunks {
    int ntiles;            // tiles of qt queries
    int max_chunks;        // lists one merge block holds
    int nchunks;           // chunks of the slice range: every slice in exactly one, none empty
    int slices_per_chunk;  // a multiple of the block's waves
    int ngroups;           // 0: one merge level
    int M1, M;             // pow2 entries of the first (0 without groups) and the final merge
    size_t lds_partial, lds_merge;  // their dynamic LDS
};

// range_slices >= 1 candidate slices, nq >= 1 queries in tiles of qt, `waves` waves a block, 1 <= K <= 1024;
// env_blocks > 0 (LOCREC_KNN_BLOCKS) replaces the block target
inline KnnTopkChunks knn_topk_chunks(int range_slices, int64_t nq, int qt, int waves, int K, bool use_ht, int env_blocks)
{
    KnnTopkChunks c{};
    c.ntiles = (int)((nq + qt - 1) / qt);
    // enough blocks to fill the chip; when that needs more chunks than one merge block can sort (a single request), the
    // merge runs in two levels
    c.max_chunks = std::max(1, kTopkMergeCap / K);
    // target number of blocks.  The row scan was tuned at 2048.  The head / tail scan does better with ONE chunk per tile
    // at the bench batch (1024 blocks = exactly two rounds): a chunk more per tile means another K*ln(N/K) list insertions
    // and another list to merge (cfg2: 23.2 -> 19.0 ms per 16,384-query batch).
    int want = std::max(1, ((use_ht ? kTopkBlocksHeadTail : kTopkBlocksRowScan) + c.ntiles - 1) / c.ntiles);
    if (env_blocks > 0) want = std::max(1, (env_blocks + c.ntiles - 1) / c.ntiles);  // tuning
    int nchunks = std::min(std::min(want, c.max_chunks * c.max_chunks), std::max(1, range_slices / 8));
    int spc = (range_slices + nchunks - 1) / nchunks;
    spc = std::max(waves, (spc + waves - 1) / waves * waves);
    c.slices_per_chunk = spc;
    c.nchunks = std::max(1, (range_slices + spc - 1) / spc);
    c.ngroups = c.nchunks > c.max_chunks ? (c.nchunks + c.max_chunks - 1) / c.max_chunks : 0;
    c.M1 = c.ngroups ? knn_topk_pow2ceil(std::max(2, c.max_chunks * K)) : 0;
    c.lds_partial = (size_t)c.M1 * 12;
    c.M = knn_topk_pow2ceil(std::max(2, (c.ngroups ? c.ngroups : c.nchunks) * K));
    c.lds_merge = (size_t)c.M * 12;
    return c;
}

// ---- admission of a batch to the head / tail form (knn_ht.h) ----
// The hit pre-pass holds a tile's (query, tail place) pairs in LDS and addresses its hits with 32 bits: every tile of qt
// rows must have at most max_entries tail entries (kHtMaxEntries) and fewer than 2^32 hits.  rows: the batch's rows, or
// null for the rows row0 .. row0 + nq - 1; tail_nnz[r]: tail entries of row r; tail_hits_ps: prefix sums of the rows' hits.
// *total_hits: the hits of all tiles (what the pre-pass's buffer is sized from), complete when the batch is admitted.
inline bool knn_topk_admit_head_tail(const int32_t *rows, int32_t row0, int64_t nq, int qt, const int32_t *tail_nnz,
                                     const int64_t *tail_hits_ps, int64_t max_entries, int64_t *total_hits)
{
    bool ok = true;
    *total_hits = 0;
    for (int64_t t0 = 0; ok && t0 < nq; t0 += qt) {
        int64_t ent = 0, hits = 0;
        for (int64_t i = t0; i < std::min(nq, t0 + qt); ++i) {
            const int32_t r = rows ? rows[i] : row0 + (int32_t)i;
            ent += tail_nnz[r];
            hits += tail_hits_ps[(size_t)r + 1] - tail_hits_ps[(size_t)r];
        }
        ok = ent <= max_entries && hits < ((int64_t)1 << 32);
        *total_hits += hits;
    }
    return ok;
}

// ---- LDS of knn_side_topk (knn_side.h): the index's wide rows merged into every K-list ----
// The merged list (cap entries of 12 bytes), the query's category table (c_dim doubles) and its place hash (hash_cap slots
// of 12 bytes: 2 x the longest query of the batch, at most 8192 slots; a longer query merges rows instead).
// (The sum is known to overshoot what the kernel touches - ADVICE.md - and a large enough index of wide rows could be
// refused a launch it would fit: the formula is kept as it was, trimming it is a change of behaviour of its own.)
struct KnnSideTopkLds {
    int cap, hash_cap;
    size_t slds;
};
inline KnnSideTopkLds knn_side_topk_lds(int K, int nwide, int max_nnz_p, int c_dim)
{
    KnnSideTopkLds l{2, 64, 0};
    while (l.cap < K + nwide) l.cap <<= 1;
    while (l.hash_cap < 2 * max_nnz_p && l.hash_cap < 8192) l.hash_cap <<= 1;
    l.slds = (size_t)l.cap * 12 + (size_t)c_dim * 8 + (size_t)l.hash_cap * 12;
    return l;
}

}  // namespace locrec
