// knn_pool_api.h -- the shared-launch path of a pool of indexes (knn_pool.h, compiled with knn_large.hip) as the entry
// points of knn_batch.hip (locrec_knn_pool_*) see it.
#pragma once

#include <vector>

#include "knn_index.h"
#include "knn_pool_plan.h"

namespace locrec {

// what the last pool call of this thread did (locrec_knn_pool_stats)
struct KnnPoolStats {
    int64_t waves = 0;             // tile waves of the shared path
    int64_t member_tiles = 0;      // tiles of kLkbQt queries over all members and waves
    int64_t fill_launches = 0;     // lkb_fill_pool (set and wipe, both families)
    int64_t scan_launches = 0;     // lkb_scan_pool
    int64_t aggregate_launches = 0;  // lk_aggregate_segments_pool (one per wave; sum, count and emit go with it)
    int64_t finish_launches = 0;   // lk_sum_segments_pool + lk_finish_count_pool + lk_finish_emit_pool
    int64_t delegated_members = 0; // members served by their own public call
    int64_t emitted_rows = 0;      // rows lk_finish_emit_pool wrote
    int64_t readback_bytes = 0;    // every byte that reached host memory
    int64_t host_syncs = 0;        // waits for the pool's stream
};
KnnPoolStats &knn_pool_stats();

// The pool-owned buffers of the shared path: launch tables, candidate counters, the wave's tile counts, the result rows.
struct KnnPoolShared;
KnnPoolShared *knn_pool_shared_create();
void knn_pool_shared_destroy(KnnPoolShared *ws);

// the distinct requests of one member in the "every positive neighbour" regime (k > LOCREC_KNN_BATCH_MAX_K and
// k >= n - 1): rows[0 .. n) are internal rows of valid queries; request j of the member is request first + j of the call
struct KnnPoolBatch {
    locrec_knn_index *ix;
    const int32_t *rows;
    int64_t n;
    int64_t first;
};

// makeRecommendations for every request of every batch, all members' tiles side by side (knn_pool.h).  On return the
// rows of request u lie at [row_base[u], row_base[u] + row_len[u]) of *out_place / *out_est (device, owned by ws), ordered
// by place id; the stream s is idle.  Every member is left with nothing resident.
int32_t knn_pool_shared_run(KnnPoolShared *ws, hipStream_t s, const std::vector<KnnPoolBatch> &batches, double pw, double cw,
                            int64_t *row_base, int64_t *row_len, const int64_t **out_place, const double **out_est);

}  // namespace locrec
