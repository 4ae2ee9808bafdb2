// knn_pool_visitors_api.h -- one mixed batch of visitors over a pool of indexes (knn_pool_visitors.h, compiled with
// knn_large.hip) as the entry points of knn_batch.hip (locrec_knn_pool_visitors_*, knn_pool_visitors_entry.h) see it.
#pragma once

#include <vector>

#include "knn_index.h"
#include "knn_pool_api.h"
#include "knn_pool_visitors_plan.h"
#include "knn_visitors_side.h"

namespace locrec {

// what the last pool-visitors call of this thread did (locrec_knn_pool_visitors_stats, in this order)
struct KnnPoolVisitorsStats {
    int64_t waves = 0;              // tile waves of the shared path
    int64_t member_tiles = 0;       // tiles of kLkbQt visitors over all members and waves
    int64_t stage_launches = 0;     // lkv_stage_pool
    int64_t fill_launches = 0;      // lkb_fill_pool (set and wipe, both families)
    int64_t scan_launches = 0;      // lkv_scan_pool
    int64_t aggregate_launches = 0; // lk_aggregate_segments_pool
    int64_t finish_launches = 0;    // lk_sum_segments_pool + lk_finish_count_pool + lk_finish_emit_pool
    int64_t delegated_members = 0;  // members served by their own visitors call
    int64_t beyond = 0;             // entries beyond the members' dimensions (vector norm only)
    int64_t emitted_rows = 0;       // rows lk_finish_emit_pool wrote
    int64_t readback_bytes = 0;     // every byte that reached host memory through the pool
    int64_t host_syncs = 0;         // waits for the pool's stream
};
KnnPoolVisitorsStats &knn_pool_visitors_stats();

// The pool-owned buffers of the visitors' stage (the staged vectors of ALL members, their lengths and norms, host arrays
// on their way in) and of the gather for delegated members.
struct KnnPoolVisitors;
KnnPoolVisitors *knn_pool_visitors_create();
void knn_pool_visitors_destroy(KnnPoolVisitors *pv);

// a member during one call: an asked one's visitor state (its new_of_old) is read by the stage, nobody touches the others'
struct KnnPoolVisitorsMember {
    locrec_knn_index *ix;
    bool asked;
};

// Checks and stages every visitor of every member in ONE launch (lkv_stage_pool) on the pool's stream: visitor i is
// checked against, and renumbered for, member index_of[i].  On a refusal *bad = the first offending position in call
// order and nothing else is done.
int32_t knn_pool_visitors_stage(KnnPoolVisitors *pv, int device, hipStream_t s, const std::vector<KnnPoolVisitorsMember> &members,
                                const int32_t *index_of, const KnnVisitorVectors &v, int64_t *bad);

// a sharing member's cut: its visitors (positions of the call, in call order)
struct KnnPoolVisitorsBatch {
    locrec_knn_index *ix;
    const int64_t *visitors;
    int64_t n;
};

// makeRecommendations for the staged visitors of every batch, all members' tiles side by side.  On return the rows of
// visitor i lie at [row_base[i], row_base[i] + row_len[i]) of *out_place / *out_est (device, owned by ws), ordered by place
// id; the stream s is idle.  Every member is left with nothing resident.
int32_t knn_pool_visitors_run(KnnPoolShared *ws, KnnPoolVisitors *pv, hipStream_t s, const std::vector<KnnPoolVisitorsBatch> &batches,
                              double pw, double cw, int64_t *row_base, int64_t *row_len, const int64_t **out_place,
                              const double **out_est);

// The vectors of the listed visitors (positions of the call, ascending) as a CSR of their own, in v.mem: host arrays are
// gathered on the host, device arrays device to device (one copy per visitor and array: the delegated regime is not the
// one the pool exists for).  The result lives in pv until the next gather; the stream s is idle on return.
int32_t knn_pool_visitors_gather(KnnPoolVisitors *pv, hipStream_t s, const KnnVisitorVectors &v, const int64_t *visitors, int64_t n,
                                 KnnVisitorVectors *out);

}  // namespace locrec
