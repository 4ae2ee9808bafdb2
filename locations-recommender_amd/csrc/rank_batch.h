// rank_batch.h -- the segmented ranker's internal entry (rank_batch.hip): "places of the target region, top N by
// score" for many row ranges of one device-resident (ids, scores) pair at once.  locrec_rank_recommendations_batch
// and the ranked KNN batches call it; every pointer is a device pointer of the current device.
#pragma once

#include "common.h"

namespace locrec {

// what the last ranking of this thread did (locrec_rank_recommendations_batch_stats)
struct RankBatchStats {
    int64_t one_block = 0;        // segments one block served from its LDS list
    int64_t split = 0;            // segments cut into chunks and merged
    int64_t chunks = 0;           // chunks of the split segments
    int64_t sorted = 0;           // segments the global radix sort served
    int64_t membership_form = 0;  // 0: binary search in the (region, place id) table (the only form)
    int64_t host_assembled = 0;   // segments whose rows the host assembled and uploaded
    int64_t host_syncs = 0;       // explicit stream synchronisations of the call (the hipFree of a work buffer waits too)
};
RankBatchStats &rank_batch_stats();

// Segment s is rows [seg_begin[s], seg_begin[s] + seg_len[s]) of ids / scores (0 <= seg_len[s] < 2^31; checked on the
// device before any row is read, with *invalid_flag - when given - as one more reason to refuse: LOCREC_E_INVALID_ARG
// and nothing written).  Row s of out_ids / out_scores (stride max_recommendations > 0) gets the segment's ranking,
// padded with id -1 and score 0.0; out_counts[s] the rows written.  The call waits for the stream twice at the most
// (host_syncs) and frees its call-local work buffers at the end, each hipFree a wait of its own.
int32_t rank_segments_device(int64_t n_segments, const int64_t *seg_begin, const int64_t *seg_len, const int64_t *ids,
                             const double *scores, int64_t n_places, const int64_t *place_ids,
                             const int64_t *place_region_ids, const int64_t *target_region_ids, int64_t max_recommendations,
                             int64_t *out_ids, double *out_scores, int64_t *out_counts,
                             const unsigned long long *invalid_flag, int64_t host_assembled, hipStream_t s);

}  // namespace locrec
