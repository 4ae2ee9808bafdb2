// knn_anyk.h -- batched top-K at any K (knn_large.hip): the tiled selection behind the batch entry points of
// knn_batch.hip when K exceeds the per-query LDS lists (LOCREC_KNN_BATCH_MAX_K).
#pragma once

#include "knn_index.h"

namespace locrec {

// findSimilarPersons for the internal rows rows[0 .. nq), 16 per tile: query i's neighbours into slot i of the device
// result arrays (out_ids / out_sims / out_rows: stride k, padded with -1 / 0.0 / -1; out_cnt).  K_eff = min(k, n - 1)
// (H4).  A row without a place or category vector gets no neighbours, and count -1 when mark_absent is set.
int32_t knn_topk_tiled(locrec_knn_index *ix, const int32_t *rows, int64_t nq, double pw, double cw, int64_t k, bool mark_absent);

// makeRecommendations for the internal rows rows[0 .. nq) with K < the number of candidates: each query's top-K as
// above, then knn_large_recommend_batch's place-major aggregation.  Results stay on the device as that function leaves
// them (ix->lkb_place / lkb_est / lkb_off, have_lkb).
int32_t knn_topk_recommend_batch(locrec_knn_index *ix, const int32_t *rows, int64_t nq, double pw, double cw, int64_t k);

}  // namespace locrec
