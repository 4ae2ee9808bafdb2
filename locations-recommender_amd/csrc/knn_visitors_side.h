// knn_visitors_side.h -- the visitors' path over a KNN handle (rating vectors that are no rows of the index): what
// knn_visitors.h (compiled with knn_large.hip) offers the entry points of knn_batch.hip's unit.  The state itself -
// KnnVisitorSide: the new_of_old renumbering and the stage buffers - is the handle's member `visitors` (knn_index.h);
// both builders leave new_of_old there as the last step of a successful build, and it is freed with the handle.
#pragma once

#include <vector>

#include "knn_index.h"
#include "knn_visitors_plan.h"

namespace locrec {

// what the last visitors call of this thread did (locrec_knn_visitors_stats)
struct KnnVisitorsStats {
    int64_t tiles = 0;           // tiles of kLkbQt visitors
    int64_t tiles_all = 0;       // ... served without a top-K (K >= n)
    int64_t tiles_topk = 0;      // ... through the tiled selection
    int64_t beyond = 0;          // entries beyond the index's dimensions (vector norm only)
    int64_t renumbered = 0;      // the index renumbers its place dimensions
    int64_t stage_launches = 0;  // lkv_stage
    int64_t scan_launches = 0;   // lkv_scan
    int64_t host_syncs = 0;      // waits for the stream
};
KnnVisitorsStats &knn_visitors_stats();

// the visitors' vectors of one call: six arrays in `mem`, nv + 1 row pointers a family
struct KnnVisitorVectors {
    int64_t nv;
    const int64_t *p_ptr;
    const int32_t *p_idx;
    const double *p_val;
    const int64_t *c_ptr;
    const int32_t *c_idx;
    const double *c_val;
    int32_t mem;
};

// Checks and stages the vectors (lkv_stage): on a refusal *bad = the first offending visitor (or -1) and nothing else is
// done.  Afterwards side holds the staged vectors of all nv visitors.
int32_t knn_visitors_stage(locrec_knn_index *ix, KnnVisitorSide &side, const KnnVisitorVectors &v, int64_t *bad);

// findSimilarPersons for the staged visitors [v0, v0 + nv): visitor v0 + i's list in slot i of the handle's device result
// arrays (out_ids / out_sims / out_rows: stride k, padded; out_cnt), as knn_topk_tiled leaves a batch
int32_t knn_visitors_topk(locrec_knn_index *ix, KnnVisitorSide &side, int64_t v0, int64_t nv, double pw, double cw, int64_t k);

// makeRecommendations for the staged visitors [0, nv): rows in ix->lkb_place / lkb_est, visitor i's at
// [lkb_off[i], lkb_off[i + 1]), ordered by place id (as knn_large_recommend_batch leaves them; have_lkb stays false)
int32_t knn_visitors_recommend(locrec_knn_index *ix, KnnVisitorSide &side, int64_t nv, double pw, double cw, int64_t k);

}  // namespace locrec
