// knn_visitors_side.h -- what a KNN handle needs to serve visitors (rating vectors that are no rows of the index) and has
// no member for: the handle's layout is part of the hash that ties the committed counter record to the kernels it
// measured, so it lives in a side record per handle - a registry keyed by the handle's address, under a mutex
// (knn_visitors.h, compiled with knn_large.hip).  Both builders attach the record as the last step of a successful
// build; locrec_knn_destroy (knn_batch.hip) drops it.
#pragma once

#include <memory>
#include <vector>

#include "knn_index.h"
#include "knn_visitors_plan.h"

namespace locrec {

struct KnnVisitorSide {
    // the popularity renumbering of the place dimensions (old index -> stored index), p null: the index stores the
    // caller's indices
    DevBuf<int32_t> new_of_old;
    bool renumbered() const { return new_of_old.p != nullptr; }
    // the stage (grow-only): the visitors' vectors as the scan's fill reads them, their lengths, their vector norms
    DevBuf<int64_t> bounds_p, bounds_c;
    DevBuf<int32_t> idx_p, idx_c, lens;
    DevBuf<double> val_p, val_c, norm_p, norm_c;
    DevBuf<unsigned long long> report;  // [2]: the first refusal, the entries beyond the dimensions
    // host arrays on their way in (grow-only)
    DevBuf<int64_t> in_ptr_p, in_ptr_c;
    DevBuf<int32_t> in_idx_p, in_idx_c;
    DevBuf<double> in_val_p, in_val_c;
    std::vector<int32_t> h_lens;        // host copy of lens: [2][nv]
    // the ranked form's call-local arrays (grow-only)
    DevBuf<int64_t> rk_in, rk_out;
};

// The record of a freshly built handle; replaces whatever is registered under the same address (a handle that was freed
// without locrec_knn_destroy can leave nothing behind: only a finished build attaches).  new_of_old: p_dim device words
// that become the record's (taken out of the DevBuf), or empty.
int32_t knn_visitors_attach(const locrec_knn_index *ix, DevBuf<int32_t> &new_of_old);
// the same from the host builder's map (empty: no renumbering)
int32_t knn_visitors_attach_host(const locrec_knn_index *ix, const std::vector<int32_t> &new_of_old);
// the handle's record, or null (a handle no builder of this library finished)
std::shared_ptr<KnnVisitorSide> knn_visitors_side(const locrec_knn_index *ix);
void knn_visitors_drop(const locrec_knn_index *ix);

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
