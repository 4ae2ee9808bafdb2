// knn_format_plan.h -- the ONE decision that selects a KNN index's format and kernel path (DESIGN.md "Numeric limits"),
// taken by both builders (knn_build.hip, knn_host_build.h) from what their validation found.  Plain C++, nothing from
// HIP: tests/host/knn_format_plan_check.cpp compiles it alone; knn_index.h's cfg:: constants come in as KnnFormatLimits.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace locrec {

inline int ceil_log2_64(int64_t v) { int l = 0; while (((int64_t)1 << l) < v) ++l; return l; }

// largest |value| and largest sum of squares of a row, per family, over some set of rows
struct KnnMaxima {
    double pvmax = 0, cvmax = 0, pss = 0, css = 0;
};

struct KnnFormatLimits {  // cfg::kHtHead, kHtQt, kHtCatRows, kPopTable, kDirectMaxBytes
    int ht_head, ht_qt, ht_cat_rows, pop_table, direct_max_bytes;
};

struct KnnFormatSwitches {  // the handle's (knn_read_env)
    bool force_generic = false, no_row_fallback = false, no_pack16 = false, no_ht = false, no_pop = false, force_hash = false;
    int32_t env_ht_h = 0, env_pop_h = 0;
};

struct KnnFormatInput {
    int64_t n = 0;
    int32_t p_dim = 0, c_dim = 0;
    bool integral = true;  // every value is an integer count >= 1
    KnnMaxima all;         // over all rows
    KnnMaxima narrow;      // over the rows that are not wide (kb_validate)
    KnnFormatSwitches sw;
    KnnFormatLimits lim{};
};

struct KnnFormatPlan {
    int64_t n_wide = 0;  // wide rows kept out of the packed images (0: no fallback)
    int p_vbits = 0, c_vbits = 0;
    bool packed = false, pack16 = false, want_ht = false, use_pop = false;
    int32_t ht_h = 0;   // head width of the head / tail form
    int32_t pop_h = 0;  // size of the popular-prefix table (0 without the renumbering)
    int32_t key_h = 0;  // third row-order key: a row's count of renumbered indices below this
};

// Per-row format fallback.  Counts are unbounded in the reference's data (RatingVectorsBuilder.scala:69): ONE person with
// 256 visits to a place, or one row with a sum of squares of 65,536, would demote the WHOLE index from the head / tail
// form to PACK32 (3.6 x slower per pair).  When such "wide" rows are few they stay out of the packed images, the rest is
// judged on its own maxima, and knn.hip adds them back through the side kernels and the dense CSR scan.  Integer data
// only: a non-integer value selects GENERIC for everybody.  Asked first: only then does a build count its wide rows.
inline bool knn_row_fallback_eligible(const KnnFormatInput &in)
{
    const KnnMaxima &m = in.all;
    const bool any_wide = m.pvmax >= 256.0 || m.cvmax >= 256.0 || m.pss >= 65536.0 || m.css >= 65536.0;
    return any_wide && in.integral && !in.sw.force_generic && !in.sw.no_row_fallback && !in.sw.no_pack16 && !in.sw.no_ht &&
           in.n < ((int64_t)1 << 24) && in.c_dim <= in.lim.ht_cat_rows &&
           in.p_dim < (1 << 20) - 1;  // (a place dimension no packed format holds: GENERIC keeps every row in its image)
}

// wide_count: the number of wide rows where the fallback is eligible (not looked at otherwise)
inline KnnFormatPlan knn_format_plan(const KnnFormatInput &in, int64_t wide_count)
{
    KnnFormatPlan pl;
    // at most max(256, n / 512) wide rows, capped at 4096 (the side kernels score every (query, wide row) pair by
    // merging two CSR rows), and not every row
    const int64_t cap = std::min<int64_t>(4096, std::max<int64_t>(256, in.n / 512));
    if (knn_row_fallback_eligible(in) && wide_count > 0 && wide_count <= cap && wide_count < in.n) pl.n_wide = wide_count;
    const KnnMaxima &m = pl.n_wide > 0 ? in.narrow : in.all;  // with the fallback the narrow rows decide the rest
    pl.p_vbits = std::min(24, 32 - ceil_log2_64(in.p_dim));
    pl.c_vbits = std::min(24, 32 - ceil_log2_64(in.c_dim));
    // exact u32 dots need every dot < 2^32; |dot| <= sqrt(ss_a * ss_b) <= max ss
    pl.packed = !in.sw.force_generic && in.integral && in.p_dim < (1 << 20) - 1 && in.c_dim < (1 << 20) - 1 &&
                m.pvmax < (double)(1u << pl.p_vbits) && m.cvmax < (double)(1u << pl.c_vbits) && m.pss < 4294967296.0 &&
                m.css < 4294967296.0;
    pl.pack16 = pl.packed && m.pss < 65536.0 && m.css < 65536.0 && m.pvmax < 65536.0 && m.cvmax < 65536.0 && !in.sw.no_pack16;
    // head / tail form (knn_ht.h): PACK16 data whose values fit a byte and whose rows fit 24 bits
    pl.ht_h = std::min<int32_t>(in.p_dim, in.lim.ht_head);
    if (in.sw.env_ht_h > 0) pl.ht_h = std::min<int32_t>(in.p_dim, in.sw.env_ht_h);  // tuning
    pl.ht_h = std::min<int32_t>(pl.ht_h, 65536 / (2 * in.lim.ht_qt));  // the element's low half is the panel row's byte offset
    pl.want_ht = pl.pack16 && !in.sw.no_ht && !in.sw.force_generic && in.n > 0 && in.n < ((int64_t)1 << 24) && m.pvmax < 256.0 &&
                 m.cvmax < 256.0 && in.c_dim <= in.lim.ht_cat_rows;
    // popularity renumbering of the place dimensions (PACKED formats): for the hashed panel and the head / tail form
    pl.use_pop = pl.packed && !in.sw.no_pop && in.n > 0 &&
                 (in.sw.force_hash || (size_t)in.p_dim * 2 > (size_t)in.lim.direct_max_bytes || pl.want_ht);
    if (pl.use_pop) {
        pl.pop_h = std::min<int32_t>(in.p_dim, in.lim.pop_table);
        if (in.sw.env_pop_h > 0) pl.pop_h = std::min<int32_t>(in.p_dim, in.sw.env_pop_h);  // tuning
    }
    // of HEAD indices when the head / tail form is built, so that the head rows of a slice have (nearly) one length
    pl.key_h = pl.want_ht ? pl.ht_h : pl.pop_h;
    return pl;
}

}  // namespace locrec
