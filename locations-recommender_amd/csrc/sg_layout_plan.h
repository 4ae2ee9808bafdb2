// sg_layout_plan.h -- the one statement of every rule of the stochastic graph's layout: the constants, the three per-row
// rules, the piece plan in closed form from a scan's totals, the smaller decisions and the byte figures.
// Both builders take them from here - the host build (sg_host_layout.h) and the device build (sg_create_device.hip,
// whose kernels share the per-row rules) - and sg.hip's kSlots, kLongRow and kDictMax are these constants.  Plain C++,
// nothing from HIP and no device call: tests/host/sg_layout_plan_check.cpp compiles it alone and compares it with a
// row-by-row walk of the layout, under a host sanitizer.
#pragma once

#include <cstdint>

#if defined(__HIP__)  // (the compiler's own macro: the HIP runtime header is the includer's business)
#define LOCREC_SG_PLAN_FN __host__ __device__ __forceinline__
#else
#define LOCREC_SG_PLAN_FN inline
#endif

namespace locrec {

constexpr int kSgPlanSlots = 256;     // sg.hip's kSlots: edge slots per piece (64 lanes x 4)
constexpr int kSgPlanLongRow = 8;     // kLongRow: rows with more full pieces are summed by a whole wave
constexpr int kSgPlanDictMax = 8192;  // kDictMax: distinct weights the dictionary form takes (64 KB of LDS)
constexpr int kSgPlanClasses = 7;     // remainder classes 0 .. 6: a segment of 4 << c slots, 64 >> c segments per piece

// ---- per row: what the kernels ask too ------------------------------------------------------------------------------

// the remainder class: ceil_log2((rem + 3) / 4), the smallest c whose segment of 4 << c slots holds rem in 1 .. 256
LOCREC_SG_PLAN_FN int sg_remainder_class(int rem)
{
    const int v = (rem + 3) / 4;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// a row with more than two full pieces lives in the long area (behind the three partial slots of every row)
LOCREC_SG_PLAN_FN bool sg_in_long_area(int degree) { return degree / kSgPlanSlots > 2; }

// ... and one with more than kLongRow of them is summed by a whole wave (the front part of lrows)
LOCREC_SG_PLAN_FN bool sg_wave_row(int nfull) { return nfull > kSgPlanLongRow; }

// first partial slot of row l >= n_short, which has full_begin full pieces in front of it (SgLayoutPlan::long_base)
LOCREC_SG_PLAN_FN int32_t sg_long_begin(int32_t long_base, int32_t full_begin, int32_t l) { return long_base + full_begin + l; }

// ---- the plan from the scan's totals --------------------------------------------------------------------------------

enum class SgPlanStatus {
    ok,
    too_many_slots,     // "graph too large for int32 slot ids"
    too_many_partials,  // "graph too large for int32 partial slots"
};

struct SgLayoutPlan {
    SgPlanStatus status = SgPlanStatus::ok;
    // 64-bit whatever the status: the pieces, the segments ("parts") and the partial slots of one PA half
    int64_t np = 0, npart = 0, pa = 0;
    // filled when status == ok: the full pieces come first in row order, then the remainder pieces by class 6 down to 0
    int32_t piece_begin[kSgPlanClasses] = {}, part_begin[kSgPlanClasses] = {};
    int32_t nfull_total = 0, T = 0, n_short = 0;
    int32_t long_base = 0;  // sg_long_begin
    int64_t nslots() const { return np * kSgPlanSlots; }
    int32_t long_area_rows() const { return T - n_short; }
};

// rows_of_class[c]: live rows with a remainder of class c; nfull_total: full pieces of all rows; full_before_short: those
// of the rows in front of row n_short (the short ones); T live rows, the first n_short of them outside the long area.
inline SgLayoutPlan sg_layout_plan(const int32_t rows_of_class[kSgPlanClasses], int32_t nfull_total, int32_t full_before_short,
                                   int32_t T, int32_t n_short)
{
    SgLayoutPlan pl;
    int64_t piece_begin[kSgPlanClasses], part_begin[kSgPlanClasses];
    pl.np = pl.npart = nfull_total;
    for (int c = kSgPlanClasses - 1; c >= 0; --c) {
        const int segs_per_piece = 64 >> c;
        const int64_t pieces = ((int64_t)rows_of_class[c] + segs_per_piece - 1) / segs_per_piece;
        piece_begin[c] = pl.np;
        part_begin[c] = pl.npart;
        pl.np += pieces;
        pl.npart += pieces * segs_per_piece;
    }
    // the long area: a run of nfull + 1 slots per row from n_short on, in row order.  Row l's run starts at
    // 3T + (full pieces of the long rows before it) + (l - n_short), which is long_base + full_begin[l] + l with the
    // base below, and the area ends at pa.  (On a shard n_short follows the degrees over all edges and the pieces the
    // shard's own: a row of the long area may have no full piece there.)
    pl.pa = 3 * (int64_t)T + ((int64_t)nfull_total - full_before_short) + ((int64_t)T - n_short);
    if (pl.np >= ((int64_t)1 << 31) / kSgPlanSlots) {
        pl.status = SgPlanStatus::too_many_slots;
        return pl;
    }
    if (pl.pa >= ((int64_t)1 << 30)) {
        pl.status = SgPlanStatus::too_many_partials;
        return pl;
    }
    for (int c = 0; c < kSgPlanClasses; ++c) {
        pl.piece_begin[c] = (int32_t)piece_begin[c];
        pl.part_begin[c] = (int32_t)part_begin[c];
    }
    pl.nfull_total = nfull_total;
    pl.T = T;
    pl.n_short = n_short;
    pl.long_base = (int32_t)(3 * (int64_t)T - full_before_short - n_short);
    return pl;
}

// ---- the smaller decisions ------------------------------------------------------------------------------------------

// vertex ranking through a table over [min, max] instead of a sort: ids that sit close together (id_span = max - min)
inline bool sg_dense_ids(uint64_t id_span, int64_t ne) { return id_span < (uint64_t)(8 * ne) + (1u << 20); }

// 16-bit columns: every live index and the two extra entries of x fit
inline bool sg_use16(int32_t T) { return (int64_t)T + 2 <= 65536; }

// the dictionary form: at least one and at most kDictMax distinct weights
inline bool sg_dict_fits(int32_t distinct) { return distinct >= 1 && distinct <= kSgPlanDictMax; }

// radix bits that hold every key below n
inline int sg_radix_bits(int64_t n)
{
    int b = 1;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}

inline int64_t sg_layout_bytes(int64_t np, int32_t T) { return np * kSgPlanSlots * 12 + np * 8 + (int64_t)T * 12; }

// what one sweep + finalize really moves in this layout (padding included): columns and weights (or their dictionary index) of
// every slot, piece descriptors, one partial written and read back per segment, x read and x' written once per live row
inline int64_t sg_device_sweep_bytes(int64_t np, int64_t npart, int32_t T, bool use16, bool dictionary)
{
    return np * kSgPlanSlots * (int64_t)((use16 ? 2 : 4) + (dictionary ? 2 : 8)) + np * 8 + npart * 16 + (int64_t)T * 16;
}

// pieces per wave of the persistent form with ncu compute units of 8 waves: 4 or 12, 0 where neither holds the graph
inline int sg_persist_pw(int64_t np, int ncu)
{
    const int64_t waves = (int64_t)ncu * 8;
    const int64_t need = waves > 0 ? (np + waves - 1) / waves : 1 << 30;
    return need <= 4 ? 4 : need <= 12 ? 12 : 0;
}

}  // namespace locrec
