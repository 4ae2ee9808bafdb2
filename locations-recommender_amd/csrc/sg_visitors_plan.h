// sg_visitors_plan.h -- what the host decides for a batch of SG visitors (locrec_sg_visitors_*: persons the graph has no
// vertex for, given by their out-edges; sg_visitors.h): the tiles, a tile's edges sorted by live row, the slot of every
// edge in the tile's weight table, the tables' sizes, a visitor's repeated target.  Plain C++ without a device call:
// tests/host/sg_visitors_plan_check.cpp runs it stand-alone, under a host sanitizer too.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace locrec {

constexpr int kSgVisitorsTile = 16;  // visitors of a tile, one column each (kBatchB of sg_batch.hip)
// staged edges one call may hold: the stage's positions are int32
constexpr int64_t kSgVisitorsMaxEdges = ((int64_t)1 << 31) - 1;

inline int64_t sg_visitors_tiles(int64_t nv) { return (nv + kSgVisitorsTile - 1) / kSgVisitorsTile; }

// position of the first edge of rows[0 .. n) whose row occurred before it in the same list (-1: none)
inline int64_t sg_visitors_first_repeat(const int32_t *rows, int64_t n)
{
    std::vector<int64_t> at((size_t)n);
    std::iota(at.begin(), at.end(), (int64_t)0);
    std::sort(at.begin(), at.end(), [&](int64_t a, int64_t b) { return rows[a] != rows[b] ? rows[a] < rows[b] : a < b; });
    int64_t first = -1;
    for (int64_t i = 1; i < n; ++i)
        if (rows[at[(size_t)i]] == rows[at[(size_t)i - 1]] && (first < 0 || at[(size_t)i] < first)) first = at[(size_t)i];
    return first;
}

// The call's staged edges, tile by tile; inside a tile ascending by live row, then by column.  Edge i of the stage says:
// column col[i]'s visitor points at live row row[i] with weight w[i], and row[i]'s line of the tile's weight table is
// slot[i] (the distinct rows of a tile numbered in ascending order).
struct SgVisitorsStage {
    std::vector<int64_t> tile_ptr;  // [tiles + 1] into the arrays below
    std::vector<int32_t> row, col, slot;
    std::vector<double> w;
    std::vector<int32_t> tile_slots;  // lines of every tile's weight table
    int32_t max_slots = 0;            // ... of the largest

    int64_t tiles() const { return (int64_t)tile_slots.size(); }
    int64_t edges() const { return (int64_t)row.size(); }
    // the tables' sizes: one int32 a live row; the weight lines of the largest tile, kSgVisitorsTile fp64 each (never 0)
    static size_t slot_table(int32_t T) { return (size_t)std::max<int32_t>(1, T); }
    size_t weight_table() const { return (size_t)std::max<int32_t>(1, max_slots) * kSgVisitorsTile; }
};

// nv visitors; visitor v's edges are positions offsets[v] .. offsets[v + 1] of live_row / weight (live_row: the target's
// live index, already checked: inside [0, T), no row twice in a visitor)
inline void sg_visitors_stage(int64_t nv, const int64_t *offsets, const int32_t *live_row, const double *weight, SgVisitorsStage &st)
{
    const int64_t nt = sg_visitors_tiles(nv), ne = nv > 0 ? offsets[nv] : 0;
    st.tile_ptr.assign((size_t)nt + 1, 0);
    st.row.resize((size_t)ne);
    st.col.resize((size_t)ne);
    st.slot.resize((size_t)ne);
    st.w.resize((size_t)ne);
    st.tile_slots.assign((size_t)nt, 0);
    st.max_slots = 0;
    std::vector<int64_t> at;
    std::vector<int32_t> col_of;
    for (int64_t t = 0; t < nt; ++t) {
        const int64_t v0 = t * kSgVisitorsTile, v1 = std::min(nv, v0 + kSgVisitorsTile);
        const int64_t e0 = offsets[v0], e1 = offsets[v1];
        st.tile_ptr[(size_t)t] = e0;
        st.tile_ptr[(size_t)t + 1] = e1;
        at.resize((size_t)(e1 - e0));
        col_of.resize((size_t)(e1 - e0));
        std::iota(at.begin(), at.end(), e0);
        for (int64_t v = v0; v < v1; ++v)
            for (int64_t e = offsets[v]; e < offsets[v + 1]; ++e) col_of[(size_t)(e - e0)] = (int32_t)(v - v0);
        std::sort(at.begin(), at.end(), [&](int64_t a, int64_t b) { return live_row[a] != live_row[b] ? live_row[a] < live_row[b] : a < b; });
        int32_t slots = 0;
        for (int64_t i = 0; i < e1 - e0; ++i) {
            const int64_t e = at[(size_t)i];
            if (i > 0 && live_row[e] != live_row[at[(size_t)i - 1]]) ++slots;
            st.row[(size_t)(e0 + i)] = live_row[e];
            st.col[(size_t)(e0 + i)] = col_of[(size_t)(e - e0)];
            st.slot[(size_t)(e0 + i)] = slots;
            st.w[(size_t)(e0 + i)] = weight[e];
        }
        st.tile_slots[(size_t)t] = e1 > e0 ? slots + 1 : 0;
        st.max_slots = std::max(st.max_slots, st.tile_slots[(size_t)t]);
    }
}

}  // namespace locrec
