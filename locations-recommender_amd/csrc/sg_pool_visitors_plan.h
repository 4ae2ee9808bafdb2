// sg_pool_visitors_plan.h -- what the host decides for ONE mixed batch of SG visitors over a pool of graphs
// (locrec_sg_pool_visitors_*, sg_pool_visitors.h): the members asked, each member's visitors in call order with their
// gathered CSR, its tiles and per-tile stage (sg_visitors_plan.h's), where its staged edges, its slot table and its weight
// table lie in the call's two device buffers, the number of tile waves, and every visitor's position in emit order.
// Plain C++ without a device call: tests/host/sg_pool_visitors_plan_check.cpp runs it stand-alone, under a host sanitizer too.
//
//   4-byte buffer   row[E] | col[E] | slot[E] | the asked members' slot tables, one behind the other (T entries each, at -1)
//   8-byte buffer   w[E] | the asked members' weight tables (the lines of the member's largest tile, 16 fp64 a line; every
//                   table starts on a line of its own: a multiple of 16 words)
//   E               every member's staged edges, member by member; inside a member tile by tile (SgVisitorsStage)
//   emit order      by tile wave, then member in pool order, then column: wave k of a member is its visitors 16k .. 16k+15
#pragma once

#include "sg_visitors_plan.h"

namespace locrec {

// A member somebody asks
struct SgPoolVisitorsMember {
    int32_t graph = 0;              // its index in the pool
    std::vector<int64_t> visitors;  // the call positions of its visitors, ascending
    std::vector<int64_t> offsets;   // its gathered CSR: visitor j of the member has edges offsets[j] .. offsets[j + 1]
    SgVisitorsStage st;             // tile_ptr, tile_slots, max_slots (the staged edges themselves stand in the plan's arrays)
    int64_t edge_base = 0;          // its staged edges are positions edge_base + st.tile_ptr[t] .. of the plan's arrays
    int64_t slot_off = 0, slot_len = 0;  // its slot table: words of the 4-byte buffer
    int64_t w_off = 0, w_len = 0;        // its weight table: words of the 8-byte buffer
    size_t count() const { return visitors.size(); }
    size_t waves() const { return (size_t)st.tiles(); }
};

struct SgPoolVisitorsPlan {
    std::vector<SgPoolVisitorsMember> members;  // in member order
    std::vector<int32_t> member_of;             // visitor -> its entry of members
    std::vector<int32_t> rank_of;               // visitor -> its position among its member's visitors
    std::vector<int64_t> emit_of, ord;          // visitor -> emit position, and back
    std::vector<int32_t> row, col, slot;        // the call's staged edges
    std::vector<double> w;
    int64_t words32 = 0, words64 = 0;  // the two buffers
    size_t waves = 0;
    int64_t edges() const { return (int64_t)row.size(); }
};

// nv visitors; visitor v is asked of member graph_index[v] (checked: inside [0, n_graphs)) and its edges are positions
// offsets[v] .. offsets[v + 1] of live_row / weight (live_row: the target's live index in ITS member, checked as
// sg_visitors_stage wants them).  nlive[g]: the live rows of member g.
inline void sg_pool_visitors_plan(int64_t nv, const int32_t *graph_index, const int64_t *offsets, const int32_t *live_row,
                                  const double *weight, int32_t n_graphs, const int32_t *nlive, SgPoolVisitorsPlan &out)
{
    out = SgPoolVisitorsPlan();
    out.member_of.assign((size_t)nv, 0);
    out.rank_of.assign((size_t)nv, 0);
    std::vector<int32_t> entry((size_t)n_graphs, -1);
    std::vector<int64_t> asked((size_t)n_graphs, 0);
    for (int64_t v = 0; v < nv; ++v) ++asked[(size_t)graph_index[v]];
    for (int32_t g = 0; g < n_graphs; ++g)
        if (asked[(size_t)g] > 0) {
            entry[(size_t)g] = (int32_t)out.members.size();
            out.members.emplace_back();
            out.members.back().graph = g;
            out.members.back().visitors.reserve((size_t)asked[(size_t)g]);
        }
    for (int64_t v = 0; v < nv; ++v) {
        SgPoolVisitorsMember &m = out.members[(size_t)entry[(size_t)graph_index[v]]];
        out.member_of[(size_t)v] = entry[(size_t)graph_index[v]];
        out.rank_of[(size_t)v] = (int32_t)m.visitors.size();
        m.visitors.push_back(v);
    }
    const int64_t ne = nv > 0 ? offsets[nv] : 0;
    out.row.reserve((size_t)ne);
    out.col.reserve((size_t)ne);
    out.slot.reserve((size_t)ne);
    out.w.reserve((size_t)ne);
    std::vector<int32_t> live;
    std::vector<double> wg;
    for (SgPoolVisitorsMember &m : out.members) {
        m.offsets.assign(1, 0);
        live.clear();
        wg.clear();
        for (const int64_t v : m.visitors) {
            live.insert(live.end(), live_row + offsets[v], live_row + offsets[v + 1]);
            wg.insert(wg.end(), weight + offsets[v], weight + offsets[v + 1]);
            m.offsets.push_back((int64_t)live.size());
        }
        sg_visitors_stage((int64_t)m.count(), m.offsets.data(), live.data(), wg.data(), m.st);
        m.edge_base = out.edges();
        out.row.insert(out.row.end(), m.st.row.begin(), m.st.row.end());
        out.col.insert(out.col.end(), m.st.col.begin(), m.st.col.end());
        out.slot.insert(out.slot.end(), m.st.slot.begin(), m.st.slot.end());
        out.w.insert(out.w.end(), m.st.w.begin(), m.st.w.end());
        std::vector<int32_t>().swap(m.st.row);
        std::vector<int32_t>().swap(m.st.col);
        std::vector<int32_t>().swap(m.st.slot);
        std::vector<double>().swap(m.st.w);
        out.waves = std::max(out.waves, m.waves());
    }
    out.words32 = 3 * ne;
    out.words64 = (ne + kSgVisitorsTile - 1) / kSgVisitorsTile * kSgVisitorsTile;
    for (SgPoolVisitorsMember &m : out.members) {
        m.slot_off = out.words32;
        m.slot_len = (int64_t)SgVisitorsStage::slot_table(nlive[m.graph]);
        out.words32 += m.slot_len;
        m.w_off = out.words64;
        m.w_len = (int64_t)m.st.weight_table();
        out.words64 += m.w_len;
    }
    out.emit_of.assign((size_t)nv, 0);
    out.ord.assign((size_t)nv, 0);
    int64_t at = 0;
    for (size_t k = 0; k < out.waves; ++k)
        for (const SgPoolVisitorsMember &m : out.members)
            for (size_t j = k * kSgVisitorsTile; j < std::min(m.count(), (k + 1) * kSgVisitorsTile); ++j) {
                out.emit_of[(size_t)m.visitors[j]] = at;
                out.ord[(size_t)at++] = m.visitors[j];
            }
}

}  // namespace locrec
