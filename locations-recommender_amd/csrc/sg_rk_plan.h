// sg_rk_plan.h -- the host's planning of the ranked SG entries (sg_ranked.h, sg_pool_ranked.h): the emit order of a call's
// requests, the groups whose segments share one row buffer and one ranker call, the parts they cut a tile wave into.
// Plain C++ without a device call: tests/host/sg_rk_plan_check.cpp runs it stand-alone, under a host sanitizer too.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace locrec {

// Groups: runs of the emit order.  Request k's segment has room cap[k]; a group ends in front of the request whose room
// would take the group's rows past `budget` (a group has at least one request).
struct SgRkGroups {
    std::vector<int64_t> seg_begin;  // request k's segment starts at this row of its group's buffer
    std::vector<int64_t> group_end;  // one past the last request of group i
    int64_t max_rows = 1, max_req = 1, max_cap = 0;  // the largest group's rows and requests, the largest segment
};

inline void sg_rk_form_groups(const std::vector<int64_t> &cap, int64_t budget, SgRkGroups &out)
{
    const int64_t n = (int64_t)cap.size();
    out = SgRkGroups();
    out.seg_begin.resize((size_t)n);
    int64_t cur_rows = 0, cur_first = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t c = cap[(size_t)k];
        if (k > cur_first && cur_rows + c > budget) {
            out.group_end.push_back(k);
            cur_first = k;
            cur_rows = 0;
        }
        out.seg_begin[(size_t)k] = cur_rows;
        cur_rows += c;
        out.max_rows = std::max(out.max_rows, cur_rows);
        out.max_req = std::max(out.max_req, k + 1 - cur_first);
        out.max_cap = std::max(out.max_cap, c);
    }
    out.group_end.push_back(n);
}

// The emit order of a pool call: by tile wave, then member (in the order of `nu`), then distinct target of the member's
// tile, then input position.  Member a has nu[a] distinct targets and iterates tile_max[a] of them per wave; request i
// asks member member_of[i] for its distinct target uniq_of[i].
struct SgRkPoolOrder {
    std::vector<size_t> ubase;   // member a's distinct targets are flat entries ubase[a] .. ubase[a + 1]
    std::vector<int64_t> first;  // flat entry f's requests are emit positions first[f] .. first[f] + count[f]
    std::vector<int64_t> count;
    std::vector<int64_t> ord;    // emit position -> input position
    size_t waves = 0;
    // the emit positions of member a's tile of wave k: [begin, end)
    int64_t tile_begin(size_t a, size_t k, int tile_max) const { return first[ubase[a] + k * (size_t)tile_max]; }
    int64_t tile_end(size_t a, size_t k, int tile_max) const
    {
        const size_t last = std::min(ubase[a + 1], ubase[a] + (k + 1) * (size_t)tile_max) - 1;
        return first[last] + count[last];
    }
};

inline void sg_rk_pool_order(const std::vector<size_t> &nu, const std::vector<int> &tile_max, const std::vector<int32_t> &member_of,
                             const std::vector<int32_t> &uniq_of, SgRkPoolOrder &out)
{
    const size_t na = nu.size(), n = member_of.size();
    out = SgRkPoolOrder();
    out.ubase.assign(na + 1, 0);
    for (size_t a = 0; a < na; ++a) {
        out.ubase[a + 1] = out.ubase[a] + nu[a];
        out.waves = std::max(out.waves, (nu[a] + (size_t)tile_max[a] - 1) / (size_t)tile_max[a]);
    }
    out.count.assign(out.ubase[na], 0);
    out.first.assign(out.ubase[na], 0);
    for (size_t i = 0; i < n; ++i) ++out.count[out.ubase[(size_t)member_of[i]] + (size_t)uniq_of[i]];
    int64_t at = 0;
    for (size_t k = 0; k < out.waves; ++k)
        for (size_t a = 0; a < na; ++a) {
            const size_t tm = (size_t)tile_max[a];
            for (size_t u = k * tm; u < std::min(nu[a], (k + 1) * tm); ++u) {
                out.first[out.ubase[a] + u] = at;
                at += out.count[out.ubase[a] + u];
            }
        }
    out.ord.assign(n, 0);
    std::vector<int64_t> next(out.first);
    for (size_t i = 0; i < n; ++i) out.ord[(size_t)next[out.ubase[(size_t)member_of[i]] + (size_t)uniq_of[i]]++] = (int64_t)i;
}

// A tile wave's requests are one run [lo, hi) of the emit order; the groups that end inside it cut it into parts, one
// emit launch each.  members: those with a tile in wave k, not empty.  cuts: lo, the group ends inside (lo, hi), hi.
inline void sg_rk_wave_cuts(const std::vector<size_t> &members, size_t k, const std::vector<int> &tile_max, const SgRkPoolOrder &order,
                            const std::vector<int64_t> &group_end, std::vector<int64_t> &cuts)
{
    int64_t lo = INT64_MAX, hi = 0;
    for (const size_t a : members) {
        lo = std::min(lo, order.tile_begin(a, k, tile_max[a]));
        hi = std::max(hi, order.tile_end(a, k, tile_max[a]));
    }
    cuts.assign(1, lo);
    for (auto ge = std::upper_bound(group_end.begin(), group_end.end(), lo); ge != group_end.end() && *ge < hi; ++ge) cuts.push_back(*ge);
    cuts.push_back(hi);
}

// The rows of a pool call's table: a row per member and part, of the wave that has the most
inline size_t sg_rk_pool_table_rows(const std::vector<size_t> &nu, const std::vector<int> &tile_max, const SgRkPoolOrder &order,
                                    const std::vector<int64_t> &group_end)
{
    size_t rows = 1;
    std::vector<size_t> members;
    std::vector<int64_t> cuts;
    for (size_t k = 0; k < order.waves; ++k) {
        members.clear();
        for (size_t a = 0; a < nu.size(); ++a)
            if (k * (size_t)tile_max[a] < nu[a]) members.push_back(a);
        sg_rk_wave_cuts(members, k, tile_max, order, group_end, cuts);
        rows = std::max(rows, members.size() * (cuts.size() - 1));
    }
    return rows;
}

}  // namespace locrec
