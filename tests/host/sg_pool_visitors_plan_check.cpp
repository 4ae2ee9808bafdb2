// The host plan of a pool visitors call (csrc/sg_pool_visitors_plan.h) against brute force and literals: the members asked,
// each member's visitors and gathered CSR, its tiles and stage, where its tables lie in the call's buffers, the waves and
// the emit order - which is sg_rk_pool_order's (csrc/sg_rk_plan.h) for one request per visitor.
// Stand-alone: c++ -std=c++17 -I locations-recommender_amd/csrc tests/host/sg_pool_visitors_plan_check.cpp
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "sg_pool_visitors_plan.h"
#include "sg_rk_plan.h"

using namespace locrec;

static int cases = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        ++cases;                                                        \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
            return 1;                                                   \
        }                                                               \
    } while (0)

struct Call {
    std::vector<int32_t> gi;
    std::vector<int64_t> off = {0};
    std::vector<int32_t> row;
    std::vector<double> w;
    std::vector<int32_t> nlive;
    int64_t nv() const { return (int64_t)gi.size(); }
};

// the plan against a walk of the input
static int check_plan(const Call &c)
{
    const int64_t nv = c.nv();
    const int32_t ng = (int32_t)c.nlive.size();
    SgPoolVisitorsPlan p;
    sg_pool_visitors_plan(nv, c.gi.data(), c.off.data(), c.row.data(), c.w.data(), ng, c.nlive.data(), p);
    // the members asked, in member order; nobody else
    std::map<int32_t, std::vector<int64_t>> want;
    for (int64_t v = 0; v < nv; ++v) want[c.gi[(size_t)v]].push_back(v);
    CHECK(p.members.size() == want.size());
    CHECK((int64_t)p.member_of.size() == nv && (int64_t)p.rank_of.size() == nv);
    size_t a = 0, waves = 0;
    int64_t edges = 0;
    std::vector<std::pair<int64_t, int64_t>> spans32, spans64;  // the tables' ranges
    for (const auto &kv : want) {
        const SgPoolVisitorsMember &m = p.members[a];
        CHECK(m.graph == kv.first && m.visitors == kv.second && m.count() == kv.second.size());
        CHECK(m.offsets.size() == m.count() + 1 && m.offsets[0] == 0);
        CHECK(m.waves() == (m.count() + 15) / 16 && m.st.tiles() == (int64_t)m.waves());
        CHECK(m.edge_base == edges);
        waves = std::max(waves, m.waves());
        for (size_t j = 0; j < m.count(); ++j) {
            const int64_t v = m.visitors[j];
            CHECK(p.member_of[(size_t)v] == (int32_t)a && p.rank_of[(size_t)v] == (int32_t)j);
            CHECK(m.offsets[j + 1] - m.offsets[j] == c.off[(size_t)v + 1] - c.off[(size_t)v]);
        }
        CHECK((int64_t)m.st.tile_ptr.size() == m.st.tiles() + 1 && m.st.tile_ptr[0] == 0 && m.st.tile_ptr.back() == m.offsets.back());
        // every tile's stage: each edge of its visitors once, (row, column) ascending, the slot the rank of the row
        int32_t max_slots = 0;
        for (size_t t = 0; t < m.waves(); ++t) {
            const size_t j0 = 16 * t, j1 = std::min(m.count(), j0 + 16);
            CHECK(m.st.tile_ptr[t] == m.offsets[j0] && m.st.tile_ptr[t + 1] == m.offsets[j1]);
            std::map<std::pair<int32_t, int32_t>, double> cell;
            std::set<int32_t> rows;
            for (size_t j = j0; j < j1; ++j)
                for (int64_t e = c.off[(size_t)m.visitors[j]]; e < c.off[(size_t)m.visitors[j] + 1]; ++e) {
                    cell[{c.row[(size_t)e], (int32_t)(j - j0)}] = c.w[(size_t)e];
                    rows.insert(c.row[(size_t)e]);
                    CHECK(c.row[(size_t)e] >= 0 && c.row[(size_t)e] < c.nlive[(size_t)m.graph]);
                }
            CHECK((int64_t)cell.size() == m.st.tile_ptr[t + 1] - m.st.tile_ptr[t]);
            CHECK(m.st.tile_slots[t] == (int32_t)rows.size());
            max_slots = std::max(max_slots, (int32_t)rows.size());
            const std::vector<int32_t> distinct(rows.begin(), rows.end());
            auto it = cell.begin();
            for (int64_t i = m.edge_base + m.st.tile_ptr[t]; i < m.edge_base + m.st.tile_ptr[t + 1]; ++i, ++it) {
                CHECK(p.row[(size_t)i] == it->first.first && p.col[(size_t)i] == it->first.second && p.w[(size_t)i] == it->second);
                CHECK(p.slot[(size_t)i] >= 0 && p.slot[(size_t)i] < m.st.tile_slots[t] && distinct[(size_t)p.slot[(size_t)i]] == p.row[(size_t)i]);
            }
        }
        CHECK(m.st.max_slots == max_slots);
        CHECK(m.slot_len == std::max(1, c.nlive[(size_t)m.graph]) && m.w_len == (int64_t)std::max(1, max_slots) * 16);
        CHECK(m.w_off % 16 == 0);
        spans32.push_back({m.slot_off, m.slot_off + m.slot_len});
        spans64.push_back({m.w_off, m.w_off + m.w_len});
        edges += m.offsets.back();
        ++a;
    }
    CHECK(edges == (nv > 0 ? c.off[(size_t)nv] : 0) && p.edges() == edges);
    CHECK((int64_t)p.col.size() == edges && (int64_t)p.slot.size() == edges && (int64_t)p.w.size() == edges);
    CHECK(p.waves == waves);
    // the tables lie behind the staged edges, one behind the other, inside the buffers
    int64_t at32 = 3 * edges, at64 = edges;
    for (size_t i = 0; i < spans32.size(); ++i) {
        CHECK(spans32[i].first >= at32 && spans64[i].first >= at64);
        at32 = spans32[i].second;
        at64 = spans64[i].second;
    }
    CHECK(at32 <= p.words32 && at64 <= p.words64 && p.words32 >= 3 * edges && p.words64 >= edges);
    CHECK(p.words32 == at32 && (spans64.empty() || p.words64 == at64));
    // the emit order: wave, then member, then column; a permutation and its inverse; sg_rk_pool_order's
    CHECK((int64_t)p.ord.size() == nv && (int64_t)p.emit_of.size() == nv);
    std::vector<int64_t> brute;
    for (size_t k = 0; k < waves; ++k)
        for (const auto &kv : want)
            for (size_t j = 16 * k; j < std::min(kv.second.size(), 16 * k + 16); ++j) brute.push_back(kv.second[j]);
    CHECK(brute == p.ord);
    for (int64_t k = 0; k < nv; ++k) CHECK(p.emit_of[(size_t)p.ord[(size_t)k]] == k);
    std::vector<size_t> nu;
    for (const SgPoolVisitorsMember &m : p.members) nu.push_back(m.count());
    SgRkPoolOrder order;
    sg_rk_pool_order(nu, std::vector<int>(nu.size(), 16), p.member_of, p.rank_of, order);
    CHECK(order.ord == p.ord && order.waves == waves);
    return 0;
}

// visitor of member g with the given rows
static void add(Call &c, int32_t g, std::initializer_list<int32_t> rows, double w0)
{
    c.gi.push_back(g);
    double w = w0;
    for (int32_t r : rows) {
        c.row.push_back(r);
        c.w.push_back(w);
        w += 0.125;
    }
    c.off.push_back((int64_t)c.row.size());
}

int main()
{
    // nobody
    {
        Call c;
        c.nlive = {5, 7};
        SgPoolVisitorsPlan p;
        sg_pool_visitors_plan(0, nullptr, c.off.data(), nullptr, nullptr, 2, c.nlive.data(), p);
        CHECK(p.members.empty() && p.waves == 0 && p.edges() == 0 && p.words32 == 0 && p.words64 == 0 && p.ord.empty());
        if (check_plan(c)) return 1;
    }
    // a literal: four members, member 1 is asked by nobody, the visitors interleaved
    {
        Call c;
        c.nlive = {10, 99, 4, 0x7000};
        add(c, 2, {3, 1}, 0.5);        // visitor 0
        add(c, 0, {9}, 1.0);           // 1
        add(c, 3, {100, 7, 20000}, 2.0);  // 2
        add(c, 2, {1}, 4.0);           // 3
        add(c, 0, {9, 0}, 8.0);        // 4
        SgPoolVisitorsPlan p;
        sg_pool_visitors_plan(5, c.gi.data(), c.off.data(), c.row.data(), c.w.data(), 4, c.nlive.data(), p);
        CHECK(p.members.size() == 3 && p.members[0].graph == 0 && p.members[1].graph == 2 && p.members[2].graph == 3);
        CHECK((p.members[0].visitors == std::vector<int64_t>{1, 4}) && (p.members[1].visitors == std::vector<int64_t>{0, 3}));
        CHECK((p.member_of == std::vector<int32_t>{1, 0, 2, 1, 0}) && (p.rank_of == std::vector<int32_t>{0, 0, 0, 1, 1}));
        CHECK((p.ord == std::vector<int64_t>{1, 4, 0, 3, 2}) && (p.emit_of == std::vector<int64_t>{2, 0, 4, 3, 1}) && p.waves == 1);
        // member 0: rows {9: columns 0 and 1, 0: column 1}; member 2: rows {1: columns 0 and 1, 3: column 0}; member 3
        CHECK((p.row == std::vector<int32_t>{0, 9, 9, 1, 1, 3, 7, 100, 20000}));
        CHECK((p.col == std::vector<int32_t>{1, 0, 1, 0, 1, 0, 0, 0, 0}));
        CHECK((p.slot == std::vector<int32_t>{0, 1, 1, 0, 0, 1, 0, 1, 2}));
        CHECK((p.w == std::vector<double>{8.125, 1.0, 8.0, 0.625, 4.0, 0.5, 2.125, 2.0, 2.25}));
        CHECK(p.members[0].edge_base == 0 && p.members[1].edge_base == 3 && p.members[2].edge_base == 6);
        CHECK(p.members[0].slot_off == 27 && p.members[1].slot_off == 37 && p.members[2].slot_off == 41 && p.words32 == 41 + 0x7000);
        CHECK(p.members[0].w_off == 16 && p.members[0].w_len == 32 && p.members[1].w_off == 48 && p.members[2].w_off == 80);
        CHECK(p.members[2].w_len == 48 && p.words64 == 128);
        if (check_plan(c)) return 1;
    }
    // members that drop out of the waves: 33, 2 and 17 visitors -> three waves, the last with member 0 only
    {
        Call c;
        c.nlive = {50, 50, 50};
        const int count[3] = {33, 2, 17};
        int left[3] = {33, 2, 17};
        for (int i = 0; left[0] + left[1] + left[2] > 0; ++i) {
            const int g = i % 3;
            if (left[g] == 0) continue;
            const int j = count[g] - left[g]--;
            add(c, g, {(int32_t)(j % 50), (int32_t)((j + 7) % 50)}, 1.0 + j);
        }
        SgPoolVisitorsPlan p;
        sg_pool_visitors_plan(c.nv(), c.gi.data(), c.off.data(), c.row.data(), c.w.data(), 3, c.nlive.data(), p);
        CHECK(p.waves == 3 && p.members[0].waves() == 3 && p.members[1].waves() == 1 && p.members[2].waves() == 2);
        // wave 0: 16 + 2 + 16 positions, wave 1: 16 + 1, wave 2: 1
        CHECK(p.member_of[(size_t)p.ord[15]] == 0 && p.member_of[(size_t)p.ord[16]] == 1 && p.member_of[(size_t)p.ord[18]] == 2);
        CHECK(p.member_of[(size_t)p.ord[34]] == 0 && p.rank_of[(size_t)p.ord[34]] == 16 && p.member_of[(size_t)p.ord[50]] == 2);
        CHECK(p.rank_of[(size_t)p.ord[50]] == 16 && p.member_of[(size_t)p.ord[51]] == 0 && p.rank_of[(size_t)p.ord[51]] == 32);
        if (check_plan(c)) return 1;
    }
    // generated calls: 1 .. 9 members, some asked by nobody, member sizes on both sides of a tile's 16, a deterministic generator
    for (int32_t ng : {1, 2, 5, 9}) {
        for (int64_t nv : {1, 15, 16, 17, 40, 131}) {
            uint64_t state = 88172645463325252ull + (uint64_t)nv * 1000 + (uint64_t)ng;
            auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
            Call c;
            for (int32_t g = 0; g < ng; ++g) c.nlive.push_back((int32_t)(12 + next() % 300));
            const int32_t idle = ng > 2 ? (int32_t)(next() % (uint64_t)ng) : -1;
            for (int64_t v = 0; v < nv; ++v) {
                int32_t g = (int32_t)(next() % (uint64_t)ng);
                if (next() % 3 == 0) g = 0;  // (one member gets more than the others: several waves)
                if (g == idle) g = (g + 1) % ng;
                std::set<int32_t> mine;
                const int k = 1 + (int)(next() % 12);
                while ((int)mine.size() < k) mine.insert((int32_t)(next() % (uint64_t)c.nlive[(size_t)g]));
                std::vector<int32_t> order(mine.begin(), mine.end());
                for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[next() % i]);
                c.gi.push_back(g);
                for (int32_t r : order) {
                    c.row.push_back(r);
                    c.w.push_back((double)(next() % 1000) / 1000.0);
                }
                c.off.push_back((int64_t)c.row.size());
            }
            if (check_plan(c)) return 1;
        }
    }
    printf("%d cases pass\n", cases);
    return 0;
}
