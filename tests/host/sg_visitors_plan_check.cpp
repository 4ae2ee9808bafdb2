// The host decisions of an SG visitors call (csrc/sg_visitors_plan.h) against brute force and literals: the tiles, a
// visitor's repeated target, a tile's edges by live row with their columns, slots and weights, the tables' sizes.
// Stand-alone: c++ -std=c++17 -I locations-recommender_amd/csrc tests/host/sg_visitors_plan_check.cpp
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "sg_visitors_plan.h"

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

// the stage of nv visitors against a walk of the input: every edge once, in its tile, with its visitor's column; rows
// ascending inside a tile, columns ascending inside a row; slots the rank of the row among the tile's distinct rows
static int check_stage(int64_t nv, const std::vector<int64_t> &off, const std::vector<int32_t> &row, const std::vector<double> &w)
{
    SgVisitorsStage st;
    sg_visitors_stage(nv, off.data(), row.data(), w.data(), st);
    const int64_t nt = sg_visitors_tiles(nv);
    CHECK(st.tiles() == nt && st.edges() == (nv > 0 ? off[(size_t)nv] : 0));
    CHECK((int64_t)st.tile_ptr.size() == nt + 1 && st.tile_ptr[0] == 0 && st.tile_ptr[(size_t)nt] == st.edges());
    int32_t max_slots = 0;
    for (int64_t t = 0; t < nt; ++t) {
        const int64_t v0 = t * 16, v1 = std::min<int64_t>(nv, v0 + 16);
        CHECK(st.tile_ptr[(size_t)t] == off[(size_t)v0] && st.tile_ptr[(size_t)t + 1] == off[(size_t)v1]);
        std::map<std::pair<int32_t, int32_t>, double> want;  // (row, column) -> weight
        std::set<int32_t> rows;
        for (int64_t v = v0; v < v1; ++v)
            for (int64_t e = off[(size_t)v]; e < off[(size_t)v + 1]; ++e) {
                want[{row[(size_t)e], (int32_t)(v - v0)}] = w[(size_t)e];
                rows.insert(row[(size_t)e]);
            }
        CHECK((int64_t)want.size() == off[(size_t)v1] - off[(size_t)v0]);  // (the input names a row once a visitor)
        CHECK(st.tile_slots[(size_t)t] == (int32_t)rows.size());
        max_slots = std::max(max_slots, (int32_t)rows.size());
        const std::vector<int32_t> distinct(rows.begin(), rows.end());
        auto it = want.begin();  // (a map walks (row, column) ascending: the stage's order)
        for (int64_t i = st.tile_ptr[(size_t)t]; i < st.tile_ptr[(size_t)t + 1]; ++i, ++it) {
            CHECK(st.row[(size_t)i] == it->first.first && st.col[(size_t)i] == it->first.second && st.w[(size_t)i] == it->second);
            CHECK(st.col[(size_t)i] >= 0 && st.col[(size_t)i] < kSgVisitorsTile);
            CHECK(st.slot[(size_t)i] >= 0 && st.slot[(size_t)i] < st.tile_slots[(size_t)t]);
            CHECK(distinct[(size_t)st.slot[(size_t)i]] == st.row[(size_t)i]);
        }
    }
    CHECK(st.max_slots == max_slots);
    CHECK(st.weight_table() == (size_t)std::max(1, max_slots) * 16);
    return 0;
}

int main()
{
    CHECK(kSgVisitorsTile == 16);
    for (int64_t nv : {0, 1, 15, 16, 17, 32, 33, 40}) CHECK(sg_visitors_tiles(nv) == (nv + 15) / 16);
    CHECK(sg_visitors_tiles(40) == 3 && sg_visitors_tiles(16) == 1 && sg_visitors_tiles(17) == 2 && sg_visitors_tiles(0) == 0);
    // a repeated target: the position of the first edge whose row occurred before it
    {
        const int32_t a[] = {5, 3, 9}, b[] = {5, 3, 5}, c[] = {7, 7}, d[] = {1, 2, 3, 2, 1}, e[] = {4};
        CHECK(sg_visitors_first_repeat(a, 3) == -1 && sg_visitors_first_repeat(b, 3) == 2 && sg_visitors_first_repeat(c, 2) == 1);
        CHECK(sg_visitors_first_repeat(d, 5) == 3 && sg_visitors_first_repeat(e, 1) == -1 && sg_visitors_first_repeat(e, 0) == -1);
    }
    // the sizes never are 0 (an allocation of its own), a graph without live rows included
    CHECK(SgVisitorsStage::slot_table(0) == 1 && SgVisitorsStage::slot_table(1) == 1 && SgVisitorsStage::slot_table(65535) == 65535);
    // a literal: three visitors, rows shared between them
    {
        const std::vector<int64_t> off = {0, 2, 3, 6};
        const std::vector<int32_t> row = {9, 2, 9, 4, 2, 30};
        const std::vector<double> w = {0.5, 0.25, 1.0, 0.0, -3.0, 7.0};
        SgVisitorsStage st;
        sg_visitors_stage(3, off.data(), row.data(), w.data(), st);
        CHECK((st.row == std::vector<int32_t>{2, 2, 4, 9, 9, 30}) && (st.col == std::vector<int32_t>{0, 2, 2, 0, 1, 2}));
        CHECK((st.slot == std::vector<int32_t>{0, 0, 1, 2, 2, 3}) && (st.w == std::vector<double>{0.25, -3.0, 0.0, 0.5, 1.0, 7.0}));
        CHECK(st.max_slots == 4 && st.tiles() == 1 && st.weight_table() == 64);
        if (check_stage(3, off, row, w)) return 1;
    }
    // nobody
    {
        SgVisitorsStage st;
        sg_visitors_stage(0, nullptr, nullptr, nullptr, st);
        CHECK(st.tiles() == 0 && st.edges() == 0 && st.max_slots == 0 && st.weight_table() == 16 && st.tile_ptr.size() == 1);
    }
    // generated calls on both sides of a tile's 16: 1 .. 12 distinct rows a visitor out of T, a deterministic generator
    for (int64_t nv : {1, 15, 16, 17, 31, 32, 33, 40}) {
        for (int32_t T : {12, 40, 70000}) {
            uint64_t state = 88172645463325252ull + (uint64_t)nv * 1000 + (uint64_t)T;
            auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
            std::vector<int64_t> off = {0};
            std::vector<int32_t> row;
            std::vector<double> w;
            for (int64_t v = 0; v < nv; ++v) {
                std::set<int32_t> mine;
                const int k = 1 + (int)(next() % 12);
                while ((int)mine.size() < k) mine.insert((int32_t)(next() % (uint64_t)T));
                std::vector<int32_t> order(mine.begin(), mine.end());
                for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[next() % i]);  // (any order in the input)
                for (int32_t r : order) {
                    row.push_back(r);
                    w.push_back((double)(next() % 1000) / 1000.0);
                }
                off.push_back((int64_t)row.size());
                CHECK(sg_visitors_first_repeat(row.data() + off[(size_t)v], k) == -1);
            }
            if (check_stage(nv, off, row, w)) return 1;
        }
    }
    // one tile of 255, 256 and 257 edges (a stride of the set-up kernel's loops, one short and one over): 16 visitors
    // with 16 rows each out of T = 600, visitor 9 with 15, 16 or 17
    for (int edges : {255, 256, 257}) {
        std::vector<int64_t> off = {0};
        std::vector<int32_t> row;
        std::vector<double> w;
        for (int v = 0; v < 16; ++v) {
            const int k = v == 9 ? edges - 240 : 16;
            for (int j = 0; j < k; ++j) {
                row.push_back((int32_t)((v * 37 + j * 41) % 600));  // (41 and 600 are coprime: no row twice in a visitor)
                w.push_back(1.0 / k);
            }
            off.push_back((int64_t)row.size());
            CHECK(sg_visitors_first_repeat(row.data() + off[(size_t)v], k) == -1);
        }
        SgVisitorsStage st;
        sg_visitors_stage(16, off.data(), row.data(), w.data(), st);
        CHECK(st.tiles() == 1 && st.edges() == edges && st.tile_ptr[1] == edges && st.max_slots <= edges);
        if (check_stage(16, off, row, w)) return 1;
    }
    // one visitor that names every row of T = 600, in any order: as many lines as rows and as edges, slot == row
    {
        std::vector<int64_t> off = {0, 600};
        std::vector<int32_t> row;
        std::vector<double> w;
        for (int j = 0; j < 600; ++j) {
            row.push_back((int32_t)((j * 7 + 3) % 600));
            w.push_back(1.0 / 600);
        }
        SgVisitorsStage st;
        sg_visitors_stage(1, off.data(), row.data(), w.data(), st);
        CHECK(st.max_slots == 600 && st.edges() == 600 && st.weight_table() == 600 * 16);
        for (int j = 0; j < 600; ++j) CHECK(st.row[(size_t)j] == j && st.slot[(size_t)j] == j && st.col[(size_t)j] == 0);
        if (check_stage(1, off, row, w)) return 1;
    }
    // three tiles whose tables follow each other: 16 visitors at all 40 rows of A = {0, 14, ..}; 16 visitors at B = {7, 21,
    // ..} only, each row of B named by one of them; three visitors with three rows of A, one of B and one of neither
    {
        std::vector<int64_t> off = {0};
        std::vector<int32_t> row;
        std::vector<double> w;
        auto add = [&](std::initializer_list<int32_t> rows, double x) {
            for (int32_t r : rows) {
                row.push_back(r);
                w.push_back(x);
            }
        };
        for (int v = 0; v < 16; ++v) {
            for (int k = 0; k < 40; ++k) add({(int32_t)(14 * ((k + v) % 40))}, 0.025 + v);
            off.push_back((int64_t)row.size());
        }
        for (int v = 0; v < 16; ++v) {
            for (int k = v; k < 40; k += 16) add({(int32_t)(7 + 14 * k)}, 0.5);
            off.push_back((int64_t)row.size());
        }
        const int32_t neither[3] = {13, 27, 41};
        for (int v = 0; v < 3; ++v) {
            add({(int32_t)(14 * (5 * v + 20)), (int32_t)(14 * (5 * v + 1)), (int32_t)(14 * (39 - v)), (int32_t)(7 + 14 * (30 + v)), neither[v]}, 0.2);
            off.push_back((int64_t)row.size());
        }
        SgVisitorsStage st;
        sg_visitors_stage(35, off.data(), row.data(), w.data(), st);
        CHECK((st.tile_ptr == std::vector<int64_t>{0, 640, 680, 695}) && (st.tile_slots == std::vector<int32_t>{40, 40, 15}));
        CHECK(st.max_slots == 40 && st.weight_table() == 640);
        for (int i = 0; i < 640; ++i)  // tile 0: every (slot, column) pair once, the columns of a line ascending
            CHECK(st.row[(size_t)i] == 14 * (i / 16) && st.slot[(size_t)i] == i / 16 && st.col[(size_t)i] == i % 16);
        for (int k = 0; k < 40; ++k)  // tile 1: as many lines, one column each
            CHECK(st.row[(size_t)(640 + k)] == 7 + 14 * k && st.slot[(size_t)(640 + k)] == k && st.col[(size_t)(640 + k)] == k % 16);
        // tile 2: 15 lines over rows of A, B and neither, in ascending order of the rows
        CHECK((std::vector<int32_t>(st.row.begin() + 680, st.row.end()) ==
               std::vector<int32_t>{13, 14, 27, 41, 84, 154, 280, 350, 420, 427, 441, 455, 518, 532, 546}));
        CHECK((std::vector<int32_t>(st.col.begin() + 680, st.col.end()) == std::vector<int32_t>{0, 0, 1, 2, 1, 2, 0, 1, 2, 0, 1, 2, 2, 1, 0}));
        for (int i = 0; i < 15; ++i) CHECK(st.slot[(size_t)(680 + i)] == i);
        if (check_stage(35, off, row, w)) return 1;
    }
    printf("%d cases pass\n", cases);
    return 0;
}
