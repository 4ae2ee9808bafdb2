// knn_ht_order_check.cpp -- the element order of the head / tail image (csrc/knn_ht_order.h) on literal lane groups and on
// random ones: every row keeps its (index, value) pairs, all of them in front of the slice's count, padding words are
// value 0 and name a row that is read at their position anyway, words at and behind the count and the stand-ins of wide
// rows are untouched, the modelled cycles never exceed the ascending order's, reach the lower bound max(count, distinct
// rows of the busiest slot) where the case says that it is attainable, and equal an exhaustive search on groups small
// enough for one.  The same input gives the same image twice, through the plain accessor and through the builders'
// (HtOrderSlice, every lane group of a slice).  Stand-alone, so that it also runs under a host sanitizer:
//   g++ -std=c++17 -fsanitize=address,undefined -I locations-recommender_amd/csrc tests/host/knn_ht_order_check.cpp
// Prints the number of cases and returns 0, or the first failed check and 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "knn_ht_order.h"

using namespace locrec;

static long cases = 0;

#define CHECK(cond)                                                                                 \
    do {                                                                                            \
        if (!(cond)) {                                                                              \
            std::fprintf(stderr, "%s:%d: %s fails (case %ld)\n", __FILE__, __LINE__, #cond, cases); \
            std::exit(1);                                                                           \
        }                                                                                           \
    } while (0)

typedef std::vector<std::pair<int, int>> Row;  // (index, value), ascending index

struct Plain {  // [member][position], `cap` words per member
    std::vector<uint32_t> w;
    int cap;
    uint32_t get(int i, int pos) const { return w.at((size_t)i * cap + pos); }
    void set(int i, int pos, uint32_t v) { w.at((size_t)i * cap + pos) = v; }
};

static Plain ascending(const std::vector<Row> &rows, int cap)
{
    Plain p{std::vector<uint32_t>((size_t)16 * cap, 0u), cap};
    for (int i = 0; i < 16; ++i)
        for (size_t j = 0; j < rows[i].size(); ++j) p.set(i, (int)j, ((uint32_t)rows[i][j].second << 16) | ((uint32_t)rows[i][j].first << 4));
    return p;
}

static int lower_bound_of(const std::vector<Row> &rows, int cnt, uint32_t blank)
{
    std::set<int> per_slot[16];
    for (int i = 0; i < 16; ++i)
        for (const auto &e : rows[i]) per_slot[e.first & 15].insert(e.first);
    if (blank & 0xFFFFu) per_slot[0].insert(0);
    int lb = cnt;
    for (int s = 0; s < 16; ++s) lb = std::max(lb, (int)per_slot[s].size());
    return lb;
}

// Runs the routine on the group and checks everything that holds for every group; returns the cycles.
static int run(const std::vector<Row> &rows_in, int cnt, uint32_t blank, bool attain_lb, int *asc_out = nullptr)
{
    ++cases;
    std::vector<Row> rows = rows_in;
    rows.resize(16);
    const int cap = cnt + 5;
    for (int i = 0; i < 16; ++i) {
        CHECK((int)rows[i].size() <= cnt);
        if ((blank >> i) & 1u) CHECK(rows[i].empty());
    }
    const Plain asc = ascending(rows, cap);
    Plain a = asc, b = asc;
    ht_order_group(a, cnt, blank);
    ht_order_group(b, cnt, blank);
    CHECK(a.w == b.w);  // deterministic
    for (int i = 0; i < 16; ++i) {
        std::multiset<std::pair<int, int>> have, want(rows[i].begin(), rows[i].end());
        for (int t = 0; t < cnt; ++t) {
            const uint32_t w = a.get(i, t);
            if ((blank >> i) & 1u) {
                CHECK(w == 0u);
            } else if (ht_order_is_pad(w)) {
                CHECK((w & 0xFu) == 0u);
                bool read_anyway = ht_order_row(w) == 0 && (blank & 0xFFFFu);
                bool any = (blank & 0xFFFFu) != 0;
                for (int k = 0; k < 16; ++k)
                    if (!ht_order_is_pad(a.get(k, t))) {
                        any = true;
                        read_anyway = read_anyway || ht_order_row(a.get(k, t)) == ht_order_row(w);
                    }
                CHECK(w == 0u || (any && read_anyway));  // (all zero: the ascending order was kept)
            } else {
                have.insert({ht_order_row(w), (int)(w >> 16)});
            }
        }
        CHECK(have == want);
        for (int t = cnt; t < cap; ++t) CHECK(a.get(i, t) == 0u);
    }
    const int before = ht_order_cycles(asc, cnt), after = ht_order_cycles(a, cnt);
    CHECK(after <= before);
    CHECK(after >= lower_bound_of(rows, cnt, blank) || cnt == 0);
    if (attain_lb) CHECK(after == lower_bound_of(rows, cnt, blank));
    if (asc_out) *asc_out = before;

    // the builders' accessor: the group as lane group g of a slice image, all four g
    for (int g = 0; g < kHtOrderGroups; ++g) {
        std::vector<uint32_t> slice((size_t)((cnt + 3) / 4 + 1) * 256, 0u);
        HtOrderSlice img{slice.data(), g};
        for (int i = 0; i < 16; ++i)
            for (int t = 0; t < cnt; ++t) img.set(i, t, asc.get(i, t));
        ht_order_group(img, cnt, blank);
        std::set<int> lanes;
        for (int i = 0; i < 16; ++i) {
            lanes.insert(ht_order_lane(g, i));
            for (int t = 0; t < cnt; ++t) CHECK(img.get(i, t) == a.get(i, t));
        }
        CHECK(lanes.size() == 16);
        long nonzero = 0, expect = 0;
        for (uint32_t w : slice) nonzero += w != 0u;
        for (int i = 0; i < 16; ++i)
            for (int t = 0; t < cnt; ++t) expect += a.get(i, t) != 0u;
        CHECK(nonzero == expect);  // (no word of another lane group, and none behind the count, was written)
    }
    return after;
}

// exhaustive optimum of a small group: every lane's elements in every arrangement over [0, cnt), padding free
static int brute(const std::vector<Row> &rows, int cnt)
{
    const int nl = (int)rows.size();
    std::vector<std::vector<std::vector<int>>> arr((size_t)nl);  // per lane: arrangements = row per position, -1 = padding
    for (int i = 0; i < nl; ++i) {
        std::vector<int> slots((size_t)cnt, -1);
        for (size_t j = 0; j < rows[i].size(); ++j) slots[j] = rows[i][j].first;
        std::sort(slots.begin(), slots.end());
        do arr[i].push_back(slots); while (std::next_permutation(slots.begin(), slots.end()));
    }
    int best = 1 << 30;
    std::vector<size_t> pick((size_t)nl, 0);
    for (;;) {
        int total = 0;
        for (int t = 0; t < cnt; ++t) {
            std::set<int> per_slot[16];
            for (int i = 0; i < nl; ++i)
                if (arr[i][pick[i]][t] >= 0) per_slot[arr[i][pick[i]][t] & 15].insert(arr[i][pick[i]][t]);
            int worst = 1;
            for (int s = 0; s < 16; ++s) worst = std::max(worst, (int)per_slot[s].size());
            total += worst;
        }
        best = std::min(best, total);
        int i = 0;
        while (i < nl && ++pick[i] == arr[i].size()) pick[i++] = 0;
        if (i == nl) break;
    }
    return best;
}

static Row row_of(std::initializer_list<int> idx)
{
    Row r;
    int v = 1;
    for (int i : idx) r.push_back({i, v++ % 7 + 1});
    return r;
}

int main()
{
    {  // the lanes of the four groups partition the slice as the LDS serves it
        std::set<int> all;
        for (int g = 0; g < 4; ++g)
            for (int i = 0; i < 16; ++i) all.insert(ht_order_lane(g, i));
        CHECK(all.size() == 64 && *all.begin() == 0 && *all.rbegin() == 63);
        CHECK(ht_order_lane(0, 4) == 12 && ht_order_lane(0, 8) == 20 && ht_order_lane(0, 15) == 27);
        CHECK(ht_order_lane(1, 0) == 4 && ht_order_lane(1, 8) == 16 && ht_order_lane(1, 12) == 28 && ht_order_lane(3, 15) == 63);
        CHECK(ht_order_word(5, 6) == 256 + 5 * 4 + 2);
    }
    std::mt19937 rng(12345);
    // ---- all 16 rows of length cnt: no padding anywhere, only permutations
    for (int cnt : {1, 4, 5, 17}) {
        std::vector<Row> rows(16);
        for (int i = 0; i < 16; ++i) {
            std::vector<int> pool(64);
            for (int k = 0; k < 64; ++k) pool[k] = k;
            std::shuffle(pool.begin(), pool.end(), rng);
            pool.resize((size_t)cnt);
            std::sort(pool.begin(), pool.end());
            for (int k : pool) rows[i].push_back({k, 1 + k % 5});
        }
        run(rows, cnt, 0u, false);
    }
    {  // rotations of one set: ascending puts 16 different rows of 4 slots side by side, a diagonal order is conflict-free
        std::vector<Row> rows(16);
        for (int i = 0; i < 16; ++i) rows[i] = row_of({i, 16 + i, 32 + i, 48 + i});
        CHECK(run(rows, 4, 0u, true) == 4);
        for (int i = 0; i < 16; ++i) rows[i] = row_of({0 + (i & 3), 16 + (i & 3), 32 + (i & 3), 48 + (i & 3)});
        int asc = 0;
        CHECK(run(rows, 4, 0u, true, &asc) == 4 && asc == 4);  // (4 distinct rows of a slot per position, but 4 slots: 1 each)
    }
    // ---- empty rows, cnt = 0
    run(std::vector<Row>(16), 0, 0u, false);
    run(std::vector<Row>(16), 3, 0u, true);
    run({row_of({3}), {}, row_of({19}), {}}, 1, 0u, false);   // (two rows of slot 3, no room to move: 2 cycles)
    run({row_of({3}), {}, row_of({19}), {}}, 2, 0u, true);    // one of them waits a position
    // ---- cnt = 1, 4, 5, 17 with short rows among long ones
    for (int cnt : {1, 4, 5, 17})
        for (int rep = 0; rep < 20; ++rep) {
            std::vector<Row> rows(16);
            for (int i = 0; i < 16; ++i) {
                const int len = i == 0 ? cnt : (int)(rng() % (unsigned)(cnt + 1));
                std::set<int> s;
                while ((int)s.size() < len) s.insert((int)(rng() % 40u));
                for (int k : s) rows[i].push_back({k, 1 + (int)(rng() % 200u)});
            }
            run(rows, cnt, 0u, false);
        }
    {  // ---- 16 lanes holding the same index: one read serves them all
        std::vector<Row> rows(16, row_of({7}));
        CHECK(run(rows, 1, 0u, true) == 1);
        rows.assign(16, row_of({7, 23, 39}));
        CHECK(run(rows, 3, 0u, true) == 3);
        for (int i = 0; i < 16; ++i) rows[i] = i % 2 ? row_of({7, 23}) : row_of({23});  // the short rows must line up with the long
        int asc = 0;
        CHECK(run(rows, 2, 0u, true, &asc) == 2 && asc == 3);
    }
    {  // ---- 17 distinct indices of one slot: 17 cycles whatever the order; ascending pays 18 (its zero words read row 0)
        std::vector<Row> rows(16);
        for (int i = 0; i < 16; ++i) rows[i] = row_of({16 * (i + 1)});
        rows[0] = row_of({16, 16 * 17});
        int asc = 0;
        CHECK(run(rows, 2, 0u, true, &asc) == 17 && asc == 18);
    }
    {  // ---- a category family of 20 dimensions: 16 .. 19 share the slots of 0 .. 3
        std::vector<Row> rows(16);
        rows[0] = row_of({0, 5});
        rows[1] = row_of({5, 16});
        rows[2] = row_of({1, 17});
        rows[3] = row_of({1, 6});
        rows[4] = row_of({6, 17});
        int asc = 0;
        CHECK(run(rows, 2, 0u, true, &asc) == 2 && asc > 2);
        for (int rep = 0; rep < 50; ++rep) {
            int cnt = 0;
            for (int i = 0; i < 16; ++i) {
                rows[i].clear();
                const int len = 1 + (int)(rng() % 9u);
                std::set<int> s;
                while ((int)s.size() < len) s.insert((int)(rng() % 20u));
                for (int k : s) rows[i].push_back({k, 1 + (int)(rng() % 29u)});
                cnt = std::max(cnt, len);
            }
            run(rows, cnt, 0u, false);
        }
    }
    {  // ---- a wide row's stand-in stays blank and reads row 0: index 16 collides with it, index 0 does not
        std::vector<Row> rows(16);
        rows[1] = row_of({0, 16});
        rows[2] = row_of({0});
        rows[3] = row_of({16});
        run(rows, 2, 1u << 0 | 1u << 9, false);
        rows[1] = row_of({0, 3});
        rows[3] = row_of({3});
        CHECK(run(rows, 2, 1u << 0, true) == 2);
    }
    // ---- small groups against an exhaustive search
    for (int rep = 0; rep < 60; ++rep) {
        const int nl = 2 + (int)(rng() % 3u), cnt = 2 + (int)(rng() % 3u);
        std::vector<Row> rows((size_t)nl);
        bool full = false;
        for (int i = 0; i < nl; ++i) {
            const int len = (i == 0 && !full) ? cnt : (int)(rng() % (unsigned)(cnt + 1));
            full = full || len == cnt;
            std::set<int> s;
            while ((int)s.size() < len) s.insert((int)(rng() % 4u) * 16 + (int)(rng() % 2u));  // two slots, four rows each
            for (int k : s) rows[i].push_back({k, 1 + (int)(rng() % 9u)});
        }
        const int opt = brute(rows, cnt);
        const int got = run(rows, cnt, 0u, false);
        CHECK(got >= opt);
        CHECK(got <= opt + 1);  // the search is a heuristic: within one cycle of the optimum on these
    }
    {  // ---- Zipf-like rows, the shape of the real image: a figure, and the properties
        long asc_total = 0, new_total = 0, reads = 0;
        for (int rep = 0; rep < 300; ++rep) {
            std::vector<Row> rows(16);
            int cnt = 0;
            for (int i = 0; i < 16; ++i) {
                const int len = 8 + (int)(rng() % 9u);
                std::set<int> s;
                while ((int)s.size() < len) {
                    const double u = (double)(rng() % 1000000u + 1u) / 1000001.0;
                    s.insert((int)std::min(511.0, 1.0 / (u * u) - 1.0));
                }
                for (int k : s) rows[i].push_back({k, 1 + (int)(rng() % 5u)});
                cnt = std::max(cnt, len);
            }
            int asc = 0;
            new_total += run(rows, cnt, 0u, false, &asc);
            asc_total += asc;
            reads += cnt;
        }
        std::printf("zipf groups: %.3f cycles per read ascending, %.3f ordered\n", (double)asc_total / (double)reads,
                    (double)new_total / (double)reads);
        CHECK((new_total - reads) * 2 <= (asc_total - reads));  // at least half of the conflict cycles go
    }
    std::printf("knn_ht_order_check: %ld cases pass\n", cases);
    return 0;
}
