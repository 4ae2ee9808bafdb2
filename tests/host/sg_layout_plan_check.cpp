// sg_layout_plan_check.cpp -- the host arithmetic of the stochastic graph's device build (csrc/sg_layout_plan.h) against
// a walk of the layout.  walk() lays a list of in-degrees out one row after the other, the way DESIGN.md section 4 and
// sg_create_impl state it: a running count of full pieces, one segment counter per remainder class, the classes from 6
// down to 0 with a new piece whenever a class's counter fills one, a running pa behind the three slots of every row (for
// a shard's handle too: the area from the degrees over all shards, the pieces from the shard's own).  The
// header's closed forms must give the same numbers from the eight totals alone, and every graph's figures are also
// literals worked out by hand.  The refusals and the small rules stand against literals.  Stand-alone, so that it runs
// under a host sanitizer:
//   g++ -std=c++17 -fsanitize=address,undefined -I locations-recommender_amd/csrc tests/host/sg_layout_plan_check.cpp
// Prints the number of cases and returns 0, or the first failed check and 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sg_layout_plan.h"

using namespace locrec;

static long cases = 0;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        ++cases;                                                                                     \
        if (!(cond)) {                                                                               \
            std::fprintf(stderr, "%s:%d: %s fails (check %ld)\n", __FILE__, __LINE__, #cond, cases); \
            std::exit(1);                                                                            \
        }                                                                                            \
    } while (0)

// ---- the walk -------------------------------------------------------------------------------------------------------

struct Row {
    int degree = 0, nfull = 0, rem = 0, cls = -1;
    int area_degree = 0;      // what decides the row's area: the degree itself, on a shard the degree over all shards
    int64_t full_begin = 0;   // first full piece
    int64_t rem_part = -1;    // the segment of the remainder, -1 without one
    int64_t rem_slot0 = -1;   // absolute slot of remainder element 0
    int64_t long_begin = -1;  // first partial slot of a row of the long area
};

struct Walk {
    std::vector<Row> rows;  // in live order
    int32_t T = 0, n_short = 0, wave_rows = 0;
    int32_t rows_of_class[7] = {0, 0, 0, 0, 0, 0, 0};
    int64_t nfull_total = 0, full_before_short = 0, np = 0, npart = 0, pa = 0;
    int64_t piece_begin[7], part_begin[7];
};

// degrees: the in-degree of every vertex, ascending vertex; a vertex without inbound edges is not a row.  A shard's
// handle: `degrees` count the shard's own edges and all_degrees the edges of all shards - a vertex is a row, and a row
// of the long area, by all_degrees, while its pieces follow degrees (which may be 0)
static Walk walk(const std::vector<int> &degrees, const std::vector<int> &all_degrees)
{
    Walk w;
    // live order: rows with at most two full pieces (of 256 slots) first, ascending vertex inside each kind
    for (int pass = 0; pass < 2; ++pass) {
        for (size_t v = 0; v < degrees.size(); ++v)
            if (all_degrees[v] > 0 && (all_degrees[v] / 256 <= 2) == (pass == 0)) {
                Row r;
                r.degree = degrees[v];
                r.area_degree = all_degrees[v];
                w.rows.push_back(r);
            }
        if (pass == 0) w.n_short = (int32_t)w.rows.size();
    }
    w.T = (int32_t)w.rows.size();
    // full pieces in row order; a remainder takes the smallest segment of 4 << c slots that holds it
    for (int32_t l = 0; l < w.T; ++l) {
        Row &r = w.rows[(size_t)l];
        if (l == w.n_short) w.full_before_short = w.nfull_total;
        r.nfull = r.degree / 256;
        r.rem = r.degree % 256;
        r.full_begin = w.nfull_total;
        w.nfull_total += r.nfull;
        if (r.rem > 0) {
            r.cls = 0;
            while ((4 << r.cls) < r.rem) ++r.cls;
            ++w.rows_of_class[r.cls];
        }
        if (r.nfull > 8) ++w.wave_rows;
    }
    if (w.n_short == w.T) w.full_before_short = w.nfull_total;
    // remainder pieces behind the full ones, class 6 down to 0; a piece of class c has 64 >> c segments
    w.np = w.npart = w.nfull_total;
    for (int c = 6; c >= 0; --c) {
        const int per = 64 >> c;
        w.piece_begin[c] = w.np;
        w.part_begin[c] = w.npart;
        int64_t used = 0, piece = -1;
        for (Row &r : w.rows) {
            if (r.cls != c) continue;
            if (used % per == 0) {  // the class's last piece is full (or there is none yet): a new one
                piece = w.np++;
                w.npart += per;
            }
            r.rem_part = w.part_begin[c] + used;
            r.rem_slot0 = piece * 256 + (used % per) * (4 << c);
            ++used;
        }
    }
    // partial slots: three per row, then a run of nfull + 1 for every row of the long area, in row order
    w.pa = 3 * (int64_t)w.T;
    for (int32_t l = w.n_short; l < w.T; ++l) {
        w.rows[(size_t)l].long_begin = w.pa;
        w.pa += w.rows[(size_t)l].nfull + 1;
    }
    return w;
}

// the figures of a graph worked out by hand
struct Expect {
    int32_t T, n_short;
    int64_t nfull_total, np, npart, pa;
    int32_t long_base, wave_rows;
};

// the header's plan from the walk's totals, against the walk row by row and against the literals
static SgLayoutPlan check_graph(const std::vector<int> &degrees, const Expect &x, const std::vector<int> *all_degrees = nullptr)
{
    const Walk w = walk(degrees, all_degrees ? *all_degrees : degrees);
    CHECK(w.T == x.T && w.n_short == x.n_short && w.nfull_total == x.nfull_total && w.wave_rows == x.wave_rows);
    CHECK(w.np == x.np && w.npart == x.npart && w.pa == x.pa);
    const SgLayoutPlan pl = sg_layout_plan(w.rows_of_class, (int32_t)w.nfull_total, (int32_t)w.full_before_short, w.T, w.n_short);
    CHECK(pl.status == SgPlanStatus::ok);
    CHECK(pl.np == x.np && pl.npart == x.npart && pl.pa == x.pa && pl.long_base == x.long_base);
    CHECK(pl.nfull_total == x.nfull_total && pl.T == x.T && pl.n_short == x.n_short);
    CHECK(pl.nslots() == x.np * 256 && pl.long_area_rows() == x.T - x.n_short);
    for (int c = 0; c < 7; ++c) CHECK(pl.piece_begin[c] == w.piece_begin[c] && pl.part_begin[c] == w.part_begin[c]);
    int32_t wave_rows = 0;
    for (int32_t l = 0; l < w.T; ++l) {
        const Row &r = w.rows[(size_t)l];
        CHECK(sg_in_long_area(r.area_degree) == (l >= w.n_short));
        if (r.rem > 0) CHECK(sg_remainder_class(r.rem) == r.cls);
        if (l >= w.n_short) CHECK(sg_long_begin(pl.long_base, (int32_t)r.full_begin, l) == r.long_begin);
        wave_rows += sg_wave_row(r.nfull) ? 1 : 0;
        // the walk's own sanity: every slot of the remainder lies inside the layout
        if (r.rem > 0) CHECK(r.rem_part < w.npart && r.rem_slot0 + r.rem <= w.np * 256);
    }
    CHECK(wave_rows == x.wave_rows);
    return pl;
}

// ---- graphs ---------------------------------------------------------------------------------------------------------

static void check_no_live_row()
{
    SgLayoutPlan pl = check_graph({}, {0, 0, 0, 0, 0, 0, 0, 0});
    for (int c = 0; c < 7; ++c) CHECK(pl.piece_begin[c] == 0 && pl.part_begin[c] == 0);
    pl = check_graph({0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0});  // vertices without inbound edges
    CHECK(pl.np == 0 && pl.nslots() == 0);
}

// one row of every degree at which its class, its full pieces or its area changes
static void check_single_rows()
{
    struct {
        int degree, cls;  // -1: no remainder
        Expect x;
    } const rows[] = {
        // both ends of every remainder class: no full piece, one remainder piece of 64 >> c segments
        {1, 0, {1, 1, 0, 1, 64, 3, 2, 0}},    {4, 0, {1, 1, 0, 1, 64, 3, 2, 0}},   {5, 1, {1, 1, 0, 1, 32, 3, 2, 0}},
        {8, 1, {1, 1, 0, 1, 32, 3, 2, 0}},    {9, 2, {1, 1, 0, 1, 16, 3, 2, 0}},   {16, 2, {1, 1, 0, 1, 16, 3, 2, 0}},
        {17, 3, {1, 1, 0, 1, 8, 3, 2, 0}},    {32, 3, {1, 1, 0, 1, 8, 3, 2, 0}},   {33, 4, {1, 1, 0, 1, 4, 3, 2, 0}},
        {64, 4, {1, 1, 0, 1, 4, 3, 2, 0}},    {65, 5, {1, 1, 0, 1, 2, 3, 2, 0}},   {128, 5, {1, 1, 0, 1, 2, 3, 2, 0}},
        {129, 6, {1, 1, 0, 1, 1, 3, 2, 0}},   {255, 6, {1, 1, 0, 1, 1, 3, 2, 0}},
        // no remainder; the first full piece plus one
        {256, -1, {1, 1, 1, 1, 1, 3, 1, 0}},  {257, 0, {1, 1, 1, 2, 65, 3, 1, 0}},
        // two full pieces keep the row short, three move it to the long area: a run of nfull + 1 slots behind 3T
        {767, 6, {1, 1, 2, 3, 3, 3, 0, 0}},   {768, -1, {1, 0, 3, 3, 3, 7, 3, 0}},
        // eight full pieces are summed by one thread, more by a whole wave
        {2048, -1, {1, 0, 8, 8, 8, 12, 3, 0}}, {2304, -1, {1, 0, 9, 9, 9, 13, 3, 1}}, {2560, -1, {1, 0, 10, 10, 10, 14, 3, 1}},
    };
    for (const auto &r : rows) {
        check_graph({r.degree}, r.x);
        const int rem = r.degree % 256;
        CHECK((rem > 0) == (r.cls >= 0));
        if (rem > 0) CHECK(sg_remainder_class(rem) == r.cls);
    }
    CHECK(!sg_in_long_area(767) && sg_in_long_area(768) && !sg_wave_row(8) && sg_wave_row(9));
}

// exactly 64 >> c rows of class c fill one piece; one more opens a piece with a single owned segment
static void check_full_class_pieces()
{
    const int low_end[7] = {1, 5, 9, 17, 33, 65, 129};
    const int per_piece[7] = {64, 32, 16, 8, 4, 2, 1};
    for (int c = 0; c < 7; ++c) {
        const int32_t n = per_piece[c];
        check_graph(std::vector<int>((size_t)n, low_end[c]), {n, n, 0, 1, n, 3 * (int64_t)n, 2 * n, 0});
        check_graph(std::vector<int>((size_t)n + 1, low_end[c]), {n + 1, n + 1, 0, 2, 2 * (int64_t)n, 3 * (int64_t)n + 3, 2 * n + 2, 0});
    }
}

static void check_mixed_graphs()
{
    // only short rows.  1: class 0; 300 = 256 + 44: class 4; 600 = 512 + 88: class 5; 256; 7: class 1
    SgLayoutPlan pl = check_graph({1, 300, 600, 256, 7}, {5, 5, 4, 8, 106, 15, 6, 0});
    const int32_t short_piece[7] = {7, 6, 6, 6, 5, 4, 4}, short_part[7] = {42, 10, 10, 10, 6, 4, 4};
    for (int c = 0; c < 7; ++c) CHECK(pl.piece_begin[c] == short_piece[c] && pl.part_begin[c] == short_part[c]);
    // only long rows.  768 = 3 * 256; 1000 = 768 + 232: class 6; 2305 = 9 * 256 + 1: class 0, a whole wave's row
    pl = check_graph({768, 1000, 2305}, {3, 0, 15, 17, 80, 27, 9, 1});
    const int32_t long_piece[7] = {16, 16, 16, 16, 16, 16, 15}, long_part[7] = {16, 16, 16, 16, 16, 16, 15};
    for (int c = 0; c < 7; ++c) CHECK(pl.piece_begin[c] == long_piece[c] && pl.part_begin[c] == long_part[c]);
    CHECK(sg_long_begin(pl.long_base, 0, 0) == 9 && sg_long_begin(pl.long_base, 3, 1) == 13 && sg_long_begin(pl.long_base, 6, 2) == 17);
    // the two kinds alternating: live order 10, 256, 513 | 800, 3000, 769; full pieces 0 1 2 | 3 11 3; classes 2 - 0 | 3 6 0
    pl = check_graph({10, 800, 256, 3000, 513, 769}, {6, 3, 20, 24, 109, 38, 12, 1});
    const int32_t mixed_piece[7] = {23, 23, 22, 21, 21, 21, 20}, mixed_part[7] = {45, 45, 29, 21, 21, 21, 20};
    for (int c = 0; c < 7; ++c) CHECK(pl.piece_begin[c] == mixed_piece[c] && pl.part_begin[c] == mixed_part[c]);
    CHECK(sg_long_begin(pl.long_base, 3, 3) == 18 && sg_long_begin(pl.long_base, 6, 4) == 22 && sg_long_begin(pl.long_base, 17, 5) == 34);
    // DESIGN.md's hand-checked graph: classes 77 / 2 / 2 / 2 / 2 / 2 / 4 and 32 full pieces make 43 pieces, 226 parts
    const int32_t by_class[7] = {77, 2, 2, 2, 2, 2, 4};
    pl = sg_layout_plan(by_class, 32, 0, 94, 90);
    CHECK(pl.status == SgPlanStatus::ok && pl.np == 43 && pl.npart == 226);
}

// a shard's handle: the area from the degrees over all shards, the pieces from the shard's own
static void check_sharded_totals()
{
    // all: 10, 800, 256, 3000, 513, 769 -> live order 10, 256, 513 | 800, 3000, 769 (as in the mixed graph above).
    // This shard holds 4, 300, 0, 2600, 513, 100 of them: full pieces 0 0 2 | 1 10 0, classes 0 - 0 | 4 4 5; a row
    // without an edge here (256) and long-area rows with one full piece or none (800, 769) keep their places.
    const std::vector<int> all = {10, 800, 256, 3000, 513, 769}, own = {4, 300, 0, 2600, 513, 100};
    // pieces: 13 full + class 5: 1, class 4: 1, class 0: 1 = 16; parts 13 + 2 + 4 + 64 = 83; pa = 18 + (1+1) + (10+1) + (0+1)
    SgLayoutPlan pl = check_graph(own, {6, 3, 13, 16, 83, 32, 13, 1}, &all);
    const int32_t piece[7] = {15, 15, 15, 15, 14, 13, 13}, part[7] = {19, 19, 19, 19, 15, 13, 13};
    for (int c = 0; c < 7; ++c) CHECK(pl.piece_begin[c] == piece[c] && pl.part_begin[c] == part[c]);
    CHECK(sg_long_begin(pl.long_base, 2, 3) == 18 && sg_long_begin(pl.long_base, 3, 4) == 20 && sg_long_begin(pl.long_base, 13, 5) == 31);
    // a shard without a single edge of the graph: every row keeps its three slots, the long area one slot per row
    const std::vector<int> nothing = {0, 0, 0, 0, 0, 0};
    pl = check_graph(nothing, {6, 3, 0, 0, 0, 21, 15, 0}, &all);
    CHECK(sg_long_begin(pl.long_base, 0, 3) == 18 && sg_long_begin(pl.long_base, 0, 5) == 20);
    // the other way round does not occur (a shard's degree never exceeds the total), and the whole graph is its own shard
    check_graph(all, {6, 3, 20, 24, 109, 38, 12, 1}, &all);
}

// ---- the refusals, from totals alone --------------------------------------------------------------------------------

static void check_refusals()
{
    const int32_t none[7] = {0, 0, 0, 0, 0, 0, 0};
    // np one below 2^31 / 256 = 8388608, and at it: by full pieces, then by the last remainder piece
    SgLayoutPlan pl = sg_layout_plan(none, 8388607, 0, 1, 0);
    CHECK(pl.status == SgPlanStatus::ok && pl.np == 8388607 && pl.npart == 8388607 && pl.pa == 8388611);
    CHECK(pl.piece_begin[0] == 8388607 && pl.piece_begin[6] == 8388607 && pl.nslots() == 2147483392);
    pl = sg_layout_plan(none, 8388608, 0, 1, 0);
    CHECK(pl.status == SgPlanStatus::too_many_slots && pl.np == 8388608);
    const int32_t one_big[7] = {0, 0, 0, 0, 0, 0, 1}, two_big[7] = {0, 0, 0, 0, 0, 0, 2};
    pl = sg_layout_plan(one_big, 8388606, 0, 1, 0);
    CHECK(pl.status == SgPlanStatus::ok && pl.np == 8388607 && pl.piece_begin[6] == 8388606 && pl.piece_begin[5] == 8388607);
    pl = sg_layout_plan(two_big, 8388606, 0, 2, 0);
    CHECK(pl.status == SgPlanStatus::too_many_slots && pl.np == 8388608);
    // the totals are int32: their sums are taken in 64 bits.  Every total at INT32_MAX:
    // pieces 2^25 + 2^26 + ... + 2^30 + (2^31 - 1), parts 6 * 2^31 + (2^31 - 1), both on top of 2^31 - 1 full pieces
    const int32_t all_max[7] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX};
    pl = sg_layout_plan(all_max, INT32_MAX, 0, INT32_MAX, 0);
    CHECK(pl.status == SgPlanStatus::too_many_slots && pl.np == 6408896510 && pl.npart == 17179869182 && pl.pa == 10737418235);
    // pa one below 2^30: 357,913,941 rows of class 0, all short (3T = 2^30 - 1; 3T does not fit 32 bits)
    const int32_t small_rows[7] = {357913941, 0, 0, 0, 0, 0, 0};
    pl = sg_layout_plan(small_rows, 0, 0, 357913941, 357913941);
    CHECK(pl.status == SgPlanStatus::ok && pl.np == 5592406 && pl.npart == 357913984 && pl.pa == 1073741823);
    CHECK(pl.long_base == 715827882 && pl.part_begin[0] == 0 && pl.piece_begin[0] == 0);
    // ... and at it: 357,913,939 such rows and one row of three full pieces in the long area (3T + 3 + 1 = 2^30)
    const int32_t fewer_rows[7] = {357913939, 0, 0, 0, 0, 0, 0};
    pl = sg_layout_plan(fewer_rows, 3, 0, 357913940, 357913939);
    CHECK(pl.status == SgPlanStatus::too_many_partials && pl.np == 5592409 && pl.pa == 1073741824);
    // both: the slot ids are refused first
    pl = sg_layout_plan(small_rows, 8388608, 0, 357913942, 357913942);
    CHECK(pl.status == SgPlanStatus::too_many_slots);
}

// ---- the smaller rules ----------------------------------------------------------------------------------------------

static void check_small_rules()
{
    // the id table: id_span < 8 * ne + 2^20, unsigned
    CHECK(sg_dense_ids(0, 1) && sg_dense_ids(1048583, 1) && !sg_dense_ids(1048584, 1));
    CHECK(sg_dense_ids(17180917751ull, 2147483647) && !sg_dense_ids(17180917752ull, 2147483647));
    const uint64_t whole_range = (uint64_t)INT64_MAX - (uint64_t)INT64_MIN;  // ids from INT64_MIN to INT64_MAX
    CHECK(whole_range == 18446744073709551615ull && !sg_dense_ids(whole_range, 1) && !sg_dense_ids(whole_range, 2147483647));
    // 16-bit columns: T + 2 <= 65536
    CHECK(sg_use16(0) && sg_use16(65533) && sg_use16(65534) && !sg_use16(65535) && !sg_use16(INT32_MAX));
    CHECK(!sg_dict_fits(0) && sg_dict_fits(1) && sg_dict_fits(8192) && !sg_dict_fits(8193));
    // radix bits that hold every key below n (never fewer than one)
    CHECK(sg_radix_bits(1) == 1 && sg_radix_bits(2) == 1 && sg_radix_bits(3) == 2 && sg_radix_bits(4) == 2 && sg_radix_bits(5) == 3);
    CHECK(sg_radix_bits(2147483646) == 31);
    // pieces per wave of 8 * ncu waves: need = 4, 5, 12, 13 with one compute unit; none without a compute unit
    CHECK(sg_persist_pw(32, 1) == 4 && sg_persist_pw(33, 1) == 12 && sg_persist_pw(96, 1) == 12 && sg_persist_pw(97, 1) == 0);
    CHECK(sg_persist_pw(0, 1) == 4 && sg_persist_pw(1, 0) == 0 && sg_persist_pw(0, 0) == 0 && sg_persist_pw(8192, 256) == 4);
    // the byte figures, on DESIGN.md's hand-checked graph (43 pieces, 226 parts, 94 rows) and past 32 bits
    CHECK(sg_layout_bytes(43, 94) == 133568 && sg_layout_bytes(8388607, 0) == 25836909560);
    CHECK(sg_device_sweep_bytes(43, 226, 94, true, true) == 49496 && sg_device_sweep_bytes(43, 226, 94, true, false) == 115544);
    CHECK(sg_device_sweep_bytes(43, 226, 94, false, true) == 71512 && sg_device_sweep_bytes(43, 226, 94, false, false) == 137560);
}

int main()
{
    check_no_live_row();
    check_single_rows();
    check_full_class_pieces();
    check_mixed_graphs();
    check_sharded_totals();
    check_refusals();
    check_small_rules();
    std::printf("%ld cases pass\n", cases);
    return 0;
}
