// knn_format_plan_check.cpp -- the decision that selects a KNN index's format and kernel path (csrc/knn_format_plan.h,
// taken by both builders) on both sides of every limit of DESIGN.md's "Numeric limits" table.  Every expected value is a
// literal worked out from that table, never a second copy of the expressions.  Stand-alone, so that it runs under a host
// sanitizer:
//   g++ -std=c++17 -fsanitize=address,undefined -I locations-recommender_amd/csrc tests/host/knn_format_plan_check.cpp
// Prints the number of cases and returns 0, or the first failed check and 1.
#include <cstdio>
#include <cstdlib>

#include "knn_format_plan.h"

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

// 1000 persons, 100 places, 10 categories, small integer counts: PACK16 with the head / tail form
static KnnFormatInput base()
{
    KnnFormatInput in;
    in.n = 1000;
    in.p_dim = 100;
    in.c_dim = 10;
    in.all = {5.0, 5.0, 100.0, 100.0};
    in.narrow = in.all;
    in.lim = {512, 16, 64, 4096, 16384};  // cfg::kHtHead, kHtQt, kHtCatRows, kPopTable, kDirectMaxBytes (knn_index.h)
    return in;
}

// base() with one row-wide maximum raised; the rows that are not wide keep the small maxima
static KnnFormatInput with_max(double KnnMaxima::*which, double v)
{
    KnnFormatInput in = base();
    in.all.*which = v;
    return in;
}

static void check_base()
{
    const KnnFormatInput in = base();
    CHECK(!knn_row_fallback_eligible(in));
    const KnnFormatPlan pl = knn_format_plan(in, 0);
    CHECK(pl.n_wide == 0 && pl.p_vbits == 24 && pl.c_vbits == 24);
    CHECK(pl.packed && pl.pack16 && pl.want_ht && pl.use_pop);
    CHECK(pl.ht_h == 100 && pl.pop_h == 100 && pl.key_h == 100);
}

// a count of 256 or a row sum of squares of 65536, in either family, makes a wide row
static void check_any_wide()
{
    double KnnMaxima::*const value[2] = {&KnnMaxima::pvmax, &KnnMaxima::cvmax};
    double KnnMaxima::*const sum[2] = {&KnnMaxima::pss, &KnnMaxima::css};
    for (int f = 0; f < 2; ++f) {
        for (int k = 0; k < 2; ++k) {
            double KnnMaxima::*const m = k == 0 ? value[f] : sum[f];
            const double legal = k == 0 ? 255.0 : 65535.0, wide = k == 0 ? 256.0 : 65536.0;
            const KnnFormatInput below = with_max(m, legal);
            CHECK(!knn_row_fallback_eligible(below));
            const KnnFormatPlan pb = knn_format_plan(below, 3);  // (a count nobody made: not looked at)
            CHECK(pb.n_wide == 0 && pb.packed && pb.pack16 && pb.want_ht);
            const KnnFormatInput at = with_max(m, wide);
            CHECK(knn_row_fallback_eligible(at));
            // adopted: the non-wide maxima decide everything after it
            const KnnFormatPlan pa = knn_format_plan(at, 3);
            CHECK(pa.n_wide == 3 && pa.packed && pa.pack16 && pa.want_ht && pa.use_pop);
            // not adopted: the whole index is judged on the wide row
            KnnFormatInput off = at;
            off.sw.no_row_fallback = true;
            const KnnFormatPlan po = knn_format_plan(off, 3);
            CHECK(po.n_wide == 0 && po.packed && !po.want_ht);
            CHECK(po.pack16 == (k == 0));  // 256 < 65536 keeps PACK16, a sum of 65536 does not
        }
    }
    KnnFormatInput in = with_max(&KnnMaxima::pvmax, 300.0);
    in.narrow = {255.0, 255.0, 65535.0, 65535.0};
    const KnnFormatPlan pl = knn_format_plan(in, 1);
    CHECK(pl.n_wide == 1 && pl.packed && pl.pack16 && pl.want_ht);
}

static void check_eligibility()
{
    KnnFormatInput in = with_max(&KnnMaxima::pvmax, 256.0);
    CHECK(knn_row_fallback_eligible(in));
    in.n = (1 << 24) - 1;
    CHECK(knn_row_fallback_eligible(in) && knn_format_plan(in, 2).n_wide == 2);
    in.n = 1 << 24;
    CHECK(!knn_row_fallback_eligible(in) && knn_format_plan(in, 2).n_wide == 0);
    in = with_max(&KnnMaxima::pvmax, 256.0);
    in.c_dim = 64;
    CHECK(knn_row_fallback_eligible(in));
    in.c_dim = 65;
    CHECK(!knn_row_fallback_eligible(in) && knn_format_plan(in, 2).n_wide == 0);
    in = with_max(&KnnMaxima::pvmax, 256.0);
    in.p_dim = (1 << 20) - 2;
    CHECK(knn_row_fallback_eligible(in));
    in.p_dim = (1 << 20) - 1;
    CHECK(!knn_row_fallback_eligible(in) && knn_format_plan(in, 2).n_wide == 0);
    in = with_max(&KnnMaxima::pvmax, 256.0);
    in.integral = false;
    CHECK(!knn_row_fallback_eligible(in) && knn_format_plan(in, 2).n_wide == 0);
    bool KnnFormatSwitches::*const switches[4] = {&KnnFormatSwitches::force_generic, &KnnFormatSwitches::no_row_fallback,
                                                  &KnnFormatSwitches::no_pack16, &KnnFormatSwitches::no_ht};
    for (bool KnnFormatSwitches::*const sw : switches) {
        in = with_max(&KnnMaxima::pvmax, 256.0);
        in.sw.*sw = true;
        CHECK(!knn_row_fallback_eligible(in) && knn_format_plan(in, 2).n_wide == 0);
    }
}

// at most min(4096, max(256, n / 512)) wide rows, and fewer than n
static void check_cap()
{
    struct {
        int64_t n, kept, dropped;
    } const rows[] = {{300, 256, 257}, {131584, 257, 258}, {2097152, 4096, 4097}, {4194304, 4096, 4097}, {200, 199, 200}};
    for (const auto &r : rows) {
        KnnFormatInput in = with_max(&KnnMaxima::pss, 65536.0);
        in.n = r.n;
        const KnnFormatPlan kept = knn_format_plan(in, r.kept), dropped = knn_format_plan(in, r.dropped);
        CHECK(kept.n_wide == r.kept && kept.pack16 && kept.want_ht);
        CHECK(dropped.n_wide == 0 && !dropped.pack16 && !dropped.want_ht);
    }
    const KnnFormatPlan none = knn_format_plan(with_max(&KnnMaxima::pss, 65536.0), 0);
    CHECK(none.n_wide == 0 && !none.pack16);
}

static void check_vbits()
{
    struct {
        int32_t dim;
        int vbits;
    } const rows[] = {{1, 24}, {256, 24}, {257, 23}, {(1 << 20) - 2, 12}};
    for (const auto &r : rows) {
        KnnFormatInput in = base();
        in.p_dim = r.dim;
        CHECK(knn_format_plan(in, 0).p_vbits == r.vbits && knn_format_plan(in, 0).c_vbits == 24);
        in = base();
        in.c_dim = r.dim;
        CHECK(knn_format_plan(in, 0).c_vbits == r.vbits && knn_format_plan(in, 0).p_vbits == 24);
    }
}

static void check_packed()
{
    KnnFormatInput in = base();
    in.p_dim = 257;  // 23 value bits
    in.all.pvmax = 8388607.0;
    CHECK(knn_format_plan(in, 0).packed);
    in.all.pvmax = 8388608.0;
    CHECK(!knn_format_plan(in, 0).packed && !knn_format_plan(in, 0).pack16 && !knn_format_plan(in, 0).use_pop);
    in = base();
    in.c_dim = 257;
    in.all.cvmax = 8388607.0;
    CHECK(knn_format_plan(in, 0).packed);
    in.all.cvmax = 8388608.0;
    CHECK(!knn_format_plan(in, 0).packed);
    CHECK(knn_format_plan(with_max(&KnnMaxima::pss, 4294967295.0), 0).packed);
    CHECK(!knn_format_plan(with_max(&KnnMaxima::pss, 4294967296.0), 0).packed);
    CHECK(knn_format_plan(with_max(&KnnMaxima::css, 4294967295.0), 0).packed);
    CHECK(!knn_format_plan(with_max(&KnnMaxima::css, 4294967296.0), 0).packed);
    in = base();
    in.p_dim = (1 << 20) - 2;
    CHECK(knn_format_plan(in, 0).packed);
    in.p_dim = (1 << 20) - 1;
    CHECK(!knn_format_plan(in, 0).packed);
    in = base();
    in.c_dim = (1 << 20) - 2;
    CHECK(knn_format_plan(in, 0).packed);
    in.c_dim = (1 << 20) - 1;
    CHECK(!knn_format_plan(in, 0).packed);
    in = base();
    in.integral = false;
    CHECK(!knn_format_plan(in, 0).packed);
    in = base();
    in.sw.force_generic = true;
    CHECK(!knn_format_plan(in, 0).packed);
}

static void check_pack16()
{
    double KnnMaxima::*const all4[4] = {&KnnMaxima::pvmax, &KnnMaxima::cvmax, &KnnMaxima::pss, &KnnMaxima::css};
    for (double KnnMaxima::*const m : all4) {
        const KnnFormatPlan below = knn_format_plan(with_max(m, 65535.0), 0), at = knn_format_plan(with_max(m, 65536.0), 0);
        CHECK(below.packed && below.pack16);
        CHECK(at.packed && !at.pack16 && !at.want_ht);
    }
    KnnFormatInput in = base();
    in.sw.no_pack16 = true;
    const KnnFormatPlan pl = knn_format_plan(in, 0);
    CHECK(pl.packed && !pl.pack16 && !pl.want_ht);
}

static void check_ht_h()
{
    KnnFormatInput in = base();
    CHECK(knn_format_plan(in, 0).ht_h == 100);
    in.p_dim = 5000;
    CHECK(knn_format_plan(in, 0).ht_h == 512);
    in.sw.env_ht_h = 1000;
    CHECK(knn_format_plan(in, 0).ht_h == 1000);
    in.sw.env_ht_h = 4096;
    CHECK(knn_format_plan(in, 0).ht_h == 2048);  // 65536 / (2 * 16)
}

static void check_want_ht()
{
    CHECK(knn_format_plan(base(), 0).want_ht);
    KnnFormatInput in = base();
    in.n = 0;
    CHECK(!knn_format_plan(in, 0).want_ht);
    in.n = (1 << 24) - 1;
    CHECK(knn_format_plan(in, 0).want_ht);
    in.n = 1 << 24;
    CHECK(!knn_format_plan(in, 0).want_ht && knn_format_plan(in, 0).pack16);
    CHECK(knn_format_plan(with_max(&KnnMaxima::pvmax, 255.0), 0).want_ht);
    CHECK(!knn_format_plan(with_max(&KnnMaxima::pvmax, 256.0), 0).want_ht);
    CHECK(knn_format_plan(with_max(&KnnMaxima::cvmax, 255.0), 0).want_ht);
    CHECK(!knn_format_plan(with_max(&KnnMaxima::cvmax, 256.0), 0).want_ht);
    in = base();
    in.c_dim = 64;
    CHECK(knn_format_plan(in, 0).want_ht);
    in.c_dim = 65;
    CHECK(!knn_format_plan(in, 0).want_ht && knn_format_plan(in, 0).pack16);
    in = base();
    in.sw.no_ht = true;
    CHECK(!knn_format_plan(in, 0).want_ht && knn_format_plan(in, 0).pack16);
    CHECK(!knn_format_plan(with_max(&KnnMaxima::pss, 65536.0), 0).want_ht);  // not PACK16
}

static void check_use_pop()
{
    KnnFormatInput in = base();
    in.sw.no_ht = true;  // without the head / tail form the place panel's size decides: 2 * p_dim against 16384 bytes
    in.p_dim = 8192;
    CHECK(!knn_format_plan(in, 0).use_pop && knn_format_plan(in, 0).pop_h == 0 && knn_format_plan(in, 0).key_h == 0);
    in.p_dim = 8193;
    CHECK(knn_format_plan(in, 0).use_pop);
    CHECK(knn_format_plan(base(), 0).use_pop);  // through the head / tail form
    in = base();
    in.sw.no_ht = true;
    CHECK(!knn_format_plan(in, 0).use_pop);
    in.sw.force_hash = true;
    CHECK(knn_format_plan(in, 0).use_pop);
    in.sw.no_pop = true;
    CHECK(!knn_format_plan(in, 0).use_pop);
    in = base();
    in.sw.no_pop = true;
    CHECK(!knn_format_plan(in, 0).use_pop && knn_format_plan(in, 0).want_ht);
    in = base();
    in.sw.force_hash = true;
    in.integral = false;  // not packed
    CHECK(!knn_format_plan(in, 0).use_pop);
    in = base();
    in.sw.force_hash = true;
    in.n = 0;
    CHECK(!knn_format_plan(in, 0).use_pop);
}

static void check_pop_h_and_key_h()
{
    KnnFormatInput in = base();
    CHECK(knn_format_plan(in, 0).pop_h == 100);
    in.p_dim = 10000;
    CHECK(knn_format_plan(in, 0).pop_h == 4096);
    in.sw.env_pop_h = 64;
    CHECK(knn_format_plan(in, 0).pop_h == 64);
    // key_h: the head width with the head / tail form, else the popular-prefix table's size
    in = base();
    in.p_dim = 5000;
    CHECK(knn_format_plan(in, 0).want_ht && knn_format_plan(in, 0).pop_h == 4096 && knn_format_plan(in, 0).key_h == 512);
    in = base();
    in.p_dim = 10000;
    in.sw.no_ht = true;
    CHECK(!knn_format_plan(in, 0).want_ht && knn_format_plan(in, 0).use_pop && knn_format_plan(in, 0).key_h == 4096);
}

int main()
{
    check_base();
    check_any_wide();
    check_eligibility();
    check_cap();
    check_vbits();
    check_packed();
    check_pack16();
    check_ht_h();
    check_want_ht();
    check_use_pop();
    check_pop_h_and_key_h();
    std::printf("%ld cases pass\n", cases);
    return 0;
}
