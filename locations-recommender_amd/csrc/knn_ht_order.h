// knn_ht_order.h -- the order of a row's elements inside one slice of the head / tail image (knn_ht.h), chosen so that the
// 16 lanes one LDS cycle serves read panel rows on different slots ("Element order").  Plain C++, nothing
// from HIP and no device call: both builders (knn_build.hip on the device, build_ht in knn.hip on the host) run the same
// routine on the same words, so their images agree (integer code only); tests/host/knn_ht_order_check.cpp compiles it alone,
// under a host sanitizer.
//
// The model.  At position t of a slice every lane reads the 16-byte panel row its t-th word names (index << 4 in the low
// half).  ds_read_b128 serves the lanes in four groups of 16 (ht_order_lane); a row's slot in the 256-byte bank row is
// index mod 16; lanes that name the SAME row share one read, DIFFERENT rows on one slot take a cycle each.  So one group
// read costs max(1, the largest number of distinct rows on one slot) cycles.  Integer dots are exact in any order, hence
// the order of a row's elements inside [0, cnt) is free, and a padding word in front of cnt (value 0) may name any row
// below the panel's size: it names one that another lane of the group reads at that position anyway.
#pragma once

#include <cstdint>

#if defined(__HIP__)  // (the compiler's own macro: the HIP runtime header is the includer's business)
// minsize: serial, branchy code that every working lane runs at a place of its own - unrolled and inlined it was 166 KB
// in kb_ht_order, several times the instruction cache, and the kernel waited for its instructions
#define LOCREC_HT_ORDER_FN __host__ __device__ inline __attribute__((minsize))
#else
#define LOCREC_HT_ORDER_FN inline
#endif

namespace locrec {

constexpr int kHtOrderLanes = 16;        // lanes one LDS cycle serves
constexpr int kHtOrderGroups = 4;        // such groups in a slice of 64
constexpr int kHtOrderLook = 16;         // not yet placed elements of a lane, and positions around a conflict, that are looked at:
                                         // the work stays linear in the count (a slice of long rows is rare, and one thread's)
constexpr int kHtOrderRepairPasses = 4;  // sweeps of the repair step (each accepted swap lowers the cost: it ends anyway)

// the routines' small tables, the caller's to place: the device build keeps them in LDS - as local arrays they are scratch
// memory there, and the waves of a launch then hold more of it than the caches do
struct HtOrderWork {
    int rem[kHtOrderLanes], look[kHtOrderLanes], placed[kHtOrderLanes], match[kHtOrderLanes], lane_order[kHtOrderLanes], src[kHtOrderLanes];
    uint32_t avail[kHtOrderLanes];
    int demand[16], slot_order[16], slot_row[16], slot_cnt[16], owner[16];
    int rows[kHtOrderLanes], load[16];  // (ht_order_cycles_at)
};

// lane of the slice that is member i (0 .. 15) of group g (0 .. 3): {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, the same + 32
LOCREC_HT_ORDER_FN int ht_order_lane(int g, int i)
{
    const int base = (g >> 1) * 32;
    if ((g & 1) == 0) return base + (i < 4 ? i : i < 8 ? i + 8 : i + 12);
    return base + (i < 8 ? i + 4 : i < 12 ? i + 8 : i + 16);
}

// word of (lane, position) inside a slice's image: [position / 4][lane][position % 4]
LOCREC_HT_ORDER_FN int64_t ht_order_word(int lane, int pos) { return (int64_t)(pos >> 2) * 256 + lane * 4 + (pos & 3); }

LOCREC_HT_ORDER_FN int ht_order_row(uint32_t w) { return (int)((w >> 4) & 0xFFFu); }
LOCREC_HT_ORDER_FN bool ht_order_is_pad(uint32_t w) { return (w >> 16) == 0u; }  // (value 0 multiplies nothing)

// one lane group of one slice of an image in memory: the Img of the routines below.  Any type with get(i, pos) and
// set(i, pos, word), i = member of the group, will do.
struct HtOrderSlice {
    uint32_t *base;  // first word of the slice
    int g;
    LOCREC_HT_ORDER_FN uint32_t get(int i, int pos) const { return base[ht_order_word(ht_order_lane(g, i), pos)]; }
    LOCREC_HT_ORDER_FN void set(int i, int pos, uint32_t w) const { base[ht_order_word(ht_order_lane(g, i), pos)] = w; }
};

// LDS cycles of the group's read at one position.  free_pad: lanes (bit i) whose padding words do not count yet - they
// will name a row that is read anyway; 0 = the image as the kernel sees it.
template <class Img>
LOCREC_HT_ORDER_FN int ht_order_cycles_at(const Img &img, int pos, uint32_t free_pad, HtOrderWork &wk)
{
    int *rows = wk.rows, *load = wk.load, nrows = 0, worst = 1;
    for (int s = 0; s < 16; ++s) load[s] = 0;
    for (int i = 0; i < kHtOrderLanes; ++i) {
        const uint32_t w = img.get(i, pos);
        if (((free_pad >> i) & 1u) && ht_order_is_pad(w)) continue;
        const int r = ht_order_row(w);
        bool seen = false;
        for (int k = 0; k < nrows; ++k) seen = seen || rows[k] == r;
        if (seen) continue;
        rows[nrows++] = r;
        const int m = ++load[r & 15];
        worst = m > worst ? m : worst;
    }
    return worst;
}

// the figure of the model: cycles of all positions in front of cnt
template <class Img>
LOCREC_HT_ORDER_FN int ht_order_cycles(const Img &img, int cnt, HtOrderWork &wk)
{
    int c = 0;
    for (int t = 0; t < cnt; ++t) c += ht_order_cycles_at(img, t, 0u, wk);
    return c;
}
template <class Img>
LOCREC_HT_ORDER_FN int ht_order_cycles(const Img &img, int cnt)
{
    HtOrderWork wk;
    return ht_order_cycles(img, cnt, wk);
}

namespace ht_order_detail {

// position in [t, t + rem) of the lane's not yet placed element on panel row `row`, or -1
template <class Img>
LOCREC_HT_ORDER_FN int find_row(const Img &img, int i, int t, int rem, int row)
{
    for (int j = t; j < t + rem; ++j)
        if (ht_order_row(img.get(i, j)) == row) return j;
    return -1;
}

// ... of its element with the smallest row on `slot` (the most popular place: the one other lanes are likeliest to share)
template <class Img>
LOCREC_HT_ORDER_FN int find_on_slot(const Img &img, int i, int t, int rem, int slot)
{
    int best = -1, best_row = 1 << 30;
    for (int j = t; j < t + rem; ++j) {
        const int r = ht_order_row(img.get(i, j));
        if ((r & 15) == slot && r < best_row) {
            best_row = r;
            best = j;
        }
    }
    return best;
}

// distinct rows among placed[] (>= 0) on `slot`; whether `row` is among them
LOCREC_HT_ORDER_FN int slot_load(const int *placed, int slot)
{
    int n = 0;
    for (int i = 0; i < kHtOrderLanes; ++i) {
        if (placed[i] < 0 || (placed[i] & 15) != slot) continue;
        bool first = true;
        for (int k = 0; k < i; ++k) first = first && placed[k] != placed[i];
        n += first ? 1 : 0;
    }
    return n;
}
// the largest slot_load over all slots, in one pass (load: 16 counters of the caller)
LOCREC_HT_ORDER_FN int worst_load(const int *placed, int *load)
{
    int worst = 1;
    for (int s = 0; s < 16; ++s) load[s] = 0;
    for (int i = 0; i < kHtOrderLanes; ++i) {
        if (placed[i] < 0) continue;
        bool first = true;
        for (int k = 0; k < i; ++k) first = first && placed[k] != placed[i];
        if (!first) continue;
        const int m = ++load[placed[i] & 15];
        worst = m > worst ? m : worst;
    }
    return worst;
}
LOCREC_HT_ORDER_FN bool row_present(const int *placed, int row)
{
    bool p = false;
    for (int i = 0; i < kHtOrderLanes; ++i) p = p || placed[i] == row;
    return p;
}

// ascending order again: a lane's elements by row in front, zero words behind
template <class Img>
LOCREC_HT_ORDER_FN void restore_ascending(Img &img, int cnt, uint32_t blank)
{
    for (int i = 0; i < kHtOrderLanes; ++i) {
        if ((blank >> i) & 1u) continue;
        for (int a = 0; a < cnt; ++a) {  // insertion sort, padding last
            const uint32_t w = img.get(i, a);
            const int key = ht_order_is_pad(w) ? 1 << 30 : ht_order_row(w);
            int b = a;
            while (b > 0) {
                const uint32_t v = img.get(i, b - 1);
                const int kv = ht_order_is_pad(v) ? 1 << 30 : ht_order_row(v);
                if (kv <= key) break;
                img.set(i, b, v);
                --b;
            }
            img.set(i, b, ht_order_is_pad(w) ? 0u : w);
        }
        for (int a = 0; a < cnt; ++a)
            if (ht_order_is_pad(img.get(i, a))) img.set(i, a, 0u);
    }
}

}  // namespace ht_order_detail

// Re-orders, in place, the words of one lane group in positions [0, cnt).  On entry every lane holds its elements
// (value != 0) in ascending order in front and zero words behind, as the builders write them; cnt = the exact element
// count of the slice's widest row.  blank: lanes (bit i) that stay as they are - a wide row's stand-in, all zero.  On
// return every lane holds the same elements somewhere in [0, cnt), its other words in front of cnt are value 0 with the
// row of a lane that reads there anyway, and the modelled cycles are at most those of the ascending order - which is
// put back when the search does not beat it.  Words at and behind cnt are not touched.
//
// A greedy pass fills position after position: lanes are matched to free slots (those that cannot wait first, busiest
// slots first, one step of an alternating path where a slot is taken, lanes with the same row sharing a slot), a lane
// that found none waits on a padding word if its row is shorter than cnt, and otherwise takes the least loaded slot.
// A repair pass then moves single elements of over-full slots to other positions of their lane while that lowers the sum.
template <class Img>
LOCREC_HT_ORDER_FN void ht_order_group(Img &img, int cnt, uint32_t blank, HtOrderWork &wk)
{
    using namespace ht_order_detail;
    if (cnt <= 0) return;
    const uint32_t movable = ~blank & 0xFFFFu;
    const int before = ht_order_cycles(img, cnt, wk);
    int *rem = wk.rem, *look = wk.look, *placed = wk.placed, *match = wk.match, *lane_order = wk.lane_order, *src = wk.src;
    int *demand = wk.demand, *slot_order = wk.slot_order, *slot_row = wk.slot_row, *slot_cnt = wk.slot_cnt, *owner = wk.owner;
    uint32_t *avail = wk.avail;
    int total = 0;
    for (int i = 0; i < kHtOrderLanes; ++i) {
        rem[i] = 0;
        if ((blank >> i) & 1u) continue;
        for (int j = 0; j < cnt; ++j) rem[i] += ht_order_is_pad(img.get(i, j)) ? 0 : 1;
        total += rem[i];
    }
    if (total == 0 || before == cnt) return;  // nothing to move, or nothing to gain

    for (int t = 0; t < cnt; ++t) {
        // ---- what every lane could read at this position (look[i]: the elements of the lane that are candidates)
        // placed[i]: row the lane reads at t; -1 undecided, -2 padding
        for (int i = 0; i < kHtOrderLanes; ++i) look[i] = rem[i] < kHtOrderLook ? rem[i] : kHtOrderLook;
        int nl = 0;
        for (int s = 0; s < 16; ++s) {
            demand[s] = 0;
            slot_row[s] = -1;
            slot_cnt[s] = 0;
            owner[s] = -1;
        }
        for (int i = 0; i < kHtOrderLanes; ++i) {
            placed[i] = ((blank >> i) & 1u) ? 0 : -1;
            avail[i] = 0u;
            match[i] = -1;
            if (((blank >> i) & 1u) || rem[i] == 0) continue;
            for (int j = t; j < t + look[i]; ++j) {
                const int s = ht_order_row(img.get(i, j)) & 15;
                avail[i] |= 1u << s;
                ++demand[s];
            }
            lane_order[nl++] = i;
        }
        if (blank & 0xFFFFu) {  // the stand-ins read row 0
            slot_row[0] = 0;
            slot_cnt[0] = 2;
        }
        for (int s = 0; s < 16; ++s) {  // busiest slot first
            int b = s;
            while (b > 0 && demand[slot_order[b - 1]] < demand[s]) {
                slot_order[b] = slot_order[b - 1];
                --b;
            }
            slot_order[b] = s;
        }
        for (int a = 1; a < nl; ++a) {  // least slack first (slack = cnt - t - rem: rem descending), then lane order
            const int i = lane_order[a];
            int b = a;
            while (b > 0 && rem[lane_order[b - 1]] < rem[i]) {
                lane_order[b] = lane_order[b - 1];
                --b;
            }
            lane_order[b] = i;
        }
        // ---- lanes to slots
        for (int a = 0; a < nl; ++a) {
            const int i = lane_order[a];
            for (int k = 0; k < 16 && match[i] < 0; ++k) {
                const int s = slot_order[k];
                if (!((avail[i] >> s) & 1u)) continue;
                if (slot_row[s] < 0) {
                    slot_row[s] = ht_order_row(img.get(i, find_on_slot(img, i, t, look[i], s)));
                    slot_cnt[s] = 1;
                    owner[s] = i;
                    match[i] = s;
                } else if (find_row(img, i, t, look[i], slot_row[s]) >= 0) {
                    ++slot_cnt[s];
                    match[i] = s;
                }
            }
            for (int k = 0; k < 16 && match[i] < 0; ++k) {  // one alternating step: the slot's only lane moves on
                const int s = slot_order[k];
                if (!((avail[i] >> s) & 1u) || slot_cnt[s] != 1) continue;
                const int j = owner[s];
                for (int k2 = 0; k2 < 16; ++k2) {
                    const int s2 = slot_order[k2];
                    if (s2 == s || !((avail[j] >> s2) & 1u)) continue;
                    if (slot_row[s2] < 0) {
                        slot_row[s2] = ht_order_row(img.get(j, find_on_slot(img, j, t, look[j], s2)));
                        slot_cnt[s2] = 1;
                        owner[s2] = j;
                    } else if (find_row(img, j, t, look[j], slot_row[s2]) >= 0) {
                        ++slot_cnt[s2];
                    } else {
                        continue;
                    }
                    match[j] = s2;
                    slot_row[s] = ht_order_row(img.get(i, find_on_slot(img, i, t, look[i], s)));
                    owner[s] = i;
                    match[i] = s;
                    break;
                }
            }
        }
        // ---- place.  src[i] = position the lane's word for t comes from, -1 = padding
        for (int i = 0; i < kHtOrderLanes; ++i) {
            src[i] = -1;
            if (match[i] < 0) continue;
            src[i] = find_row(img, i, t, look[i], slot_row[match[i]]);
            placed[i] = slot_row[match[i]];
        }
        for (int pass = 0; pass < 2; ++pass) {  // the unmatched: first those that cannot wait, then the others
            bool any = false;
            for (int a = 0; a < nl; ++a) any = any || (match[lane_order[a]] < 0 && placed[lane_order[a]] == -1);
            if (!any) break;
            const int worst = pass == 1 ? worst_load(placed, wk.load) : 1;
            for (int a = 0; a < nl; ++a) {
                const int i = lane_order[a];
                const bool must = rem[i] == cnt - t;
                if (match[i] >= 0 || placed[i] != -1 || must != (pass == 0)) continue;
                int best = -1, best_cost = 1 << 30;
                for (int j = t; j < t + look[i]; ++j) {
                    const int r = ht_order_row(img.get(i, j));
                    const int c = row_present(placed, r) ? -1 : slot_load(placed, r & 15);
                    if (c < best_cost) {
                        best_cost = c;
                        best = j;
                    }
                }
                // (a lane that can wait joins a row that is read anyway, or a slot that stays within the position's worst)
                if (must || best_cost < 0 || best_cost + 1 <= worst) {
                    src[i] = best;
                    placed[i] = ht_order_row(img.get(i, best));
                } else {
                    placed[i] = -2;
                }
            }
        }
        for (int i = 0; i < kHtOrderLanes; ++i) {
            if ((blank >> i) & 1u) continue;
            if (src[i] >= 0) {
                const uint32_t a = img.get(i, t), b = img.get(i, src[i]);
                img.set(i, t, b);
                img.set(i, src[i], a);
                --rem[i];
            } else {  // padding (its row is written at the end): the element here, if any, moves behind the others
                if (rem[i] > 0) img.set(i, t + rem[i], img.get(i, t));
                img.set(i, t, 0u);
            }
        }
    }

    // ---- repair: an element of an over-full slot changes places with another word of its lane
    for (int pass = 0; pass < kHtOrderRepairPasses; ++pass) {
        bool improved = false;
        for (int t = 0; t < cnt; ++t) {
            int ct = ht_order_cycles_at(img, t, movable, wk);
            for (int i = 0; i < kHtOrderLanes && ct > 1; ++i) {
                if ((blank >> i) & 1u) continue;
                const uint32_t w = img.get(i, t);
                if (ht_order_is_pad(w)) continue;
                {  // only lanes of a slot as full as the position's worst
                    for (int k = 0; k < kHtOrderLanes; ++k) {
                        const uint32_t v = img.get(k, t);
                        placed[k] = (((movable >> k) & 1u) && ht_order_is_pad(v)) ? -2 : ht_order_row(v);
                    }
                    if (slot_load(placed, ht_order_row(w) & 15) < ct) continue;
                }
                const int u_end = t + kHtOrderLook + 1 < cnt ? t + kHtOrderLook + 1 : cnt;
                for (int u = t > kHtOrderLook ? t - kHtOrderLook : 0; u < u_end; ++u) {
                    if (u == t) continue;
                    const uint32_t v = img.get(i, u);
                    const int cu = ht_order_cycles_at(img, u, movable, wk);
                    img.set(i, t, v);
                    img.set(i, u, w);
                    const int nt = ht_order_cycles_at(img, t, movable, wk), nu = ht_order_cycles_at(img, u, movable, wk);
                    if (nt + nu < ct + cu) {
                        ct = nt;
                        improved = true;
                        break;
                    }
                    img.set(i, t, w);
                    img.set(i, u, v);
                }
            }
        }
        if (!improved) break;
    }

    // ---- padding words name a row that is read at their position anyway
    for (int t = 0; t < cnt; ++t) {
        int row = 0;
        if (!(blank & 0xFFFFu))
            for (int i = kHtOrderLanes - 1; i >= 0; --i)
                if (!ht_order_is_pad(img.get(i, t))) row = ht_order_row(img.get(i, t));
        for (int i = 0; i < kHtOrderLanes; ++i)
            if (((movable >> i) & 1u) && ht_order_is_pad(img.get(i, t))) img.set(i, t, (uint32_t)row << 4);
    }
    if (ht_order_cycles(img, cnt, wk) >= before) restore_ascending(img, cnt, blank);
}
template <class Img>
LOCREC_HT_ORDER_FN void ht_order_group(Img &img, int cnt, uint32_t blank)
{
    HtOrderWork wk;
    ht_order_group(img, cnt, blank, wk);
}

}  // namespace locrec
