// knn_ht_prepass.h -- the per-batch HIT pre-pass of the head / tail scan; textually included by knn_ht.h
// (inside knn.hip's anonymous namespace).
//
// Interface to the scans (knn_scan_ht, its seeding instantiation, knn_scan MODE 3), unchanged since round 2:
//   hit word                         lane << 21 | q << 16 | product          (ht_pack_hit)
//   hits + tile_base[tile]           the tile's hits, grouped by candidate slice; the order inside a slice is
//                                    free (the scan adds integers)
//   off[tile * off_stride + s - slice0]   start of slice s inside the tile's hits; the closing entry
//                                    (s = nslices) is the tile's total
//
// ht_tile_bases   one block: tile_base[] from the per-row totals of create time.
// ht_build_hits   one block per tile.  The candidate slices are cut into SUB-RANGES of W slices, W a power of
//                 two chosen per tile from its hit total so that an average sub-range fills about half of an
//                 LDS stage of C hits.  Per sub-range:
//                   walk    a wave step loads 64 postings: 64 / S entries x S consecutive postings from each
//                           entry's cursor, S a power of two chosen per tile to hold twice the postings an entry
//                           has in a sub-range on average (so the loaded lines are used, not 1 lane in 20 as with
//                           one entry per wave).  A wave issues the loads of kHtPreBatches steps together, then
//                           appends their postings that fall into the sub-range densely to the stage (hit word +
//                           slice number): ONE returning LDS atomic per kHtPreBatches steps, the lanes' positions
//                           come from the ballots.  A segment that was inside the sub-range to its last lane is
//                           loaded again from its new cursor.  No global store in this loop.
//                   sort    counting sort by slice inside the LDS: count over the staged records (whose hit words
//                           move into registers), prefix, place - full lanes, no global latency in the chain; the
//                           prefix is the sub-range's piece of `off`.
//                   flush   the sub-range's hits are one contiguous run of `hits`: it leaves the CU as
//                           consecutive aligned 16-byte stores (the stage is laid out with the run's
//                           misalignment, so LDS reads and global stores are both aligned).
//                 A sub-range with more than C hits (seen at the append cursor; one slice and tile can hold
//                 65,536) takes ht_pre_two_pass, the first form's count / prefix / scatter with direct
//                 4-byte stores: right for any data, fast for typical data.
// ht_build_hits_v1  the first form for everything (LOCREC_KNN_HT_PRE_V1, the A/B switch; also where the
//                 postings do not fit 32-bit cursors): sub-ranges of kHtSubSlices slices, every posting list
//                 walked twice per sub-range, every hit a scattered 4-byte store from inside the walk.
//
// Measured at cfg2 (136 M hits per 16,384-query batch, 8.5 per slice and tile): profiles/ht_prepass_perf.txt.

constexpr int kHtMaxEntries = 1024;   // (query, tail place) pairs of one tile the pre-pass holds in LDS
constexpr int kHtSubSlices = 4096;    // first form: candidate slices one counting pass covers (u32 counters in LDS)
constexpr int kHtPreThreads = 512;
constexpr int kHtPreWidthMax = 512;   // staged form: slices of the widest sub-range = its LDS counters
constexpr int kHtPreStageMax = 8192;  // hits; a thread holds stage / threads hit words in registers while they are placed:
constexpr int kHtPreStageSmall = 4096;  // up to here 8 (ht_build_hits<QT, 8>: four blocks per CU), above 16 (two blocks)
constexpr int kHtPreStageDefault = 8192;  // measured: profiles/ht_prepass_perf.txt
constexpr int kHtPreStageMin = 64;
static_assert(kHtPreWidthMax == kHtPreThreads, "the staged form's prefix gives every thread one slice");

__host__ __device__ __forceinline__ uint32_t ht_pack_hit(uint32_t lane, uint32_t q, uint32_t prod)
{
    return (lane << 21) | (q << 16) | prod;
}

struct HtPreParams {
    const int64_t *csr_ptr;     // place family, renumbered indices, ascending inside a row
    const int32_t *csr_idx;
    const double *csr_val;
    const int64_t *post_ptr;    // [p_dim - h + 1]
    const uint32_t *post;       // row << 8 | value
    const int32_t *qrows;       // or nullptr: rows qrow0 ..
    int32_t qrow0, nq;
    int32_t h;
    int32_t slice0, nslices;    // scanned candidate slices [slice0, nslices)
    const int64_t *tile_base;
    uint32_t *hits;
    uint32_t *off;
    int32_t off_stride;
    int32_t *error;             // set when a tile has more than kHtMaxEntries entries (host checks first; tripwire)
    int32_t stage;              // staged form: C, hits the LDS stage holds
};

// dynamic LDS of the staged form: [C + 4 hit words][C slice numbers (u16)]
inline size_t ht_pre_stage_bytes(int stage) { return ((size_t)stage + 4) * 4 + (size_t)stage * 2; }

// tile_base[t] = number of hits of the tiles before t: a posting of a tail place is one hit for every
// query of the tile that holds the place.  One block; tail_hits[row] is precomputed at create time.
__global__ __launch_bounds__(1024) void ht_tile_bases(const int64_t *tail_hits, const int32_t *qrows, int32_t qrow0,
                                                      int32_t nq, int32_t qt, int32_t ntiles, int64_t *tile_base)
{
    __shared__ int64_t wsum[16];
    __shared__ int64_t carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int t0 = 0; t0 < ntiles; t0 += 1024) {
        const int t = t0 + tid;
        int64_t mine = 0;
        if (t < ntiles)
            for (int q = t * qt; q < min(nq, (t + 1) * qt); ++q) mine += tail_hits[qrows ? qrows[q] : qrow0 + q];
        int64_t inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int64_t before = carry;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (t < ntiles) tile_base[t] = before + inc - mine;
        __syncthreads();
        if (tid == 1023) carry = before + inc;
        __syncthreads();
    }
    if (tid == 0) tile_base[ntiles] = carry;
}

// The tile's entries: one per (query of the tile, tail element of its place vector), with the posting range
// of the place as a cursor (CUR = int64_t, or uint32_t where the host has checked that the postings fit).
// Returns their number; starts and ends with a barrier.
template <class CUR>
__device__ int ht_pre_entries(const HtPreParams &P, int q0, int nqt, int first_slice, CUR *e_cur, CUR *e_end, uint32_t *e_qv,
                              int *s_ne)
{
    const int tid = threadIdx.x;
    if (tid == 0) *s_ne = 0;
    __syncthreads();
    for (int q = 0; q < nqt; ++q) {
        const int row = P.qrows ? P.qrows[q0 + q] : P.qrow0 + q0 + q;
        for (int64_t e = P.csr_ptr[row] + tid; e < P.csr_ptr[row + 1]; e += kHtPreThreads) {
            const int idx = P.csr_idx[e];
            if (idx >= P.h) {
                const int slot = atomicAdd(s_ne, 1);
                if (slot < kHtMaxEntries) {
                    e_cur[slot] = (CUR)P.post_ptr[idx - P.h];
                    e_end[slot] = (CUR)P.post_ptr[idx - P.h + 1];
                    e_qv[slot] = ((uint32_t)q << 16) | (uint32_t)P.csr_val[e];
                }
            }
        }
    }
    __syncthreads();
    const int ne = min(*s_ne, kHtMaxEntries);
    if (*s_ne > kHtMaxEntries && tid == 0 && P.error) atomicAdd(P.error, 1);
    // the walk starts at first_slice (a candidate shard's first slice; the slice an overflowing sub-range starts at):
    // skip the postings before its first row
    if (first_slice > 0) {
        const uint32_t first_row = (uint32_t)first_slice * 64u;
        for (int e = tid; e < ne; e += kHtPreThreads) {
            CUR a = e_cur[e], b = e_end[e];
            while (a < b) {  // lower bound of first_row
                const CUR m = a + ((b - a) >> 1);
                if ((P.post[m] >> 8) < first_row) a = m + 1; else b = m;
            }
            e_cur[e] = a;
        }
        __syncthreads();
    }
    return ne;
}

// One sub-range [sl0, sl0 + nsl) of the tile, nsl <= CAP, in two walks over the entries' postings: pass A counts
// per slice with an LDS atomic, the prefix of the counts is the sub-range's piece of `off`, pass B takes a cursor
// with a returning LDS atomic and stores the hit - a scattered 4-byte store - from inside the walk.  The entries'
// cursors (e_cur) move past the sub-range.  `run` = hits of the tile before the sub-range; returns the
// sub-range's hits (the same value in every thread); ends with a barrier.
template <class CUR, int CAP>
__device__ uint32_t ht_pre_two_pass(const HtPreParams &P, int ne, CUR *e_cur, const CUR *e_end, const uint32_t *e_qv,
                                    uint32_t *cnt, uint32_t *wtot, int sl0, int nsl, uint32_t run, uint32_t *off_row,
                                    uint32_t *hits)
{
    static_assert(CAP % kHtPreThreads == 0, "every thread owns CAP / threads consecutive counters");
    constexpr int NW = kHtPreThreads / 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t row_end = (uint32_t)(sl0 + nsl) * 64u;
    for (int i = tid; i < nsl; i += kHtPreThreads) cnt[i] = 0u;
    __syncthreads();
    // pass A: count the postings of every entry that fall into this sub-range, per slice
    for (int e = wave; e < ne; e += NW) {
        const CUR end = e_end[e];
        for (CUR p = e_cur[e]; p < end; p += 64) {
            const bool in = p + lane < end;
            const uint32_t row = in ? (P.post[p + lane] >> 8) : 0xFFFFFFFFu;
            const bool mine = in && row < row_end;
            if (mine) atomicAdd(&cnt[(row >> 6) - sl0], 1u);
            if (!__all(mine)) break;
        }
    }
    __syncthreads();
    // exclusive prefix of the counts -> offsets; every thread owns PER consecutive slices
    constexpr int PER = CAP / kHtPreThreads;
    uint32_t local[PER];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid * PER + j;
        local[j] = i < nsl ? cnt[i] : 0u;
        sum += local[j];
    }
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    if (tid == 0) {
        uint32_t acc = 0;
        for (int w = 0; w < NW; ++w) {
            const uint32_t t = wtot[w];
            wtot[w] = acc;
            acc += t;
        }
        wtot[NW] = acc;
    }
    __syncthreads();
    uint32_t excl = run + wtot[wave] + inc - sum;
    const uint32_t total = wtot[NW];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid * PER + j;
        if (i < nsl) {
            cnt[i] = excl;                           // becomes the slice's write cursor
            off_row[(sl0 - P.slice0) + i] = excl;
        }
        excl += local[j];
    }
    __syncthreads();
    // pass B: the hits themselves, and the entries' cursors move past this sub-range
    for (int e = wave; e < ne; e += NW) {
        const CUR end = e_end[e];
        const uint32_t qv = e_qv[e];
        const uint32_t q = qv >> 16, qval = qv & 0xFFFFu;
        CUR p = e_cur[e];
        for (; p < end; p += 64) {
            const bool in = p + lane < end;
            const uint32_t pv = in ? P.post[p + lane] : 0xFFFFFFFFu;
            const uint32_t row = pv >> 8;
            const bool mine = in && row < row_end;
            if (mine) {
                const uint32_t pos = atomicAdd(&cnt[(row >> 6) - sl0], 1u);
                hits[pos] = ht_pack_hit(row & 63u, q, (pv & 0xFFu) * qval);
            }
            const uint64_t m = __ballot(mine);
            if (m != ~0ull) {  // postings are sorted by row: the lanes inside the sub-range form a prefix
                p += __popcll(m);
                break;
            }
        }
        if (lane == 0) e_cur[e] = p < end ? p : end;
    }
    __syncthreads();
    return total;
}

// The first form (see the head of this file).  Measured at cfg2 (profiles/ht_prepass_perf.txt): 1.39 ms per launch
// (0.88 - 2.06 over the batches); its stores reach memory as 3.7 GB of partly filled lines per launch (2.2 - 5.3 over
// the batches) for 0.35 - 0.5 GB of hits and offsets, and its waves wait 84 % of their cycles.
template <int QT>
__global__ __launch_bounds__(kHtPreThreads) void ht_build_hits_v1(const HtPreParams P)
{
    __shared__ int64_t e_cur[kHtMaxEntries];   // next posting of the entry
    __shared__ int64_t e_end[kHtMaxEntries];
    __shared__ uint32_t e_qv[kHtMaxEntries];   // q << 16 | query value
    __shared__ uint32_t cnt[kHtSubSlices];     // per slice of the current sub-range: count, then cursor
    __shared__ uint32_t wtot[kHtPreThreads / 64 + 1];
    __shared__ int s_ne;
    const int tile = blockIdx.x;
    const int q0 = tile * QT;
    const int ne = ht_pre_entries<int64_t>(P, q0, min(QT, P.nq - q0), P.slice0, e_cur, e_end, e_qv, &s_ne);
    uint32_t *off_row = P.off + (int64_t)tile * P.off_stride;
    uint32_t *hits = P.hits + P.tile_base[tile];
    uint32_t run = 0;  // hits of this tile before the current sub-range (same value in every thread)
    for (int sl0 = P.slice0; sl0 < P.nslices; sl0 += kHtSubSlices)
        run += ht_pre_two_pass<int64_t, kHtSubSlices>(P, ne, e_cur, e_end, e_qv, cnt, wtot, sl0, min(kHtSubSlices, P.nslices - sl0),
                                                      run, off_row, hits);
    if (threadIdx.x == 0) off_row[P.nslices - P.slice0] = run;
}

// ---- staged form --------------------------------------------------------------------------------

constexpr int kHtPreBatches = 8;  // posting loads a wave keeps in flight

template <int QT, int RECS>
__global__ __launch_bounds__(kHtPreThreads, RECS == 8 ? 8 : 4) void ht_build_hits(const HtPreParams P)
{
    extern __shared__ __align__(16) unsigned char ht_pre_smem[];
    __shared__ uint32_t e_cur[kHtMaxEntries];  // next posting of the entry
    __shared__ uint32_t e_end[kHtMaxEntries];
    __shared__ uint32_t e_qv[kHtMaxEntries];   // q << 16 | query value
    __shared__ uint32_t cnt[kHtPreWidthMax];   // per slice of the current sub-range: count, then cursor
    __shared__ uint32_t wtot[kHtPreThreads / 64 + 1];
    __shared__ int s_ne;
    __shared__ uint32_t s_n;                   // append cursor of the stage = hits of the sub-range
    constexpr int NW = kHtPreThreads / 64, NB = kHtPreBatches;
    const int stage = P.stage;
    uint32_t *st_hit = reinterpret_cast<uint32_t *>(ht_pre_smem);  // [stage + 4]: the run, behind its misalignment
    unsigned short *st_sl = reinterpret_cast<unsigned short *>(st_hit + stage + 4);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x;
    const int q0 = tile * QT;
    const int nqt = min(QT, P.nq - q0);
    int ne = ht_pre_entries<uint32_t>(P, q0, nqt, P.slice0, e_cur, e_end, e_qv, &s_ne);
    uint32_t *off_row = P.off + (int64_t)tile * P.off_stride;
    const int64_t tbase = P.tile_base[tile];
    uint32_t *hits = P.hits + tbase;
    // sub-range width: the power of two nearest (in ratio) to the slices that hold stage / 2 hits on average;
    // segment: the lanes that load consecutive postings of ONE entry - the power of two that holds twice the postings
    // an entry has in a sub-range on average (a wave then loads 64 >> seg_log entries per step)
    int width = 1, seg_log = 2;
    {
        const int64_t tot = P.tile_base[tile + 1] - tbase;
        const int64_t all = P.nslices - P.slice0;
        const int64_t target = (int64_t)(stage / 2) * all / (tot > 0 ? tot : 1);
        while (width < kHtPreWidthMax && (int64_t)width * 10 <= target * 7) width *= 2;
        const int64_t per_entry2 = 2 * tot * width / (all * (ne > 0 ? ne : 1));
        while (seg_log < 6 && (1 << seg_log) < per_entry2) ++seg_log;
    }
    const int seg_lanes = 1 << seg_log;
    const int seg = lane >> seg_log;          // this lane's entry inside a wave step
    const uint32_t k = (uint32_t)lane & (uint32_t)(seg_lanes - 1);
    const uint64_t seg_mask = (seg_lanes == 64 ? ~0ull : ((1ull << seg_lanes) - 1ull)) << (seg << seg_log);
    const int per_step = 64 >> seg_log;       // entries of one wave step
    const int nsteps = (ne + per_step - 1) / per_step;
    uint32_t run = 0;  // hits of this tile before the current sub-range (same value in every thread)
    for (int sl0 = P.slice0; sl0 < P.nslices; sl0 += width) {
        const int nsl = min(width, P.nslices - sl0);
        const uint32_t row0 = (uint32_t)sl0 * 64u, row_end = (uint32_t)(sl0 + nsl) * 64u;
        const uint32_t mis = (uint32_t)((tbase + run) & 3);  // words the run starts behind a 16-byte boundary of `hits`
        if (tid < nsl) cnt[tid] = 0u;
        if (tid == 0) s_n = 0u;
        __syncthreads();
        // ---- walk: NB steps of the wave in flight, each one load of 64 postings (per_step entries x seg_lanes);
        // a step whose segment was in the sub-range to its last lane is taken again for that segment
        for (int s0 = wave; s0 < nsteps; s0 += NW * NB) {
            uint32_t c[NB], en[NB], pv[NB];
            bool act[NB], in[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int e = (s0 + j * NW) * per_step + seg;
                act[j] = s0 + j * NW < nsteps && e < ne;
                c[j] = act[j] ? e_cur[e] : 0u;
                en[j] = act[j] ? e_end[e] : 0u;
            }
            bool again;
            do {
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    in[j] = act[j] && k < en[j] - c[j];  // (c <= en: no 32-bit sum that could wrap)
                    pv[j] = in[j] ? P.post[c[j] + k] : 0u;
                }
                // one append for the NB steps: their lanes' positions come from the ballots
                uint64_t m[NB];
                uint32_t before[NB], total = 0;
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    m[j] = __ballot(in[j] && (pv[j] >> 8) < row_end);
                    before[j] = total;
                    total += (uint32_t)__popcll(m[j]);
                }
                again = false;
                if (total != 0u) {  // (wave-uniform)
                    uint32_t at = 0;
                    if (lane == 0) at = atomicAdd(&s_n, total);
                    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane(at);
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        const uint32_t row = pv[j] >> 8;
                        const uint32_t pos = base + before[j] +
                                             __builtin_amdgcn_mbcnt_hi((uint32_t)(m[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[j], 0u));
                        // (beyond the stage nothing is written; the cursor goes on counting and the sub-range is redone below)
                        if (((m[j] >> lane) & 1ull) && pos < (uint32_t)stage) {
                            const uint32_t qv = e_qv[(s0 + j * NW) * per_step + seg];
                            st_hit[mis + pos] = ht_pack_hit(row & 63u, qv >> 16, (pv[j] & 0xFFu) * (qv & 0xFFFFu));
                            st_sl[pos] = (unsigned short)((row - row0) >> 6);
                        }
                        const uint32_t took = (uint32_t)__popcll(m[j] & seg_mask);  // postings are sorted by row: a prefix of the segment
                        c[j] += took;
                        act[j] = took == (uint32_t)seg_lanes && c[j] < en[j];
                        if (k == 0u && took > 0u) e_cur[(s0 + j * NW) * per_step + seg] = c[j];
                        again = again || act[j];
                    }
                }
            } while (__any(again));
        }
        __syncthreads();
        const uint32_t n = s_n;
        if (n > (uint32_t)stage) {
            // ---- overflow: the entries again, with their cursors at the sub-range's first row, and the sub-range in
            // two passes with direct stores (which leave the cursors behind it)
            ne = ht_pre_entries<uint32_t>(P, q0, nqt, sl0, e_cur, e_end, e_qv, &s_ne);
            run += ht_pre_two_pass<uint32_t, kHtPreWidthMax>(P, ne, e_cur, e_end, e_qv, cnt, wtot, sl0, nsl, run, off_row, hits);
            continue;
        }
        if (n == 0u) {  // (the next iteration's barrier separates these counters from its own)
            if (tid < nsl) off_row[(sl0 - P.slice0) + tid] = run;
            continue;
        }
        // ---- counting sort by slice: the hit words move into registers (the placing overwrites them; the slice
        // numbers stay where they are), the stage receives them in slice order
        uint32_t rec_hit[RECS];
#pragma unroll
        for (int r = 0; r < RECS; ++r) {
            const uint32_t i = (uint32_t)(tid + r * kHtPreThreads);
            if (i < n) {
                rec_hit[r] = st_hit[mis + i];
                atomicAdd(&cnt[st_sl[i]], 1u);
            }
        }
        __syncthreads();
        const uint32_t mine = tid < nsl ? cnt[tid] : 0u;
        uint32_t inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        uint32_t excl = inc - mine;
        for (int w = 0; w < wave; ++w) excl += wtot[w];
        if (tid < nsl) {
            cnt[tid] = excl;  // becomes the slice's cursor inside the stage
            off_row[(sl0 - P.slice0) + tid] = run + excl;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RECS; ++r) {
            const uint32_t i = (uint32_t)(tid + r * kHtPreThreads);
            if (i < n) st_hit[mis + atomicAdd(&cnt[st_sl[i]], 1u)] = rec_hit[r];
        }
        __syncthreads();
        // ---- flush: stage words [mis, mis + n) -> hits[run ..), whole 16-byte groups wherever the run covers one
        {
            uint32_t *dst = hits + run - mis;  // 16-byte aligned
            const uint32_t last = mis + n;
            for (uint32_t g = (uint32_t)tid * 4u; g < last; g += kHtPreThreads * 4u) {
                if (g >= mis && g + 4u <= last) {
                    *reinterpret_cast<u32x4 *>(dst + g) = *reinterpret_cast<const u32x4 *>(st_hit + g);
                } else {
                    for (uint32_t i = max(g, mis); i < min(g + 4u, last); ++i) dst[i] = st_hit[i];
                }
            }
        }
        run += n;
        // (the next iteration's barrier stands between these reads of the stage and its walk)
    }
    if (tid == 0) off_row[P.nslices - P.slice0] = run;
}
