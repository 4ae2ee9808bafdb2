// knn_aggregate.h -- a5 makeRecommendations0 (KnnRecommender.scala:51-70): knn_aggregate and its helpers
// A fragment of knn.hip's translation unit: included by knn.hip inside its anonymous namespace, after the parameter
// blocks and the headers it names (it is not a stand-alone header; the split only keeps every file readable).
#pragma once

// a5: makeRecommendations0 (KnnRecommender.scala:51-70) for one query per block.
// The <= K neighbours' rating rows are flattened in neighbour-rank order; one 64-bit key per row,
// compact place index << 16 | sequence number, is sorted in LDS (no payload to move); the
// products rating*similarity are gathered once, in parallel, and each place is then summed left
// to right from LDS -- in neighbour-rank order, the oracle's order.
// Block-wide exclusive prefix sum of one int per thread (blockDim.x <= 1024, a multiple of 64);
// *total receives the sum.  wtot: LDS scratch of 17 ints.
__device__ __forceinline__ int block_exclusive_scan(int v, int *wtot, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int w = 0; w < nw; ++w) {
            const int t = wtot[w];
            wtot[w] = acc;
            acc += t;
        }
        wtot[16] = acc;
    }
    __syncthreads();
    *total = wtot[16];
    return wtot[wave] + inc - v;
}

// (kAggThreads and the other constants of the aggregation: knn_agg_plan.h)

// KeyT: uint32_t where (compact place index, position) fit 32 bits - half the LDS traffic of the bitonic sort, which is
// what this kernel's time goes into (2,048 keys x 66 stages per query) - else uint64_t; fbits = bits of the position.
template <typename KeyT>
__global__ __launch_bounds__(kAggThreads) void knn_aggregate(
    const int32_t *nb_rows, const double *nb_sims, const int64_t *nb_cnt, int32_t K,
    const int64_t *r_ptr, const int32_t *r_pidx, const double *r_rating, const int64_t *cplace_ids,
    int32_t M /* pow2 LDS capacity, <= kAggCap */, int64_t *out_place, double *out_est, int64_t *out_n,
    int32_t *out_overflow, int64_t out_stride, int32_t redo_only, int32_t fbits,
    unsigned char *host = nullptr /* one request: the result also goes into the pinned staging buffer, in
    locrec_knn_recommend's layout (count at 0, overflow flag at 16, *host_flag_src at 20, places at 64, estimates
    behind host_cap of them) */, const int32_t *host_flag_src = nullptr, int32_t host_cap = 0,
    unsigned long long *stats = nullptr /* locrec_knn_aggregate_stats: [1] queries summed here, [2] queries left flagged */,
    int32_t last_pass = 1 /* no redo launch follows: a flag set here is final */)
{
    // second pass of a batch: only the queries whose rows did not fit the first pass's smaller capacity
    if (redo_only && out_overflow[blockIdx.x] == 0) return;
    if (host && threadIdx.x == 0 && host_flag_src) *reinterpret_cast<int32_t *>(host + 20) = *host_flag_src;
    extern __shared__ __align__(16) unsigned char smem[];
    KeyT *key = reinterpret_cast<KeyT *>(smem);               // [M]
    double *wrv = reinterpret_cast<double *>(smem + (((size_t)M * sizeof(KeyT) + 7) & ~(size_t)7));  // [M] rating * similarity
    unsigned short *av = reinterpret_cast<unsigned short *>(wrv + M);  // [M] neighbour of the position (its similarity: simv[])
    int64_t *rbase = reinterpret_cast<int64_t *>(reinterpret_cast<unsigned char *>(av) + (((size_t)M * 2 + 7) & ~(size_t)7));  // [K] first rating row of neighbour i
    double *simv = reinterpret_cast<double *>(rbase + K);     // [K]
    int32_t *off = reinterpret_cast<int32_t *>(simv + K);     // [K+1] prefix of neighbour row counts
    const int q = blockIdx.x;
    const int tid = threadIdx.x;
    const int m = max(0, (int)nb_cnt[q]);  // -1: not a valid query (knn_mark_absent)
    const int32_t *rows = nb_rows + (int64_t)q * K;
    const double *sims = nb_sims + (int64_t)q * K;
    __shared__ int wtot[17];
    // neighbour row counts -> exclusive offsets (K <= 1024 = blockDim: one neighbour per thread);
    // counts are clamped to M + 1, so the int sums cannot overflow (<= 1024 * 4097)
    int mycnt = 0;
    if (tid < m) {
        const int64_t b = r_ptr[rows[tid]];
        rbase[tid] = b;
        simv[tid] = sims[tid];
        mycnt = (int32_t)min(r_ptr[rows[tid] + 1] - b, (int64_t)M + 1);
    }
    int Tsum = 0;
    const int myoff = block_exclusive_scan(mycnt, wtot, &Tsum);
    if (tid < m) off[tid] = myoff;
    if (tid == 0) off[m] = Tsum;
    __syncthreads();
    const int T = min(Tsum, M + 1);
    if (T > M) {
        if (tid == 0) {
            out_overflow[q] = 1;
            out_n[q] = 0;
            if (host) {
                *reinterpret_cast<int32_t *>(host + 16) = 1;
                *reinterpret_cast<int64_t *>(host) = 0;
            }
            if (stats && last_pass) atomicAdd(&stats[2], 1ull);
        }
        return;
    }
    if (stats && tid == 0) atomicAdd(&stats[1], 1ull);
    int n2 = 2;
    while (n2 < T) n2 <<= 1;  // <= M
    auto neighbour_of = [&](int f) {  // last i with off[i] <= f
        int a = 0, b = m;
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (off[mid] <= f) a = mid; else b = mid;
        }
        return a;
    };
    // (wrv / av are filled here, by ORIGINAL position f, and read through the sorted key's low bits afterwards: the rating
    // is loaded beside the place index instead of by a second search and a second round trip after the sort)
    for (int f = tid; f < n2; f += blockDim.x) {
        KeyT k = ~(KeyT)0;
        if (f < T) {
            const int a = neighbour_of(f);
            const int64_t e = rbase[a] + (f - off[a]);
            const double sim = simv[a];
            k = ((KeyT)(uint32_t)r_pidx[e] << fbits) | (KeyT)f;
            wrv[f] = r_rating[e] * sim;  // col("rating") * col("similarity") (:59)
            av[f] = (unsigned short)a;
        }
        key[f] = k;
    }
    __syncthreads();
    // Bitonic sort, ascending.  A stage whose partners lie less than C = n2 / waves apart exchanges only inside the
    // chunk of C consecutive keys a wave owns: all such stages of a level run back to back inside the wave (its LDS
    // operations complete in order) and the block meets once behind them - 21 barriers instead of 66 for 2,048 keys
    // on 16 waves, which was most of this kernel's time (1,024 threads per query: a barrier per stage is 16 waves waiting).
    {
        const int nwaves = (int)blockDim.x >> 6, wv = tid >> 6, ln = tid & 63;
        const int C = n2 / nwaves;  // keys per wave chunk (a power of two, possibly < 2)
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                if (j < C) {
                    for (int jj = j; jj > 0; jj >>= 1) {
                        for (int t = ln; t < (C >> 1); t += 64) {
                            const int tt = wv * (C >> 1) + t;
                            const int i = 2 * tt - (tt & (jj - 1));
                            const int l = i + jj;
                            const KeyT ki = key[i], kl = key[l];
                            if ((kl < ki) == ((i & k) == 0)) {
                                key[i] = kl;
                                key[l] = ki;
                            }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                    }
                    break;
                }
                for (int t = tid; t < (n2 >> 1); t += blockDim.x) {
                    const int i = 2 * t - (t & (j - 1));
                    const int l = i + j;
                    const KeyT ki = key[i], kl = key[l];
                    if ((kl < ki) == ((i & k) == 0)) {
                        key[i] = kl;
                        key[l] = ki;
                    }
                }
                __syncthreads();
            }
            __syncthreads();
        }
    }
    // heads per thread (each thread owns n2/blockDim consecutive positions)
    const int per = n2 / (int)blockDim.x > 0 ? n2 / (int)blockDim.x : 1;
    const int lo = tid * per, hi = min(lo + per, T);
    int heads = 0;
    for (int i = lo; i < hi; ++i)
        if (i == 0 || (key[i] >> fbits) != (key[i - 1] >> fbits)) ++heads;
    int nheads = 0;
    int o = block_exclusive_scan(heads, wtot, &nheads);
    if (tid == 0) {
        out_n[q] = nheads;
        out_overflow[q] = 0;
        if (host) {
            *reinterpret_cast<int32_t *>(host + 16) = 0;
            *reinterpret_cast<int64_t *>(host) = nheads;
        }
    }
    int64_t *h_place = host ? reinterpret_cast<int64_t *>(host + 64) : nullptr;
    double *h_est = host ? reinterpret_cast<double *>(host + 64 + (size_t)host_cap * 8) : nullptr;
    for (int i = lo; i < hi; ++i) {
        const KeyT pk = key[i] >> fbits;
        if (i == 0 || pk != (key[i - 1] >> fbits)) {
            double ws = 0.0, ss = 0.0;
            for (int t = i; t < T && (key[t] >> fbits) == pk; ++t) {
                const int f = (int)(key[t] & (((KeyT)1 << fbits) - 1));
                ws = ws + wrv[f];
                ss = ss + simv[av[f]];
            }
            const int64_t place = cplace_ids[pk];
            const double est = ws / ss;   // :67
            out_place[(int64_t)q * out_stride + o] = place;
            out_est[(int64_t)q * out_stride + o] = est;
            if (host) {
                h_place[o] = place;
                h_est[o] = est;
            }
            ++o;
        }
    }
}

// The same aggregation without a sort (pass 1 of every index whose place bitmap fits: knn_agg_plan.h).  The result needs
// the distinct places in ascending compact index, and inside a place its rows summed in ascending position - no total
// order of the rows.  A presence bitmap over the compact place indices gives the first: a place's slot is the rank of its
// bit, already the output order.  A counting bucket per slot gives the second: rows arrive in their bucket in the arbitrary
// order of the LDS atomics, and each then takes the place its position has among the bucket's positions, so the order of
// the fp64 additions is a function of the data alone - the same additions in the same order as knn_aggregate's.
// Same contract as knn_aggregate (one block per query, blockDim >= K, M <= blockDim * kAggPer); a query with more than M
// rows, or with more than bucket_max rows of one place (the ordering step costs their square), is flagged exactly like a
// capacity overflow and redone by knn_aggregate's redo pass.
__global__ __launch_bounds__(kAggThreads) void knn_aggregate_buckets(
    const int32_t *nb_rows, const double *nb_sims, const int64_t *nb_cnt, int32_t K,
    const int64_t *r_ptr, const int32_t *r_pidx, const double *r_rating, const int64_t *cplace_ids,
    int32_t M /* LDS capacity in rows */, int32_t nplaces, int32_t bucket_max, int64_t *out_place, double *out_est,
    int64_t *out_n, int32_t *out_overflow, int64_t out_stride, unsigned char *host, const int32_t *host_flag_src,
    int32_t host_cap, unsigned long long *stats, int32_t last_pass)
{
    if (host && threadIdx.x == 0 && host_flag_src) *reinterpret_cast<int32_t *>(host + 20) = *host_flag_src;
    extern __shared__ __align__(16) unsigned char smem[];
    const KnnAggBucketLds L = knn_agg_bucket_lds(M, K, nplaces);
    // (bitmap and prefix share their bytes with sprod and snb: the former are last read in phase 5, the latter first
    // written in phase 6, behind two block barriers - knn_agg_bucket_lds)
    double *sprod = reinterpret_cast<double *>(smem + L.prod);            // [M] rating * similarity, bucket after bucket
    int32_t *start = reinterpret_cast<int32_t *>(smem + L.start);         // [M + 1] rows per slot, then first row of the slot
    int32_t *splace = reinterpret_cast<int32_t *>(smem + L.place);        // [M] compact place index of the slot
    unsigned short *entry = reinterpret_cast<unsigned short *>(smem + L.entry);  // [M] positions, bucket after bucket, unordered
    unsigned short *snb = reinterpret_cast<unsigned short *>(smem + L.nb);       // [M] neighbour of the ordered row
    uint32_t *bitmap = reinterpret_cast<uint32_t *>(smem + L.bitmap);     // [words] places present
    unsigned short *prefix = reinterpret_cast<unsigned short *>(smem + L.prefix);  // [words] set bits before the word
    int64_t *rbase = reinterpret_cast<int64_t *>(smem + L.neighbours);    // [K] first rating row of neighbour i
    double *simv = reinterpret_cast<double *>(rbase + K);                 // [K]
    int32_t *off = reinterpret_cast<int32_t *>(simv + K);                 // [K+1] prefix of neighbour row counts
    const int q = blockIdx.x;
    const int tid = threadIdx.x, nthreads = (int)blockDim.x;
    const int m = max(0, (int)nb_cnt[q]);
    const int32_t *rows = nb_rows + (int64_t)q * K;
    const double *sims = nb_sims + (int64_t)q * K;
    const int cap = min(M, nthreads * kAggPer);
    const int nwords = knn_agg_words(nplaces);
    __shared__ int wtot[17];
    for (int w = tid; w < nwords; w += nthreads) bitmap[w] = 0u;
    // 1. neighbour row counts -> exclusive offsets, as knn_aggregate
    int mycnt = 0;
    if (tid < m) {
        const int64_t b = r_ptr[rows[tid]];
        rbase[tid] = b;
        simv[tid] = sims[tid];
        mycnt = (int32_t)min(r_ptr[rows[tid] + 1] - b, (int64_t)cap + 1);
    }
    int Tsum = 0;
    const int myoff = block_exclusive_scan(mycnt, wtot, &Tsum);
    if (tid < m) off[tid] = myoff;
    if (tid == 0) off[m] = Tsum;
    __syncthreads();
    auto flag_query = [&]() {
        if (tid == 0) {
            out_overflow[q] = 1;
            out_n[q] = 0;
            if (host) {
                *reinterpret_cast<int32_t *>(host + 16) = 1;
                *reinterpret_cast<int64_t *>(host) = 0;
            }
            if (stats && last_pass) atomicAdd(&stats[2], 1ull);
        }
    };
    const int T = min(Tsum, cap + 1);
    if (T > cap) {
        flag_query();
        return;
    }
    auto neighbour_of = [&](int f) {  // last i with off[i] <= f
        int a = 0, b = m;
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (off[mid] <= f) a = mid; else b = mid;
        }
        return a;
    };
    // 3. gather: position f = tid + j * blockDim stays in registers (place index, product, neighbour); its place's bit is set
    int32_t pidx[kAggPer], nbr[kAggPer];
    double prod[kAggPer];
    int bad = 0;
#pragma unroll
    for (int j = 0; j < kAggPer; ++j) {
        const int f = tid + j * nthreads;
        pidx[j] = -1;
        nbr[j] = 0;
        prod[j] = 0.0;
        if (f < T) {
            const int a = neighbour_of(f);
            const int64_t e = rbase[a] + (f - off[a]);
            const int32_t p = r_pidx[e];
            if ((uint32_t)p < (uint32_t)nplaces) {
                pidx[j] = p;
                nbr[j] = a;
                prod[j] = r_rating[e] * simv[a];  // col("rating") * col("similarity") (:59)
                atomicOr(&bitmap[knn_agg_word_of((uint32_t)p)], knn_agg_bit_of((uint32_t)p));
            } else {
                bad = 1;  // (no index holds such a row; the sort form does not index LDS by it)
            }
        }
    }
    __syncthreads();
    // 4. rank: exclusive popcount prefix over the words, consecutive words per thread; the total is the number of places
    const int wpt = knn_agg_words_per_thread(nwords, nthreads);
    const int w0 = min(tid * wpt, nwords), w1 = min(w0 + wpt, nwords);
    int pc = 0;
    for (int w = w0; w < w1; ++w) pc += __popc(bitmap[w]);
    int nslots = 0;
    int run = block_exclusive_scan(pc, wtot, &nslots);
    for (int w = w0; w < w1; ++w) {
        prefix[w] = (unsigned short)run;
        run += __popc(bitmap[w]);
    }
    for (int s = tid; s <= nslots; s += nthreads) start[s] = 0;
    __syncthreads();
    // 5. bucket: rows per slot (the arrival number only places the row inside its bucket), exclusive scan, scatter
    int32_t slot[kAggPer], arrival[kAggPer];
#pragma unroll
    for (int j = 0; j < kAggPer; ++j) {
        slot[j] = 0;
        arrival[j] = 0;
        if (pidx[j] >= 0) {
            const int w = knn_agg_word_of((uint32_t)pidx[j]);
            slot[j] = knn_agg_slot(prefix[w], bitmap[w], (uint32_t)pidx[j]);
            arrival[j] = atomicAdd(&start[slot[j]], 1);
        }
    }
    __syncthreads();
    const int per = max(1, (cap + nthreads - 1) / nthreads);
    const int lo = min(tid * per, nslots), hi = min(lo + per, nslots);
    int mine = 0;
    for (int s = lo; s < hi; ++s) {
        const int c = start[s];
        mine += c;
        bad |= c > bucket_max;
    }
    int total = 0;
    int first = block_exclusive_scan(mine, wtot, &total);
    for (int s = lo; s < hi; ++s) {
        const int c = start[s];
        start[s] = first;
        first += c;
    }
    if (tid == 0) start[nslots] = total;
    if (__syncthreads_or(bad)) {
        flag_query();
        return;
    }
#pragma unroll
    for (int j = 0; j < kAggPer; ++j)
        if (pidx[j] >= 0) {
            entry[start[slot[j]] + arrival[j]] = (unsigned short)(tid + j * nthreads);
            splace[slot[j]] = pidx[j];  // (every row of the slot writes the same value)
        }
    __syncthreads();
    // 6. order: a row's place inside its bucket = the bucket's positions below its own
#pragma unroll
    for (int j = 0; j < kAggPer; ++j)
        if (pidx[j] >= 0) {
            const int f = tid + j * nthreads;
            const int b = start[slot[j]], e = start[slot[j] + 1];
            int r = b;
            for (int i = b; i < e; ++i) r += (int)entry[i] < f;
            sprod[r] = prod[j];
            snb[r] = (unsigned short)nbr[j];
        }
    __syncthreads();
    // 7. sum: one thread per slot, left to right in position order
    if (tid == 0) {
        out_n[q] = nslots;
        out_overflow[q] = 0;
        if (host) {
            *reinterpret_cast<int32_t *>(host + 16) = 0;
            *reinterpret_cast<int64_t *>(host) = nslots;
        }
        if (stats) atomicAdd(&stats[0], 1ull);
    }
    int64_t *h_place = host ? reinterpret_cast<int64_t *>(host + 64) : nullptr;
    double *h_est = host ? reinterpret_cast<double *>(host + 64 + (size_t)host_cap * 8) : nullptr;
    for (int s = tid; s < nslots; s += nthreads) {
        double ws = 0.0, ss = 0.0;
        for (int t = start[s], e = start[s + 1]; t < e; ++t) {
            ws = ws + sprod[t];
            ss = ss + simv[snb[t]];
        }
        const int64_t place = cplace_ids[splace[s]];
        const double est = ws / ss;   // :67
        out_place[(int64_t)q * out_stride + s] = place;
        out_est[(int64_t)q * out_stride + s] = est;
        if (host) {
            h_place[s] = place;
            h_est[s] = est;
        }
    }
}

// rows of query q (out_n[q] of them, at q * stride) -> dense[off[q] ..): one block per query
__global__ __launch_bounds__(256) void knn_agg_compact(const int64_t *place, const double *est, const int64_t *out_n,
                                                       const int64_t *off, int64_t stride, int64_t *dense_place,
                                                       double *dense_est)
{
    const int q = blockIdx.x;
    const int64_t n = out_n[q], o = off[q];
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        dense_place[o + i] = place[(int64_t)q * stride + i];
        dense_est[o + i] = est[(int64_t)q * stride + i];
    }
}

// Range / all-pairs forms: a person whose place or category vector is empty is a legitimate
// candidate of the reference's outer join but not a valid QUERY (KnnRecommender.scala:77-83 throws
// "No such person" for it): its list is reported with count -1 instead of failing the whole batch.
__global__ void knn_mark_absent(const double *norm_p, const double *norm_c, const int32_t *qrows, int32_t qrow0,
                                int32_t nq, int32_t K, int64_t *out_ids, double *out_sims, int32_t *out_rows,
                                int64_t *out_cnt)
{
    const int q = blockIdx.x;
    if (q >= nq) return;
    const int row = qrows ? qrows[q] : qrow0 + q;
    if (norm_p[row] > 0.0 && norm_c[row] > 0.0) return;
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        out_ids[(int64_t)q * K + i] = -1;
        out_sims[(int64_t)q * K + i] = 0.0;
        out_rows[(int64_t)q * K + i] = -1;
    }
    if (threadIdx.x == 0) out_cnt[q] = -1;
}
