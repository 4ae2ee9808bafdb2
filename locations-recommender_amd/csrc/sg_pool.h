// sg_pool.h -- a pool of resident graphs that serves ONE mixed batch of (graph, vertex) requests (locrec_sg_pool_*).
// Included at the end of sg_batch.hip.
//
// The reference keeps one stochastic graph per region and per pair of regions (PlaceVisits.scala:63-67) and sends every
// input line to the graph of sorted{home, target} (StochasticRecommenderMain.scala:53-62): a serving process sees requests
// that fan out over many graphs, most of them small.  locrec_sg_recommend_batch shares the sweeps of ONE graph's targets;
// a loop over graphs still pays every graph's set-up launch, polls, read-back and two launches per round.  The pool runs
// the graphs' tiles side by side:
//
//   tile wave k   the k-th tile (sg_batch_tile_max targets) of every graph that still has one; a graph whose targets are
//                 used up contributes neither rows to the tables nor blocks to the launches
//   set-up        ONE sg_begin_pool launch per tile wave, blockIdx.y = the graph's row of a table of SgBatchBegin
//   sweep         per round ONE sg_sweep_pool launch per layout class of the wave - column width {uint16, int32} x weight
//                 form {dictionary, fp64 stream}: at most four, one for a homogeneous pool.  A block finds its graph by a
//                 scalar bisection over the block bases of the class's view table; a graph's range is whole blocks
//                 ((npieces + 3) / 4 of them), because in the dictionary classes a block loads ONE graph's table into LDS
//   finalize      ONE sg_finalize_pool launch per round, grid (kParts, graphs of the wave)
//   poll          ONE sg_poll_pool launch on sg_batch_tiles' schedule: every tile's all_done, ANDed, into a pinned word
//   read-back     ONE sg_pack_pool launch per tile wave: every graph's packed image (sg_pack_batch's) at the graph's offset
//                 of the pool's pinned buffer, one synchronisation; then sg_batch_host_rows per graph.  What happens to a
//                 finished wave is a parameter of sg_pool_waves: the ranked pool (sg_pool_ranked.h) emits and ranks instead
//   columns       what a member's columns are is a parameter too (sg_pool_waves_of's tiles policy): the distinct vertices
//                 asked of it (SgPoolPersonTiles), or its visitors (SgPoolVisitorTiles, sg_pool_visitors.h), which add one
//                 set-up launch per wave and finalize with their own kernel
//
// The bodies are sg_batch.hip's (sg_sweep_batch_body and friends), on each graph's own batch buffers (PA4 / XL / D2W /
// fused_conv) - the order of operations per column is the batch's, which is the single request's: request i's rows are
// bit for bit what locrec_sg_recommend returns for that vertex on that graph.
//
// VGPRs (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) stand in DESIGN.md section 4, "Pools of graphs"; no kernel
// of this file uses scratch.

namespace {

// A graph's row of its layout class's sweep table (sorted by block_base)
struct SgPoolView {
    const void *colv;
    const v2d *w2;
    const v4h *widx;
    const double *dict;
    const int2 *pinfo;
    const int32_t *seg_out;
    const double *xbuf;  // both parities
    double *partial;
    const SgBatchState *st;
    int64_t xstride;
    int32_t ndict, npieces, block_base, pad;
};

// A graph's row of the tile wave's table: what its finalize, the poll and its share of the pack launch need
struct SgPoolTile {
    SgBatchReq rq;
    const int4 *lrows;
    const double *partial;
    double *xbuf;   // both parities
    double *parts;  // both parities' block sums
    SgBatchState *st;
    int64_t xstride;
    int64_t pack_off;  // of this graph's packed image in the pool's pinned buffer
    int32_t n_short, nlrows, n_crows, pad;
};

template <bool COL16, bool DICT>
__global__ __launch_bounds__(256) void sg_sweep_pool(const SgPoolView *__restrict__ V, const int32_t nviews, const int32_t par)
{
    const int bx = (int)blockIdx.x;
    // the last graph whose block range starts at or before bx (as sg_sweep_group finds its graph by waves)
    int gi = 0, hi = nviews;
    while (hi - gi > 1) {
        const int mid = (gi + hi) >> 1;
        if (V[mid].block_base <= bx) gi = mid; else hi = mid;
    }
    const SgPoolView &v = V[gi];
    sg_sweep_batch_body<COL16, DICT>(v.colv, v.w2, v.widx, v.dict, v.ndict, v.pinfo, v.seg_out, v.xbuf + (size_t)par * v.xstride,
                                     v.partial, v.npieces, v.st, bx - v.block_base);
}

__global__ __launch_bounds__(256) void sg_finalize_pool(const SgPoolTile *__restrict__ tiles, const int32_t par, const int32_t first)
{
    const SgPoolTile &t = tiles[blockIdx.y];
    sg_finalize_batch_body(t.rq, (int)blockIdx.x, t.n_short, t.lrows, t.nlrows, t.n_crows, t.partial, t.xbuf + (size_t)par * t.xstride,
                           t.xbuf + (size_t)(par ^ 1) * t.xstride, t.parts + (size_t)(par ^ 1) * kParts * kBatchB,
                           t.parts + (size_t)par * kParts * kBatchB, t.st, first);
}

__global__ __launch_bounds__(256) void sg_begin_pool(const SgBatchBegin *__restrict__ tab) { sg_begin_batch_body(tab[blockIdx.y]); }

// *out = 1 when every tile of the wave has all its columns done (one wave of threads)
__global__ __launch_bounds__(64) void sg_poll_pool(const SgPoolTile *__restrict__ tiles, const int32_t ntiles, int32_t *out)
{
    int all = 1;
    for (int i = (int)threadIdx.x; i < ntiles; i += 64) all &= tiles[i].st->all_done != 0 ? 1 : 0;
    all = __all(all) ? 1 : 0;
    if (threadIdx.x == 0) *out = all;
}

__global__ __launch_bounds__(256) void sg_pack_pool(const SgPoolTile *__restrict__ tiles, unsigned char *out)
{
    const SgPoolTile &t = tiles[blockIdx.y];
    sg_pack_batch_body(t.st, t.parts, t.xbuf, t.xstride, t.rq.T + 1, out + t.pack_off);
}

struct SgPoolStats {
    int64_t tile_waves = 0, rounds = 0, sweep_launches = 0, finalize_launches = 0, polls = 0, readback_bytes = 0;
};

SgPoolStats &sg_pool_stats()
{
    thread_local SgPoolStats st;
    return st;
}

inline size_t sg_pool_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// a member's row of a visitors wave, beside its SgPoolTile row: sizeof(SgPoolVisRow), sg_pool_visitors.h (asserted there)
constexpr size_t kSgPoolVisRowBytes = 88;

}  // namespace

struct locrec_sg_pool {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;              // end of a call's launches: the members' own streams wait for it
    std::vector<locrec_sg_graph *> graphs;  // not owned
    bool no_pack = false;                   // a member was created under LOCREC_SG_NO_PACK: plain copies
    // the tables of a tile wave: one host image and one device buffer (SgPoolTile rows, SgBatchBegin rows, the four
    // classes' SgPoolView rows, then - a visitors call only - the SgPoolVisRow rows), one copy per wave; sized by the
    // number of members
    std::vector<unsigned char> tab_host;
    DevBuf<unsigned char> tab_dev;
    size_t off_begin = 0, off_views = 0, off_vis = 0;
    unsigned char *h_pack = nullptr;  // pinned: every member's packed image side by side
    unsigned char *h_pack_dev = nullptr;
    size_t h_pack_bytes = 0;
    int32_t *h_poll = nullptr;  // pinned: sg_poll_pool's answer
    int32_t *h_poll_dev = nullptr;
    DevBuf<int32_t> poll_word;  // ... where the pinned word has no device address
    std::shared_ptr<void> ranked;  // the members' resident emit-row images (sg_pool_ranked.h), built at their first ranked call
    ~locrec_sg_pool()
    {
        if (done) (void)hipEventDestroy(done);
        if (h_pack) (void)hipHostFree(h_pack);
        if (h_poll) (void)hipHostFree(h_poll);
        if (stream) (void)hipStreamDestroy(stream);
    }
    // grow-only, as locrec_sg_graph::stage
    void pack_room(size_t bytes)
    {
        if (no_pack || h_pack_bytes >= bytes) return;
        if (h_pack) (void)hipHostFree(h_pack);
        h_pack = h_pack_dev = nullptr;
        h_pack_bytes = 0;
        void *p = nullptr, *dp = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) {
            if (hipHostGetDevicePointer(&dp, p, 0) == hipSuccess) {
                h_pack = static_cast<unsigned char *>(p);
                h_pack_dev = static_cast<unsigned char *>(dp);
                h_pack_bytes = bytes;
                return;
            }
            (void)hipHostFree(p);
        }
        (void)hipGetLastError();
    }
};

extern "C" int32_t locrec_sg_pool_create(locrec_sg_graph *const *graphs, int32_t n_graphs, locrec_sg_pool **out) try
{
    if (!out) return fail(LOCREC_E_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!graphs || n_graphs <= 0 || n_graphs > 65535) return fail(LOCREC_E_INVALID_ARG, "a pool needs 1 .. 65535 graphs");
    auto pool = std::make_unique<locrec_sg_pool>();
    size_t pack_bytes = 0;
    for (int32_t i = 0; i < n_graphs; ++i) {
        locrec_sg_graph *g = graphs[i];
        if (!g) return fail(LOCREC_E_INVALID_ARG, "graph %d is NULL", i);
        for (int32_t j = 0; j < i; ++j)
            if (graphs[j] == g) return fail(LOCREC_E_INVALID_ARG, "graph %d appears twice in the pool", i);
        if (const char *why = sg_batch_refusal(g)) return fail(LOCREC_E_INVALID_ARG, "graph %d: %s", i, why);
        if (g->ppw != 1 || g->gs_blocks > 0)
            return fail(LOCREC_E_INVALID_ARG, "graph %d was created with a non-default sweep form (LOCREC_SG_PPW / LOCREC_SG_GS)", i);
        if (i == 0) pool->device = g->device;
        else if (g->device != pool->device) return fail(LOCREC_E_INVALID_ARG, "graph %d lives on another device", i);
        pool->no_pack |= g->no_pack;
        pack_bytes += sg_pool_align(sg_batch_pack_bytes(g->nlive));
        pool->graphs.push_back(g);
    }
    LOCREC_HIP_TRY(hipSetDevice(pool->device));
    LOCREC_HIP_TRY(hipStreamCreateWithFlags(&pool->stream, hipStreamNonBlocking));
    LOCREC_HIP_TRY(hipEventCreateWithFlags(&pool->done, hipEventDisableTiming));
    const size_t n = (size_t)n_graphs;
    pool->off_begin = sg_pool_align(n * sizeof(SgPoolTile));
    pool->off_views = pool->off_begin + sg_pool_align(n * sizeof(SgBatchBegin));
    pool->off_vis = pool->off_views + sg_pool_align(n * sizeof(SgPoolView));
    pool->tab_host.assign(pool->off_vis + n * kSgPoolVisRowBytes, 0);
    LOCREC_TRY(pool->tab_dev.alloc(pool->tab_host.size()));
    LOCREC_TRY(pool->poll_word.alloc(1));
    pool->pack_room(pack_bytes);  // (a tile wave holds at most every member once)
    if (!pool->no_pack) {
        void *hp = nullptr, *dp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocDefault) == hipSuccess) {
            pool->h_poll = static_cast<int32_t *>(hp);
            if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) pool->h_poll_dev = static_cast<int32_t *>(dp);
        }
        (void)hipGetLastError();
    }
    *out = pool.release();
    return LOCREC_OK;
} LOCREC_CATCH_ALL

extern "C" void locrec_sg_pool_destroy(locrec_sg_pool *pool)
{
    if (!pool) return;
    (void)hipSetDevice(pool->device);
    if (pool->stream) (void)hipStreamSynchronize(pool->stream);
    delete pool;
}

extern "C" int32_t locrec_sg_pool_stats(int64_t *out_tile_waves, int64_t *out_rounds, int64_t *out_sweep_launches,
                                        int64_t *out_finalize_launches, int64_t *out_polls, int64_t *out_readback_bytes)
{
    const SgPoolStats &st = sg_pool_stats();
    if (out_tile_waves) *out_tile_waves = st.tile_waves;
    if (out_rounds) *out_rounds = st.rounds;
    if (out_sweep_launches) *out_sweep_launches = st.sweep_launches;
    if (out_finalize_launches) *out_finalize_launches = st.finalize_launches;
    if (out_polls) *out_polls = st.polls;
    if (out_readback_bytes) *out_readback_bytes = st.readback_bytes;
    return LOCREC_OK;
}

namespace {

// A member's share of one call
struct SgPoolMember {
    std::vector<int32_t> uniq;                 // vertex index of each distinct target, in order of appearance
    std::unordered_map<int32_t, int32_t> seen;  // vertex index -> its entry of uniq
    std::vector<SlotRange> pointed;            // slot ranges that point at a private row (or at Q) and go back to D next
    SgBatchRows res;
    std::vector<double> both;  // the plain-copy path's two parities of x
};

// A tile wave whose last round has been launched: what its consumer gets
struct SgPoolWave {
    size_t k;                             // the wave: member j iterates its targets uniq[k * tile_max ..)
    const std::vector<int32_t> &members;  // in member order
    const std::vector<int> &nb;           // targets of each member's tile
    const SgPoolTile *tiles, *tiles_dev;  // the wave's table, a row per member
    size_t pack_bytes;                    // of all packed images side by side
    unsigned pack_blocks;
};

// What the columns of a pool call's tiles are: distinct vertices of the members (here), or visitors (SgPoolVisitorTiles,
// sg_pool_visitors.h).  Member gi has mem[gi].uniq.size() columns either way.
struct SgPoolPersonTiles {
    int tile_max(const locrec_sg_graph *g) const { return sg_batch_tile_max(g); }
    // the set-up and finalize rows of member gi's tile of wave k: its columns t0 .. t0 + nb
    void rows(int32_t, const locrec_sg_graph *g, SgPoolMember &m, size_t, size_t t0, int nb, double alpha, double eps2, SgBatchBegin &b,
              SgBatchReq &rq) const
    {
        sg_batch_tile_rows(g, m.uniq, t0, nb, alpha, eps2, m.pointed, b, rq);
    }
    void member_row(locrec_sg_pool *, unsigned, int32_t, size_t) const {}  // (rows of the wave's table beside SgPoolTile's: none)
    // bytes of the wave's table that travel to the device
    size_t table_bytes(const locrec_sg_pool *pool, size_t nviews, unsigned) const { return pool->off_views + nviews * sizeof(SgPoolView); }
    void set_up(locrec_sg_pool *, hipStream_t, unsigned) const {}  // (launches behind the wave's sg_begin_pool: none)
    void finalize(locrec_sg_pool *, hipStream_t s, unsigned nw, const SgPoolTile *tiles_dev, int par, int32_t first) const
    {
        hipLaunchKernelGGL(sg_finalize_pool, dim3(kParts, nw), dim3(256), 0, s, tiles_dev, par, first);
    }
};

// Every tile wave of a call: set-up, rounds and polls, then consume(wave) - after the wave's last round and before the
// next wave's set-up overwrites x and the tables; it returns with the stream synchronised.  `act` lists the members with
// requests, `tp` says what their columns are.
template <class Tiles, class Consume>
int32_t sg_pool_waves_of(locrec_sg_pool *pool, const std::vector<int32_t> &act, std::vector<SgPoolMember> &mem, Tiles &&tp,
                         double alpha, double epsilon, int64_t max_iterations, SgPoolStats &stats, Consume &&consume)
{
    hipStream_t s = pool->stream;
    const double eps2 = epsilon * epsilon;  // :40
    const bool poll = epsilon > 0 && max_iterations > 4;
    size_t nwaves = 0;
    for (const int32_t gi : act) {
        const size_t tm = (size_t)tp.tile_max(pool->graphs[(size_t)gi]);
        nwaves = std::max(nwaves, (mem[(size_t)gi].uniq.size() + tm - 1) / tm);
    }
    SgPoolTile *tiles = reinterpret_cast<SgPoolTile *>(pool->tab_host.data());
    SgBatchBegin *begins = reinterpret_cast<SgBatchBegin *>(pool->tab_host.data() + pool->off_begin);
    SgPoolView *views = reinterpret_cast<SgPoolView *>(pool->tab_host.data() + pool->off_views);
    const SgPoolTile *tiles_dev = reinterpret_cast<const SgPoolTile *>(pool->tab_dev.p);
    const SgBatchBegin *begins_dev = reinterpret_cast<const SgBatchBegin *>(pool->tab_dev.p + pool->off_begin);
    const SgPoolView *views_dev = reinterpret_cast<const SgPoolView *>(pool->tab_dev.p + pool->off_views);
    std::vector<int32_t> wave;  // the members of this tile wave
    std::vector<int> wave_nb;
    for (size_t k = 0; k < nwaves; ++k) {
        wave.clear();
        wave_nb.clear();
        for (const int32_t gi : act) {
            const size_t tm = (size_t)tp.tile_max(pool->graphs[(size_t)gi]), nu = mem[(size_t)gi].uniq.size();
            if (k * tm < nu) {
                wave.push_back(gi);
                wave_nb.push_back((int)std::min(tm, nu - k * tm));
            }
        }
        const unsigned nw = (unsigned)wave.size();
        // the tables: a row per member for set-up, finalize and pack, and a row of its layout class's sweep table
        size_t pack_bytes = 0;
        unsigned pack_blocks = 1;
        int class_n[4] = {0, 0, 0, 0}, class_blocks[4] = {0, 0, 0, 0}, class_ndict[4] = {0, 0, 0, 0}, class_at[4];
        auto class_of = [](const locrec_sg_graph *g) { return (g->use16 ? 0 : 2) + (g->ndict > 0 ? 0 : 1); };
        for (unsigned j = 0; j < nw; ++j) {
            const locrec_sg_graph *g = pool->graphs[(size_t)wave[j]];
            if (g->npieces > 0) ++class_n[class_of(g)];
        }
        class_at[0] = 0;
        for (int c = 1; c < 4; ++c) class_at[c] = class_at[c - 1] + class_n[c - 1];
        int class_fill[4] = {0, 0, 0, 0};
        for (unsigned j = 0; j < nw; ++j) {
            locrec_sg_graph *g = pool->graphs[(size_t)wave[j]];
            SgPoolMember &m = mem[(size_t)wave[j]];
            const size_t t0 = k * (size_t)tp.tile_max(g);
            SgPoolTile &t = tiles[j];
            tp.rows(wave[j], g, m, k, t0, wave_nb[j], alpha, eps2, begins[j], t.rq);
            tp.member_row(pool, j, wave[j], k);
            t.lrows = g->lrows.p;
            t.partial = g->XL.p;
            t.xbuf = g->PA4.p;
            t.parts = g->D2W.p;
            t.st = reinterpret_cast<SgBatchState *>(g->fused_conv.p);
            t.xstride = sg_batch_xstride(g);
            t.pack_off = (int64_t)pack_bytes;
            t.n_short = g->n_short;
            t.nlrows = g->nlrows;
            t.n_crows = g->n_crows;
            t.pad = 0;
            pack_bytes += sg_pool_align(sg_batch_pack_bytes(g->nlive));
            pack_blocks = std::max(pack_blocks, sg_batch_pack_blocks(g->nlive));
            if (g->npieces > 0) {
                const int c = class_of(g);
                SgPoolView &v = views[class_at[c] + class_fill[c]++];
                v.colv = sg_batch_columns(g);
                v.w2 = reinterpret_cast<const v2d *>(g->w2.p);
                v.widx = reinterpret_cast<const v4h *>(g->widx.p);
                v.dict = g->dict.p;
                v.pinfo = g->pinfo.p;
                v.seg_out = g->seg_out.p;
                v.xbuf = g->PA4.p;
                v.partial = g->XL.p;
                v.st = t.st;
                v.xstride = t.xstride;
                v.ndict = g->ndict;
                v.npieces = g->npieces;
                v.block_base = class_blocks[c];
                v.pad = 0;
                class_blocks[c] += (g->npieces + 3) / 4;  // whole blocks: a block's four waves belong to one graph
                class_ndict[c] = std::max(class_ndict[c], g->ndict);
            }
        }
        const size_t nviews = (size_t)(class_at[3] + class_n[3]);
        LOCREC_HIP_TRY(hipMemcpyAsync(pool->tab_dev.p, pool->tab_host.data(), tp.table_bytes(pool, nviews, nw), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(sg_begin_pool, dim3(kBeginBlocks, nw), dim3(256), 0, s, begins_dev);
        tp.set_up(pool, s, nw);
        ++stats.tile_waves;
        auto launch_round = [&](int64_t i) {
            const int par = (int)(i & 1);
#define LOCREC_SWEEP_POOL(CLS, C16, DICT)                                                                                   \
    if (class_n[CLS] > 0) {                                                                                                 \
        hipLaunchKernelGGL((sg_sweep_pool<C16, DICT>), dim3((unsigned)class_blocks[CLS]), dim3(256),                       \
                           DICT ? (size_t)class_ndict[CLS] * sizeof(double) : 0, s, views_dev + class_at[CLS], class_n[CLS], par); \
        ++stats.sweep_launches;                                                                                             \
    }
            LOCREC_SWEEP_POOL(0, true, true)
            LOCREC_SWEEP_POOL(1, true, false)
            LOCREC_SWEEP_POOL(2, false, true)
            LOCREC_SWEEP_POOL(3, false, false)
#undef LOCREC_SWEEP_POOL
            tp.finalize(pool, s, nw, tiles_dev, par, i == 0 ? 1 : 0);
            ++stats.finalize_launches;
            ++stats.rounds;
        };
        // step() (:92-106) for every column of every tile; the host looks at "all tiles done" on sg_batch_tiles' schedule
        int64_t next_check = 4;
        for (int64_t i = 0; i < max_iterations;) {
            const int64_t stop = poll ? std::min(max_iterations, next_check) : max_iterations;
            for (int64_t r = i; r < stop; ++r) launch_round(r);
            i = stop;
            if (poll && stop == next_check && stop < max_iterations) {
                int32_t all_done = 0;
                if (pool->h_poll_dev) {
                    hipLaunchKernelGGL(sg_poll_pool, dim3(1), dim3(64), 0, s, tiles_dev, (int32_t)nw, pool->h_poll_dev);
                    LOCREC_HIP_TRY(hipStreamSynchronize(s));
                    all_done = *pool->h_poll;
                } else {
                    hipLaunchKernelGGL(sg_poll_pool, dim3(1), dim3(64), 0, s, tiles_dev, (int32_t)nw, pool->poll_word.p);
                    LOCREC_HIP_TRY(hipMemcpyAsync(&all_done, pool->poll_word.p, sizeof all_done, hipMemcpyDeviceToHost, s));
                    LOCREC_HIP_TRY(hipStreamSynchronize(s));
                }
                ++stats.polls;
                if (all_done) break;
                next_check += next_check < 8 ? 2 : (next_check < 16 ? 4 : kCheckEvery);
            }
        }
        LOCREC_TRY(consume(SgPoolWave{k, wave, wave_nb, tiles, tiles_dev, pack_bytes, pack_blocks}));
    }
    return LOCREC_OK;
}

// ... of the members' distinct targets
template <class Consume>
int32_t sg_pool_waves(locrec_sg_pool *pool, const std::vector<int32_t> &act, std::vector<SgPoolMember> &mem, double alpha,
                      double epsilon, int64_t max_iterations, SgPoolStats &stats, Consume &&consume)
{
    return sg_pool_waves_of(pool, act, mem, SgPoolPersonTiles{}, alpha, epsilon, max_iterations, stats, consume);
}

// Every graph index of a call (its requests, or its visitors) names a member.  *out_bad: the position of the first that does not
int32_t sg_pool_graph_indices(const locrec_sg_pool *pool, int64_t n, const int32_t *graph_index, int64_t *out_bad)
{
    const int32_t ng = (int32_t)pool->graphs.size();
    for (int64_t i = 0; i < n; ++i)
        if (graph_index[i] < 0 || graph_index[i] >= ng) {
            if (out_bad) *out_bad = i;
            return fail(LOCREC_E_INVALID_ARG, "request %lld names graph %d: the pool holds graphs 0 .. %d", (long long)i,
                        graph_index[i], ng - 1);
        }
    return LOCREC_OK;
}

// Every graph index, then isVertexExist (:70-77) for every request, before any device work: the members' distinct
// targets, the members with requests (`act`, in order of appearance) and request -> its entry of its member's uniq.  On a
// refusal nothing is written but *out_bad_request (when given): the position of the first offending request; else -1.
int32_t sg_pool_requests(const locrec_sg_pool *pool, int64_t n_requests, const int32_t *graph_index, const int64_t *vertex_ids,
                         std::vector<SgPoolMember> &mem, std::vector<int32_t> &act, std::vector<int32_t> &uniq_of,
                         int64_t *out_bad_request)
{
    const int32_t ng = (int32_t)pool->graphs.size();
    LOCREC_TRY(sg_pool_graph_indices(pool, n_requests, graph_index, out_bad_request));
    mem = std::vector<SgPoolMember>((size_t)ng);
    act.clear();
    uniq_of.assign((size_t)n_requests, 0);
    for (int64_t i = 0; i < n_requests; ++i) {
        const int32_t tv = sg_vertex_index(pool->graphs[(size_t)graph_index[i]], vertex_ids[i]);
        if (tv < 0) {
            if (out_bad_request) *out_bad_request = i;
            return fail(LOCREC_E_NOT_FOUND, "No such vertex in the graph: %lld", (long long)vertex_ids[i]);
        }
        SgPoolMember &m = mem[(size_t)graph_index[i]];
        if (m.uniq.empty()) act.push_back(graph_index[i]);
        auto ins = m.seen.emplace(tv, (int32_t)m.uniq.size());
        if (ins.second) m.uniq.push_back(tv);
        uniq_of[(size_t)i] = ins.first->second;
    }
    if (out_bad_request) *out_bad_request = -1;
    return LOCREC_OK;
}

// In front of a call's waves: the members' own work is over, `act` is in member order, its members have their batch
// buffers and their patched slots are the call's
int32_t sg_pool_begin_call(locrec_sg_pool *pool, std::vector<int32_t> &act, std::vector<SgPoolMember> &mem)
{
    LOCREC_HIP_TRY(hipSetDevice(pool->device));
    // whatever the members were doing on their own streams is over before the pool's first launch
    for (locrec_sg_graph *g : pool->graphs) LOCREC_HIP_TRY(hipStreamSynchronize(g->stream));
    std::sort(act.begin(), act.end());  // member order: the tables' rows and the launches' blocks follow it
    for (const int32_t gi : act) {
        locrec_sg_graph *g = pool->graphs[(size_t)gi];
        LOCREC_TRY(sg_batch_buffers(g, pool->stream));
        sg_batch_take_patched(g, mem[(size_t)gi].pointed);
    }
    return LOCREC_OK;
}

// Behind a call's waves, whatever their status: every member's slots back at D, the members' streams behind the pool's
int32_t sg_pool_end_call(locrec_sg_pool *pool, const std::vector<int32_t> &act, const std::vector<SgPoolMember> &mem,
                         int32_t status)
{
    hipStream_t s = pool->stream;
    // every member's slots back at D in one more set-up launch: its column array is as a fresh handle's
    {
        SgBatchBegin *begins = reinterpret_cast<SgBatchBegin *>(pool->tab_host.data() + pool->off_begin);
        unsigned nr = 0;
        for (const int32_t gi : act)
            if (!mem[(size_t)gi].pointed.empty()) sg_batch_restore_row(pool->graphs[(size_t)gi], mem[(size_t)gi].pointed, begins[nr++]);
        if (nr > 0) {
            // (the last wave's consumer has synchronised the stream: nothing reads the tables any more)
            const hipError_t e = hipMemcpyAsync(pool->tab_dev.p + pool->off_begin, begins, nr * sizeof(SgBatchBegin),
                                                hipMemcpyHostToDevice, s);
            if (e == hipSuccess)
                hipLaunchKernelGGL(sg_begin_pool, dim3(kBeginBlocks, nr), dim3(256), 0, s,
                                   reinterpret_cast<const SgBatchBegin *>(pool->tab_dev.p + pool->off_begin));
            else if (status == LOCREC_OK)
                status = fail(LOCREC_E_DEVICE, "hipMemcpyAsync failed: %s", hipGetErrorName(e));
        }
    }
    // a request on a member synchronises ITS stream: make that stream wait for the pool's launches (as group_run does)
    LOCREC_HIP_TRY(hipEventRecord(pool->done, s));
    for (locrec_sg_graph *g : pool->graphs) LOCREC_HIP_TRY(hipStreamWaitEvent(g->stream, pool->done, 0));
    LOCREC_TRY(status);
    LOCREC_HIP_TRY(hipGetLastError());
    return LOCREC_OK;
}

// A wave's read-back for the unranked entries: one pack launch and one synchronisation for all its graphs, then the rows
// of every member's columns.  own: the plain-copy path's images.
template <class Tiles>
int32_t sg_pool_read_back(locrec_sg_pool *pool, const SgPoolWave &w, std::vector<SgPoolMember> &mem, Tiles &&tp, double eps2,
                          int64_t max_iterations, SgPoolStats &stats, std::vector<unsigned char> &own)
{
    hipStream_t s = pool->stream;
    const bool packed = !pool->no_pack && pool->h_pack_dev != nullptr;
    const unsigned nw = (unsigned)w.members.size();
    const unsigned char *host = nullptr;
    if (packed && pool->h_pack_bytes >= w.pack_bytes) {
        hipLaunchKernelGGL(sg_pack_pool, dim3(w.pack_blocks, nw), dim3(256), 0, s, w.tiles_dev, pool->h_pack_dev);
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        host = pool->h_pack;
    } else {
        own.resize(w.pack_bytes);
        for (unsigned j = 0; j < nw; ++j)
            LOCREC_TRY(sg_batch_copy_enqueue(pool->graphs[(size_t)w.members[j]], s, own.data() + w.tiles[j].pack_off,
                                             mem[(size_t)w.members[j]].both));
        LOCREC_HIP_TRY(hipStreamSynchronize(s));
        for (unsigned j = 0; j < nw; ++j)
            sg_batch_copy_assemble(pool->graphs[(size_t)w.members[j]]->nlive, own.data() + w.tiles[j].pack_off,
                                   mem[(size_t)w.members[j]].both);
        host = own.data();
    }
    LOCREC_HIP_TRY(hipGetLastError());
    stats.readback_bytes += (int64_t)w.pack_bytes;
    for (unsigned j = 0; j < nw; ++j) {
        locrec_sg_graph *g = pool->graphs[(size_t)w.members[j]];
        SgPoolMember &m = mem[(size_t)w.members[j]];
        LOCREC_TRY(sg_batch_host_rows(g, host + w.tiles[j].pack_off, m.uniq, w.k * (size_t)tp.tile_max(g), w.nb[j], eps2,
                                      max_iterations, m.res));
    }
    return LOCREC_OK;
}

}  // namespace

extern "C" int32_t locrec_sg_pool_recommend_batch(locrec_sg_pool *pool, int64_t n_requests, const int32_t *graph_index,
                                                  const int64_t *vertex_ids, double alpha, double epsilon, int64_t max_iterations,
                                                  int64_t *out_offsets, int64_t *out_ids, double *out_probs,
                                                  int64_t *inout_capacity, int64_t *out_iterations, int32_t *out_converged,
                                                  int64_t *out_bad_request) try
{
    if (!pool) return fail(LOCREC_E_INVALID_ARG, "pool is NULL");
    if (n_requests < 0 || (n_requests > 0 && (!graph_index || !vertex_ids)) || !out_offsets || !inout_capacity)
        return fail(LOCREC_E_INVALID_ARG, "bad arguments");
    LOCREC_TRY(sg_batch_requires(epsilon, max_iterations));
    std::vector<SgPoolMember> mem;
    std::vector<int32_t> act, uniq_of;
    LOCREC_TRY(sg_pool_requests(pool, n_requests, graph_index, vertex_ids, mem, act, uniq_of, out_bad_request));
    SgPoolStats &stats = sg_pool_stats();
    stats = SgPoolStats{};
    if (n_requests == 0) {
        out_offsets[0] = 0;
        *inout_capacity = 0;
        return LOCREC_OK;
    }
    if (max_iterations > INT32_MAX) max_iterations = INT32_MAX;
    LOCREC_TRY(sg_pool_begin_call(pool, act, mem));
    for (const int32_t gi : act) mem[(size_t)gi].res.resize(mem[(size_t)gi].uniq.size());
    const double eps2 = epsilon * epsilon;  // :40
    std::vector<unsigned char> own;  // the plain-copy path's images
    auto read_back = [&](const SgPoolWave &w) -> int32_t {
        return sg_pool_read_back(pool, w, mem, SgPoolPersonTiles{}, eps2, max_iterations, stats, own);
    };
    const int32_t status = sg_pool_waves(pool, act, mem, alpha, epsilon, max_iterations, stats, read_back);
    LOCREC_TRY(sg_pool_end_call(pool, act, mem, status));
    return sg_batch_output(
        n_requests, [&](int64_t i) { return SgBatchRowRef{&mem[(size_t)graph_index[i]].res, (size_t)uniq_of[(size_t)i]}; },
        out_offsets, out_ids, out_probs, inout_capacity, out_iterations, out_converged);
} LOCREC_CATCH_ALL
