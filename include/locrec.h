/*
 * locrec.h -- C ABI of liblocrec.so, the MI355X (gfx950) implementation of the
 * two hot paths of tashoyan/locations-recommender.
 *
 * The reference has NO native boundary (it is 100 % Scala on Spark); the
 * drop-in boundary is the public surface of two Scala classes, and this header
 * is the FFI a JNI shim under those classes binds (INTEGRATION.md shows the
 * shim).  Reference paths below are relative to
 *   recommender/src/main/scala/com/github/tashoyan/recommender/
 *
 *   knn/KnnRecommender.scala:9-25        class KnnRecommender(placeRatingVectors,
 *                                        categoryRatingVectors, placeRatings,
 *                                        placeWeight, categoryWeight, kNearest)
 *                                        .makeRecommendations(personId)
 *   stochastic/StochasticRecommender.scala:28-34,66-71
 *                                        class StochasticRecommender(stochasticEdges,
 *                                        epsilon, maxIterations)
 *                                        .makeRecommendations(vertexId)
 *
 * Conventions
 *   - every function returns an int32 status; LOCREC_OK == 0.  The message of
 *     the last failure on the calling thread is locrec_last_error().
 *   - LOCREC_E_INVALID_ARG and LOCREC_E_NOT_FOUND correspond to the
 *     IllegalArgumentException the reference throws (KnnRecommender.scala:17-20,83;
 *     StochasticRecommender.scala:33-34,70); the message text is the reference's.
 *   - handles are opaque; inputs are caller-owned host arrays that are COPIED to
 *     the device at create time (the library never retains a caller pointer);
 *     outputs go to caller-allocated buffers with an in/out element count: on
 *     entry the capacity, on return the number of rows the result HAS (which
 *     may exceed the capacity; only min(capacity, count) rows are written).
 *   - one handle = one device + one HIP stream; calls on one handle must be
 *     serialised by the caller, distinct handles are independent.
 *   - plain C types only: pointers, sizes, doubles.  No C++/torch types.
 */
#ifndef LOCREC_H
#define LOCREC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOCREC_OK 0
#define LOCREC_E_INVALID_ARG 1 /* IllegalArgumentException: require() failed            */
#define LOCREC_E_NOT_FOUND 2   /* IllegalArgumentException: "No such person / vertex"    */
#define LOCREC_E_DEVICE 3      /* HIP runtime failure, no GPU, kernel image missing      */
#define LOCREC_E_OOM 4         /* host or device allocation failed                        */
#define LOCREC_E_ARITHMETIC 5  /* ArithmeticException: "Index out of Int range: $l"
                                  (knn/RatingVectorsBuilder.scala:36-41)                  */

/* Where the arrays of the locrec_calc_* / locrec_build_* functions live. */
#define LOCREC_MEM_HOST 0      /* caller-owned host arrays, copied in and out            */
#define LOCREC_MEM_DEVICE 1    /* arrays of the CURRENT HIP device, inputs and outputs   */

/* Thread-local message of the last non-OK status returned on this thread. */
const char *locrec_last_error(void);
/* Library version string, e.g. "locrec 0.1 (gfx950)". */
const char *locrec_version(void);

/* Number of visible HIP devices / select the device new handles are created on. */
int32_t locrec_device_count(int32_t *out_count);
int32_t locrec_set_device(int32_t ordinal);
/* Device allocations (hipMalloc) this process has made through the library so far.  Diagnostic: the difference
 * across a stretch of steady-state calls should be 0 - work buffers live with their handle and only ever grow. */
int32_t locrec_device_allocations(int64_t *out_count);

/* Bytes of device memory the library holds right now (every handle's index / graph and work buffers). */
int32_t locrec_device_bytes_in_use(int64_t *out_bytes);

/* ===================================================================== */
/* Handle cache: the "handle persists across requests" half of the drop-in.
 *
 * The reference's mains construct a NEW recommender from freshly read DataFrames for every request
 * (knn/KnnRecommenderMain.scala:53-67, stochastic/StochasticRecommenderMain.scala:53-62) and never close
 * anything.  Behind those unchanged mains the device index must outlive the object that built it: the host
 * class derives a KEY from what its DataFrames are (input files + sizes + modification times; the weights,
 * K, epsilon and maxIterations are per-request arguments of the calls below and NOT part of the key), and
 *     locrec_cache_acquire(kind, key, &h)         h != NULL: a hit, reference taken - skip collect / create
 *     locrec_*_create(...)  +  locrec_cache_publish(kind, key, created, bytes, &h)
 *                                                 on a miss: the cache takes OWNERSHIP of `created` (if the key
 *                                                 appeared meanwhile the newcomer is destroyed and the cached
 *                                                 handle returned); reference taken
 *     locrec_cache_release(kind, h)               when the host object is closed or collected (close(),
 *                                                 java.lang.ref.Cleaner, __del__): drops the reference; the
 *                                                 handle STAYS cached.  A handle that was never published is
 *                                                 destroyed, so hosts release every handle the same way.
 * Unreferenced entries are destroyed least-recently-used first while the library's live device bytes
 * (locrec_device_bytes_in_use) exceed the byte limit or the entry count its limit (defaults 64 GiB / 64
 * entries; LOCREC_CACHE_BYTES / LOCREC_CACHE_ENTRIES or locrec_cache_set_limits, -1 = keep).  A handle is
 * still one device + one stream: users of one cached handle serialise their calls (the host classes lock).
 */
#define LOCREC_CACHE_KNN 0
#define LOCREC_CACHE_SG 1
int32_t locrec_cache_acquire(int32_t kind, const char *key, void **out_handle);
int32_t locrec_cache_publish(int32_t kind, const char *key, void *handle, int64_t device_bytes, void **out_handle);
int32_t locrec_cache_release(int32_t kind, void *handle);
int32_t locrec_cache_set_limits(int64_t max_device_bytes, int64_t max_entries);
int32_t locrec_cache_clear(void); /* drop every entry; referenced ones are destroyed by their last release */
int32_t locrec_cache_stats(int64_t *out_entries, int64_t *out_entry_bytes, int64_t *out_hits,
                           int64_t *out_misses, int64_t *out_evictions);

/* ===================================================================== */
/* KNN: knn/KnnRecommender.scala, knn/Distance.scala                     */

typedef struct locrec_knn_index locrec_knn_index;

/*
 * Replaces the three DataFrames of the KnnRecommender constructor
 * (KnnRecommender.scala:9-16), collected to CSR:
 *   person_ids[n]                      person_id column (distinct)
 *   p_rowptr[n+1], p_idx[], p_val[]    placeRatingVectors: per person the
 *                                      SparseVector(size = p_dim, indices
 *                                      ascending, values)   (RatingVectorsBuilder.scala:74-77)
 *   c_rowptr[n+1], c_idx[], c_val[]    categoryRatingVectors, size = c_dim
 *   r_rowptr[n+1], r_place[], r_rating[]  placeRatings (person_id, place_id,
 *                                      rating: Long) grouped by person; pass
 *                                      r_rowptr == NULL to use the place vectors
 *                                      themselves (what RatingVectorsBuilderMain
 *                                      .scala:41-73 writes: the same data in COO).
 * A person with an empty row in a family is absent from that family's frame.
 * Rows whose stored values have zero norm, non-finite values, unsorted or
 * out-of-range indices are rejected with LOCREC_E_INVALID_ARG.
 * Norms (Distance.scala:11-16) are computed ONCE here, on the device.
 */
int32_t locrec_knn_create(
    int64_t n, const int64_t *person_ids,
    const int64_t *p_rowptr, const int32_t *p_idx, const double *p_val, int32_t p_dim,
    const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t c_dim,
    const int64_t *r_rowptr, const int64_t *r_place, const int64_t *r_rating,
    locrec_knn_index **out_index);

/*
 * The same with every array already in DEVICE memory of the current device (row pointers included):
 * nothing passes through the host, the whole index is built by kernels and device sorts
 * (csrc/knn_build.hip).  This is what a device-side rating-vector builder or an
 * RCCL all-gather of per-rank shards (8 e) hands over.  The arrays are only read; the caller keeps them.
 */
int32_t locrec_knn_create_from_device(
    int64_t n, const int64_t *person_ids,
    const int64_t *p_rowptr, const int32_t *p_idx, const double *p_val, int32_t p_dim,
    const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t c_dim,
    const int64_t *r_rowptr, const int64_t *r_place, const int64_t *r_rating,
    locrec_knn_index **out_index);

int32_t locrec_knn_destroy(locrec_knn_index *index);

/* Number of persons; bytes the candidate rows occupy in HBM in the layout the
 * scan kernel streams (the "algorithmic bytes" of one query-vs-all pass).    */
int32_t locrec_knn_info(const locrec_knn_index *index, int64_t *out_n,
                        int64_t *out_scan_bytes, int32_t *out_packed);

/* Bytes of the image the BATCHED scan streams per query tile: the head / tail form (SELL rows of the head
 * elements + the inverted tail, knn_ht.h) where the index has it, else the same as locrec_knn_info's. */
int32_t locrec_knn_batch_scan_bytes(const locrec_knn_index *index, int64_t *out_scan_bytes);

/* Measurement only: sizes of the head / tail image (knn_ht.h) - 32-bit element words of the SELL head rows of both
 * families as STORED, incl. the padding to whole groups of four, postings of the inverted tail, and the number of rows
 * kept out of the image by the per-row format fallback.  Zeros without the image. */
int32_t locrec_knn_ht_image_info(const locrec_knn_index *index, int64_t *out_head_words, int64_t *out_tail_postings,
                                 int64_t *out_wide_rows);

/* Measurement only: the words of that image knn_scan_ht MULTIPLIES per query tile - per slice 64 lanes x the exact
 * element count of its widest row, both families (all of them rounded up to four under LOCREC_KNN_HT_ROUND4).  Every
 * such word costs one tile 8 v_pk_mad_u16 and one address v_and: the multiply-add count of a launch is tiles x words / 8
 * wave instructions, which the roofline derivation in profiles/ uses.  real elements <= this <= head_words. */
int32_t locrec_knn_ht_multiplied_words(const locrec_knn_index *index, int64_t *out_words);

/* Measurement and tests only: the per-slice element counts behind that figure, in slice order - out_place[s] and
 * out_category[s] for the first min(capacity, *out_slices) slices; *out_slices = the number of slices (0 without the
 * image).  Call with capacity 0 to size the arrays. */
int32_t locrec_knn_ht_slice_counts(const locrec_knn_index *index, int64_t capacity, int32_t *out_place, int32_t *out_category,
                                   int64_t *out_slices);

/* Measurement and tests only: the LDS model of the head / tail image's element order (csrc/knn_ht_order.h), computed
 * over the stored image by a small kernel on demand.  Counted are the positions in front of every slice's element
 * counts, both families, for each of the four groups of 16 lanes that one LDS cycle serves: *out_group_reads = such
 * (slice, position, group) reads, *out_cycles = the cycles they take when different panel rows on one slot (index mod
 * 16) cost a cycle each and equal rows share one.  cycles - group_reads = modelled bank-conflict cycles per plane read.
 * Zeros without the image.  Synchronises the handle's stream. */
int32_t locrec_knn_ht_lds_model(locrec_knn_index *index, int64_t *out_group_reads, int64_t *out_cycles);

/* Measurement and tests only: the queries the LDS aggregation (csrc/knn_aggregate.h; K <= LOCREC_KNN_BATCH_MAX_K) has
 * served on this handle since the previous call of this function: out[0] summed by the bucket form
 * (knn_aggregate_buckets), out[1] summed by the sort form (knn_aggregate: the redo pass of a flagged query, an index with
 * too many places for the bucket form, LOCREC_KNN_AGG_SORT), out[2] left flagged, their rows being assembled by the
 * host or the place-major pass.  Device counters: reads and resets them, synchronises the handle's stream. */
int32_t locrec_knn_aggregate_stats(locrec_knn_index *index, int64_t out[3]);

/* Measurement and tests only: what the hit pre-pass of the last batched head / tail scan on this handle left on the
 * device (csrc/knn_ht_prepass.h).  nq names that batch, as for locrec_knn_fetch_topk; call directly after the batch.
 * *out_query_tile, *out_tiles, [*out_slice0, *out_nslices) = the handle's candidate slices (the off rows have one entry
 * per slice and a closing one), *out_total = hit words of all tiles; out_tile_base[t] = first hit word of tile t
 * (*out_tiles + 1 entries, the last one the total), out_off[t * (*out_nslices - *out_slice0 + 1) + s - *out_slice0] =
 * start of slice s inside tile t's hits (the closing entry is the tile's total), out_hits = the hit words
 * (lane << 21 | query of the tile << 16 | product), grouped by slice, in any order inside a slice.  At most
 * tile_capacity / off_capacity / hit_capacity entries of the three arrays are written: call with capacities 0 to size
 * them.  Synchronises the handle's stream.  Refused ("no matching hit pre-pass to read") when the last scan recorded
 * on the handle was not a batched head / tail scan of nq queries (scan plan kernel 2 or 3): none yet, another size,
 * or a scan without a pre-pass. */
int32_t locrec_knn_ht_last_hits(locrec_knn_index *index, int64_t nq, int64_t tile_capacity, int64_t off_capacity,
                                int64_t hit_capacity, int32_t *out_query_tile, int64_t *out_tiles, int32_t *out_slice0,
                                int32_t *out_nslices, int64_t *out_tile_base, uint32_t *out_off, uint32_t *out_hits,
                                int64_t *out_total);

/*
 * Plan of the last batched scan enqueued on this handle (measurement only; bench.py prints it):
 * kernel 1 = knn_scan (row scan over a query panel in LDS), 2 = knn_scan_ht (head / tail form: dense
 * head panel in LDS + inverted tail, knn_ht.h), 3 = knn_scan in its head / tail mode (A/B partner of 2),
 * 0 = none yet; mode 0 / 1 / 2 = GENERIC (fp64) / PACK32 / PACK16, 3 = head / tail (u16 dots); the
 * query tile (queries sharing one read of a candidate row) and the waves per block.
 */
int32_t locrec_knn_scan_plan(const locrec_knn_index *index, int32_t *out_kernel, int32_t *out_mode,
                             int32_t *out_query_tile, int32_t *out_waves_per_block);

/*
 * Distance.vectorLength (knn/Distance.scala:11-16) of every person's two vectors, as
 * computed on the device at create time; arrays of n in the order of person_ids[].
 * An absent (empty) vector has length 0.0 (DistanceTest.scala:10-14).
 */
int32_t locrec_knn_vector_lengths(locrec_knn_index *index, double *out_place_lengths,
                                  double *out_category_lengths);

/*
 * Distance.cosineSimilarity (knn/Distance.scala:7-9) of two persons' place vectors and of their category vectors,
 * computed on the device from the index's own fp64 rows and lengths: (v1 dot v2) / (len(v1) * len(v2)), any sign
 * (findSimilarPersons only ever shows the positive ones, KnnRecommender.scala:91-93), NaN where a vector is empty.
 * DistanceTest.scala:16-60 through the ABI.  LOCREC_E_NOT_FOUND for an unknown id.
 */
int32_t locrec_knn_cosine_similarity(locrec_knn_index *index, int64_t person_a, int64_t person_b,
                                     double *out_place_cosine, double *out_category_cosine);

/*
 * findSimilarPersons (KnnRecommender.scala:27-49): the K nearest persons of
 * person_id, ordered by (similarity desc, person_id asc).
 * place_weight/category_weight/k_nearest are validated exactly as the
 * constructor does (:17-20).  There is no limit on the length of the person's
 * vectors (a row up to 2^21 - 1 non-zeros per family is accepted at create
 * time) nor on k_nearest: a vector too long for an on-chip panel takes a
 * slower global-memory scan with identical results; this holds for every
 * query / recommend function below, batched ones included.
 */
int32_t locrec_knn_query(
    locrec_knn_index *index, int64_t person_id,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_person_ids, double *out_similarities, int64_t *inout_count);

/*
 * makeRecommendations (KnnRecommender.scala:22-25,51-70):
 * rows (place_id, estimated_rating), ordered by place_id ascending (the
 * reference leaves the order undefined).
 */
int32_t locrec_knn_recommend(
    locrec_knn_index *index, int64_t person_id,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_place_ids, double *out_estimated_ratings, int64_t *inout_count);

/*
 * Batched makeRecommendations (KnnRecommender.scala:22-25 for many persons; the additive
 * "makeRecommendationsBatch" of SURVEY.md 8b): findSimilarPersons AND makeRecommendations0 on the
 * device for every listed person.  Rows of person i are [out_offsets[i], out_offsets[i+1]) of
 * out_place_ids / out_estimated_ratings, ordered by place id; out_offsets has nq + 1 entries.
 * *inout_capacity: in = room in the two output arrays, out = rows needed; when the room is too
 * small only out_offsets is filled and the call is repeated with larger arrays.
 */
int32_t locrec_knn_recommend_batch(
    locrec_knn_index *index, int64_t nq, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_offsets, int64_t *out_place_ids, double *out_estimated_ratings, int64_t *inout_capacity);
/* device-resident form over the internal rows [first, first + nq) (see locrec_knn_topk_range_async) */
int32_t locrec_knn_recommend_range_async(
    locrec_knn_index *index, int64_t first, int64_t nq,
    double place_weight, double category_weight, int64_t k_nearest);
int32_t locrec_knn_fetch_recommend(
    locrec_knn_index *index, int64_t nq,
    int64_t *out_offsets, int64_t *out_place_ids, double *out_estimated_ratings, int64_t *inout_capacity);

/*
 * The batched request to its end: makeRecommendations for nq persons, then printRecommendations per
 * person (the places of target_region_ids[i] JOIN the person's rows ON id, ORDER BY score DESC, LIMIT
 * max_recommendations; see locrec_rank_recommendations_batch for the order) - ranked on the device
 * where the rows are, so only max_recommendations rows a person reach the host.  Row i of
 * out_place_ids / out_estimated_ratings (host, row-major, stride max(0, max_recommendations)) belongs
 * to person_ids[i], padded with id -1 and rating 0.0; out_counts[i] = rows written.  A repeated
 * person gets identical rows.  Errors as locrec_knn_recommend_batch.  place_ids / place_region_ids /
 * target_region_ids are host arrays.  locrec_knn_fetch_ranked is the same last stage for the range
 * left by locrec_knn_recommend_range_async (target_region_ids[i] for internal row first + i; a row
 * that is no valid query gets count 0).  locrec_rank_recommendations_batch_stats describes the call.
 */
int32_t locrec_knn_recommend_ranked_batch(
    locrec_knn_index *index, int64_t nq, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    int64_t *out_place_ids, double *out_estimated_ratings, int64_t *out_counts);
int32_t locrec_knn_fetch_ranked(
    locrec_knn_index *index, int64_t nq,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    int64_t *out_place_ids, double *out_estimated_ratings, int64_t *out_counts);
/*
 * The unvisited forms of the two calls above - same arguments, outputs, padding, errors and refusals - which
 * recommend only new places: person i's ranking leaves out every place the index holds a placeRatings row of
 * that person for (where create was given no ratings: the entries of the person's place vector).  The lists
 * are read where they lie on the device (locrec_rank_recommendations_batch_excluding's ranker with begins and
 * lengths into the index's rating rows).  Afterwards the plain calls return what they did before.
 */
int32_t locrec_knn_recommend_ranked_batch_unvisited(
    locrec_knn_index *index, int64_t nq, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    int64_t *out_place_ids, double *out_estimated_ratings, int64_t *out_counts);
int32_t locrec_knn_fetch_ranked_unvisited(
    locrec_knn_index *index, int64_t nq,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    int64_t *out_place_ids, double *out_estimated_ratings, int64_t *out_counts);
/*
 * Within reach: locrec_knn_recommend_ranked_batch with a circle per position
 * (locrec_rank_recommendations_batch_near's semantics, requires and refusals; host arrays, checked before the
 * index is looked at).  place_latitudes / place_longitudes: one per row of the place table; center_*,
 * radius_meters: one per position.  unvisited != 0: the _unvisited form's lists as well.  out_meters (nq x
 * max_recommendations, may be NULL): the distance of each output row, padding 0.0.  Both resident row forms and
 * the second ranker call for host-assembled overflow queries go through the near ranker; a repeated person is
 * ranked per position with its own circle.  Afterwards the plain calls return what they did before.
 */
int32_t locrec_knn_recommend_ranked_batch_near(
    locrec_knn_index *index, int64_t nq, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const double *place_latitudes, const double *place_longitudes,
    const int64_t *target_region_ids,
    const double *center_latitudes, const double *center_longitudes, const double *radius_meters,
    int64_t max_recommendations, int32_t unvisited,
    int64_t *out_place_ids, double *out_estimated_ratings, double *out_meters, int64_t *out_counts);
/*
 * By category: locrec_knn_recommend_ranked_batch_near with the circles optional (all five coordinate arrays NULL:
 * none, out_meters unused) and an allow-list of categories and a cap per category for every position
 * (locrec_rank_recommendations_batch_by_category's semantics, requires and refusals; host arrays, checked before
 * the index is looked at).  place_category_ids: one per row of the place table; allowed_offsets (nq + 1 entries,
 * NULL: no lists), allowed_category_ids (n_allowed entries) and max_per_category (one per position, NULL: no caps)
 * as there.  unvisited != 0: the _unvisited form's lists as well.  Both resident row forms and the second ranker
 * call for host-assembled overflow queries go through the by-category ranker; a repeated person is ranked per
 * position with its own list and cap.  With no lists and no cap below max_recommendations the result is the plain,
 * unvisited or near call's.
 */
int32_t locrec_knn_recommend_ranked_batch_by_category(
    locrec_knn_index *index, int64_t nq, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const double *place_latitudes, const double *place_longitudes, const int64_t *place_category_ids,
    const int64_t *target_region_ids,
    const double *center_latitudes, const double *center_longitudes, const double *radius_meters,
    int64_t max_recommendations, int32_t unvisited,
    const int64_t *allowed_offsets, int64_t n_allowed, const int64_t *allowed_category_ids,
    const int64_t *max_per_category,
    int64_t *out_place_ids, double *out_estimated_ratings, double *out_meters, int64_t *out_counts);

/*
 * A pool of resident indexes that serves ONE mixed batch of (index, person[, target region]) requests - the queue of
 * KnnRecommenderMain's loop, whose lines fan out over the indexes of sorted{home, target}
 * (KnnRecommenderMain.scala:53-67).  A member in the "every positive neighbour" regime (k_nearest >
 * LOCREC_KNN_BATCH_MAX_K and k_nearest >= its person count - 1: the shipped --k-nearest 2000000) shares its launches
 * with the others: its distinct requests are cut into tiles of 16, wave w holds the w-th tile of every such member, and
 * every kernel of the large-K batch is launched ONCE per wave for all of them, on the pool's own stream, with one
 * read-back of tile counts and one wait per wave.  Any other member's requests go to its own
 * locrec_knn_recommend_batch / locrec_knn_recommend_ranked_batch call.  All calls are synchronous.
 * create: 1 .. 65535 distinct indexes on one device; the pool does not own them: destroy it before them.  Refused
 * (LOCREC_E_INVALID_ARG, the message names the member): a NULL list, a NULL member, a member listed twice, members on
 * different devices.
 * recommend_batch: request i asks index index_of_request[i] (a position of create's list) for person_ids[i].  Rows
 * (ordered by place id), offsets, the capacity protocol and the NULL rules are those of locrec_knn_recommend_batch;
 * request i's rows equal bit for bit what that call returns for the person on the member alone.  A repeated (index,
 * person) pair is computed once; the same person id in two members is two requests.  Before any device work: every
 * index position (LOCREC_E_INVALID_ARG, "... names index <k> ..."), then the requires on the weights and k_nearest with
 * their messages, then every person (LOCREC_E_NOT_FOUND, "No such person: <id>"; a person without a place or category
 * vector is not found).  On a failure nothing is written except *out_bad_request (may be NULL): the position of the
 * first offending request; -1 on success.  n_requests == 0: out_offsets[0] = 0, capacity 0.
 * recommend_ranked_batch: request i gets the places of target_region_ids[i], top max_recommendations by estimated
 * rating.  Outputs, padding (-1 / 0.0) and the checks on n_places, the arrays and max_recommendations are those of
 * locrec_knn_recommend_ranked_batch; request i's values equal that call's on the member alone bit for bit.  ONE places
 * table serves all members, uploaded once; the sharing members' rows are ranked by one call of the segmented ranker
 * where they lie, and max_recommendations rows a request reach the host.
 * After any pool call every member serves single requests and its own batches as a fresh handle does, and nothing is
 * resident for locrec_knn_fetch_*.
 * stats: this thread's last pool call (any pointer may be NULL): tile waves, member tiles (tiles of 16 over all members
 * and waves), launches of the fill kernel (set and wipe: 2 a wave), of the scan kernel (1), of the segment aggregation
 * (1) and of the sum / count / emit kernels (3), members served by their own call, rows emitted on the device, bytes
 * read back, waits for the pool's stream.
 */
typedef struct locrec_knn_pool locrec_knn_pool;
int32_t locrec_knn_pool_create(locrec_knn_index *const *indexes, int32_t n_indexes, locrec_knn_pool **out_pool);
void locrec_knn_pool_destroy(locrec_knn_pool *pool);
int32_t locrec_knn_pool_recommend_batch(
    locrec_knn_pool *pool, int64_t n_requests, const int32_t *index_of_request, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_offsets, int64_t *out_place_ids, double *out_estimated_ratings, int64_t *inout_capacity,
    int64_t *out_bad_request);
int32_t locrec_knn_pool_recommend_ranked_batch(
    locrec_knn_pool *pool, int64_t n_requests, const int32_t *index_of_request, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    int64_t *out_place_ids, double *out_estimated_ratings, int64_t *out_counts, int64_t *out_bad_request);
int32_t locrec_knn_pool_stats(int64_t *out_waves, int64_t *out_member_tiles, int64_t *out_fill_launches,
                              int64_t *out_scan_launches, int64_t *out_aggregate_launches, int64_t *out_finish_launches,
                              int64_t *out_delegated_members, int64_t *out_emitted_rows, int64_t *out_readback_bytes,
                              int64_t *out_host_syncs);

/*
 * KNN for visitors: rating vectors that are no rows of the index - a person who arrived after the cut of the visit
 * table the index was built from, or whose visits have changed since.  nv visitors as two CSR families (nv + 1 row
 * pointers each, indices in the index's ORIGINAL place / category numbering, strictly ascending) in `mem`
 * (LOCREC_MEM_HOST, or LOCREC_MEM_DEVICE: on the index's device); every other array is a host array.
 * For a visitor v and an index built from the persons P, every result equals what locrec_knn_query_batch,
 * locrec_knn_recommend_batch and locrec_knn_recommend_ranked_batch return for v on an index built from P + {v}, with v
 * under an id no person has: neighbour ids, counts and similarity bits, place ids and row counts are identical,
 * estimated ratings within 1e-6 relative.  So v is a candidate of nobody, nobody is left out as "self", v has no
 * rating rows, ties fall by (similarity desc, person_id asc) among P, a list holds at most min(k_nearest, n) entries
 * and "every positive neighbour" begins at k_nearest >= n.  An entry at an index >= the index's place / category
 * dimension is legal (the reference's builder would have given every vector the larger size): it enters the vector's
 * length and no dot product.
 * Output layouts, padding (-1 / 0.0), the capacity protocol and the chunking of huge nv x k_nearest results are those
 * of the three person calls.  exclude_offsets[nv + 1] / exclude_place_ids: per visitor a list of place ids its ranking
 * leaves out (locrec_rank_recommendations_batch_excluding's lists; a caller who wants only new places passes the
 * visitor's rated places), or NULL, NULL.
 * Refusals, all before any result is written, *out_bad_visitor (may be NULL) = the first offending visitor, or -1 when
 * no single visitor is at fault: NULL arguments and negative counts; the requires on the weights and k_nearest with
 * their messages; then per visitor what create refuses in a row - row pointers that turn back, negative, unsorted or
 * repeated indices, a non-finite value, a zero norm, 2^21 or more entries (LOCREC_E_INVALID_ARG) - an empty place or
 * category vector (LOCREC_E_NOT_FOUND, "No such person: ..."), and, on an index that renumbers its place dimensions
 * by popularity (integer data by construction), a place value that is no integer below 65536 (LOCREC_E_INVALID_ARG:
 * its dot products would be summed in another order than BLAS.dot's; category dimensions are never renumbered, so
 * category values may be any finite numbers).  An index without the renumbering takes any finite values and stays
 * bit-exact.  nv == 0 succeeds with empty outputs.
 * All calls are synchronous.  Afterwards nothing is resident for locrec_knn_fetch_*, and every other call on the
 * handle returns what it returned before.
 * stats: this thread's last visitors call: out[0] tiles of 16 visitors, [1] tiles served without a top-K
 * (k_nearest >= n), [2] tiles through the tiled selection, [3] entries beyond the index's dimensions, [4] 1 if the
 * index renumbers its place dimensions, [5] launches of the stage kernel, [6] launches of the scan kernel, [7] waits
 * for the stream.
 */
int32_t locrec_knn_visitors_query_batch(
    locrec_knn_index *index, int64_t nv,
    const int64_t *p_rowptr, const int32_t *p_idx, const double *p_val,
    const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t mem,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_person_ids, double *out_similarities, int64_t *out_counts, int64_t *out_bad_visitor);
int32_t locrec_knn_visitors_recommend_batch(
    locrec_knn_index *index, int64_t nv,
    const int64_t *p_rowptr, const int32_t *p_idx, const double *p_val,
    const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t mem,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_offsets, int64_t *out_place_ids, double *out_estimated_ratings, int64_t *inout_capacity,
    int64_t *out_bad_visitor);
int32_t locrec_knn_visitors_recommend_ranked_batch(
    locrec_knn_index *index, int64_t nv,
    const int64_t *p_rowptr, const int32_t *p_idx, const double *p_val,
    const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t mem,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    const int64_t *exclude_offsets, const int64_t *exclude_place_ids,
    int64_t *out_place_ids, double *out_estimated_ratings, int64_t *out_counts, int64_t *out_bad_visitor);
int32_t locrec_knn_visitors_stats(int64_t out[8]);

/*
 * One mixed batch of visitors over a pool of indexes: visitors fan out over region sets exactly as persons do.  Visitor
 * i asks member index_of_visitor[i] (a host array; a position of locrec_knn_pool_create's list); the six vector arrays
 * are ONE CSR over all nv visitors in call order, in `mem` (LOCREC_MEM_HOST, or LOCREC_MEM_DEVICE: on the pool's device),
 * in one numbering for all members: an entry beyond a member's dimensions is legal for that member, as above.  Output
 * layouts, padding, the capacity protocol, the NULL rules and the exclusion lists are those of
 * locrec_knn_visitors_recommend_batch / _recommend_ranked_batch, and visitor i's rows and ranked row equal, bit for bit,
 * what those calls return for that vector on member index_of_visitor[i] alone.  Visitors carry no id: a vector given
 * twice is computed twice, and a visitor's result depends on its own vector and its member only.
 * A member of n > 0 persons shares the pool's launches when k_nearest > LOCREC_KNN_BATCH_MAX_K and k_nearest >= n (its
 * own visitors call would serve every tile without a top-K): ONE stage launch checks and stages every visitor of every
 * member, then every kernel of the large-K batch is launched once per wave of tiles for all members, with one read-back
 * of tile counts and one wait per wave.  A member without persons has no rows.  Any other asked member's visitors are
 * gathered in call order into a CSR of their own (device arrays: device to device) and served by its own
 * locrec_knn_visitors_* call.
 * Checks, all before any result is written and in this order, *out_bad_visitor (may be NULL) = the first offending
 * position, or -1: a NULL pool (nothing at all is written); NULL arguments and negative counts, `mem`, the ranked
 * arguments and the exclusion offsets with the per-index calls' texts; every index position (LOCREC_E_INVALID_ARG,
 * "visitor <i> names index <k> of a pool of <m>"); the requires on the weights and k_nearest; a member without a record
 * for visitors; then the per-visitor refusals of the per-index calls with their messages - the integer rule only for
 * visitors of members that renumber their place dimensions - where the first offender is the smallest position in call
 * order across members, the place family first; then a call whose rows may exceed 48 GB in total ("... split it").
 * nv == 0 succeeds with empty outputs.  All calls are synchronous.  Afterwards every asked member has nothing resident
 * for locrec_knn_fetch_* and serves persons, visitors and the pool's person calls as before.
 * stats: this thread's last pool-visitors call: out[0] waves, [1] member tiles, [2] launches of the stage kernel (1),
 * [3] of the fill kernel (2 a wave), [4] of the scan kernel (1 a wave), [5] of the segment aggregation (1 a wave), [6] of
 * the sum / count / emit kernels (3 a wave), [7] members served by their own call, [8] entries beyond the members'
 * dimensions, [9] rows emitted on the device, [10] bytes read back, [11] waits for the pool's stream.
 */
int32_t locrec_knn_pool_visitors_recommend_batch(
    locrec_knn_pool *pool, int64_t nv, const int32_t *index_of_visitor,
    const int64_t *p_rowptr, const int32_t *p_idx, const double *p_val,
    const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t mem,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_offsets, int64_t *out_place_ids, double *out_estimated_ratings, int64_t *inout_capacity,
    int64_t *out_bad_visitor);
int32_t locrec_knn_pool_visitors_recommend_ranked_batch(
    locrec_knn_pool *pool, int64_t nv, const int32_t *index_of_visitor,
    const int64_t *p_rowptr, const int32_t *p_idx, const double *p_val,
    const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t mem,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    const int64_t *exclude_offsets, const int64_t *exclude_place_ids,
    int64_t *out_place_ids, double *out_estimated_ratings, int64_t *out_counts, int64_t *out_bad_visitor);
int32_t locrec_knn_pool_visitors_stats(int64_t out[12]);

/*
 * One request with its candidate scan split over several GPUs (SURVEY.md 8e "KNN single request,
 * latency mode").  Every GPU holds the whole index (132 MB at cfg2, 1.3 GB at cfg4: nothing next to
 * 288 GB) and scans candidate shard shard_index of shard_count, a contiguous range of the
 * length-sorted rows holding ~1/shard_count of the stored elements:
 *     locrec_knn_query_shard          findSimilarPersons (:27-49) over that shard -> local top-K
 *     all-gather of the local lists   by the caller (K * 16 bytes per GPU), merge by
 *                                     (similarity desc, person_id asc) -> the K nearest
 *     locrec_knn_recommend_neighbours makeRecommendations0 (:51-70) for that list, on any one GPU
 * The union over all shards of the local lists contains the unsharded answer, so the merged
 * result is identical to locrec_knn_query's.
 * locrec_knn_recommend_neighbours rejects a neighbour id that is listed twice (LOCREC_E_INVALID_ARG).
 */
int32_t locrec_knn_query_shard(
    locrec_knn_index *index, int64_t person_id,
    double place_weight, double category_weight, int64_t k_nearest,
    int32_t shard_index, int32_t shard_count,
    int64_t *out_person_ids, double *out_similarities, int64_t *inout_count);
int32_t locrec_knn_recommend_neighbours(
    locrec_knn_index *index, int64_t n_neighbours,
    const int64_t *neighbour_person_ids, const double *similarities,
    int64_t *out_place_ids, double *out_estimated_ratings, int64_t *inout_count);

/*
 * Batched findSimilarPersons: the additive "all-pairs" surface.
 * out_person_ids / out_similarities are [nq * k_nearest] row-major, padded with
 * id -1 / similarity 0.0; out_counts[nq] is the number of valid entries (at most
 * min(k_nearest, N - 1)).
 * LOCREC_KNN_BATCH_MAX_K is the largest K the per-query LDS lists of a batch serve.  A larger K
 * takes the tiled top-K (tiles of 16 queries, the candidates at or above each query's deciding
 * similarity sorted on the device) with identical results; the synchronous forms work through the
 * queries in chunks whose device result arrays stay within 2 GiB.
 */
#define LOCREC_KNN_BATCH_MAX_K 1024
int32_t locrec_knn_query_batch(
    locrec_knn_index *index, int64_t nq, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_person_ids, double *out_similarities, int64_t *out_counts);

/* Every person as the query, in the order of person_ids[] given at create.  A person whose place
 * or category vector is empty is a candidate of the others' outer join (KnnRecommender.scala:39-40)
 * but not a valid query (:77-83 throws "No such person" for it): its out_counts entry is -1 and its
 * row is padded; the call does not fail. */
int32_t locrec_knn_all_pairs_topk(
    locrec_knn_index *index,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_person_ids, double *out_similarities, int64_t *out_counts);

/*
 * Device-resident form (used by bench.py; no host buffers inside the timed
 * region).  The index keeps the persons in an internal ROW order (ascending
 * vector length, so a tile of consecutive rows holds queries of similar size);
 * the queries of this call are the persons at rows [first_row, first_row + nq).
 * Kernels are enqueued on the handle's stream and the result stays in HBM until
 * locrec_knn_fetch_topk().  locrec_knn_row_person_ids() names the persons.
 * Rows that are not valid queries (an empty place or category vector) get count -1, as above;
 * the batched aggregation gives them zero recommendation rows.  Beyond LOCREC_KNN_BATCH_MAX_K the
 * whole range's nq x k_nearest result stays resident until the fetch: the caller bounds it by nq.
 */
int32_t locrec_knn_row_person_ids(locrec_knn_index *index, int64_t first_row, int64_t nq,
                                  int64_t *out_person_ids);
int32_t locrec_knn_topk_range_async(
    locrec_knn_index *index, int64_t first_row, int64_t nq,
    double place_weight, double category_weight, int64_t k_nearest);
int32_t locrec_knn_fetch_topk(
    locrec_knn_index *index, int64_t nq, int64_t k_nearest,
    int64_t *out_person_ids, double *out_similarities, int64_t *out_counts);

/* Use an externally created hipStream_t (passed as void*) for this handle. */
/*
 * Statistics of the batched scan's barrier-free insertion path: how many flush intervals (4 slices
 * of one block), since the index was created, overran a wave's survivor queue and were replayed
 * with synchronous insertion inside the kernel.  Results are never affected and nothing is redone
 * on the host; a few hundred per million intervals is normal (runs of tied candidates).
 */
int32_t locrec_knn_replayed_intervals(locrec_knn_index *index, int64_t *out_blocks);

int32_t locrec_knn_set_stream(locrec_knn_index *index, void *hip_stream);
int32_t locrec_knn_synchronize(locrec_knn_index *index);
/*
 * HIP-event profile of the dominant (scan) kernel: when enabled every scan
 * launch is bracketed by events on the handle's stream; read returns the
 * summed duration and launch count since the last reset and resets them.
 */
int32_t locrec_knn_profile_enable(locrec_knn_index *index, int32_t on);
int32_t locrec_knn_profile_read(locrec_knn_index *index, double *out_scan_ms, int64_t *out_launches);

/* ===================================================================== */
/* SG: stochastic/StochasticRecommender.scala                            */

typedef struct locrec_sg_graph locrec_sg_graph;

/*
 * Replaces the stochasticEdges DataFrame (source_id, target_id,
 * balanced_weight) of the constructor (StochasticRecommender.scala:28-31).
 * Builds vertexes = distinct(source U target) (:42-49) and the device layout.
 */
int32_t locrec_sg_create(
    int64_t n_edges, const int64_t *source_ids, const int64_t *target_ids,
    const double *balanced_weights, locrec_sg_graph **out_graph);

/*
 * The same handle from an edge list that already lives in DEVICE memory (the current HIP device), e.g. the
 * output of locrec_build_balanced_edges with mem = device: the SG counterpart of locrec_knn_create_from_device.
 * The three arrays are only read and the caller keeps them; no array of n_edges elements crosses to the host.
 *
 * The handle is an ordinary, unsharded locrec_sg_graph, and its layout equals the one locrec_sg_create builds
 * from the same edge list element for element: the same ascending vertex ids, live order, piece plan, slot of
 * every edge (edge-list order inside a row), weight interleave, partial-slot maps, dead-slot lists, column
 * width and weight dictionary.  A row's sum runs in slot order, so every request, batch and group answers bit
 * for bit what it answers on the host-built handle; info / device_bytes / weight_dictionary / live_count agree.
 *
 * Built by kernels on the handle's stream (csrc/sg_create_device.hip; DESIGN.md 4, "Device build"): vertex
 * ranking through a table over [min id, max id] or a sort of the 2 E ids (the rule of locrec_sg_create,
 * LOCREC_SG_NO_DENSE_IDS included), one stable radix sort of the edges by target vertex, scans for the live
 * order and the piece plan, a second stable sort for the out-edges of source-only vertices.  No position comes
 * from an atomic, so the layout does not depend on scheduling.  Only vertex-sized arrays (vertex ids, live
 * order, dead-slot row pointers) are read back; temporaries are freed before the call returns, and it returns
 * when the handle is complete.
 *
 * n_edges in [0, 2^31), else LOCREC_E_INVALID_ARG; n_edges == 0 behaves as locrec_sg_create(0, ...); NULL
 * arrays with n_edges > 0, arrays that are not device memory of the current device, and out_graph == NULL are
 * LOCREC_E_INVALID_ARG; "too many vertices" and "graph too large for int32 slot ids / partial slots" are
 * reported as by locrec_sg_create.  The create-time switches LOCREC_SG_NO_COL16, NO_DICT, NO_DENSE_IDS, GS,
 * PPW, DICT_*, NO_GRAPH and NO_PACK are honoured as there.  The two experiments (LOCREC_SG_FUSED,
 * LOCREC_SG_PERSIST) keep their host-only extra layouts: a handle created under either switch copies the three
 * columns to the host once and goes through the host build.
 */
int32_t locrec_sg_create_from_device(
    int64_t n_edges, const int64_t *source_ids, const int64_t *target_ids,
    const double *balanced_weights, locrec_sg_graph **out_graph);

/* HIP-event milliseconds of the phases of this thread's last locrec_sg_create_from_device (measurement): vertex
 * ranking, live order + piece plan + maps, the two sorts + the scatter, the weight dictionary.  Zeros after a
 * call that took the host build.  Every pointer may be NULL. */
int32_t locrec_sg_create_from_device_stats(double *out_ranking_ms, double *out_plan_ms, double *out_scatter_ms,
                                           double *out_dictionary_ms);

int32_t locrec_sg_destroy(locrec_sg_graph *graph);

/* vertexCount (:51); edges; bytes one sweep x -> x' streams (algorithmic). */
int32_t locrec_sg_info(const locrec_sg_graph *graph, int64_t *out_vertices,
                       int64_t *out_edges, int64_t *out_sweep_bytes);

/* Bytes one sweep x -> x' moves in the DEVICE layout (uint16 / int32 columns + fp64 weights of every
 * slot incl. padding, piece descriptors, partial sums written and re-read, x and x'): the figure
 * bench.py prices the SG kernels against (locrec_sg_info's is SURVEY 8d's reference-width model). */
int32_t locrec_sg_device_bytes(const locrec_sg_graph *graph, int64_t *out_sweep_bytes);

/* Distinct balanced_weight values (by bit pattern, +0.0 of the padding slots included) when the handle streams a
 * uint16 index per edge and looks the fp64 value up in a table (at most 8192 of them: the weights are count / total x
 * beta, few distinct values); 0 when it streams the fp64 weights themselves.  Same results either way, bit for bit. */
int32_t locrec_sg_weight_dictionary(const locrec_sg_graph *graph, int32_t *out_entries);

/*
 * makeRecommendations (StochasticRecommender.scala:66-141).
 * alpha is 0.15 in the reference (:38) and is a parameter here.
 * Rows (id, probability) with id != vertex_id and probability > 0 (:84-88),
 * ordered by id ascending (the reference leaves the order undefined).
 * out_iterations: the 0-based counter the reference prints (:94,100);
 * out_converged: 1 = "Converged in N iterations", 0 = maximum reached.
 */
int32_t locrec_sg_recommend(
    locrec_sg_graph *graph, int64_t vertex_id,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t *out_ids, double *out_probabilities, int64_t *inout_count,
    int64_t *out_iterations, int32_t *out_converged);

/*
 * makeRecommendations (StochasticRecommender.scala:66-141) for n_targets vertices of ONE graph.
 * Rows of target i are [out_offsets[i], out_offsets[i+1]) of out_ids / out_probabilities, with the same
 * rows, order and values locrec_sg_recommend returns for that vertex alone; out_offsets has n_targets + 1
 * entries, out_iterations / out_converged n_targets (either may be NULL).
 * *inout_capacity: in = room in the two row arrays, out = rows needed; when the room is too small only
 * out_offsets (and the counters) are filled and the call is repeated with larger arrays.
 * Every id is checked before any device work (LOCREC_E_NOT_FOUND, "No such vertex in the graph: <id>",
 * nothing written); a repeated id is computed once.  Up to 16 distinct targets share each sweep of the
 * graph; each stops at its own isConverged, and every result equals the single request's bit for bit.
 * Afterwards the handle serves single requests exactly as before.  Refused (LOCREC_E_INVALID_ARG) on
 * sharded handles and on handles created under the fused or persistent experiment
 * (LOCREC_SG_FUSED / LOCREC_SG_PERSIST); every other switch is served.
 */
int32_t locrec_sg_recommend_batch(
    locrec_sg_graph *graph, int64_t n_targets, const int64_t *vertex_ids,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t *out_offsets, int64_t *out_ids, double *out_probabilities, int64_t *inout_capacity,
    int64_t *out_iterations, int32_t *out_converged);

/*
 * The batched request to its end (StochasticRecommenderMain.scala:53-75): makeRecommendations for n_targets
 * vertices of ONE graph, then per request the places of ITS target region, top max_recommendations by
 * probability - emitted and ranked on the device; x is never read back.  All arrays are host arrays.
 * Row i of out_ids / out_probabilities (row-major, stride max(0, max_recommendations)) holds bit for bit what
 * locrec_rank_recommendations returns for the rows locrec_sg_recommend returns for vertex_ids[i], with
 * target_region_ids[i]; padded with id -1 / probability 0.0.  out_counts[i]: rows written.  out_row_counts[i]
 * (may be NULL): the rows makeRecommendations itself has for that vertex (id != vertex and p > 0, before the
 * region join), counted on the device.  out_iterations / out_converged as in locrec_sg_recommend_batch
 * (either may be NULL).  A repeated vertex is iterated once; each of its positions is ranked with its own
 * region.  Errors and refusals are those of locrec_sg_recommend_batch (LOCREC_E_NOT_FOUND for any unknown
 * vertex before any device work, nothing written); n_places, n_targets and max_recommendations take the checks
 * of locrec_rank_recommendations_batch.  max_recommendations <= 0 or n_places == 0: the iteration still runs,
 * every count is 0.  Afterwards the handle serves single requests and locrec_sg_recommend_batch as before.
 * The segments of a group of requests are ranked by one call of the segmented ranker; a group ends where its
 * rows would pass LOCREC_SG_RANKED_ROW_BUDGET (default 2^24 rows; the result does not depend on it).
 */
int32_t locrec_sg_recommend_ranked_batch(
    locrec_sg_graph *graph, int64_t n_targets, const int64_t *vertex_ids,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    int64_t *out_ids, double *out_probabilities, int64_t *out_counts,
    int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged);
/*
 * The same batch with a caller-given list of ids per position to leave out of the ranking (the places a person
 * has been to: the targets of the vertex's out-edges): position i ranks the rows of vertex_ids[i] whose id is
 * none of excluded_ids[excluded_offsets[i] .. excluded_offsets[i + 1]), as
 * locrec_rank_recommendations_batch_excluding does.  Host arrays; excluded_offsets has n_targets + 1 entries,
 * non-decreasing inside [0, n_excluded], n_excluded < 2^31 - refused with LOCREC_E_INVALID_ARG before any
 * device work otherwise.  A repeated vertex is iterated once; each of its positions is ranked with its own
 * region and its own list.  The emit, the segments' room, out_row_counts, iterations and converged are those of
 * locrec_sg_recommend_ranked_batch, and the result does not depend on LOCREC_SG_RANKED_ROW_BUDGET either.
 */
int32_t locrec_sg_recommend_ranked_batch_excluding(
    locrec_sg_graph *graph, int64_t n_targets, const int64_t *vertex_ids,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids,
    int64_t *out_ids, double *out_probabilities, int64_t *out_counts,
    int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged);
/*
 * Within reach: locrec_sg_recommend_ranked_batch_excluding with a circle per position
 * (locrec_rank_recommendations_batch_near's semantics, requires and refusals; host arrays, checked before the
 * graph is looked at).  excluded_offsets == NULL: no lists.  place_latitudes / place_longitudes: one per row of
 * the place table; center_*, radius_meters: one per position.  out_meters (n_targets x max_recommendations, may
 * be NULL): the distance of each output row, padding 0.0.  The emit and the segments' room see only the region;
 * the group's ranker call applies the circle: out_row_counts, iterations and converged are the plain call's, and
 * the result does not depend on LOCREC_SG_RANKED_ROW_BUDGET.  A repeated vertex is iterated once and ranked per
 * position with its own circle.
 */
int32_t locrec_sg_recommend_ranked_batch_near(
    locrec_sg_graph *graph, int64_t n_targets, const int64_t *vertex_ids,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const double *place_latitudes, const double *place_longitudes,
    const int64_t *target_region_ids,
    const double *center_latitudes, const double *center_longitudes, const double *radius_meters,
    int64_t max_recommendations,
    const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids,
    int64_t *out_ids, double *out_probabilities, double *out_meters, int64_t *out_counts,
    int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged);
/*
 * By category: locrec_sg_recommend_ranked_batch_near with the circles optional (all five coordinate arrays NULL:
 * none, out_meters unused) and an allow-list of categories and a cap per category for every position
 * (locrec_rank_recommendations_batch_by_category's semantics, requires and refusals; host arrays, checked before
 * the graph is looked at).  place_category_ids: one per row of the place table; allowed_offsets (n_targets + 1
 * entries, NULL: no lists), allowed_category_ids (n_allowed entries) and max_per_category (one per position, NULL:
 * no caps) as there.  Lists and caps are uploaded once in emit order and every group's ranker call gets the
 * sub-range of its segments: out_row_counts, iterations and converged are the plain call's, and the result does not
 * depend on LOCREC_SG_RANKED_ROW_BUDGET.  A repeated vertex is iterated once and ranked per position with its own
 * list and cap.
 */
int32_t locrec_sg_recommend_ranked_batch_by_category(
    locrec_sg_graph *graph, int64_t n_targets, const int64_t *vertex_ids,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const double *place_latitudes, const double *place_longitudes, const int64_t *place_category_ids,
    const int64_t *target_region_ids,
    const double *center_latitudes, const double *center_longitudes, const double *radius_meters,
    int64_t max_recommendations,
    const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids,
    const int64_t *allowed_offsets, int64_t n_allowed, const int64_t *allowed_category_ids,
    const int64_t *max_per_category,
    int64_t *out_ids, double *out_probabilities, double *out_meters, int64_t *out_counts,
    int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged);
/*
 * What this thread's last locrec_sg_recommend_ranked_batch (or _excluding) did (any pointer may be NULL): tiles iterated,
 * ranker calls (groups), rows emitted into segments, and every byte the call copied to host memory or had the
 * device write there (state, block sums, polls, results), with the number of waits for the stream.
 */
int32_t locrec_sg_recommend_ranked_batch_stats(
    int64_t *out_tiles, int64_t *out_groups, int64_t *out_emitted_rows,
    int64_t *out_readback_bytes, int64_t *out_host_syncs);

/*
 * SG for visitors: makeRecommendations for persons the graph has no vertex for - they arrived after the cut the graph
 * was built from, or their visits have changed since - without rebuilding it.  Visitor v is given by its out-edges
 * (target_ids[e], weights[e]), e in [edge_offsets[v], edge_offsets[v + 1]): the person -> place and person -> category
 * edges build_balanced_edges would give it.  All arrays are host arrays; visitors carry no id.
 * With G the resident graph (N vertices), every visitor gets what makeRecommendations(V) returns on G + v: G's edge
 * list followed by (V, t_k, w_k) in the given order, V an id no edge of G has.  vertexCount is N + 1 there, V itself is
 * never a row, and V's own squared difference enters isConverged.  A visitor's result depends on G and its own edges
 * only: not on the other visitors of the call, its position or the tile it falls into, bit for bit.
 * A person who IS a vertex of G and comes back as a visitor keeps that vertex in G, as the ordinary source-only
 * vertex it is: its old edges still count as edges of G (nothing points at a person, so they reach no result).
 * Outputs and the capacity protocol are those of locrec_sg_recommend_batch (nv positions; a visitor given twice is
 * computed twice).  Up to 16 visitors share each sweep of the graph, whatever its size.
 * Refused before any device work and before anything but *out_bad_visitor is written; *out_bad_visitor (may be NULL)
 * is the first offending visitor, -1 otherwise:
 *   LOCREC_E_INVALID_ARG  NULL arguments, negative counts, edge_offsets that do not start at 0 or that turn back;
 *                         the constructor's two require()s; sharded, fused or persistent handles
 *                         (locrec_sg_recommend_batch's texts); a target that is a source-only vertex of G (the layout
 *                         has no row for it); a target repeated inside one visitor; a non-finite weight
 *   LOCREC_E_NOT_FOUND    a visitor without edges; a target id that is no vertex of G ("No such vertex in the graph:
 *                         <id>")
 * Any finite weight, zero included, is served (the reference does not check stochasticity either).  nv == 0 succeeds
 * with empty outputs.  Afterwards the handle serves single, batched, ranked and pooled requests exactly as before.
 */
int32_t locrec_sg_visitors_recommend_batch(
    locrec_sg_graph *graph, int64_t nv, const int64_t *edge_offsets, const int64_t *target_ids, const double *weights,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t *out_offsets, int64_t *out_ids, double *out_probabilities, int64_t *inout_capacity,
    int64_t *out_iterations, int32_t *out_converged, int64_t *out_bad_visitor);
/*
 * locrec_sg_recommend_ranked_batch_excluding for visitors: the same tiles to their end, per visitor the places of ITS
 * target region, top max_recommendations by probability, emitted and ranked on the device; x never crosses PCIe.  Row i
 * holds bit for bit what locrec_rank_recommendations_batch_excluding returns for the rows
 * locrec_sg_visitors_recommend_batch returns for visitor i.  excluded_offsets == NULL: nothing is left out (n_excluded
 * and excluded_ids are not read).  Refusals are those of locrec_sg_visitors_recommend_batch and of
 * locrec_sg_recommend_ranked_batch_excluding; the result does not depend on LOCREC_SG_RANKED_ROW_BUDGET.
 * locrec_sg_recommend_ranked_batch_stats reports on this call too.
 */
int32_t locrec_sg_visitors_recommend_ranked_batch(
    locrec_sg_graph *graph, int64_t nv, const int64_t *edge_offsets, const int64_t *target_ids, const double *weights,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids,
    int64_t *out_ids, double *out_probabilities, int64_t *out_counts,
    int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged, int64_t *out_bad_visitor);
/*
 * What this thread's last locrec_sg_visitors_* call did: tiles, visitors, staged edges, lines of the largest tile's
 * weight table, set-up launches, finalize launches, convergence polls, waits for the stream.
 */
int32_t locrec_sg_visitors_stats(int64_t out[8]);
/*
 * What each of n ids is to the graph (host arrays, no device work): 0 = no vertex, 1 = a source-only vertex (no edge
 * points at it: a visitor may not name it), 2 = a live vertex (a visitor's edge may point at it).
 */
int32_t locrec_sg_vertex_kinds(const locrec_sg_graph *graph, int64_t n, const int64_t *vertex_ids, int32_t *out_kinds);

/* Device-resident form (bench.py): enqueue the iteration, read back later. */
int32_t locrec_sg_iterate_async(
    locrec_sg_graph *graph, int64_t vertex_id,
    double alpha, double epsilon, int64_t max_iterations);
/*
 * Exactly `sweeps` applications of calcNextX (:108-128) with the fused convergence sum
 * still computed but never acted on -- the fixed-work form the benchmark times (with
 * epsilon = 0 the reference's loop stops as soon as x reaches an exact fp64 fixed point,
 * which is data dependent).  locrec_sg_fetch() then reports converged = 0.
 */
int32_t locrec_sg_sweeps_async(locrec_sg_graph *graph, int64_t vertex_id, double alpha, int64_t sweeps);
int32_t locrec_sg_fetch(
    locrec_sg_graph *graph,
    int64_t *out_ids, double *out_probabilities, int64_t *inout_count,
    int64_t *out_iterations, int32_t *out_converged);

/*
 * Row-sharded form (one graph over several GPUs; BASELINE.json configs[4]: "SpMV rows sharded ...
 * with RCCL all-reduce of x each iteration").  Every rank creates a handle from the SAME edge list
 * with its own shard_index: the handle keeps the edges whose source vertex falls into the shard
 * ("rows of P"), while the vertex set and the layout of x are global and identical on every rank.
 * One iteration of calcNextX (:108-128) is then
 *     locrec_sg_shard_sigma(g, sigma)      this shard's partial sigma over all live vertices
 *     all-reduce(sum) of sigma[0 .. live)  by the caller, on the handle's stream (RCCL / torch.distributed)
 *     locrec_sg_shard_apply(g, sigma, alpha)
 * and the caller runs step()'s loop (:92-106), reading isConverged's sum with locrec_sg_shard_d2.
 * sigma is a caller-owned DEVICE buffer of locrec_sg_live_count() doubles.  Only the live entries of x
 * are exchanged: a vertex without inbound edges never needs communication.
 */
int32_t locrec_sg_create_sharded(
    int64_t n_edges, const int64_t *source_ids, const int64_t *target_ids, const double *balanced_weights,
    int32_t shard_index, int32_t shard_count, locrec_sg_graph **out_graph);
/*
 * The same protocol with the rows of P^T (targets) sharded: live row l - position l of sigma -
 * belongs to shard l % shard_count, which keeps ALL inbound edges of its rows.  locrec_sg_shard_sigma
 * then yields the complete sigma[l] for the owned l (summed in the single-GPU kernel's fixed order) and
 * 0 elsewhere, so the exchange is an all-GATHER of the owned entries (half the bytes of the all-reduce)
 * and the result is bit-identical to the unsharded one.  begin / sigma / apply / d2 / finish as above.
 */
int32_t locrec_sg_create_target_sharded(
    int64_t n_edges, const int64_t *source_ids, const int64_t *target_ids, const double *balanced_weights,
    int32_t shard_index, int32_t shard_count, locrec_sg_graph **out_graph);
int32_t locrec_sg_live_count(const locrec_sg_graph *graph, int64_t *out_live);
int32_t locrec_sg_shard_begin(locrec_sg_graph *graph, int64_t vertex_id);
int32_t locrec_sg_shard_sigma(locrec_sg_graph *graph, double *sigma_device);
int32_t locrec_sg_shard_apply(locrec_sg_graph *graph, const double *sigma_device, double alpha);
int32_t locrec_sg_shard_d2(locrec_sg_graph *graph, double *out_diff_squared);
int32_t locrec_sg_shard_finish(locrec_sg_graph *graph, int64_t iterations, int32_t converged);

/*
 * A group of independent graphs iterated together (BASELINE.json configs[4]: many graphs per GPU, e.g. one
 * per region pair, PlaceVisits.scala:63-67): one sweep kernel and one combine kernel per round for ALL graphs
 * of the group instead of two launches per graph, on the group's own stream.  The graphs stay usable on their
 * own; after locrec_sg_group_sweeps_async every graph holds its result as after locrec_sg_sweeps_async
 * (same kernels' bodies, bit-identical) and is read with locrec_sg_fetch or awaited with
 * locrec_sg_group_synchronize.  The group does not own the graphs: destroy it before them.
 */
typedef struct locrec_sg_group locrec_sg_group;
int32_t locrec_sg_group_create(locrec_sg_graph *const *graphs, int32_t n_graphs, locrec_sg_group **out_group);
void locrec_sg_group_destroy(locrec_sg_group *group);
int32_t locrec_sg_group_sweeps_async(locrec_sg_group *group, const int64_t *vertex_ids, double alpha, int64_t sweeps);
/* makeRecommendations' iteration (StochasticRecommender.scala:92-106) for every graph of the group: up to
 * max_iterations rounds, each graph stopping at its own isConverged (:130-141); read the results - ids,
 * probabilities, the iteration counter the reference prints, converged or not - with locrec_sg_fetch. */
int32_t locrec_sg_group_iterate_async(locrec_sg_group *group, const int64_t *vertex_ids, double alpha, double epsilon,
                                      int64_t max_iterations);
int32_t locrec_sg_group_synchronize(locrec_sg_group *group);

/*
 * A pool of resident graphs that serves ONE mixed batch of (graph, vertex) requests - the queue of
 * StochasticRecommenderMain's loop, whose lines fan out over the graphs of sorted{home, target}
 * (StochasticRecommenderMain.scala:53-62) - with every graph's current tile of up to 16 targets sharing the
 * launches of a round: per tile wave one set-up launch and one read-back, per round one sweep launch per layout
 * class present (column width x weight form: at most four, one for a pool of one kind) and one finalize launch,
 * on the pool's own stream.
 * create: 1 .. 65535 distinct graphs on one device; the pool does not own them: destroy it before them.  Refused
 * (LOCREC_E_INVALID_ARG, the message names the member): NULL, a graph listed twice, sharded handles, handles of
 * the fused or persistent experiment (the refusals of locrec_sg_recommend_batch) and handles created with
 * LOCREC_SG_PPW / LOCREC_SG_GS (the refusal of locrec_sg_group_create).  Column widths and weight forms may be
 * mixed.  The pool's tables and pinned buffer are sized at create: a repeated call of the same shape makes no
 * device allocation.
 * recommend_batch: request i asks graph graph_index[i] (a position of create's list) for vertex_ids[i].  Rows,
 * offsets, the capacity protocol, the counters and the NULL rules are those of locrec_sg_recommend_batch;
 * request i's rows equal bit for bit what locrec_sg_recommend returns for that vertex on that graph.  A repeated
 * (graph, vertex) pair is iterated once; the same vertex id in two graphs is two requests.  Before any device
 * work every graph index is checked (LOCREC_E_INVALID_ARG), then every vertex (LOCREC_E_NOT_FOUND, "No such
 * vertex in the graph: <id>"); on either failure nothing is written except *out_bad_request (may be NULL): the
 * position of the first offending request; -1 on success.  n_requests == 0: out_offsets[0] = 0, capacity 0.
 * Afterwards every member serves single requests, locrec_sg_recommend_batch and group runs as a fresh handle.
 * stats: this thread's last recommend_batch (any pointer may be NULL): tile waves, rounds, sweep and finalize
 * kernel launches (launches, not graphs), convergence polls, bytes read back.
 */
typedef struct locrec_sg_pool locrec_sg_pool;
int32_t locrec_sg_pool_create(locrec_sg_graph *const *graphs, int32_t n_graphs, locrec_sg_pool **out_pool);
void locrec_sg_pool_destroy(locrec_sg_pool *pool);
int32_t locrec_sg_pool_recommend_batch(
    locrec_sg_pool *pool, int64_t n_requests, const int32_t *graph_index, const int64_t *vertex_ids,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t *out_offsets, int64_t *out_ids, double *out_probabilities, int64_t *inout_capacity,
    int64_t *out_iterations, int32_t *out_converged, int64_t *out_bad_request);
int32_t locrec_sg_pool_stats(int64_t *out_tile_waves, int64_t *out_rounds, int64_t *out_sweep_launches,
                             int64_t *out_finalize_launches, int64_t *out_polls, int64_t *out_readback_bytes);
/*
 * The pool's batch to its end (StochasticRecommenderMain.scala:53-75): request i asks graph graph_index[i] for
 * vertex_ids[i] and gets the places of target_region_ids[i], top max_recommendations by probability - every member's
 * tile emitted and ranked on the device in shared launches; no member's x is read back.  ONE places table serves all
 * members.  The requires, the order of the checks and *out_bad_request are locrec_sg_pool_recommend_batch's (every
 * graph index, then every vertex, before any device work; on a refusal nothing is written but the position); the
 * checks on n_places, the request count, max_recommendations and the arrays, and the outputs - rows of stride
 * max(0, max_recommendations) padded with id -1 / probability 0.0, out_counts, out_row_counts (makeRecommendations'
 * own row count), out_iterations, out_converged, the last three may be NULL - are
 * locrec_sg_recommend_ranked_batch's: request i's values equal bit for bit what that call returns for the request on
 * its member alone, and what locrec_sg_pool_recommend_batch's rows give through locrec_rank_recommendations_batch.
 * The requests are emitted by tile wave, then member, then the ranked batch's order within a tile; a group of that
 * order within LOCREC_SG_RANKED_ROW_BUDGET rows is ranked by one call of the segmented ranker (the result does not
 * depend on the budget).  The pool keeps each member's emit-row image resident from its first ranked call.
 * Afterwards every member is as after locrec_sg_pool_recommend_batch.
 * stats: this thread's last ranked pool call (any pointer may be NULL): tile waves, member tiles, rounds, ranker
 * calls (groups), emit launches, rows emitted into segments, every byte that reached host memory (caps, polls,
 * states, the ranker's headers, ranked rows, the final tail) and the waits for the stream.
 */
int32_t locrec_sg_pool_recommend_ranked_batch(
    locrec_sg_pool *pool, int64_t n_requests, const int32_t *graph_index, const int64_t *vertex_ids,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    int64_t *out_ids, double *out_probabilities, int64_t *out_counts,
    int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged,
    int64_t *out_bad_request);
int32_t locrec_sg_pool_recommend_ranked_batch_stats(
    int64_t *out_tile_waves, int64_t *out_tiles, int64_t *out_rounds, int64_t *out_groups,
    int64_t *out_emit_launches, int64_t *out_emitted_rows, int64_t *out_readback_bytes, int64_t *out_host_syncs);
/*
 * Visitors across a pool: ONE CSR of visitors (locrec_sg_visitors_recommend_batch's), visitor v asked of member
 * graph_index[v].  Visitor v's rows, iterations and converged flag equal bit for bit what
 * locrec_sg_visitors_recommend_batch returns for it on its member alone; the ranked call's row, count and row count equal
 * locrec_sg_visitors_recommend_ranked_batch's on its member alone.  A visitor's result depends on its member and its own
 * edges only - not on the other visitors, the other members, its position, its tile or its wave; a visitor given twice
 * is computed twice.  Offsets, the capacity protocol and the NULL rules are locrec_sg_recommend_batch's; the ranked
 * outputs are locrec_sg_pool_recommend_ranked_batch's (ONE places table serves all members);
 * excluded_offsets == NULL: nothing is left out; the result does not depend on LOCREC_SG_RANKED_ROW_BUDGET.
 * Every member's tile of 16 visitors (wave k of a member: its visitors 16k .. 16k+15 in call order) shares the launches
 * of a round: per call one staging, per wave one set-up pair and one read-back or emit, per round one sweep launch per
 * layout class present and one finalize launch, whatever the number of members.  A member nobody asks costs nothing.
 * All checks run before any device work; on a refusal nothing is written but *out_bad_visitor (may be NULL; -1 on
 * success), in this order:
 *   1. NULL and count checks, the CSR's shape, the constructor's two require()s (locrec_sg_visitors_recommend_batch's
 *      texts; *out_bad_visitor = -1)
 *   2. the ranked call's own arguments and exclusion lists (locrec_sg_recommend_ranked_batch_excluding's)
 *   3. every graph index: LOCREC_E_INVALID_ARG, locrec_sg_pool_recommend_batch's text, the visitor's position
 *   4. the visitors in call order, each against its own member: no edges, a non-finite weight, an unknown id, a
 *      source-only target, a target repeated (locrec_sg_visitors_recommend_batch's codes and texts): the first offender
 *      in call order, whichever member it belongs to
 * nv == 0 succeeds with empty outputs.  Afterwards every member serves single, batched, ranked and visitors requests as
 * a fresh handle would, and the pool its person calls; person calls and visitor calls may alternate on one pool.
 * stats: this thread's last pool visitors call: tile waves, member tiles, visitors, staged edges, stagings, sg_begin_pool
 * launches, set-up launches, rounds, sweep launches, finalize launches, convergence polls, read-backs or emits (one a
 * wave).  locrec_sg_pool_recommend_ranked_batch_stats reports on the ranked call too.
 */
int32_t locrec_sg_pool_visitors_recommend_batch(
    locrec_sg_pool *pool, int64_t nv, const int32_t *graph_index,
    const int64_t *edge_offsets, const int64_t *target_ids, const double *weights,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t *out_offsets, int64_t *out_ids, double *out_probabilities, int64_t *inout_capacity,
    int64_t *out_iterations, int32_t *out_converged, int64_t *out_bad_visitor);
int32_t locrec_sg_pool_visitors_recommend_ranked_batch(
    locrec_sg_pool *pool, int64_t nv, const int32_t *graph_index,
    const int64_t *edge_offsets, const int64_t *target_ids, const double *weights,
    double alpha, double epsilon, int64_t max_iterations,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const int64_t *target_region_ids, int64_t max_recommendations,
    const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids,
    int64_t *out_ids, double *out_probabilities, int64_t *out_counts,
    int64_t *out_row_counts, int64_t *out_iterations, int32_t *out_converged, int64_t *out_bad_visitor);
int32_t locrec_sg_pool_visitors_stats(int64_t out[12]);

int32_t locrec_sg_set_stream(locrec_sg_graph *graph, void *hip_stream);
int32_t locrec_sg_synchronize(locrec_sg_graph *graph);
int32_t locrec_sg_profile_enable(locrec_sg_graph *graph, int32_t on);
/* Summed duration of the sweep (SpMV) kernel and its launch count; resets. */
int32_t locrec_sg_profile_read(locrec_sg_graph *graph, double *out_sweep_ms, int64_t *out_launches);

/* ===================================================================== */
/* Several devices in one process (SURVEY.md 8b "locrec_set_devices", 8e).
 *
 * The Scala host the reference prescribes is ONE JVM: it cannot start a process per GPU.  These entry points are the
 * multi-GPU forms of both paths inside the library - per-device streams, events and peer access, threads only around
 * calls that block - so that one `new KnnRecommender(...)` can use every GPU of the node (csrc/multi.hip).
 * n_devices = 0 (and device_ids NULL) takes the list given to locrec_set_devices, or the current device when there
 * is none.  A device may be listed more than once (logical shards on one GPU: how the one-GPU test box rehearses it).
 */
int32_t locrec_set_devices(int32_t n_devices, const int32_t *device_ids); /* n_devices = 0 forgets the list */

/*
 * KNN, persons (queries) sharded / candidates on every device (BASELINE.json configs[3]).  Create = locrec_knn_create's
 * arguments; set-up is the block all-gather of the CSR arrays in tiles: device r uploads tile r of every array over
 * PCIe, every other device pulls it over xGMI (hipMemcpyPeerAsync) as soon as it has landed, while later tiles are
 * still uploading; then every device builds its index from device arrays (locrec_knn_create_from_device), all at once.
 * The batch calls hand replica r the r-th contiguous share of the queries and run the replicas concurrently; results
 * are those of the single-device calls of the same names, bit for bit (same kernels, same per-query order).
 */
typedef struct locrec_knn_replicas locrec_knn_replicas;
int32_t locrec_knn_replicas_create(
    int32_t n_devices, const int32_t *device_ids, int64_t n, const int64_t *person_ids,
    const int64_t *p_rowptr, const int32_t *p_idx, const double *p_val, int32_t p_dim,
    const int64_t *c_rowptr, const int32_t *c_idx, const double *c_val, int32_t c_dim,
    const int64_t *r_rowptr, const int64_t *r_place, const int64_t *r_rating, locrec_knn_replicas **out_replicas);
void locrec_knn_replicas_destroy(locrec_knn_replicas *replicas);
/* number of replicas; the first replica's index (owned by the handle): single requests go to it */
int32_t locrec_knn_replicas_info(const locrec_knn_replicas *replicas, int32_t *out_devices, locrec_knn_index **out_first);
int32_t locrec_knn_replicas_recommend_batch(
    locrec_knn_replicas *replicas, int64_t nq, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_offsets, int64_t *out_place_ids, double *out_estimated_ratings, int64_t *inout_capacity);
int32_t locrec_knn_replicas_query_batch(
    locrec_knn_replicas *replicas, int64_t nq, const int64_t *person_ids,
    double place_weight, double category_weight, int64_t k_nearest,
    int64_t *out_person_ids, double *out_similarities, int64_t *out_counts);

/*
 * SG, one graph with its rows sharded over the devices (BASELINE.json configs[4]).  by_target = 0: rows of P (sources)
 * sharded, the T live entries of sigma all-REDUCED per sweep - the additions run in device order on every device, so
 * the result is deterministic (to rounding of the unsharded one); by_target = 1: rows of P^T sharded, owned entries
 * all-GATHERED, bit-identical to one device.  The exchange is a kernel reading the peers' sigma buffers directly
 * (peer access; staged peer copies without it), ordered by events: no host synchronisation in a fixed-sweep run,
 * one 8-byte read per sweep (isConverged, StochasticRecommender.scala:99) otherwise.  Results as locrec_sg_recommend.
 */
typedef struct locrec_sg_sharded locrec_sg_sharded;
int32_t locrec_sg_sharded_create(int32_t n_devices, const int32_t *device_ids, int64_t n_edges, const int64_t *source_ids,
                                 const int64_t *target_ids, const double *balanced_weights, int32_t by_target,
                                 locrec_sg_sharded **out_sharded);
void locrec_sg_sharded_destroy(locrec_sg_sharded *sharded);
int32_t locrec_sg_sharded_info(const locrec_sg_sharded *sharded, int32_t *out_devices, int32_t *out_peer_access,
                               int64_t *out_exchanged_entries, int64_t *out_vertices);
int32_t locrec_sg_sharded_recommend(locrec_sg_sharded *sharded, int64_t vertex_id, double alpha, double epsilon,
                                    int64_t max_iterations, int64_t *out_ids, double *out_probabilities,
                                    int64_t *inout_count, int64_t *out_iterations, int32_t *out_converged);
int32_t locrec_sg_sharded_iterate_async(locrec_sg_sharded *sharded, int64_t vertex_id, double alpha, double epsilon,
                                        int64_t max_iterations);
int32_t locrec_sg_sharded_sweeps_async(locrec_sg_sharded *sharded, int64_t vertex_id, double alpha, int64_t sweeps);
/* the result as device `which` of the handle holds it (all hold the same x) */
int32_t locrec_sg_sharded_fetch(locrec_sg_sharded *sharded, int32_t which, int64_t *out_ids, double *out_probabilities,
                                int64_t *inout_count, int64_t *out_iterations, int32_t *out_converged);

/* ===================================================================== */
/* The producers of the two paths' inputs (f-2, f-4).       */
/* Stateless; they run on the current device (locrec_set_device) and      */
/* return when the outputs are complete.  `mem` says where ALL arrays of  */
/* a call live (LOCREC_MEM_HOST / LOCREC_MEM_DEVICE); counts always come  */
/* back through host pointers.                                            */

/*
 * RatingsBuilder.calcRatings (knn/RatingsBuilder.scala:32-48): visits (person_id, entity_id) ->
 * rows (person_id, entity_id, rating = count("*")) whose SQL rank() by rating descending within
 * the person is <= top_n (ties share a rank, so a tie straddling top_n is kept whole).  Rows
 * come back ordered by (person_id, entity_id) - the reference leaves the order undefined.
 * The three outputs need room for n rows; *out_count = rows written.
 */
int32_t locrec_calc_ratings(int64_t n, const int64_t *person_ids, const int64_t *entity_ids, int64_t top_n,
                            int32_t mem, int64_t *out_person_ids, int64_t *out_entity_ids,
                            int64_t *out_ratings, int64_t *out_count);

/*
 * RatingVectorsBuilder.calcRatingVectors (knn/RatingVectorsBuilder.scala:10-25,52-84): ratings
 * (person_id, entity_id, rating: Long) -> one SparseVector per person as CSR: out_person_ids
 * ascending, indices ascending within a person, an index that repeats keeps its FIRST rating in
 * input order (the TreeSet of :43-50 does not replace), values = rating.toDouble (:69),
 * *out_size = max entity id + 1 (:27-34).  An id outside Int range -> LOCREC_E_ARITHMETIC with
 * the reference's message; a negative id or max id == Int.MaxValue -> LOCREC_E_INVALID_ARG (the
 * SparseVector constructor's require()s).  out_person_ids / out_idx / out_val need n entries,
 * out_rowptr n + 1.  The outputs are exactly locrec_knn_create[_from_device]'s vector inputs.
 */
int32_t locrec_calc_rating_vectors(int64_t n, const int64_t *person_ids, const int64_t *entity_ids,
                                   const int64_t *ratings, int32_t mem, int64_t *out_person_ids,
                                   int64_t *out_rowptr, int32_t *out_idx, double *out_val,
                                   int64_t *out_npersons, int64_t *out_nnz, int64_t *out_size);

/*
 * StochasticGraphBuilder.buildWithBalancedWeights (stochastic/StochasticGraphBuilder.scala:8-28):
 * family f's `weight` times betas[f], families concatenated in the given order - the
 * (source_id, target_id, balanced_weight) edge list locrec_sg_create takes.  betas[] / counts[]
 * and the three arrays of per-family pointers are always host memory; `mem` is about the
 * pointed-to columns and the outputs (sum of counts entries each).  n_families <= 0 fails as
 * betas.head of an empty Seq does.
 */
int32_t locrec_build_balanced_edges(int32_t n_families, const double *betas, const int64_t *counts,
                                    const int64_t *const *source_ids, const int64_t *const *target_ids,
                                    const double *const *weights, int32_t mem, int64_t *out_source_ids,
                                    int64_t *out_target_ids, double *out_balanced_weights);

/*
 * The counted edge families of the stochastic graph (StochasticGraphBuilderMain.scala:47-66):
 * PersonLikesPlace.calcPersonLikesPlaceEdges (stochastic/PersonLikesPlace.scala:12-37) with
 * (person_id, place_id), PersonLikesCategory with (person_id, category_id), CategorySelectedPlace
 * with (category_id, place_id) as (source, target) columns of the place visits:
 * count("*") per (source, target) -> SQL rank() by count descending within the source -> keep
 * rank <= top_n (a tie straddling top_n is kept whole) -> weight = count / (sum of the KEPT counts
 * of that source), as double / double, so every source's weights sum to 1 up to rounding.
 * top_n <= 0 keeps nothing.  Rows come back ordered by (source, target) ascending - the same rows
 * in the same order as locrec_calc_ratings.  The three outputs need room for n rows;
 * *out_count = rows written.
 */
int32_t locrec_calc_count_edges(int64_t n, const int64_t *source_ids, const int64_t *target_ids, int64_t top_n,
                                int32_t mem, int64_t *out_source_ids, int64_t *out_target_ids, double *out_weights,
                                int64_t *out_count);

/*
 * PlaceSimilarPlace.calcPlaceSimilarPlaceEdges (stochastic/PlaceSimilarPlace.scala:18-63): every
 * ORDERED pair of visit rows (a, b) of one person with place[a] != place[b] and
 * |timestamp[a] - timestamp[b]| <= interval counts once for (place[a], place[b]) - count("person_id")
 * counts row pairs, not distinct persons, and both (a, b) and (b, a) are pairs; then rank / keep /
 * normalise per source place exactly as locrec_calc_count_edges does.  `interval` is in the unit of
 * the timestamps (the reference: 7 days in milliseconds, :13-14,27); a negative interval or
 * top_n <= 0 gives no rows.  The difference of any two timestamps must fit in int64.  Pair counts
 * are 64-bit.  The candidate pairs are produced and reduced in chunks of at most
 * LOCREC_PREP_PAIR_BUDGET (default 2^28) pairs, so device memory stays bounded however dense the
 * visits are; the result does not depend on the budget.  Rows ordered by (source, target)
 * ascending.  *inout_count: capacity in, rows the result HAS out (may exceed the capacity, then
 * only the first `capacity` rows are written; call with 0 to size the buffers).
 */
int32_t locrec_calc_similar_place_edges(int64_t n, const int64_t *person_ids, const int64_t *place_ids,
                                        const int64_t *timestamps, int64_t interval, int64_t top_n, int32_t mem,
                                        int64_t *out_source_ids, int64_t *out_target_ids, double *out_weights,
                                        int64_t *inout_count);

/* What this thread's last locrec_calc_similar_place_edges did (measurement): candidate pairs produced,
 * chunks they were produced in, and HIP-event milliseconds of its sort / pair-emission / merge-and-rank
 * phases.  Every pointer may be NULL. */
int32_t locrec_similar_place_edges_stats(int64_t *out_pairs, int64_t *out_chunks, double *out_sort_ms,
                                         double *out_emit_ms, double *out_merge_ms);

/*
 * PlaceVisits.calcPlaceVisits (PlaceVisits.scala:11-46): location visits with timestamp >=
 * visits_from (:24) joined with the places of the same region_id (:31) and kept where
 * Location.distanceMeters (Location.scala:30-38, haversine on a 6371 km sphere) <= max_meters
 * (100 in the reference, PlaceVisits.scala:127).  visits_from is calcVisitsFromTimestamp's result
 * (:48-58), computed by the caller in its session time zone; timestamps are opaque int64.
 * Output columns as :40-46 (person_id, timestamp, place_id, region_id, category_id), ordered by
 * (visit row, place row) - the reference leaves the order undefined.  *inout_count: capacity in,
 * number of matches out (may exceed the capacity, then the first `capacity` rows of the full result
 * are written, also where the capacity ends inside one visit's matches; call with 0 to size the buffers).
 * A latitude / longitude outside its range (or NaN) in a row that takes part in the join fails as
 * Location's require does: LOCREC_E_INVALID_ARG with the reference's message, *inout_count =
 * -(1 + visit row) or -(1 + n_visits + place row).
 */
int32_t locrec_calc_place_visits(int64_t n_visits, const int64_t *v_person_ids, const int64_t *v_timestamps,
                                 const double *v_latitudes, const double *v_longitudes,
                                 const int64_t *v_region_ids, int64_t n_places, const int64_t *p_ids,
                                 const double *p_latitudes, const double *p_longitudes,
                                 const int64_t *p_region_ids, const int64_t *p_category_ids,
                                 int64_t visits_from, double max_meters, int32_t mem,
                                 int64_t *out_person_ids, int64_t *out_timestamps, int64_t *out_place_ids,
                                 int64_t *out_region_ids, int64_t *out_category_ids, int64_t *inout_count);

/*
 * The steps around the per-set work of the two builder mains (knn/RatingVectorsBuilderMain.scala:33-76,
 * stochastic/StochasticGraphBuilderMain.scala:36-45), csrc/region_sets.hip.
 *
 * max(timestamp) of PlaceVisits.calcVisitsFromTimestamp (PlaceVisits.scala:50-61); the day arithmetic in the
 * session's time zone stays with the caller.  n == 0 -> LOCREC_E_INVALID_ARG (the reference dereferences a
 * null there); n in [1, 2^31).
 */
int32_t locrec_visits_max_timestamp(int64_t n, const int64_t *timestamps, int32_t mem, int64_t *out_max);

/*
 * PlaceVisits.extractRegionIds (PlaceVisits.scala:69-78): the distinct values of a region_id column,
 * ASCENDING (Spark leaves the order of distinct().collect() undefined; this project defines it).
 * *inout_count: capacity of out_ids in, number of distinct ids out (may exceed the capacity, then the first
 * `capacity` ids are written); out_ids == NULL only counts.  n in [0, 2^31).
 */
int32_t locrec_extract_region_ids(int64_t n, const int64_t *region_ids, int32_t mem, int64_t *out_ids,
                                  int64_t *inout_count);

/*
 * The rows of a table grouped by region, once for all region sets (PlaceVisits.scala:63-67,80-87).
 * region_ids: the n_regions listed regions, strictly ascending (else LOCREC_E_INVALID_ARG), in `mem`.
 * out_rows (n_rows entries, in `mem`): the row numbers 0 .. n_rows - 1 grouped by the rank of their region in
 * region_ids, ascending inside a group.  out_offsets (ALWAYS host memory, n_regions + 2 entries): group g is
 * out_rows[out_offsets[g] : out_offsets[g + 1]]; the last group, g = n_regions, holds the rows whose region is
 * not listed - they belong to no set.  n_rows in [0, 2^31), n_regions in [0, 2^24).
 */
int32_t locrec_region_partition(int64_t n_rows, const int64_t *row_region_ids, int64_t n_regions,
                                const int64_t *region_ids, int32_t mem, int32_t *out_rows, int64_t *out_offsets);

/*
 * The rows of one region set: where(region_id === a or region_id === b) in input order, as the stable merge of
 * the two ascending runs rows[a_begin : a_end] and rows[b_begin : b_end] of locrec_region_partition's out_rows
 * (n_rows entries), with every column gathered through it.  The second run is empty for a single region.
 * cols / out_cols: HOST arrays of n_cols (1 to 8) pointers to int64 columns in `mem`: n_rows entries in, room
 * for (a_end - a_begin) + (b_end - b_begin) entries out.  Before anything is read through `rows` the runs are
 * checked: each strictly ascending, every entry in [0, n_rows), the two ranges inside [0, n_rows] and not
 * overlapping - else LOCREC_E_INVALID_ARG, and nothing is written.
 */
int32_t locrec_region_set_gather(int64_t n_rows, int32_t n_cols, const int64_t *const *cols, const int32_t *rows,
                                 int64_t a_begin, int64_t a_end, int64_t b_begin, int64_t b_end, int32_t mem,
                                 int64_t *const *out_cols);

/* Location.distanceMeters (Location.scala:30-38) of n pairs with the join's own device code
 * (LocationTest.scala:8-27 runs against it); NaN for a pair with an out-of-range coordinate. */
int32_t locrec_distance_meters(int64_t n, const double *lat1, const double *lon1, const double *lat2,
                               const double *lon2, int32_t mem, double *out_meters);

/*
 * printRecommendations of both mains (knn/KnnRecommenderMain.scala:90-101,
 * stochastic/StochasticRecommenderMain.scala:64-75):
 * places.where(region_id === target_region_id) JOIN recommendations ON id, ORDER BY score DESC,
 * LIMIT max_recommendations.  Rows whose id is not a place of the target region (persons,
 * categories, places elsewhere) drop out in the join; a place listed twice counts once; ties
 * (Spark: undefined) are ordered by id ascending, then by input row.  Scores compare as Spark SQL
 * compares doubles: every NaN (either sign, any payload) is one value above +inf, -0.0 equals 0.0.
 * Outputs need room for min(n, max_recommendations) rows; *out_count = rows written.
 */
int32_t locrec_rank_recommendations(int64_t n, const int64_t *ids, const double *scores, int64_t n_places,
                                    const int64_t *place_ids, const int64_t *place_region_ids,
                                    int64_t target_region_id, int64_t max_recommendations, int32_t mem,
                                    int64_t *out_ids, double *out_scores, int64_t *out_count);

/*
 * The same ranking for many row ranges of one (ids, scores) pair at once - the last stage of a batched
 * request (locrec_knn_recommend_batch, locrec_sg_recommend_batch hand back every person's rows as one
 * CSR).  Segment s is rows [offsets[s], offsets[s + 1]); row s of out_ids / out_scores (row-major,
 * stride max(0, max_recommendations)) is exactly what locrec_rank_recommendations returns for those
 * rows with target_region_ids[s], padded with id -1 and score 0.0; out_counts[s] = rows written.
 * `mem` covers every array, offsets, target_region_ids and out_counts included.  offsets must be
 * non-decreasing with offsets[0] >= 0 and offsets[n_segments] <= n (rows outside the segments are
 * ignored); n, n_places and n_segments are < 2^31.  This is checked - for device memory on the device -
 * before anything reads through the offsets: LOCREC_E_INVALID_ARG, nothing written.
 * max_recommendations <= 0, n_segments == 0 or n_places == 0: counts 0, no row is read.
 * Up to LOCREC_RANK_BATCH_MAX_N rows a segment are selected in LDS lists (one block per segment, or per
 * chunk of a long segment plus a merge); a larger limit takes three radix passes over the kept rows.
 * Any limit gives the same answer.  The number of host synchronisations does not depend on n_segments.
 */
#define LOCREC_RANK_BATCH_MAX_N 256
int32_t locrec_rank_recommendations_batch(int64_t n_segments, const int64_t *offsets, int64_t n, const int64_t *ids,
                                          const double *scores, int64_t n_places, const int64_t *place_ids,
                                          const int64_t *place_region_ids, const int64_t *target_region_ids,
                                          int64_t max_recommendations, int32_t mem, int64_t *out_ids,
                                          double *out_scores, int64_t *out_counts);

/*
 * The same with a list of ids per segment to leave out ("recommend only new places"): segment s ranks its
 * rows whose id is none of excluded_ids[excluded_offsets[s] .. excluded_offsets[s + 1]) - exactly what
 * locrec_rank_recommendations returns for those rows, which stay in their input order (the ties fall as
 * before).  Ids match by int64 equality, whatever their region; a list may be unsorted, repeat an id and
 * name ids the segment lacks.  `mem` covers excluded_offsets (n_segments + 1 entries) and excluded_ids
 * (n_excluded < 2^31 entries) as well; excluded_offsets takes the rules and the refusal of offsets, inside
 * [0, n_excluded].  With every list empty the result and the stats are locrec_rank_recommendations_batch's;
 * the host synchronisations are no more in any case (3 at the most).  On the device the lists become one
 * table of (segment, id) pairs sorted by two radix passes, searched per row that passed the region join: a
 * list has no length limit.
 */
int32_t locrec_rank_recommendations_batch_excluding(int64_t n_segments, const int64_t *offsets, int64_t n,
                                                    const int64_t *ids, const double *scores, int64_t n_places,
                                                    const int64_t *place_ids, const int64_t *place_region_ids,
                                                    const int64_t *target_region_ids, int64_t max_recommendations,
                                                    const int64_t *excluded_offsets, int64_t n_excluded,
                                                    const int64_t *excluded_ids, int32_t mem, int64_t *out_ids,
                                                    double *out_scores, int64_t *out_counts);

/*
 * Within reach: the same with a circle per segment.  Segment s keeps a row iff its id is a place of the target
 * region AND some listing of that place in that region has
 * locrec_distance_meters((center_latitudes[s], center_longitudes[s]), listing) <= radius_meters[s] - Spark's
 * places.where(region_id === target && distance <= radius) JOIN rows ON id, a place counting once.  The order,
 * the padding, the radix path above LOCREC_RANK_BATCH_MAX_N and the two environment switches are
 * locrec_rank_recommendations_batch's.  radius_meters[s] >= 0 or +inf; +inf keeps every place of the region
 * (with every radius +inf the ids, scores, counts and stats are the plain / excluding call's bit for bit);
 * radius 0 keeps a place whose coordinates equal the centre.  A place listed several times in the region
 * passes if any listing passes; the listing that counts is the first inside the radius in the table's input
 * order.  out_meters (the shape of out_scores; may be NULL) gets that listing's distance with the bits of
 * locrec_distance_meters, padding 0.0.  excluded_offsets == NULL: no lists (n_excluded, excluded_ids unused);
 * otherwise locrec_rank_recommendations_batch_excluding's lists, combined with the circle.  `mem` covers every
 * array.  LOCREC_E_INVALID_ARG and nothing written, the message naming the argument: a radius that is NaN or
 * negative; a centre or a row of the place table with a latitude outside [-90, 90] or a longitude outside
 * [-180, 180] (NaN fails); NULL coordinate arrays with n_places > 0.  Host arrays are checked on the host
 * before any device work, device arrays on the device before any row is read.  At most 3 host
 * synchronisations.  Not built: a circle that reaches into a second region.
 */
int32_t locrec_rank_recommendations_batch_near(
    int64_t n_segments, const int64_t *offsets, int64_t n, const int64_t *ids, const double *scores,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const double *place_latitudes, const double *place_longitudes,
    const int64_t *target_region_ids,
    const double *center_latitudes, const double *center_longitudes, const double *radius_meters,
    int64_t max_recommendations,
    const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids,
    int32_t mem, int64_t *out_ids, double *out_scores, double *out_meters, int64_t *out_counts);

/*
 * By category: the same with an allow-list of categories and a cap per category for every segment - Spark's
 * places.where(region_id === target && [distance <= radius] && [category_id isin allowed]) JOIN rows ON id, a
 * place counting once, then row_number() OVER (PARTITION BY category ORDER BY score DESC, id, input row) <= cap,
 * then ORDER BY score DESC, id, input row LIMIT max_recommendations.  This is
 * locrec_rank_recommendations_batch_near's argument list with three changes: the five coordinate arrays and
 * out_meters are optional (all five NULL: no circles, out_meters unused); place_category_ids, allowed_offsets,
 * n_allowed, allowed_category_ids and max_per_category are added; `mem` covers every array.
 * place_category_ids: one int64 per row of the place table, any value.  A place listed several times in the
 * target region passes if some listing passes every predicate given (region, circle, allow-list); the listing
 * that counts is the first passing one in the table's input order: its category is the row's category for the
 * cap, its distance the row's out_meters.  The allow-lists are a CSR, segment s's being
 * allowed_category_ids[allowed_offsets[s] .. allowed_offsets[s + 1]) of n_allowed < 2^31 entries:
 * allowed_offsets == NULL is no lists (n_allowed, allowed_category_ids unused), an empty list allows every
 * category, a list may be unsorted, repeat a category and name categories no place has, and a list none of whose
 * categories occurs in the region gives count 0; allowed_offsets takes the rules and the refusal of
 * excluded_offsets, inside [0, n_allowed].  max_per_category: one int64 >= 1 per segment, NULL: no caps.  A row is
 * eligible iff fewer than max_per_category[s] kept rows of its category precede it in the order (score desc, id
 * asc, input row asc); the output is the first max_recommendations eligible rows in that order.  Rows are rows: an
 * id repeated inside a segment counts twice.  A cap >= max_recommendations is no cap.  With no lists and every cap
 * NULL or >= max_recommendations the call runs the plain, excluding or near call's kernels and its ids, score
 * bits, counts, out_meters and stats are theirs bit for bit.
 * Up to LOCREC_RANK_BATCH_MAX_N a capped segment is selected in an LDS list whose entries carry their category: a
 * compaction orders the buffer by (category, score, id, row), drops every entry with `cap` entries of its category
 * in front of it, then keeps the best max_recommendations of the rest - exact, since the eligible rows in front of
 * a row can only grow; a larger limit takes one more radix pass by (segment, category) behind the three.  Any limit
 * gives the same answer.
 * LOCREC_E_INVALID_ARG and nothing written, the message naming the argument: a max_per_category <= 0;
 * place_category_ids NULL with n_places > 0 and lists or caps given; allowed_offsets that break the offset rules;
 * n_allowed outside [0, 2^31); allowed_category_ids NULL with n_allowed > 0; and every refusal of
 * locrec_rank_recommendations_batch_near.  Host arrays are checked on the host before any device work, device
 * arrays on the device before any row is read.  At most 3 host synchronisations.
 */
int32_t locrec_rank_recommendations_batch_by_category(
    int64_t n_segments, const int64_t *offsets, int64_t n, const int64_t *ids, const double *scores,
    int64_t n_places, const int64_t *place_ids, const int64_t *place_region_ids,
    const double *place_latitudes, const double *place_longitudes, const int64_t *place_category_ids,
    const int64_t *target_region_ids,
    const double *center_latitudes, const double *center_longitudes, const double *radius_meters,
    int64_t max_recommendations,
    const int64_t *excluded_offsets, int64_t n_excluded, const int64_t *excluded_ids,
    const int64_t *allowed_offsets, int64_t n_allowed, const int64_t *allowed_category_ids,
    const int64_t *max_per_category,
    int32_t mem, int64_t *out_ids, double *out_scores, double *out_meters, int64_t *out_counts);

/* What the last ranked batch of this thread did (locrec_rank_recommendations_batch and the ranked KNN
 * batches): segments served by one block, segments split into chunks, those chunks, segments that took
 * the radix sort, the membership form (0: binary search in the sorted (region, place id) table),
 * segments ranked from rows the host assembled, and the host synchronisations of the call. */
int32_t locrec_rank_recommendations_batch_stats(int64_t *out_one_block, int64_t *out_split, int64_t *out_chunks,
                                                int64_t *out_sorted, int64_t *out_membership_form,
                                                int64_t *out_host_assembled, int64_t *out_host_syncs);

/*
 * Offline evaluation (csrc/eval.hip; no counterpart in the reference, which has no metric anywhere): the two ends
 * of the hold-out protocol around the builds and the ranked batches above.
 *
 * locrec_eval_ranked_batch scores ranked rows against one list of relevant ids per segment.  rec_ids / rec_counts
 * are what every *_ranked_batch call returns: row s (stride `width`) holds rec_counts[s] ids and then padding, which
 * is never read - a relevant id -1 does not match it.  The relevant lists are CSR: segment s's is
 * rel_ids[rel_offsets[s] .. rel_offsets[s + 1]), unsorted, with repeats and with ids no row has, as it comes; ids are
 * arbitrary int64 and match per (segment, id).  cutoffs: a HOST array of n_cutoffs (1 .. LOCREC_EVAL_MAX_CUTOFFS)
 * values > 0, in any order, repeated or beyond `width` if the caller likes.  For segment s and cutoff k, with
 * c = rec_counts[s], L = min(k, c), R = the distinct ids of the list, position r < L a HIT iff rec_ids[s][r] is in the
 * list and no earlier position of the row holds the same id, h(r) = hits at positions <= r, d[r] = 1 / log2(r + 2):
 *   hits = h(L - 1)   precision = hits / k   recall = hits / R   rr = 1 / (first hit position + 1), 0 without a hit
 *   ap = (sum over hits of h(r) / (r + 1)) / min(R, k)   ndcg = (sum over hits of d[r]) / (sum of d[r], r < min(R, k))
 * A segment with R == 0 gets zeros and is not evaluated.  `mem` covers rec_ids, rec_counts, rel_offsets, rel_ids,
 * out_relevant [n_segments], out_hits [n_segments x n_cutoffs] and out_metrics [n_segments x n_cutoffs x 5, in the
 * order above]; the last two may be NULL, and then nothing per segment but out_relevant leaves the device.  HOST
 * outputs: out_means [n_cutoffs x 6] - the means of the five metrics over the evaluated segments and the share of
 * them with hits > 0, zeros when none is evaluated; out_coverage [n_cutoffs] - the distinct ids at positions
 * < min(k, c) of ALL segments; *out_evaluated - the segments with R > 0.
 * LOCREC_E_INVALID_ARG and nothing written, the message naming the argument: n_cutoffs outside 1 .. 8, a cutoff
 * <= 0, width < 0, n_segments, n_rel or n_segments x width >= 2^31, rel_offsets that are not non-decreasing inside
 * [0, n_rel] (locrec_rank_recommendations_batch's rules), a rec_counts entry outside [0, width], a NULL out_means,
 * out_coverage, out_evaluated or out_relevant.  Host arrays are checked on the host before any device work, device
 * arrays on the device before anything is read through them.  n_segments == 0: zeros and no device work;
 * width == 0: every count is 0, so the metrics and the coverage are zeros and no row is read (out_relevant and
 * *out_evaluated still say what the lists hold).  Rows and lists have no length limit; two host synchronisations
 * whatever n_segments; the same input gives the same bits in every output (fixed summation trees, integer atomics
 * only).  Cutoffs above 2^53 lose bits in precision's division.
 */
#define LOCREC_EVAL_MAX_CUTOFFS 8
int32_t locrec_eval_ranked_batch(int64_t n_segments, int64_t width, const int64_t *rec_ids, const int64_t *rec_counts,
                                 const int64_t *rel_offsets, int64_t n_rel, const int64_t *rel_ids,
                                 int32_t n_cutoffs, const int64_t *cutoffs, int32_t mem,
                                 int64_t *out_relevant, int64_t *out_hits, double *out_metrics,
                                 double *out_means, int64_t *out_coverage, int64_t *out_evaluated);

/* What the last locrec_eval_ranked_batch of this thread did: the (segment, id) entries of the relevant table after
 * de-duplication, the segments evaluated, the host synchronisations, and the path - 1: the wave-per-segment walk
 * (the only one), 0: no device work (no segments, or a refusal on the host). */
int32_t locrec_eval_ranked_batch_stats(int64_t *out_table_entries, int64_t *out_evaluated, int64_t *out_host_syncs,
                                       int64_t *out_path);

/*
 * A visit table (the columns of locrec_calc_place_visits, n < 2^31 rows in `mem`) cut at a time.
 * Train: the rows with timestamp < cut_timestamp, their numbers ascending in out_train_rows (room for n entries, in
 * `mem`; NULL: only counted) - the row list a gather takes; *out_train_count (HOST) their number.
 * Held out: the distinct (person, region, place) triples among the rows with timestamp >= cut_timestamp whose person
 * has at least one train row - with new_places_only != 0 only those whose (person, place) has no train row -
 * sorted by person, then region, then place, ascending as signed int64.  *inout_held_count (HOST): capacity in,
 * number of triples out, with locrec_calc_place_visits' protocol: it may exceed the capacity, then the first
 * `capacity` triples are written; any of the three outputs NULL only counts.  At most four host synchronisations
 * whatever n.
 */
int32_t locrec_holdout_split(int64_t n, const int64_t *person_ids, const int64_t *timestamps, const int64_t *place_ids,
                             const int64_t *region_ids, int64_t cut_timestamp, int32_t new_places_only, int32_t mem,
                             int32_t *out_train_rows, int64_t *out_train_count,
                             int64_t *out_person_ids, int64_t *out_region_ids, int64_t *out_place_ids,
                             int64_t *inout_held_count);

/* ===================================================================== */
/* The place deduplicator (deduplicator/PlaceDeduplicator.scala,          */
/* deduplicator/Levenshtein.scala).  Stateless, on the current device,    */
/* with the producers' conventions for `mem` and counts.                  */
/* Names are CSR: int64 offsets[n + 1] (offsets[0] >= 0, never decreasing) */
/* plus uint16 UTF-16 code units, ALREADY LOWER-CASED by the caller:      */
/* toLowerCase is the host language's own, locale rules included, so the  */
/* library compares the units as given (a surrogate pair is two units,    */
/* as Java chars are).  Names have no length limit.                       */

/*
 * Levenshtein.lev (deduplicator/Levenshtein.scala:18-57) of n pairs (a[i], b[i]).
 * max_difference < 0: the exact distance.  max_difference >= 0: min(lev, max_difference + 1),
 * computed by the very kernel locrec_find_duplicate_places uses for that threshold - this function
 * is to the deduplicator what locrec_distance_meters is to the visit join.  n in [0, 2^31).
 */
int32_t locrec_lev_distances(int64_t n, const int64_t *a_offsets, const uint16_t *a_units, const int64_t *b_offsets,
                             const uint16_t *b_units, int32_t max_difference, int32_t mem, int32_t *out_distances);

/*
 * PlaceDeduplicator(maxPlaceDistanceMeters, maxNameDifference).dropDuplicates
 * (deduplicator/PlaceDeduplicator.scala:13-54).  A pair is (place p, confirmed place c) with equal
 * region_id (:39) and different id (:40).  It is SAME when distanceMeters(p, c) <= max_meters and
 * lev(p.name, c.name) <= max_name_difference (:34-35, negated).  The same pairs come back as
 * (place row, confirmed row, exact name difference), ordered by (place row, confirmed row).
 * *inout_count: capacity in, number of same pairs out (may exceed the capacity, then the first
 * `capacity` rows of the full result are written; call with 0 to size the buffers).
 * out_not_same_counts (n_places entries, may be NULL): (confirmed rows of place i's region whose id
 * differs from p_ids[i]) - (same pairs of place i) - how often the reference's literal inner join
 * (:38-53) returns place i.  A place whose region has no confirmed place gets 0.
 * max_meters < 0 or max_name_difference < 0 is legal: no pair can be same.
 * Limits of this implementation (not reference behaviour): max_meters NaN or >= the earth radius
 * (6371 km) fails with LOCREC_E_INVALID_ARG - the grid cannot prune there, as in
 * locrec_calc_place_visits; at most 2^24 - 1 distinct regions; row counts in [0, 2^31).
 * A latitude / longitude outside its range (or NaN) in a row whose region has at least one row on
 * the other side fails as Location's require does (Location.scala:7-8): LOCREC_E_INVALID_ARG with
 * the reference's message, *inout_count = -(1 + place row) or -(1 + n_places + confirmed row).
 * The candidates (pairs within the radius) are produced and compared in chunks of places of at most
 * LOCREC_DEDUP_PAIR_BUDGET (default 2^26) pairs; the result does not depend on the budget.
 */
int32_t locrec_find_duplicate_places(
    int64_t n_places, const int64_t *p_ids, const int64_t *p_region_ids, const double *p_latitudes,
    const double *p_longitudes, const int64_t *p_name_offsets, const uint16_t *p_name_units,
    int64_t n_confirmed, const int64_t *c_ids, const int64_t *c_region_ids, const double *c_latitudes,
    const double *c_longitudes, const int64_t *c_name_offsets, const uint16_t *c_name_units,
    double max_meters, int32_t max_name_difference, int32_t mem,
    int64_t *out_place_rows, int64_t *out_confirmed_rows, int32_t *out_name_differences, int64_t *inout_count,
    int64_t *out_not_same_counts);

/* What this thread's last locrec_find_duplicate_places did (measurement): candidate pairs (within the
 * radius, ids differ), same pairs, chunks, and HIP-event milliseconds of its grid (keys, sorts, walks),
 * Levenshtein and compaction phases.  Every pointer may be NULL. */
int32_t locrec_find_duplicate_places_stats(int64_t *out_candidates, int64_t *out_same, int64_t *out_chunks,
                                           double *out_grid_ms, double *out_lev_ms, double *out_compact_ms);

/* ===================================================================== */
/* The sample generator (sample/LocationVisitsSampleGenerator.scala,      */
/* sample/PlacesSampleGenerator.scala, sample/SampleGeneratorMain.scala), */
/* csrc/sample.hip.  Stateless, on the current device, with the           */
/* producers' conventions: `mem` names where the COLUMN arrays live;      */
/* region tables (ids, boxes), category-name tables and counts are always */
/* host memory; a call returns when its outputs are complete.             */
/* Regions: n_regions in [1, 2^24) distinct non-negative ids; boxes are   */
/* [n_regions][4] = minLatitude, maxLatitude, minLongitude, maxLongitude, */
/* finite, min <= max, inside [-90, 90] x [-180, 180].                    */
/* Random numbers: Spark's rand(seed) depends on the partition layout and */
/* cannot be reproduced (parity unpinned).  Every factor here is          */
/* u01(seed, stream, row, slot) of the package's counter-based generator  */
/* (synth.u01: three splitmix64 steps, (k >> 11) * 2^-53), bit-identical  */
/* on host and device; DESIGN.md section 9b gives the keying.             */

/*
 * generatePersons (LocationVisitsSampleGenerator.scala:55-68): ppr = person_count / n_regions (integer
 * division, the remainder is dropped); region r of the list, in the GIVEN order, gets the ids
 * min_person_id + r.id * ppr ... min_person_id + (r.id + 1) * ppr - 1 ascending - the formula uses the region's
 * id, not its position - with home_region_id = r.id.  The outputs need room for ppr * n_regions rows;
 * *out_count = rows written.  An id range that leaves int64: LOCREC_E_INVALID_ARG.
 */
int32_t locrec_sample_persons(int32_t n_regions, const int64_t *region_ids, int64_t person_count,
                              int64_t min_person_id, int32_t mem, int64_t *out_ids, int64_t *out_home_region_ids,
                              int64_t *out_count);

/*
 * withVisits / withGeoLocations / withTimestamps (LocationVisitsSampleGenerator.scala:78-133) for the persons
 * table (person_ids, home_region_ids; n_persons rows in `mem`).  Person row p has the index
 * person_index_base + p, and its rows depend on (seed, that index) alone: a shard of the persons generated
 * with its own base reproduces the rows of the whole table.  The person gets
 * (int)(f * max_visits_per_person) + 1 rows, f = u01(seed, 1, index, 0); row k of it carries
 *   person_id, region_id = the home region,
 *   latitude  = minLat + (maxLat - minLat) * g_lat, longitude likewise (fp64, three separate operations),
 *   timestamp = from_timestamp_ms + (long)(interval_hours * g_t) * 3,600,000   (epoch milliseconds),
 *   year_month = year * 100 + month of the timestamp (int32, e.g. 201803), by a civil-from-days computation
 *   in UTC with floor division (right before 1970, leap years with the century rules).  Spark's year() and
 *   month() would use the session time zone; the reference's launcher leaves it at the JVM's default.
 * shared_factor = 1: g_lat = g_lon = g_t = u01(seed, 2, index, 3k) - in the reference the three columns are
 * rand(0) over the same rows, one stream, so a visit lies on its region's diagonal.  shared_factor = 0:
 * g_lat, g_lon, g_t = u01(seed, 2, index, 3k / 3k + 1 / 3k + 2).
 * Rows are ordered by (person row, k).  *inout_count: capacity in, rows the result HAS out (may exceed the
 * capacity, then the first `capacity` rows of the full result are written; call with 0 to size the buffers,
 * the outputs may then be NULL).  Counts and offsets are 64-bit: the generator has no 2^31 limit (the
 * producers downstream have).  A person whose home region is not listed fails with LOCREC_E_INVALID_ARG
 * naming the first such row, as regions.find(...).get throws (:33-36).  max_visits_per_person in [1, 2^31),
 * interval_hours >= 0, and the whole interval within 100,000,000 days of 1970.
 */
int32_t locrec_sample_location_visits(int64_t n_persons, const int64_t *person_ids, const int64_t *home_region_ids,
                                      int64_t person_index_base, int32_t n_regions, const int64_t *region_ids,
                                      const double *region_boxes, int64_t from_timestamp_ms, int64_t interval_hours,
                                      int64_t max_visits_per_person, uint64_t seed, int32_t shared_factor,
                                      int32_t mem, int64_t *out_person_ids, int64_t *out_region_ids,
                                      double *out_latitudes, double *out_longitudes, int64_t *out_timestamps,
                                      int32_t *out_year_months, int64_t *inout_count);

/* What this thread's last locrec_sample_location_visits did (measurement): rows written, bytes written
 * (44 a row), and HIP-event milliseconds of its count-and-scan phase and of its fill phase.  Every pointer
 * may be NULL. */
int32_t locrec_sample_location_visits_stats(int64_t *out_rows, int64_t *out_bytes, double *out_count_ms,
                                            double *out_fill_ms);

/*
 * withGeo / withCategories (PlacesSampleGenerator.scala:41-77): ppr = place_count / n_regions,
 * c = floor(sqrt(ppr)) (computed on the host; ppr == 0 gives no places and no division); every region of the
 * list, in the given order, gets a c x c grid, latitude index outer, both indices from 1:
 *   latitude = minLat + latStep * latIdx with latStep = (maxLat - minLat) / c, longitude likewise,
 *   id = min_place_id + r.id * c^2 + (latIdx - 1) * c + (lonIdx - 1),
 *   category_id = min_category_id + (long)(f * n_categories), f = u01(seed, 3, place row, 0).
 * The outputs need room for c^2 * n_regions rows; *out_count = rows written.  place_count in [0, 2^52],
 * n_categories in [1, 2^31); an id range that leaves int64: LOCREC_E_INVALID_ARG.
 */
int32_t locrec_sample_places(int32_t n_regions, const int64_t *region_ids, const double *region_boxes,
                             int64_t place_count, int64_t min_place_id, int64_t n_categories,
                             int64_t min_category_id, uint64_t seed, int32_t mem, int64_t *out_ids,
                             double *out_latitudes, double *out_longitudes, int64_t *out_region_ids,
                             int64_t *out_category_ids, int64_t *out_count);

/*
 * withNames (PlacesSampleGenerator.scala:79-90): name = description = "<category name>-<id>" of n places as
 * the CSR locrec_find_duplicate_places takes: out_offsets int64[n + 1] plus UTF-16 code units.  The category
 * names are a HOST CSR of n_categories names (offsets[n_categories + 1], units), entry category_id -
 * min_category_id; their units are copied as they are.  Ids are non-negative (up to 19 digits); a negative id
 * or a category outside the table fails with LOCREC_E_INVALID_ARG naming the first such row.  Two phases:
 * lengths, a scan, the fill.  *inout_units: capacity of out_units in, units the result HAS out (may exceed the
 * capacity, then the first `capacity` units are written; with capacity 0 out_offsets and out_units may be
 * NULL).  out_offsets, when given, is always written whole.
 */
int32_t locrec_sample_place_names(int64_t n, const int64_t *place_ids, const int64_t *category_ids,
                                  int64_t min_category_id, int64_t n_categories,
                                  const int64_t *category_name_offsets, const uint16_t *category_name_units,
                                  int32_t mem, int64_t *out_offsets, uint16_t *out_units, int64_t *inout_units);

#ifdef __cplusplus
}
#endif
#endif /* LOCREC_H */
