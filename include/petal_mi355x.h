/*
 * petal_mi355x.h -- C ABI of the MI355X-native exact k-NN engine that drops in
 * behind petal-neighbors' BallTree::{euclidean, query, query_radius,
 * query_nearest} and distance::{Euclidean, pairwise}.
 *
 * petal-neighbors (Rust, /root/reference) has no FFI of its own: its boundary
 * is the public Rust API.  Each entry point below cites the reference item it
 * replaces (file:line relative to the reference checkout).  INTEGRATION.md
 * shows the Rust `extern "C"` block + safe wrapper a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no exceptions, no C++ or torch types.
 *   - every function returns PN_OK (0) or a PN_ERR_* code; pn_last_error()
 *     returns a thread-local message for the last failure on this thread.
 *   - strides are in ELEMENTS, not bytes.
 *   - "host" entry points take host pointers (what an ndarray hands over), do
 *     the PCIe transfers themselves and return when the results are in the
 *     caller's buffers; "_device" entry points take pointers into the index's
 *     GPU memory and a hipStream_t (as void*; NULL = HIP's default stream),
 *     ENQUEUE all their work on that stream and return without waiting for it
 *     and without reading anything back: results are ready in stream order
 *     (synchronise the stream, or keep enqueueing consumers on it).  Even the
 *     second tier for queries the first tier could not prove is enqueued
 *     unconditionally and sized by a count that stays on the device.
 *   - results are written into caller-allocated buffers; the only
 *     library-allocated result (radius CSR indices) is released with pn_free.
 *   - all query functions are re-entrant on a shared `const pn_index*`
 *     (BallTree queries take &self and `Euclidean: Sync`, src/distance.rs:19):
 *     every call works in its own pooled workspace, calls from several host
 *     threads run side by side; create/destroy/set_option must not race with
 *     queries on the same handle.
 *   - statistics (pn_index_get_stats) are collected lazily: that call waits
 *     for the device and then reads the counters the kernels kept.
 *   - there is NO CPU fallback: if no usable GPU is present every compute entry
 *     point fails with PN_ERR_DEVICE.
 *
 * Result contract
 *   - distances are bit-identical to the reference's sequential, unfused
 *     fold + sqrt (src/distance.rs:26-35) in the index's element type.
 *   - neighbours are ordered by (distance, index); NaN distances sort last
 *     (ordered-float semantics used at src/ball_tree.rs:396-421).  The
 *     reference's order inside groups of exactly equal distances is
 *     unspecified (it depends on tree shape and heap internals); this library
 *     returns ascending index there.
 */
#ifndef PETAL_MI355X_H
#define PETAL_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 4): + pn_query_radius_device_*, pn_sharded_query_radius_device_*, pn_bf16_selftest,
 * pn_debug_seed_model_feedback, PN_OPT_BF16_WAVES, PN_OPT_SEED_MODEL, pn_info.seed_model (the former reserved word);
 * PN_OPT_MFMA_STRUCTURE = 1 is now PN_ERR_INVALID.  Everything of version 2 is unchanged.
 * Additive within version 3 (callers detect them by symbol): pn_query_radius_with_distance_{,device_}{f32,f64},
 * pn_sharded_query_radius_with_distance_{,device_}{f32,f64}, PN_RADIUS_SORTED; pn_query_self_{,device_}{f32,f64},
 * pn_query_radius_self_{,device_}{f32,f64}, PN_SELF_INCLUDE; pn_sharded_query_self_{,device_}{f32,f64},
 * pn_sharded_query_radius_self_{,device_}{f32,f64}; pn_query_radii_{,device_,self_,self_device_}{f32,f64};
 * pn_dbscan_{,device_}{f32,f64}, PN_OPT_DBSCAN_PIECE; pn_mst_{,device_}{f32,f64}, PN_OPT_MST_BATCH;
 * pn_linkage_{,device_}{f32,f64}, pn_hdbscan_{,device_}{f32,f64}; pn_lof_{,device_}{f32,f64},
 * pn_lof_score_{,device_}{f32,f64}; pn_knn_classify_{,device_,self_,self_device_}{f32,f64},
 * pn_knn_regress_{,device_,self_,self_device_}{f32,f64}, PN_KNN_WEIGHT_DISTANCE;
 * pn_optics_{,device_}{f32,f64}, pn_optics_dbscan_{,device_}{f32,f64},
 * PN_OPT_OPTICS_PIECE; pn_kde_{,device_,self_,self_device_}{f32,f64}, PN_KDE_*, PN_OPT_KDE_PIECE;
 * pn_mean_shift_{,device_,merge_,merge_device_,labels_,labels_device_}{f32,f64}, PN_MS_*, PN_OPT_MS_PIECE;
 * pn_kmeans_{,device_}{f32,f64}, pn_kmeans_assign_{,device_}{f32,f64}, pn_kmeans_bounds_f32,
 * PN_OPT_KMEANS_FILTER. */
#define PN_ABI_VERSION 3

/* ---- error codes.  EMPTY / NOT_CONTIGUOUS are ArrayError (src/lib.rs:9-16). */
enum {
    PN_OK = 0,
    PN_ERR_EMPTY = 1,          /* "array is empty"                     src/ball_tree.rs:44-46 */
    PN_ERR_NOT_CONTIGUOUS = 2, /* "array is not contiguous in memory"  src/ball_tree.rs:47-49 */
    PN_ERR_INVALID = 3,        /* NULL pointer / bad argument (no reference counterpart) */
    PN_ERR_DEVICE = 4,         /* HIP failure or no GPU */
    PN_ERR_NOMEM = 5,
    PN_ERR_UNSUPPORTED = 6,
    PN_ERR_EMPTY_MATRIX = 7,   /* zero columns with >= 2 rows: the reference panics "empty matrix" (src/ball_tree.rs:582) */
    PN_ERR_COMM = 8            /* RCCL failure, or RCCL not loadable (row-sharded corpora only) */
};

/* engine selection, PN_OPT_ENGINE */
enum {
    PN_ENGINE_AUTO = 0,  /* bf16 filter -> f32 MFMA filter -> exact scan, each tier taking what the previous
                            one could not prove; tiers that cannot serve the index are skipped */
    PN_ENGINE_EXACT = 1, /* exact VALU scan only (always bit-exact by construction) */
    PN_ENGINE_MFMA = 2,  /* force the f32 MFMA filter path (f32 only); verified, falls back per query */
    PN_ENGINE_BF16 = 3   /* force the bf16 MFMA filter as first tier (f32, D <= 1024); verified, falls back per query */
};

enum {
    PN_OPT_ENGINE = 1,
    PN_OPT_SEGMENTS = 2,    /* corpus row segments per query tile; 0 = auto */
    PN_OPT_INDEX_BASE = 3,  /* added to every returned index (row-sharded corpora) */
    PN_OPT_PROFILE = 4,     /* 1: bracket the dominant kernel with hipEvents on its stream (hot_ms); 2: also the whole
                               call (last_call_ms) -- every event record costs the stream a few microseconds */
    PN_OPT_FILTER_SLOTS = 5, /* k' kept by the MFMA filter per (query, segment); 0 = auto */
    PN_OPT_MFMA_STRUCTURE = 6, /* f32 MFMA tier: 0 auto; 2 = persistent partition, LDS candidate buffers, 1 workgroup/CU;
                                 3 = persistent partition, HBM candidate buffers, 2 workgroups/CU (1, the first
                                 structure -- a (query tile x segment) grid -- was retired in round 4: PN_ERR_INVALID).
                                 The LDS buffers of structure 2 hold k' <= 30 candidates per (query, segment): a call
                                 that needs more (k above 27, or PN_OPT_FILTER_SLOTS above 30) is not an error -- the
                                 f32 MFMA tier steps aside and the next tier answers it, as for every k' the tier
                                 cannot hold */
    PN_OPT_EXCHANGE_ALWAYS = 7, /* pn_sharded_set_option only.  A handle with ONE shard answers straight into the
                                  caller's buffers (nothing to exchange); 1 sends it through the packed buffer, the
                                  all-gather and the merge all the same (tests: RCCL at world size 1) */
    PN_OPT_SHARED_THRESHOLDS = 8, /* bf16 tier, plans with several row segments per query: 1 (default) = the segments
                                  of a query tighten each other's thresholds while the filter runs (refresher
                                  workgroups in the idle workgroup slots); 0 = off; n >= 2 = on with the shared
                                  threshold at the n-th smallest bound of the union (experiments).  Never changes a
                                  result: only how many candidates the filter keeps. */
    PN_OPT_BF16_WAVES = 9,       /* bf16 tier, narrow rows, main pass of a k-NN call: 0 (default) = the library picks -- the
                                  8-wave kernel (one 32-query column block per wave, four waves per SIMD) for short runs,
                                  the 4-wave kernel (two column blocks per wave, two waves per SIMD) or, for long runs
                                  over at least two query tiles with 64-slot buffers and no refreshers on a grid that
                                  fills every workgroup slot of the device, the paired
                                  kernel (one 8-wave workgroup per CU over two query tiles, its SIMD partners in
                                  anti-phase); 4 / 8 = always that kernel where it applies; 16 = the paired kernel where
                                  it applies, else the 4-wave kernel; 32 = likewise the paired kernel with two row tiles
                                  per workgroup meeting.  Never changes a result (A/B measurements, tests of all the
                                  kernels). */
    PN_OPT_SEED_MODEL = 10,      /* bf16 tier, indexes of narrow rows (D <= 128) whose seed model was accepted at build
                                  (pn_info.seed_model): 1 (default) = k-NN calls with k <= 128 take their starting
                                  thresholds from the model (no scout launch); 0 = always scout.  Never changes a result:
                                  a threshold only decides which tier answers a query. */
    PN_OPT_DBSCAN_PIECE = 11,    /* pn_dbscan_*: the most list entries (64-bit indices in workspace scratch) one piece of
                                  the union stage holds; 0 (default) = 2^27, i.e. 1 GiB.  A row whose own list is longer
                                  is a piece of its own.  Never changes a result. */
    PN_OPT_MST_BATCH = 12,       /* pn_mst_*: the most listed rows one scan launch takes; 0 (default) = 2^18, the
                                  self-queries' chunk; negative: PN_ERR_INVALID.  Never changes a result (it lets tests
                                  force several launches per round at small n). */
    PN_OPT_OPTICS_PIECE = 13,    /* pn_optics_*: the most list entries one piece of the graph fill holds in workspace
                                  scratch before it is packed into the graph store; 0 (default) = 2^27; negative:
                                  PN_ERR_INVALID.  A row whose own list is longer is a piece of its own.  Never changes a
                                  result (it lets tests force several pieces at small n). */
    PN_OPT_KDE_PIECE = 14,       /* pn_kde_*: the most list entries (a 64-bit index and a distance each, in workspace
                                  scratch) one piece of the sum stage holds; 0 (default) = 2^27; negative: PN_ERR_INVALID.
                                  A query whose own list is longer is a piece of its own.  Never changes a result. */
    PN_OPT_MS_PIECE = 15,        /* pn_mean_shift_*: the most list entries (a 64-bit index each, in workspace scratch) one
                                  piece of an iteration's step stage holds; 0 (default) = 2^27; negative: PN_ERR_INVALID.
                                  A seed whose own list is longer is a piece of its own.  Never changes a result. */
    PN_OPT_KMEANS_FILTER = 16    /* pn_kmeans_*: 0 (default) = PN_OPT_ENGINE decides; 1 = the MFMA filter wherever it is
                                  eligible (8 <= dim <= 320), on any handle; 2 = never.  Other values: PN_ERR_INVALID.
                                  Never changes a result (it lets tests force the filter at small n). */
};

/* kernels of pn_kde_* (scikit-learn's names; its sixth, `cosine`, is left out: the name collides with the Cosine metric
 * and its normaliser is an alternating series that cancels to a negative number at D = 16) */
enum {
    PN_KDE_GAUSSIAN = 0,
    PN_KDE_TOPHAT = 1,
    PN_KDE_EPANECHNIKOV = 2,
    PN_KDE_EXPONENTIAL = 3,
    PN_KDE_LINEAR = 4
};

typedef struct pn_index pn_index;

typedef struct pn_info {
    uint64_t n_points; /* BallTree::num_points  src/ball_tree.rs:351-353 */
    uint64_t dim;
    uint64_t row_stride_device; /* padded row length in HBM (elements) */
    int32_t elem_bytes;         /* 4 = f32, 8 = f64 */
    int32_t device;
    int32_t mfma_eligible; /* 1 when the f32 MFMA filter path can serve this index */
    int32_t bf16_eligible; /* 1 when the bf16 MFMA filter path can serve this index */
    int32_t bf16_layout;   /* 0 none; 1 = five extra columns per row; 2 = row norm as the accumulator's initial value and
                              a per-query error constant (rows of homogeneous norm, D mod 16 in {0, 12..15}) */
    int32_t seed_model;    /* 1 when the index's seed model was accepted at build: uniform-like
                              corpora; clustered ones keep the scout launch */
} pn_info;

typedef struct pn_stats {
    uint64_t queries;          /* k-NN queries served */
    uint64_t fallback_queries; /* queries whose MFMA-filter result failed verification and were re-run exactly */
    uint64_t candidates;       /* candidates re-ranked exactly */
    uint64_t hot_launches;     /* launches of the dominant kernel inside profiled calls */
    double hot_ms;             /* their summed hipEvent duration (PN_OPT_PROFILE=1) */
    double last_call_ms;       /* hipEvent duration of the whole last profiled *_device call */
    uint64_t radius_results;
    uint64_t evaluations;      /* candidates whose exact distance was actually computed (the others were proven
                                  farther than the k-th from their filter bound alone) */
    double shard_ms;           /* pn_sharded_* under PN_OPT_PROFILE: summed hipEvent time of the local half of the calls
                                  (every local shard's filter + re-rank + local merge) ... */
    double exchange_ms;        /* ... and of their exchange half (pack is in the local half; ncclAllGather + final merge) */
    uint64_t reserved[1];
} pn_stats;

const char *pn_last_error(void);
const char *pn_strerror(int code);
int pn_abi_version(void);
int pn_device_count(int *count);

/* ---- construction: BallTree::new / BallTree::euclidean
 * (src/ball_tree.rs:38-63, 367-373).  Validation is the reference's: zero
 * rows -> PN_ERR_EMPTY; inner (column) stride != 1 with more than one column
 * -> PN_ERR_NOT_CONTIGUOUS (only the inner stride is checked, as at :47); the
 * row stride is free.  The host array is borrowed for the duration of the
 * call only; the index keeps a zero-padded copy in HBM (plus row norms).
 * The ball tree itself is not built: the walk is replaced by a batched scan. */
int pn_index_create_f32(const float *points, size_t n_rows, size_t n_cols, ptrdiff_t row_stride,
                        ptrdiff_t col_stride, int device, pn_index **out);
int pn_index_create_f64(const double *points, size_t n_rows, size_t n_cols, ptrdiff_t row_stride,
                        ptrdiff_t col_stride, int device, pn_index **out);
/* BallTree::new(points, Cosine) (src/ball_tree.rs:38 with src/distance.rs:76-122).  Cosine distance is not a metric
 * (no triangle inequality), so the reference's ball-pruned walk may skip true neighbours under it and its answers
 * depend on the tree's shape; this engine does not walk a tree: every query function on a Cosine index returns the EXACT
 * answer -- the k smallest (Cosine::distance, index) / every row with Cosine::distance < r -- in the reference's
 * arithmetic (three sequential sums, 1 - dot / (|a| |b|), zip-truncated dot product).  Where the reference's walk prunes
 * nothing the two agree bit for bit; where it prunes wrongly this engine returns the true nearest rows.
 * MEASURED DEVIATION (tests/test_gpu_tree_chain.py, the oracle's faithful walk under Cosine vs this index, 256 queries
 * each, uniform [-0.5, 0.5) data, profiles/r04_tree_chain.log): 60 000 x 16, k = 10: the walk misses a true neighbour on
 * 77.7 % of the queries; 20 000 x 3, k = 5: 64.8 %; 200 000 x 128, k = 10: 0 % (at that dimension the walk prunes nothing).
 * Wherever the answers differ, every entry of this index's answer is at most the walk's entry of the same rank.
 * Engines: k-NN on an index whose rows all have a squared norm inside [2^-100, 2^100] is served by the bf16 MFMA filter
 * over the rows NORMALISED in f64 (|q/|q| - p/|p||^2 = 2 (1 - cos): the Euclidean tier's images and kernels, DESIGN.md
 * 4.8) + a re-rank that evaluates Cosine::distance itself + a per-query proof; query_radius with 0 < r < 1 by the same
 * filter against each query's fixed bound + the Cosine::distance check of its survivors (1M x 128, 10^4 queries: 2.1 ms
 * against the exact scan's 126); unproven queries, queries of another length than the rows, other radii and every other
 * index take the exact scan.  Results never depend on the filter. */
int pn_index_create_cosine_f32(const float *points, size_t n_rows, size_t n_cols, ptrdiff_t row_stride,
                               ptrdiff_t col_stride, int device, pn_index **out);
int pn_index_create_cosine_f64(const double *points, size_t n_rows, size_t n_cols, ptrdiff_t row_stride,
                               ptrdiff_t col_stride, int device, pn_index **out);
/* same, from rows already resident on `device` (row-major, inner stride 1) */
int pn_index_create_device_f32(const float *d_points, size_t n_rows, size_t n_cols, size_t row_stride,
                               int device, void *stream, pn_index **out);
int pn_index_create_device_f64(const double *d_points, size_t n_rows, size_t n_cols, size_t row_stride,
                               int device, void *stream, pn_index **out);
void pn_index_destroy(pn_index *index);
int pn_index_info(const pn_index *index, pn_info *out);
int pn_index_set_option(pn_index *index, int option, int64_t value);
int pn_index_get_stats(const pn_index *index, pn_stats *out, int reset);

/* ---- k-NN: BallTree::query (src/ball_tree.rs:102-121, 203-243) for a batch of
 * queries (the reference takes one point per call; nq = 1 is that call).
 * q_cols is the length of each query vector: like the reference's `zip`
 * (src/distance.rs:27-28) the distance runs over min(q_cols, dim) coordinates.
 * Writes nq rows of kout = min(k, n_points) results, ascending by distance;
 * k = 0 writes nothing and succeeds (src/ball_tree.rs:106-108).  Never fails on
 * NaN coordinates (CHANGELOG.md:113-115).
 * One point per call is a supported pattern: corpora of at most 4096 rows answer a call of <= 64 queries with one
 * kernel launch (query and answer through mapped pinned memory); a handful of queries against a large corpus are spread
 * over every CU.  f64 indexes take the same first tier as f32 ones (bf16 filter, then f64 re-rank and proof).
 * Scratch: every call works in a pooled per-handle workspace that grows to the largest call seen -- for a filter-tier
 * batch of 10^4 queries ~0.4 GB (candidate buffers + the second tier's worst case), allocated on the first such call
 * (hipMalloc: no device-wide wait); a buffer that has to grow is retired behind the workspace's end-of-use event, never
 * freed inside a call.  Each concurrent host thread (and each shard sharing a GPU) has its own workspace. */
int pn_query_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols,
                 ptrdiff_t q_row_stride, size_t k, uint64_t *idx_out, float *dist_out);
int pn_query_f64(const pn_index *index, const double *queries, size_t nq, size_t q_cols,
                 ptrdiff_t q_row_stride, size_t k, uint64_t *idx_out, double *dist_out);
int pn_query_device_f32(const pn_index *index, const float *d_queries, size_t nq, size_t q_cols,
                        size_t q_row_stride, size_t k, uint64_t *d_idx_out, float *d_dist_out,
                        void *stream);
int pn_query_device_f64(const pn_index *index, const double *d_queries, size_t nq, size_t q_cols,
                        size_t q_row_stride, size_t k, uint64_t *d_idx_out, double *d_dist_out,
                        void *stream);

/* ---- 1-NN: BallTree::query_nearest (src/ball_tree.rs:80-86, 149-196). */
int pn_query_nearest_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols,
                         ptrdiff_t q_row_stride, uint64_t *idx_out, float *dist_out);
int pn_query_nearest_f64(const pn_index *index, const double *queries, size_t nq, size_t q_cols,
                         ptrdiff_t q_row_stride, uint64_t *idx_out, double *dist_out);

/* ---- radius: BallTree::query_radius (src/ball_tree.rs:137-142, 250-294).
 * Returns, per query, { i : distance(q, p_i) < r } (the leaf test at :277 is
 * strict) in ascending index order (the reference's order is unspecified; its
 * tests sort, :667, :777).  CSR output: offsets[nq + 1] is caller-allocated,
 * *idx_out is allocated by the library (release with pn_free). */
int pn_query_radius_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols,
                        ptrdiff_t q_row_stride, float radius, uint64_t *offsets, uint64_t **idx_out);
int pn_query_radius_f64(const pn_index *index, const double *queries, size_t nq, size_t q_cols,
                        ptrdiff_t q_row_stride, double radius, uint64_t *offsets, uint64_t **idx_out);
void pn_free(void *p);
/* The same for queries ALREADY IN HBM (round 4), everything enqueued on `stream`, nothing read back: the caller supplies
 * d_idx and its capacity (entries).  d_offsets [nq + 1] always receives the complete CSR offsets (per-query counts scanned
 * on the device); the rows of query q land at d_idx[d_offsets[q] ...] wherever that position is below `capacity`; and
 * d_total[0] (nullable) = d_offsets[nq].  A total above the capacity means "call again with a larger buffer" -- every
 * offset is right and the first `capacity` entries are in place even then; capacity = 0 (d_idx may be NULL) only counts.
 * Same lists, same order as pn_query_radius_* (strict '<', ascending index).  q_row_stride in elements. */
int pn_query_radius_device_f32(const pn_index *index, const float *d_queries, size_t nq, size_t q_cols,
                               size_t q_row_stride, float radius, uint64_t *d_offsets, uint64_t *d_idx, size_t capacity,
                               uint64_t *d_total, void *stream);
int pn_query_radius_device_f64(const pn_index *index, const double *d_queries, size_t nq, size_t q_cols,
                               size_t q_row_stride, double radius, uint64_t *d_offsets, uint64_t *d_idx, size_t capacity,
                               uint64_t *d_total, void *stream);

/* ---- radius with distances: the lists of pn_query_radius_* (same index sets, same edge cases -- r <= 0, NaN, +inf,
 * Cosine r >= 1 --, index_base, pn_stats.radius_results) and, next to every index, its distance: bit-identical to the
 * reference's metric.distance(q, p) in the index's element type (Euclidean: the sequential unfused fold over
 * min(q_cols, dim) coordinates and a correctly rounded sqrt; Cosine: the three sums and 1 - dot / (|a| |b|)).
 * flags: 0 = each list in ascending index order, as pn_query_radius_*; PN_RADIUS_SORTED = each list nearest-first, by
 * (distance, index) ascending -- the k-NN answers' order, so the first k entries of a list of at least k equal
 * pn_query_*'s answer.  Any other bit: PN_ERR_INVALID.
 * Host entry points: offsets [nq + 1] caller-allocated; *idx_out and *dist_out allocated by the library (pn_free). */
#define PN_RADIUS_SORTED 1
int pn_query_radius_with_distance_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols,
                                      ptrdiff_t q_row_stride, float radius, unsigned flags, uint64_t *offsets,
                                      uint64_t **idx_out, float **dist_out);
int pn_query_radius_with_distance_f64(const pn_index *index, const double *queries, size_t nq, size_t q_cols,
                                      ptrdiff_t q_row_stride, double radius, unsigned flags, uint64_t *offsets,
                                      uint64_t **idx_out, double **dist_out);
/* Device entry points: the contract of pn_query_radius_device_* (complete offsets, entries below `capacity` written,
 * capacity = 0 only counts), d_dist [capacity] next to d_idx; d_dist must not be NULL when capacity > 0.  With
 * PN_RADIUS_SORTED and a total above the capacity, every list that lies wholly below the capacity is complete and
 * sorted; the list that straddles the capacity holds its first entries in ascending index order, unsorted.  A sorted
 * call that may meet a list longer than 2048 entries reserves scratch for min(capacity, nq * n_points) entries in the
 * handle's workspace. */
int pn_query_radius_with_distance_device_f32(const pn_index *index, const float *d_queries, size_t nq, size_t q_cols,
                                             size_t q_row_stride, float radius, unsigned flags, uint64_t *d_offsets,
                                             uint64_t *d_idx, float *d_dist, size_t capacity, uint64_t *d_total,
                                             void *stream);
int pn_query_radius_with_distance_device_f64(const pn_index *index, const double *d_queries, size_t nq, size_t q_cols,
                                             size_t q_row_stride, double radius, unsigned flags, uint64_t *d_offsets,
                                             uint64_t *d_idx, double *d_dist, size_t capacity, uint64_t *d_total,
                                             void *stream);

/* ---- self-queries: every indexed row i against its own index (DBSCAN / OPTICS / HDBSCAN core distances, kNN graphs),
 * the row itself left out.  The queries are the index's own rows in HBM: nothing is copied up, and every tier serves
 * them as it serves ordinary queries of the rows' length.  Rows are answered 2^18 at a time (k-NN and radius alike), so
 * the handle's workspace is sized as for a batch of at most 2^18 queries: a chunk's rows are packed into it like any
 * query batch's (the narrow bf16 tier's k-NN reads them in place), never the whole corpus.  Row i is identified as
 * i + PN_OPT_INDEX_BASE.  Row-sharded handles: pn_sharded_query_self_* below.  pn_stats.queries counts n queries, as a
 * batch of n would.
 *
 * k-NN: row i's answer is the first kout entries of the list of the rows j != i, ordered as pn_query_*'s answers
 * ((distance, index), NaN last), distances bit-identical to metric.distance(p_i, p_j); kout = min(k, n - 1).  Exactly:
 * pn_query_*(rows, k + 1) with, in each row's answer, the entry i + base dropped if present, else the last one -- for
 * every input: duplicated rows, NaN rows, Cosine (where a row's distance to itself need not be 0).
 * flags: PN_SELF_INCLUDE keeps row i in its own list: kout = min(k, n) and the answer equals pn_query_*(rows, k).  Any
 * other bit, PN_RADIUS_SORTED included: PN_ERR_INVALID.  kout = 0 (k = 0, or n = 1 without the flag) writes nothing.
 * Host entry points: idx_out / dist_out [n][kout]; the device holds O(2^18 x (k + 1)) entries of staging beyond the
 * workspace (rows are answered 2^18 at a time).  Device entry points: d_idx / d_dist [n][kout] in HBM, enqueued on
 * `stream` with the ordering contract of pn_query_device_*. */
#define PN_SELF_INCLUDE 2
int pn_query_self_f32(const pn_index *index, size_t k, unsigned flags, uint64_t *idx_out, float *dist_out);
int pn_query_self_f64(const pn_index *index, size_t k, unsigned flags, uint64_t *idx_out, double *dist_out);
int pn_query_self_device_f32(const pn_index *index, size_t k, unsigned flags, uint64_t *d_idx, float *d_dist, void *stream);
int pn_query_self_device_f64(const pn_index *index, size_t k, unsigned flags, uint64_t *d_idx, double *d_dist,
                             void *stream);
/* radius: row i's list is { j != i : distance(p_i, p_j) < r } -- the index sets and edge cases of pn_query_radius_* (r <= 0,
 * NaN, +inf, Cosine r >= 1) -- in ascending index order, or nearest-first by (distance, index) with PN_RADIUS_SORTED;
 * PN_SELF_INCLUDE keeps row i wherever distance(p_i, p_i) < r (the answer is then pn_query_radius_with_distance_*'s for
 * the rows).  Distances are optional (dist_out / d_dist NULL); PN_RADIUS_SORTED needs them.  Unknown flag bits:
 * PN_ERR_INVALID.
 * Host entry points: offsets [n + 1] caller-allocated; *idx_out (and *dist_out) allocated by the library (pn_free).  They
 * run the pipeline twice -- a count, then the lists into staging of the exact total -- and fail with PN_ERR_DEVICE if a
 * row's self flag (its own distance below r, evaluated from the row) ever disagreed with its list.
 * Device entry points: the capacity contract of pn_query_radius_with_distance_device_* -- d_offsets [n + 1] always
 * complete, entries below `capacity` written, capacity = 0 only counts (d_idx / d_dist may then be NULL), d_total[0]
 * (nullable) = d_offsets[n], and its sorted / straddle rule.  Scratch beyond a 2^18-query batch's: one chunk's lists with
 * the rows themselves, capacity + 2^18 entries (at most 2^18 x n), and O(2^18) words, in the handle's workspace.  They
 * read nothing back, so they do not report a flag / list disagreement (the offsets stay well formed); the host entry
 * points do. */
int pn_query_radius_self_f32(const pn_index *index, float radius, unsigned flags, uint64_t *offsets, uint64_t **idx_out,
                             float **dist_out);
int pn_query_radius_self_f64(const pn_index *index, double radius, unsigned flags, uint64_t *offsets, uint64_t **idx_out,
                             double **dist_out);
int pn_query_radius_self_device_f32(const pn_index *index, float radius, unsigned flags, uint64_t *d_offsets,
                                    uint64_t *d_idx, float *d_dist, size_t capacity, uint64_t *d_total, void *stream);
int pn_query_radius_self_device_f64(const pn_index *index, double radius, unsigned flags, uint64_t *d_offsets,
                                    uint64_t *d_idx, double *d_dist, size_t capacity, uint64_t *d_total, void *stream);

/* ---- one radius per query (scikit-learn's BallTree.query_radius(X, r) with an array r): radii [nq] (self-queries:
 * [n], row i's own radius) in the index's element type.  List q is the single list pn_query_radius_with_distance_*
 * returns for query q alone with radius radii[q] and the same flags -- same index set, same order, bit-identical distances
 * (self-queries: pn_query_radius_self_* with radii[i], row i's list) -- so the scalar contract holds PER QUERY: strict '<';
 * a radius <= 0 or NaN gives an empty list and +inf every row whose distance is not NaN; Cosine radii >= 1 are answered
 * by the exact scan; ascending index order, or nearest-first by (distance, index) with PN_RADIUS_SORTED, which needs
 * the distances; PN_SELF_INCLUDE on the self entry points only; unknown flag bits: PN_ERR_INVALID; PN_OPT_INDEX_BASE
 * applies; pn_stats.queries / radius_results advance as the corresponding scalar entry point's do.  Distances are optional
 * (dist_out / d_dist NULL).  radii NULL with nq > 0 (n > 0): PN_ERR_INVALID, like every argument error reported before
 * any device is touched.
 * Which tier answers a query is decided per query ON THE DEVICE: a query whose radius the first tier cannot serve (not
 * finite positive, Cosine r >= 1, r^2 beyond the filter's range) or whose survivor list overflows is listed on the device
 * and answered by the exact scan with its own radius, while the rest of the batch stays in the filter.  The number of
 * listed queries is added (by a kernel, nothing is read back) to the device word pn_index_get_stats folds into
 * pn_stats.fallback_queries -- once per call; the scalar entry points do not report it.  It counts queries listed OUT OF
 * an entered first tier: a call that never enters it (fewer than 4096 rows or 8 columns, queries of another length than
 * the rows, an engine option) answers every query by the exact scan, as the scalar call does, and adds nothing.
 * Device entry points: the capacity contract of pn_query_radius_with_distance_device_* (d_offsets always complete, entries
 * below `capacity` written, capacity = 0 only counts and d_idx / d_dist may then be NULL, d_total (nullable) = the total,
 * the same sorted / straddle rule); d_radii in HBM; nothing is read back, everything is enqueued on `stream`.
 * Host entry points: built on that pipeline, as pn_query_radius_self_* -- queries and radii up, a counting pass, the
 * exact total allocated (pn_free), a fill pass.  The scalar host path's f32 MFMA radius tier and its one-launch path for
 * tiny corpora do not take arrays: the latency of small calls is not a goal of these entry points. */
int pn_query_radii_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
                       const float *radii, unsigned flags, uint64_t *offsets, uint64_t **idx_out, float **dist_out);
int pn_query_radii_f64(const pn_index *index, const double *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
                       const double *radii, unsigned flags, uint64_t *offsets, uint64_t **idx_out, double **dist_out);
int pn_query_radii_device_f32(const pn_index *index, const float *d_queries, size_t nq, size_t q_cols, size_t q_row_stride,
                              const float *d_radii, unsigned flags, uint64_t *d_offsets, uint64_t *d_idx, float *d_dist,
                              size_t capacity, uint64_t *d_total, void *stream);
int pn_query_radii_device_f64(const pn_index *index, const double *d_queries, size_t nq, size_t q_cols,
                              size_t q_row_stride, const double *d_radii, unsigned flags, uint64_t *d_offsets,
                              uint64_t *d_idx, double *d_dist, size_t capacity, uint64_t *d_total, void *stream);
int pn_query_radii_self_f32(const pn_index *index, const float *radii, unsigned flags, uint64_t *offsets,
                            uint64_t **idx_out, float **dist_out);
int pn_query_radii_self_f64(const pn_index *index, const double *radii, unsigned flags, uint64_t *offsets,
                            uint64_t **idx_out, double **dist_out);
int pn_query_radii_self_device_f32(const pn_index *index, const float *d_radii, unsigned flags, uint64_t *d_offsets,
                                   uint64_t *d_idx, float *d_dist, size_t capacity, uint64_t *d_total, void *stream);
int pn_query_radii_self_device_f64(const pn_index *index, const double *d_radii, unsigned flags, uint64_t *d_offsets,
                                   uint64_t *d_idx, double *d_dist, size_t capacity, uint64_t *d_total, void *stream);

/* ---- DBSCAN on the device: cluster labels of the indexed rows without materialising the eps-graph.
 * For a radius eps and min_samples >= 1:
 *   N(i)    = { j : distance(p_i, p_j) < eps }: row i's list from pn_query_radius_self_* with PN_SELF_INCLUDE -- strict '<',
 *             bit-identical distances, row i itself counted iff its own distance is < eps (a NaN row: empty).  eps <= 0 or
 *             NaN: every N(i) is empty by definition, every row is noise.
 *   core[i] = |N(i)| >= min_samples.
 *   Clusters are the connected components of the core rows under "j in N(i)", numbered 0, 1, ... by ascending lowest core
 *   row.  labels[i] = its component's number for a core row; for a non-core row with a core row in N(i) (a border row) the
 *   LOWEST-numbered cluster among its core neighbours; -1 otherwise (noise).
 * This is the labelling of the classic scan-order algorithm (rows visited in index order, each new cluster expanded fully
 * before the next; scikit-learn's, with '<' in place of '<='), and it depends on the data alone, not on scheduling:
 * every union links the larger root under the smaller.
 * labels [n] int64; core [n] bytes of 0 / 1, nullable; n_clusters [1], nullable.  flags must be 0.  Euclidean and Cosine
 * indexes alike; PN_OPT_INDEX_BASE does not affect the labels.  flags != 0, min_samples == 0, NULL labels, a NULL index, a
 * wrong element type: PN_ERR_INVALID, in that order, before any device is touched; more than 2^31 - 1 rows:
 * PN_ERR_UNSUPPORTED (parents are 32-bit).  pn_stats.queries counts n queries.
 * The call runs the radius pipeline twice over the rows -- a count, then the lists piece by piece (at most 2^18 rows and
 * PN_OPT_DBSCAN_PIECE entries each) into workspace scratch, where a union-find kernel consumes them.  Device memory beyond
 * a 2^18-query batch's workspace: 37 bytes per row, 8 bytes per entry of the largest piece, 4 bytes per entry of the
 * non-core rows' lists (fewer than n (min_samples - 1) entries).
 * Device entry points: outputs in HBM, written in stream order on `stream`; the call BLOCKS THE HOST ONCE, after the
 * counting pass, to read the n + 1 offsets it cuts the pieces from -- it is not capturable into a graph.
 * Not yet: row-sharded handles (pn_sharded_*) and one eps per row. */
int pn_dbscan_f32(const pn_index *index, float eps, size_t min_samples, unsigned flags, int64_t *labels, uint8_t *core,
                  uint64_t *n_clusters);
int pn_dbscan_f64(const pn_index *index, double eps, size_t min_samples, unsigned flags, int64_t *labels, uint8_t *core,
                  uint64_t *n_clusters);
int pn_dbscan_device_f32(const pn_index *index, float eps, size_t min_samples, unsigned flags, int64_t *d_labels,
                         uint8_t *d_core, uint64_t *d_n_clusters, void *stream);
int pn_dbscan_device_f64(const pn_index *index, double eps, size_t min_samples, unsigned flags, int64_t *d_labels,
                         uint8_t *d_core, uint64_t *d_n_clusters, void *stream);

/* ---- Minimum spanning tree of the indexed rows under mutual reachability (HDBSCAN; single linkage without cores),
 * exact and on the device.  The graph is complete over the n rows; the edge {i, j}, i < j, weighs
 *     w(i, j) = max(d(i, j), core[i], core[j]),
 * d = the index's metric.distance(p_i, p_j), bit-identical to the reference and symmetric bit for bit, the maximum taken in
 * the library's key order: NaN above +inf, -0 counts as +0 (a weight is written as the value of its key: -0 as +0, any NaN
 * as the canonical quiet NaN); a Cosine index orders all floats, on a Euclidean index a negative core value acts as 0.
 * core: n values of the index's element type, row i's core distance -- for HDBSCAN the distance to its min_samples-th
 * nearest OTHER row, the last column of pn_query_self_*(min_samples) (scikit-learn counts the row itself: its m is this
 * library's m - 1).  core == NULL: no cores, w = d -- the Euclidean / Cosine MST, i.e. single linkage (on a Euclidean index
 * the same as all zeros).
 * Edges are totally ordered by (key(w), i, j), and the answer is THE minimum spanning tree under that strict order: n - 1
 * edges with src < dst (PN_OPT_INDEX_BASE added to both ends), written ascending in that order -- the merge order of a
 * single-linkage dendrogram.  Because the order is strict the result depends on the data alone, not on scheduling, the
 * engine or PN_OPT_MST_BATCH.  Rows with NaN coordinates are vertices like any other: their edges weigh NaN and come last.
 * n = 1 writes nothing and succeeds.
 * flags must be 0.  Argument errors, before any device is touched and in this order: flags != 0, a NULL output with n > 1,
 * NULL index, wrong element type: PN_ERR_INVALID; more than 2^31 - 1 rows: PN_ERR_UNSUPPORTED.  pn_stats.queries counts n.
 * work_out (nullable, a HOST pointer in both variants) receives {rounds, rows scanned}: the Boruvka rounds run, and the rows
 * handed to a scan summed over the rounds (a round answered by the k-NN pipeline counts n).  Without cores round 0 is
 * pn_query_self_device_*(k = 1) on the handle's engine; every other round is an exact masked scan of the rows whose cached
 * candidate has joined their own component.  Device memory beyond a 2^18-query batch's workspace: about
 * 100 bytes per row (f64: 130).
 * Device entry points: d_core (nullable) and the outputs in HBM, written in stream order on `stream`; the call BLOCKS THE
 * HOST ONCE PER ROUND, to read the number of components left and the length of the list of rows to scan -- like
 * pn_dbscan_device_* it is not capturable into a graph.
 * Not in this version: row-sharded handles (pn_sharded_*), and a first-tier (bf16) filter for the masked scans. */
int pn_mst_f32(const pn_index *index, const float *core, unsigned flags, uint64_t *src_out, uint64_t *dst_out,
               float *weight_out, uint64_t *work_out);
int pn_mst_f64(const pn_index *index, const double *core, unsigned flags, uint64_t *src_out, uint64_t *dst_out,
               double *weight_out, uint64_t *work_out);
int pn_mst_device_f32(const pn_index *index, const float *d_core, unsigned flags, uint64_t *d_src, uint64_t *d_dst,
                      float *d_weight, uint64_t *work_out, void *stream);
int pn_mst_device_f64(const pn_index *index, const double *d_core, unsigned flags, uint64_t *d_src, uint64_t *d_dst,
                      double *d_weight, uint64_t *work_out, void *stream);

/* ---- Single-linkage dendrogram of a spanning tree's sorted edges, on the device.
 * Input: the n - 1 edges of a spanning tree over the rows 0 .. n - 1 in the format pn_mst_* writes -- PN_OPT_INDEX_BASE
 * added to both ends, in merge order (pn_mst_* writes them ascending); the handle supplies n, the device and the workspace.
 * Output: SciPy's linkage layout as four arrays of length n - 1.  The r-th edge makes node n + r with the children
 * left[r] and right[r]: node ids, < n a row (no index base), >= n an earlier merge; left is the subtree that holds
 * src[r], right the one that holds dst[r]; weight_out[r] = weight[r] (it may be the same array); size[r] = the rows
 * under the node.  The result is a function of the edges alone: it is the tree a sequential union-find over the edges in
 * the given order builds, whatever the schedule.  The work is log2(n) levels of O(n) each and no step walks the tree, so
 * the time does not grow with the dendrogram's height.  n <= 1 writes nothing and succeeds.
 * Edges that do not form a spanning tree (an end that is no row, a repeated edge, a cycle: the last node does not hold
 * n rows): PN_ERR_INVALID after the device work, the outputs unspecified.  The host variant reads that one word back;
 * the device variant writes PN_OK or PN_ERR_INVALID to d_error[0] (an int32 in HBM, nullable) in stream order, returns
 * PN_OK and never waits for the device.
 * flags must be 0.  Argument errors, before any device is touched and in this order: flags != 0, a NULL array with n > 1
 * (src, dst, weight, left, right, weight_out, size), NULL index, wrong element type: PN_ERR_INVALID; more than 2^31 - 1
 * rows: PN_ERR_UNSUPPORTED.  Device memory: 48 bytes per row. */
int pn_linkage_f32(const pn_index *index, const uint64_t *src, const uint64_t *dst, const float *weight, unsigned flags,
                   uint64_t *left_out, uint64_t *right_out, float *weight_out, uint64_t *size_out);
int pn_linkage_f64(const pn_index *index, const uint64_t *src, const uint64_t *dst, const double *weight, unsigned flags,
                   uint64_t *left_out, uint64_t *right_out, double *weight_out, uint64_t *size_out);
int pn_linkage_device_f32(const pn_index *index, const uint64_t *d_src, const uint64_t *d_dst, const float *d_weight,
                          unsigned flags, uint64_t *d_left, uint64_t *d_right, float *d_weight_out, uint64_t *d_size,
                          int32_t *d_error, void *stream);
int pn_linkage_device_f64(const pn_index *index, const uint64_t *d_src, const uint64_t *d_dst, const double *d_weight,
                          unsigned flags, uint64_t *d_left, uint64_t *d_right, double *d_weight_out, uint64_t *d_size,
                          int32_t *d_error, void *stream);

/* ---- HDBSCAN labels of the indexed rows, on the device: pn_query_self_device_*(min_samples)'s last column (the core
 * distances) -> pn_mst_device_* -> the dendrogram above -> condensed tree, stability, excess-of-mass selection, labels and
 * membership probabilities.  Nothing leaves HBM but the outputs.
 * labels: n int64, 0 .. n_clusters - 1 or -1 (noise); probabilities (nullable): n values of the index's element type;
 * n_clusters (nullable): one word.  min_samples counts OTHER rows (scikit-learn counts the row itself: its min_samples is
 * this library's + 1); m = min_cluster_size.  The contract, all arithmetic in f64:
 *   lambda(w) of a merge weight w: 1 / w for w > 2^-100; 2^100 for w <= 2^-100 (duplicate rows, Cosine's non-positive
 *     weights: finite, so no inf - inf); 0 for a NaN weight.  lambda(node) = lambda(the node's weight).
 *   A dendrogram node is a TRUE SPLIT when both children hold at least m rows.  The condensed clusters are the root and
 *     both children of every true split; ctop(x), for a node of at least m rows, is its nearest ancestor-or-self that is
 *     such a cluster top.
 *   Row p FALLS OUT at a(p), its lowest ancestor with at least m rows: out of the cluster ctop(a(p)), with
 *     lambda_p = lambda(a(p)).
 *   birth(c) = lambda(parent(top of c)), 0 for the root.
 *     stability(c) = sum over the rows p that fall out of c of (lambda_p - birth(c))
 *                    + size(s) * (lambda(s) - birth(c)), s = the true split that ends c, if there is one.
 *     death(c) = the largest of those lambda.
 *   Selection (excess of mass), bottom-up: a non-root cluster is FLAGGED unless the sum of its children's best values is
 *     strictly greater than its stability; best = the stability if flagged, else that sum.  The root is never flagged
 *     (no allow_single_cluster in this version).  SELECTED are the flagged clusters without a flagged ancestor.
 *   labels[p] = the selected ancestor-or-self of the cluster p falls out of, else -1; the selected clusters are numbered
 *     by ascending lowest member row, like pn_dbscan_*.  probabilities[p] = min(lambda_p, death) / death with the
 *     selected cluster's death, 1 where death == 0, 0 for noise.
 *   n < m, or no true split: all noise, 0 clusters.  Rows with NaN coordinates end as noise.
 * This is scikit-learn's tree_to_labels(..., "eom", allow_single_cluster=False) up to the numbering.  The result depends
 * on the data alone: the tree is unique (pn_mst_*), the dendrogram a function of it, the stability sums have a shape
 * fixed by the tree (no floating-point atomics) and everything else is integer or a maximum.
 * flags must be 0.  Argument errors, before any device is touched and in this order: flags != 0, NULL labels, NULL index,
 * wrong element type, min_cluster_size < 2, min_samples outside [1, n - 1] when n >= 2: PN_ERR_INVALID; more than
 * 2^31 - 1 rows: PN_ERR_UNSUPPORTED.  Device memory beyond pn_mst_*'s: about 190 bytes per row (f64: 200).
 * Device entry points: the outputs in HBM, written in stream order on `stream`; the call keeps the host waits of
 * pn_mst_device_* (one per Boruvka round) and adds none: the dendrogram and the extraction are enqueued and left.
 * Not in this version: row-sharded handles, allow_single_cluster, leaf selection, a cluster_selection_epsilon. */
int pn_hdbscan_f32(const pn_index *index, size_t min_samples, size_t min_cluster_size, unsigned flags, int64_t *labels,
                   float *probabilities, uint64_t *n_clusters);
int pn_hdbscan_f64(const pn_index *index, size_t min_samples, size_t min_cluster_size, unsigned flags, int64_t *labels,
                   double *probabilities, uint64_t *n_clusters);
int pn_hdbscan_device_f32(const pn_index *index, size_t min_samples, size_t min_cluster_size, unsigned flags,
                          int64_t *d_labels, float *d_probabilities, uint64_t *d_n_clusters, void *stream);
int pn_hdbscan_device_f64(const pn_index *index, size_t min_samples, size_t min_cluster_size, unsigned flags,
                          int64_t *d_labels, double *d_probabilities, uint64_t *d_n_clusters, void *stream);

/* ---- Local Outlier Factor of the indexed rows, on the device (scikit-learn's neighbors.LocalOutlierFactor with
 * n_neighbors = k): the k self-query -> the graph packed in HBM -> one gather pass for the local reachability densities
 * and one for the scores.  Nothing leaves HBM but the outputs.
 * lof: n doubles, required; lrd (nullable): n doubles; kdist (nullable): n values of the index's element type.  lrd and
 * kdist are what pn_lof_score_* takes back: the library keeps no fit in the handle.  The contract, all arithmetic in IEEE
 * f64, unfused, no special cases:
 *   For row i let (j_0 .. j_{k-1}, d_0 .. d_{k-1}) be its answer from pn_query_self_*(k) with flags 0: the k nearest OTHER
 *     rows ordered by (distance, index), NaN last, the distances bit-identical to the reference metric.
 *   kdist[i] = d_{k-1}, in the index's element type: the bits of the last column of pn_query_self_*.
 *   v_t = NaN if d_t or kdist[j_t] is NaN, else max((double)d_t, (double)kdist[j_t], +0.0).  The clamp at 0 matters only for
 *     a Cosine index, where a distance can be a few ulp below 0; the NaN rule is np.maximum's, not fmax's.
 *   S_i = (...((0.0 + v_0) + v_1) ... + v_{k-1}): added one by one in list order.
 *   lrd[i] = 1.0 / (S_i / (double)k + 1e-10): scikit-learn's formula with its 1e-10, so duplicate rows give lrd = 1e10,
 *     never inf.
 *   lof[i] = (...((0.0 + lrd[j_0] / lrd[i]) + lrd[j_1] / lrd[i]) ... ) / (double)k: each ratio divided first, added in list
 *     order.
 *   Score of a query q (pn_lof_score_*): (j_t, d_t) = q's answer from pn_query_*(q, k) -- the query is excluded from
 *     nothing -- v_t as above from d_t and kdist[j_t], lrd_q = 1.0 / (S / k + 1e-10), score = (sum_t lrd[j_t] / lrd_q) / k
 *     in the same order.  lrd and kdist are those of pn_lof_* with the same k.  A fitted row scored as a query finds itself
 *     at distance 0 and so does not reproduce its fit score; scikit-learn's score_samples behaves the same way.
 * lof = -negative_outlier_factor_ of LocalOutlierFactor(n_neighbors = k), up to this library's distance arithmetic and tie
 * order.  The result depends on the data alone: the k-NN answer is unique and fixes the order of every sum; there are no
 * floating-point atomics and no reduction whose shape depends on the launch.
 * A row with a NaN coordinate scores NaN, and so does every row with such a row in its list.  Euclidean and Cosine
 * indexes, f32 and f64.  PN_OPT_INDEX_BASE affects no output (neighbour ids are used without the base).
 * pn_stats.queries advances by n for a fit and by nq for a scoring call.
 * flags must be 0.  Argument errors, before any device is touched and in this order: flags != 0; NULL lof / score_out
 * (scoring with nq > 0: also NULL queries, lrd or kdist); NULL index; wrong element type; k outside [1, n - 1] (an index
 * of fewer than 2 rows is always an error): PN_ERR_INVALID; more than 2^31 - 1 rows: PN_ERR_UNSUPPORTED (stored
 * neighbour ids are 32-bit).  nq = 0 writes nothing and succeeds.
 * Device entry points: the outputs (and lrd, kdist, the queries of a scoring call) in HBM, everything enqueued on
 * `stream`; the call never waits for the device, as the self-query it builds on does not.
 * Device memory of a fit, beyond a 2^18-query batch's workspace: n * k * (4 + sizeof T) + n * (8 + sizeof T) bytes -- the
 * whole graph as 32-bit ids and distances, plus lrd and kdist where the caller supplied no buffer.  Scoring: a 2^18-query
 * batch's workspace and its k-NN answer.
 * Not in this version: row-sharded handles. */
int pn_lof_f32(const pn_index *index, size_t k, unsigned flags, double *lof, double *lrd, float *kdist);
int pn_lof_f64(const pn_index *index, size_t k, unsigned flags, double *lof, double *lrd, double *kdist);
int pn_lof_device_f32(const pn_index *index, size_t k, unsigned flags, double *d_lof, double *d_lrd, float *d_kdist,
                      void *stream);
int pn_lof_device_f64(const pn_index *index, size_t k, unsigned flags, double *d_lof, double *d_lrd, double *d_kdist,
                      void *stream);
int pn_lof_score_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
                     size_t k, const double *lrd, const float *kdist, unsigned flags, double *score_out);
int pn_lof_score_f64(const pn_index *index, const double *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
                     size_t k, const double *lrd, const double *kdist, unsigned flags, double *score_out);
int pn_lof_score_device_f32(const pn_index *index, const float *d_queries, size_t nq, size_t q_cols, size_t q_row_stride,
                            size_t k, const double *d_lrd, const float *d_kdist, unsigned flags, double *d_score,
                            void *stream);
int pn_lof_score_device_f64(const pn_index *index, const double *d_queries, size_t nq, size_t q_cols, size_t q_row_stride,
                            size_t k, const double *d_lrd, const double *d_kdist, unsigned flags, double *d_score,
                            void *stream);

/* ---- k-NN classification and regression on the device (scikit-learn's neighbors.KNeighborsClassifier and
 * KNeighborsRegressor with n_neighbors = k, and their leave-one-out forms): the k-NN query -> one vote or one weighted
 * mean per list, in HBM.  Neither the [nq][k] lists nor the labels leave the device; nothing leaves HBM but the outputs.
 * The list of a query is (j_0 .. j_{k-1}, d_0 .. d_{k-1}): for new points (pn_knn_classify_*, pn_knn_regress_*) its answer
 * from pn_query_*(q, k); for the _self entries row i's answer from pn_query_self_*(k) with flags 0, where k counts OTHER
 * rows and the row itself is left out (leave-one-out).  The list is ordered by (distance, index), NaN last; ids are taken
 * without the index base (PN_OPT_INDEX_BASE affects no output).  The contract, all arithmetic in IEEE f64, unfused; every
 * sum is the sequential fold in list order, starting from 0.0:
 *   Poison rule: if any d_t is NaN -- or, classifying, any gathered label labels[j_t] is outside [0, n_classes) -- the list
 *     is answered with pred = `-1`, a proba row of NaN and a regression row of NaN, under both weightings.
 *   Clamp: v_t = d_t > 0 ? (double)d_t : +0.0.  A Cosine distance a few ulp below 0 counts as 0, as in pn_lof_*.
 *   Weights: flags = 0 (uniform): w_t = 1.0.  flags = PN_KNN_WEIGHT_DISTANCE: if some v_t == 0 then
 *     w_t = (v_t == 0) ? 1.0 : 0.0, otherwise w_t = 1.0 / v_t -- scikit-learn's _get_weights rule: a list that holds a
 *     zero distance counts its zero-distance entries alone.  An infinite distance weighs 0.
 *   Normaliser: S = (...((0.0 + w_0) + w_1) ... + w_{k-1}); under uniform weights this is exactly k.
 *   Classification: labels is int64 [n], class codes in [0, n_classes).  W_c = 0.0 + the w_t of the entries with
 *     labels[j_t] == c, added in list order.  pred = the c with the largest W_c; ties go to the smallest c
 *     (scikit-learn's weighted_mode / argmax behaviour).  The prediction is taken on the unnormalised W_c, so it never
 *     depends on the division.  proba[q][c] = W_c / S, 0.0 for a class that is not in the list: a dense double
 *     [nq][n_classes] output, optional -- NULL: neither computed nor written.
 *     Where this differs from scikit-learn's predict_proba: their normaliser sums the class row W_0 .. W_{C-1} with NumPy's
 *     pairwise shape, ours is the list-order S; the difference is a few ulp (none under uniform weights, where both are k).
 *   Regression: targets is double [n][n_out], contiguous, n_out >= 1.  out[q][o] = N_o / S with
 *     N_o = (...((0.0 + w_0 * y[j_0][o]) + w_1 * y[j_1][o]) ... ): each product rounded before its addition.  Inf or NaN in
 *     a target propagates by IEEE rules; with the zero-distance rule 0 * inf is NaN, as in scikit-learn.
 * The result depends on the data alone: the k-NN answer is unique and fixes the order of every sum; the winner is found by
 * comparisons on (W_c descending, c ascending), which no order of evaluation changes; there are no floating-point atomics
 * and no reduction whose shape depends on the launch.
 * Limits: new points 1 <= k <= n; _self entries 1 <= k <= n - 1 and n >= 2; k > 1024: PN_ERR_UNSUPPORTED for both
 * families (the class sums compare every list entry with every other); 1 <= n_classes <= 2^31 - 1; more than 2^31 - 1 rows:
 * PN_ERR_UNSUPPORTED, as pn_lof_*.  Euclidean and Cosine indexes, f32 and f64.
 * Labels: the host entries scan labels before touching the device and return PN_ERR_INVALID naming the first offending
 * position and value.  The device entries cannot scan without waiting: they rely on the poison rule, and a label out of
 * range never causes an out-of-bounds store.
 * Argument errors, before any device is touched and in this order, the same in the host and device entries: unknown flags;
 * NULL pred_out (classification) / out (regression); with nq > 0 (the _self entries: always) the first NULL input, named
 * (queries, then labels or targets); NULL index; wrong element type; n_classes / n_out out of range; k out of range: all
 * PN_ERR_INVALID; k > 1024, then too many rows: PN_ERR_UNSUPPORTED; the host entries' label scan.  nq = 0 writes nothing and
 * returns PN_OK after the checks.
 * pn_stats.queries advances by nq for new points and by n for the _self entries.
 * Host entry points: strides as pn_lof_score_*; they wait once, for their final copy.  Device entry points: queries, labels
 * or targets and the outputs in HBM (d_pred int64 [nq], d_proba double [nq][n_classes] or NULL, d_out double [nq][n_out]),
 * everything enqueued on `stream`; the call never waits for the device.
 * Device memory beyond a 2^18-query batch's workspace and its k-NN answer: the host entries' labels or targets and outputs.
 * Not in this version: row-sharded handles, radius-neighbour voting, callable weights, multi-label classification. */
#define PN_KNN_WEIGHT_DISTANCE 1u /* flags of pn_knn_classify_* / pn_knn_regress_*: weigh each neighbour by 1 / distance */
int pn_knn_classify_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
                        size_t k, const int64_t *labels, size_t n_classes, unsigned flags, int64_t *pred_out,
                        double *proba_out);
int pn_knn_classify_f64(const pn_index *index, const double *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
                        size_t k, const int64_t *labels, size_t n_classes, unsigned flags, int64_t *pred_out,
                        double *proba_out);
int pn_knn_classify_device_f32(const pn_index *index, const float *d_queries, size_t nq, size_t q_cols,
                               size_t q_row_stride, size_t k, const int64_t *d_labels, size_t n_classes, unsigned flags,
                               int64_t *d_pred, double *d_proba, void *stream);
int pn_knn_classify_device_f64(const pn_index *index, const double *d_queries, size_t nq, size_t q_cols,
                               size_t q_row_stride, size_t k, const int64_t *d_labels, size_t n_classes, unsigned flags,
                               int64_t *d_pred, double *d_proba, void *stream);
int pn_knn_classify_self_f32(const pn_index *index, size_t k, const int64_t *labels, size_t n_classes, unsigned flags,
                             int64_t *pred_out, double *proba_out);
int pn_knn_classify_self_f64(const pn_index *index, size_t k, const int64_t *labels, size_t n_classes, unsigned flags,
                             int64_t *pred_out, double *proba_out);
int pn_knn_classify_self_device_f32(const pn_index *index, size_t k, const int64_t *d_labels, size_t n_classes,
                                    unsigned flags, int64_t *d_pred, double *d_proba, void *stream);
int pn_knn_classify_self_device_f64(const pn_index *index, size_t k, const int64_t *d_labels, size_t n_classes,
                                    unsigned flags, int64_t *d_pred, double *d_proba, void *stream);
int pn_knn_regress_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
                       size_t k, const double *targets, size_t n_out, unsigned flags, double *out);
int pn_knn_regress_f64(const pn_index *index, const double *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
                       size_t k, const double *targets, size_t n_out, unsigned flags, double *out);
int pn_knn_regress_device_f32(const pn_index *index, const float *d_queries, size_t nq, size_t q_cols, size_t q_row_stride,
                              size_t k, const double *d_targets, size_t n_out, unsigned flags, double *d_out,
                              void *stream);
int pn_knn_regress_device_f64(const pn_index *index, const double *d_queries, size_t nq, size_t q_cols, size_t q_row_stride,
                              size_t k, const double *d_targets, size_t n_out, unsigned flags, double *d_out,
                              void *stream);
int pn_knn_regress_self_f32(const pn_index *index, size_t k, const double *targets, size_t n_out, unsigned flags,
                            double *out);
int pn_knn_regress_self_f64(const pn_index *index, size_t k, const double *targets, size_t n_out, unsigned flags,
                            double *out);
int pn_knn_regress_self_device_f32(const pn_index *index, size_t k, const double *d_targets, size_t n_out, unsigned flags,
                                   double *d_out, void *stream);
int pn_knn_regress_self_device_f64(const pn_index *index, size_t k, const double *d_targets, size_t n_out, unsigned flags,
                                   double *d_out, void *stream);

/* ---- OPTICS on the device (scikit-learn's cluster.OPTICS with metric = this index's, min_samples = this library's + 1):
 * the ordering, the reachability plot, predecessors and core distances of the indexed rows, and the DBSCAN labelling at
 * any eps <= max_eps read off that ordering.  The min_samples self-query gives the core distances, the max_eps radius
 * self-query the graph, which is kept whole in HBM; nothing leaves HBM but the outputs.
 * min_samples >= 1 counts OTHER rows, as pn_hdbscan_* and pn_lof_* do; max_eps is in the index's element type.  The
 * contract:
 *   core[i]  = the last column of pn_query_self_*(min_samples), flags 0, if that value is < max_eps -- strict '<', like
 *              every radius in this library; a NaN value is not < max_eps -- else +inf (undefined).
 *   N(i)     = { j != i : distance(p_i, p_j) < max_eps } with the distances of pn_query_radius_self_*(max_eps), flags 0:
 *              bit-identical to the metric.  max_eps <= 0 or NaN: empty lists everywhere; +inf: every row whose distance
 *              is not NaN.
 *   Start:     reach[i] = +inf, pred[i] = -1, nothing processed.
 *   n times:   p = the unprocessed row with the smallest (reach, row): reach compared by IEEE '<', ties broken by the
 *              lower row.  p is appended to the ordering and marked processed.  If core[p] is finite, then for every
 *              unprocessed q in N(p): new = d(p, q) > core[p] ? d(p, q) : core[p]; if new < reach[q] (strict):
 *              reach[q] = new, pred[q] = p.
 * ordering [n] uint64: row numbers WITHOUT PN_OPT_INDEX_BASE (they index the other three arrays); reachability [n] of
 * the element type, indexed by row, +inf for a row picked with nothing reaching it; predecessor [n] int64, -1 for such a
 * row, nullable; core_distances [n] of the element type, nullable.  ordering and reachability are required.
 * This is scikit-learn's algorithm on THIS library's distances: ordering_ and predecessor_ equal those of
 * OPTICS(min_samples + 1, max_eps, metric = "precomputed") fed with this library's distance matrix, up to this library's
 * distance arithmetic -- scikit-learn's own pairwise distances differ in the last bits and break the frequent exact ties
 * reach = core[p] differently.  The result depends on the data alone: nothing in it depends on scheduling, the engine
 * or PN_OPT_OPTICS_PIECE.  A row with a NaN coordinate has an empty list and an undefined core and appears in no list:
 * it comes out as an isolated +inf entry.  Euclidean and Cosine indexes, f32 and f64.  n = 1: ordering = {0}, reach and
 * core +inf, pred -1.  pn_stats.queries advances by n.
 * flags must be 0.  Argument errors, before any device is touched and in this order: flags != 0; NULL ordering or
 * reachability; NULL index; wrong element type; min_samples outside [1, n - 1] when n >= 2: PN_ERR_INVALID; more than
 * 2^31 - 1 rows: PN_ERR_UNSUPPORTED (stored neighbour ids are 32-bit).
 * The call: the self-query chunk by chunk for the cores; a counting pass of the per-row-radius pipeline (radius max_eps
 * for the rows with a defined core, 0 for the others: only core rows ever relax anything, so the others cost no entries);
 * a fill piece by piece (at most 2^18 rows and PN_OPT_OPTICS_PIECE entries each), every piece repacked into the graph
 * store; then ONE launch of ONE workgroup that runs the n dependent steps over a 64-ary tournament tree of packed
 * (reach, row) keys -- no launch per step, no host round trip, no waiting between workgroups.
 * Device memory beyond a 2^18-query batch's workspace, with E = the number of stored list entries:
 * E * (4 + sizeof T) + 8 (n + 1) bytes for the graph (32-bit ids, distances, offsets), (8 + sizeof T) bytes per entry of the
 * largest piece while it is filled, and about 4.1 * sizeof T bytes per row (radii, cores, and the tree's 1.016 n keys of
 * 2 * sizeof T bytes).  A graph that does not fit: PN_ERR_NOMEM, pn_last_error() names the bytes the graph store needs.
 * Device entry points: outputs in HBM, written in stream order on `stream`; the call BLOCKS THE HOST ONCE, after the
 * counting pass, to read the n + 1 offsets it cuts the pieces from -- like pn_dbscan_device_* it is not capturable into a
 * graph.
 *
 * pn_optics_dbscan_*: the labels DBSCAN(eps, min_samples) gives, read off an ordering (scikit-learn's
 * cluster_optics_dbscan with '<' in place of '<='); eps <= the max_eps of the ordering.  The handle supplies n, the
 * device and the workspace; ordering, reachability and core_distances are pn_optics_*'s outputs.
 *   far[i]  = !(reach[i] < eps);  near[i] = core[i] < eps.
 *   labels[ordering[t]] = (the number of s <= t with far && near at ordering[s]) - 1; then labels[i] = -1 wherever
 *   far[i] && !near[i].
 * Clusters are numbered by first appearance in the ordering -- this is NOT pn_dbscan_*'s "lowest member row" numbering;
 * the partition of the rows with core < eps is the same, border rows may be assigned differently.  labels [n] int64;
 * n_clusters [1] nullable.  On the device: a flag pass, one prefix sum over the ordering, a scatter; nothing waits.
 * An ordering that is not a permutation of 0 .. n - 1: PN_ERR_INVALID after the device work, the labels unspecified.
 * The host variant reads that one word back; the device variant writes PN_OK or PN_ERR_INVALID to d_error[0] (an int32
 * in HBM, nullable) in stream order, returns PN_OK and never waits for the device.
 * flags must be 0.  Argument errors, before any device is touched and in this order: flags != 0; NULL labels; NULL
 * ordering, reachability or core_distances; NULL index; wrong element type: PN_ERR_INVALID; more than 2^31 - 1 rows:
 * PN_ERR_UNSUPPORTED.  Device memory: 16 bytes per row.
 * Not in this version: row-sharded handles, xi extraction. */
int pn_optics_f32(const pn_index *index, size_t min_samples, float max_eps, unsigned flags, uint64_t *ordering,
                  float *reachability, int64_t *predecessor, float *core_distances);
int pn_optics_f64(const pn_index *index, size_t min_samples, double max_eps, unsigned flags, uint64_t *ordering,
                  double *reachability, int64_t *predecessor, double *core_distances);
int pn_optics_device_f32(const pn_index *index, size_t min_samples, float max_eps, unsigned flags, uint64_t *d_ordering,
                         float *d_reachability, int64_t *d_predecessor, float *d_core_distances, void *stream);
int pn_optics_device_f64(const pn_index *index, size_t min_samples, double max_eps, unsigned flags, uint64_t *d_ordering,
                         double *d_reachability, int64_t *d_predecessor, double *d_core_distances, void *stream);
int pn_optics_dbscan_f32(const pn_index *index, const uint64_t *ordering, const float *reachability,
                         const float *core_distances, float eps, unsigned flags, int64_t *labels, uint64_t *n_clusters);
int pn_optics_dbscan_f64(const pn_index *index, const uint64_t *ordering, const double *reachability,
                         const double *core_distances, double eps, unsigned flags, int64_t *labels, uint64_t *n_clusters);
int pn_optics_dbscan_device_f32(const pn_index *index, const uint64_t *d_ordering, const float *d_reachability,
                                const float *d_core_distances, float eps, unsigned flags, int64_t *d_labels,
                                uint64_t *d_n_clusters, int32_t *d_error, void *stream);
int pn_optics_dbscan_device_f64(const pn_index *index, const uint64_t *d_ordering, const double *d_reachability,
                                const double *d_core_distances, double eps, unsigned flags, int64_t *d_labels,
                                uint64_t *d_n_clusters, int32_t *d_error, void *stream);

/* ---- Kernel density sums on the device (the engine of scikit-learn's neighbors.KernelDensity and of
 * BallTree.kernel_density; with count alone: query_radius(count_only = True)): per query the raw, unnormalised sum of
 * the kernel over the rows within a cutoff, the number of such rows, and the cutoff.  The cutoff kernel -> a counting
 * pass of the per-query-radius pipeline -> the lists with distances piece by piece into workspace scratch -> one wave
 * per query sums its list.  Nothing leaves HBM but the outputs; normalisation and logarithms are the callers'.
 * h: the bandwidths, in the index's element type T; n_h = 1 (one for all queries) or the number of queries / rows (one
 * each: the balloon estimator).  kernel: PN_KDE_*.  atol: a double, finite and >= 0, the absolute error the two smooth
 * kernels may trade for a finite cutoff; the three compact kernels ignore it.  The contract:
 *   Cutoff c_q (T) of query q with bandwidth h_q:
 *     tophat, epanechnikov, linear: c_q = h_q.
 *     gaussian, exponential: with n = the number of indexed rows, on the host in f64
 *       L = log((double)n / atol);  f = (gaussian ? sqrt(2.0 * L) : L) * (1.0 + 2^-30)       (libm log, IEEE sqrt)
 *     and per query x = (double)h_q * f (one f64 product), c_q = (T)x rounded to nearest, then the next T towards +inf
 *     if (double)c_q < x: the smallest T >= x.  So c_q >= h_q sqrt(2 ln(n / atol)) resp. h_q ln(n / atol), and exceeds
 *     it by less than a factor (1 + 2^-30)(1 + 2^-23) (f32; f64: (1 + 2^-30)(1 + 2^-52)); the safety factor 2^-30 covers the
 *     rounding of log, sqrt and the product.
 *     atol >= n: c_q = 0, the list is empty.  atol == 0: c_q = +inf, every row with a non-NaN distance is a term.
 *     A bandwidth in an array that is not positive, or NaN, is its own cutoff: such a radius gives an empty list.
 *   List L_q = what pn_query_radii_with_distance_* returns for q with radius c_q and flags 0: the rows with
 *     distance < c_q (strict), in ascending row index, the distances bit-identical to the reference metric; a row whose
 *     distance is NaN is in no list.  Self entries: the list of pn_query_radii_self_* with the same flags -- by default the
 *     row itself is left out (the leave-one-out density), PN_SELF_INCLUDE keeps it.
 *   Terms, in IEEE f64, unfused, operations in the order written, d = max((double)dist, +0.0) (the clamp pn_lof_* uses: a
 *     Cosine distance can be a few ulp below 0) and h = (double)h_q:
 *       tophat 1.0;  epanechnikov 1.0 - (d*d) / (h*h);  linear 1.0 - d / h;
 *       gaussian exp(-((d*d) / (2.0 * (h*h))));  exponential exp(-(d / h))     (exp: the device library's f64 exp)
 *   Sum, fixed shape: with the terms t_0 .. t_{m-1} in list order,
 *       lane partial P_l = (...((0.0 + t_l) + t_{l+64}) + t_{l+128} ...) for l = 0 .. 63 (missing positions add nothing),
 *       S = (...((P_0 + P_1) + P_2) ... + P_63).
 *     The shape depends on m alone: one wave per query, no floating-point atomics, no reduction whose shape depends on
 *     the launch -- the result depends on the data alone, not on the engine, PN_OPT_KDE_PIECE or scheduling.
 *   Guarantee: with S_all the same sum over every row (the atol = 0 result), S_all - atol <= S <= S_all up to the rounding
 *     of the sums: a row left out has d >= c_q, so its term is at most atol / n.
 * Outputs, per query: sum (f64; nullable only if count is given -- then only the counting pass runs and no list is ever
 * written), count (uint64, nullable: m), cutoff (T, nullable: c_q).
 * Euclidean and Cosine indexes, f32 and f64.  PN_OPT_INDEX_BASE affects no output.  A query with a NaN coordinate has an
 * empty list: sum 0, count 0.  pn_stats.queries advances by nq (n for the self entries).
 * flags: 0 for the query entries; PN_SELF_INCLUDE or 0 for the self entries.  Argument errors, before any device is
 * touched and in this order: unknown flags; unknown kernel; atol negative, NaN or infinite; sum and count both NULL;
 * with nq > 0 NULL queries (q_cols > 0) or NULL h (self entries: NULL h); n_h neither 1 nor nq; NULL index; wrong element
 * type: PN_ERR_INVALID; more than 2^31 - 1 rows or queries: PN_ERR_UNSUPPORTED.  The self entries compare n_h with n
 * after the handle's checks.  Host entries with n_h = 1: a bandwidth that is not finite and positive is PN_ERR_INVALID,
 * checked last.  nq = 0 writes nothing and succeeds.
 * Device entry points: queries, h and the outputs in HBM, written in stream order on `stream`; with a sum the call BLOCKS
 * THE HOST ONCE, after the counting pass, to read the nq + 1 offsets it cuts the pieces from -- like pn_dbscan_device_* it
 * is not capturable into a graph.  Without a sum nothing waits.
 * Device memory beyond a 2^18-query batch's workspace: 16 + 2 sizeof T bytes per query, and 8 + sizeof T bytes per entry
 * of the largest piece (at most 2^18 queries and PN_OPT_KDE_PIECE entries; a longer single list is a piece of its own).
 * Known slow case: with atol = 0 the two smooth kernels list every row for every query; all queries then go through the
 * exact scan and n entries each are written and read back -- the price of an exact infinite-support sum.
 * Not in this version: row-sharded handles, scikit-learn's `cosine` kernel, rtol. */
int pn_kde_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
               const float *h, size_t n_h, int kernel, double atol, unsigned flags, double *sum_out, uint64_t *count_out,
               float *cutoff_out);
int pn_kde_f64(const pn_index *index, const double *queries, size_t nq, size_t q_cols, ptrdiff_t q_row_stride,
               const double *h, size_t n_h, int kernel, double atol, unsigned flags, double *sum_out, uint64_t *count_out,
               double *cutoff_out);
int pn_kde_device_f32(const pn_index *index, const float *d_queries, size_t nq, size_t q_cols, size_t q_row_stride,
                      const float *d_h, size_t n_h, int kernel, double atol, unsigned flags, double *d_sum,
                      uint64_t *d_count, float *d_cutoff, void *stream);
int pn_kde_device_f64(const pn_index *index, const double *d_queries, size_t nq, size_t q_cols, size_t q_row_stride,
                      const double *d_h, size_t n_h, int kernel, double atol, unsigned flags, double *d_sum,
                      uint64_t *d_count, double *d_cutoff, void *stream);
int pn_kde_self_f32(const pn_index *index, const float *h, size_t n_h, int kernel, double atol, unsigned flags,
                    double *sum_out, uint64_t *count_out, float *cutoff_out);
int pn_kde_self_f64(const pn_index *index, const double *h, size_t n_h, int kernel, double atol, unsigned flags,
                    double *sum_out, uint64_t *count_out, double *cutoff_out);
int pn_kde_self_device_f32(const pn_index *index, const float *d_h, size_t n_h, int kernel, double atol, unsigned flags,
                           double *d_sum, uint64_t *d_count, float *d_cutoff, void *stream);
int pn_kde_self_device_f64(const pn_index *index, const double *d_h, size_t n_h, int kernel, double atol, unsigned flags,
                           double *d_sum, uint64_t *d_count, double *d_cutoff, void *stream);

/* ---- Mean shift on the device (scikit-learn's cluster.MeanShift with its flat kernel: the mode seeking of
 * _mean_shift_single_seed, the merge of the converged modes, the labels): it climbs the tophat density pn_kde_* evaluates.
 * Three entries, each usable alone: pn_mean_shift_* moves seeds to their modes, pn_mean_shift_merge_* turns modes into
 * centres, pn_mean_shift_labels_* labels the indexed rows.  Euclidean indexes only (a Cosine index: PN_ERR_UNSUPPORTED),
 * f32 and f64; T is the index's element type.  Every operation below is plain IEEE f64, unfused, unless it says T.
 * The contract:
 *   One step of a seed at position p (T, dim columns) with bandwidth h (T):
 *     List L = what pn_query_radii_* returns for p with radius h and flags 0: the rows with distance < h (strict), in
 *       ascending row index; h <= 0 or NaN gives an empty list; m = its length.
 *     Dead seed: m == 0 -- the position is unchanged and points_within = 0.
 *     Sum, fixed shape, for every column c, with x = the indexed rows as given at index build:
 *       lane partial P_l = (...((0.0 + (double)x[L_l][c]) + (double)x[L_{l+64}][c]) + ...) for l = 0 .. 63 (missing
 *       positions add nothing),  S_c = (...((P_0 + P_1) + P_2) ... + P_63).
 *       This is the shape of the pn_kde_* sum: the result depends on the list alone -- no floating-point atomics, no
 *       reduction whose shape depends on the launch, PN_OPT_MS_PIECE or scheduling.
 *     New position p'_c = (T)(S_c / (double)m).
 *     Shift: dd_c = (double)p'_c - (double)p_c, t_c = dd_c * dd_c, summed in the same 64-partial shape over the columns
 *       (column c goes to partial c mod 64, ascending c within a partial), shift = sqrt(that sum), correctly rounded.
 *   Mode seeking, a seed starting at p^0, t = 1, 2, ...: at iteration t take the list at p^(t-1).  An empty list: the seed
 *     stops dead -- mode = p^(t-1), points_within = 0, iterations = t - 1, shift = NaN.  Otherwise p^t is the step's
 *     result, and the seed stops when shift <= tol or t == max_iter: mode = p^t, points_within = m (the list the last mean
 *     was taken over, as in scikit-learn), iterations = t, shift = the last one.  max_iter = 1 is exactly one step.  A
 *     seed that has stopped is never queried again.  This is scikit-learn's _mean_shift_single_seed with '<' for '<='.
 *   Merge of modes [ns][dim], points_within [ns] at bandwidth h (T, one value): dead seeds (points_within = 0) take no
 *     part.  The live ones are ranked by (points_within descending, seed number ascending) -- one 64-bit key; scikit-learn
 *     breaks ties of points_within by the coordinates instead.  Walking the ranks, a mode is a centre iff no earlier
 *     centre c has d(centre_c, mode) < h, d = the library's Euclidean distance in T, the bits of pn_euclidean_*.  Centres
 *     are numbered in rank order.  (A points_within above 2^31 - 1, which only a caller's own counts can hold, ranks as
 *     2^31 - 1.)  centre_of_seed[i] = the lowest-numbered centre within h of mode i (a centre's own
 *     number), -1 for a dead seed.  centre_points[c] = that centre's points_within.  Rows of centres_out and
 *     centre_points_out at and beyond n_centres are not written.
 *   Labels: labels[i] = the answer of a k = 1 pn_query_* for indexed row i on an index made of the centres: the nearest
 *     centre by (distance, centre number).  With PN_MS_ORPHANS a row whose nearest centre is not < h away gets -1
 *     (scikit-learn's cluster_all = False); without it h is not looked at.  nc == 0 gives all -1.
 * pn_mean_shift_*: seeds [ns] rows of s_cols columns; s_cols must equal the index's dim (no zip truncation: a mean needs
 * every column).  PN_MS_SEED_ROWS: the indexed rows are the seeds -- seeds must be NULL, ns is taken as n.  h: n_h = 1 (one
 * bandwidth) or ns (one per seed).  tol: a double >= 0.  Outputs by seed: modes_out [ns][dim] dense, points_within_out,
 * iterations_out (nullable), shift_out (nullable); work (nullable, HOST memory in both entries) = {iterations run,
 * seed-steps}: the second is the sum over the iterations of the seeds queried in that iteration.  pn_stats.queries
 * advances by the seed-steps.  PN_OPT_INDEX_BASE affects no output.
 * Argument errors, before any device is touched and in this order: unknown flags; tol NaN or negative; max_iter == 0;
 * NULL outputs (modes, points_within; merge: centres, n_centres; labels: labels); NULL inputs (seeds -- or seeds given
 * with PN_MS_SEED_ROWS --, h; merge: modes, points_within; labels: centres with nc > 0); n_h neither 1 nor ns; s_cols == 0;
 * NULL index; wrong element type: PN_ERR_INVALID; a Cosine index: PN_ERR_UNSUPPORTED; then, with the handle: s_cols other
 * than dim, n_h neither 1 nor n with PN_MS_SEED_ROWS: PN_ERR_INVALID; more than 2^31 - 1 rows or seeds:
 * PN_ERR_UNSUPPORTED.  ns = 0 writes nothing and succeeds (merge: n_centres = 0).
 * Device entry points: everything in HBM but work, written in stream order on `stream`.  Mode seeking BLOCKS THE HOST
 * TWICE PER ITERATION: once after the counting pass, to read the active seeds' offsets it cuts the pieces from, and once
 * after the compaction, to read the number of seeds that go on -- it is not capturable into a graph.  Merge and labels
 * never wait: the merge is a rank sort and 2 ceil(ns / 1024) launches, the labels are one launch.
 * Device memory: mode seeking 2 (dim + 1) sizeof T + 24 bytes per seed, 8 bytes per entry of the largest piece (at most
 * 2^18 seeds and PN_OPT_MS_PIECE entries), and the radius pipeline's workspace -- for a piece that of a batch of at most
 * 2^18 queries, for the counting pass, which takes the active seeds in one call, a padded copy of their positions and 12
 * bytes per (seed, row segment): proportional to the active seeds, never ns x lists.  Merge: 16 N + 12 ns + 40 bytes
 * with N = ns rounded up to a power of two, at least 1024 (28 to 44 bytes per seed at large ns) -- no ns x ns graph.  Known slow case of the merge: a bandwidth so small that nearly every mode is a centre -- the
 * exact work is ns x n_centres x dim.
 * Not in this version: row-sharded handles, Cosine, kernels other than the flat one, estimate_bandwidth. */
#define PN_MS_SEED_ROWS 4
#define PN_MS_ORPHANS 8
int pn_mean_shift_f32(const pn_index *index, const float *seeds, size_t ns, size_t s_cols, ptrdiff_t s_row_stride,
                      const float *h, size_t n_h, double tol, size_t max_iter, unsigned flags, float *modes_out,
                      uint64_t *points_within_out, uint32_t *iterations_out, double *shift_out, uint64_t *work);
int pn_mean_shift_device_f32(const pn_index *index, const float *d_seeds, size_t ns, size_t s_cols, size_t s_row_stride,
                             const float *d_h, size_t n_h, double tol, size_t max_iter, unsigned flags, float *d_modes,
                             uint64_t *d_points_within, uint32_t *d_iterations, double *d_shift, uint64_t *work,
                             void *stream);
int pn_mean_shift_merge_f32(const pn_index *index, const float *modes, size_t ns, const uint64_t *points_within,
                            float h, unsigned flags, float *centres_out, uint64_t *centre_points_out,
                            int64_t *centre_of_seed_out, uint64_t *n_centres_out);
int pn_mean_shift_merge_device_f32(const pn_index *index, const float *d_modes, size_t ns,
                                   const uint64_t *d_points_within, float h, unsigned flags, float *d_centres,
                                   uint64_t *d_centre_points, int64_t *d_centre_of_seed, uint64_t *d_n_centres,
                                   void *stream);
int pn_mean_shift_labels_f32(const pn_index *index, const float *centres, size_t nc, float h, unsigned flags,
                             int64_t *labels);
int pn_mean_shift_labels_device_f32(const pn_index *index, const float *d_centres, size_t nc, float h, unsigned flags,
                                    int64_t *d_labels, void *stream);
int pn_mean_shift_f64(const pn_index *index, const double *seeds, size_t ns, size_t s_cols, ptrdiff_t s_row_stride,
                      const double *h, size_t n_h, double tol, size_t max_iter, unsigned flags, double *modes_out,
                      uint64_t *points_within_out, uint32_t *iterations_out, double *shift_out, uint64_t *work);
int pn_mean_shift_device_f64(const pn_index *index, const double *d_seeds, size_t ns, size_t s_cols,
                             size_t s_row_stride, const double *d_h, size_t n_h, double tol, size_t max_iter,
                             unsigned flags, double *d_modes, uint64_t *d_points_within, uint32_t *d_iterations,
                             double *d_shift, uint64_t *work, void *stream);
int pn_mean_shift_merge_f64(const pn_index *index, const double *modes, size_t ns, const uint64_t *points_within,
                            double h, unsigned flags, double *centres_out, uint64_t *centre_points_out,
                            int64_t *centre_of_seed_out, uint64_t *n_centres_out);
int pn_mean_shift_merge_device_f64(const pn_index *index, const double *d_modes, size_t ns,
                                   const uint64_t *d_points_within, double h, unsigned flags, double *d_centres,
                                   uint64_t *d_centre_points, int64_t *d_centre_of_seed, uint64_t *d_n_centres,
                                   void *stream);
int pn_mean_shift_labels_f64(const pn_index *index, const double *centres, size_t nc, double h, unsigned flags,
                             int64_t *labels);
int pn_mean_shift_labels_device_f64(const pn_index *index, const double *d_centres, size_t nc, double h, unsigned flags,
                                    int64_t *d_labels, void *stream);

/* ---- k-means (extension; Euclidean indexes only; T = the index's element type).  DESIGN.md 4.22.
 *   Assignment of the indexed rows to centres [nc][dim] (dense, T): labels[i] = exactly what
 *     pn_mean_shift_labels_*(centres, nc, h, flags = 0) writes: the nearest centre by (distance key, centre number), the
 *     distance being the bits of pn_euclidean_* and a NaN distance the canonical NaN key above +inf; nc == 0 gives all -1.
 *     dist[i] = that distance, NaN where the label is -1.
 *   SUM4096, the one sum shape of these entry points; it depends on the length of the sequence alone.  Cut the sequence
 *     into consecutive segments of 4096 terms.  A segment's sum is the 64-lane shape of pn_kde_* / pn_mean_shift_*:
 *     P_l = (((0.0 + t_l) + t_(l+64)) + ...) for l = 0 .. 63 (a lane without a term: 0.0), S = ((P_0 + P_1) + ... + P_63).
 *     The total is ((S_0 + S_1) + S_2) ... in segment order; an empty sequence sums to 0.0.  IEEE f64, unfused, no
 *     floating-point atomics: the result does not depend on the launch.
 *   Inertia = SUM4096 over i = 0 .. n - 1 of (double)dist[i] * (double)dist[i], the term of a row with label -1 being 0.0.
 *   pn_kmeans_*: Lloyd iterations from the caller's initial centres [nc][dim].  Iteration t = 1, 2, ...: assign to the
 *     current centres; for every cluster c let m_c be the number of its members, taken in ascending row index.  m_c = 0:
 *     the centre is unchanged (scikit-learn relocates it; a stated deviation, visible in counts_out).  Otherwise, per
 *     column, S = SUM4096(members' (double)x[i][col]) and the new centre is (T)(S / (double)m_c).  t_c = the sum over the
 *     columns of ((double)new - (double)old)^2 in the 64-partial shape (column col to partial col mod 64, ascending
 *     within a partial from 0.0; then ((p_0 + p_1) + ... + p_63)), exactly as mean shift's shift;
 *     shift2 = (((0.0 + t_0) + t_1) + ...) in centre order.  Stop when shift2 <= tol (a double >= 0, absolute) or
 *     t == max_iter.  After the stop there is one more assignment to the final centres: labels, distances, counts and
 *     inertia belong to the centres returned.  iterations = the t of the stop, shift2 = the last one.
 *   Outputs: centres_out [nc][dim], labels_out [n], dist_out [n] (nullable), counts_out [nc] (nullable: the members of the
 *   final assignment), inertia_out, iterations_out, shift2_out (one value each, nullable).  flags must be 0.
 *   PN_OPT_INDEX_BASE affects no output.  pn_stats.queries advances by n per assignment.
 * Engines (PN_OPT_ENGINE; results never depend on them).  The filter of DESIGN.md 4.22 -- a bf16 MFMA lower bound of every
 * (row, centre) distance, one candidate per row evaluated exactly, a proof per row -- takes 8 <= dim <= 320, f32 and f64
 * indexes alike; rows it cannot prove (ties, rows within the filter's slack of a bisector, anything not finite or with a
 * squared norm of 2^100 or more) are listed on the device and answered by the exact kernel, and their number is added to
 * pn_stats.fallback_queries.  PN_ENGINE_EXACT: the exact kernel alone.  PN_ENGINE_BF16: the filter wherever it is
 * eligible (pn_index_set_option accepts that engine, as ever, only on a handle whose k-NN bf16 tier exists;
 * PN_OPT_KMEANS_FILTER = 1 forces the k-means filter on any handle).  PN_ENGINE_AUTO (and PN_ENGINE_MFMA): the filter
 * where it is eligible, nc >= 64, dim >= 64 and n * nc * dim >= 8e9 (16e9 where dim < 128); below that the exact kernel, whose whole work is as
 * small as the filter's fixed cost (and on narrow rows no dearer per centre than the filter).  One centre (nc = 1) is
 * always the exact kernel's: there is nothing to filter.
 * Argument errors, before any device is touched and in this order: unknown flags; (pn_kmeans_*) tol NaN or negative;
 * max_iter == 0; NULL required outputs (labels; pn_kmeans_*: centres_out); NULL inputs (centres with nc > 0; pn_kmeans_*:
 * the initial centres); (pn_kmeans_*) nc == 0; NULL index; wrong element type: PN_ERR_INVALID; a Cosine index:
 * PN_ERR_UNSUPPORTED; more than 2^31 - 1 rows or centres: PN_ERR_UNSUPPORTED.  n == 0 succeeds: inertia 0, counts 0, the
 * centres copied, iterations 0, shift2 0.
 * Device entry points: everything in HBM, written in stream order on `stream`.  pn_kmeans_assign_device_* never waits.
 * pn_kmeans_device_* BLOCKS THE HOST ONCE PER ITERATION, to read the stop word (16 bytes) -- it is not capturable into a
 * graph.  Device memory of a call (workspace of the handle): the exact path needs none per row but sizeof T bytes when
 * the inertia is asked for without the distances (and 8 bytes per 4096 rows for the inertia); the filter adds
 * 4 * dp + 32 bytes per row (dp = dim rounded up to 16: the two bf16 row images, packed once per call, their norms, the
 * candidate, its threshold and the list of unproven rows) and 4 * dp + 4 bytes per centre rounded up to 32;
 * pn_kmeans_*: 16 N bytes (N = n rounded up to a power of two, at least 1024: the sort of the members' lists),
 * 8 * dim * (n / 4096 + nc) bytes of segment sums and 36 bytes per centre.
 * Not in this version: Cosine / spherical k-means, row-sharded handles, mini-batch, empty-cluster relocation, a
 * device-driven iteration loop. */
int pn_kmeans_assign_f32(const pn_index *index, const float *centres, size_t nc, unsigned flags, int64_t *labels_out,
                         float *dist_out, double *inertia_out);
int pn_kmeans_assign_device_f32(const pn_index *index, const float *d_centres, size_t nc, unsigned flags,
                                int64_t *d_labels, float *d_dist, double *d_inertia, void *stream);
int pn_kmeans_f32(const pn_index *index, const float *init_centres, size_t nc, double tol, size_t max_iter, unsigned flags,
                  float *centres_out, int64_t *labels_out, float *dist_out, uint64_t *counts_out, double *inertia_out,
                  uint64_t *iterations_out, double *shift2_out);
int pn_kmeans_device_f32(const pn_index *index, const float *d_init_centres, size_t nc, double tol, size_t max_iter,
                         unsigned flags, float *d_centres, int64_t *d_labels, float *d_dist, uint64_t *d_counts,
                         double *d_inertia, uint64_t *d_iterations, double *d_shift2, void *stream);
int pn_kmeans_assign_f64(const pn_index *index, const double *centres, size_t nc, unsigned flags, int64_t *labels_out,
                         double *dist_out, double *inertia_out);
int pn_kmeans_assign_device_f64(const pn_index *index, const double *d_centres, size_t nc, unsigned flags,
                                int64_t *d_labels, double *d_dist, double *d_inertia, void *stream);
int pn_kmeans_f64(const pn_index *index, const double *init_centres, size_t nc, double tol, size_t max_iter, unsigned flags,
                  double *centres_out, int64_t *labels_out, double *dist_out, uint64_t *counts_out, double *inertia_out,
                  uint64_t *iterations_out, double *shift2_out);
int pn_kmeans_device_f64(const pn_index *index, const double *d_init_centres, size_t nc, double tol, size_t max_iter,
                         unsigned flags, double *d_centres, int64_t *d_labels, double *d_dist, uint64_t *d_counts,
                         double *d_inertia, uint64_t *d_iterations, double *d_shift2, void *stream);
/* diagnostic: the k-means filter's lower bounds themselves.  bounds_out[i * nc + c] = L(x_i, c) <= |x_i - c|^2 in real
 * arithmetic for every indexed row i and centre c (kmeans.hip states the bound), NaN where the row or a centre is flagged
 * (not finite, a squared norm of 2^100 or more).  Host pointers; 8 <= dim <= 320, else PN_ERR_UNSUPPORTED.  Tests check
 * the inequality pair by pair. */
int pn_kmeans_bounds_f32(const pn_index *index, const float *centres, size_t nc, double *bounds_out);

/* ---- distance::pairwise(x, &Euclidean) (src/distance.rs:58-74): n x n
 * symmetric matrix, zero diagonal, n < 2 -> zeros. Host in, host out. */
int pn_pairwise_f32(const float *x, size_t n_rows, size_t n_cols, ptrdiff_t row_stride, int device,
                    float *out);
int pn_pairwise_f64(const double *x, size_t n_rows, size_t n_cols, ptrdiff_t row_stride, int device,
                    double *out);
/* the same with rows and the n x n result in HBM (extension; row_stride >= n_cols elements), enqueued on `stream` and
 * complete when the call returns.  Only the pairs i < j are evaluated, each written twice (src/distance.rs:66-72). */
int pn_pairwise_device_f32(const float *d_x, size_t n_rows, size_t n_cols, size_t row_stride, int device, float *d_out,
                           void *stream);
int pn_pairwise_device_f64(const double *d_x, size_t n_rows, size_t n_cols, size_t row_stride, int device,
                           double *d_out, void *stream);

/* ---- Metric<A> for Euclidean (src/distance.rs:21-55): scalar, host-side by
 * design (one pair per call is not GPU work); bit-exact with the batched path. */
float pn_euclidean_f32(const float *a, const float *b, size_t len);
double pn_euclidean_f64(const double *a, const double *b, size_t len);
float pn_reuclidean_f32(const float *a, const float *b, size_t len);
double pn_reuclidean_f64(const double *a, const double *b, size_t len);
float pn_rdistance_to_distance_f32(float d);
double pn_rdistance_to_distance_f64(double d);
float pn_distance_to_rdistance_f32(float d);
double pn_distance_to_rdistance_f64(double d);

/* ---- Metric<A> for Cosine (src/distance.rs:76-122): distance = 1 - dot / (|a| |b|) with the reference's three
 * sequential sums (the dot product over the shorter length, each norm over its own vector); rdistance and both
 * conversions are the identity there.  pn_pairwise_cosine_*: distance::pairwise(x, &Cosine) on the GPU, same
 * contract as pn_pairwise_*.  BallTree::new(points, Cosine): pn_index_create_cosine_* above. */
float pn_cosine_f32(const float *a, size_t len_a, const float *b, size_t len_b);
double pn_cosine_f64(const double *a, size_t len_a, const double *b, size_t len_b);
int pn_pairwise_cosine_f32(const float *x, size_t n_rows, size_t n_cols, ptrdiff_t row_stride, int device,
                           float *out);
int pn_pairwise_cosine_f64(const double *x, size_t n_rows, size_t n_cols, ptrdiff_t row_stride, int device,
                           double *out);

/* ---- row-sharded corpora: merge `n_parts` per-shard results
 * (each nq x k_part, already carrying global indices via PN_OPT_INDEX_BASE and
 * sorted by (distance, index)) into the global top k_out.  Device pointers.
 * Part p's indices start at d_idx_parts + p * idx_part_stride (elements), its
 * distances at d_dist_parts + p * dist_part_stride, each laid out [query][k_part]
 * -- so one all-gather of a packed per-rank buffer {idx[nq][k] | dist[nq][k]}
 * can be merged in place.  Slots with index UINT64_MAX are treated as absent. */
int pn_merge_topk_device_f32(const uint64_t *d_idx_parts, const float *d_dist_parts, size_t n_parts,
                             size_t idx_part_stride, size_t dist_part_stride, size_t nq, size_t k_part,
                             size_t k_out, uint64_t *d_idx_out, float *d_dist_out, int device, void *stream);
int pn_merge_topk_device_f64(const uint64_t *d_idx_parts, const double *d_dist_parts, size_t n_parts,
                             size_t idx_part_stride, size_t dist_part_stride, size_t nq, size_t k_part,
                             size_t k_out, uint64_t *d_idx_out, double *d_dist_out, int device, void *stream);

/* ---- tree introspection: BallTree::{num_nodes, children_of, points_of, radius_of, compare_nodes,
 * node_distance_lower_bound} (src/ball_tree.rs:296-353), public in the reference for downstream dual-tree algorithms.
 * Queries on this engine never use a tree; the first call of any function below builds -- once, on the host, from the
 * index's own copy of the points -- the implicit complete binary ball tree exactly as the reference does
 * (src/ball_tree.rs:38-63, 445-461, 504-613: node i has children 2i+1 / 2i+2, median split on the column of maximum
 * spread, sequential-mean centroid, radius = largest distance to it UNDER THE INDEX'S METRIC -- Node::init and
 * node_distance_lower_bound call metric.distance, src/ball_tree.rs:309, 459: on a pn_index_create_cosine_* index
 * radius_of, compare_nodes and node_distance_lower_bound are Cosine::distance values, the split and the permutation do
 * not depend on the metric), so every answer equals the reference's node for node.  O(n d log n) time and (nodes x d) extra host memory, paid only by callers of this API.
 * A node number >= num_nodes is PN_ERR_INVALID (the reference panics).
 *   children_of:   *is_some = 0 for a leaf (None), else 1 with (*left, *right) = (2n+1, 2n+2)
 *   points_of:     *idx points INTO the tree's permutation (valid until pn_index_destroy), *count entries
 *   compare_nodes: *ordering = -1 Less / 0 Equal / 1 Greater by radius, 2 = None (a NaN radius)
 *   pn_tree_centroid_of: the node's centroid (n_cols elements of the index's type); private in the reference, exported
 *                  for tests */
int pn_tree_num_nodes(const pn_index *index, uint64_t *out);
int pn_tree_children_of(const pn_index *index, uint64_t node, int *is_some, uint64_t *left, uint64_t *right);
int pn_tree_points_of(const pn_index *index, uint64_t node, const uint64_t **idx, uint64_t *count);
int pn_tree_radius_of_f32(const pn_index *index, uint64_t node, float *out);
int pn_tree_radius_of_f64(const pn_index *index, uint64_t node, double *out);
int pn_tree_compare_nodes(const pn_index *index, uint64_t x, uint64_t y, int *ordering);
int pn_tree_node_distance_lower_bound_f32(const pn_index *index, uint64_t n1, uint64_t n2, float *out);
int pn_tree_node_distance_lower_bound_f64(const pn_index *index, uint64_t n1, uint64_t n2, double *out);
int pn_tree_centroid_of(const pn_index *index, uint64_t node, void *out_n_cols_elements);

/* ---- row-sharded corpora with the exchange behind the ABI (north_star: "the corpus shards by row
 * across the 8 GPUs of one node, per-shard (idx, dist) top-k merged by one RCCL allgather over xGMI").  Shard g of G
 * holds rows [g ceil(N/G), min(N, (g+1) ceil(N/G))); queries are replicated; each shard answers on its rows with global
 * indices; ONE ncclAllGather per query batch of the packed per-GPU buffer {idx[nq][k'] | dist[nq][k']}; a merge kernel
 * ordered by (distance, index).  Results are identical for every number of shards.  RCCL is loaded at run time; if
 * it cannot be, these entry points fail with PN_ERR_COMM (everything else keeps working).
 *
 *   pn_sharded_create_f32             BallTree::new over `n_devices` row shards driven by THIS process: shard g lives
 *                                     on devices[g] (ncclCommInitAll over the distinct devices; a device named several
 *                                     times holds several shards, merged locally before the exchange).  Same
 *                                     validation and errors as pn_index_create_f32.
 *   pn_comm_unique_id +               one process per GPU: rank 0 gets a communicator id (PN_COMM_ID_BYTES bytes),
 *   pn_sharded_create_rank_device_f32 the host program carries it to the other ranks, every rank passes it with ITS
 *                                     rows (already on `device`, row-major, inner stride 1): n_local must be the
 *                                     library's shard size for (n_total, rank, world) -- 0 for a rank beyond the corpus,
 *                                     which still takes part in every exchange.  Collective: all ranks must call it.
 *   pn_sharded_query_f32              host queries in, host results out (BallTree::query semantics, pn_query_f32's
 *                                     argument meaning); with one process per GPU every rank must call it with the SAME
 *                                     queries and every rank receives the full answer.
 *   pn_sharded_query_device_f32       the same, queries/results in HBM of the GPU this process drives, enqueued on
 *                                     `stream` (handles that drive exactly one GPU); batches above 131 072 queries are
 *                                     cut into chunks whose exchange + merge overlap the next chunk's filter.
 *   pn_sharded_query_radius_f32       BallTree::query_radius over all shards, CSR like pn_query_radius_f32.
 * One query at a time per handle (the communicator and the exchange buffers are per-handle state, serialised inside). */
#define PN_COMM_ID_BYTES 128
typedef struct pn_sharded pn_sharded;
typedef struct pn_sharded_info_t {
    uint64_t n_points;        /* rows of the whole corpus */
    uint64_t dim;
    uint64_t local_first_row; /* first row held by this process */
    uint64_t local_rows;      /* rows held by this process */
    int32_t n_shards;         /* row shards over all processes */
    int32_t world;            /* ranks of the RCCL communicator = GPUs */
    int32_t local_shards;     /* shards held by this process */
    int32_t rank;             /* this process's rank (0 with one process) */
    int32_t mfma_eligible;    /* every local shard can be served by the f32 MFMA filter / the bf16 filter (pn_info) */
    int32_t bf16_eligible;
} pn_sharded_info_t;
int pn_comm_unique_id(void *id_out /* PN_COMM_ID_BYTES */);
int pn_sharded_create_f32(const float *points, size_t n_rows, size_t n_cols, ptrdiff_t row_stride,
                          ptrdiff_t col_stride, const int *devices, int n_devices, pn_sharded **out);
int pn_sharded_create_rank_device_f32(const float *d_rows, size_t n_local, size_t n_cols, size_t row_stride,
                                      uint64_t n_total, int rank, int world, const void *comm_id, int device,
                                      void *stream, pn_sharded **out);
/* the same over an f64 corpus (BallTree<f64, Euclidean>): every shard is an f64 index (pn_index_create_f64: bf16 filter,
 * f64 re-rank and proof), distances travel and merge as f64 */
int pn_sharded_create_f64(const double *points, size_t n_rows, size_t n_cols, ptrdiff_t row_stride,
                          ptrdiff_t col_stride, const int *devices, int n_devices, pn_sharded **out);
int pn_sharded_create_rank_device_f64(const double *d_rows, size_t n_local, size_t n_cols, size_t row_stride,
                                      uint64_t n_total, int rank, int world, const void *comm_id, int device,
                                      void *stream, pn_sharded **out);
/* BallTree::new(points, Cosine) over row shards driven by THIS process (every shard a pn_index_create_cosine_* index;
 * queries through pn_sharded_query_* / pn_sharded_query_radius_* of the same element type) */
int pn_sharded_create_cosine_f32(const float *points, size_t n_rows, size_t n_cols, ptrdiff_t row_stride,
                                 ptrdiff_t col_stride, const int *devices, int n_devices, pn_sharded **out);
int pn_sharded_create_cosine_f64(const double *points, size_t n_rows, size_t n_cols, ptrdiff_t row_stride,
                                 ptrdiff_t col_stride, const int *devices, int n_devices, pn_sharded **out);
void pn_sharded_destroy(pn_sharded *sharded);
int pn_sharded_info(const pn_sharded *sharded, pn_sharded_info_t *out);
int pn_sharded_set_option(pn_sharded *sharded, int option, int64_t value); /* forwarded to every local shard */
int pn_sharded_get_stats(const pn_sharded *sharded, pn_stats *out, int reset); /* summed over the local shards */
int pn_sharded_query_f32(const pn_sharded *sharded, const float *queries, size_t nq, size_t q_cols,
                         ptrdiff_t q_row_stride, size_t k, uint64_t *idx_out, float *dist_out);
int pn_sharded_query_device_f32(const pn_sharded *sharded, const float *d_queries, size_t nq, size_t q_cols,
                                size_t q_row_stride, size_t k, uint64_t *d_idx_out, float *d_dist_out, void *stream);
int pn_sharded_query_radius_f32(const pn_sharded *sharded, const float *queries, size_t nq, size_t q_cols,
                                ptrdiff_t q_row_stride, float radius, uint64_t *offsets, uint64_t **idx_out);
int pn_sharded_query_f64(const pn_sharded *sharded, const double *queries, size_t nq, size_t q_cols,
                         ptrdiff_t q_row_stride, size_t k, uint64_t *idx_out, double *dist_out);
int pn_sharded_query_device_f64(const pn_sharded *sharded, const double *d_queries, size_t nq, size_t q_cols,
                                size_t q_row_stride, size_t k, uint64_t *d_idx_out, double *d_dist_out, void *stream);
int pn_sharded_query_radius_f64(const pn_sharded *sharded, const double *queries, size_t nq, size_t q_cols,
                                ptrdiff_t q_row_stride, double radius, uint64_t *offsets, uint64_t **idx_out);
/* pn_query_radius_device_* on a sharded handle with ONE shard (what a rank of a one-GPU job holds); several shards:
 * PN_ERR_UNSUPPORTED -- their ragged exchange goes through the host entry point above. */
int pn_sharded_query_radius_device_f32(const pn_sharded *sharded, const float *d_queries, size_t nq, size_t q_cols,
                                       size_t q_row_stride, float radius, uint64_t *d_offsets, uint64_t *d_idx,
                                       size_t capacity, uint64_t *d_total, void *stream);
int pn_sharded_query_radius_device_f64(const pn_sharded *sharded, const double *d_queries, size_t nq, size_t q_cols,
                                       size_t q_row_stride, double radius, uint64_t *d_offsets, uint64_t *d_idx,
                                       size_t capacity, uint64_t *d_total, void *stream);
/* pn_query_radius_with_distance_* over all shards: the lists of pn_sharded_query_radius_* with their distances (global
 * rows); PN_RADIUS_SORTED: each query's list by (distance, global row), merged from the shards' sorted lists.  With one
 * process per GPU the distances travel by a second padded all-gather of the lists' shape. */
int pn_sharded_query_radius_with_distance_f32(const pn_sharded *sharded, const float *queries, size_t nq, size_t q_cols,
                                              ptrdiff_t q_row_stride, float radius, unsigned flags, uint64_t *offsets,
                                              uint64_t **idx_out, float **dist_out);
int pn_sharded_query_radius_with_distance_f64(const pn_sharded *sharded, const double *queries, size_t nq, size_t q_cols,
                                              ptrdiff_t q_row_stride, double radius, unsigned flags, uint64_t *offsets,
                                              uint64_t **idx_out, double **dist_out);
/* pn_query_radius_with_distance_device_* on a handle with ONE shard; several shards: PN_ERR_UNSUPPORTED */
int pn_sharded_query_radius_with_distance_device_f32(const pn_sharded *sharded, const float *d_queries, size_t nq,
                                                     size_t q_cols, size_t q_row_stride, float radius, unsigned flags,
                                                     uint64_t *d_offsets, uint64_t *d_idx, float *d_dist,
                                                     size_t capacity, uint64_t *d_total, void *stream);
int pn_sharded_query_radius_with_distance_device_f64(const pn_sharded *sharded, const double *d_queries, size_t nq,
                                                     size_t q_cols, size_t q_row_stride, double radius, unsigned flags,
                                                     uint64_t *d_offsets, uint64_t *d_idx, double *d_dist,
                                                     size_t capacity, uint64_t *d_total, void *stream);
/* self-queries over row shards: every LOCAL row (rows [local_first_row, local_first_row + local_rows) of
 * pn_sharded_info -- all n rows for a pn_sharded_create_* handle, the rank's own rows in rank mode, none for a rank beyond
 * the corpus) against the whole corpus, with global row numbers.  The answer of local row i is bit-identical to that of
 * global row local_first_row + i from pn_query_self_* / pn_query_radius_self_* over the whole corpus (same indices,
 * distance bits and order) for every shard count and placement; flags, kout and errors are theirs.  In rank mode every
 * entry is collective: all ranks call it with the same k / r / flags.
 * Each step, every GPU contributes up to 2^18 / world of its rows, one all-gather makes them the query batch of every
 * GPU, and each GPU keeps only the answers of its own rows: the workspace stays that of a 2^18-query batch.  A rank whose
 * local work fails still enters the step's exchange; the host entry points then fail on every rank (the device entry
 * returns the error on the failing rank only -- it reads nothing back).
 *   pn_sharded_query_self_*               host [local_rows][kout]
 *   pn_sharded_query_self_device_*        [local_rows][kout] in HBM of the ONE GPU the handle drives (rank mode, or all
 *                                         shards on one device; else PN_ERR_UNSUPPORTED), enqueued on `stream` with the
 *                                         contract of pn_sharded_query_device_*
 *   pn_sharded_query_radius_self_*        CSR over the local rows: offsets [local_rows + 1], *idx_out / *dist_out
 *                                         allocated by the library (pn_free)
 *   pn_sharded_query_radius_self_device_* pn_query_radius_self_device_* on a handle with ONE shard; several shards:
 *                                         PN_ERR_UNSUPPORTED (their ragged exchange goes through the host entry). */
int pn_sharded_query_self_f32(const pn_sharded *sharded, size_t k, unsigned flags, uint64_t *idx_out, float *dist_out);
int pn_sharded_query_self_f64(const pn_sharded *sharded, size_t k, unsigned flags, uint64_t *idx_out, double *dist_out);
int pn_sharded_query_self_device_f32(const pn_sharded *sharded, size_t k, unsigned flags, uint64_t *d_idx, float *d_dist,
                                     void *stream);
int pn_sharded_query_self_device_f64(const pn_sharded *sharded, size_t k, unsigned flags, uint64_t *d_idx, double *d_dist,
                                     void *stream);
int pn_sharded_query_radius_self_f32(const pn_sharded *sharded, float radius, unsigned flags, uint64_t *offsets,
                                     uint64_t **idx_out, float **dist_out);
int pn_sharded_query_radius_self_f64(const pn_sharded *sharded, double radius, unsigned flags, uint64_t *offsets,
                                     uint64_t **idx_out, double **dist_out);
int pn_sharded_query_radius_self_device_f32(const pn_sharded *sharded, float radius, unsigned flags, uint64_t *d_offsets,
                                            uint64_t *d_idx, float *d_dist, size_t capacity, uint64_t *d_total,
                                            void *stream);
int pn_sharded_query_radius_self_device_f64(const pn_sharded *sharded, double radius, unsigned flags, uint64_t *d_offsets,
                                            uint64_t *d_idx, double *d_dist, size_t capacity, uint64_t *d_total,
                                            void *stream);

/* ---- diagnostic: the first-tier filter's lower bounds themselves.  bounds_out[q * n_rows + i] = L'(q, p_i)
 * for the first n_rows corpus rows (clamped to n_points), with L' + qnorm_out[q] <= |q - p_i|^2 in real
 * arithmetic; qnorm_out[q] <= |q - mu|^2 where mu (mu_out, n_cols floats, nullable) is the translation vector the
 * tier works with -- the corpus mean (petal-neighbors_amd/csrc/bf16_filter.hip states the bound).  Host pointers;
 * q_cols must equal the index dimension.  Not part of the reference's interface: tests use it to check the
 * inequality and to measure the matrix core's accumulation error against the allowance the proof makes. */
int pn_bf16_bounds_f32(const pn_index *index, const float *queries, size_t nq, size_t q_cols,
                       ptrdiff_t q_row_stride, size_t n_rows, float *bounds_out, double *qnorm_out, float *mu_out);
/* ---- diagnostic: the bf16 tier's hardware self-test (round 4).  The bound allows the matrix core's f32 accumulation an
 * error of 2^-13 * sum|terms| -- a measured property of gfx950, not a documented one.  The library checks it itself the
 * first time an index on `device` is given its bf16 tier (synthetic chains of 8 and 65 MFMA steps against terms rebuilt
 * in f64) and refuses the tier (bf16_eligible = 0, pn_last_error says why) when the error exceeds 2 % of the allowance.
 * This entry runs the check (again) and returns the measured fraction of the allowance in *ratio_out. */
int pn_bf16_selftest(int device, float *ratio_out);
/* ---- diagnostic: the handle's seed-model feedback (round 4).  Every finished bf16-tier call tells the
 * handle whether its starting thresholds -- from the index's seed model or from a scout launch -- left queries unproven;
 * the handle then aims higher, goes back to the scout, or (after 64 scouted calls, at most three times) gives the model
 * another try.  This entry feeds one such observation (model_seed: the call was seeded by the model; `unproven` of `nq`
 * queries went to the next tier) into the handle exactly as a finished call would and returns the state in out[4] =
 * { off, widen steps, scouted calls since off, retries used }: tests drive the state machine without having to
 * construct corpora and batches that defeat the model. */
int pn_debug_seed_model_feedback(pn_index *index, int model_seed, uint64_t unproven, uint64_t nq, int32_t *out4);

/* ---- synthetic data (bench / tests): uniform [0,1) with exactly 24 random
 * bits, x[i] = (mix32(seed, first_counter + i) >> 8) * 2^-24, generated in
 * HBM; bit-identical to oracle_fill_uniform_f32. */
int pn_fill_uniform_device_f32(float *d_out, uint64_t count, uint64_t seed, uint64_t first_counter,
                               int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PETAL_MI355X_H */
