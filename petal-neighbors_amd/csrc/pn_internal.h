// pn_internal.h -- shared declarations between the translation units of
// libpetal_mi355x.so (gfx950 only).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <type_traits>

#include "bf16_launch.h"

namespace pn {

// PN_DEBUG_PLAN (read once per process): index.hip prints every bf16 plan, bf16_filter.hip every main-pass launch
inline bool debug_plan() {
    static const bool on = getenv("PN_DEBUG_PLAN") != nullptr;
    return on;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel instantiation, device): the attribute belongs to
// the device's copy of the kernel, and index handles on different devices -- or threads -- may launch the same
// instantiation.  One static instance per launcher.
struct LdsAttrOnce {
    std::atomic<uint64_t> done{0};
    hipError_t ensure(const void *kern, size_t bytes) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const uint64_t bit = 1ull << (dev & 63);
        if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
        e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
        return e;
    }
};

// ---- tiling constants of the exact scan (exact_scan.hip)
constexpr int kTileQ = 64;    // queries per workgroup tile
constexpr int kTileP = 64;    // corpus rows per tile step
constexpr int kChunkK = 32;   // coordinates staged per LDS chunk
constexpr int kRowAlign = 8;  // device rows are zero-padded to a multiple of 8 elements
constexpr int kRowPad = 256;  // device row COUNT is padded (zero rows) to a multiple of this

// ---- sortable integer keys.  Distances are >= +0 or NaN, so the IEEE bit
// pattern read as an unsigned integer is monotone; NaN is canonicalised to the
// quiet-NaN pattern, which is greater than +inf: exactly ordered-float's total
// order used by Neighbor (reference src/ball_tree.rs:396-421).
template <typename T> struct KeyOf;
template <> struct KeyOf<float> {
    using type = uint32_t;
    static constexpr type kMax = 0xFFFFFFFFu;
    static constexpr type kNaN = 0x7FC00000u;
};
template <> struct KeyOf<double> {
    using type = uint64_t;
    static constexpr type kMax = 0xFFFFFFFFFFFFFFFFull;
    static constexpr type kNaN = 0x7FF8000000000000ull;
};

// Per-(segment, query) candidate buffers in HBM, filled by the scan kernels and
// consumed by the select kernel.  Layout: [seg][query][slot].
struct CandBuf {
    void *keys;      // KeyOf<T>::type (exact) or float bits of the lower bound (MFMA filter)
    uint32_t *idx;   // corpus row (local to this index)
    uint32_t *cnt;   // entries in use            [seg][query]
    void *tau;       // last threshold (same type as keys) [seg][query]
    size_t nq_pad;   // queries padded to a multiple of kTileQ
    int nseg;
    int cap;         // slots per (segment, query); multiple of 64
    int idx_stride = 1;  // 2: keys and idx interleaved as (key, row) pairs, idx = keys + 1 (bf16 filter)
    int final_keep = 0;  // bf16 filter, 64-slot buffers: a buffer holding at most this many entries ends its run uncut (0: k')
};

inline size_t round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// ---- exact_scan.hip
// lo_key/lo_idx (nullable, [nq_pad]): only entries strictly after (lo_key[q], lo_idx[q]) take part
// nq_dev (nullable) / nq_off: device-driven query count -- only the first min(nq, max(*nq_dev - nq_off, 0)) queries
// exist; the grid is sized for nq and the surplus query tiles exit at once (second tier behind a filter)
// pnorm / qnorm (nullable, together): the index's metric is Cosine -- distance = 1 - dot / (qnorm[q] pnorm[row])
// qsel (nullable, f32 Euclidean only): query r of the launch is row qsel[nq_off + r] of Q -- the flagged queries of a
// filter tier read in place (no gather launch)
template <typename T>
hipError_t launch_exact_knn(const T *P, size_t n, int dim, size_t ldp, const T *Q, int nq, size_t ldq, int kp,
                            size_t seg_len, const CandBuf &cb, const void *lo_key, const uint32_t *lo_idx,
                            const uint32_t *nq_dev, uint32_t nq_off, const T *pnorm, const T *qnorm, hipStream_t s,
                            const uint32_t *qsel = nullptr);
// radius: count pass (fill == nullptr) then fill pass.  counts/offsets are [query][seg].
template <typename T>
hipError_t launch_exact_radius(const T *P, size_t n, int dim, size_t ldp, const T *Q, int nq, size_t ldq, T r,
                               size_t seg_len, int nseg, uint32_t *counts, const uint64_t *offsets, uint64_t *fill,
                               uint64_t index_base, const T *pnorm, const T *qnorm, hipStream_t s,
                               const uint32_t *qsel = nullptr, const uint32_t *nq_dev = nullptr,
                               uint64_t capacity = ~0ull, T *fill_dist = nullptr, const T *radii = nullptr);
// qsel / nq_dev (nullable): query r of the launch is row qsel[r] of Q, only the first *nq_dev listed queries exist (grid
// sized for nq); counts / offsets indexed by r.  capacity: fill positions at or beyond it are not written.
// fill_dist (nullable): the fill pass also writes each listed row's distance at its position

// ---- radius_device.hip: the device-side plumbing of pn_query_radius_device_* (no host round trip)
// list the queries the exact scan must answer: need[q] = over[q] | bad[q] (either nullable); sel[0 .. *nsel) <- those q
// ascending, pos[q] <- position in sel or 0xFFFFFFFF; nkept[q] <- 0 for listed queries.  nsel zeroed by the caller.
hipError_t launch_rad_list(const uint32_t *over, const uint32_t *bad, int nq, uint32_t *nkept, uint32_t *sel,
                           uint32_t *pos, uint32_t *nsel, hipStream_t s);
// per-query result counts: fin[q] = pos[q] valid ? sum_seg counts_x[pos[q] * nseg + seg] : nkept[q]
// (pos / nkept nullable: every query listed at its own position / none kept)
hipError_t launch_rad_counts(const uint32_t *nkept, const uint32_t *pos, const uint32_t *counts_x, int nseg, int nq,
                             uint32_t *fin, hipStream_t s);
// offsets[0 .. n] <- exclusive prefix sums of in[0 .. n) (64-bit); scratch: >= (n / 4096 + 2) * 8 bytes; total (nullable)
// <- offsets[n]
hipError_t launch_exclusive_scan_u32(const uint32_t *in, size_t n, uint64_t *offsets, uint64_t *scratch, uint64_t *total,
                                     hipStream_t s);
// offs_x[r * nseg + seg] <- offsets[sel ? sel[r] : r] + sum_{t < seg} counts_x[r * nseg + t], r < (nsel ? *nsel : nq)
hipError_t launch_rad_seg_offsets(const uint64_t *offsets, const uint32_t *sel, const uint32_t *nsel, int nq,
                                  const uint32_t *counts_x, int nseg, uint64_t *offs_x, hipStream_t s);
// out[offsets[q] + e] <- index_base + kept[q * kept_stride + e], e < nkept[q], positions below capacity only
// kept_dist / out_dist (nullable, elements of dist_bytes = 4 | 8): the kept rows' distances go along
hipError_t launch_radius_gather_cap(const uint32_t *kept, const uint32_t *nkept, const uint64_t *offsets, int nq,
                                    size_t kept_stride, uint64_t index_base, uint64_t *out, uint64_t capacity,
                                    hipStream_t s, const void *kept_dist = nullptr, void *out_dist = nullptr,
                                    int dist_bytes = 0);

// ---- self_graph.hip: self-queries of an index (pn_query_self_*, pn_query_radius_self_*)
// out[q][r] (r < kout = kin - 1) <- in[q][r] with the entry equal to self0 + q dropped, else the last one
template <typename T>
hipError_t launch_knn_self_exclude(const uint64_t *in_idx, const T *in_dist, size_t nq, int kin, int kout,
                                   uint64_t self0, uint64_t *out_idx, T *out_dist, hipStream_t s);
// flag[i] <- exclude && distance(p_i, p_i) < r in the metric's arithmetic (cnorm: the rows' Cosine norms, NULL for
// Euclidean); cnt[i] <- in_off[i + 1] - in_off[i] - flag[i]; *bad += flagged rows with an empty list (never, see the kernel)
template <typename T>
hipError_t launch_radius_self_counts(const T *P, size_t n, int dim, size_t ld, const T *cnorm, T r, bool exclude,
                                     const uint64_t *in_off, uint32_t *flag, uint32_t *cnt, uint32_t *bad,
                                     hipStream_t s, const T *radii = nullptr);
// out[1 + j] <- out[0] + part[j + 1], j < nq (a chunk's scan behind the rows before it)
hipError_t launch_radius_self_place(const uint64_t *part, size_t nq, uint64_t *out, hipStream_t s);
// out[out_off[i] + t] <- row i's list (in_off, ascending index, entries below in_cap) without self0 + i where flag[i],
// positions below cap only; out_dist / in_dist nullable together; *bad += flagged, wholly written lists without it
template <typename T>
hipError_t launch_radius_self_compact(const uint64_t *in_off, const uint64_t *in_idx, const T *in_dist, uint64_t in_cap,
                                      const uint32_t *flag, const uint64_t *out_off, size_t n, uint64_t self0,
                                      uint64_t *out_idx, T *out_dist, uint64_t cap, uint32_t *bad, hipStream_t s);

// ---- components.hip: DBSCAN over the radius self-lists (pn_dbscan_*): lock-free union-find on the core rows
// core[i] <- off[i + 1] - off[i] >= min_samples; parent[i] <- i; side_len[i] <- core[i] ? 0 : the list's length
hipError_t launch_dbscan_init(const uint64_t *off, size_t n, uint64_t min_samples, uint8_t *core, uint32_t *parent,
                              uint32_t *side_len, hipStream_t s);
// a piece's lists (rows r0 .. r0 + nq, entries base + j, all of them below in_cap): core rows are united with the core rows
// of their lists, non-core rows copy theirs to side[side_off[row] ..], non-core entries as 0xFFFFFFFF
hipError_t launch_dbscan_union(const uint64_t *in_off, const uint64_t *in_idx, uint64_t in_cap, size_t nq, size_t r0,
                               size_t n, uint64_t base, const uint8_t *core, uint32_t *parent, const uint64_t *side_off,
                               uint32_t *side, hipStream_t s);
// root[i] <- find(i) (core rows, else 0xFFFFFFFF); is_root[i] <- root[i] == i
hipError_t launch_dbscan_flatten(uint32_t *parent, const uint8_t *core, size_t n, uint32_t *root, uint32_t *is_root,
                                 hipStream_t s);
// labels[i] <- num[root[i]] (core) | num[smallest root in the side list] (border) | -1; num = exclusive scan of is_root
hipError_t launch_dbscan_label(const uint32_t *root, const uint64_t *num, const uint8_t *core, const uint64_t *side_off,
                               const uint32_t *side, size_t n, int64_t *labels, hipStream_t s);
// labels <- -1, core (nullable) <- 0, *n_clusters (nullable) <- 0
hipError_t launch_dbscan_noise(size_t n, int64_t *labels, uint8_t *core, uint64_t *n_clusters, hipStream_t s);

// ---- exact_scan.hip, for mst.hip: the masked nearest-outside-row scan.  Listed row qsel[r] (r < nq) against rows
// [0, n) in nseg segments of seg_len rows (a multiple of kTileP): seg_key / seg_j [seg][round_up(nq, kTileQ)] <- the
// segment's least (key(max(d, core keys)), j) over rows j with comp[j] != comp[qsel[r]], or (kMax, 0xFFFFFFFF).
// comp / ckey: [n]; cnorm: the rows' Cosine norms, NULL for Euclidean (then the keys are the unsigned ones)
template <typename T>
hipError_t launch_mst_scan(const T *P, size_t n, int dim, size_t ldp, const uint32_t *qsel, int nq, size_t seg_len,
                           int nseg, const uint32_t *comp, const typename KeyOf<T>::type *ckey, const T *cnorm,
                           typename KeyOf<T>::type *seg_key, uint32_t *seg_j, hipStream_t s);

// ---- mst.hip: Boruvka under the strict edge order (pn_mst_*): bookkeeping kernels and the round loop
struct MstArgs {
    const void *P = nullptr;      // the index's rows [n_pad][ld] of T
    size_t n = 0, ld = 0;
    int dim = 0;
    const void *cnorm = nullptr;  // Cosine: the rows' norms (T); NULL: Euclidean
    const void *d_core = nullptr; // [n] of T in HBM, nullable (all zeros)
    // round 0 of the un-cored call, answered by the k-NN pipeline: every row's nearest other row (index_base added) and
    // its distance, [n] each; both NULL: round 0 is a full scan
    const uint64_t *nn_idx = nullptr;
    const void *nn_dist = nullptr;
    uint64_t index_base = 0;
    size_t batch = 0;             // listed rows per scan launch (>= 1)
    int n_cu = 256;
    void *buf = nullptr;          // mst_buffer_bytes() bytes of scratch
    uint64_t *d_src = nullptr, *d_dst = nullptr;  // [n - 1]
    void *d_weight = nullptr;     // [n - 1] of T
    uint64_t work[2] = {0, 0};    // out: rounds, rows scanned
};
size_t mst_buffer_bytes(size_t n, int elem_bytes, size_t batch, int n_cu);
// enqueues on s, blocks the host once per round; PN_OK or an error code with pn_last_error() set
template <typename T>
int mst_enqueue(MstArgs &a, hipStream_t s);

// ---- linkage.hip: the single-linkage dendrogram of sorted tree edges (pn_linkage_*) and HDBSCAN's extraction from it
// (pn_hdbscan_*); nothing in it waits for the device
struct LinkageArgs {
    size_t n = 0;
    uint64_t index_base = 0;
    const uint64_t *d_src = nullptr, *d_dst = nullptr;  // [n - 1], as pn_mst_* writes them
    const void *d_weight = nullptr;                     // [n - 1] of T
    void *buf = nullptr;                                // linkage_buffer_bytes() (or hdbscan_buffer_bytes()) of scratch
    // outputs [n - 1], all three or none; d_weight_out (of T) nullable or d_weight itself; d_err [1] nullable
    uint64_t *d_left = nullptr, *d_right = nullptr, *d_size = nullptr;
    void *d_weight_out = nullptr;
    int32_t *d_err = nullptr;
};
size_t linkage_buffer_bytes(size_t n);
template <typename T>
int linkage_enqueue(const LinkageArgs &a, hipStream_t s);
// the extraction reads the dendrogram that linkage_enqueue left at the head of the same buffer; n >= min_cluster_size
struct HdbscanArgs {
    size_t n = 0, min_cluster_size = 2;
    const void *d_weight = nullptr;  // [n - 1] of T: the merge weights
    void *buf = nullptr;             // hdbscan_buffer_bytes() of scratch
    int64_t *d_labels = nullptr;     // [n]
    void *d_prob = nullptr;          // [n] of T, nullable
    uint64_t *d_n_clusters = nullptr;  // [1], nullable
};
size_t hdbscan_buffer_bytes(size_t n);
template <typename T>
int hdbscan_extract_enqueue(const HdbscanArgs &a, hipStream_t s);
// out[i] = d[i][k - 1] of a [rows][k] matrix (the core distances out of a self-query's answer)
template <typename T>
hipError_t launch_last_column(const T *d, size_t rows, size_t k, T *out, hipStream_t s);

// ---- lof.hip: Local Outlier Factor over the self-k-NN graph (pn_lof_*, pn_lof_score_*); nothing in it waits for the device.
// pack: a self-query chunk's answer [nq][k] (ids with the index base) -> the store's rows: ids [nq][k] uint32 without the
// base, dist [nq][k], kdist [nq] = the last column
template <typename T>
hipError_t launch_lof_pack(const uint64_t *in_idx, const T *in_dist, size_t nq, int k, uint64_t index_base,
                           uint32_t *ids, T *dist, T *kdist, hipStream_t s);
// lrd [n] from the store and kdist [n]; lof [n] from the store's ids and lrd [n]
template <typename T>
hipError_t launch_lof_lrd(const uint32_t *ids, const T *dist, const T *kdist, size_t n, int k, double *lrd,
                          hipStream_t s);
hipError_t launch_lof_lof(const uint32_t *ids, const double *lrd, size_t n, int k, double *lof, hipStream_t s);
// score [nq] of queries from their k-NN answer [nq][k] (ids with the index base) and the fit's lrd [n], kdist [n]
template <typename T>
hipError_t launch_lof_score(const uint64_t *q_idx, const T *q_dist, size_t nq, int k, uint64_t index_base, size_t n,
                            const double *lrd, const T *kdist, double *score, hipStream_t s);

// ---- knn_predict.hip: the vote and the weighted mean over the k-NN lists (pn_knn_classify_*, pn_knn_regress_*); nothing
// in it waits for the device.  q_idx / q_dist: a chunk's k-NN answer [nq][k] (ids with the index base), 1 <= k <= 1024;
// flags: PN_KNN_WEIGHT_DISTANCE or 0.
// pred [nq] (-1: a poisoned list) and, where proba is not NULL, proba [nq][n_classes] (zeroed here, on s) from labels [n]
template <typename T>
hipError_t launch_knn_vote(const uint64_t *q_idx, const T *q_dist, size_t nq, int k, uint64_t index_base, size_t n,
                           const int64_t *labels, size_t n_classes, unsigned flags, int64_t *pred, double *proba,
                           hipStream_t s);
// out [nq][n_out] from targets [n][n_out]
template <typename T>
hipError_t launch_knn_mean(const uint64_t *q_idx, const T *q_dist, size_t nq, int k, uint64_t index_base, size_t n,
                           const double *targets, size_t n_out, unsigned flags, double *out, hipStream_t s);

// ---- kde.hip: kernel density sums over the radius lists (pn_kde_*); nothing in it waits for the device.
// hq [nq] <- h broadcast (n_h = 1) or copied (n_h = nq); cut [nq] <- the cutoffs.  mode 0: cut = h; 1: the smallest T >=
// (double)h * f; 2: 0; 3: +inf; a bandwidth that is not positive is its own cutoff in every mode
template <typename T>
hipError_t launch_kde_cutoff(const T *h, size_t n_h, size_t nq, int mode, double f, T *hq, T *cut, hipStream_t s);
// count[q] = off[q + 1] - off[q]
hipError_t launch_kde_counts(const uint64_t *off, size_t nq, uint64_t *count, hipStream_t s);
// sum [nq] (and count [nq], nullable) of a piece's lists (piece-local offsets off, 64-bit ids with the index base,
// distances) with the bandwidths hq [nq]; own_first != ~0: query q is row id own_first + q and its own entry is left out
template <typename T>
hipError_t launch_kde_sum(const uint64_t *off, const uint64_t *idx, const T *dist, const T *hq, size_t nq, int kernel,
                          uint64_t own_first, double *sum, uint64_t *count, hipStream_t s);

// ---- mean_shift.hip: mean shift over the radius lists (pn_mean_shift_*); nothing in it waits for the device.
// the start of a call: pos [ns][dim] dense <- the seeds' rows (row stride s_stride), hq [ns] <- h broadcast (n_h = 1) or
// copied, slot[i] <- i
template <typename T>
hipError_t launch_ms_init(const T *seeds, size_t s_stride, size_t ns, int dim, const T *h, size_t n_h, T *pos, T *hq,
                          uint32_t *slot, hipStream_t s);
// One step of a piece's nq active seeds (one wave each).  off / idx: the piece's CSR as radius_device_enqueue writes it
// without distances (piece-local offsets, 64-bit row ids with index_base); X [n][ld]: the indexed rows (ld a multiple of
// kRowAlign); pos [nq][dim] dense: read, and overwritten with the new positions; slot [nq]: each seed's output row.
// iter: the iteration's number t >= 1; last: t == max_iter.  keep[q] <- 0 where the seed stopped (shift <= tol, last, or
// an empty list: dead), else 1; a stopped seed's mode [dim], points_within, iterations (nullable) and shift (nullable) go
// to its slot of the outputs.
template <typename T>
struct MsStep {
    const uint64_t *off, *idx;
    uint64_t index_base;
    const T *X;
    size_t ld;
    int dim;
    T *pos;
    const uint32_t *slot;
    size_t nq;
    double tol;
    uint32_t iter;
    int last;
    uint32_t *keep;
    T *modes;
    uint64_t *points;
    uint32_t *iters;
    double *shift;
};
template <typename T>
hipError_t launch_ms_step(const MsStep<T> &a, hipStream_t s);
// a piece whose lists are all empty (no CSR exists): every seed of it stops dead (the fields off, idx, X are not read)
template <typename T>
hipError_t launch_ms_dead(const MsStep<T> &a, hipStream_t s);
// the next iteration's active set: row i < *nsel of the outputs <- row sel[i] of the inputs (grid sized for n_in)
template <typename T>
hipError_t launch_ms_gather(const uint32_t *sel, const uint32_t *nsel, size_t n_in, int dim, const T *pos_in, const T *h_in,
                            const uint32_t *slot_in, T *pos_out, T *h_out, uint32_t *slot_out, hipStream_t s);
// The merge of the converged modes (the contract: petal_mi355x.h).  buf: ms_merge_bytes(ns) bytes of scratch, 8-byte
// aligned.  Enqueues the rank sort and 2 ceil(ns / kMsMergeRound) round launches; nothing is read back.
constexpr int kMsMergeRound = 1024;  // consecutive ranks one round of the merge decides
size_t ms_merge_bytes(size_t ns);
template <typename T>
hipError_t ms_merge_enqueue(const T *modes, size_t ns, int dim, const uint64_t *points, T h, void *buf, T *centres,
                            uint64_t *centre_points, int64_t *centre_of_seed, uint64_t *n_centres, hipStream_t s);
// labels[i] <- the centre nearest to row i of X by (distance key, centre number): a k = 1 query's answer on an index made
// of the centres; orphans: -1 unless that distance is < h; nc == 0: all -1
template <typename T>
hipError_t launch_ms_labels(const T *X, size_t n, size_t ld, int dim, const T *centres, size_t nc, T h, bool orphans,
                            int64_t *labels, hipStream_t s);

// ---- kmeans.hip: k-means (pn_kmeans_*, pn_kmeans_assign_*); nothing in it waits for the device.
// The filter takes 8 <= dim <= 320 (km_filter_supported); its tiles (the test suite
// asks for them): 128 rows per workgroup (64 beyond 256 padded columns), 32 centres per MFMA tile.
bool km_filter_supported(int dim);
int km_row_tile();
int km_centre_tile();
// the packed operands, carved from one 16-byte aligned buffer each (km_*_image_bytes, km_*_image_at)
struct KmRowImage {
    uint16_t *img = nullptr, *lo = nullptr;  // [n_img][dp] bf16 bits each (x^ and x~), rows at and beyond n zero
    double *xn = nullptr;     // [n] |x|^2 rounded down; NaN: the row is flagged (not finite, or a norm beyond 2^100)
    float *xh = nullptr, *xl = nullptr, *xe = nullptr;  // [n] upper bounds of |x^|, |x~| and |e_x|
    size_t n_img = 0;         // n rounded up to the row tile
    int dp = 0;               // dim rounded up to 16
};
struct KmCentreImage {
    uint16_t *img = nullptr, *lo = nullptr;  // [nc_pad][dp] each
    float *cn = nullptr;      // [nc_pad] |c|^2 rounded down, +inf for the padding
    unsigned long long *cc = nullptr;  // [8]: the bits of Ce, B, Ch, Cl (kmeans.hip), then the "a centre is flagged" word
    size_t nc_pad = 0;
};
size_t km_row_image_bytes(size_t n, int dim);
size_t km_centre_image_bytes(size_t nc, int dim);
KmRowImage km_row_image_at(void *buf, size_t n, int dim);
KmCentreImage km_centre_image_at(void *buf, size_t nc, int dim);
template <typename T>
hipError_t launch_km_pack_rows(const T *X, size_t n, size_t ld, int dim, const KmRowImage &r, hipStream_t s);
template <typename T>
hipError_t launch_km_pack_centres(const T *centres, size_t nc, int dim, const KmCentreImage &c, hipStream_t s);
// cand [n] <- the centre of each row's smallest key, tau [n] <- the second smallest key (+inf: there is none)
hipError_t launch_km_filter(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, uint32_t *cand, float *tau,
                            hipStream_t s);
// diagnostic: bounds[i * nc + c] <- L(x_i, c)
hipError_t launch_km_bounds(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, double *bounds, hipStream_t s);
// the candidates in the reference's fold; proven rows get their label and distance (dist nullable), the others are listed:
// sel[0 .. *nsel) in any order (nsel zeroed by the caller, sel [n])
template <typename T>
hipError_t launch_km_rerank(const T *X, size_t n, size_t ld, int dim, const T *centres, size_t nc, const uint32_t *cand,
                            const float *tau, const KmRowImage &r, const KmCentreImage &c, uint32_t *sel, uint32_t *nsel,
                            int64_t *labels, T *dist, hipStream_t s);
// every row (sel == nullptr) or the listed rows against every centre: launch_ms_labels' answer, and the distance
// (nullable); nc == 0: labels -1, distances NaN
template <typename T>
hipError_t launch_km_exact(const T *X, size_t n, size_t ld, int dim, const T *centres, size_t nc, const uint32_t *sel,
                           const uint32_t *nsel, int64_t *labels, T *dist, hipStream_t s);
// *out <- SUM4096 of (double)dist[i]^2 (0 where labels[i] < 0); buf: km_inertia_bytes(n)
size_t km_inertia_bytes(size_t n);
template <typename T>
hipError_t launch_km_inertia(const int64_t *labels, const T *dist, size_t n, void *buf, double *out, hipStream_t s);
// The members' lists of labels [n] (one sort), counts [nc] (nullable) and, with centres != nullptr, one update of the
// centres [nc][dim] in place; *stop_out <- where the 16 bytes {shift2, stop word = shift2 <= tol || last} will be (in
// buf: km_update_bytes(n, nc, dim), 8-byte aligned).  n, nc >= 1.
size_t km_update_bytes(size_t n, size_t nc, int dim);
template <typename T>
hipError_t km_update_enqueue(const T *X, size_t n, size_t ld, int dim, const int64_t *labels, size_t nc, void *buf,
                             T *centres, uint64_t *counts, double tol, int last, double **stop_out, hipStream_t s);

// ---- mst.hip, for mean_shift.hip and kmeans.hip: the bitonic network over (key, pair), ascending by key then pair.  N =
// sort_key_pair_len(count): count padded to a power of two, at least the block one workgroup sorts in LDS; the caller pads
// the arrays (all-ones keys sort last)
size_t sort_key_pair_len(size_t count);
hipError_t launch_sort_key_pair_u64(uint64_t *key, unsigned long long *pair, size_t N, hipStream_t s);

// ---- optics.hip: OPTICS over the max_eps self-graph (pn_optics_*) and the extraction at one eps (pn_optics_dbscan_*);
// nothing in it waits for the device.
// core[i] <- v < max_eps ? v : +inf, v = in_dist[i][k - 1] of a self-query chunk's answer [nq][k] (in_dist == nullptr: +inf);
// radii[i] <- max_eps where core[i] is finite, else 0 (the row's list stays empty)
template <typename T>
hipError_t launch_optics_core(const T *in_dist, size_t nq, size_t k, T max_eps, T *core, T *radii, hipStream_t s);
// a fill piece's lists (rows [row0, row0 + rows), piece-local offsets in_off, 64-bit ids with the index base, the rows
// themselves among them; entries below in_cap are there) -> the graph store at the final offsets off[row0 ..]: uint32 ids
// without the base, the row itself dropped
template <typename T>
hipError_t launch_optics_repack(const uint64_t *in_off, const uint64_t *in_idx, const T *in_dist, uint64_t in_cap,
                                size_t rows, size_t row0, uint64_t index_base, const uint64_t *off, uint32_t *ids,
                                T *dist, hipStream_t s);
// the ordering: one workgroup runs the n steps.  tree: optics_tree_bytes(n, sizeof T) bytes, 16-byte aligned; pred nullable
size_t optics_tree_bytes(size_t n, int elem_bytes);
template <typename T>
hipError_t launch_optics_order(size_t n, const uint64_t *off, const uint32_t *ids, const T *dist, uint64_t n_entries,
                               const T *core, void *tree, uint64_t *ordering, T *reach, int64_t *pred, hipStream_t s);
// labels of the DBSCAN clustering at eps from an ordering; buf: optics_extract_bytes(n) bytes; n_clusters, d_error nullable
// (*d_error <- PN_OK, or PN_ERR_INVALID when ordering is no permutation of 0 .. n - 1: the labels are then unspecified)
size_t optics_extract_bytes(size_t n);
template <typename T>
hipError_t launch_optics_extract(const uint64_t *ordering, const T *reach, const T *core, size_t n, T eps, void *buf,
                                 int64_t *labels, uint64_t *n_clusters, int32_t *d_error, hipStream_t s);

// ---- csr_sort.hip: order every list of a radius answer by (distance, index) in place (PN_RADIUS_SORTED)
constexpr int kSortTile = 2048;  // longest list sorted by one workgroup in LDS; longer lists: chunks + merge passes
struct CsrSortScratch {
    uint32_t *nch = nullptr;        // [nq] chunks per long list
    uint64_t *chunk_off = nullptr;  // [nq + 1] their exclusive scan
    uint64_t *scan = nullptr;       // (nq / 4096 + 2) words of scan scratch
    uint64_t *idx = nullptr;        // ping-pong copy: csr_sort_scratch_entries() entries
    void *dist = nullptr;
};
// entries of the ping-pong copy a call needs (0: no list can exceed kSortTile entries); max_row bounds every list's
// length (the corpus' rows), limit the positions sorted (lists that do not end at or below it are left unsorted)
size_t csr_sort_scratch_entries(size_t nq, size_t max_row, size_t limit);
template <typename T>
hipError_t launch_csr_sort(const uint64_t *offsets, int nq, uint64_t *idx, T *dist, uint64_t limit, size_t max_row,
                           const CsrSortScratch &w, int n_cu, hipStream_t s);
// Cosine's norms: norms[i] = sqrt(sequential sum of x_i[k]^2, k < dim) in T
template <typename T>
hipError_t launch_cosine_norms(const T *X, size_t n, int dim, size_t ld, T *norms, hipStream_t s);
template <typename T>
hipError_t launch_exact_pairwise(const T *X, size_t n, int dim, size_t ld, T *out, hipStream_t s);
// distance::pairwise under the Cosine metric; norms: n elements of scratch
template <typename T>
hipError_t launch_cosine_pairwise(const T *X, size_t n, int dim, size_t ld, T *norms, T *out, hipStream_t s);

// ---- select.hip
// Exact mode: keys are exact distance keys; picks the kout smallest (key, idx).
// writes results r < kout of query q at [q * out_stride + out_off + r]; when lo_key != nullptr also
// records the last (key, row) written per query as the next round's lower bound
// osel (nullable): the results of query q go to output row osel[nq_off + q] instead of row q (scatter in place)
template <typename T>
hipError_t launch_select_exact(const CandBuf &cb, int nq, int kout, uint64_t index_base, uint64_t *idx_out, T *dist_out,
                               size_t out_stride, size_t out_off, void *lo_key, uint32_t *lo_idx, const uint32_t *nq_dev,
                               uint32_t nq_off, bool signed_keys, hipStream_t s, const uint32_t *osel = nullptr);
template <typename T>
hipError_t launch_select_exact_groups(const CandBuf &cb, int groups, int kp, int nq, int kout, uint64_t index_base,
                                      uint64_t *idx_out, T *dist_out, size_t out_group_stride, const uint32_t *nq_dev,
                                      uint32_t nq_off, hipStream_t s, bool signed_keys = false);
// MFMA mode: keys are f32 lower bounds L; recomputes every candidate's distance
// in the reference's operation order, selects, and verifies the filter's
// exclusions (flags[q] = 1 -> the query must be re-run exactly).
// qn / qbad (nullable, [nq]): the thresholds bound |q-p|^2 - |q|^2 (bf16 filter), qn[q] <= |q|^2 is added back;
// qbad[q] != 0 flags the query outright
// results of query q go to idx_out/dist_out[q * out_stride + r]; n_flagged: per-call count of flagged queries (device,
// zeroed by the caller); sel (nullable, [nq]): the flagged queries are LISTED here as they are found (sel[0 ..
// *n_flagged), any order) -- the second tier's work list, no listing launch; stats (nullable): the index's running
// device counters, kPnStatWords words: [0] fallback queries, then kPnStatSlots pairs {candidates, exact evaluations}
// that the queries add to by q mod kPnStatSlots (10^4 waves adding to ONE address cost as much as the whole kernel)
constexpr int kPnStatSlots = 64, kPnStatWords = 4 + 2 * kPnStatSlots;
template <typename T>
hipError_t launch_select_rerank(const CandBuf &cb, const T *P, size_t n, int dim, size_t ldp, const T *Q, int nq, size_t ldq,
                                int kout, uint64_t index_base, uint64_t *idx_out, T *dist_out, size_t out_stride,
                                uint32_t *flags, uint32_t *n_flagged, const double *qn, const uint32_t *qbad, uint32_t *sel,
                                unsigned long long *stats, hipStream_t s, int first_eval = 0, int cell_max = 0,
                                const T *cnorm = nullptr, const T *qnorm = nullptr);
// first_eval: candidates (smallest bounds first) evaluated in the first round, >= kout (0: kout); cell_max: entries a
// (segment, query) cell holds at most (0: cb.cap) -- sizes the kernel's LDS
// The re-rank kernel's dynamic LDS: 12 (f32) or 16 (f64) bytes per entry the nseg cells of a query can hold + the query
// row.  The launchers refuse a launch above kSelectRerankLdsMax; a planner asks THIS function before it picks a tier, so
// that what it admits is what the launcher takes.
constexpr size_t kSelectRerankLdsMax = 64 * 1024;
inline size_t select_rerank_lds_bytes(int nseg, int cap, int cell_max, size_t dim, size_t elem_bytes) {
    const size_t per_cell = cell_max > 0 && cell_max < cap ? (size_t)cell_max : (size_t)cap;
    return (size_t)nseg * per_cell * (elem_bytes + 8) + (dim + 8) * elem_bytes;
}
// f64 indexes (behind the bf16 filter only: qn required): distances in the reference's f64 fold, proof with u = 2^-53
// cnorm / qnorm (nullable, together): a Cosine index behind the bf16 filter (select.hip, cos_proof_lb) -- the rows' [n] /
// queries' [nq] norms in the index's type (cosine_norms_kernel), candidates evaluated by Cosine::distance,
// order-preserving keys of ALL floats
// osel (nullable): the merged result of query q goes to row osel[q] of the outputs (row stride out_stride, 0 = k_out);
// host_count (nullable, mapped pinned memory): block 0 copies *nq_dev there (the count a LATER call looks at)
// Small corpora, a few queries per call: the whole call in one launch (one wave per query over all rows); Q and the
// outputs may be mapped pinned host memory.  radius_mode: out row q = {count, rows ascending ...} (out_stride >= n + 1),
// dist_out (nullable) row q = {-, their distances ...} at the same positions
size_t tiny_query_lds_bytes(size_t n, int dim_eff, int elem_bytes);  // must be <= 64 KiB
template <typename T>
hipError_t launch_tiny_query(const T *P, size_t n, int dim_eff, size_t ldp, const T *Q, size_t ldq, int nq, int kout,
                             bool radius_mode, T radius, uint64_t index_base, uint64_t *idx_out, T *dist_out,
                             size_t out_stride, hipStream_t s);
template <typename T>
hipError_t launch_merge_topk(const uint64_t *idx_parts, const T *dist_parts, int n_parts, size_t idx_part_stride,
                             size_t dist_part_stride, int nq, int k_part, int k_out, uint64_t *idx_out, T *dist_out,
                             hipStream_t s, const uint32_t *nq_dev = nullptr, const uint32_t *osel = nullptr,
                             size_t out_stride = 0, uint32_t *host_count = nullptr, bool signed_keys = false);
// gather rows sel[off + i] of src into dst row i / scatter result rows i back to query sel[off + i], for
// i < min(max_rows, *nsel - off): the count stays on the device
template <typename T>  // T = float | double (explicitly instantiated)
hipError_t launch_gather_rows(const T *src, size_t ld, const uint32_t *sel, const uint32_t *nsel, uint32_t off,
                              uint32_t max_rows, T *dst, hipStream_t s);
template <typename T>
hipError_t launch_radius_check(const uint32_t *rcnt, const uint32_t *ridx, size_t nq_pad, int nseg, uint32_t cap,
                               const T *P, size_t ldp, const T *Q, int nq, int dim, T r, uint32_t *kept,
                               uint32_t *nkept, uint32_t *overflow, int ridx_stride, uint32_t *over_q, hipStream_t s,
                               const T *cnorm = nullptr, const T *qnorm = nullptr,  // (both: Cosine::distance < r)
                               T *kept_dist = nullptr,  // (nullable: [2][nq][nseg * cap], the second half gets
                                                        // the kept rows' distances next to `kept`)
                               const T *radii = nullptr);  // (nullable, [nq]: query q is compared with radii[q], not r)
hipError_t launch_gather_rows_f32(const float *src, size_t ld, const uint32_t *sel, const uint32_t *nsel, uint32_t off,
                                  uint32_t max_rows, float *dst, hipStream_t s);
hipError_t launch_scatter_results_f32(const uint64_t *idx_in, const float *dist_in, const uint32_t *sel,
                                      const uint32_t *nsel, uint32_t off, uint32_t max_rows, int kout, uint64_t *idx_out,
                                      float *dist_out, size_t out_stride, hipStream_t s);
hipError_t launch_compact_flags(const uint32_t *flags, int nq, uint32_t *sel, uint32_t *nsel, hipStream_t s);

// ---- pack.hip
// dst[r][c] = (r < n && c < cols) ? src[r*row_stride + c] : 0  for r < n_pad, c < ld
template <typename T>
hipError_t launch_pack_rows(const T *src, size_t n, size_t cols, size_t row_stride, T *dst, size_t n_pad, size_t ld,
                            hipStream_t s);
hipError_t launch_fill_uniform_f32(float *out, uint64_t count, uint64_t seed, uint64_t first, hipStream_t s);
// scaled squared row norms for the MFMA lower bound (see mfma_filter_v2.hip)
hipError_t launch_row_norms_f32(const float *X, size_t n_pad, size_t n, int dim, size_t ld, float alpha,
                                float *norm_out, uint32_t *nonfinite_flag, hipStream_t s);

// ---- mfma_filter_v2.hip (the f32 MFMA tier; round 4: the first structure, a (query tile x segment) grid in
// mfma_filter.hip, is retired -- nothing selected it but PN_OPT_MFMA_STRUCTURE = 1)
bool mfma_supported(int dim, size_t ld);
// persistent balanced partition, k' <= 32 with LDS buffers / k' <= 224 with HBM buffers
int mfma_v2_max_segments(size_t q_tiles, int n_wg);
// gcand != nullptr: candidate buffers in HBM (mfma_v2_gcand_bytes(n_wg) bytes), 2 workgroups per CU
size_t mfma_v2_gcand_bytes(int n_wg, int kp);
int mfma_v2_cap_for(int kp);
hipError_t launch_mfma_filter_v2_f32(const float *P, const float *pnorm, size_t n, size_t ldp, const float *Q,
                                     const float *qnorm, size_t ldq, int kp, const CandBuf &cb, int n_wg,
                                     uint32_t *gcand, hipStream_t s);

// radius filter (mfma_filter_v2.hip) + exact check / ascending-row ordering of its survivors (select.hip)
hipError_t launch_mfma_radius_f32(const float *P, const float *pnorm, size_t n, size_t ldp, const float *Q,
                                  const float *qnorm, size_t nq_pad, float tau_excl, uint32_t cap, uint32_t *rcnt,
                                  uint32_t *ridx, int n_wg, hipStream_t s);
// per query: exact distance of every listed row, keep dist < r, order by row; kept[q][*], nkept[q]; *overflow += 1
// when some list of the query exceeded `cap`
// ridx_stride: element stride of the row lists (2 when they are the rows of (key, row) pairs)
hipError_t launch_radius_check_f32(const uint32_t *rcnt, const uint32_t *ridx, size_t nq_pad, int nseg, uint32_t cap,
                                   const float *P, size_t ldp, const float *Q, int nq, int dim, float r,
                                   uint32_t *kept, uint32_t *nkept, uint32_t *overflow, int ridx_stride,
                                   uint32_t *over_q /* nullable: per-query overflow flags */, hipStream_t s,
                                   float *kept_dist = nullptr);
hipError_t launch_radius_gather(const uint32_t *kept, const uint32_t *nkept, const uint64_t *offsets, int nq,
                                size_t kept_stride, uint64_t index_base, uint64_t *out, hipStream_t s,
                                const void *kept_dist = nullptr, void *out_dist = nullptr, int dist_bytes = 0);

// ---- bf16_filter.hip: first-tier filter (bf16 MFMA lower bound of |q-p|^2 - |q|^2), D <= 128
bool bf16_supported(int dim);
bool bf16_is_wide(int dim);  // 128 < D: K-chunked kernel (launch_bf16_wide_filter), images in the chunked layout
// ci: the "norm in the accumulator" layout (bf16_filter.hip, bf16_ci_dim): no extra columns, row norms as the
// chain's initial value, the error products as a per-query constant folded into qn
int bf16_ks_for(int dim, bool ci);
bool bf16_ci_candidate(int dim);
size_t bf16_image_bytes(size_t n, int dim, bool ci);        // corpus tile images
size_t bf16_query_bytes(size_t nq_pad, int dim, bool ci);   // packed query rows
int bf16_cap_for(int kp);                          // slots per (segment, query): 64 / 128 / 256
int bf16_query_tile();                             // queries per workgroup (256)
// mu: translation vector [dim]; sums: [dim + 1] per-dimension f64 sums of the corpus + the sum of all squares
// (zeroed by the caller)
template <typename T>  // T = float | double (explicitly instantiated): the index's element type
hipError_t launch_bf16_column_sums(const T *P, size_t n, int dim, size_t ld, double *sums, hipStream_t s);
// out[0] <- the largest |delivered - exact| / (2^-13 sum|terms|) over synthetic chains of 8 and 65 MFMA steps: the matrix
// core's accumulation error against the allowance the bf16 bound makes for it (bf16_filter.hip, bf16_selftest_kernel)
hipError_t launch_bf16_selftest(float *out, hipStream_t s);
// mu [dim] <- the per-dimension mean (f32) when translating by it shrinks the sum of squared norms 16x (wide rows: 2x), else
// zero; words[0] <- 1 / 0 accordingly.  never: always zero (no caller asks for it)
hipError_t launch_bf16_decide_mu(const double *sums, size_t n, int dim, bool never, float *mu, uint32_t *words, hipStream_t s);
// out4 (zeroed by the caller): max Bp, max Dp, sum Bp, sum Dp over the rows
template <typename T>
hipError_t launch_bf16_row_stats(const T *P, const float *mu, size_t n, int dim, size_t ld, double *out4,
                                 hipStream_t s);
// Cosine indexes: rows normalised in f64 (bf16_filter.hip, cos_normalize_rows_kernel); out [n_out][ld_out], rows >= n_valid
// zero; a row with a squared norm outside [2^-100, 2^100] raises *bad, or (nan_rows) becomes NaNs
template <typename T>
hipError_t launch_cos_normalize_rows(const T *X, size_t n_valid, size_t n_out, int dim, size_t ld_in, double *out,
                                     size_t ld_out, uint32_t *bad, bool nan_rows, hipStream_t s);
template <typename T>
hipError_t launch_bf16_pack_corpus(const T *P, const float *mu, size_t n, int dim, size_t ld, void *img,
                                   uint32_t *bad, bool ci, hipStream_t s);
// Qp / ldq / misc (nullable, narrow rows only: bf16_pack_fused_supported): Q is the CALLER's array (row stride ld); the
// kernel also writes the zero-padded f32 copy Qp[nq_pad][ldq] and zeroes the 16 counter words at misc -- the three
// launches at the head of a call in one
bool bf16_pack_fused_supported(int dim);
// Seed model of an index (round 4; index.hip, seed_model_build): starting thresholds of a k-NN call from per-dimension
// moments of the corpus instead of a scout launch.  m1 / a / b: [dim] f32 (M1_k, 4 (M2_k - M1_k^2), 4 (M3_k - M2_k M1_k)
// of u = p - mu), c0 = sum M2_k, v0 = sum (M4_k - M2_k^2), z = the calibrated number of standard deviations below the mean;
// seed_out [nq_pad] receives the sortable keys (nullptr: no seeds).
struct Bf16SeedModel {
    const float *m1 = nullptr, *a = nullptr, *b = nullptr;
    double c0 = 0.0, v0 = 0.0, z = 0.0;
    uint32_t *seed_out = nullptr;
};
template <typename T>
hipError_t launch_bf16_pack_queries(const T *Q, const float *mu, size_t nq, size_t nq_pad, int dim, size_t ld,
                                    void *B, double *qn, uint32_t *qbad, bool ci, double bmax, double dmax,
                                    hipStream_t s, T *Qp = nullptr, size_t ldq = 0, uint32_t *misc = nullptr,
                                    const Bf16SeedModel *sm = nullptr);
// out[j * dim + k] += sum over rows of (p_k - mu_k)^(j + 1), j = 0 .. 3 (zeroed by the caller)
template <typename T>
hipError_t launch_bf16_column_moments(const T *P, const float *mu, size_t n, int dim, size_t ld, double *out, hipStream_t s);
// One launch of the first tier.  grid: bf16_grid of (n, cb.nq_pad, n_wg, split) -- cb.nseg >= grid.nseg, and cells without
// a writer must read "empty" (cnt 0, tau +inf, lists +inf) unless grid.aligned; cb.cnt / cb.tau as the pass needs them.
// scout_tiles: ScoutOnly -- the tiles of a run that are scouted; SelfScout -- the cap on the tiles a run contracts
// first, without buffers, to seed its threshold (0 = none).  Wide rows: in 256-row tiles.
// tau ([nq_pad] sortable keys; Seeded, Radius): starting / fixed thresholds.  scout_out (ScoutOnly): every run leaves
// its lanes' smallest block minima in scout_out[cell][2][bf16_scout_list()] (pre-filled with +inf unless aligned).
// Seed in the kernel (narrow rows, <= 32 segments, bf16_seed_in_kernel): the main launch derives its starting
// thresholds itself from the scout launch's `lists` (rank-th smallest of a query's union, `nq` real queries) -- no
// bf16_seed_kernel launch between; the scout launch of a plan with refreshers is given it too and sets `words`
// ([nq_pad], the words the refreshers lower) to +inf.
struct Bf16SeedLists {
    const float *lists;
    uint32_t rank, nq;
    uint32_t *words;
};
// Shared thresholds (Seeded pass of an aligned plan, 64- / 128-slot buffers): n_refresh extra "refresher" workgroups merge
// what the segments of a query hold and lower the query's word in tau while the pass runs (bf16_filter.hip, "Shared
// thresholds").  pcnt: [nseg][nq_pad] words (zeroed whenever the geometry changes), done: one word, ZEROED before the
// launch; epoch 1 .. 4095, different from the previous launch on pcnt; rank: r-th smallest.
struct Bf16Refresh {
    uint32_t *pcnt, *done;
    uint32_t epoch, rank;
    int n_refresh;
};
struct Bf16Launch {
    const void *img;  // corpus tile images of n rows of dim columns; ci: the layout (narrow rows)
    size_t n;
    int dim;
    bool ci;
    const void *B;    // packed queries
    int kp;
    CandBuf cb;
    Bf16Grid grid;
    Bf16Pass pass;
    Bf16Kernel kernel;  // what bf16_main_kernel chose (narrow rows) or Wide: the launcher checks that it may run, no more
    int scout_tiles = 0;
    const uint32_t *tau = nullptr;
    float *scout_out = nullptr;
    std::optional<Bf16SeedLists> seed;
    std::optional<Bf16Refresh> refresh;
};
bool bf16_seed_in_kernel(int nseg);
bool bf16_shared_supported(int cap);
hipError_t launch_bf16_filter(const Bf16Launch &l, hipStream_t s);
// wide rows: grid.n_wg persistent workgroups (one per CU) over equal slices of the (query tile, row tile) list
hipError_t launch_bf16_wide_filter(const Bf16Launch &l, hipStream_t s);
int bf16_scout_list();
int bf16_cell_max(int kp, int cap, int nseg, bool wide);  // entries a cell holds at most after a k-NN launch = CandBuf::final_keep to launch with
// out[q] = key just above the rank-th smallest value over the lists of q's nseg cells
// nq (0: nq_pad): the queries beyond it are padding and get the threshold -inf
hipError_t launch_bf16_seed(const float *lists, size_t nq_pad, int nseg, int rank, uint32_t *out, hipStream_t s,
                            size_t nq = 0);
hipError_t launch_bf16_radius_tau(const double *qn, size_t nq_pad, double tau_r, uint32_t *out, hipStream_t s);

// ---- radii_tau.hip: launch_bf16_radius_tau for one radius per query (pn_query_radii_*).  radii [nq] in the index's
// type T; out[q] = the threshold key launch_bf16_radius_tau gives for tau_r(radii[q]) (the three formulas of
// radius_bf16_enqueue, evaluated per query in f64); a query whose radius the filter cannot serve (not finite positive,
// Cosine r >= 1, tau_r >= 1e37) gets the key of -inf and qbad[q] = 1; q >= nq: -inf
template <typename T>
hipError_t launch_bf16_radii_tau(const double *qn, const T *radii, size_t nq, size_t nq_pad, int dim, bool cosine,
                                 uint32_t *out, uint32_t *qbad, hipStream_t s);
// stats[0] += *nsel (one thread; the listed queries of a pn_query_radii_* call into pn_stats.fallback_queries)
hipError_t launch_radii_add_listed(const uint32_t *nsel, unsigned long long *stats, hipStream_t s);
// diagnostic: out[q][row] = L'(q, row), q < nq, row < n_rows
hipError_t launch_bf16_bound(const void *img, const void *B, size_t n_rows, size_t nq, int dim, float *out, bool ci,
                             hipStream_t s);

}  // namespace pn

#include "host_tree.h"  // tree.cpp: the reference's ball tree, built on the host only when its introspection API is used

// ---- index.hip, for the other translation units
struct pn_index;
namespace pn {
int set_error(int code, const char *fmt, ...);
int query_device_strided_f32(const pn_index *ix, const float *d_q, size_t nq, size_t q_cols, size_t q_stride, size_t k,
                             uint64_t *d_idx, float *d_dist, size_t out_stride, hipStream_t s);
int query_device_strided_f64(const pn_index *ix, const double *d_q, size_t nq, size_t q_cols, size_t q_stride, size_t k,
                             uint64_t *d_idx, double *d_dist, size_t out_stride, hipStream_t s);
// the index's rows in HBM as the queries of its self-queries read them: [n][*ld] of its element type (sharded.hip)
const void *index_rows(const pn_index *ix, size_t *ld);
int merge_topk_device_keys_f32(const uint64_t *pi, const float *pd, size_t np, size_t is, size_t ds, size_t nq, size_t kp,
                               size_t ko, uint64_t *oi, float *od, int device, void *stream, bool signed_keys);
int merge_topk_device_keys_f64(const uint64_t *pi, const double *pd, size_t np, size_t is, size_t ds, size_t nq, size_t kp,
                               size_t ko, uint64_t *oi, double *od, int device, void *stream, bool signed_keys);
}  // namespace pn
