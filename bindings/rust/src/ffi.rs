//! UNVERIFIED SOURCE (no rustc in the build image).
//! What `bindgen` emits from `include/petal_mi355x.h` (ABI version 2), trimmed to what `lib.rs` calls.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_uint, c_void};

/// `flags` of the radius calls with distances: each list by (distance, index) ascending
pub const PN_RADIUS_SORTED: c_uint = 1;
pub const PN_SELF_INCLUDE: c_uint = 2;
/// `flags` of pn_mean_shift_*: the indexed rows are the seeds / of pn_mean_shift_labels_*: rows beyond h of every centre get -1
pub const PN_MS_SEED_ROWS: c_uint = 4;
pub const PN_MS_ORPHANS: c_uint = 8;
pub const PN_KNN_WEIGHT_DISTANCE: c_uint = 1;
/// `kernel` of the pn_kde_* calls
pub const PN_KDE_GAUSSIAN: c_int = 0;
pub const PN_KDE_TOPHAT: c_int = 1;
pub const PN_KDE_EPANECHNIKOV: c_int = 2;
pub const PN_KDE_EXPONENTIAL: c_int = 3;
pub const PN_KDE_LINEAR: c_int = 4;

#[repr(C)]
pub struct pn_index {
    _private: [u8; 0],
}
#[repr(C)]
pub struct pn_sharded {
    _private: [u8; 0],
}

pub const PN_OK: c_int = 0;
pub const PN_ERR_EMPTY: c_int = 1; // ArrayError::Empty          src/lib.rs:12
pub const PN_ERR_NOT_CONTIGUOUS: c_int = 2; // ArrayError::NotContiguous  src/lib.rs:14
pub const PN_ERR_COMM: c_int = 8;

extern "C" {
    pub fn pn_last_error() -> *const c_char;
    pub fn pn_index_destroy(index: *mut pn_index);
    pub fn pn_free(p: *mut c_void);

    pub fn pn_index_create_f32(points: *const f32, n_rows: usize, n_cols: usize, row_stride: isize, col_stride: isize,
                               device: c_int, out: *mut *mut pn_index) -> c_int;
    pub fn pn_index_create_f64(points: *const f64, n_rows: usize, n_cols: usize, row_stride: isize, col_stride: isize,
                               device: c_int, out: *mut *mut pn_index) -> c_int;
    pub fn pn_index_create_cosine_f32(points: *const f32, n_rows: usize, n_cols: usize, row_stride: isize,
                                      col_stride: isize, device: c_int, out: *mut *mut pn_index) -> c_int;
    pub fn pn_index_create_cosine_f64(points: *const f64, n_rows: usize, n_cols: usize, row_stride: isize,
                                      col_stride: isize, device: c_int, out: *mut *mut pn_index) -> c_int;

    pub fn pn_query_f32(index: *const pn_index, queries: *const f32, nq: usize, q_cols: usize, q_row_stride: isize,
                        k: usize, idx_out: *mut u64, dist_out: *mut f32) -> c_int;
    pub fn pn_query_f64(index: *const pn_index, queries: *const f64, nq: usize, q_cols: usize, q_row_stride: isize,
                        k: usize, idx_out: *mut u64, dist_out: *mut f64) -> c_int;
    pub fn pn_query_radius_f32(index: *const pn_index, queries: *const f32, nq: usize, q_cols: usize,
                               q_row_stride: isize, radius: f32, offsets: *mut u64, idx_out: *mut *mut u64) -> c_int;
    pub fn pn_query_radius_f64(index: *const pn_index, queries: *const f64, nq: usize, q_cols: usize,
                               q_row_stride: isize, radius: f64, offsets: *mut u64, idx_out: *mut *mut u64) -> c_int;
    /// flags: 0 = ascending index, PN_RADIUS_SORTED = by (distance, index); *dist_out released with pn_free
    pub fn pn_query_radius_with_distance_f32(index: *const pn_index, queries: *const f32, nq: usize, q_cols: usize,
                                             q_row_stride: isize, radius: f32, flags: c_uint, offsets: *mut u64,
                                             idx_out: *mut *mut u64, dist_out: *mut *mut f32) -> c_int;
    pub fn pn_query_radius_with_distance_f64(index: *const pn_index, queries: *const f64, nq: usize, q_cols: usize,
                                             q_row_stride: isize, radius: f64, flags: c_uint, offsets: *mut u64,
                                             idx_out: *mut *mut u64, dist_out: *mut *mut f64) -> c_int;
    pub fn pn_query_radius_with_distance_device_f32(index: *const pn_index, d_queries: *const f32, nq: usize,
                                                    q_cols: usize, q_row_stride: usize, radius: f32, flags: c_uint,
                                                    d_offsets: *mut u64, d_idx: *mut u64, d_dist: *mut f32,
                                                    capacity: usize, d_total: *mut u64, stream: *mut c_void) -> c_int;
    pub fn pn_query_radius_with_distance_device_f64(index: *const pn_index, d_queries: *const f64, nq: usize,
                                                    q_cols: usize, q_row_stride: usize, radius: f64, flags: c_uint,
                                                    d_offsets: *mut u64, d_idx: *mut u64, d_dist: *mut f64,
                                                    capacity: usize, d_total: *mut u64, stream: *mut c_void) -> c_int;
    pub fn pn_sharded_query_radius_with_distance_f32(sharded: *const pn_sharded, queries: *const f32, nq: usize,
                                                     q_cols: usize, q_row_stride: isize, radius: f32, flags: c_uint,
                                                     offsets: *mut u64, idx_out: *mut *mut u64,
                                                     dist_out: *mut *mut f32) -> c_int;
    pub fn pn_sharded_query_radius_with_distance_f64(sharded: *const pn_sharded, queries: *const f64, nq: usize,
                                                     q_cols: usize, q_row_stride: isize, radius: f64, flags: c_uint,
                                                     offsets: *mut u64, idx_out: *mut *mut u64,
                                                     dist_out: *mut *mut f64) -> c_int;
    pub fn pn_sharded_query_radius_with_distance_device_f32(sharded: *const pn_sharded, d_queries: *const f32, nq: usize,
                                                            q_cols: usize, q_row_stride: usize, radius: f32,
                                                            flags: c_uint, d_offsets: *mut u64, d_idx: *mut u64,
                                                            d_dist: *mut f32, capacity: usize, d_total: *mut u64,
                                                            stream: *mut c_void) -> c_int;
    pub fn pn_sharded_query_radius_with_distance_device_f64(sharded: *const pn_sharded, d_queries: *const f64, nq: usize,
                                                            q_cols: usize, q_row_stride: usize, radius: f64,
                                                            flags: c_uint, d_offsets: *mut u64, d_idx: *mut u64,
                                                            d_dist: *mut f64, capacity: usize, d_total: *mut u64,
                                                            stream: *mut c_void) -> c_int;
    /// self-queries over row shards: the local rows against the whole corpus (global rows), as pn_query_self_* /
    /// pn_query_radius_self_*; collective in rank mode
    pub fn pn_sharded_query_self_f32(sharded: *const pn_sharded, k: usize, flags: c_uint, idx_out: *mut u64,
                                     dist_out: *mut f32) -> c_int;
    pub fn pn_sharded_query_self_f64(sharded: *const pn_sharded, k: usize, flags: c_uint, idx_out: *mut u64,
                                     dist_out: *mut f64) -> c_int;
    pub fn pn_sharded_query_self_device_f32(sharded: *const pn_sharded, k: usize, flags: c_uint, d_idx: *mut u64,
                                            d_dist: *mut f32, stream: *mut c_void) -> c_int;
    pub fn pn_sharded_query_self_device_f64(sharded: *const pn_sharded, k: usize, flags: c_uint, d_idx: *mut u64,
                                            d_dist: *mut f64, stream: *mut c_void) -> c_int;
    pub fn pn_sharded_query_radius_self_f32(sharded: *const pn_sharded, radius: f32, flags: c_uint, offsets: *mut u64,
                                            idx_out: *mut *mut u64, dist_out: *mut *mut f32) -> c_int;
    pub fn pn_sharded_query_radius_self_f64(sharded: *const pn_sharded, radius: f64, flags: c_uint, offsets: *mut u64,
                                            idx_out: *mut *mut u64, dist_out: *mut *mut f64) -> c_int;
    pub fn pn_sharded_query_radius_self_device_f32(sharded: *const pn_sharded, radius: f32, flags: c_uint,
                                                   d_offsets: *mut u64, d_idx: *mut u64, d_dist: *mut f32,
                                                   capacity: usize, d_total: *mut u64, stream: *mut c_void) -> c_int;
    pub fn pn_sharded_query_radius_self_device_f64(sharded: *const pn_sharded, radius: f64, flags: c_uint,
                                                   d_offsets: *mut u64, d_idx: *mut u64, d_dist: *mut f64,
                                                   capacity: usize, d_total: *mut u64, stream: *mut c_void) -> c_int;

    /// self-queries: every indexed row against its own index, the row itself left out (PN_SELF_INCLUDE keeps it)
    pub fn pn_query_self_f32(index: *const pn_index, k: usize, flags: c_uint, idx_out: *mut u64, dist_out: *mut f32) -> c_int;
    pub fn pn_query_self_f64(index: *const pn_index, k: usize, flags: c_uint, idx_out: *mut u64, dist_out: *mut f64) -> c_int;
    pub fn pn_query_self_device_f32(index: *const pn_index, k: usize, flags: c_uint, d_idx: *mut u64, d_dist: *mut f32,
                                    stream: *mut c_void) -> c_int;
    pub fn pn_query_self_device_f64(index: *const pn_index, k: usize, flags: c_uint, d_idx: *mut u64, d_dist: *mut f64,
                                    stream: *mut c_void) -> c_int;
    /// DBSCAN on the device: labels [n] (-1 = noise), core [n] bytes (nullable), n_clusters [1] (nullable); flags = 0.
    /// The device entry points write in stream order and block the host once
    pub fn pn_dbscan_f32(index: *const pn_index, eps: f32, min_samples: usize, flags: c_uint, labels: *mut i64,
                         core: *mut u8, n_clusters: *mut u64) -> c_int;
    pub fn pn_dbscan_f64(index: *const pn_index, eps: f64, min_samples: usize, flags: c_uint, labels: *mut i64,
                         core: *mut u8, n_clusters: *mut u64) -> c_int;
    pub fn pn_dbscan_device_f32(index: *const pn_index, eps: f32, min_samples: usize, flags: c_uint, d_labels: *mut i64,
                                d_core: *mut u8, d_n_clusters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn pn_dbscan_device_f64(index: *const pn_index, eps: f64, min_samples: usize, flags: c_uint, d_labels: *mut i64,
                                d_core: *mut u8, d_n_clusters: *mut u64, stream: *mut c_void) -> c_int;
    /// Minimum spanning tree under mutual reachability: core [n] (nullable: no cores), src / dst / weight [n - 1] ascending
    /// by (weight, src, dst), work_out (nullable, a host pointer in both variants) = {rounds, rows scanned}; flags = 0.
    /// The device entry points write in stream order and block the host once per round
    pub fn pn_mst_f32(index: *const pn_index, core: *const f32, flags: c_uint, src_out: *mut u64, dst_out: *mut u64,
                      weight_out: *mut f32, work_out: *mut u64) -> c_int;
    pub fn pn_mst_f64(index: *const pn_index, core: *const f64, flags: c_uint, src_out: *mut u64, dst_out: *mut u64,
                      weight_out: *mut f64, work_out: *mut u64) -> c_int;
    pub fn pn_mst_device_f32(index: *const pn_index, d_core: *const f32, flags: c_uint, d_src: *mut u64, d_dst: *mut u64,
                             d_weight: *mut f32, work_out: *mut u64, stream: *mut c_void) -> c_int;
    pub fn pn_mst_device_f64(index: *const pn_index, d_core: *const f64, flags: c_uint, d_src: *mut u64, d_dst: *mut u64,
                             d_weight: *mut f64, work_out: *mut u64, stream: *mut c_void) -> c_int;
    /// Single-linkage dendrogram of n - 1 sorted tree edges (as pn_mst_* writes them): left / right / weight_out / size
    /// [n - 1], node n + r = the r-th merge; flags = 0.  Edges that are no spanning tree: PN_ERR_INVALID (device entry:
    /// written to d_error, an int32 in HBM, nullable; it never waits for the device)
    pub fn pn_linkage_f32(index: *const pn_index, src: *const u64, dst: *const u64, weight: *const f32, flags: c_uint,
                          left_out: *mut u64, right_out: *mut u64, weight_out: *mut f32, size_out: *mut u64) -> c_int;
    pub fn pn_linkage_f64(index: *const pn_index, src: *const u64, dst: *const u64, weight: *const f64, flags: c_uint,
                          left_out: *mut u64, right_out: *mut u64, weight_out: *mut f64, size_out: *mut u64) -> c_int;
    pub fn pn_linkage_device_f32(index: *const pn_index, d_src: *const u64, d_dst: *const u64, d_weight: *const f32,
                                 flags: c_uint, d_left: *mut u64, d_right: *mut u64, d_weight_out: *mut f32,
                                 d_size: *mut u64, d_error: *mut i32, stream: *mut c_void) -> c_int;
    pub fn pn_linkage_device_f64(index: *const pn_index, d_src: *const u64, d_dst: *const u64, d_weight: *const f64,
                                 flags: c_uint, d_left: *mut u64, d_right: *mut u64, d_weight_out: *mut f64,
                                 d_size: *mut u64, d_error: *mut i32, stream: *mut c_void) -> c_int;
    /// HDBSCAN: labels [n] (-1 = noise), probabilities [n] (nullable), n_clusters [1] (nullable); min_samples counts other
    /// rows; flags = 0.  The device entry points keep the host waits of pn_mst_device_* and add none
    pub fn pn_hdbscan_f32(index: *const pn_index, min_samples: usize, min_cluster_size: usize, flags: c_uint,
                          labels: *mut i64, probabilities: *mut f32, n_clusters: *mut u64) -> c_int;
    pub fn pn_hdbscan_f64(index: *const pn_index, min_samples: usize, min_cluster_size: usize, flags: c_uint,
                          labels: *mut i64, probabilities: *mut f64, n_clusters: *mut u64) -> c_int;
    pub fn pn_hdbscan_device_f32(index: *const pn_index, min_samples: usize, min_cluster_size: usize, flags: c_uint,
                                 d_labels: *mut i64, d_probabilities: *mut f32, d_n_clusters: *mut u64,
                                 stream: *mut c_void) -> c_int;
    pub fn pn_hdbscan_device_f64(index: *const pn_index, min_samples: usize, min_cluster_size: usize, flags: c_uint,
                                 d_labels: *mut i64, d_probabilities: *mut f64, d_n_clusters: *mut u64,
                                 stream: *mut c_void) -> c_int;
    /// Local Outlier Factor of the indexed rows: lof [n] (required), lrd [n] and kdist [n] (nullable; the fit that
    /// pn_lof_score_* takes back); k counts other rows, 1 <= k <= n - 1; flags = 0.  The device entry points never wait
    pub fn pn_lof_f32(index: *const pn_index, k: usize, flags: c_uint, lof: *mut f64, lrd: *mut f64,
                      kdist: *mut f32) -> c_int;
    pub fn pn_lof_f64(index: *const pn_index, k: usize, flags: c_uint, lof: *mut f64, lrd: *mut f64,
                      kdist: *mut f64) -> c_int;
    pub fn pn_lof_device_f32(index: *const pn_index, k: usize, flags: c_uint, d_lof: *mut f64, d_lrd: *mut f64,
                             d_kdist: *mut f32, stream: *mut c_void) -> c_int;
    pub fn pn_lof_device_f64(index: *const pn_index, k: usize, flags: c_uint, d_lof: *mut f64, d_lrd: *mut f64,
                             d_kdist: *mut f64, stream: *mut c_void) -> c_int;
    /// scores [nq] of new points against a fit (lrd, kdist of pn_lof_* with the same k)
    pub fn pn_lof_score_f32(index: *const pn_index, queries: *const f32, nq: usize, q_cols: usize, q_row_stride: isize,
                            k: usize, lrd: *const f64, kdist: *const f32, flags: c_uint, score_out: *mut f64) -> c_int;
    pub fn pn_lof_score_f64(index: *const pn_index, queries: *const f64, nq: usize, q_cols: usize, q_row_stride: isize,
                            k: usize, lrd: *const f64, kdist: *const f64, flags: c_uint, score_out: *mut f64) -> c_int;
    pub fn pn_lof_score_device_f32(index: *const pn_index, d_queries: *const f32, nq: usize, q_cols: usize,
                                   q_row_stride: usize, k: usize, d_lrd: *const f64, d_kdist: *const f32, flags: c_uint,
                                   d_score: *mut f64, stream: *mut c_void) -> c_int;
    pub fn pn_lof_score_device_f64(index: *const pn_index, d_queries: *const f64, nq: usize, q_cols: usize,
                                   q_row_stride: usize, k: usize, d_lrd: *const f64, d_kdist: *const f64, flags: c_uint,
                                   d_score: *mut f64, stream: *mut c_void) -> c_int;
    /// k-NN classification: pred [nq] int64 (required; -1 = a list with a NaN distance or a label out of range), proba
    /// [nq][n_classes] f64 (nullable); labels [n] int64 codes in [0, n_classes); flags = 0 or PN_KNN_WEIGHT_DISTANCE (1);
    /// 1 <= k <= min(n, 1024).  The _self entries predict every indexed row from its k nearest other rows, k <= n - 1.
    /// The device entry points never wait
    pub fn pn_knn_classify_f32(index: *const pn_index, queries: *const f32, nq: usize, q_cols: usize, q_row_stride: isize,
                               k: usize, labels: *const i64, n_classes: usize, flags: c_uint, pred_out: *mut i64,
                               proba_out: *mut f64) -> c_int;
    pub fn pn_knn_classify_f64(index: *const pn_index, queries: *const f64, nq: usize, q_cols: usize, q_row_stride: isize,
                               k: usize, labels: *const i64, n_classes: usize, flags: c_uint, pred_out: *mut i64,
                               proba_out: *mut f64) -> c_int;
    pub fn pn_knn_classify_device_f32(index: *const pn_index, d_queries: *const f32, nq: usize, q_cols: usize,
                                      q_row_stride: usize, k: usize, d_labels: *const i64, n_classes: usize, flags: c_uint,
                                      d_pred: *mut i64, d_proba: *mut f64, stream: *mut c_void) -> c_int;
    pub fn pn_knn_classify_device_f64(index: *const pn_index, d_queries: *const f64, nq: usize, q_cols: usize,
                                      q_row_stride: usize, k: usize, d_labels: *const i64, n_classes: usize, flags: c_uint,
                                      d_pred: *mut i64, d_proba: *mut f64, stream: *mut c_void) -> c_int;
    pub fn pn_knn_classify_self_f32(index: *const pn_index, k: usize, labels: *const i64, n_classes: usize, flags: c_uint,
                                    pred_out: *mut i64, proba_out: *mut f64) -> c_int;
    pub fn pn_knn_classify_self_f64(index: *const pn_index, k: usize, labels: *const i64, n_classes: usize, flags: c_uint,
                                    pred_out: *mut i64, proba_out: *mut f64) -> c_int;
    pub fn pn_knn_classify_self_device_f32(index: *const pn_index, k: usize, d_labels: *const i64, n_classes: usize,
                                           flags: c_uint, d_pred: *mut i64, d_proba: *mut f64, stream: *mut c_void) -> c_int;
    pub fn pn_knn_classify_self_device_f64(index: *const pn_index, k: usize, d_labels: *const i64, n_classes: usize,
                                           flags: c_uint, d_pred: *mut i64, d_proba: *mut f64, stream: *mut c_void) -> c_int;
    /// k-NN regression: out [nq][n_out] f64 (required) from targets [n][n_out] f64; flags, k and the _self entries as above
    pub fn pn_knn_regress_f32(index: *const pn_index, queries: *const f32, nq: usize, q_cols: usize, q_row_stride: isize,
                              k: usize, targets: *const f64, n_out: usize, flags: c_uint, out: *mut f64) -> c_int;
    pub fn pn_knn_regress_f64(index: *const pn_index, queries: *const f64, nq: usize, q_cols: usize, q_row_stride: isize,
                              k: usize, targets: *const f64, n_out: usize, flags: c_uint, out: *mut f64) -> c_int;
    pub fn pn_knn_regress_device_f32(index: *const pn_index, d_queries: *const f32, nq: usize, q_cols: usize,
                                     q_row_stride: usize, k: usize, d_targets: *const f64, n_out: usize, flags: c_uint,
                                     d_out: *mut f64, stream: *mut c_void) -> c_int;
    pub fn pn_knn_regress_device_f64(index: *const pn_index, d_queries: *const f64, nq: usize, q_cols: usize,
                                     q_row_stride: usize, k: usize, d_targets: *const f64, n_out: usize, flags: c_uint,
                                     d_out: *mut f64, stream: *mut c_void) -> c_int;
    pub fn pn_knn_regress_self_f32(index: *const pn_index, k: usize, targets: *const f64, n_out: usize, flags: c_uint,
                                   out: *mut f64) -> c_int;
    pub fn pn_knn_regress_self_f64(index: *const pn_index, k: usize, targets: *const f64, n_out: usize, flags: c_uint,
                                   out: *mut f64) -> c_int;
    pub fn pn_knn_regress_self_device_f32(index: *const pn_index, k: usize, d_targets: *const f64, n_out: usize,
                                          flags: c_uint, d_out: *mut f64, stream: *mut c_void) -> c_int;
    pub fn pn_knn_regress_self_device_f64(index: *const pn_index, k: usize, d_targets: *const f64, n_out: usize,
                                          flags: c_uint, d_out: *mut f64, stream: *mut c_void) -> c_int;
    /// OPTICS of the indexed rows: ordering [n] (row numbers, no index base) and reachability [n] required, predecessor [n]
    /// and core_distances [n] nullable; min_samples counts other rows, 1 <= min_samples <= n - 1; flags = 0.  The device
    /// entry points write in stream order and block the host once
    pub fn pn_optics_f32(index: *const pn_index, min_samples: usize, max_eps: f32, flags: c_uint, ordering: *mut u64,
                         reachability: *mut f32, predecessor: *mut i64, core_distances: *mut f32) -> c_int;
    pub fn pn_optics_f64(index: *const pn_index, min_samples: usize, max_eps: f64, flags: c_uint, ordering: *mut u64,
                         reachability: *mut f64, predecessor: *mut i64, core_distances: *mut f64) -> c_int;
    pub fn pn_optics_device_f32(index: *const pn_index, min_samples: usize, max_eps: f32, flags: c_uint,
                                d_ordering: *mut u64, d_reachability: *mut f32, d_predecessor: *mut i64,
                                d_core_distances: *mut f32, stream: *mut c_void) -> c_int;
    pub fn pn_optics_device_f64(index: *const pn_index, min_samples: usize, max_eps: f64, flags: c_uint,
                                d_ordering: *mut u64, d_reachability: *mut f64, d_predecessor: *mut i64,
                                d_core_distances: *mut f64, stream: *mut c_void) -> c_int;
    /// DBSCAN labels at eps read off an ordering: labels [n] (-1 = noise, clusters numbered by first appearance in the
    /// ordering), n_clusters [1] nullable; an ordering that is no permutation: PN_ERR_INVALID (device: d_error [1], nullable)
    pub fn pn_optics_dbscan_f32(index: *const pn_index, ordering: *const u64, reachability: *const f32,
                                core_distances: *const f32, eps: f32, flags: c_uint, labels: *mut i64,
                                n_clusters: *mut u64) -> c_int;
    pub fn pn_optics_dbscan_f64(index: *const pn_index, ordering: *const u64, reachability: *const f64,
                                core_distances: *const f64, eps: f64, flags: c_uint, labels: *mut i64,
                                n_clusters: *mut u64) -> c_int;
    pub fn pn_optics_dbscan_device_f32(index: *const pn_index, d_ordering: *const u64, d_reachability: *const f32,
                                       d_core_distances: *const f32, eps: f32, flags: c_uint, d_labels: *mut i64,
                                       d_n_clusters: *mut u64, d_error: *mut i32, stream: *mut c_void) -> c_int;
    pub fn pn_optics_dbscan_device_f64(index: *const pn_index, d_ordering: *const u64, d_reachability: *const f64,
                                       d_core_distances: *const f64, eps: f64, flags: c_uint, d_labels: *mut i64,
                                       d_n_clusters: *mut u64, d_error: *mut i32, stream: *mut c_void) -> c_int;
    /// kernel density sums: per query the raw sum of `kernel` (PN_KDE_*) over the rows within the kernel's cutoff, the
    /// number of terms and the cutoff; h: n_h = 1 or one bandwidth per query; sum nullable if count is given (then only
    /// the counting pass runs); flags = 0 (self entries: PN_SELF_INCLUDE or 0).  The device entry points write in stream
    /// order and block the host once when a sum is asked for
    pub fn pn_kde_f32(index: *const pn_index, queries: *const f32, nq: usize, q_cols: usize, q_row_stride: isize,
                      h: *const f32, n_h: usize, kernel: c_int, atol: f64, flags: c_uint, sum_out: *mut f64,
                      count_out: *mut u64, cutoff_out: *mut f32) -> c_int;
    pub fn pn_kde_device_f32(index: *const pn_index, d_queries: *const f32, nq: usize, q_cols: usize, q_row_stride: usize,
                             d_h: *const f32, n_h: usize, kernel: c_int, atol: f64, flags: c_uint, d_sum: *mut f64,
                             d_count: *mut u64, d_cutoff: *mut f32, stream: *mut c_void) -> c_int;
    pub fn pn_kde_self_f32(index: *const pn_index, h: *const f32, n_h: usize, kernel: c_int, atol: f64, flags: c_uint,
                           sum_out: *mut f64, count_out: *mut u64, cutoff_out: *mut f32) -> c_int;
    pub fn pn_kde_self_device_f32(index: *const pn_index, d_h: *const f32, n_h: usize, kernel: c_int, atol: f64,
                                  flags: c_uint, d_sum: *mut f64, d_count: *mut u64, d_cutoff: *mut f32,
                                  stream: *mut c_void) -> c_int;
    pub fn pn_kde_f64(index: *const pn_index, queries: *const f64, nq: usize, q_cols: usize, q_row_stride: isize,
                      h: *const f64, n_h: usize, kernel: c_int, atol: f64, flags: c_uint, sum_out: *mut f64,
                      count_out: *mut u64, cutoff_out: *mut f64) -> c_int;
    pub fn pn_kde_device_f64(index: *const pn_index, d_queries: *const f64, nq: usize, q_cols: usize, q_row_stride: usize,
                             d_h: *const f64, n_h: usize, kernel: c_int, atol: f64, flags: c_uint, d_sum: *mut f64,
                             d_count: *mut u64, d_cutoff: *mut f64, stream: *mut c_void) -> c_int;
    pub fn pn_kde_self_f64(index: *const pn_index, h: *const f64, n_h: usize, kernel: c_int, atol: f64, flags: c_uint,
                           sum_out: *mut f64, count_out: *mut u64, cutoff_out: *mut f64) -> c_int;
    pub fn pn_kde_self_device_f64(index: *const pn_index, d_h: *const f64, n_h: usize, kernel: c_int, atol: f64,
                                  flags: c_uint, d_sum: *mut f64, d_count: *mut u64, d_cutoff: *mut f64,
                                  stream: *mut c_void) -> c_int;
    /// mean shift (flat kernel): seeds to modes (only the seeds still moving are queried; the device entry blocks the
    /// host twice per iteration; work = {iterations, seed-steps} in host memory, nullable), modes to centres, rows to
    /// labels (these two never wait); h: n_h = 1 or one bandwidth per seed; iterations / shift nullable
    pub fn pn_mean_shift_f32(index: *const pn_index, seeds: *const f32, ns: usize, s_cols: usize, s_row_stride: isize,
                             h: *const f32, n_h: usize, tol: f64, max_iter: usize, flags: c_uint, modes_out: *mut f32,
                             points_within_out: *mut u64, iterations_out: *mut u32, shift_out: *mut f64,
                             work: *mut u64) -> c_int;
    pub fn pn_mean_shift_device_f32(index: *const pn_index, d_seeds: *const f32, ns: usize, s_cols: usize,
                                    s_row_stride: usize, d_h: *const f32, n_h: usize, tol: f64, max_iter: usize,
                                    flags: c_uint, d_modes: *mut f32, d_points_within: *mut u64, d_iterations: *mut u32,
                                    d_shift: *mut f64, work: *mut u64, stream: *mut c_void) -> c_int;
    pub fn pn_mean_shift_merge_f32(index: *const pn_index, modes: *const f32, ns: usize, points_within: *const u64, h: f32,
                                   flags: c_uint, centres_out: *mut f32, centre_points_out: *mut u64,
                                   centre_of_seed_out: *mut i64, n_centres_out: *mut u64) -> c_int;
    pub fn pn_mean_shift_merge_device_f32(index: *const pn_index, d_modes: *const f32, ns: usize,
                                          d_points_within: *const u64, h: f32, flags: c_uint, d_centres: *mut f32,
                                          d_centre_points: *mut u64, d_centre_of_seed: *mut i64, d_n_centres: *mut u64,
                                          stream: *mut c_void) -> c_int;
    pub fn pn_mean_shift_labels_f32(index: *const pn_index, centres: *const f32, nc: usize, h: f32, flags: c_uint,
                                    labels: *mut i64) -> c_int;
    pub fn pn_mean_shift_labels_device_f32(index: *const pn_index, d_centres: *const f32, nc: usize, h: f32, flags: c_uint,
                                           d_labels: *mut i64, stream: *mut c_void) -> c_int;
    pub fn pn_mean_shift_f64(index: *const pn_index, seeds: *const f64, ns: usize, s_cols: usize, s_row_stride: isize,
                             h: *const f64, n_h: usize, tol: f64, max_iter: usize, flags: c_uint, modes_out: *mut f64,
                             points_within_out: *mut u64, iterations_out: *mut u32, shift_out: *mut f64,
                             work: *mut u64) -> c_int;
    pub fn pn_mean_shift_device_f64(index: *const pn_index, d_seeds: *const f64, ns: usize, s_cols: usize,
                                    s_row_stride: usize, d_h: *const f64, n_h: usize, tol: f64, max_iter: usize,
                                    flags: c_uint, d_modes: *mut f64, d_points_within: *mut u64, d_iterations: *mut u32,
                                    d_shift: *mut f64, work: *mut u64, stream: *mut c_void) -> c_int;
    pub fn pn_mean_shift_merge_f64(index: *const pn_index, modes: *const f64, ns: usize, points_within: *const u64, h: f64,
                                   flags: c_uint, centres_out: *mut f64, centre_points_out: *mut u64,
                                   centre_of_seed_out: *mut i64, n_centres_out: *mut u64) -> c_int;
    pub fn pn_mean_shift_merge_device_f64(index: *const pn_index, d_modes: *const f64, ns: usize,
                                          d_points_within: *const u64, h: f64, flags: c_uint, d_centres: *mut f64,
                                          d_centre_points: *mut u64, d_centre_of_seed: *mut i64, d_n_centres: *mut u64,
                                          stream: *mut c_void) -> c_int;
    pub fn pn_mean_shift_labels_f64(index: *const pn_index, centres: *const f64, nc: usize, h: f64, flags: c_uint,
                                    labels: *mut i64) -> c_int;
    pub fn pn_mean_shift_labels_device_f64(index: *const pn_index, d_centres: *const f64, nc: usize, h: f64, flags: c_uint,
                                           d_labels: *mut i64, stream: *mut c_void) -> c_int;
    /// k-means (include/petal_mi355x.h): dist / counts / inertia / iterations / shift2 outputs nullable
    pub fn pn_kmeans_assign_f32(index: *const pn_index, centres: *const f32, nc: usize, flags: c_uint,
                                labels_out: *mut i64, dist_out: *mut f32, inertia_out: *mut f64) -> c_int;
    pub fn pn_kmeans_assign_device_f32(index: *const pn_index, d_centres: *const f32, nc: usize, flags: c_uint,
                                       d_labels: *mut i64, d_dist: *mut f32, d_inertia: *mut f64,
                                       stream: *mut c_void) -> c_int;
    pub fn pn_kmeans_f32(index: *const pn_index, init_centres: *const f32, nc: usize, tol: f64, max_iter: usize,
                         flags: c_uint, centres_out: *mut f32, labels_out: *mut i64, dist_out: *mut f32,
                         counts_out: *mut u64, inertia_out: *mut f64, iterations_out: *mut u64,
                         shift2_out: *mut f64) -> c_int;
    pub fn pn_kmeans_device_f32(index: *const pn_index, d_init_centres: *const f32, nc: usize, tol: f64, max_iter: usize,
                                flags: c_uint, d_centres: *mut f32, d_labels: *mut i64, d_dist: *mut f32,
                                d_counts: *mut u64, d_inertia: *mut f64, d_iterations: *mut u64, d_shift2: *mut f64,
                                stream: *mut c_void) -> c_int;
    pub fn pn_kmeans_assign_f64(index: *const pn_index, centres: *const f64, nc: usize, flags: c_uint,
                                labels_out: *mut i64, dist_out: *mut f64, inertia_out: *mut f64) -> c_int;
    pub fn pn_kmeans_assign_device_f64(index: *const pn_index, d_centres: *const f64, nc: usize, flags: c_uint,
                                       d_labels: *mut i64, d_dist: *mut f64, d_inertia: *mut f64,
                                       stream: *mut c_void) -> c_int;
    pub fn pn_kmeans_f64(index: *const pn_index, init_centres: *const f64, nc: usize, tol: f64, max_iter: usize,
                         flags: c_uint, centres_out: *mut f64, labels_out: *mut i64, dist_out: *mut f64,
                         counts_out: *mut u64, inertia_out: *mut f64, iterations_out: *mut u64,
                         shift2_out: *mut f64) -> c_int;
    pub fn pn_kmeans_device_f64(index: *const pn_index, d_init_centres: *const f64, nc: usize, tol: f64, max_iter: usize,
                                flags: c_uint, d_centres: *mut f64, d_labels: *mut i64, d_dist: *mut f64,
                                d_counts: *mut u64, d_inertia: *mut f64, d_iterations: *mut u64, d_shift2: *mut f64,
                                stream: *mut c_void) -> c_int;
    pub fn pn_kmeans_bounds_f32(index: *const pn_index, centres: *const f32, nc: usize, bounds_out: *mut f64) -> c_int;
    /// dist_out nullable (PN_RADIUS_SORTED needs it); *idx_out / *dist_out released with pn_free
    pub fn pn_query_radius_self_f32(index: *const pn_index, radius: f32, flags: c_uint, offsets: *mut u64,
                                    idx_out: *mut *mut u64, dist_out: *mut *mut f32) -> c_int;
    pub fn pn_query_radius_self_f64(index: *const pn_index, radius: f64, flags: c_uint, offsets: *mut u64,
                                    idx_out: *mut *mut u64, dist_out: *mut *mut f64) -> c_int;
    pub fn pn_query_radius_self_device_f32(index: *const pn_index, radius: f32, flags: c_uint, d_offsets: *mut u64,
                                           d_idx: *mut u64, d_dist: *mut f32, capacity: usize, d_total: *mut u64,
                                           stream: *mut c_void) -> c_int;
    pub fn pn_query_radius_self_device_f64(index: *const pn_index, radius: f64, flags: c_uint, d_offsets: *mut u64,
                                           d_idx: *mut u64, d_dist: *mut f64, capacity: usize, d_total: *mut u64,
                                           stream: *mut c_void) -> c_int;

    /// one radius per query (radii [nq]; self-queries: [n]): list q is the scalar entry point's for query q with radii[q]
    pub fn pn_query_radii_f32(index: *const pn_index, queries: *const f32, nq: usize, q_cols: usize, q_row_stride: isize,
                              radii: *const f32, flags: c_uint, offsets: *mut u64, idx_out: *mut *mut u64,
                              dist_out: *mut *mut f32) -> c_int;
    pub fn pn_query_radii_f64(index: *const pn_index, queries: *const f64, nq: usize, q_cols: usize, q_row_stride: isize,
                              radii: *const f64, flags: c_uint, offsets: *mut u64, idx_out: *mut *mut u64,
                              dist_out: *mut *mut f64) -> c_int;
    pub fn pn_query_radii_device_f32(index: *const pn_index, d_queries: *const f32, nq: usize, q_cols: usize,
                                     q_row_stride: usize, d_radii: *const f32, flags: c_uint, d_offsets: *mut u64,
                                     d_idx: *mut u64, d_dist: *mut f32, capacity: usize, d_total: *mut u64,
                                     stream: *mut c_void) -> c_int;
    pub fn pn_query_radii_device_f64(index: *const pn_index, d_queries: *const f64, nq: usize, q_cols: usize,
                                     q_row_stride: usize, d_radii: *const f64, flags: c_uint, d_offsets: *mut u64,
                                     d_idx: *mut u64, d_dist: *mut f64, capacity: usize, d_total: *mut u64,
                                     stream: *mut c_void) -> c_int;
    pub fn pn_query_radii_self_f32(index: *const pn_index, radii: *const f32, flags: c_uint, offsets: *mut u64,
                                   idx_out: *mut *mut u64, dist_out: *mut *mut f32) -> c_int;
    pub fn pn_query_radii_self_f64(index: *const pn_index, radii: *const f64, flags: c_uint, offsets: *mut u64,
                                   idx_out: *mut *mut u64, dist_out: *mut *mut f64) -> c_int;
    pub fn pn_query_radii_self_device_f32(index: *const pn_index, d_radii: *const f32, flags: c_uint, d_offsets: *mut u64,
                                          d_idx: *mut u64, d_dist: *mut f32, capacity: usize, d_total: *mut u64,
                                          stream: *mut c_void) -> c_int;
    pub fn pn_query_radii_self_device_f64(index: *const pn_index, d_radii: *const f64, flags: c_uint, d_offsets: *mut u64,
                                          d_idx: *mut u64, d_dist: *mut f64, capacity: usize, d_total: *mut u64,
                                          stream: *mut c_void) -> c_int;

    pub fn pn_pairwise_f32(x: *const f32, n_rows: usize, n_cols: usize, row_stride: isize, device: c_int,
                           out: *mut f32) -> c_int;
    pub fn pn_pairwise_f64(x: *const f64, n_rows: usize, n_cols: usize, row_stride: isize, device: c_int,
                           out: *mut f64) -> c_int;
    pub fn pn_pairwise_cosine_f32(x: *const f32, n_rows: usize, n_cols: usize, row_stride: isize, device: c_int,
                                  out: *mut f32) -> c_int;
    pub fn pn_pairwise_cosine_f64(x: *const f64, n_rows: usize, n_cols: usize, row_stride: isize, device: c_int,
                                  out: *mut f64) -> c_int;
    pub fn pn_euclidean_f32(a: *const f32, b: *const f32, len: usize) -> f32;
    pub fn pn_euclidean_f64(a: *const f64, b: *const f64, len: usize) -> f64;
    pub fn pn_reuclidean_f32(a: *const f32, b: *const f32, len: usize) -> f32;
    pub fn pn_reuclidean_f64(a: *const f64, b: *const f64, len: usize) -> f64;
    pub fn pn_cosine_f32(a: *const f32, len_a: usize, b: *const f32, len_b: usize) -> f32;
    pub fn pn_cosine_f64(a: *const f64, len_a: usize, b: *const f64, len_b: usize) -> f64;

    // tree introspection (src/ball_tree.rs:296-353)
    pub fn pn_tree_num_nodes(index: *const pn_index, out: *mut u64) -> c_int;
    pub fn pn_tree_children_of(index: *const pn_index, node: u64, is_some: *mut c_int, left: *mut u64,
                               right: *mut u64) -> c_int;
    pub fn pn_tree_points_of(index: *const pn_index, node: u64, idx: *mut *const u64, count: *mut u64) -> c_int;
    pub fn pn_tree_radius_of_f32(index: *const pn_index, node: u64, out: *mut f32) -> c_int;
    pub fn pn_tree_radius_of_f64(index: *const pn_index, node: u64, out: *mut f64) -> c_int;
    pub fn pn_tree_compare_nodes(index: *const pn_index, x: u64, y: u64, ordering: *mut c_int) -> c_int;
    pub fn pn_tree_node_distance_lower_bound_f32(index: *const pn_index, n1: u64, n2: u64, out: *mut f32) -> c_int;
    pub fn pn_tree_node_distance_lower_bound_f64(index: *const pn_index, n1: u64, n2: u64, out: *mut f64) -> c_int;

    // row shards over several GPUs, one RCCL all-gather per batch behind the ABI
    pub fn pn_sharded_create_f32(points: *const f32, n_rows: usize, n_cols: usize, row_stride: isize,
                                 col_stride: isize, devices: *const c_int, n_devices: c_int,
                                 out: *mut *mut pn_sharded) -> c_int;
    pub fn pn_sharded_destroy(sharded: *mut pn_sharded);
    pub fn pn_sharded_query_f32(sharded: *const pn_sharded, queries: *const f32, nq: usize, q_cols: usize,
                                q_row_stride: isize, k: usize, idx_out: *mut u64, dist_out: *mut f32) -> c_int;
    pub fn pn_sharded_query_radius_f32(sharded: *const pn_sharded, queries: *const f32, nq: usize, q_cols: usize,
                                       q_row_stride: isize, radius: f32, offsets: *mut u64,
                                       idx_out: *mut *mut u64) -> c_int;
    // the same over an f64 corpus
    pub fn pn_sharded_create_f64(points: *const f64, n_rows: usize, n_cols: usize, row_stride: isize,
                                 col_stride: isize, devices: *const c_int, n_devices: c_int,
                                 out: *mut *mut pn_sharded) -> c_int;
    pub fn pn_sharded_query_f64(sharded: *const pn_sharded, queries: *const f64, nq: usize, q_cols: usize,
                                q_row_stride: isize, k: usize, idx_out: *mut u64, dist_out: *mut f64) -> c_int;
    pub fn pn_sharded_query_radius_f64(sharded: *const pn_sharded, queries: *const f64, nq: usize, q_cols: usize,
                                       q_row_stride: isize, radius: f64, offsets: *mut u64,
                                       idx_out: *mut *mut u64) -> c_int;
}
