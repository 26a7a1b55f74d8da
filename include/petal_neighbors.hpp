// petal_neighbors.hpp -- header-only C++17 mirror of petal-neighbors' public API for the
// hot path (reference src/lib.rs:1-16, src/ball_tree.rs:15-374, src/distance.rs:9-74) over
// the C ABI in petal_mi355x.h.  Same names, argument meaning and error behaviour as the
// Rust types; results as std::vector like the Rust `Vec`s.  Link with -lpetal_mi355x.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "petal_mi355x.h"

namespace petal {

// ArrayError (src/lib.rs:9-16)
struct ArrayError : std::runtime_error {
    enum Kind { Empty, NotContiguous } kind;
    ArrayError(Kind k) : std::runtime_error(k == Empty ? "array is empty" : "array is not contiguous in memory"), kind(k) {}
};
struct DeviceError : std::runtime_error {
    int code;
    DeviceError(int c, const char *m) : std::runtime_error(m), code(c) {}
};

inline void check(int rc) {
    if (rc == PN_OK) return;
    if (rc == PN_ERR_EMPTY) throw ArrayError(ArrayError::Empty);
    if (rc == PN_ERR_NOT_CONTIGUOUS) throw ArrayError(ArrayError::NotContiguous);
    throw DeviceError(rc, pn_last_error());
}

namespace distance {
// Euclidean (src/distance.rs:16-55): zero-sized tag + Metric<A>
struct Euclidean {
    bool operator==(const Euclidean &) const { return true; }
    float distance(const float *a, const float *b, size_t len) const { return pn_euclidean_f32(a, b, len); }
    double distance(const double *a, const double *b, size_t len) const { return pn_euclidean_f64(a, b, len); }
    float rdistance(const float *a, const float *b, size_t len) const { return pn_reuclidean_f32(a, b, len); }
    double rdistance(const double *a, const double *b, size_t len) const { return pn_reuclidean_f64(a, b, len); }
    float rdistance_to_distance(float d) const { return pn_rdistance_to_distance_f32(d); }
    double rdistance_to_distance(double d) const { return pn_rdistance_to_distance_f64(d); }
    float distance_to_rdistance(float d) const { return pn_distance_to_rdistance_f32(d); }
    double distance_to_rdistance(double d) const { return pn_distance_to_rdistance_f64(d); }
};
// Cosine (src/distance.rs:76-122): 1 - dot / (|a| |b|); rdistance and the conversions are the identity
struct Cosine {
    bool operator==(const Cosine &) const { return true; }
    float distance(const float *a, const float *b, size_t len) const { return pn_cosine_f32(a, len, b, len); }
    double distance(const double *a, const double *b, size_t len) const { return pn_cosine_f64(a, len, b, len); }
    float rdistance(const float *a, const float *b, size_t len) const { return distance(a, b, len); }
    double rdistance(const double *a, const double *b, size_t len) const { return distance(a, b, len); }
    float rdistance_to_distance(float d) const { return d; }
    double rdistance_to_distance(double d) const { return d; }
    float distance_to_rdistance(float d) const { return d; }
    double distance_to_rdistance(double d) const { return d; }
};
// pairwise(x, &Cosine)
inline std::vector<float> pairwise(const float *x, size_t n, size_t d, const Cosine &, int device = 0) {
    std::vector<float> out(n * n);
    check(pn_pairwise_cosine_f32(x, n, d, (ptrdiff_t)d, device, out.data()));
    return out;
}
inline std::vector<double> pairwise(const double *x, size_t n, size_t d, const Cosine &, int device = 0) {
    std::vector<double> out(n * n);
    check(pn_pairwise_cosine_f64(x, n, d, (ptrdiff_t)d, device, out.data()));
    return out;
}
// pairwise (src/distance.rs:58-74): n x n row-major
inline std::vector<float> pairwise(const float *x, size_t n, size_t d, int device = 0) {
    std::vector<float> out(n * n);
    check(pn_pairwise_f32(x, n, d, (ptrdiff_t)d, device, out.data()));
    return out;
}
inline std::vector<double> pairwise(const double *x, size_t n, size_t d, int device = 0) {
    std::vector<double> out(n * n);
    check(pn_pairwise_f64(x, n, d, (ptrdiff_t)d, device, out.data()));
    return out;
}
}  // namespace distance

// the answer of BallTree::dbscan
struct Dbscan {
    std::vector<int64_t> labels;  // [n]: cluster number, -1 = noise
    std::vector<uint8_t> core;    // [n]: 1 = core row
    size_t n_clusters = 0;
};
// the answer of BallTree::mst: n - 1 edges with src < dst, ascending by (weight, src, dst)
template <typename A>
struct Mst {
    std::vector<size_t> src, dst;
    std::vector<A> weight;
    size_t rounds = 0, rows_scanned = 0;  // Boruvka rounds run, rows handed to a scan over all of them
};
// the answer of BallTree::linkage, SciPy's layout: merge r makes node n + r with the children left[r] (the subtree that
// holds the edge's src) and right[r]; ids below n are rows; size[r] = rows under the node
template <typename A>
struct Linkage {
    std::vector<size_t> left, right, size;
    std::vector<A> weight;
};
// the answer of BallTree::hdbscan
template <typename A>
struct Hdbscan {
    std::vector<int64_t> labels;   // [n]: cluster number (by ascending lowest member row), -1 = noise
    std::vector<A> probabilities;  // [n]: membership strength, 0 for noise
    size_t n_clusters = 0;
};
// the answer of BallTree::lof: lof[i] = row i's Local Outlier Factor; lrd (local reachability densities) and kdist
// (distances to the k-th nearest other row) are the fit that BallTree::lof_score takes back
template <typename A>
struct Lof {
    std::vector<double> lof, lrd;
    std::vector<A> kdist;
};
// the answer of BallTree::knn_classify: pred[q] = the winning class code (-1: a poisoned list, one with a NaN distance);
// proba [nq][n_classes] row-major, empty unless asked for
struct KnnClasses {
    std::vector<int64_t> pred;
    std::vector<double> proba;
};
// the answer of BallTree::kernel_density: per query the raw kernel sum (not normalised), the number of terms and the
// cutoff radius the terms were taken within
template <typename A>
struct Kde {
    std::vector<double> sum;
    std::vector<size_t> count;
    std::vector<A> cutoff;
};
// the answers of BallTree::mean_shift_modes / mean_shift_merge / mean_shift: modes [ns][dim] dense, per seed the rows within
// the bandwidth of the last mean (0: a dead seed), the iterations and the last shift (NaN: dead); centres [n_centres][dim]
// in rank order with their points, centre_of_seed (-1: dead); labels per indexed row (-1: an orphan)
template <typename A>
struct MeanShift {
    std::vector<A> modes;
    std::vector<size_t> points_within;
    std::vector<uint32_t> iterations;
    std::vector<double> shift;
    size_t n_iter = 0, seed_steps = 0;
    std::vector<A> centres;
    std::vector<size_t> centre_points;
    std::vector<int64_t> centre_of_seed;
    size_t n_centres = 0;
    std::vector<int64_t> labels;
};
// the answer of BallTree::kmeans / kmeans_assign: centres [k][dim] dense, per indexed row the nearest centre (by distance,
// then centre number) and the distance to it, per centre its members in the final assignment (0: the centre lost them all
// and kept its place), the inertia in the library's fixed sum shape, the iterations run and the last summed squared move
template <typename A>
struct KMeans {
    std::vector<A> centres;
    std::vector<int64_t> labels;
    std::vector<A> dist;
    std::vector<size_t> counts;
    double inertia = 0.0, shift2 = 0.0;
    size_t n_iter = 0;
};
// the answer of BallTree::optics: ordering[t] = the t-th row OPTICS visits (a plain row number); reachability, predecessor
// (-1 = none) and core_distances are indexed by row, +inf where undefined
template <typename A>
struct Optics {
    std::vector<size_t> ordering;
    std::vector<A> reachability, core_distances;
    std::vector<int64_t> predecessor;
};
// the answer of BallTree::optics_dbscan: labels [n], clusters numbered by first appearance in the ordering, -1 = noise
struct OpticsDbscan {
    std::vector<int64_t> labels;
    size_t n_clusters = 0;
};
// the CSR answer of BallTree::query_radius_self: row i's neighbours are idx[offsets[i] .. offsets[i + 1]] (dist beside
// them when asked for)
template <typename A>
struct SelfRadius {
    std::vector<size_t> offsets, idx;
    std::vector<A> dist;
};

// BallTree<'a, A, M> (src/ball_tree.rs:15-24): M = distance::Euclidean (default) or distance::Cosine.  Under Cosine
// every query is an exact scan (cosine distance is not a metric; see pn_index_create_cosine_* in petal_mi355x.h).
template <typename A, typename M = distance::Euclidean>
class BallTree {
    static_assert(std::is_same<A, float>::value || std::is_same<A, double>::value, "A is f32 or f64");
    static_assert(std::is_same<M, distance::Euclidean>::value || std::is_same<M, distance::Cosine>::value,
                  "M is Euclidean or Cosine");
    static constexpr bool kF32 = std::is_same<A, float>::value;
    pn_index *h_ = nullptr;
    size_t n_ = 0, dim_ = 0;
    explicit BallTree(pn_index *h, size_t n, size_t d) : h_(h), n_(n), dim_(d) {}

  public:
    M metric;
    BallTree(BallTree &&o) noexcept : h_(o.h_), n_(o.n_), dim_(o.dim_) { o.h_ = nullptr; }
    BallTree(const BallTree &) = delete;
    ~BallTree() { pn_index_destroy(h_); }

    // BallTree::new(points, metric) (src/ball_tree.rs:38-63); strides in elements
    static BallTree create(const A *points, size_t rows, size_t cols, M = M{}, ptrdiff_t row_stride = -1,
                           ptrdiff_t col_stride = 1, int device = 0) {
        pn_index *h = nullptr;
        if (row_stride < 0) row_stride = (ptrdiff_t)cols;
        if constexpr (std::is_same<M, distance::Cosine>::value) {
            if constexpr (kF32)
                check(pn_index_create_cosine_f32(points, rows, cols, row_stride, col_stride, device, &h));
            else
                check(pn_index_create_cosine_f64(points, rows, cols, row_stride, col_stride, device, &h));
        } else {
            if constexpr (kF32)
                check(pn_index_create_f32(points, rows, cols, row_stride, col_stride, device, &h));
            else
                check(pn_index_create_f64(points, rows, cols, row_stride, col_stride, device, &h));
        }
        return BallTree(h, rows, cols);
    }

    // ---- tree introspection (src/ball_tree.rs:296-353); the tree is built on first use (petal_mi355x.h, pn_tree_*)
    size_t num_nodes() const {
        uint64_t v = 0;
        check(pn_tree_num_nodes(h_, &v));
        return (size_t)v;
    }
    // children_of(n) -> Option<(usize, usize)>: {false, ...} for a leaf
    struct Children { bool some; size_t left, right; };
    Children children_of(size_t n) const {
        int some = 0;
        uint64_t l = 0, r = 0;
        check(pn_tree_children_of(h_, n, &some, &l, &r));
        return Children{some != 0, (size_t)l, (size_t)r};
    }
    std::vector<size_t> points_of(size_t n) const {
        const uint64_t *p = nullptr;
        uint64_t c = 0;
        check(pn_tree_points_of(h_, n, &p, &c));
        return std::vector<size_t>(p, p + c);
    }
    A radius_of(size_t n) const {
        A v = 0;
        if constexpr (kF32) check(pn_tree_radius_of_f32(h_, n, &v)); else check(pn_tree_radius_of_f64(h_, n, &v));
        return v;
    }
    // compare_nodes(x, y) -> Option<Ordering>: -1 / 0 / 1, or 2 for None (a NaN radius)
    int compare_nodes(size_t x, size_t y) const {
        int o = 0;
        check(pn_tree_compare_nodes(h_, x, y, &o));
        return o;
    }
    A node_distance_lower_bound(size_t n1, size_t n2) const {
        A v = 0;
        if constexpr (kF32)
            check(pn_tree_node_distance_lower_bound_f32(h_, n1, n2, &v));
        else
            check(pn_tree_node_distance_lower_bound_f64(h_, n1, n2, &v));
        return v;
    }

    // BallTree::euclidean / ::new (src/ball_tree.rs:38-63, 367-373); strides in elements
    static BallTree euclidean(const A *points, size_t rows, size_t cols, ptrdiff_t row_stride = -1,
                              ptrdiff_t col_stride = 1, int device = 0) {
        static_assert(std::is_same<M, distance::Euclidean>::value, "euclidean() builds a BallTree<A, Euclidean>");
        return create(points, rows, cols, M{}, row_stride, col_stride, device);
    }
    size_t num_points() const { return n_; }  // src/ball_tree.rs:351

    // query (src/ball_tree.rs:102): ascending, min(k, n) results, k == 0 -> empty
    std::pair<std::vector<size_t>, std::vector<A>> query(const A *point, size_t len, size_t k) const {
        const size_t kout = k < n_ ? k : n_;
        std::vector<uint64_t> idx(kout);
        std::vector<A> dist(kout);
        if constexpr (std::is_same<A, float>::value)
            check(pn_query_f32(h_, point, 1, len, (ptrdiff_t)len, k, idx.data(), dist.data()));
        else
            check(pn_query_f64(h_, point, 1, len, (ptrdiff_t)len, k, idx.data(), dist.data()));
        return {std::vector<size_t>(idx.begin(), idx.end()), std::move(dist)};
    }
    // query_nearest (src/ball_tree.rs:80)
    std::pair<size_t, A> query_nearest(const A *point, size_t len) const {
        uint64_t i = 0;
        A d = 0;
        if constexpr (std::is_same<A, float>::value)
            check(pn_query_nearest_f32(h_, point, 1, len, (ptrdiff_t)len, &i, &d));
        else
            check(pn_query_nearest_f64(h_, point, 1, len, (ptrdiff_t)len, &i, &d));
        return {(size_t)i, d};
    }
    // query_radius (src/ball_tree.rs:137); ascending indices
    std::vector<size_t> query_radius(const A *point, size_t len, A distance) const {
        uint64_t off[2] = {0, 0};
        uint64_t *out = nullptr;
        if constexpr (std::is_same<A, float>::value)
            check(pn_query_radius_f32(h_, point, 1, len, (ptrdiff_t)len, distance, off, &out));
        else
            check(pn_query_radius_f64(h_, point, 1, len, (ptrdiff_t)len, distance, off, &out));
        std::vector<size_t> v(out, out + off[1]);
        pn_free(out);
        return v;
    }
    // extension: query_radius with each neighbour's distance (pn_query_radius_with_distance_*); ascending indices, or
    // nearest first by (distance, index) with sorted = true
    std::pair<std::vector<size_t>, std::vector<A>> query_radius_with_distance(const A *point, size_t len, A distance,
                                                                              bool sorted) const {
        uint64_t off[2] = {0, 0};
        uint64_t *out = nullptr;
        A *dout = nullptr;
        const unsigned flags = sorted ? PN_RADIUS_SORTED : 0u;
        if constexpr (std::is_same<A, float>::value)
            check(pn_query_radius_with_distance_f32(h_, point, 1, len, (ptrdiff_t)len, distance, flags, off, &out, &dout));
        else
            check(pn_query_radius_with_distance_f64(h_, point, 1, len, (ptrdiff_t)len, distance, flags, off, &out, &dout));
        std::pair<std::vector<size_t>, std::vector<A>> r(std::vector<size_t>(out, out + off[1]),
                                                         std::vector<A>(dout, dout + off[1]));
        pn_free(out);
        pn_free(dout);
        return r;
    }
    // extension: a batch of points per call (row-major queries), results nq x min(k, n)
    void query_batch(const A *queries, size_t nq, size_t len, size_t k, uint64_t *idx_out, A *dist_out) const {
        if constexpr (std::is_same<A, float>::value)
            check(pn_query_f32(h_, queries, nq, len, (ptrdiff_t)len, k, idx_out, dist_out));
        else
            check(pn_query_f64(h_, queries, nq, len, (ptrdiff_t)len, k, idx_out, dist_out));
    }
    // extension: self-queries (pn_query_self_*): the k nearest OTHER rows of every indexed row, [n][kout] row-major with
    // kout = min(k, n - 1); include_self keeps each row in its own list (kout = min(k, n))
    std::pair<std::vector<size_t>, std::vector<A>> query_self(size_t k, bool include_self) const {
        const size_t cap = include_self ? n_ : n_ - 1;
        const size_t kout = k < cap ? k : cap;
        std::vector<uint64_t> idx(n_ * kout);
        std::vector<A> dist(n_ * kout);
        const unsigned flags = include_self ? PN_SELF_INCLUDE : 0u;
        if (kout) {
            if constexpr (kF32)
                check(pn_query_self_f32(h_, k, flags, idx.data(), dist.data()));
            else
                check(pn_query_self_f64(h_, k, flags, idx.data(), dist.data()));
        }
        return {std::vector<size_t>(idx.begin(), idx.end()), std::move(dist)};
    }
    // extension: { j != i : distance(p_i, p_j) < r } for every indexed row i (pn_query_radius_self_*) as CSR; dist stays
    // empty unless with_distance; sorted (needs with_distance): nearest first by (distance, index)
    SelfRadius<A> query_radius_self(A r, bool with_distance, bool sorted, bool include_self) const {
        SelfRadius<A> res;
        std::vector<uint64_t> off(n_ + 1, 0);
        uint64_t *out = nullptr;
        A *dout = nullptr;
        const unsigned flags = (sorted ? PN_RADIUS_SORTED : 0u) | (include_self ? PN_SELF_INCLUDE : 0u);
        if constexpr (kF32)
            check(pn_query_radius_self_f32(h_, r, flags, off.data(), &out, with_distance ? &dout : nullptr));
        else
            check(pn_query_radius_self_f64(h_, r, flags, off.data(), &out, with_distance ? &dout : nullptr));
        const uint64_t total = off[n_];
        res.offsets.assign(off.begin(), off.end());
        res.idx.assign(out, out + total);
        if (dout) res.dist.assign(dout, dout + total);
        pn_free(out);
        pn_free(dout);
        return res;
    }
    // extension: DBSCAN of the indexed rows on the device (pn_dbscan_*): labels[i] = the row's cluster (numbered by
    // ascending lowest core row; a border row takes the lowest-numbered cluster among its core neighbours) or -1 for
    // noise; core[i] = the row has at least min_samples rows within eps (strict '<', itself included)
    Dbscan dbscan(A eps, size_t min_samples) const {
        Dbscan res;
        res.labels.resize(n_);
        res.core.resize(n_);
        uint64_t ncl = 0;
        if constexpr (kF32)
            check(pn_dbscan_f32(h_, eps, min_samples, 0u, res.labels.data(), res.core.data(), &ncl));
        else
            check(pn_dbscan_f64(h_, eps, min_samples, 0u, res.labels.data(), res.core.data(), &ncl));
        res.n_clusters = (size_t)ncl;
        return res;
    }
    // extension: the minimum spanning tree of the indexed rows under mutual reachability (pn_mst_*): edge {i, j} weighs
    // max(distance(i, j), core[i], core[j]), edges are ordered by (weight, i, j), the tree is the unique one under that
    // strict order.  core: size() values, row i's core distance -- for HDBSCAN the distance to its min_samples-th nearest
    // OTHER row -- or nullptr for the plain Euclidean / Cosine MST (single linkage)
    Mst<A> mst(const A *core = nullptr) const {
        Mst<A> res;
        const size_t ne = n_ ? n_ - 1 : 0;
        std::vector<uint64_t> src(ne), dst(ne);
        res.weight.resize(ne);
        uint64_t work[2] = {0, 0};
        if constexpr (kF32)
            check(pn_mst_f32(h_, core, 0u, src.data(), dst.data(), res.weight.data(), work));
        else
            check(pn_mst_f64(h_, core, 0u, src.data(), dst.data(), res.weight.data(), work));
        res.src.assign(src.begin(), src.end());
        res.dst.assign(dst.begin(), dst.end());
        res.rounds = (size_t)work[0];
        res.rows_scanned = (size_t)work[1];
        return res;
    }
    // extension: the single-linkage dendrogram (pn_linkage_*) of a spanning tree's edges in merge order -- by default
    // those of mst(core).  Edges that are no spanning tree throw
    Linkage<A> linkage(const Mst<A> &tree) const {
        Linkage<A> res;
        const size_t ne = n_ ? n_ - 1 : 0;
        if (tree.src.size() != ne || tree.dst.size() != ne || tree.weight.size() != ne)
            throw std::invalid_argument("linkage: the tree must hold n - 1 edges");
        std::vector<uint64_t> src(tree.src.begin(), tree.src.end()), dst(tree.dst.begin(), tree.dst.end());
        std::vector<uint64_t> left(ne), right(ne), size(ne);
        res.weight.resize(ne);
        if constexpr (kF32)
            check(pn_linkage_f32(h_, src.data(), dst.data(), tree.weight.data(), 0u, left.data(), right.data(),
                                 res.weight.data(), size.data()));
        else
            check(pn_linkage_f64(h_, src.data(), dst.data(), tree.weight.data(), 0u, left.data(), right.data(),
                                 res.weight.data(), size.data()));
        res.left.assign(left.begin(), left.end());
        res.right.assign(right.begin(), right.end());
        res.size.assign(size.begin(), size.end());
        return res;
    }
    Linkage<A> linkage(const A *core = nullptr) const { return linkage(mst(core)); }
    // extension: HDBSCAN labels and membership probabilities on the device (pn_hdbscan_*).  min_samples counts OTHER rows
    // (scikit-learn's value minus one); 0 = min_cluster_size, capped at size() - 1
    Hdbscan<A> hdbscan(size_t min_cluster_size, size_t min_samples = 0) const {
        Hdbscan<A> res;
        if (min_samples == 0) min_samples = std::max<size_t>(std::min(min_cluster_size, n_ ? n_ - 1 : 0), 1);
        res.labels.resize(n_);
        res.probabilities.resize(n_);
        uint64_t ncl = 0;
        if constexpr (kF32)
            check(pn_hdbscan_f32(h_, min_samples, min_cluster_size, 0u, res.labels.data(), res.probabilities.data(), &ncl));
        else
            check(pn_hdbscan_f64(h_, min_samples, min_cluster_size, 0u, res.labels.data(), res.probabilities.data(), &ncl));
        res.n_clusters = (size_t)ncl;
        return res;
    }
    // extension: Local Outlier Factor on the device (pn_lof_*): scikit-learn's LocalOutlierFactor(n_neighbors = k), lof =
    // -negative_outlier_factor_; k counts OTHER rows, 1 <= k <= size() - 1
    Lof<A> lof(size_t k) const {
        Lof<A> res;
        res.lof.resize(n_);
        res.lrd.resize(n_);
        res.kdist.resize(n_);
        if constexpr (kF32)
            check(pn_lof_f32(h_, k, 0u, res.lof.data(), res.lrd.data(), res.kdist.data()));
        else
            check(pn_lof_f64(h_, k, 0u, res.lof.data(), res.lrd.data(), res.kdist.data()));
        return res;
    }
    // extension: the scores of nq new points (row-major, as long as the indexed rows) against a fit of the same k (pn_lof_score_*).  A
    // fitted row scored here finds itself at distance 0: it does not reproduce its fit score
    std::vector<double> lof_score(const A *queries, size_t nq, const Lof<A> &fit, size_t k) const {
        if (fit.lrd.size() != n_ || fit.kdist.size() != n_)
            throw std::invalid_argument("lof_score: the fit must hold one lrd and one kdist per indexed row");
        std::vector<double> score(nq);
        double none = 0.0;  // (nq = 0: the library still wants an address)
        double *out = nq ? score.data() : &none;
        if constexpr (kF32)
            check(pn_lof_score_f32(h_, queries, nq, dim_, (ptrdiff_t)dim_, k, fit.lrd.data(), fit.kdist.data(), 0u, out));
        else
            check(pn_lof_score_f64(h_, queries, nq, dim_, (ptrdiff_t)dim_, k, fit.lrd.data(), fit.kdist.data(), 0u, out));
        return score;
    }
    // extension: k-NN classification on the device (pn_knn_classify_*): scikit-learn's KNeighborsClassifier(n_neighbors = k).
    // labels: one class code in [0, n_classes) per indexed row; distance_weights: 1 / distance instead of uniform weights;
    // with_proba: also the class shares [nq][n_classes].  pred[q] = -1 for a poisoned list (a NaN distance; labels out of range are refused)
    KnnClasses knn_classify(const A *queries, size_t nq, size_t k, const std::vector<int64_t> &labels, size_t n_classes,
                            bool distance_weights = false, bool with_proba = false) const {
        if (labels.size() != n_) throw std::invalid_argument("knn_classify: one label per indexed row");
        KnnClasses res;
        res.pred.resize(nq);
        if (with_proba) res.proba.resize(nq * n_classes);
        int64_t none = 0;  // (nq = 0: the library still wants an address)
        const unsigned flags = distance_weights ? PN_KNN_WEIGHT_DISTANCE : 0u;
        if constexpr (kF32)
            check(pn_knn_classify_f32(h_, queries, nq, dim_, (ptrdiff_t)dim_, k, labels.data(), n_classes, flags,
                                      nq ? res.pred.data() : &none, with_proba ? res.proba.data() : nullptr));
        else
            check(pn_knn_classify_f64(h_, queries, nq, dim_, (ptrdiff_t)dim_, k, labels.data(), n_classes, flags,
                                      nq ? res.pred.data() : &none, with_proba ? res.proba.data() : nullptr));
        return res;
    }
    // the same for every indexed row from its k nearest OTHER rows (leave-one-out), 1 <= k <= size() - 1
    KnnClasses knn_classify_self(size_t k, const std::vector<int64_t> &labels, size_t n_classes, bool distance_weights = false,
                                 bool with_proba = false) const {
        if (labels.size() != n_) throw std::invalid_argument("knn_classify_self: one label per indexed row");
        KnnClasses res;
        res.pred.resize(n_);
        if (with_proba) res.proba.resize(n_ * n_classes);
        const unsigned flags = distance_weights ? PN_KNN_WEIGHT_DISTANCE : 0u;
        if constexpr (kF32)
            check(pn_knn_classify_self_f32(h_, k, labels.data(), n_classes, flags, res.pred.data(),
                                           with_proba ? res.proba.data() : nullptr));
        else
            check(pn_knn_classify_self_f64(h_, k, labels.data(), n_classes, flags, res.pred.data(),
                                           with_proba ? res.proba.data() : nullptr));
        return res;
    }
    // extension: k-NN regression on the device (pn_knn_regress_*): scikit-learn's KNeighborsRegressor(n_neighbors = k).
    // targets: [size()][n_out] row-major; the answer is [nq][n_out]
    std::vector<double> knn_regress(const A *queries, size_t nq, size_t k, const std::vector<double> &targets, size_t n_out,
                                    bool distance_weights = false) const {
        if (n_out == 0 || targets.size() != n_ * n_out)
            throw std::invalid_argument("knn_regress: targets must hold n_out >= 1 values per indexed row");
        std::vector<double> out(nq * n_out);
        double none = 0.0;
        const unsigned flags = distance_weights ? PN_KNN_WEIGHT_DISTANCE : 0u;
        if constexpr (kF32)
            check(pn_knn_regress_f32(h_, queries, nq, dim_, (ptrdiff_t)dim_, k, targets.data(), n_out, flags,
                                     nq ? out.data() : &none));
        else
            check(pn_knn_regress_f64(h_, queries, nq, dim_, (ptrdiff_t)dim_, k, targets.data(), n_out, flags,
                                     nq ? out.data() : &none));
        return out;
    }
    std::vector<double> knn_regress_self(size_t k, const std::vector<double> &targets, size_t n_out,
                                         bool distance_weights = false) const {
        if (n_out == 0 || targets.size() != n_ * n_out)
            throw std::invalid_argument("knn_regress_self: targets must hold n_out >= 1 values per indexed row");
        std::vector<double> out(n_ * n_out);
        const unsigned flags = distance_weights ? PN_KNN_WEIGHT_DISTANCE : 0u;
        if constexpr (kF32)
            check(pn_knn_regress_self_f32(h_, k, targets.data(), n_out, flags, out.data()));
        else
            check(pn_knn_regress_self_f64(h_, k, targets.data(), n_out, flags, out.data()));
        return out;
    }
    // extension: kernel density sums on the device (pn_kde_*): per query the raw sum of `kernel` (PN_KDE_*) with bandwidth
    // h over the rows within the kernel's cutoff, in a fixed order; atol lets the two smooth kernels stop at a finite
    // cutoff (sum_all - atol <= sum <= sum_all), atol = 0 visits every row.  Normalisation is the caller's
    Kde<A> kernel_density(const A *queries, size_t nq, A h, int kernel = PN_KDE_GAUSSIAN, double atol = 0.0) const {
        return kernel_density(queries, nq, &h, 1, kernel, atol);
    }
    // ... with one bandwidth per query (n_h = nq; the balloon estimator) or one for all (n_h = 1)
    Kde<A> kernel_density(const A *queries, size_t nq, const A *h, size_t n_h, int kernel = PN_KDE_GAUSSIAN,
                          double atol = 0.0) const {
        Kde<A> res;
        res.sum.resize(nq);
        res.cutoff.resize(nq);
        std::vector<uint64_t> cnt(nq);
        double none = 0.0;  // (nq = 0: the library still wants an address)
        double *out = nq ? res.sum.data() : &none;
        if constexpr (kF32)
            check(pn_kde_f32(h_, queries, nq, dim_, (ptrdiff_t)dim_, h, n_h, kernel, atol, 0u, out, cnt.data(), res.cutoff.data()));
        else
            check(pn_kde_f64(h_, queries, nq, dim_, (ptrdiff_t)dim_, h, n_h, kernel, atol, 0u, out, cnt.data(), res.cutoff.data()));
        res.count.assign(cnt.begin(), cnt.end());
        return res;
    }
    // extension: the same for the indexed rows themselves (pn_kde_self_*); by default each row is left out of its own sum
    // (the leave-one-out density)
    Kde<A> kernel_density_self(A h, int kernel = PN_KDE_GAUSSIAN, double atol = 0.0, bool include_self = false) const {
        Kde<A> res;
        res.sum.resize(n_);
        res.cutoff.resize(n_);
        std::vector<uint64_t> cnt(n_);
        const unsigned flags = include_self ? PN_SELF_INCLUDE : 0u;
        if constexpr (kF32)
            check(pn_kde_self_f32(h_, &h, 1, kernel, atol, flags, res.sum.data(), cnt.data(), res.cutoff.data()));
        else
            check(pn_kde_self_f64(h_, &h, 1, kernel, atol, flags, res.sum.data(), cnt.data(), res.cutoff.data()));
        res.count.assign(cnt.begin(), cnt.end());
        return res;
    }
    // extension: the number of rows with distance < r (strict) per query; only the counting pass runs, no list is written
    std::vector<size_t> query_radius_count(const A *queries, size_t nq, A r) const {
        std::vector<uint64_t> cnt(nq);
        uint64_t none = 0;
        uint64_t *out = nq ? cnt.data() : &none;
        if constexpr (kF32)
            check(pn_kde_f32(h_, queries, nq, dim_, (ptrdiff_t)dim_, &r, 1, PN_KDE_TOPHAT, 0.0, 0u, nullptr, out, nullptr));
        else
            check(pn_kde_f64(h_, queries, nq, dim_, (ptrdiff_t)dim_, &r, 1, PN_KDE_TOPHAT, 0.0, 0u, nullptr, out, nullptr));
        return std::vector<size_t>(cnt.begin(), cnt.end());
    }
    // extension: mean shift on the device (pn_mean_shift_*; scikit-learn's MeanShift with its flat kernel, every radius a
    // strict '<').  mean_shift_modes moves the seeds (seeds == nullptr: every indexed row) to their modes; only the seeds
    // still moving are queried.  tol < 0: 1e-3 * h
    MeanShift<A> mean_shift_modes(A h, const A *seeds = nullptr, size_t ns = 0, double tol = -1.0, size_t max_iter = 300) const {
        MeanShift<A> res;
        const bool rows = seeds == nullptr;
        if (rows) ns = n_;
        res.modes.resize(ns * dim_ + 1);
        res.iterations.resize(ns + 1);
        res.shift.resize(ns + 1);
        std::vector<uint64_t> pw(ns + 1);
        uint64_t work[2] = {0, 0};
        if (tol < 0.0) tol = 1e-3 * (double)h;
        const unsigned flags = rows ? (unsigned)PN_MS_SEED_ROWS : 0u;
        if constexpr (kF32)
            check(pn_mean_shift_f32(h_, seeds, rows ? 0 : ns, dim_, (ptrdiff_t)dim_, &h, 1, tol, max_iter, flags, res.modes.data(),
                                    pw.data(), res.iterations.data(), res.shift.data(), work));
        else
            check(pn_mean_shift_f64(h_, seeds, rows ? 0 : ns, dim_, (ptrdiff_t)dim_, &h, 1, tol, max_iter, flags, res.modes.data(),
                                    pw.data(), res.iterations.data(), res.shift.data(), work));
        res.modes.resize(ns * dim_);
        res.iterations.resize(ns);
        res.shift.resize(ns);
        res.points_within.assign(pw.begin(), pw.begin() + ns);
        res.n_iter = (size_t)work[0];
        res.seed_steps = (size_t)work[1];
        return res;
    }
    // ... the merge of res.modes into res.centres (ranked by points_within descending, then seed number)
    void mean_shift_merge(MeanShift<A> &res, A h) const {
        const size_t ns = res.points_within.size();
        std::vector<uint64_t> pw(res.points_within.begin(), res.points_within.end()), cp(ns + 1);
        res.centres.resize(ns * dim_ + 1);
        res.centre_of_seed.resize(ns + 1);
        uint64_t nc = 0;
        if constexpr (kF32)
            check(pn_mean_shift_merge_f32(h_, res.modes.data(), ns, pw.data(), h, 0u, res.centres.data(), cp.data(),
                                          res.centre_of_seed.data(), &nc));
        else
            check(pn_mean_shift_merge_f64(h_, res.modes.data(), ns, pw.data(), h, 0u, res.centres.data(), cp.data(),
                                          res.centre_of_seed.data(), &nc));
        res.n_centres = (size_t)nc;
        res.centres.resize(res.n_centres * dim_);
        res.centre_of_seed.resize(ns);
        res.centre_points.assign(cp.begin(), cp.begin() + res.n_centres);
    }
    // ... the nearest centre of every indexed row; cluster_all = false: -1 unless it is within h
    void mean_shift_labels(MeanShift<A> &res, A h, bool cluster_all = true) const {
        res.labels.resize(n_ + 1);
        const unsigned flags = cluster_all ? 0u : (unsigned)PN_MS_ORPHANS;
        if constexpr (kF32)
            check(pn_mean_shift_labels_f32(h_, res.centres.data(), res.n_centres, h, flags, res.labels.data()));
        else
            check(pn_mean_shift_labels_f64(h_, res.centres.data(), res.n_centres, h, flags, res.labels.data()));
        res.labels.resize(n_);
    }
    // ... the three in a row: scikit-learn's MeanShift(bandwidth = h, seeds, cluster_all).fit(rows)
    MeanShift<A> mean_shift(A h, const A *seeds = nullptr, size_t ns = 0, bool cluster_all = true, double tol = -1.0,
                            size_t max_iter = 300) const {
        MeanShift<A> res = mean_shift_modes(h, seeds, ns, tol, max_iter);
        mean_shift_merge(res, h);
        mean_shift_labels(res, h, cluster_all);
        return res;
    }
    // extension: k-means on the device (pn_kmeans_*).  kmeans_assign: the nearest of k centres [k][dim] for every indexed
    // row, the labels of mean_shift_labels, with distances and inertia
    KMeans<A> kmeans_assign(const A *centres, size_t k) const {
        KMeans<A> res;
        res.centres.assign(centres, centres + k * dim_);
        res.labels.resize(n_ + 1);
        res.dist.resize(n_ + 1);
        if constexpr (kF32)
            check(pn_kmeans_assign_f32(h_, centres, k, 0u, res.labels.data(), res.dist.data(), &res.inertia));
        else
            check(pn_kmeans_assign_f64(h_, centres, k, 0u, res.labels.data(), res.dist.data(), &res.inertia));
        res.labels.resize(n_);
        res.dist.resize(n_);
        return res;
    }
    // ... Lloyd iterations from the initial centres [k][dim] until the summed squared moves are <= tol (absolute) or
    // max_iter; a cluster without members keeps its centre
    KMeans<A> kmeans(const A *init, size_t k, double tol, size_t max_iter = 300) const {
        KMeans<A> res;
        res.centres.resize(k * dim_ + 1);
        res.labels.resize(n_ + 1);
        res.dist.resize(n_ + 1);
        std::vector<uint64_t> counts(k + 1);
        uint64_t iters = 0;
        if constexpr (kF32)
            check(pn_kmeans_f32(h_, init, k, tol, max_iter, 0u, res.centres.data(), res.labels.data(), res.dist.data(),
                                counts.data(), &res.inertia, &iters, &res.shift2));
        else
            check(pn_kmeans_f64(h_, init, k, tol, max_iter, 0u, res.centres.data(), res.labels.data(), res.dist.data(),
                                counts.data(), &res.inertia, &iters, &res.shift2));
        res.centres.resize(k * dim_);
        res.labels.resize(n_);
        res.dist.resize(n_);
        res.counts.assign(counts.begin(), counts.begin() + k);
        res.n_iter = (size_t)iters;
        return res;
    }
    // extension: OPTICS on the device (pn_optics_*): scikit-learn's OPTICS(min_samples + 1, max_eps) on this library's
    // distances; min_samples counts OTHER rows, every radius is a strict '<'
    Optics<A> optics(size_t min_samples, A max_eps = std::numeric_limits<A>::infinity()) const {
        Optics<A> res;
        std::vector<uint64_t> ord(n_);
        res.reachability.resize(n_);
        res.core_distances.resize(n_);
        res.predecessor.resize(n_);
        if constexpr (kF32)
            check(pn_optics_f32(h_, min_samples, max_eps, 0u, ord.data(), res.reachability.data(), res.predecessor.data(),
                                res.core_distances.data()));
        else
            check(pn_optics_f64(h_, min_samples, max_eps, 0u, ord.data(), res.reachability.data(), res.predecessor.data(),
                                res.core_distances.data()));
        res.ordering.assign(ord.begin(), ord.end());
        return res;
    }
    // extension: the DBSCAN labels at eps (<= the ordering's max_eps) read off an ordering (pn_optics_dbscan_*): clusters
    // numbered by first appearance in the ordering, -1 = noise.  An ordering that is no permutation of the rows throws
    OpticsDbscan optics_dbscan(const Optics<A> &o, A eps) const {
        if (o.ordering.size() != n_ || o.reachability.size() != n_ || o.core_distances.size() != n_)
            throw std::invalid_argument("optics_dbscan: the ordering must hold one entry per indexed row");
        OpticsDbscan res;
        std::vector<uint64_t> ord(o.ordering.begin(), o.ordering.end());
        res.labels.resize(n_);
        uint64_t ncl = 0;
        if constexpr (kF32)
            check(pn_optics_dbscan_f32(h_, ord.data(), o.reachability.data(), o.core_distances.data(), eps, 0u,
                                       res.labels.data(), &ncl));
        else
            check(pn_optics_dbscan_f64(h_, ord.data(), o.reachability.data(), o.core_distances.data(), eps, 0u,
                                       res.labels.data(), &ncl));
        res.n_clusters = (size_t)ncl;
        return res;
    }
    // extension: one radius per row (pn_query_radii_self_*): radii [size()], row i's list is the scalar overload's for
    // r = radii[i].  (Taken for pointer arguments only: a literal 0 or NULL stays a call of the scalar overload.)
    template <typename P, typename = typename std::enable_if<std::is_pointer<P>::value &&
                                                             std::is_convertible<P, const A *>::value>::type>
    SelfRadius<A> query_radius_self(P radii, bool with_distance, bool sorted, bool include_self) const {
        std::vector<uint64_t> off(n_ + 1, 0);
        uint64_t *out = nullptr;
        A *dout = nullptr;
        const unsigned flags = (sorted ? PN_RADIUS_SORTED : 0u) | (include_self ? PN_SELF_INCLUDE : 0u);
        if constexpr (kF32)
            check(pn_query_radii_self_f32(h_, radii, flags, off.data(), &out, with_distance ? &dout : nullptr));
        else
            check(pn_query_radii_self_f64(h_, radii, flags, off.data(), &out, with_distance ? &dout : nullptr));
        return take_csr(off, out, dout);
    }
    // extension: nq queries of `len` elements (contiguous rows), one radius each (pn_query_radii_*): list q is
    // query_radius / query_radius_with_distance(queries + q * len, len, radii[q], sorted); the same CSR struct
    SelfRadius<A> query_radii(const A *queries, size_t nq, size_t len, const A *radii, bool with_distance,
                              bool sorted) const {
        std::vector<uint64_t> off(nq + 1, 0);
        uint64_t *out = nullptr;
        A *dout = nullptr;
        const unsigned flags = sorted ? PN_RADIUS_SORTED : 0u;
        if constexpr (kF32)
            check(pn_query_radii_f32(h_, queries, nq, len, (ptrdiff_t)len, radii, flags, off.data(), &out,
                                     with_distance ? &dout : nullptr));
        else
            check(pn_query_radii_f64(h_, queries, nq, len, (ptrdiff_t)len, radii, flags, off.data(), &out,
                                     with_distance ? &dout : nullptr));
        return take_csr(off, out, dout);
    }
    pn_index *handle() const { return h_; }

  private:
    // a library-allocated CSR answer (offsets, lists, distances or NULL) into vectors; the lists are freed
    static SelfRadius<A> take_csr(const std::vector<uint64_t> &off, uint64_t *out, A *dout) {
        SelfRadius<A> res;
        const uint64_t total = off.back();
        res.offsets.assign(off.begin(), off.end());
        if (out) res.idx.assign(out, out + total);
        if (dout) res.dist.assign(dout, dout + total);
        pn_free(out);
        pn_free(dout);
        return res;
    }
};

// VantagePointTree (src/vantage_point_tree.rs:13-98): the reference's second index answers 1-NN only and returns the
// neighbour BallTree::query_nearest returns; on this engine both are the k = 1 case of the same exact scan.
template <typename A>
class VantagePointTree {
    BallTree<A> tree_;
    explicit VantagePointTree(BallTree<A> &&t) : tree_(std::move(t)) {}

  public:
    // VantagePointTree::euclidean / ::new (src/vantage_point_tree.rs:31-72): the same ArrayError cases as BallTree::new
    static VantagePointTree euclidean(const A *points, size_t rows, size_t cols, ptrdiff_t row_stride = -1,
                                      ptrdiff_t col_stride = 1, int device = 0) {
        return VantagePointTree(BallTree<A>::euclidean(points, rows, cols, row_stride, col_stride, device));
    }
    // query_nearest (src/vantage_point_tree.rs:88-98)
    std::pair<size_t, A> query_nearest(const A *point, size_t len) const { return tree_.query_nearest(point, len); }
};

// Row-sharded BallTree<A, Euclidean> over several GPUs driven by this process (petal_mi355x.h, pn_sharded_*): shard g of
// devices.size() lives on devices[g]; one RCCL all-gather per query batch; answers equal the single-index answers.
// A = float | double (the reference is generic over A, src/ball_tree.rs:26-30).
namespace detail {
inline int sh_create(const float *p, size_t r, size_t c, ptrdiff_t rs, ptrdiff_t cs, const int *d, int n, pn_sharded **o) {
    return pn_sharded_create_f32(p, r, c, rs, cs, d, n, o);
}
inline int sh_create(const double *p, size_t r, size_t c, ptrdiff_t rs, ptrdiff_t cs, const int *d, int n, pn_sharded **o) {
    return pn_sharded_create_f64(p, r, c, rs, cs, d, n, o);
}
inline int sh_query(const pn_sharded *h, const float *q, size_t nq, size_t len, size_t k, uint64_t *i, float *d) {
    return pn_sharded_query_f32(h, q, nq, len, (ptrdiff_t)len, k, i, d);
}
inline int sh_query(const pn_sharded *h, const double *q, size_t nq, size_t len, size_t k, uint64_t *i, double *d) {
    return pn_sharded_query_f64(h, q, nq, len, (ptrdiff_t)len, k, i, d);
}
inline int sh_radius(const pn_sharded *h, const float *q, size_t len, float r, uint64_t *off, uint64_t **out) {
    return pn_sharded_query_radius_f32(h, q, 1, len, (ptrdiff_t)len, r, off, out);
}
inline int sh_radius(const pn_sharded *h, const double *q, size_t len, double r, uint64_t *off, uint64_t **out) {
    return pn_sharded_query_radius_f64(h, q, 1, len, (ptrdiff_t)len, r, off, out);
}
inline int sh_radius_wd(const pn_sharded *h, const float *q, size_t len, float r, unsigned fl, uint64_t *off, uint64_t **out,
                        float **dout) {
    return pn_sharded_query_radius_with_distance_f32(h, q, 1, len, (ptrdiff_t)len, r, fl, off, out, dout);
}
inline int sh_radius_wd(const pn_sharded *h, const double *q, size_t len, double r, unsigned fl, uint64_t *off,
                        uint64_t **out, double **dout) {
    return pn_sharded_query_radius_with_distance_f64(h, q, 1, len, (ptrdiff_t)len, r, fl, off, out, dout);
}
}  // namespace detail
template <typename A>
class ShardedBallTreeT {
    pn_sharded *h_ = nullptr;
    size_t n_ = 0;

  public:
    ShardedBallTreeT(const A *points, size_t rows, size_t cols, const std::vector<int> &devices,
                     ptrdiff_t row_stride = -1, ptrdiff_t col_stride = 1)
        : n_(rows) {
        if (row_stride < 0) row_stride = (ptrdiff_t)cols;
        check(detail::sh_create(points, rows, cols, row_stride, col_stride, devices.data(), (int)devices.size(), &h_));
    }
    ShardedBallTreeT(const ShardedBallTreeT &) = delete;
    ~ShardedBallTreeT() { pn_sharded_destroy(h_); }
    size_t num_points() const { return n_; }
    std::pair<std::vector<size_t>, std::vector<A>> query(const A *point, size_t len, size_t k) const {
        const size_t kout = k < n_ ? k : n_;
        std::vector<uint64_t> idx(kout);
        std::vector<A> dist(kout);
        check(detail::sh_query(h_, point, 1, len, k, idx.data(), dist.data()));
        return {std::vector<size_t>(idx.begin(), idx.end()), std::move(dist)};
    }
    void query_batch(const A *queries, size_t nq, size_t len, size_t k, uint64_t *idx_out, A *dist_out) const {
        check(detail::sh_query(h_, queries, nq, len, k, idx_out, dist_out));
    }
    std::vector<size_t> query_radius(const A *point, size_t len, A distance) const {
        uint64_t off[2] = {0, 0};
        uint64_t *out = nullptr;
        check(detail::sh_radius(h_, point, len, distance, off, &out));
        std::vector<size_t> v(out, out + off[1]);
        pn_free(out);
        return v;
    }
    // query_radius_with_distance over all shards (global rows); nearest first by (distance, row) with sorted = true
    std::pair<std::vector<size_t>, std::vector<A>> query_radius_with_distance(const A *point, size_t len, A distance,
                                                                              bool sorted) const {
        uint64_t off[2] = {0, 0};
        uint64_t *out = nullptr;
        A *dout = nullptr;
        check(detail::sh_radius_wd(h_, point, len, distance, sorted ? PN_RADIUS_SORTED : 0u, off, &out, &dout));
        std::pair<std::vector<size_t>, std::vector<A>> r(std::vector<size_t>(out, out + off[1]),
                                                         std::vector<A>(dout, dout + off[1]));
        pn_free(out);
        pn_free(dout);
        return r;
    }
    // self-queries over the shards (pn_sharded_query_self_*): BallTreeT::query_self of the whole corpus, global rows
    std::pair<std::vector<size_t>, std::vector<A>> query_self(size_t k, bool include_self) const {
        const size_t cap = include_self ? n_ : n_ - 1;
        const size_t kout = k < cap ? k : cap;
        std::vector<uint64_t> idx(n_ * kout);
        std::vector<A> dist(n_ * kout);
        const unsigned flags = include_self ? PN_SELF_INCLUDE : 0u;
        if (kout) {
            if constexpr (std::is_same<A, float>::value)
                check(pn_sharded_query_self_f32(h_, k, flags, idx.data(), dist.data()));
            else
                check(pn_sharded_query_self_f64(h_, k, flags, idx.data(), dist.data()));
        }
        return {std::vector<size_t>(idx.begin(), idx.end()), std::move(dist)};
    }
    // pn_sharded_query_radius_self_*: BallTreeT::query_radius_self of the whole corpus, global rows
    SelfRadius<A> query_radius_self(A r, bool with_distance, bool sorted, bool include_self) const {
        SelfRadius<A> res;
        std::vector<uint64_t> off(n_ + 1, 0);
        uint64_t *out = nullptr;
        A *dout = nullptr;
        const unsigned flags = (sorted ? PN_RADIUS_SORTED : 0u) | (include_self ? PN_SELF_INCLUDE : 0u);
        if constexpr (std::is_same<A, float>::value)
            check(pn_sharded_query_radius_self_f32(h_, r, flags, off.data(), &out, with_distance ? &dout : nullptr));
        else
            check(pn_sharded_query_radius_self_f64(h_, r, flags, off.data(), &out, with_distance ? &dout : nullptr));
        const uint64_t total = off[n_];
        res.offsets.assign(off.begin(), off.end());
        res.idx.assign(out, out + total);
        if (dout) res.dist.assign(dout, dout + total);
        pn_free(out);
        pn_free(dout);
        return res;
    }
};
using ShardedBallTree = ShardedBallTreeT<float>;

}  // namespace petal
