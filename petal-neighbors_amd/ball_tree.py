"""Host mirror of ``petal_neighbors::BallTree`` (reference src/ball_tree.rs:15-374).

Same constructor names, argument meaning, result shapes and error behaviour as
the Rust type, so tests read like the reference's own; the work is done by the
HIP kernels behind the C ABI (``include/petal_mi355x.h``).  The ball tree walk
is not reproduced: ``BallTree`` here owns a zero-padded copy of the points in
HBM and answers queries by batched exact scans.

Batch methods (``query_batch`` etc.) are extensions: the reference takes one
point per call (src/ball_tree.rs:102); ``nq = 1`` is that call.  The searches
shared with ``ShardedIndex`` and every argument helper live in ``_binding.Handle``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._binding import ENGINES, NP, Handle, stream_arg, suffix  # noqa: F401  (ENGINES: part of this module's names)
from .distance import Cosine, Euclidean
from .errors import NotContiguous, check


def _float_array(a):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):  # `A: FloatCore` is f32 or f64 in practice
        a = a.astype(np.float64)
    return a


KDE_KERNELS = {"gaussian": _lib.PN_KDE_GAUSSIAN, "tophat": _lib.PN_KDE_TOPHAT, "epanechnikov": _lib.PN_KDE_EPANECHNIKOV,
               "exponential": _lib.PN_KDE_EXPONENTIAL, "linear": _lib.PN_KDE_LINEAR}
KNN_WEIGHTS = {"uniform": 0, "distance": _lib.PN_KNN_WEIGHT_DISTANCE}


def _log_vn(d):
    """log of the volume of the unit ball in ``d`` dimensions"""
    return 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1.0)


def _log_sn(d):
    """log of the surface of the unit sphere in ``d + 1`` dimensions"""
    return math.log(2.0 * math.pi) + _log_vn(d - 1)


def kde_log_norm(kernel: str, dim: int, h):
    """log of the normaliser of ``kernel`` with bandwidth ``h`` (scalar or array) in ``dim`` dimensions: the density is
    ``exp(kde_log_norm) * sum / n``.  The closed forms are scikit-learn's (``_kde_norm`` of its ball tree)."""
    if kernel not in KDE_KERNELS:
        raise ValueError(f"unknown kernel {kernel!r}: one of {sorted(KDE_KERNELS)}")
    d = int(dim)
    if kernel == "gaussian":
        factor = 0.5 * d * math.log(2.0 * math.pi)
    elif kernel == "tophat":
        factor = _log_vn(d)
    elif kernel == "epanechnikov":
        factor = _log_vn(d) + math.log(2.0 / (d + 2.0))
    elif kernel == "exponential":
        factor = _log_sn(d - 1) + math.lgamma(d)
    else:
        factor = _log_vn(d) - math.log(d + 1.0)
    return -factor - d * np.log(np.asarray(h, dtype=np.float64))


def mean_shift_bin_seeds(X, bin_size, min_bin_freq: int = 1):
    """Seeds for ``BallTree.mean_shift`` on a grid of cell size ``bin_size``: the centres of the cells that hold at least
    ``min_bin_freq`` rows of ``X``, the same set of rows as scikit-learn's ``get_bin_seeds`` (``X`` itself when
    ``bin_size`` is 0, or when every row is a cell of its own)."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be 2-D")
    if not (float(bin_size) >= 0.0):
        raise ValueError("bin_size must be >= 0")
    if bin_size == 0:
        return X
    cells, counts = np.unique(np.round(X / bin_size), axis=0, return_counts=True)
    seeds = cells[counts >= min_bin_freq].astype(np.float32)  # (scikit-learn keeps its cell points in float32)
    if seeds.shape[0] == X.shape[0]:
        return X
    return seeds * bin_size


class BallTree(Handle):
    """``BallTree<'a, A, Euclidean>``: ``points`` / ``metric`` stay readable like the pub fields
    at src/ball_tree.rs:20-23 (``idx`` and ``nodes`` do not exist: no tree is built)."""

    def __init__(self, handle, points, metric, dtype, device):
        self._h = C.c_void_p(handle)
        self.points = points
        self.metric = metric
        self.dtype = np.dtype(dtype)
        self.device = device
        self._sfx = suffix(self.dtype)
        info = _lib.PnInfo()
        check(_lib.lib().pn_index_info(self._h, C.byref(info)))
        self._n, self._dim = int(info.n_points), int(info.dim)
        self.mfma_eligible = bool(info.mfma_eligible)
        self.bf16_eligible = bool(info.bf16_eligible)
        self.bf16_layout = int(info.bf16_layout)
        self.seed_model = bool(info.seed_model)

    @property
    def _total(self):
        return self._n

    _rows = _total  # every indexed row answers a self-query

    # ------------------------------------------------------------ construction
    @classmethod
    def new(cls, points, metric, device: int = 0):
        """``BallTree::new(points, metric)`` (src/ball_tree.rs:38-63).

        Raises ``ArrayError.Empty`` for zero rows and ``ArrayError.NotContiguous`` when the
        inner stride is not 1 (only the inner stride is checked, as at :47)."""
        if not isinstance(metric, (Euclidean, Cosine)):
            raise NotImplementedError("the MI355X path serves distance.Euclidean and distance.Cosine")
        a = _float_array(points)
        if a.ndim != 2:
            raise ValueError("points must be a 2-D array (Ix2)")
        n, d = a.shape
        item = a.itemsize
        rs, cs = (a.strides[0] // item, a.strides[1] // item)
        if a.strides[0] % item or a.strides[1] % item or (n > 1 and rs < 0):
            a = np.ascontiguousarray(a)  # exotic views: ndarray would accept them; copy, same values
            rs, cs = d, 1
        if d <= 1:
            cs = 1
            if d == 1 and a.strides[1] != item:
                a = np.ascontiguousarray(a)
                rs = d
        h = C.c_void_p(0)
        # Cosine: an exact scan under Cosine::distance (it is not a metric: the reference's pruned walk can miss true
        # neighbours under it; include/petal_mi355x.h, pn_index_create_cosine_*)
        stem = "pn_index_create_cosine_" if isinstance(metric, Cosine) else "pn_index_create_"
        check(getattr(_lib.lib(), stem + suffix(a.dtype))(a.ctypes.data if a.size else None, n, d, rs, cs, device,
                                                           C.byref(h)))
        return cls(h.value, a, metric, a.dtype, device)

    @classmethod
    def euclidean(cls, points, device: int = 0):
        """``BallTree::euclidean(points)`` (src/ball_tree.rs:367-373)."""
        return cls.new(points, Euclidean(), device)

    @classmethod
    def from_device(cls, tensor, stream=None):
        """Build from a row-major float32 or float64 CUDA tensor already in HBM (extension)."""
        import torch
        if tensor.dtype not in (torch.float32, torch.float64) or tensor.dim() != 2 or not tensor.is_cuda:
            raise ValueError("from_device takes a 2-D float32 or float64 CUDA tensor")
        if tensor.shape[1] > 1 and tensor.stride(1) != 1:
            raise NotContiguous()
        n, d = tensor.shape
        dev = tensor.device.index or 0
        h = C.c_void_p(0)
        sfx = suffix(tensor.dtype)
        check(getattr(_lib.lib(), "pn_index_create_device_" + sfx)(
            tensor.data_ptr() if n * d else None, n, d, tensor.stride(0) if n > 1 else max(d, 1), dev,
            stream_arg(stream, tensor.device), C.byref(h)))
        return cls(h.value, None, Euclidean(), NP[sfx], dev)

    # ---------------------------------------------------------------- accessors
    def num_points(self) -> int:
        """``BallTree::num_points`` (src/ball_tree.rs:351-353)."""
        return self._n

    @property
    def dim(self) -> int:
        return self._dim

    # Tree introspection (src/ball_tree.rs:296-353).  No tree exists until one of these is called; the library then
    # builds the reference's implicit ball tree once, on the host (csrc/tree.cpp) -- queries never use it.
    def num_nodes(self) -> int:
        """``BallTree::num_nodes`` (src/ball_tree.rs:345-348)."""
        out = C.c_uint64(0)
        check(_lib.lib().pn_tree_num_nodes(self._h, C.byref(out)))
        return int(out.value)

    def _node(self, n):
        n = int(n)
        if n < 0 or n >= self.num_nodes():
            raise IndexError(f"node {n} out of range")  # the reference panics
        return n

    def children_of(self, n: int):
        """``BallTree::children_of(n) -> Option<(usize, usize)>`` (src/ball_tree.rs:320-329): None for a leaf."""
        some, left, right = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        check(_lib.lib().pn_tree_children_of(self._h, self._node(n), C.byref(some), C.byref(left), C.byref(right)))
        return (int(left.value), int(right.value)) if some.value else None

    def points_of(self, n: int):
        """``BallTree::points_of(n) -> &[usize]`` (src/ball_tree.rs:331-334): the node's slice of ``idx``."""
        ptr, cnt = C.POINTER(C.c_uint64)(), C.c_uint64(0)
        check(_lib.lib().pn_tree_points_of(self._h, self._node(n), C.byref(ptr), C.byref(cnt)))
        return np.ctypeslib.as_array(ptr, shape=(int(cnt.value),)).copy() if cnt.value else np.empty(0, dtype=np.uint64)

    def radius_of(self, n: int):
        """``BallTree::radius_of(n)`` (src/ball_tree.rs:336-339)."""
        out = self._real(0)
        check(self._fn("tree_radius_of")(self._h, self._node(n), C.byref(out)))
        return self.dtype.type(out.value)

    def compare_nodes(self, x: int, y: int):
        """``BallTree::compare_nodes(x, y) -> Option<Ordering>`` by radius (src/ball_tree.rs:340-343):
        -1 / 0 / 1 for Less / Equal / Greater, None when a radius is NaN."""
        out = C.c_int(0)
        check(_lib.lib().pn_tree_compare_nodes(self._h, self._node(x), self._node(y), C.byref(out)))
        return None if out.value == 2 else int(out.value)

    def node_distance_lower_bound(self, n1: int, n2: int):
        """``BallTree::node_distance_lower_bound(n1, n2)`` = max(|c1 - c2| - R1 - R2, 0) (src/ball_tree.rs:303-318)."""
        out = self._real(0)
        check(self._fn("tree_node_distance_lower_bound")(self._h, self._node(n1), self._node(n2), C.byref(out)))
        return self.dtype.type(out.value)

    def _centroid_of(self, n: int):
        c = np.empty(self._dim, dtype=self.dtype)
        check(_lib.lib().pn_tree_centroid_of(self._h, self._node(n), c.ctypes.data))
        return c

    # ------------------------------------------------------------------ queries
    # (query_batch, the radius searches, the device forms and the self-queries: ``_binding.Handle``)
    def query(self, point, k: int):
        """``BallTree::query(point, k) -> (Vec<usize>, Vec<A>)`` ascending (src/ball_tree.rs:102-121);
        ``k == 0`` returns two empty arrays (:106-108)."""
        idx, dist = self._knn(self._queries(point, True), k)
        return idx[0], dist[0]

    def query_nearest(self, point):
        """``BallTree::query_nearest(point) -> (usize, A)`` (src/ball_tree.rs:80-86)."""
        a = self._queries(point, True)
        idx = np.empty(1, dtype=np.uint64)
        dist = np.empty(1, dtype=self.dtype)
        check(self._fn("query_nearest")(self._h, a.ctypes.data, 1, a.shape[1], max(a.shape[1], 1), idx.ctypes.data,
                                        dist.ctypes.data))
        return int(idx[0]), dist[0]

    def query_radius(self, point, distance):
        """``BallTree::query_radius(point, distance) -> Vec<usize>`` (src/ball_tree.rs:137-142).
        The reference's order is unspecified (its tests sort, :667/:777); here: ascending."""
        return self._radius(self._queries(point, True), distance)[1]

    def query_radius_with_distance(self, point, distance, sort: bool = False):
        """``query_radius(point, distance)`` and the distance of each neighbour: ``(idx, dist)``, ascending by index, or
        nearest first (by (distance, index)) with ``sort=True``."""
        _, idx, dist = self.query_radius_with_distance_batch(self._queries(point, True), distance, sort)
        return idx, dist

    # ------------------------------------------------------------------- DBSCAN
    def _dbscan_args(self, eps, min_samples):
        if int(min_samples) < 1:
            raise ValueError("min_samples must be >= 1")
        return self._real(eps), int(min_samples)

    def dbscan(self, eps, min_samples: int):
        """DBSCAN of the indexed rows on the device (``pn_dbscan_*``): ``(labels int64 [n], core bool [n])``.  Row i's
        neighbourhood is ``{ j : distance(p_i, p_j) < eps }`` (itself included where its own distance is below eps), a
        core row has at least ``min_samples`` of them, clusters are numbered by ascending lowest core row, a border row
        takes the lowest-numbered cluster among its core neighbours, noise is -1."""
        e, m = self._dbscan_args(eps, min_samples)
        labels = np.empty(self._n, dtype=np.int64)
        core = np.empty(self._n, dtype=np.uint8)
        check(self._fn("dbscan")(self._h, e, m, 0, labels.ctypes.data, core.ctypes.data, None))
        return labels, core.astype(bool)

    def dbscan_device(self, eps, min_samples: int, out_labels=None, out_core=None, out_n_clusters=None, stream=None):
        """``dbscan`` with the results in HBM: CUDA tensors ``(labels int64 [n], core uint8 [n], n_clusters int64 [1])``,
        written in stream order on ``stream`` (default: the current torch stream).  The call waits for the device once."""
        import torch
        e, m = self._dbscan_args(eps, min_samples)
        n = self._n
        labels, core, ncl = self._outs((out_labels, n, torch.int64, n), (out_core, n, torch.uint8, n),
                                       (out_n_clusters, 1, torch.int64, 1))
        check(self._fn("dbscan_device")(self._h, e, m, 0, labels.data_ptr(), core.data_ptr(), ncl.data_ptr(),
                                        stream_arg(stream, self._dev)))
        return labels, core, ncl

    # ---------------------------------------------------------------------- MST
    # The minimum spanning tree of the indexed rows under mutual reachability (``pn_mst_*``): edge {i, j} weighs
    # max(d(i, j), core[i], core[j]), edges are ordered by (weight, i, j) and the tree is the unique one under that strict
    # order, its n - 1 edges written ascending -- the merge order of a single-linkage dendrogram.  ``core[i]`` is row i's
    # core distance: for HDBSCAN the distance to its ``min_samples``-th nearest OTHER row, ``query_self(min_samples)``'s
    # last column (scikit-learn counts the row itself, so its m is this library's m - 1).  ``core=None``: the plain
    # Euclidean / Cosine MST (single linkage).
    def mst(self, core=None):
        """``(src uint64 [n-1], dst uint64 [n-1], weight [n-1])`` with ``src < dst``, ascending by (weight, src, dst).
        ``core``: None or n values (converted to the tree's element type).  ``self.last_mst_work`` then holds
        ``(rounds, rows scanned)``."""
        c = None
        if core is not None:
            c = self._per_row(core, self.dtype, f"core must hold one value per indexed row ({self._n})")
        ne = max(self._n - 1, 0)
        src = np.empty(ne, dtype=np.uint64)
        dst = np.empty(ne, dtype=np.uint64)
        weight = np.empty(ne, dtype=self.dtype)
        work = np.zeros(2, dtype=np.uint64)
        check(self._fn("mst")(self._h, c.ctypes.data if c is not None else None, 0, src.ctypes.data, dst.ctypes.data,
                              weight.ctypes.data, work.ctypes.data))
        self.last_mst_work = (int(work[0]), int(work[1]))
        return src, dst, weight

    def mst_device(self, core=None, out_src=None, out_dst=None, out_weight=None, stream=None):
        """``mst`` in HBM: ``core`` None or a 1-D CUDA tensor of n values of the tree's element type; CUDA tensors
        ``(src int64 [n-1], dst int64 [n-1], weight [n-1])`` written in stream order on ``stream`` (default: the current
        torch stream).  The call waits for the device once per Boruvka round."""
        import torch
        ne = max(self._n - 1, 0)
        if core is not None:
            if not isinstance(core, torch.Tensor):
                raise ValueError("core must be a CUDA tensor (or None)")
            if core.dtype != self._tdt or core.dim() != 1 or core.numel() != self._n or not core.is_cuda:
                raise ValueError(f"core must be a 1-D CUDA tensor of {self._n} values of the tree's element type")
            core = core.contiguous()
        src, dst, weight = self._outs((out_src, ne, torch.int64, ne), (out_dst, ne, torch.int64, ne),
                                      (out_weight, ne, self._tdt, ne))
        work = np.zeros(2, dtype=np.uint64)
        check(self._fn("mst_device")(self._h, core.data_ptr() if core is not None else None, 0, src.data_ptr(),
                                     dst.data_ptr(), weight.data_ptr(), work.ctypes.data, stream_arg(stream, self._dev)))
        self.last_mst_work = (int(work[0]), int(work[1]))
        return src, dst, weight

    def mutual_reachability_mst(self, min_samples: int):
        """HDBSCAN's tree without leaving HBM: ``query_self_device(min_samples)``'s last column -- the distance to the
        ``min_samples``-th nearest other row -- fed to ``mst_device``, all on the current torch stream.  Returns CUDA
        tensors ``(src, dst, weight)``."""
        if int(min_samples) < 1 or int(min_samples) > self._n - 1:
            raise ValueError("min_samples must be in [1, n - 1]")
        _, dist = self.query_self_device(int(min_samples))
        return self.mst_device(dist[:, -1].contiguous())

    # ------------------------------------------------------- dendrogram, HDBSCAN
    # The single-linkage dendrogram of sorted tree edges (``pn_linkage_*``) in SciPy's layout: the r-th edge makes node
    # n + r with children ``left[r]`` (the subtree that holds ``src[r]``) and ``right[r]``; ids below n are rows.
    def linkage(self, core=None, edges=None):
        """``(left uint64 [n-1], right uint64 [n-1], weight [n-1], size uint64 [n-1])``: the dendrogram of
        ``edges = (src, dst, weight)`` -- a spanning tree's edges in merge order, as ``mst`` returns them -- or, without
        ``edges``, of ``self.mst(core)``.  Edges that are no spanning tree raise."""
        if edges is None:
            edges = self.mst(core)
        elif core is not None:
            raise ValueError("give core or edges, not both")
        ne = max(self._n - 1, 0)
        src, dst, w = (self._per_row(t, dt, f"edges must be three arrays of n - 1 = {ne} values", ne)
                       for t, dt in zip(edges, (np.uint64, np.uint64, self.dtype)))
        left = np.empty(ne, dtype=np.uint64)
        right = np.empty(ne, dtype=np.uint64)
        weight = np.empty(ne, dtype=self.dtype)
        size = np.empty(ne, dtype=np.uint64)
        check(self._fn("linkage")(self._h, src.ctypes.data, dst.ctypes.data, w.ctypes.data, 0, left.ctypes.data,
                                  right.ctypes.data, weight.ctypes.data, size.ctypes.data))
        return left, right, weight, size

    def linkage_device(self, core=None, edges=None, out_left=None, out_right=None, out_weight=None, out_size=None,
                       out_error=None, stream=None):
        """``linkage`` in HBM: ``edges`` are CUDA tensors ``(src int64, dst int64, weight)`` (default:
        ``mst_device(core)``); returns CUDA tensors ``(left int64, right int64, weight, size int64, error int32 [1])``
        written in stream order on ``stream`` (default: the current torch stream) without waiting for the device.
        ``error[0]`` is 0, or ``PN_ERR_INVALID`` when the edges are no spanning tree."""
        import torch
        ne = max(self._n - 1, 0)
        if edges is None:
            edges = self.mst_device(core, stream=stream)
        elif core is not None:
            raise ValueError("give core or edges, not both")
        src, dst, w = edges
        for t, want in ((src, torch.int64), (dst, torch.int64), (w, self._tdt)):
            if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != want or t.dim() != 1 or t.numel() != ne
                    or not t.is_contiguous()):
                raise ValueError(f"edges must be three contiguous 1-D CUDA tensors of n - 1 = {ne} values (int64, int64, "
                                 "the tree's element type)")
        left, right, weight, size, err = self._outs((out_left, ne, torch.int64, ne), (out_right, ne, torch.int64, ne),
                                                    (out_weight, ne, self._tdt, ne), (out_size, ne, torch.int64, ne),
                                                    (out_error, 1, torch.int32, 1, True))
        check(self._fn("linkage_device")(
            self._h, src.data_ptr(), dst.data_ptr(), w.data_ptr(), 0, left.data_ptr(), right.data_ptr(), weight.data_ptr(),
            size.data_ptr(), err.data_ptr(), stream_arg(stream, self._dev)))
        return left, right, weight, size, err

    def _hdbscan_args(self, min_cluster_size, min_samples):
        m = int(min_cluster_size)
        if m < 2:
            raise ValueError("min_cluster_size must be at least 2")
        if min_samples is None:
            k = max(min(m, self._n - 1), 1)
        else:
            k = int(min_samples)
            if self._n >= 2 and (k < 1 or k > self._n - 1):
                raise ValueError("min_samples must be in [1, n - 1]")
        return m, k

    def hdbscan(self, min_cluster_size, min_samples=None):
        """HDBSCAN on the device (``pn_hdbscan_*``): ``(labels int64 [n], probabilities [n])``; labels are
        0 .. n_clusters - 1 by ascending lowest member row, -1 is noise.  ``min_samples`` counts OTHER rows (scikit-learn's
        value minus one); the default is ``min_cluster_size``, capped at n - 1.  ``self.last_n_clusters`` then holds the
        number of clusters."""
        m, k = self._hdbscan_args(min_cluster_size, min_samples)
        labels = np.empty(self._n, dtype=np.int64)
        prob = np.empty(self._n, dtype=self.dtype)
        ncl = np.zeros(1, dtype=np.uint64)
        check(self._fn("hdbscan")(self._h, k, m, 0, labels.ctypes.data, prob.ctypes.data, ncl.ctypes.data))
        self.last_n_clusters = int(ncl[0])
        return labels, prob

    def hdbscan_device(self, min_cluster_size, min_samples=None, out_labels=None, out_probabilities=None,
                       out_n_clusters=None, stream=None):
        """``hdbscan`` in HBM: CUDA tensors ``(labels int64 [n], probabilities [n], n_clusters int64 [1])`` written in
        stream order on ``stream`` (default: the current torch stream).  The call waits for the device once per Boruvka
        round of the tree and not after it."""
        import torch
        m, k = self._hdbscan_args(min_cluster_size, min_samples)
        n = self._n
        labels, prob, ncl = self._outs((out_labels, n, torch.int64, n), (out_probabilities, n, self._tdt, n),
                                       (out_n_clusters, 1, torch.int64, 1, True))
        check(self._fn("hdbscan_device")(self._h, k, m, 0, labels.data_ptr(), prob.data_ptr(), ncl.data_ptr(),
                                         stream_arg(stream, self._dev)))
        return labels, prob, ncl

    # ------------------------------------------------------ Local Outlier Factor
    # scikit-learn's ``LocalOutlierFactor(n_neighbors=k)`` on the device (``pn_lof_*``): the k self-query, packed in HBM,
    # one gather pass for the local reachability densities and one for the scores; ``lof == -negative_outlier_factor_``.
    # ``lrd`` and ``kdist`` are the fit: ``lof_score`` takes them back to score new points (``score_samples`` negated).
    def _lof_k(self, k):
        k = int(k)
        if k < 1 or k > self._n - 1:
            raise ValueError(f"k must be in [1, n - 1] = [1, {self._n - 1}]")
        return k

    def lof(self, k: int = 20, full: bool = False):
        """Local Outlier Factor of every indexed row over its ``k`` nearest OTHER rows: ``scores float64 [n]``, or
        ``(scores, lrd float64 [n], kdist [n])`` with ``full=True``."""
        k = self._lof_k(k)
        scores = np.empty(self._n, dtype=np.float64)
        lrd = np.empty(self._n, dtype=np.float64) if full else None
        kdist = np.empty(self._n, dtype=self.dtype) if full else None
        check(self._fn("lof")(self._h, k, 0, scores.ctypes.data, lrd.ctypes.data if full else None,
                              kdist.ctypes.data if full else None))
        return (scores, lrd, kdist) if full else scores

    def lof_device(self, k: int = 20, out_lof=None, out_lrd=None, out_kdist=None, stream=None):
        """``lof`` in HBM: CUDA tensors ``(lof float64 [n], lrd float64 [n], kdist [n])`` written in stream order on
        ``stream`` (default: the current torch stream); the call does not wait for the device."""
        import torch
        k = self._lof_k(k)
        n = self._n
        lof, lrd, kdist = self._outs((out_lof, n, torch.float64, n), (out_lrd, n, torch.float64, n),
                                     (out_kdist, n, self._tdt, n))
        check(self._fn("lof_device")(self._h, k, 0, lof.data_ptr(), lrd.data_ptr(), kdist.data_ptr(),
                                     stream_arg(stream, self._dev)))
        return lof, lrd, kdist

    def lof_score(self, queries, k: int, lrd, kdist):
        """Outlier scores ``float64 [nq]`` of new points against a fit: ``lrd`` and ``kdist`` are ``lof(k, full=True)``'s,
        with the same ``k``.  A fitted row scored here finds itself at distance 0, so it does not reproduce its fit score
        (scikit-learn's ``score_samples`` behaves the same way)."""
        k = self._lof_k(k)
        message = f"lrd and kdist must hold one value per indexed row ({self._n})"
        lrd = self._per_row(lrd, np.float64, message)
        kdist = self._per_row(kdist, self.dtype, message)
        a = self._queries(queries, False)
        nq, qc = a.shape
        scores = np.empty(nq, dtype=np.float64)
        if nq:
            check(self._fn("lof_score")(self._h, a.ctypes.data, nq, qc, max(qc, 1), k, lrd.ctypes.data, kdist.ctypes.data,
                                        0, scores.ctypes.data))
        return scores

    def lof_score_device(self, queries, k: int, lrd, kdist, out=None, stream=None):
        """``lof_score`` in HBM: ``queries`` a 2-D CUDA tensor of the tree's element type, ``lrd`` (float64) and ``kdist``
        contiguous 1-D CUDA tensors of n values (``lof_device``'s); returns the CUDA tensor ``scores float64 [nq]``,
        written in stream order on ``stream`` (default: the current torch stream)."""
        import torch
        k = self._lof_k(k)
        for t, want in ((lrd, torch.float64), (kdist, self._tdt)):
            self._per_row_device(t, want, f"lrd and kdist must be contiguous 1-D CUDA tensors of {self._n} values on the "
                                          "tree's device (float64, the tree's element type)")
        q, nq, qc, ptr, ld = self._device_queries(queries, on_device=True, null_empty=False)
        scores = self._out(out, nq, torch.float64, nq, dev=q.device)
        if nq:
            check(self._fn("lof_score_device")(self._h, ptr, nq, qc, ld, k, lrd.data_ptr(), kdist.data_ptr(), 0,
                                               scores.data_ptr(), stream_arg(stream, q.device)))
        return scores

    # ------------------------------------------- k-NN classification and regression
    # scikit-learn's ``KNeighborsClassifier`` / ``KNeighborsRegressor(n_neighbors=k, weights=...)`` on the device
    # (``pn_knn_classify_*`` / ``pn_knn_regress_*``): the k-NN query, then one vote or one weighted mean per list in HBM; the
    # ``_self`` methods predict every indexed row from its k nearest OTHER rows (leave-one-out).  Every sum runs in list
    # order, so the result depends on the data alone (the header has the contract).
    def _knn_k(self, k, leave_one_out):
        k, top = int(k), self._n - 1 if leave_one_out else self._n
        if k < 1 or k > top:
            raise ValueError(f"k must be in [1, {'n - 1' if leave_one_out else 'n'}] = [1, {top}]")
        if k > 1024:
            raise ValueError("k-NN prediction serves k <= 1024")
        return k

    @staticmethod
    def _knn_flags(weights):
        if not isinstance(weights, str) or weights not in KNN_WEIGHTS:
            raise ValueError(f"weights must be one of {sorted(KNN_WEIGHTS)}, not {weights!r}")
        return KNN_WEIGHTS[weights]

    def _knn_labels(self, labels):
        """``(classes, codes int64 [n])`` of any 1-D array of one label per indexed row"""
        a = np.asarray(labels)
        if a.ndim != 1 or a.shape[0] != self._n:
            raise ValueError(f"labels must be 1-D with one label per indexed row ({self._n})")
        classes, codes = np.unique(a, return_inverse=True)
        return classes, np.ascontiguousarray(codes.reshape(-1), dtype=np.int64)

    def _knn_targets(self, targets):
        """``(y float64 [n, n_out], one_d)`` of ``[n]`` or ``[n, n_out]`` targets of any real dtype"""
        y = np.asarray(targets)
        if y.ndim not in (1, 2) or y.shape[0] != self._n or (y.ndim == 2 and y.shape[1] < 1):
            raise ValueError(f"targets must be [n] or [n, n_out >= 1] with one row per indexed row ({self._n})")
        if y.dtype.kind not in "fiub":
            raise ValueError(f"targets must be real numbers, not {y.dtype}")
        return np.ascontiguousarray(y.reshape(self._n, -1), dtype=np.float64), y.ndim == 1

    def _knn_n_classes(self, n_classes):
        c = int(n_classes)
        if c < 1 or c > 2 ** 31 - 1:
            raise ValueError("n_classes must be in [1, 2^31 - 1]")
        return c

    @staticmethod
    def _knn_decode(pred, pr, classes, proba):
        bad = int(np.count_nonzero(pred < 0))
        if bad:
            raise ValueError(f"{bad} of {len(pred)} lists are poisoned (a NaN distance): they have no prediction")
        out = classes[pred]
        return (out, pr, classes) if proba else out

    def knn_classify(self, queries, k: int, labels, weights: str = "uniform", proba: bool = False):
        """The class of every row of ``queries`` by the vote of its ``k`` nearest indexed rows.  ``labels``: any 1-D array
        of one label per indexed row; ``weights``: ``"uniform"`` or ``"distance"`` (1 / distance; a zero distance counts
        alone).  Returns the predictions in ``labels``' dtype -- ties go to the smallest class -- or, with ``proba=True``,
        ``(pred, proba float64 [nq, n_classes], classes)``, the columns of ``proba`` in the order of ``classes``."""
        k, flags = self._knn_k(k, False), self._knn_flags(weights)
        classes, codes = self._knn_labels(labels)
        a = self._queries(queries, False)
        nq, qc = a.shape
        pred = np.zeros(nq, dtype=np.int64)
        pr = np.zeros((nq, len(classes)), dtype=np.float64) if proba else None
        if nq:
            check(self._fn("knn_classify")(self._h, a.ctypes.data, nq, qc, max(qc, 1), k, codes.ctypes.data, len(classes),
                                           flags, pred.ctypes.data, pr.ctypes.data if proba else None))
        return self._knn_decode(pred, pr, classes, proba)

    def knn_classify_self(self, k: int, labels, weights: str = "uniform", proba: bool = False):
        """``knn_classify`` of every indexed row from its ``k`` nearest OTHER rows: the leave-one-out predictions."""
        k, flags = self._knn_k(k, True), self._knn_flags(weights)
        classes, codes = self._knn_labels(labels)
        pred = np.zeros(self._n, dtype=np.int64)
        pr = np.zeros((self._n, len(classes)), dtype=np.float64) if proba else None
        check(self._fn("knn_classify_self")(self._h, k, codes.ctypes.data, len(classes), flags, pred.ctypes.data,
                                            pr.ctypes.data if proba else None))
        return self._knn_decode(pred, pr, classes, proba)

    def knn_regress(self, queries, k: int, targets, weights: str = "uniform"):
        """The weighted mean of the targets of the ``k`` nearest indexed rows, for every row of ``queries``.  ``targets``:
        ``[n]`` or ``[n, n_out]`` of any real dtype (taken as float64); returns float64 ``[nq]`` or ``[nq, n_out]``.  A
        query with a NaN distance in its list gets NaN."""
        k, flags = self._knn_k(k, False), self._knn_flags(weights)
        y, one_d = self._knn_targets(targets)
        a = self._queries(queries, False)
        nq, qc = a.shape
        out = np.zeros((nq, y.shape[1]), dtype=np.float64)
        if nq:
            check(self._fn("knn_regress")(self._h, a.ctypes.data, nq, qc, max(qc, 1), k, y.ctypes.data, y.shape[1], flags,
                                          out.ctypes.data))
        return out[:, 0] if one_d else out

    def knn_regress_self(self, k: int, targets, weights: str = "uniform"):
        """``knn_regress`` of every indexed row from its ``k`` nearest OTHER rows (leave-one-out)."""
        k, flags = self._knn_k(k, True), self._knn_flags(weights)
        y, one_d = self._knn_targets(targets)
        out = np.zeros((self._n, y.shape[1]), dtype=np.float64)
        check(self._fn("knn_regress_self")(self._h, k, y.ctypes.data, y.shape[1], flags, out.ctypes.data))
        return out[:, 0] if one_d else out

    def _knn_classify_device(self, q, k, labels, n_classes, weights, proba, out_pred, out_proba, stream):
        """the two device votes: ``q`` = ``_device_queries``' answer, or None for the indexed rows"""
        import torch
        flags, c = self._knn_flags(weights), self._knn_n_classes(n_classes)
        self._per_row_device(labels, torch.int64, f"labels must be a contiguous 1-D int64 CUDA tensor of {self._n} class "
                                                  "codes on the tree's device")
        count, dev = (self._n, self._dev) if q is None else (q[1], q[0].device)
        specs = [(out_pred, count, torch.int64, count)]
        if proba:
            specs.append((out_proba, (count, c), torch.float64, count * c))
        elif out_proba is not None:
            raise ValueError("out_proba needs proba=True")
        outs = self._outs(*specs, dev=dev)
        pr = outs[1].data_ptr() if proba else None
        if q is None:
            check(self._fn("knn_classify_self_device")(self._h, k, labels.data_ptr(), c, flags, outs[0].data_ptr(), pr,
                                                       stream_arg(stream, dev)))
        elif count:
            check(self._fn("knn_classify_device")(self._h, q[3], count, q[2], q[4], k, labels.data_ptr(), c, flags,
                                                  outs[0].data_ptr(), pr, stream_arg(stream, dev)))
        return (outs[0], outs[1]) if proba else outs[0]

    def knn_classify_device(self, queries, k: int, labels, n_classes: int, weights: str = "uniform", proba: bool = False,
                            out_pred=None, out_proba=None, stream=None):
        """``knn_classify`` in HBM: ``queries`` a 2-D CUDA tensor of the tree's element type, ``labels`` a contiguous int64
        CUDA tensor of n class codes in ``[0, n_classes)``.  Returns the CUDA tensor ``pred int64 [nq]`` (-1: a list with a
        NaN distance or a label out of range), or ``(pred, proba float64 [nq, n_classes])`` with ``proba=True``, written in
        stream order on ``stream`` (default: the current torch stream); the call does not wait for the device."""
        k = self._knn_k(k, False)
        q = self._device_queries(queries, on_device=True, null_empty=False)
        return self._knn_classify_device(q, k, labels, n_classes, weights, proba, out_pred, out_proba, stream)

    def knn_classify_self_device(self, k: int, labels, n_classes: int, weights: str = "uniform", proba: bool = False,
                                 out_pred=None, out_proba=None, stream=None):
        """``knn_classify_self`` in HBM, as ``knn_classify_device``: ``pred int64 [n]`` or ``(pred, proba [n, n_classes])``."""
        k = self._knn_k(k, True)
        return self._knn_classify_device(None, k, labels, n_classes, weights, proba, out_pred, out_proba, stream)

    def _knn_regress_device(self, q, k, targets, weights, out, stream):
        import torch
        flags = self._knn_flags(weights)
        if (not self._on_device(targets, torch.float64, self._n) or targets.dim() not in (1, 2)
                or targets.shape[0] != self._n or targets.numel() == 0):
            raise ValueError(f"targets must be a contiguous float64 CUDA tensor [n] or [n, n_out >= 1] on the tree's device "
                             f"(n = {self._n})")
        n_out = targets.numel() // self._n
        count, dev = (self._n, self._dev) if q is None else (q[1], q[0].device)
        shape = count if targets.dim() == 1 else (count, n_out)
        out = self._out(out, shape, torch.float64, count * n_out, dev=dev)
        if q is None:
            check(self._fn("knn_regress_self_device")(self._h, k, targets.data_ptr(), n_out, flags, out.data_ptr(),
                                                      stream_arg(stream, dev)))
        elif count:
            check(self._fn("knn_regress_device")(self._h, q[3], count, q[2], q[4], k, targets.data_ptr(), n_out, flags,
                                                 out.data_ptr(), stream_arg(stream, dev)))
        return out

    def knn_regress_device(self, queries, k: int, targets, weights: str = "uniform", out=None, stream=None):
        """``knn_regress`` in HBM: ``targets`` a contiguous float64 CUDA tensor ``[n]`` or ``[n, n_out]``; returns the CUDA
        tensor float64 ``[nq]`` or ``[nq, n_out]``, written in stream order on ``stream``."""
        k = self._knn_k(k, False)
        q = self._device_queries(queries, on_device=True, null_empty=False)
        return self._knn_regress_device(q, k, targets, weights, out, stream)

    def knn_regress_self_device(self, k: int, targets, weights: str = "uniform", out=None, stream=None):
        """``knn_regress_self`` in HBM, as ``knn_regress_device``: float64 ``[n]`` or ``[n, n_out]``."""
        k = self._knn_k(k, True)
        return self._knn_regress_device(None, k, targets, weights, out, stream)

    # ------------------------------------------------------------------- OPTICS
    # scikit-learn's ``OPTICS(min_samples + 1, max_eps)`` on the device (``pn_optics_*``): the ordering, the reachability
    # plot, predecessors and core distances, and (``optics_dbscan``) the DBSCAN labels at any eps <= max_eps read off the
    # ordering.  ``min_samples`` counts OTHER rows; every radius is a strict '<'.  ``ordering`` holds plain row numbers
    # (no ``PN_OPT_INDEX_BASE``): it indexes the other arrays.
    def _optics_args(self, min_samples, max_eps):
        k = int(min_samples)
        if k < 1 or (self._n >= 2 and k > self._n - 1):
            raise ValueError(f"min_samples must be in [1, n - 1] = [1, {max(self._n - 1, 1)}]")
        return k, self._real(max_eps)

    def optics(self, min_samples: int, max_eps=np.inf):
        """``(ordering uint64 [n], reachability [n], predecessor int64 [n], core_distances [n])``: rows in the order
        OPTICS visits them; ``reachability`` / ``predecessor`` / ``core_distances`` are indexed by row (+inf, -1, +inf
        where undefined)."""
        k, e = self._optics_args(min_samples, max_eps)
        ordering = np.empty(self._n, dtype=np.uint64)
        reach = np.empty(self._n, dtype=self.dtype)
        pred = np.empty(self._n, dtype=np.int64)
        core = np.empty(self._n, dtype=self.dtype)
        check(self._fn("optics")(self._h, k, e, 0, ordering.ctypes.data, reach.ctypes.data, pred.ctypes.data,
                                 core.ctypes.data))
        return ordering, reach, pred, core

    def optics_device(self, min_samples: int, max_eps=np.inf, out_ordering=None, out_reachability=None,
                      out_predecessor=None, out_core=None, stream=None):
        """``optics`` in HBM: CUDA tensors ``(ordering int64 [n], reachability [n], predecessor int64 [n],
        core_distances [n])`` written in stream order on ``stream`` (default: the current torch stream).  The call waits
        for the device once, after the counting pass."""
        import torch
        k, e = self._optics_args(min_samples, max_eps)
        n = self._n
        ordering, reach, pred, core = self._outs((out_ordering, n, torch.int64, n),
                                                 (out_reachability, n, self._tdt, n),
                                                 (out_predecessor, n, torch.int64, n), (out_core, n, self._tdt, n))
        check(self._fn("optics_device")(self._h, k, e, 0, ordering.data_ptr(), reach.data_ptr(), pred.data_ptr(),
                                        core.data_ptr(), stream_arg(stream, self._dev)))
        return ordering, reach, pred, core

    def optics_dbscan(self, eps, ordering, reachability, core_distances):
        """``(labels int64 [n], n_clusters)``: the DBSCAN labels at ``eps`` (<= the ordering's max_eps) read off
        ``optics``'s outputs; clusters are numbered by first appearance in the ordering, noise is -1.  An ordering that
        is no permutation of the rows raises ``PetalError``."""
        message = f"ordering, reachability and core_distances must hold one value per indexed row ({self._n})"
        o = self._per_row(ordering, np.uint64, message)
        r = self._per_row(reachability, self.dtype, message)
        c = self._per_row(core_distances, self.dtype, message)
        labels = np.empty(self._n, dtype=np.int64)
        ncl = np.zeros(1, dtype=np.uint64)
        check(self._fn("optics_dbscan")(self._h, o.ctypes.data, r.ctypes.data, c.ctypes.data, self._real(eps), 0,
                                        labels.ctypes.data, ncl.ctypes.data))
        return labels, int(ncl[0])

    def optics_dbscan_device(self, eps, ordering, reachability, core_distances, out_labels=None, out_n_clusters=None,
                             out_error=None, stream=None):
        """``optics_dbscan`` in HBM: the inputs are ``optics_device``'s tensors; returns CUDA tensors ``(labels int64 [n],
        n_clusters int64 [1], error int32 [1])`` written in stream order on ``stream`` (default: the current torch
        stream) without waiting for the device.  ``error[0]`` is 0, or ``PN_ERR_INVALID`` when the ordering is no
        permutation of the rows."""
        import torch
        n = self._n
        for t, want in ((ordering, torch.int64), (reachability, self._tdt), (core_distances, self._tdt)):
            self._per_row_device(t, want, f"ordering, reachability and core_distances must be contiguous 1-D CUDA tensors "
                                          f"of {n} values on the tree's device (int64, the tree's element type)")
        labels, ncl, err = self._outs((out_labels, n, torch.int64, n), (out_n_clusters, 1, torch.int64, 1, True),
                                      (out_error, 1, torch.int32, 1, True))
        check(self._fn("optics_dbscan_device")(
            self._h, ordering.data_ptr(), reachability.data_ptr(), core_distances.data_ptr(), self._real(eps), 0,
            labels.data_ptr(), ncl.data_ptr(), err.data_ptr(), stream_arg(stream, self._dev)))
        return labels, ncl, err

    # -------------------------------------------------- kernel density estimation
    # scikit-learn's ``BallTree.kernel_density`` on the device (``pn_kde_*``): per query the sum of the kernel over the rows
    # within the kernel's cutoff, one wave per query in a fixed order.  ``h`` is a scalar or one bandwidth per query (the
    # balloon estimator); ``atol`` lets the two smooth kernels stop at a finite cutoff (``sum_all - atol <= sum <= sum_all``);
    # with ``atol=0`` they visit every row.  Every comparison is a strict '<'.
    def _kde_kernel(self, kernel, atol):
        if kernel not in KDE_KERNELS:
            raise ValueError(f"unknown kernel {kernel!r}: one of {sorted(KDE_KERNELS)}")
        atol = float(atol)
        if not (atol >= 0.0) or math.isinf(atol):
            raise ValueError("atol must be finite and >= 0")
        return KDE_KERNELS[kernel]

    def _kde_args(self, h, kernel, atol, count, normalize=False):
        """(kernel number, the bandwidths as a contiguous array of the tree's dtype: one, or ``count``)"""
        kn = self._kde_kernel(kernel, atol)
        if normalize and isinstance(self.metric, Cosine):
            raise ValueError("normalize=True needs a Euclidean tree: the normalisers are volumes of Euclidean balls")
        ha = self._radii(h, count)
        if ha is None:
            ha = np.array([h], dtype=self.dtype)
            if not (ha[0] > 0) or not np.isfinite(ha[0]):
                raise ValueError("the bandwidth must be finite and positive")
        return kn, ha

    def _kde_finish(self, s, ha, kernel, return_log, normalize):
        with np.errstate(divide="ignore", invalid="ignore"):
            if return_log:
                out = np.log(s)
                return out + kde_log_norm(kernel, self._dim, ha if ha.shape[0] > 1 else ha[0]) if normalize else out
            return s * np.exp(kde_log_norm(kernel, self._dim, ha if ha.shape[0] > 1 else ha[0])) if normalize else s

    def _kde(self, queries, ha, kn, atol, flags, s, cnt, cut):
        """the one host call: ``queries`` (an array, or None: the indexed rows) against bandwidths ``ha``; ``s`` / ``cnt``
        / ``cut`` are the output arrays, each may be None"""
        outs = [None if t is None else t.ctypes.data for t in (s, cnt, cut)]
        if queries is None:
            check(self._fn("kde_self")(self._h, ha.ctypes.data, ha.shape[0], kn, float(atol), flags, *outs))
        elif queries.shape[0]:
            nq, qc = queries.shape
            check(self._fn("kde")(self._h, queries.ctypes.data, nq, qc, max(qc, 1), ha.ctypes.data, ha.shape[0], kn,
                                  float(atol), 0, *outs))

    def kernel_density(self, queries, h, kernel: str = "gaussian", atol: float = 0.0, return_log: bool = False,
                       normalize: bool = True):
        """Kernel density of every row of ``queries``: ``float64 [nq]``.  With ``normalize`` the kernel's normaliser for the
        row dimension is applied, as scikit-learn's ``BallTree.kernel_density`` does; the result is not divided by n.  An
        empty list gives 0 (``-inf`` with ``return_log``)."""
        a = self._queries(queries, False)
        kn, ha = self._kde_args(h, kernel, atol, a.shape[0], normalize)
        s = np.zeros(a.shape[0], dtype=np.float64)
        self._kde(a, ha, kn, atol, 0, s, None, None)
        return self._kde_finish(s, ha, kernel, return_log, normalize)

    def kernel_density_self(self, h, kernel: str = "gaussian", atol: float = 0.0, return_log: bool = False,
                            normalize: bool = True, include_self: bool = False):
        """``kernel_density`` of the indexed rows themselves; by default each row is left out of its own estimate (the
        leave-one-out density)."""
        kn, ha = self._kde_args(h, kernel, atol, self._n, normalize)
        s = np.zeros(self._n, dtype=np.float64)
        self._kde(None, ha, kn, atol, self._self_flags(include_self), s, None, None)
        return self._kde_finish(s, ha, kernel, return_log, normalize)

    def kernel_density_raw(self, queries, h, kernel: str = "gaussian", atol: float = 0.0, include_self: bool = False):
        """The C ABI's three outputs on the host: ``(sum float64, count uint64, cutoff)`` per query; ``queries=None``: the
        indexed rows themselves (``include_self`` as in ``kernel_density_self``)."""
        a = None if queries is None else self._queries(queries, False)
        nq = self._n if a is None else a.shape[0]
        kn, ha = self._kde_args(h, kernel, atol, nq)
        s = np.zeros(nq, dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.uint64)
        cut = np.zeros(nq, dtype=self.dtype)
        self._kde(a, ha, kn, atol, self._self_flags(include_self), s, cnt, cut)
        return s, cnt, cut

    def _kde_device_args(self, h, kernel, atol, count, outs):
        import torch
        kn = self._kde_kernel(kernel, atol)
        ht = self._radii_device(h, count, self._dev)
        if ht is None and (not (float(h) > 0.0) or math.isinf(float(h))):
            raise ValueError("the bandwidth must be finite and positive")
        s, cnt, cut = self._outs((outs[0], count, torch.float64, count), (outs[1], count, torch.int64, count),
                                 (outs[2], count, self._tdt, count))
        if ht is None:
            ht = torch.full((1,), float(h), dtype=self._tdt, device=self._dev)
        return kn, ht, s, cnt, cut

    def kernel_density_device(self, queries, h, kernel: str = "gaussian", atol: float = 0.0, out_sum=None, out_count=None,
                              out_cutoff=None, stream=None):
        """The raw sums in HBM: ``queries`` a 2-D CUDA tensor of the tree's element type, ``h`` a scalar or a 1-D CUDA tensor
        of one bandwidth per query; returns CUDA tensors ``(sum float64 [nq], count int64 [nq], cutoff [nq])`` written in
        stream order on ``stream`` (default: the current torch stream).  The call waits for the device once (it reads
        the list offsets back to cut its pieces) and cannot be captured into a graph."""
        q, nq, qc, ptr, ld = self._device_queries(queries, on_device=True, null_empty=False)
        kn, ht, s, cnt, cut = self._kde_device_args(h, kernel, atol, nq, (out_sum, out_count, out_cutoff))
        if nq:
            check(self._fn("kde_device")(self._h, ptr, nq, qc, ld, ht.data_ptr(), ht.shape[0], kn, float(atol), 0,
                                         s.data_ptr(), cnt.data_ptr(), cut.data_ptr(), stream_arg(stream, q.device)))
        return s, cnt, cut

    def kernel_density_self_device(self, h, kernel: str = "gaussian", atol: float = 0.0, include_self: bool = False,
                                   out_sum=None, out_count=None, out_cutoff=None, stream=None):
        """``kernel_density_device`` of the indexed rows themselves (``h``: a scalar or one bandwidth per row)."""
        kn, ht, s, cnt, cut = self._kde_device_args(h, kernel, atol, self._n, (out_sum, out_count, out_cutoff))
        check(self._fn("kde_self_device")(self._h, ht.data_ptr(), ht.shape[0], kn, float(atol),
                                          self._self_flags(include_self), s.data_ptr(), cnt.data_ptr(), cut.data_ptr(),
                                          stream_arg(stream, self._dev)))
        return s, cnt, cut

    def query_radius_count(self, queries, r):
        """The number of rows with distance < ``r`` (strict) per query: ``uint64 [nq]``; ``r`` a scalar or one radius per
        query.  Only the counting pass runs: no list is written (scikit-learn's ``query_radius(count_only=True)``)."""
        a = self._queries(queries, False)
        nq = a.shape[0]
        ra = self._radii(r, nq)
        if ra is None:  # (a radius that is not finite and positive is served as an array: empty lists, or every row)
            ok = float(r) > 0.0 and not math.isinf(float(r))
            ra = np.array([r], dtype=self.dtype) if ok else np.full(nq, r, dtype=self.dtype)
        cnt = np.zeros(nq, dtype=np.uint64)
        self._kde(a, ra, _lib.PN_KDE_TOPHAT, 0.0, 0, None, cnt, None)
        return cnt

    def two_point_correlation(self, queries, r):
        """For each entry of the 1-D array ``r``: the number of (query, row) pairs with distance < ``r[i]``, ``int64``.
        scikit-learn's ``two_point_correlation`` counts distance <= r; every radius in this library is strict."""
        ra = np.asarray(r)
        if ra.ndim != 1:
            raise ValueError("r must be 1-D")
        a = self._queries(queries, False)
        return np.array([int(self.query_radius_count(a, x).sum()) for x in ra.tolist()], dtype=np.int64)

    # -------------------------------------------------- k-means
    # Lloyd's k-means on the device (``pn_kmeans_*``): the rows are assigned to their nearest centres behind a bf16 MFMA
    # filter with an exact re-rank and a proof per row, the centres become means summed in a fixed order.  Labels are those
    # of ``mean_shift_labels``; every sum has one stated shape, so a result does not depend on the engine or the launch.
    def _euclidean_only(self, what):
        if isinstance(self.metric, Cosine):
            raise ValueError(f"{what} needs a Euclidean tree")

    def _centres(self, centres):
        c = self._queries(centres, False)
        if c.shape[0] and c.shape[1] != self._dim:
            raise ValueError(f"centres must have the tree's {self._dim} columns")
        return c

    def _centres_device(self, centres):
        """contiguous ``[nc][dim]`` centres in HBM: ``(centres, nc, pointer)``"""
        c, nc, qc, ptr, _ = self._device_queries(centres, f"centres ([nc][{self._dim}])", on_device=True, contiguous=True)
        if nc and qc != self._dim:
            raise ValueError(f"centres must have the tree's {self._dim} columns")
        return c, nc, ptr

    def kmeans_assign(self, centres):
        """The nearest centre of every indexed row by (distance, centre number), as ``mean_shift_labels`` gives it:
        ``(labels int64 [n], dist [n], inertia)`` with ``dist`` the distance to that centre and ``inertia`` the sum of
        the squared distances in the library's fixed shape (a float)."""
        self._euclidean_only("k-means")
        c = self._centres(centres)
        labels = np.empty(self._n, dtype=np.int64)
        dist = np.empty(self._n, dtype=self.dtype)
        inertia = C.c_double(0.0)
        check(self._fn("kmeans_assign")(self._h, c.ctypes.data if c.shape[0] else None, c.shape[0], 0, labels.ctypes.data,
                                        dist.ctypes.data, C.byref(inertia)))
        return labels, dist, float(inertia.value)

    def kmeans_assign_device(self, centres, out_labels=None, out_dist=None, out_inertia=None, stream=None):
        """``kmeans_assign`` in HBM: ``centres`` a contiguous 2-D CUDA tensor; returns CUDA tensors ``(labels int64 [n],
        dist [n], inertia float64 [1])``.  Never waits."""
        import torch
        self._euclidean_only("k-means")
        centres, nc, ptr = self._centres_device(centres)
        labels, dist, inertia = self._outs((out_labels, self._n, torch.int64, self._n),
                                           (out_dist, self._n, self._tdt, self._n),
                                           (out_inertia, 1, torch.float64, 1, True))
        check(self._fn("kmeans_assign_device")(self._h, ptr, nc, 0, labels.data_ptr(), dist.data_ptr(), inertia.data_ptr(),
                                               stream_arg(stream, self._dev)))
        return labels, dist, inertia

    def _km_tol(self, tol, abs_tol, max_iter):
        if int(max_iter) < 1:
            raise ValueError("max_iter must be at least 1")
        if abs_tol is None:
            if not (float(tol) >= 0.0):
                raise ValueError("tol must be >= 0")
            if self.points is None:
                raise ValueError("a tree built from a device tensor needs abs_tol (the rows are not on the host)")
            # scikit-learn's _tolerance: tol times the mean of the columns' variances
            abs_tol = float(tol) * float(np.mean(np.var(np.asarray(self.points, dtype=np.float64), axis=0)))
        abs_tol = float(abs_tol)
        if not (abs_tol >= 0.0):
            raise ValueError("tol must be >= 0")
        return abs_tol, int(max_iter)

    def kmeans_plusplus(self, k: int, seed=None):
        """k-means++ seeding (D^2 sampling): ``k`` rows of the corpus as ``[k][dim]`` host array.  Every round is one
        ``kmeans_assign_device`` call with the one centre just drawn; the running minimum and the draw are torch's.  NOT
        bit-contractual: the draws are those of torch's generator (reproducible for one seed in one process and
        version), the distances are the library's.  An assignment to one centre is always the exact kernel's, whatever
        engine the tree is set to: a round packs nothing."""
        import torch
        self._euclidean_only("k-means")
        k = int(k)
        if k < 1 or k > self._n:
            raise ValueError("k must be between 1 and the number of rows")
        if self.points is None:
            raise ValueError("kmeans_plusplus needs the rows on the host")
        dev = self._dev
        g = torch.Generator(device="cpu")
        if seed is None:
            g.seed()
        else:
            g.manual_seed(int(seed))
        rows = np.ascontiguousarray(self.points)
        chosen = [int(torch.randint(self._n, (1,), generator=g).item())]
        mind2 = None
        for _ in range(1, k):
            c = torch.from_numpy(rows[chosen[-1]:chosen[-1] + 1].copy()).to(dev)
            _, dist, _ = self.kmeans_assign_device(c)
            d2 = dist.to(torch.float64) ** 2
            mind2 = d2 if mind2 is None else torch.minimum(mind2, d2)
            cs = torch.cumsum(torch.nan_to_num(mind2, nan=0.0, posinf=0.0), 0)
            total = float(cs[-1].item())
            if not total > 0.0:
                raise ValueError("fewer distinct rows than centres")
            u = float(torch.rand(1, generator=g, dtype=torch.float64).item()) * total
            i = int(torch.searchsorted(cs, torch.tensor([u], dtype=torch.float64, device=dev), right=True).item())
            chosen.append(min(i, self._n - 1))
        return rows[np.asarray(chosen)].copy()

    def kmeans(self, centres_or_k, tol: float = 1e-4, max_iter: int = 300, seed=None, abs_tol=None, full: bool = False):
        """Lloyd's k-means from the given initial centres ``[k][dim]``, or from ``kmeans_plusplus(k, seed)`` when an integer
        is given: ``(centres [k][dim], labels int64 [n], inertia)``; with ``full=True`` also ``dist [n]``, ``counts uint64
        [k]``, ``iterations`` and ``shift2``.  ``tol`` is scikit-learn's: relative to the mean variance of the columns
        (computed on the host); ``abs_tol`` gives the absolute bound on the summed squared moves itself.  A cluster that
        loses every member keeps its centre (scikit-learn relocates it): look at ``counts``.  ``last_n_iter`` holds the
        iterations run."""
        self._euclidean_only("k-means")
        abs_tol, max_iter = self._km_tol(tol, abs_tol, max_iter)
        if np.ndim(centres_or_k) == 0:
            init = self.kmeans_plusplus(int(centres_or_k), seed)
        else:
            init = self._centres(centres_or_k)
        k = init.shape[0]
        if k < 1:
            raise ValueError("k-means needs at least one centre")
        init = np.ascontiguousarray(init, dtype=self.dtype)
        centres = np.zeros((k, self._dim), dtype=self.dtype)
        labels = np.empty(self._n, dtype=np.int64)
        dist = np.empty(self._n, dtype=self.dtype)
        counts = np.zeros(k, dtype=np.uint64)
        inertia, shift2, iters = C.c_double(0.0), C.c_double(0.0), C.c_uint64(0)
        check(self._fn("kmeans")(
            self._h, init.ctypes.data, k, abs_tol, max_iter, 0, centres.ctypes.data, labels.ctypes.data, dist.ctypes.data,
            counts.ctypes.data, C.byref(inertia), C.byref(iters), C.byref(shift2)))
        self.last_n_iter = int(iters.value)
        if full:
            return centres, labels, float(inertia.value), dist, counts, int(iters.value), float(shift2.value)
        return centres, labels, float(inertia.value)

    def kmeans_device(self, centres, abs_tol, max_iter: int = 300, stream=None):
        """``kmeans`` in HBM from initial centres given as a contiguous 2-D CUDA tensor, with the absolute tolerance:
        CUDA tensors ``(centres, labels int64 [n], dist [n], counts int64 [k], inertia float64 [1], iterations int64 [1],
        shift2 float64 [1])``.  The call waits for the device once per iteration and cannot be captured into a graph."""
        import torch
        self._euclidean_only("k-means")
        centres, k, _ = self._centres_device(centres)
        abs_tol, max_iter = self._km_tol(0.0, abs_tol, max_iter)
        if k < 1:
            raise ValueError("k-means needs at least one centre")
        dev = self._dev
        out_c = torch.empty((k, self._dim), dtype=self._tdt, device=dev)
        labels = torch.empty(self._n, dtype=torch.int64, device=dev)
        dist = torch.empty(self._n, dtype=self._tdt, device=dev)
        counts = torch.zeros(k, dtype=torch.int64, device=dev)
        inertia = torch.zeros(1, dtype=torch.float64, device=dev)
        iters = torch.zeros(1, dtype=torch.int64, device=dev)
        shift2 = torch.zeros(1, dtype=torch.float64, device=dev)
        check(self._fn("kmeans_device")(
            self._h, centres.data_ptr(), k, abs_tol, max_iter, 0, out_c.data_ptr(), labels.data_ptr(), dist.data_ptr(),
            counts.data_ptr(), inertia.data_ptr(), iters.data_ptr(), shift2.data_ptr(), stream_arg(stream, dev)))
        return out_c, labels, dist, counts, inertia, iters, shift2

    def kmeans_bounds(self, centres):
        """Diagnostic: the k-means filter's lower bounds ``L[i][c] <= |x_i - c|^2`` (float64 ``[n][nc]``), f32 trees."""
        c = self._centres(centres)
        out = np.zeros((self._n, c.shape[0]), dtype=np.float64)
        check(_lib.lib().pn_kmeans_bounds_f32(self._h, c.ctypes.data if c.shape[0] else None, c.shape[0], out.ctypes.data))
        return out

    # -------------------------------------------------- mean shift
    # scikit-learn's ``MeanShift`` (flat kernel) on the device (``pn_mean_shift_*``): seeds climb to the modes of the tophat
    # density, every step the mean of a radius list summed by one wave in a fixed order; only the seeds still moving are
    # queried.  Then the converged modes are merged into centres and the rows labelled.  Every comparison is a strict '<'.
    def _ms_h(self, h, count):
        ha = self._radii(h, count)
        if ha is None:
            ha = np.array([h], dtype=self.dtype)
        return ha

    @staticmethod
    def _ms_tol(h, tol, max_iter):
        if tol is None:
            if np.ndim(h) != 0:
                raise ValueError("tol must be given with one bandwidth per seed")
            tol = 1e-3 * float(h)
        tol = float(tol)
        if not (tol >= 0.0):
            raise ValueError("tol must be >= 0")
        if int(max_iter) < 1:
            raise ValueError("max_iter must be at least 1")
        return tol, int(max_iter)

    def mean_shift_modes(self, h, seeds=None, tol=None, max_iter: int = 300, full: bool = False):
        """Moves every seed (``seeds=None``: every indexed row) to its mode with bandwidth ``h`` (a scalar, or one per seed):
        ``(modes [ns][dim], points_within uint64 [ns])``; with ``full=True`` also ``iterations uint32 [ns]``,
        ``shift float64 [ns]`` and ``work = (iterations run, seed-steps)``.  A seed with no row within ``h`` is dead:
        ``points_within`` 0, ``shift`` NaN.  ``tol`` defaults to ``1e-3 * h``.  ``last_n_iter`` holds the iterations run."""
        self._euclidean_only("mean shift")
        tol, max_iter = self._ms_tol(h, tol, max_iter)
        if seeds is None:
            a, ns, flags = None, self._n, _lib.PN_MS_SEED_ROWS
        else:
            a = self._queries(seeds, False)
            ns, flags = a.shape[0], 0
            if a.shape[1] != self._dim:
                raise ValueError(f"seeds must have the tree's {self._dim} columns")
        ha = self._ms_h(h, ns)
        modes = np.zeros((ns, self._dim), dtype=self.dtype)
        pw = np.zeros(ns, dtype=np.uint64)
        it = np.zeros(ns, dtype=np.uint32)
        sh = np.zeros(ns, dtype=np.float64)
        work = np.zeros(2, dtype=np.uint64)
        check(self._fn("mean_shift")(
            self._h, None if a is None else a.ctypes.data, 0 if a is None else ns, self._dim, self._dim, ha.ctypes.data,
            ha.shape[0], tol, max_iter, flags, modes.ctypes.data, pw.ctypes.data, it.ctypes.data, sh.ctypes.data,
            work.ctypes.data))
        self.last_n_iter = int(work[0])
        return (modes, pw, it, sh, (int(work[0]), int(work[1]))) if full else (modes, pw)

    def mean_shift_modes_device(self, h, seeds=None, tol=None, max_iter: int = 300, stream=None):
        """``mean_shift_modes`` in HBM: ``seeds`` a 2-D CUDA tensor of the tree's element type (or None: the indexed rows),
        ``h`` a scalar or a 1-D CUDA tensor of one bandwidth per seed; returns CUDA tensors ``(modes, points_within int64,
        iterations int32, shift float64)`` and ``work``.  The call waits for the device twice per iteration and cannot
        be captured into a graph."""
        import torch
        self._euclidean_only("mean shift")
        tol, max_iter = self._ms_tol(h, tol, max_iter)
        dev = self._dev
        if seeds is None:
            ns, flags, sp, stride = self._n, _lib.PN_MS_SEED_ROWS, None, 0
        else:
            seeds, ns, qc, sp, stride = self._device_queries(seeds, "seeds", on_device=True, null_empty=False)
            flags = 0
            if qc != self._dim:
                raise ValueError(f"seeds must have the tree's {self._dim} columns")
        ht = self._radii_device(h, ns, dev)
        if ht is None:
            ht = torch.full((1,), float(h), dtype=self._tdt, device=dev)
        modes = torch.zeros((ns, self._dim), dtype=self._tdt, device=dev)
        pw = torch.zeros(ns, dtype=torch.int64, device=dev)
        it = torch.zeros(ns, dtype=torch.int32, device=dev)
        sh = torch.zeros(ns, dtype=torch.float64, device=dev)
        work = np.zeros(2, dtype=np.uint64)
        check(self._fn("mean_shift_device")(
            self._h, sp, 0 if seeds is None else ns, self._dim, stride, ht.data_ptr(), ht.shape[0], tol, max_iter, flags,
            modes.data_ptr(), pw.data_ptr(), it.data_ptr(), sh.data_ptr(), work.ctypes.data, stream_arg(stream, dev)))
        self.last_n_iter = int(work[0])
        return modes, pw, it, sh, (int(work[0]), int(work[1]))

    def mean_shift_merge(self, modes, points_within, h):
        """scikit-learn's merge of converged modes: ``(centres [nc][dim], centre_points uint64 [nc], centre_of_seed int64
        [ns])``.  Live modes are ranked by (``points_within`` descending, seed ascending); a mode is a centre iff no earlier
        centre lies within ``h``; ``centre_of_seed`` is the lowest-numbered centre within ``h``, -1 for a dead seed."""
        self._euclidean_only("mean shift")
        m = self._queries(modes, False)
        if m.shape[1] != self._dim:
            raise ValueError(f"modes must have the tree's {self._dim} columns")
        ns = m.shape[0]
        pw = self._per_row(points_within, np.uint64, "points_within must hold one count per mode", ns)
        if np.ndim(h) != 0:
            raise ValueError("the merge takes one bandwidth")
        centres = np.zeros((ns, self._dim), dtype=self.dtype)
        cp = np.zeros(ns, dtype=np.uint64)
        cos = np.zeros(ns, dtype=np.int64)
        nc = C.c_uint64(0)
        check(self._fn("mean_shift_merge")(
            self._h, m.ctypes.data if ns else None, ns, pw.ctypes.data if ns else None, self._real(float(h)), 0,
            centres.ctypes.data, cp.ctypes.data, cos.ctypes.data, C.byref(nc)))
        k = int(nc.value)
        return centres[:k].copy(), cp[:k].copy(), cos

    def mean_shift_merge_device(self, modes, points_within, h, stream=None):
        """``mean_shift_merge`` in HBM: CUDA tensors in, ``(centres [ns][dim], centre_points int64 [ns], centre_of_seed int64
        [ns], n_centres int64 [1])`` out -- the first ``n_centres`` rows of the first two are written.  Never waits."""
        import torch
        self._euclidean_only("mean shift")
        modes, ns, qc, ptr, _ = self._device_queries(modes, f"modes ([ns][{self._dim}])", on_device=True, contiguous=True)
        if qc != self._dim:
            raise ValueError(f"modes must have the tree's {self._dim} columns")
        if not self._on_device(points_within, torch.int64, ns) or points_within.numel() != ns:
            raise ValueError("points_within must be a contiguous int64 CUDA tensor of one count per mode")
        if np.ndim(h) != 0:
            raise ValueError("the merge takes one bandwidth")
        dev = self._dev
        centres = torch.zeros((ns, self._dim), dtype=self._tdt, device=dev)
        cp = torch.zeros(ns, dtype=torch.int64, device=dev)
        cos = torch.zeros(ns, dtype=torch.int64, device=dev)
        nc = torch.zeros(1, dtype=torch.int64, device=dev)
        check(self._fn("mean_shift_merge_device")(
            self._h, ptr, ns, points_within.data_ptr() if ns else None, self._real(float(h)), 0, centres.data_ptr(),
            cp.data_ptr(), cos.data_ptr(), nc.data_ptr(), stream_arg(stream, dev)))
        return centres, cp, cos, nc

    def mean_shift_labels(self, centres, h, cluster_all: bool = True):
        """The nearest centre of every indexed row by (distance, centre number): ``int64 [n]``; with
        ``cluster_all=False`` a row whose nearest centre is not within ``h`` gets -1."""
        self._euclidean_only("mean shift")
        c = self._centres(centres)
        if np.ndim(h) != 0:
            raise ValueError("the labels take one bandwidth")
        labels = np.empty(self._n, dtype=np.int64)
        check(self._fn("mean_shift_labels")(
            self._h, c.ctypes.data if c.shape[0] else None, c.shape[0], self._real(float(h)),
            0 if cluster_all else _lib.PN_MS_ORPHANS, labels.ctypes.data))
        return labels

    def mean_shift_labels_device(self, centres, h, cluster_all: bool = True, n_centres=None, out_labels=None, stream=None):
        """``mean_shift_labels`` in HBM: ``centres`` a contiguous 2-D CUDA tensor, of which the first ``n_centres`` rows
        (default: all) are the centres; returns the labels, a CUDA int64 tensor.  Never waits."""
        import torch
        self._euclidean_only("mean shift")
        centres, rows, _ = self._centres_device(centres)
        nc = rows if n_centres is None else int(n_centres)
        if nc < 0 or nc > rows:
            raise ValueError("n_centres exceeds the rows of centres")
        if np.ndim(h) != 0:
            raise ValueError("the labels take one bandwidth")
        labels = self._out(out_labels, self._n, torch.int64, self._n)
        check(self._fn("mean_shift_labels_device")(
            self._h, centres.data_ptr() if nc else None, nc, self._real(float(h)),
            0 if cluster_all else _lib.PN_MS_ORPHANS, labels.data_ptr(), stream_arg(stream, self._dev)))
        return labels

    def mean_shift(self, h, seeds=None, cluster_all: bool = True, tol=None, max_iter: int = 300):
        """scikit-learn's ``MeanShift(bandwidth=h, seeds=seeds, cluster_all=cluster_all).fit(rows)``: ``(labels int64 [n],
        centres [nc][dim])``; ``last_n_iter`` holds the iterations run.  ``seeds=None``: every row is a seed
        (``mean_shift_bin_seeds`` gives scikit-learn's ``bin_seeding``)."""
        if np.ndim(h) != 0:
            raise ValueError("mean_shift takes one bandwidth")
        modes, pw = self.mean_shift_modes(h, seeds, tol, max_iter)
        centres, _, _ = self.mean_shift_merge(modes, pw, h)
        return self.mean_shift_labels(centres, h, cluster_all), centres
