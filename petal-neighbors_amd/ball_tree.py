"""Host mirror of ``petal_neighbors::BallTree`` (reference src/ball_tree.rs:15-374).

Same constructor names, argument meaning, result shapes and error behaviour as
the Rust type, so tests read like the reference's own; the work is done by the
HIP kernels behind the C ABI (``include/petal_mi355x.h``).  The ball tree walk
is not reproduced: ``BallTree`` here owns a zero-padded copy of the points in
HBM and answers queries by batched exact scans.

Batch methods (``query_batch`` etc.) are extensions: the reference takes one
point per call (src/ball_tree.rs:102); ``nq = 1`` is that call.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .distance import Euclidean
from .errors import check

ENGINES = {"auto": _lib.PN_ENGINE_AUTO, "exact": _lib.PN_ENGINE_EXACT, "mfma": _lib.PN_ENGINE_MFMA,
           "bf16": _lib.PN_ENGINE_BF16}


def _float_array(a):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):  # `A: FloatCore` is f32 or f64 in practice
        a = a.astype(np.float64)
    return a


KDE_KERNELS = {"gaussian": _lib.PN_KDE_GAUSSIAN, "tophat": _lib.PN_KDE_TOPHAT, "epanechnikov": _lib.PN_KDE_EPANECHNIKOV,
               "exponential": _lib.PN_KDE_EXPONENTIAL, "linear": _lib.PN_KDE_LINEAR}


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


class BallTree:
    """``BallTree<'a, A, Euclidean>``: ``points`` / ``metric`` stay readable like the pub fields
    at src/ball_tree.rs:20-23 (``idx`` and ``nodes`` do not exist: no tree is built)."""

    def __init__(self, handle, points, metric, dtype, device):
        self._h = C.c_void_p(handle)
        self.points = points
        self.metric = metric
        self.dtype = np.dtype(dtype)
        self.device = device
        self._sfx = "f32" if self.dtype == np.float32 else "f64"
        info = _lib.PnInfo()
        check(_lib.lib().pn_index_info(self._h, C.byref(info)))
        self._n, self._dim = int(info.n_points), int(info.dim)
        self.mfma_eligible = bool(info.mfma_eligible)
        self.bf16_eligible = bool(info.bf16_eligible)
        self.bf16_layout = int(info.bf16_layout)
        self.seed_model = bool(info.seed_model)

    # ------------------------------------------------------------ construction
    @classmethod
    def new(cls, points, metric, device: int = 0):
        """``BallTree::new(points, metric)`` (src/ball_tree.rs:38-63).

        Raises ``ArrayError.Empty`` for zero rows and ``ArrayError.NotContiguous`` when the
        inner stride is not 1 (only the inner stride is checked, as at :47)."""
        from .distance import Cosine
        if not isinstance(metric, (Euclidean, Cosine)):
            raise NotImplementedError("the MI355X path serves distance.Euclidean and distance.Cosine")
        cosine = isinstance(metric, Cosine)
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
        L = _lib.lib()
        h = C.c_void_p(0)
        # Cosine: an exact scan under Cosine::distance (it is not a metric: the reference's pruned walk can miss true
        # neighbours under it; include/petal_mi355x.h, pn_index_create_cosine_*)
        sfx = "f32" if a.dtype == np.float32 else "f64"
        fn = getattr(L, f"pn_index_create_cosine_{sfx}" if cosine else f"pn_index_create_{sfx}")
        check(fn(a.ctypes.data if a.size else None, n, d, rs, cs, device, C.byref(h)))
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
            from .errors import NotContiguous
            raise NotContiguous()
        n, d = tensor.shape
        dev = tensor.device.index or 0
        h = C.c_void_p(0)
        st = stream if stream is not None else torch.cuda.current_stream(tensor.device).cuda_stream
        f64 = tensor.dtype == torch.float64
        create = _lib.lib().pn_index_create_device_f64 if f64 else _lib.lib().pn_index_create_device_f32
        check(create(tensor.data_ptr() if n * d else None, n, d, tensor.stride(0) if n > 1 else max(d, 1), dev,
                     C.c_void_p(st), C.byref(h)))
        return cls(h.value, None, Euclidean(), np.float64 if f64 else np.float32, dev)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().pn_index_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    # ------------------------------------------------------------------ options
    def set_engine(self, name: str):
        check(_lib.lib().pn_index_set_option(self._h, _lib.PN_OPT_ENGINE, ENGINES[name]))
        return self

    def set_option(self, opt: int, value: int):
        check(_lib.lib().pn_index_set_option(self._h, opt, int(value)))
        return self

    def stats(self, reset: bool = False):
        s = _lib.PnStats()
        check(_lib.lib().pn_index_get_stats(self._h, C.byref(s), int(reset)))
        return {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}

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
        out = C.c_float(0) if self._sfx == "f32" else C.c_double(0)
        check(getattr(_lib.lib(), f"pn_tree_radius_of_{self._sfx}")(self._h, self._node(n), C.byref(out)))
        return self.dtype.type(out.value)

    def compare_nodes(self, x: int, y: int):
        """``BallTree::compare_nodes(x, y) -> Option<Ordering>`` by radius (src/ball_tree.rs:340-343):
        -1 / 0 / 1 for Less / Equal / Greater, None when a radius is NaN."""
        out = C.c_int(0)
        check(_lib.lib().pn_tree_compare_nodes(self._h, self._node(x), self._node(y), C.byref(out)))
        return None if out.value == 2 else int(out.value)

    def node_distance_lower_bound(self, n1: int, n2: int):
        """``BallTree::node_distance_lower_bound(n1, n2)`` = max(|c1 - c2| - R1 - R2, 0) (src/ball_tree.rs:303-318)."""
        out = C.c_float(0) if self._sfx == "f32" else C.c_double(0)
        check(getattr(_lib.lib(), f"pn_tree_node_distance_lower_bound_{self._sfx}")(self._h, self._node(n1), self._node(n2),
                                                                                      C.byref(out)))
        return self.dtype.type(out.value)

    def _centroid_of(self, n: int):
        c = np.empty(self._dim, dtype=self.dtype)
        check(_lib.lib().pn_tree_centroid_of(self._h, self._node(n), c.ctypes.data))
        return c

    # ------------------------------------------------------------------ queries
    def _queries(self, q, one: bool):
        a = np.ascontiguousarray(q, dtype=self.dtype)
        if one:
            if a.ndim != 1:
                raise ValueError("point must be 1-D (Ix1)")
            a = a.reshape(1, -1)
        elif a.ndim != 2:
            raise ValueError("queries must be 2-D")
        return a

    # One radius per query (``pn_query_radii_*``): the batch-shaped radius methods take, for ``distance`` / ``r``, a scalar
    # or a 1-D array of one radius per query (self-queries: per indexed row).  A scalar goes to the scalar entry points.
    def _radii(self, r, count):
        """None for a scalar radius, else the ``count`` radii as a contiguous array of the tree's dtype."""
        if np.ndim(r) == 0:
            return None
        if isinstance(r, np.ndarray) and r.dtype != self.dtype:
            raise ValueError(f"radii must have the tree's dtype {self.dtype}, not {r.dtype}")
        a = np.ascontiguousarray(r, dtype=self.dtype)
        if a.ndim != 1:
            raise ValueError("radii must be a scalar or 1-D")
        if a.shape[0] != count:
            raise ValueError(f"{a.shape[0]} radii for {count} queries")
        return a

    def _radii_device(self, r, count, dev):
        """None for a scalar radius, else ``r`` checked: ``count`` radii, a contiguous 1-D CUDA tensor of the tree's dtype
        on device ``dev`` (the call only enqueues work: the tensor is read later, so no temporary copy is made here)."""
        if np.ndim(r) == 0:  # (a tensor answers with its own .ndim: nothing is copied)
            return None
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        if not isinstance(r, torch.Tensor) or not r.is_cuda or r.dtype != tdt:
            raise ValueError("radii must be a scalar or a CUDA tensor of the tree's element type")
        if r.dim() != 1:
            raise ValueError("radii must be a scalar or 1-D")
        if r.shape[0] != count:
            raise ValueError(f"{r.shape[0]} radii for {count} queries")
        if r.device != dev:
            raise ValueError(f"radii are on {r.device}, the queries / the index on {dev}")
        if count > 1 and r.stride(0) != 1:
            raise ValueError("radii must be contiguous")
        return r

    def _csr_out(self, offsets, out_i, out_d, with_distance):
        """Copies of the library-allocated CSR lists (freed by the caller)."""
        total = int(offsets[-1])
        idx = np.empty(0, dtype=np.uint64)
        dist = np.empty(0, dtype=self.dtype) if with_distance else None
        if total:
            idx = np.frombuffer((C.c_uint64 * total).from_address(out_i.value), dtype=np.uint64).copy()
            if with_distance:
                ct = C.c_float if self._sfx == "f32" else C.c_double
                dist = np.frombuffer((ct * total).from_address(out_d.value), dtype=self.dtype).copy()
        return idx, dist

    def _query_radii(self, a, radii, with_distance, sort):
        nq, qc = a.shape
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        out_i, out_d = C.c_void_p(0), C.c_void_p(0)
        fn = getattr(_lib.lib(), f"pn_query_radii_{self._sfx}")
        try:
            check(fn(self._h, a.ctypes.data, nq, qc, max(qc, 1), radii.ctypes.data if nq else None,
                     _lib.PN_RADIUS_SORTED if sort else 0, offsets.ctypes.data, C.byref(out_i),
                     C.byref(out_d) if with_distance else None))
            idx, dist = self._csr_out(offsets, out_i, out_d, with_distance)
        finally:
            for p in (out_i, out_d):
                if p.value:
                    _lib.lib().pn_free(p)
        return offsets, idx, dist

    def query_batch(self, queries, k: int):
        """k-NN for every row of ``queries``: (nq, min(k, n)) indices (uint64) and distances."""
        a = self._queries(queries, False)
        nq, qc = a.shape
        kout = min(int(k), self._n)
        idx = np.empty((nq, kout), dtype=np.uint64)
        dist = np.empty((nq, kout), dtype=self.dtype)
        if nq and kout:
            fn = getattr(_lib.lib(), f"pn_query_{self._sfx}")
            check(fn(self._h, a.ctypes.data, nq, qc, max(qc, 1), int(k), idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def query(self, point, k: int):
        """``BallTree::query(point, k) -> (Vec<usize>, Vec<A>)`` ascending (src/ball_tree.rs:102-121);
        ``k == 0`` returns two empty arrays (:106-108)."""
        idx, dist = self.query_batch(self._queries(point, True), k)
        return idx[0], dist[0]

    def query_nearest(self, point):
        """``BallTree::query_nearest(point) -> (usize, A)`` (src/ball_tree.rs:80-86)."""
        a = self._queries(point, True)
        idx = np.empty(1, dtype=np.uint64)
        dist = np.empty(1, dtype=self.dtype)
        fn = getattr(_lib.lib(), f"pn_query_nearest_{self._sfx}")
        check(fn(self._h, a.ctypes.data, 1, a.shape[1], max(a.shape[1], 1), idx.ctypes.data, dist.ctypes.data))
        return int(idx[0]), dist[0]

    def query_radius_batch(self, queries, distance):
        """CSR (offsets[nq+1], indices) of ``{ i : dist(q, p_i) < distance }``, ascending per query.  ``distance``: a
        scalar, or a 1-D array of nq radii -- list q is then the scalar call's for query q with ``distance[q]``."""
        a = self._queries(queries, False)
        nq, qc = a.shape
        radii = self._radii(distance, nq)
        if radii is not None:
            return self._query_radii(a, radii, False, False)[:2]
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        out = C.c_void_p(0)
        r = C.c_float(distance) if self._sfx == "f32" else C.c_double(distance)
        fn = getattr(_lib.lib(), f"pn_query_radius_{self._sfx}")
        check(fn(self._h, a.ctypes.data, nq, qc, max(qc, 1), r, offsets.ctypes.data, C.byref(out)))
        total = int(offsets[-1])
        try:
            if total:
                buf = (C.c_uint64 * total).from_address(out.value)
                idx = np.frombuffer(buf, dtype=np.uint64).copy()
            else:
                idx = np.empty(0, dtype=np.uint64)
        finally:
            if out.value:
                _lib.lib().pn_free(out)
        return offsets, idx

    def query_radius(self, point, distance):
        """``BallTree::query_radius(point, distance) -> Vec<usize>`` (src/ball_tree.rs:137-142).
        The reference's order is unspecified (its tests sort, :667/:777); here: ascending."""
        _, idx = self.query_radius_batch(self._queries(point, True), distance)
        return idx

    def query_radius_with_distance_batch(self, queries, distance, sort: bool = False):
        """``query_radius_batch`` plus each neighbour's distance (``pn_query_radius_with_distance_*``):
        ``(offsets uint64 [nq+1], idx uint64, dist)``.  The lists are ascending by index, or by (distance, index) --
        nearest first, the k-NN order -- with ``sort=True``.  ``distance``: a scalar, or a 1-D array of nq radii."""
        a = self._queries(queries, False)
        nq, qc = a.shape
        radii = self._radii(distance, nq)
        if radii is not None:
            return self._query_radii(a, radii, True, sort)
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        out_i, out_d = C.c_void_p(0), C.c_void_p(0)
        r = C.c_float(distance) if self._sfx == "f32" else C.c_double(distance)
        flags = _lib.PN_RADIUS_SORTED if sort else 0
        fn = getattr(_lib.lib(), f"pn_query_radius_with_distance_{self._sfx}")
        try:
            check(fn(self._h, a.ctypes.data, nq, qc, max(qc, 1), r, flags, offsets.ctypes.data, C.byref(out_i),
                     C.byref(out_d)))
            total = int(offsets[-1])
            idx = np.empty(0, dtype=np.uint64)
            dist = np.empty(0, dtype=self.dtype)
            if total:
                idx = np.frombuffer((C.c_uint64 * total).from_address(out_i.value), dtype=np.uint64).copy()
                ct = C.c_float if self._sfx == "f32" else C.c_double
                dist = np.frombuffer((ct * total).from_address(out_d.value), dtype=self.dtype).copy()
        finally:
            for p in (out_i, out_d):
                if p.value:
                    _lib.lib().pn_free(p)
        return offsets, idx, dist

    def query_radius_with_distance(self, point, distance, sort: bool = False):
        """``query_radius(point, distance)`` and the distance of each neighbour: ``(idx, dist)``, ascending by index, or
        nearest first (by (distance, index)) with ``sort=True``."""
        _, idx, dist = self.query_radius_with_distance_batch(self._queries(point, True), distance, sort)
        return idx, dist

    # --------------------------------------------------------- device-resident
    def query_radius_device(self, queries, distance, capacity: int, out_offsets=None, out_idx=None, out_total=None,
                            stream=None):
        """``query_radius`` with queries and results in HBM, nothing read back (``pn_query_radius_device_*``).

        Returns CUDA tensors ``(offsets int64 [nq+1], idx int64 [capacity], total int64 [1])``: the CSR offsets are always
        complete; rows are written where their position is below ``capacity``; ``total > capacity`` (whenever the caller
        looks) means the buffer was too small -- call again with ``capacity >= total``."""
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        if queries.dtype != tdt or queries.dim() != 2 or not queries.is_cuda:
            raise ValueError("queries must be a 2-D CUDA tensor of the tree's element type")
        if queries.shape[1] > 1 and queries.stride(1) != 1:
            queries = queries.contiguous()
        nq, qc = queries.shape
        dev = queries.device
        offs = out_offsets if out_offsets is not None else torch.empty(nq + 1, dtype=torch.int64, device=dev)
        idx = out_idx if out_idx is not None else torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
        tot = out_total if out_total is not None else torch.empty(1, dtype=torch.int64, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        radii = self._radii_device(distance, nq, dev)
        if radii is not None:  # one radius per query
            fn = getattr(_lib.lib(), f"pn_query_radii_device_{self._sfx}")
            check(fn(self._h, queries.data_ptr() if nq * qc else None, nq, qc, queries.stride(0) if nq > 1 else max(qc, 1),
                     radii.data_ptr() if nq else None, 0, offs.data_ptr(), idx.data_ptr(), None, int(capacity),
                     tot.data_ptr(), C.c_void_p(st)))
            return offs, idx, tot
        r = C.c_float(distance) if self._sfx == "f32" else C.c_double(distance)
        fn = getattr(_lib.lib(), f"pn_query_radius_device_{self._sfx}")
        check(fn(self._h, queries.data_ptr() if nq * qc else None, nq, qc, queries.stride(0) if nq > 1 else max(qc, 1), r,
                 offs.data_ptr(), idx.data_ptr(), int(capacity), tot.data_ptr(), C.c_void_p(st)))
        return offs, idx, tot

    def query_radius_with_distance_device(self, queries, distance, capacity: int, sort: bool = False, out_offsets=None,
                                          out_idx=None, out_dist=None, out_total=None, stream=None):
        """``query_radius_device`` plus each neighbour's distance (``pn_query_radius_with_distance_device_*``):
        ``(offsets int64 [nq+1], idx int64 [capacity], dist [capacity], total int64 [1])`` as CUDA tensors.  With
        ``sort=True`` every list lying wholly below ``capacity`` is ordered by (distance, index); a list straddling the
        capacity is left unsorted."""
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        if not isinstance(queries, torch.Tensor) or queries.dtype != tdt or queries.dim() != 2 or not queries.is_cuda:
            raise ValueError("queries must be a 2-D CUDA tensor of the tree's element type")
        if int(capacity) < 0:
            raise ValueError("capacity must be >= 0")
        if queries.shape[1] > 1 and queries.stride(1) != 1:
            queries = queries.contiguous()
        nq, qc = queries.shape
        dev = queries.device
        cap = max(int(capacity), 1)
        offs = out_offsets if out_offsets is not None else torch.empty(nq + 1, dtype=torch.int64, device=dev)
        idx = out_idx if out_idx is not None else torch.empty(cap, dtype=torch.int64, device=dev)
        dist = out_dist if out_dist is not None else torch.empty(cap, dtype=tdt, device=dev)
        tot = out_total if out_total is not None else torch.empty(1, dtype=torch.int64, device=dev)
        if dist.dtype != tdt or idx.numel() < int(capacity) or dist.numel() < int(capacity) or offs.numel() < nq + 1:
            raise ValueError("output tensors are too small or of the wrong type")
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        flags = _lib.PN_RADIUS_SORTED if sort else 0
        radii = self._radii_device(distance, nq, dev)
        if radii is not None:  # one radius per query
            fn = getattr(_lib.lib(), f"pn_query_radii_device_{self._sfx}")
            check(fn(self._h, queries.data_ptr() if nq * qc else None, nq, qc, queries.stride(0) if nq > 1 else max(qc, 1),
                     radii.data_ptr() if nq else None, flags, offs.data_ptr(), idx.data_ptr(), dist.data_ptr(),
                     int(capacity), tot.data_ptr(), C.c_void_p(st)))
            return offs, idx, dist, tot
        r = C.c_float(distance) if self._sfx == "f32" else C.c_double(distance)
        fn = getattr(_lib.lib(), f"pn_query_radius_with_distance_device_{self._sfx}")
        check(fn(self._h, queries.data_ptr() if nq * qc else None, nq, qc, queries.stride(0) if nq > 1 else max(qc, 1), r,
                 flags, offs.data_ptr(), idx.data_ptr(), dist.data_ptr(), int(capacity), tot.data_ptr(), C.c_void_p(st)))
        return offs, idx, dist, tot

    def query_device(self, queries, k: int, out_idx=None, out_dist=None, stream=None):
        """k-NN with queries and results in HBM (torch CUDA tensors of the tree's element type; indices as int64)."""
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        if queries.dtype != tdt or queries.dim() != 2 or not queries.is_cuda:
            raise ValueError(f"queries must be a 2-D {tdt} CUDA tensor")
        if queries.shape[1] > 1 and queries.stride(1) != 1:
            queries = queries.contiguous()
        nq, qc = queries.shape
        kout = min(int(k), self._n)
        if out_idx is None:
            out_idx = torch.empty((nq, kout), dtype=torch.int64, device=queries.device)
        if out_dist is None:
            out_dist = torch.empty((nq, kout), dtype=tdt, device=queries.device)
        if nq and kout:
            st = stream if stream is not None else torch.cuda.current_stream(queries.device).cuda_stream
            check(getattr(_lib.lib(), f"pn_query_device_{self._sfx}")(self._h, queries.data_ptr(), nq, qc,
                                                 queries.stride(0) if nq > 1 else max(qc, 1), int(k),
                                                 out_idx.data_ptr(), out_dist.data_ptr(), C.c_void_p(st)))
        return out_idx, out_dist

    # ------------------------------------------------------------- self-queries
    # Every indexed row against its own index, the row itself left out (``pn_query_self_*`` / ``pn_query_radius_self_*``):
    # the rows already in HBM are the queries -- nothing is sent up again.
    def _self_flags(self, include_self, sort=False):
        return (_lib.PN_SELF_INCLUDE if include_self else 0) | (_lib.PN_RADIUS_SORTED if sort else 0)

    def _self_k(self, k, include_self):
        if int(k) < 0:
            raise ValueError("k must be >= 0")
        return min(int(k), self._n if include_self else self._n - 1)

    def query_self(self, k: int, include_self: bool = False):
        """The k nearest OTHER rows of every indexed row: ``(idx uint64 [n, kout], dist [n, kout])``, kout = min(k, n - 1),
        each row's list ordered by (distance, index).  ``include_self=True``: the row stays in its own list, kout =
        min(k, n) -- ``query_batch(rows, k)``."""
        kout = self._self_k(k, include_self)
        idx = np.empty((self._n, kout), dtype=np.uint64)
        dist = np.empty((self._n, kout), dtype=self.dtype)
        if kout:
            fn = getattr(_lib.lib(), f"pn_query_self_{self._sfx}")
            check(fn(self._h, int(k), self._self_flags(include_self), idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def query_self_device(self, k: int, include_self: bool = False, out_idx=None, out_dist=None, stream=None):
        """``query_self`` with the results in HBM: CUDA tensors ``(idx int64 [n, kout], dist [n, kout])``, enqueued on
        ``stream`` (default: the current torch stream)."""
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        kout = self._self_k(k, include_self)
        dev = torch.device("cuda", self.device)
        if out_idx is None:
            out_idx = torch.empty((self._n, kout), dtype=torch.int64, device=dev)
        if out_dist is None:
            out_dist = torch.empty((self._n, kout), dtype=tdt, device=dev)
        if out_dist.dtype != tdt or out_idx.numel() < self._n * kout or out_dist.numel() < self._n * kout:
            raise ValueError("output tensors are too small or of the wrong type")
        if kout:
            st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
            check(getattr(_lib.lib(), f"pn_query_self_device_{self._sfx}")(
                self._h, int(k), self._self_flags(include_self), out_idx.data_ptr(), out_dist.data_ptr(), C.c_void_p(st)))
        return out_idx, out_dist

    def query_radius_self(self, r, with_distance: bool = False, sort: bool = False, include_self: bool = False):
        """``{ j != i : distance(p_i, p_j) < r }`` for every indexed row i, as CSR: ``(offsets uint64 [n+1], idx uint64,
        dist or None)``; lists ascending by index, or by (distance, index) with ``sort=True`` (needs ``with_distance``).
        ``include_self=True`` keeps row i wherever its distance to itself is below r.  ``r``: a scalar, or a 1-D array of
        n radii, row i's own (``pn_query_radii_self_*``)."""
        if sort and not with_distance:
            raise ValueError("sort=True needs with_distance=True")
        radii = self._radii(r, self._n)
        offsets = np.zeros(self._n + 1, dtype=np.uint64)
        out_i, out_d = C.c_void_p(0), C.c_void_p(0)
        if radii is not None:
            rr = radii.ctypes.data
            fn = getattr(_lib.lib(), f"pn_query_radii_self_{self._sfx}")
        else:
            rr = C.c_float(r) if self._sfx == "f32" else C.c_double(r)
            fn = getattr(_lib.lib(), f"pn_query_radius_self_{self._sfx}")
        try:
            check(fn(self._h, rr, self._self_flags(include_self, sort), offsets.ctypes.data, C.byref(out_i),
                     C.byref(out_d) if with_distance else None))
            total = int(offsets[-1])
            idx = np.empty(0, dtype=np.uint64)
            dist = np.empty(0, dtype=self.dtype) if with_distance else None
            if total:
                idx = np.frombuffer((C.c_uint64 * total).from_address(out_i.value), dtype=np.uint64).copy()
                if with_distance:
                    ct = C.c_float if self._sfx == "f32" else C.c_double
                    dist = np.frombuffer((ct * total).from_address(out_d.value), dtype=self.dtype).copy()
        finally:
            for p in (out_i, out_d):
                if p.value:
                    _lib.lib().pn_free(p)
        return offsets, idx, dist

    def query_radius_self_device(self, r, capacity: int, with_distance: bool = False, sort: bool = False,
                                 include_self: bool = False, out_offsets=None, out_idx=None, out_dist=None, out_total=None,
                                 stream=None):
        """``query_radius_self`` in HBM with the capacity contract of ``query_radius_with_distance_device``: CUDA tensors
        ``(offsets int64 [n+1], idx int64 [capacity], dist [capacity] or None, total int64 [1])``.  ``r``: a scalar, or a
        1-D CUDA tensor of n radii of the tree's element type."""
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        if int(capacity) < 0:
            raise ValueError("capacity must be >= 0")
        if sort and not with_distance:
            raise ValueError("sort=True needs with_distance=True")
        dev = torch.device("cuda", self.device)
        radii = self._radii_device(r, self._n, dev)
        cap = max(int(capacity), 1)
        offs = out_offsets if out_offsets is not None else torch.empty(self._n + 1, dtype=torch.int64, device=dev)
        idx = out_idx if out_idx is not None else torch.empty(cap, dtype=torch.int64, device=dev)
        dist = None
        if with_distance:
            dist = out_dist if out_dist is not None else torch.empty(cap, dtype=tdt, device=dev)
            if dist.dtype != tdt or dist.numel() < int(capacity):
                raise ValueError("output tensors are too small or of the wrong type")
        tot = out_total if out_total is not None else torch.empty(1, dtype=torch.int64, device=dev)
        if idx.numel() < int(capacity) or offs.numel() < self._n + 1:
            raise ValueError("output tensors are too small")
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        if radii is not None:
            rr = radii.data_ptr()
            fn = getattr(_lib.lib(), f"pn_query_radii_self_device_{self._sfx}")
        else:
            rr = C.c_float(r) if self._sfx == "f32" else C.c_double(r)
            fn = getattr(_lib.lib(), f"pn_query_radius_self_device_{self._sfx}")
        check(fn(self._h, rr, self._self_flags(include_self, sort), offs.data_ptr(), idx.data_ptr(),
                 dist.data_ptr() if dist is not None else None, int(capacity), tot.data_ptr(), C.c_void_p(st)))
        return offs, idx, dist, tot

    # ------------------------------------------------------------------- DBSCAN
    def _dbscan_args(self, eps, min_samples):
        if int(min_samples) < 1:
            raise ValueError("min_samples must be >= 1")
        return (C.c_float(eps) if self._sfx == "f32" else C.c_double(eps)), int(min_samples)

    def dbscan(self, eps, min_samples: int):
        """DBSCAN of the indexed rows on the device (``pn_dbscan_*``): ``(labels int64 [n], core bool [n])``.  Row i's
        neighbourhood is ``{ j : distance(p_i, p_j) < eps }`` (itself included where its own distance is below eps), a
        core row has at least ``min_samples`` of them, clusters are numbered by ascending lowest core row, a border row
        takes the lowest-numbered cluster among its core neighbours, noise is -1."""
        e, m = self._dbscan_args(eps, min_samples)
        labels = np.empty(self._n, dtype=np.int64)
        core = np.empty(self._n, dtype=np.uint8)
        check(getattr(_lib.lib(), f"pn_dbscan_{self._sfx}")(self._h, e, m, 0, labels.ctypes.data, core.ctypes.data, None))
        return labels, core.astype(bool)

    def dbscan_device(self, eps, min_samples: int, out_labels=None, out_core=None, out_n_clusters=None, stream=None):
        """``dbscan`` with the results in HBM: CUDA tensors ``(labels int64 [n], core uint8 [n], n_clusters int64 [1])``,
        written in stream order on ``stream`` (default: the current torch stream).  The call waits for the device once."""
        e, m = self._dbscan_args(eps, min_samples)
        import torch
        dev = torch.device("cuda", self.device)
        labels = out_labels if out_labels is not None else torch.empty(self._n, dtype=torch.int64, device=dev)
        core = out_core if out_core is not None else torch.empty(self._n, dtype=torch.uint8, device=dev)
        ncl = out_n_clusters if out_n_clusters is not None else torch.empty(1, dtype=torch.int64, device=dev)
        if labels.dtype != torch.int64 or core.dtype != torch.uint8 or ncl.dtype != torch.int64 or \
                labels.numel() < self._n or core.numel() < self._n or ncl.numel() < 1:
            raise ValueError("output tensors are too small or of the wrong type")
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_dbscan_device_{self._sfx}")(
            self._h, e, m, 0, labels.data_ptr(), core.data_ptr(), ncl.data_ptr(), C.c_void_p(st)))
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
            c = np.ascontiguousarray(core, dtype=self.dtype)
            if c.ndim != 1 or c.shape[0] != self._n:
                raise ValueError(f"core must hold one value per indexed row ({self._n})")
        ne = max(self._n - 1, 0)
        src = np.empty(ne, dtype=np.uint64)
        dst = np.empty(ne, dtype=np.uint64)
        weight = np.empty(ne, dtype=self.dtype)
        work = np.zeros(2, dtype=np.uint64)
        check(getattr(_lib.lib(), f"pn_mst_{self._sfx}")(self._h, c.ctypes.data if c is not None else None, 0,
                                                       src.ctypes.data, dst.ctypes.data, weight.ctypes.data,
                                                       work.ctypes.data))
        self.last_mst_work = (int(work[0]), int(work[1]))
        return src, dst, weight

    def mst_device(self, core=None, out_src=None, out_dst=None, out_weight=None, stream=None):
        """``mst`` in HBM: ``core`` None or a 1-D CUDA tensor of n values of the tree's element type; CUDA tensors
        ``(src int64 [n-1], dst int64 [n-1], weight [n-1])`` written in stream order on ``stream`` (default: the current
        torch stream).  The call waits for the device once per Boruvka round."""
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
        ne = max(self._n - 1, 0)
        if core is not None:
            if not isinstance(core, torch.Tensor):
                raise ValueError("core must be a CUDA tensor (or None)")
            if core.dtype != tdt or core.dim() != 1 or core.numel() != self._n or not core.is_cuda:
                raise ValueError(f"core must be a 1-D CUDA tensor of {self._n} values of the tree's element type")
            core = core.contiguous()
        for t, want in ((out_src, torch.int64), (out_dst, torch.int64), (out_weight, tdt)):
            if t is not None and (t.dtype != want or t.numel() < ne or not t.is_contiguous()):
                raise ValueError("output tensors are too small or of the wrong type")
        src = out_src if out_src is not None else torch.empty(ne, dtype=torch.int64, device=dev)
        dst = out_dst if out_dst is not None else torch.empty(ne, dtype=torch.int64, device=dev)
        weight = out_weight if out_weight is not None else torch.empty(ne, dtype=tdt, device=dev)
        work = np.zeros(2, dtype=np.uint64)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_mst_device_{self._sfx}")(
            self._h, core.data_ptr() if core is not None else None, 0, src.data_ptr(), dst.data_ptr(), weight.data_ptr(),
            work.ctypes.data, C.c_void_p(st)))
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
        src = np.ascontiguousarray(edges[0], dtype=np.uint64)
        dst = np.ascontiguousarray(edges[1], dtype=np.uint64)
        w = np.ascontiguousarray(edges[2], dtype=self.dtype)
        for t in (src, dst, w):
            if t.ndim != 1 or t.shape[0] != ne:
                raise ValueError(f"edges must be three arrays of n - 1 = {ne} values")
        left = np.empty(ne, dtype=np.uint64)
        right = np.empty(ne, dtype=np.uint64)
        weight = np.empty(ne, dtype=self.dtype)
        size = np.empty(ne, dtype=np.uint64)
        check(getattr(_lib.lib(), f"pn_linkage_{self._sfx}")(
            self._h, src.ctypes.data, dst.ctypes.data, w.ctypes.data, 0, left.ctypes.data, right.ctypes.data,
            weight.ctypes.data, size.ctypes.data))
        return left, right, weight, size

    def linkage_device(self, core=None, edges=None, out_left=None, out_right=None, out_weight=None, out_size=None,
                       out_error=None, stream=None):
        """``linkage`` in HBM: ``edges`` are CUDA tensors ``(src int64, dst int64, weight)`` (default:
        ``mst_device(core)``); returns CUDA tensors ``(left int64, right int64, weight, size int64, error int32 [1])``
        written in stream order on ``stream`` (default: the current torch stream) without waiting for the device.
        ``error[0]`` is 0, or ``PN_ERR_INVALID`` when the edges are no spanning tree."""
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
        ne = max(self._n - 1, 0)
        if edges is None:
            edges = self.mst_device(core, stream=stream)
        elif core is not None:
            raise ValueError("give core or edges, not both")
        src, dst, w = edges
        for t, want in ((src, torch.int64), (dst, torch.int64), (w, tdt)):
            if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != want or t.dim() != 1 or t.numel() != ne
                    or not t.is_contiguous()):
                raise ValueError(f"edges must be three contiguous 1-D CUDA tensors of n - 1 = {ne} values (int64, int64, "
                                 "the tree's element type)")
        for t, want, need in ((out_left, torch.int64, ne), (out_right, torch.int64, ne), (out_weight, tdt, ne),
                              (out_size, torch.int64, ne), (out_error, torch.int32, 1)):
            if t is not None and (t.dtype != want or t.numel() < need or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("output tensors are too small or of the wrong type")
        left = out_left if out_left is not None else torch.empty(ne, dtype=torch.int64, device=dev)
        right = out_right if out_right is not None else torch.empty(ne, dtype=torch.int64, device=dev)
        weight = out_weight if out_weight is not None else torch.empty(ne, dtype=tdt, device=dev)
        size = out_size if out_size is not None else torch.empty(ne, dtype=torch.int64, device=dev)
        err = out_error if out_error is not None else torch.zeros(1, dtype=torch.int32, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_linkage_device_{self._sfx}")(
            self._h, src.data_ptr(), dst.data_ptr(), w.data_ptr(), 0, left.data_ptr(), right.data_ptr(), weight.data_ptr(),
            size.data_ptr(), err.data_ptr(), C.c_void_p(st)))
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
        check(getattr(_lib.lib(), f"pn_hdbscan_{self._sfx}")(self._h, k, m, 0, labels.ctypes.data, prob.ctypes.data,
                                                            ncl.ctypes.data))
        self.last_n_clusters = int(ncl[0])
        return labels, prob

    def hdbscan_device(self, min_cluster_size, min_samples=None, out_labels=None, out_probabilities=None,
                       out_n_clusters=None, stream=None):
        """``hdbscan`` in HBM: CUDA tensors ``(labels int64 [n], probabilities [n], n_clusters int64 [1])`` written in
        stream order on ``stream`` (default: the current torch stream).  The call waits for the device once per Boruvka
        round of the tree and not after it."""
        import torch
        m, k = self._hdbscan_args(min_cluster_size, min_samples)
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
        n = self._n
        for t, want, need in ((out_labels, torch.int64, n), (out_probabilities, tdt, n), (out_n_clusters, torch.int64, 1)):
            if t is not None and (t.dtype != want or t.numel() < need or not t.is_contiguous() or not t.is_cuda):
                raise ValueError("output tensors are too small or of the wrong type")
        labels = out_labels if out_labels is not None else torch.empty(n, dtype=torch.int64, device=dev)
        prob = out_probabilities if out_probabilities is not None else torch.empty(n, dtype=tdt, device=dev)
        ncl = out_n_clusters if out_n_clusters is not None else torch.zeros(1, dtype=torch.int64, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_hdbscan_device_{self._sfx}")(
            self._h, k, m, 0, labels.data_ptr(), prob.data_ptr(), ncl.data_ptr(), C.c_void_p(st)))
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

    def _lof_on_device(self, t, want, need):
        """``t`` is a contiguous CUDA tensor of dtype ``want`` on the tree's device with at least ``need`` elements"""
        import torch
        return (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype == want
                and t.numel() >= need and t.is_contiguous())

    def lof(self, k: int = 20, full: bool = False):
        """Local Outlier Factor of every indexed row over its ``k`` nearest OTHER rows: ``scores float64 [n]``, or
        ``(scores, lrd float64 [n], kdist [n])`` with ``full=True``."""
        k = self._lof_k(k)
        scores = np.empty(self._n, dtype=np.float64)
        lrd = np.empty(self._n, dtype=np.float64) if full else None
        kdist = np.empty(self._n, dtype=self.dtype) if full else None
        check(getattr(_lib.lib(), f"pn_lof_{self._sfx}")(self._h, k, 0, scores.ctypes.data,
                                                        lrd.ctypes.data if full else None,
                                                        kdist.ctypes.data if full else None))
        return (scores, lrd, kdist) if full else scores

    def lof_device(self, k: int = 20, out_lof=None, out_lrd=None, out_kdist=None, stream=None):
        """``lof`` in HBM: CUDA tensors ``(lof float64 [n], lrd float64 [n], kdist [n])`` written in stream order on
        ``stream`` (default: the current torch stream); the call does not wait for the device."""
        import torch
        k = self._lof_k(k)
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
        n = self._n
        for t, want in ((out_lof, torch.float64), (out_lrd, torch.float64), (out_kdist, tdt)):
            if t is not None and not self._lof_on_device(t, want, n):
                raise ValueError(f"output tensors must be contiguous CUDA tensors of at least {n} values on the tree's "
                                 "device (float64; kdist of the tree's element type)")
        lof = out_lof if out_lof is not None else torch.empty(n, dtype=torch.float64, device=dev)
        lrd = out_lrd if out_lrd is not None else torch.empty(n, dtype=torch.float64, device=dev)
        kdist = out_kdist if out_kdist is not None else torch.empty(n, dtype=tdt, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_lof_device_{self._sfx}")(self._h, k, 0, lof.data_ptr(), lrd.data_ptr(),
                                                               kdist.data_ptr(), C.c_void_p(st)))
        return lof, lrd, kdist

    def lof_score(self, queries, k: int, lrd, kdist):
        """Outlier scores ``float64 [nq]`` of new points against a fit: ``lrd`` and ``kdist`` are ``lof(k, full=True)``'s,
        with the same ``k``.  A fitted row scored here finds itself at distance 0, so it does not reproduce its fit score
        (scikit-learn's ``score_samples`` behaves the same way)."""
        k = self._lof_k(k)
        lrd = np.ascontiguousarray(lrd, dtype=np.float64)
        kdist = np.ascontiguousarray(kdist, dtype=self.dtype)
        if lrd.ndim != 1 or lrd.shape[0] != self._n or kdist.ndim != 1 or kdist.shape[0] != self._n:
            raise ValueError(f"lrd and kdist must hold one value per indexed row ({self._n})")
        a = self._queries(queries, False)
        nq, qc = a.shape
        scores = np.empty(nq, dtype=np.float64)
        if nq:
            check(getattr(_lib.lib(), f"pn_lof_score_{self._sfx}")(
                self._h, a.ctypes.data, nq, qc, max(qc, 1), k, lrd.ctypes.data, kdist.ctypes.data, 0, scores.ctypes.data))
        return scores

    def lof_score_device(self, queries, k: int, lrd, kdist, out=None, stream=None):
        """``lof_score`` in HBM: ``queries`` a 2-D CUDA tensor of the tree's element type, ``lrd`` (float64) and ``kdist``
        contiguous 1-D CUDA tensors of n values (``lof_device``'s); returns the CUDA tensor ``scores float64 [nq]``,
        written in stream order on ``stream`` (default: the current torch stream)."""
        import torch
        k = self._lof_k(k)
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        for t, want in ((lrd, torch.float64), (kdist, tdt)):
            if not self._lof_on_device(t, want, self._n) or t.dim() != 1 or t.numel() != self._n:
                raise ValueError(f"lrd and kdist must be contiguous 1-D CUDA tensors of {self._n} values on the tree's "
                                 "device (float64, the tree's element type)")
        if (not isinstance(queries, torch.Tensor) or queries.dtype != tdt or queries.dim() != 2 or not queries.is_cuda
                or queries.device.index != self.device):
            raise ValueError(f"queries must be a 2-D {tdt} CUDA tensor on the tree's device")
        if queries.shape[1] > 1 and queries.stride(1) != 1:
            queries = queries.contiguous()
        nq, qc = queries.shape
        if out is not None and not self._lof_on_device(out, torch.float64, nq):
            raise ValueError(f"out must be a contiguous float64 CUDA tensor of at least {nq} values on the tree's device")
        scores = out if out is not None else torch.empty(nq, dtype=torch.float64, device=queries.device)
        if nq:
            st = stream if stream is not None else torch.cuda.current_stream(queries.device).cuda_stream
            check(getattr(_lib.lib(), f"pn_lof_score_device_{self._sfx}")(
                self._h, queries.data_ptr(), nq, qc, queries.stride(0) if nq > 1 else max(qc, 1), k, lrd.data_ptr(),
                kdist.data_ptr(), 0, scores.data_ptr(), C.c_void_p(st)))
        return scores

    # ------------------------------------------------------------------- OPTICS
    # scikit-learn's ``OPTICS(min_samples + 1, max_eps)`` on the device (``pn_optics_*``): the ordering, the reachability
    # plot, predecessors and core distances, and (``optics_dbscan``) the DBSCAN labels at any eps <= max_eps read off the
    # ordering.  ``min_samples`` counts OTHER rows; every radius is a strict '<'.  ``ordering`` holds plain row numbers
    # (no ``PN_OPT_INDEX_BASE``): it indexes the other arrays.
    def _optics_args(self, min_samples, max_eps):
        k = int(min_samples)
        if k < 1 or (self._n >= 2 and k > self._n - 1):
            raise ValueError(f"min_samples must be in [1, n - 1] = [1, {max(self._n - 1, 1)}]")
        return k, (C.c_float(max_eps) if self._sfx == "f32" else C.c_double(max_eps))

    def optics(self, min_samples: int, max_eps=np.inf):
        """``(ordering uint64 [n], reachability [n], predecessor int64 [n], core_distances [n])``: rows in the order
        OPTICS visits them; ``reachability`` / ``predecessor`` / ``core_distances`` are indexed by row (+inf, -1, +inf
        where undefined)."""
        k, e = self._optics_args(min_samples, max_eps)
        ordering = np.empty(self._n, dtype=np.uint64)
        reach = np.empty(self._n, dtype=self.dtype)
        pred = np.empty(self._n, dtype=np.int64)
        core = np.empty(self._n, dtype=self.dtype)
        check(getattr(_lib.lib(), f"pn_optics_{self._sfx}")(self._h, k, e, 0, ordering.ctypes.data, reach.ctypes.data,
                                                           pred.ctypes.data, core.ctypes.data))
        return ordering, reach, pred, core

    def optics_device(self, min_samples: int, max_eps=np.inf, out_ordering=None, out_reachability=None,
                      out_predecessor=None, out_core=None, stream=None):
        """``optics`` in HBM: CUDA tensors ``(ordering int64 [n], reachability [n], predecessor int64 [n],
        core_distances [n])`` written in stream order on ``stream`` (default: the current torch stream).  The call waits
        for the device once, after the counting pass."""
        import torch
        k, e = self._optics_args(min_samples, max_eps)
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
        n = self._n
        for t, want in ((out_ordering, torch.int64), (out_reachability, tdt), (out_predecessor, torch.int64), (out_core, tdt)):
            if t is not None and not self._lof_on_device(t, want, n):
                raise ValueError(f"output tensors must be contiguous CUDA tensors of at least {n} values on the tree's "
                                 "device (int64; reachability and core distances of the tree's element type)")
        ordering = out_ordering if out_ordering is not None else torch.empty(n, dtype=torch.int64, device=dev)
        reach = out_reachability if out_reachability is not None else torch.empty(n, dtype=tdt, device=dev)
        pred = out_predecessor if out_predecessor is not None else torch.empty(n, dtype=torch.int64, device=dev)
        core = out_core if out_core is not None else torch.empty(n, dtype=tdt, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_optics_device_{self._sfx}")(
            self._h, k, e, 0, ordering.data_ptr(), reach.data_ptr(), pred.data_ptr(), core.data_ptr(), C.c_void_p(st)))
        return ordering, reach, pred, core

    def optics_dbscan(self, eps, ordering, reachability, core_distances):
        """``(labels int64 [n], n_clusters)``: the DBSCAN labels at ``eps`` (<= the ordering's max_eps) read off
        ``optics``'s outputs; clusters are numbered by first appearance in the ordering, noise is -1.  An ordering that
        is no permutation of the rows raises ``PetalError``."""
        o = np.ascontiguousarray(ordering, dtype=np.uint64)
        r = np.ascontiguousarray(reachability, dtype=self.dtype)
        c = np.ascontiguousarray(core_distances, dtype=self.dtype)
        for a in (o, r, c):
            if a.ndim != 1 or a.shape[0] != self._n:
                raise ValueError(f"ordering, reachability and core_distances must hold one value per indexed row ({self._n})")
        e = C.c_float(eps) if self._sfx == "f32" else C.c_double(eps)
        labels = np.empty(self._n, dtype=np.int64)
        ncl = np.zeros(1, dtype=np.uint64)
        check(getattr(_lib.lib(), f"pn_optics_dbscan_{self._sfx}")(self._h, o.ctypes.data, r.ctypes.data, c.ctypes.data, e, 0,
                                                                  labels.ctypes.data, ncl.ctypes.data))
        return labels, int(ncl[0])

    def optics_dbscan_device(self, eps, ordering, reachability, core_distances, out_labels=None, out_n_clusters=None,
                             out_error=None, stream=None):
        """``optics_dbscan`` in HBM: the inputs are ``optics_device``'s tensors; returns CUDA tensors ``(labels int64 [n],
        n_clusters int64 [1], error int32 [1])`` written in stream order on ``stream`` (default: the current torch
        stream) without waiting for the device.  ``error[0]`` is 0, or ``PN_ERR_INVALID`` when the ordering is no
        permutation of the rows."""
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        n = self._n
        for t, want in ((ordering, torch.int64), (reachability, tdt), (core_distances, tdt)):
            if not self._lof_on_device(t, want, n) or t.dim() != 1 or t.numel() != n:
                raise ValueError(f"ordering, reachability and core_distances must be contiguous 1-D CUDA tensors of {n} "
                                 "values on the tree's device (int64, the tree's element type)")
        for t, want, need in ((out_labels, torch.int64, n), (out_n_clusters, torch.int64, 1), (out_error, torch.int32, 1)):
            if t is not None and not self._lof_on_device(t, want, need):
                raise ValueError("output tensors are too small or of the wrong type")
        dev = torch.device("cuda", self.device)
        labels = out_labels if out_labels is not None else torch.empty(n, dtype=torch.int64, device=dev)
        ncl = out_n_clusters if out_n_clusters is not None else torch.zeros(1, dtype=torch.int64, device=dev)
        err = out_error if out_error is not None else torch.zeros(1, dtype=torch.int32, device=dev)
        e = C.c_float(eps) if self._sfx == "f32" else C.c_double(eps)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_optics_dbscan_device_{self._sfx}")(
            self._h, ordering.data_ptr(), reachability.data_ptr(), core_distances.data_ptr(), e, 0, labels.data_ptr(),
            ncl.data_ptr(), err.data_ptr(), C.c_void_p(st)))
        return labels, ncl, err

    # -------------------------------------------------- kernel density estimation
    # scikit-learn's ``BallTree.kernel_density`` on the device (``pn_kde_*``): per query the sum of the kernel over the rows
    # within the kernel's cutoff, one wave per query in a fixed order.  ``h`` is a scalar or one bandwidth per query (the
    # balloon estimator); ``atol`` lets the two smooth kernels stop at a finite cutoff (``sum_all - atol <= sum <= sum_all``);
    # with ``atol=0`` they visit every row.  Every comparison is a strict '<'.
    def _kde_args(self, h, kernel, atol, count, normalize=False):
        """(kernel number, the bandwidths as a contiguous array of the tree's dtype: one, or ``count``)"""
        if kernel not in KDE_KERNELS:
            raise ValueError(f"unknown kernel {kernel!r}: one of {sorted(KDE_KERNELS)}")
        atol = float(atol)
        if not (atol >= 0.0) or math.isinf(atol):
            raise ValueError("atol must be finite and >= 0")
        if normalize:
            from .distance import Cosine
            if isinstance(self.metric, Cosine):
                raise ValueError("normalize=True needs a Euclidean tree: the normalisers are volumes of Euclidean balls")
        ha = self._radii(h, count)
        if ha is None:
            ha = np.array([h], dtype=self.dtype)
            if not (ha[0] > 0) or not np.isfinite(ha[0]):
                raise ValueError("the bandwidth must be finite and positive")
        return KDE_KERNELS[kernel], ha

    def _kde_finish(self, s, ha, kernel, return_log, normalize):
        with np.errstate(divide="ignore", invalid="ignore"):
            if return_log:
                out = np.log(s)
                return out + kde_log_norm(kernel, self._dim, ha if ha.shape[0] > 1 else ha[0]) if normalize else out
            return s * np.exp(kde_log_norm(kernel, self._dim, ha if ha.shape[0] > 1 else ha[0])) if normalize else s

    def kernel_density(self, queries, h, kernel: str = "gaussian", atol: float = 0.0, return_log: bool = False,
                       normalize: bool = True):
        """Kernel density of every row of ``queries``: ``float64 [nq]``.  With ``normalize`` the kernel's normaliser for the
        row dimension is applied, as scikit-learn's ``BallTree.kernel_density`` does; the result is not divided by n.  An
        empty list gives 0 (``-inf`` with ``return_log``)."""
        a = self._queries(queries, False)
        nq, qc = a.shape
        kn, ha = self._kde_args(h, kernel, atol, nq, normalize)
        s = np.zeros(nq, dtype=np.float64)
        if nq:
            check(getattr(_lib.lib(), f"pn_kde_{self._sfx}")(self._h, a.ctypes.data, nq, qc, max(qc, 1), ha.ctypes.data,
                                                            ha.shape[0], kn, float(atol), 0, s.ctypes.data, None, None))
        return self._kde_finish(s, ha, kernel, return_log, normalize)

    def kernel_density_self(self, h, kernel: str = "gaussian", atol: float = 0.0, return_log: bool = False,
                            normalize: bool = True, include_self: bool = False):
        """``kernel_density`` of the indexed rows themselves; by default each row is left out of its own estimate (the
        leave-one-out density)."""
        kn, ha = self._kde_args(h, kernel, atol, self._n, normalize)
        s = np.zeros(self._n, dtype=np.float64)
        check(getattr(_lib.lib(), f"pn_kde_self_{self._sfx}")(self._h, ha.ctypes.data, ha.shape[0], kn, float(atol),
                                                             _lib.PN_SELF_INCLUDE if include_self else 0, s.ctypes.data,
                                                             None, None))
        return self._kde_finish(s, ha, kernel, return_log, normalize)

    def kernel_density_raw(self, queries, h, kernel: str = "gaussian", atol: float = 0.0, include_self: bool = False):
        """The C ABI's three outputs on the host: ``(sum float64, count uint64, cutoff)`` per query; ``queries=None``: the
        indexed rows themselves (``include_self`` as in ``kernel_density_self``)."""
        if queries is None:
            nq = self._n
            kn, ha = self._kde_args(h, kernel, atol, nq)
        else:
            a = self._queries(queries, False)
            nq, qc = a.shape
            kn, ha = self._kde_args(h, kernel, atol, nq)
        s = np.zeros(nq, dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.uint64)
        cut = np.zeros(nq, dtype=self.dtype)
        if queries is None:
            check(getattr(_lib.lib(), f"pn_kde_self_{self._sfx}")(
                self._h, ha.ctypes.data, ha.shape[0], kn, float(atol), _lib.PN_SELF_INCLUDE if include_self else 0,
                s.ctypes.data, cnt.ctypes.data, cut.ctypes.data))
        elif nq:
            check(getattr(_lib.lib(), f"pn_kde_{self._sfx}")(self._h, a.ctypes.data, nq, qc, max(qc, 1), ha.ctypes.data,
                                                            ha.shape[0], kn, float(atol), 0, s.ctypes.data, cnt.ctypes.data,
                                                            cut.ctypes.data))
        return s, cnt, cut

    def _kde_device_args(self, h, kernel, atol, count, outs):
        import torch
        if kernel not in KDE_KERNELS:
            raise ValueError(f"unknown kernel {kernel!r}: one of {sorted(KDE_KERNELS)}")
        atol = float(atol)
        if not (atol >= 0.0) or math.isinf(atol):
            raise ValueError("atol must be finite and >= 0")
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
        ht = self._radii_device(h, count, dev)
        if ht is None and (not (float(h) > 0.0) or math.isinf(float(h))):
            raise ValueError("the bandwidth must be finite and positive")
        for t, want in zip(outs, (torch.float64, torch.int64, tdt)):
            if t is not None and not self._lof_on_device(t, want, count):
                raise ValueError(f"output tensors must be contiguous CUDA tensors of at least {count} values on the tree's "
                                 "device (sum float64, count int64, cutoff of the tree's element type)")
        if ht is None:
            ht = torch.full((1,), float(h), dtype=tdt, device=dev)
        s = outs[0] if outs[0] is not None else torch.empty(count, dtype=torch.float64, device=dev)
        cnt = outs[1] if outs[1] is not None else torch.empty(count, dtype=torch.int64, device=dev)
        cut = outs[2] if outs[2] is not None else torch.empty(count, dtype=tdt, device=dev)
        return KDE_KERNELS[kernel], ht, s, cnt, cut

    def kernel_density_device(self, queries, h, kernel: str = "gaussian", atol: float = 0.0, out_sum=None, out_count=None,
                              out_cutoff=None, stream=None):
        """The raw sums in HBM: ``queries`` a 2-D CUDA tensor of the tree's element type, ``h`` a scalar or a 1-D CUDA tensor
        of one bandwidth per query; returns CUDA tensors ``(sum float64 [nq], count int64 [nq], cutoff [nq])`` written in
        stream order on ``stream`` (default: the current torch stream).  The call waits for the device once (it reads
        the list offsets back to cut its pieces) and cannot be captured into a graph."""
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        if (not isinstance(queries, torch.Tensor) or queries.dtype != tdt or queries.dim() != 2 or not queries.is_cuda
                or queries.device.index != self.device):
            raise ValueError(f"queries must be a 2-D {tdt} CUDA tensor on the tree's device")
        if queries.shape[1] > 1 and queries.stride(1) != 1:
            queries = queries.contiguous()
        nq, qc = queries.shape
        kn, ht, s, cnt, cut = self._kde_device_args(h, kernel, atol, nq, (out_sum, out_count, out_cutoff))
        if nq:
            st = stream if stream is not None else torch.cuda.current_stream(queries.device).cuda_stream
            check(getattr(_lib.lib(), f"pn_kde_device_{self._sfx}")(
                self._h, queries.data_ptr(), nq, qc, queries.stride(0) if nq > 1 else max(qc, 1), ht.data_ptr(),
                ht.shape[0], kn, float(atol), 0, s.data_ptr(), cnt.data_ptr(), cut.data_ptr(), C.c_void_p(st)))
        return s, cnt, cut

    def kernel_density_self_device(self, h, kernel: str = "gaussian", atol: float = 0.0, include_self: bool = False,
                                   out_sum=None, out_count=None, out_cutoff=None, stream=None):
        """``kernel_density_device`` of the indexed rows themselves (``h``: a scalar or one bandwidth per row)."""
        import torch
        kn, ht, s, cnt, cut = self._kde_device_args(h, kernel, atol, self._n, (out_sum, out_count, out_cutoff))
        st = stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        check(getattr(_lib.lib(), f"pn_kde_self_device_{self._sfx}")(
            self._h, ht.data_ptr(), ht.shape[0], kn, float(atol), _lib.PN_SELF_INCLUDE if include_self else 0,
            s.data_ptr(), cnt.data_ptr(), cut.data_ptr(), C.c_void_p(st)))
        return s, cnt, cut

    def query_radius_count(self, queries, r):
        """The number of rows with distance < ``r`` (strict) per query: ``uint64 [nq]``; ``r`` a scalar or one radius per
        query.  Only the counting pass runs: no list is written (scikit-learn's ``query_radius(count_only=True)``)."""
        a = self._queries(queries, False)
        nq, qc = a.shape
        ra = self._radii(r, nq)
        if ra is None:  # (a radius that is not finite and positive is served as an array: empty lists, or every row)
            ok = float(r) > 0.0 and not math.isinf(float(r))
            ra = np.array([r], dtype=self.dtype) if ok else np.full(nq, r, dtype=self.dtype)
        cnt = np.zeros(nq, dtype=np.uint64)
        if nq:
            check(getattr(_lib.lib(), f"pn_kde_{self._sfx}")(self._h, a.ctypes.data, nq, qc, max(qc, 1), ra.ctypes.data,
                                                            ra.shape[0], _lib.PN_KDE_TOPHAT, 0.0, 0, None, cnt.ctypes.data,
                                                            None))
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
    def _km_check(self):
        from .distance import Cosine
        if isinstance(self.metric, Cosine):
            raise ValueError("k-means needs a Euclidean tree")

    def _km_centres(self, centres):
        c = self._queries(centres, False)
        if c.shape[0] and c.shape[1] != self._dim:
            raise ValueError(f"centres must have the tree's {self._dim} columns")
        return c

    def _km_centres_device(self, centres):
        import torch
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        if (not isinstance(centres, torch.Tensor) or centres.dim() != 2 or not self._lof_on_device(centres, tdt, 0)
                or (centres.shape[0] and centres.shape[1] != self._dim)):
            raise ValueError(f"centres must be a contiguous [nc][{self._dim}] {tdt} CUDA tensor on the tree's device")
        return tdt, torch.device("cuda", self.device)

    def kmeans_assign(self, centres):
        """The nearest centre of every indexed row by (distance, centre number), as ``mean_shift_labels`` gives it:
        ``(labels int64 [n], dist [n], inertia)`` with ``dist`` the distance to that centre and ``inertia`` the sum of
        the squared distances in the library's fixed shape (a float)."""
        self._km_check()
        c = self._km_centres(centres)
        labels = np.empty(self._n, dtype=np.int64)
        dist = np.empty(self._n, dtype=self.dtype)
        inertia = C.c_double(0.0)
        check(getattr(_lib.lib(), f"pn_kmeans_assign_{self._sfx}")(
            self._h, c.ctypes.data if c.shape[0] else None, c.shape[0], 0, labels.ctypes.data, dist.ctypes.data,
            C.byref(inertia)))
        return labels, dist, float(inertia.value)

    def kmeans_assign_device(self, centres, out_labels=None, out_dist=None, out_inertia=None, stream=None):
        """``kmeans_assign`` in HBM: ``centres`` a contiguous 2-D CUDA tensor; returns CUDA tensors ``(labels int64 [n],
        dist [n], inertia float64 [1])``.  Never waits."""
        import torch
        self._km_check()
        tdt, dev = self._km_centres_device(centres)
        nc = centres.shape[0]
        for t, want, name in ((out_labels, torch.int64, "out_labels"), (out_dist, tdt, "out_dist")):
            if t is not None and not self._lof_on_device(t, want, self._n):
                raise ValueError(f"{name} must be a contiguous {want} CUDA tensor of at least {self._n} values")
        if out_inertia is not None and not self._lof_on_device(out_inertia, torch.float64, 1):
            raise ValueError("out_inertia must be a float64 CUDA tensor of one value")
        labels = out_labels if out_labels is not None else torch.empty(self._n, dtype=torch.int64, device=dev)
        dist = out_dist if out_dist is not None else torch.empty(self._n, dtype=tdt, device=dev)
        inertia = out_inertia if out_inertia is not None else torch.zeros(1, dtype=torch.float64, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_kmeans_assign_device_{self._sfx}")(
            self._h, centres.data_ptr() if nc else None, nc, 0, labels.data_ptr(), dist.data_ptr(), inertia.data_ptr(),
            C.c_void_p(st)))
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
        self._km_check()
        k = int(k)
        if k < 1 or k > self._n:
            raise ValueError("k must be between 1 and the number of rows")
        if self.points is None:
            raise ValueError("kmeans_plusplus needs the rows on the host")
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
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
        self._km_check()
        abs_tol, max_iter = self._km_tol(tol, abs_tol, max_iter)
        if np.ndim(centres_or_k) == 0:
            init = self.kmeans_plusplus(int(centres_or_k), seed)
        else:
            init = self._km_centres(centres_or_k)
        k = init.shape[0]
        if k < 1:
            raise ValueError("k-means needs at least one centre")
        init = np.ascontiguousarray(init, dtype=self.dtype)
        centres = np.zeros((k, self._dim), dtype=self.dtype)
        labels = np.empty(self._n, dtype=np.int64)
        dist = np.empty(self._n, dtype=self.dtype)
        counts = np.zeros(k, dtype=np.uint64)
        inertia, shift2, iters = C.c_double(0.0), C.c_double(0.0), C.c_uint64(0)
        check(getattr(_lib.lib(), f"pn_kmeans_{self._sfx}")(
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
        self._km_check()
        tdt, dev = self._km_centres_device(centres)
        abs_tol, max_iter = self._km_tol(0.0, abs_tol, max_iter)
        k = centres.shape[0]
        if k < 1:
            raise ValueError("k-means needs at least one centre")
        out_c = torch.empty((k, self._dim), dtype=tdt, device=dev)
        labels = torch.empty(self._n, dtype=torch.int64, device=dev)
        dist = torch.empty(self._n, dtype=tdt, device=dev)
        counts = torch.zeros(k, dtype=torch.int64, device=dev)
        inertia = torch.zeros(1, dtype=torch.float64, device=dev)
        iters = torch.zeros(1, dtype=torch.int64, device=dev)
        shift2 = torch.zeros(1, dtype=torch.float64, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_kmeans_device_{self._sfx}")(
            self._h, centres.data_ptr(), k, abs_tol, max_iter, 0, out_c.data_ptr(), labels.data_ptr(), dist.data_ptr(),
            counts.data_ptr(), inertia.data_ptr(), iters.data_ptr(), shift2.data_ptr(), C.c_void_p(st)))
        return out_c, labels, dist, counts, inertia, iters, shift2

    def kmeans_bounds(self, centres):
        """Diagnostic: the k-means filter's lower bounds ``L[i][c] <= |x_i - c|^2`` (float64 ``[n][nc]``), f32 trees."""
        c = self._km_centres(centres)
        out = np.zeros((self._n, c.shape[0]), dtype=np.float64)
        check(_lib.lib().pn_kmeans_bounds_f32(self._h, c.ctypes.data if c.shape[0] else None, c.shape[0], out.ctypes.data))
        return out

    # -------------------------------------------------- mean shift
    # scikit-learn's ``MeanShift`` (flat kernel) on the device (``pn_mean_shift_*``): seeds climb to the modes of the tophat
    # density, every step the mean of a radius list summed by one wave in a fixed order; only the seeds still moving are
    # queried.  Then the converged modes are merged into centres and the rows labelled.  Every comparison is a strict '<'.
    def _ms_check(self):
        from .distance import Cosine
        if isinstance(self.metric, Cosine):
            raise ValueError("mean shift needs a Euclidean tree")

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
        self._ms_check()
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
        check(getattr(_lib.lib(), f"pn_mean_shift_{self._sfx}")(
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
        self._ms_check()
        tol, max_iter = self._ms_tol(h, tol, max_iter)
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
        if seeds is None:
            ns, flags, sp, stride = self._n, _lib.PN_MS_SEED_ROWS, None, 0
        else:
            if (not isinstance(seeds, torch.Tensor) or seeds.dtype != tdt or seeds.dim() != 2 or not seeds.is_cuda
                    or seeds.device.index != self.device):
                raise ValueError(f"seeds must be a 2-D {tdt} CUDA tensor on the tree's device")
            if seeds.shape[1] != self._dim:
                raise ValueError(f"seeds must have the tree's {self._dim} columns")
            if seeds.shape[1] > 1 and seeds.stride(1) != 1:
                seeds = seeds.contiguous()
            ns, flags, sp = seeds.shape[0], 0, seeds.data_ptr()
            stride = seeds.stride(0) if ns > 1 else self._dim
        ht = self._radii_device(h, ns, dev)
        if ht is None:
            ht = torch.full((1,), float(h), dtype=tdt, device=dev)
        modes = torch.zeros((ns, self._dim), dtype=tdt, device=dev)
        pw = torch.zeros(ns, dtype=torch.int64, device=dev)
        it = torch.zeros(ns, dtype=torch.int32, device=dev)
        sh = torch.zeros(ns, dtype=torch.float64, device=dev)
        work = np.zeros(2, dtype=np.uint64)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_mean_shift_device_{self._sfx}")(
            self._h, sp, 0 if seeds is None else ns, self._dim, stride, ht.data_ptr(), ht.shape[0], tol, max_iter, flags,
            modes.data_ptr(), pw.data_ptr(), it.data_ptr(), sh.data_ptr(), work.ctypes.data, C.c_void_p(st)))
        self.last_n_iter = int(work[0])
        return modes, pw, it, sh, (int(work[0]), int(work[1]))

    def mean_shift_merge(self, modes, points_within, h):
        """scikit-learn's merge of converged modes: ``(centres [nc][dim], centre_points uint64 [nc], centre_of_seed int64
        [ns])``.  Live modes are ranked by (``points_within`` descending, seed ascending); a mode is a centre iff no earlier
        centre lies within ``h``; ``centre_of_seed`` is the lowest-numbered centre within ``h``, -1 for a dead seed."""
        self._ms_check()
        m = self._queries(modes, False)
        if m.shape[1] != self._dim:
            raise ValueError(f"modes must have the tree's {self._dim} columns")
        ns = m.shape[0]
        pw = np.ascontiguousarray(points_within, dtype=np.uint64)
        if pw.shape != (ns,):
            raise ValueError("points_within must hold one count per mode")
        if np.ndim(h) != 0:
            raise ValueError("the merge takes one bandwidth")
        centres = np.zeros((ns, self._dim), dtype=self.dtype)
        cp = np.zeros(ns, dtype=np.uint64)
        cos = np.zeros(ns, dtype=np.int64)
        nc = C.c_uint64(0)
        check(getattr(_lib.lib(), f"pn_mean_shift_merge_{self._sfx}")(
            self._h, m.ctypes.data if ns else None, ns, pw.ctypes.data if ns else None, float(h), 0, centres.ctypes.data,
            cp.ctypes.data, cos.ctypes.data, C.byref(nc)))
        k = int(nc.value)
        return centres[:k].copy(), cp[:k].copy(), cos

    def mean_shift_merge_device(self, modes, points_within, h, stream=None):
        """``mean_shift_merge`` in HBM: CUDA tensors in, ``(centres [ns][dim], centre_points int64 [ns], centre_of_seed int64
        [ns], n_centres int64 [1])`` out -- the first ``n_centres`` rows of the first two are written.  Never waits."""
        import torch
        self._ms_check()
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
        if (not isinstance(modes, torch.Tensor) or modes.dtype != tdt or modes.dim() != 2 or modes.shape[1] != self._dim
                or not self._lof_on_device(modes, tdt, 0)):
            raise ValueError(f"modes must be a contiguous [ns][{self._dim}] {tdt} CUDA tensor on the tree's device")
        ns = modes.shape[0]
        if not self._lof_on_device(points_within, torch.int64, ns) or points_within.numel() != ns:
            raise ValueError("points_within must be a contiguous int64 CUDA tensor of one count per mode")
        if np.ndim(h) != 0:
            raise ValueError("the merge takes one bandwidth")
        centres = torch.zeros((ns, self._dim), dtype=tdt, device=dev)
        cp = torch.zeros(ns, dtype=torch.int64, device=dev)
        cos = torch.zeros(ns, dtype=torch.int64, device=dev)
        nc = torch.zeros(1, dtype=torch.int64, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_mean_shift_merge_device_{self._sfx}")(
            self._h, modes.data_ptr() if ns else None, ns, points_within.data_ptr() if ns else None, float(h), 0,
            centres.data_ptr(), cp.data_ptr(), cos.data_ptr(), nc.data_ptr(), C.c_void_p(st)))
        return centres, cp, cos, nc

    def mean_shift_labels(self, centres, h, cluster_all: bool = True):
        """The nearest centre of every indexed row by (distance, centre number): ``int64 [n]``; with
        ``cluster_all=False`` a row whose nearest centre is not within ``h`` gets -1."""
        self._ms_check()
        c = self._queries(centres, False)
        if c.shape[0] and c.shape[1] != self._dim:
            raise ValueError(f"centres must have the tree's {self._dim} columns")
        if np.ndim(h) != 0:
            raise ValueError("the labels take one bandwidth")
        labels = np.empty(self._n, dtype=np.int64)
        check(getattr(_lib.lib(), f"pn_mean_shift_labels_{self._sfx}")(
            self._h, c.ctypes.data if c.shape[0] else None, c.shape[0], float(h), 0 if cluster_all else _lib.PN_MS_ORPHANS,
            labels.ctypes.data))
        return labels

    def mean_shift_labels_device(self, centres, h, cluster_all: bool = True, n_centres=None, out_labels=None, stream=None):
        """``mean_shift_labels`` in HBM: ``centres`` a contiguous 2-D CUDA tensor, of which the first ``n_centres`` rows
        (default: all) are the centres; returns the labels, a CUDA int64 tensor.  Never waits."""
        import torch
        self._ms_check()
        tdt = torch.float32 if self._sfx == "f32" else torch.float64
        dev = torch.device("cuda", self.device)
        if (not isinstance(centres, torch.Tensor) or centres.dim() != 2 or not self._lof_on_device(centres, tdt, 0)
                or (centres.shape[0] and centres.shape[1] != self._dim)):
            raise ValueError(f"centres must be a contiguous [nc][{self._dim}] {tdt} CUDA tensor on the tree's device")
        nc = centres.shape[0] if n_centres is None else int(n_centres)
        if nc < 0 or nc > centres.shape[0]:
            raise ValueError("n_centres exceeds the rows of centres")
        if np.ndim(h) != 0:
            raise ValueError("the labels take one bandwidth")
        if out_labels is not None and not self._lof_on_device(out_labels, torch.int64, self._n):
            raise ValueError(f"out_labels must be a contiguous int64 CUDA tensor of at least {self._n} values")
        labels = out_labels if out_labels is not None else torch.empty(self._n, dtype=torch.int64, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(getattr(_lib.lib(), f"pn_mean_shift_labels_device_{self._sfx}")(
            self._h, centres.data_ptr() if nc else None, nc, float(h), 0 if cluster_all else _lib.PN_MS_ORPHANS,
            labels.data_ptr(), C.c_void_p(st)))
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
