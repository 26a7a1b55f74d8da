"""The one argument layer between the Python mirror and the C ABI (``include/petal_mi355x.h``).

``Handle`` is the base of ``BallTree`` and ``ShardedIndex``.  It owns what every entry point needs -- the element type,
the symbol lookup, the stream, output tensors, device-resident queries, the library-allocated CSR lists, per-row host
inputs -- and the searches the two handles share.  A method on it validates what is specific to it, builds its outputs,
makes one library call and returns; a new entry point is a method on this layer, not a copy of another one.

Everything here works from the attributes a handle carries anyway (``_h``, ``_sfx``, ``dtype``, ``device`` and the row
counts); the only thing it adds to an instance is the lazily filled table of looked-up functions.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .errors import check

ENGINES = {"auto": _lib.PN_ENGINE_AUTO, "exact": _lib.PN_ENGINE_EXACT, "mfma": _lib.PN_ENGINE_MFMA,
           "bf16": _lib.PN_ENGINE_BF16}


NP = {"f32": np.float32, "f64": np.float64}  # suffix -> NumPy's element type (ctypes': ``_lib.REAL``)


def suffix(dtype) -> str:
    """the symbol suffix of a float32 / float64 ``np.dtype`` or ``torch.dtype``: the one place that tells the two apart"""
    return "f32" if dtype.itemsize == 4 else "f64"


def stream_arg(stream, dev):
    """``stream``, or torch's current stream on ``dev``, as the ``void *`` the library takes"""
    import torch
    return C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)


class Handle:
    _prefix = "pn_"        # of the searches: pn_<stem>_<sfx> (ShardedIndex: pn_sharded_<stem>_<sfx>)
    _object = "pn_index_"  # of destroy / set_option / get_stats

    # the subclass names its row counts: ``_total`` rows are indexed, ``_rows`` of them answer a self-query here
    # ------------------------------------------------------------ element type
    @property
    def _real(self):
        """the ctypes scalar of the element type: ``self._real(v)`` is the ``float`` / ``double`` argument"""
        return _lib.REAL[self._sfx]

    @property
    def _tdt(self):
        import torch
        return getattr(torch, self.dtype.name)

    @property
    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    def _fn(self, stem):
        """the library function ``pn_<stem>_<sfx>``, looked up once per handle (the one-point-per-call path is host-bound)"""
        fns = self.__dict__.setdefault("_fns", {})
        fn = fns.get(stem)
        if fn is None:
            fn = fns[stem] = getattr(_lib.lib(), f"{self._prefix}{stem}_{self._sfx}")
        return fn

    # ------------------------------------------------------------ outputs
    def _on_device(self, t, dtype, need, dev=None):
        """The one rule for a tensor the library reads or writes through its ``data_ptr()``: a contiguous CUDA tensor of
        ``dtype`` on the handle's device (``dev``: the queries') with at least ``need`` elements."""
        import torch
        return (isinstance(t, torch.Tensor) and t.is_cuda and t.device == (dev if dev is not None else self._dev)
                and t.dtype == dtype and t.is_contiguous() and t.numel() >= need)

    def _out(self, t, shape, dtype, need, zero=False, dev=None):
        """The output tensor of one library call, which writes ``need`` elements of ``dtype``: the caller's ``t`` where it
        passes ``_on_device``, or a fresh tensor of ``shape`` there."""
        import torch
        if t is None:
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=dev if dev is not None else self._dev)
        if not self._on_device(t, dtype, need, dev):
            raise ValueError(f"an output tensor must be a contiguous {dtype} CUDA tensor of at least {need} values on the "
                             "device of the call")
        return t

    def _outs(self, *specs, dev=None):
        """``_out`` for every ``(t, shape, dtype, need[, zero])`` of one call; every given tensor is checked before a
        fresh one is made, so a bad argument never costs an allocation"""
        for t, _, dtype, need, *_ in specs:
            if t is not None:
                self._out(t, None, dtype, need, dev=dev)
        return [self._out(*spec, dev=dev) for spec in specs]

    def _csr_outs(self, count, capacity, out_offsets, out_idx, out_dist, out_total, with_distance, dev=None):
        """the four outputs of a device radius search over ``count`` lists: ``(offsets, idx, dist or None, total)``"""
        import torch
        cap, need = max(int(capacity), 1), int(capacity)
        specs = [(out_offsets, count + 1, torch.int64, count + 1), (out_idx, cap, torch.int64, need),
                 (out_total, 1, torch.int64, 1)]
        if with_distance:
            specs.append((out_dist, cap, self._tdt, need))
        outs = self._outs(*specs, dev=dev)
        return outs[0], outs[1], outs[3] if with_distance else None, outs[2]

    # ------------------------------------------------------------ inputs
    def _queries(self, q, one: bool):
        a = np.ascontiguousarray(q, dtype=self.dtype)
        if one:
            if a.ndim != 1:
                raise ValueError("point must be 1-D (Ix1)")
            a = a.reshape(1, -1)
        elif a.ndim != 2:
            raise ValueError("queries must be 2-D")
        return a

    def _device_queries(self, q, what="queries", on_device=False, contiguous=False, null_empty=True):
        """Device-resident queries / centres / seeds: ``(q, nq, qc, pointer, leading stride)``.  ``q`` is a 2-D CUDA
        tensor of the element type (``on_device``: on the handle's GPU) whose inner stride is made 1 -- or, with
        ``contiguous``, must be contiguous already.  ``null_empty``: an empty matrix is handed over as NULL."""
        import torch
        if (not isinstance(q, torch.Tensor) or q.dtype != self._tdt or q.dim() != 2 or not q.is_cuda
                or (on_device and q.device.index != self.device) or (contiguous and not q.is_contiguous())):
            raise ValueError(f"{what} must be a {'contiguous ' if contiguous else ''}2-D {self._tdt} CUDA tensor"
                             + (" on the handle's device" if on_device else ""))
        if q.shape[1] > 1 and q.stride(1) != 1:
            q = q.contiguous()
        nq, qc = q.shape
        return q, nq, qc, q.data_ptr() if nq * qc or not null_empty else None, q.stride(0) if nq > 1 else max(qc, 1)

    def _per_row(self, a, dtype, message, count=None):
        """``a`` as a contiguous 1-D array of ``dtype`` with one value per indexed row (or ``count``)"""
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.ndim != 1 or a.shape[0] != (self._total if count is None else count):
            raise ValueError(message)
        return a

    def _per_row_device(self, t, dtype, message, count=None):
        """``t`` passes ``_on_device`` and is 1-D with one value per indexed row (or ``count``)"""
        n = self._total if count is None else count
        if not self._on_device(t, dtype, n) or t.dim() != 1 or t.numel() != n:
            raise ValueError(message)
        return t

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
        if not isinstance(r, torch.Tensor) or not r.is_cuda or r.dtype != self._tdt:
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

    # ------------------------------------------------------------ host CSR results
    def _csr(self, status, offsets, out_i, out_d, with_distance):
        """``(idx, dist or None)``: copies of the CSR lists the library allocated for a call that returned ``status``,
        which are freed here whatever happens (``out_d`` may be None where the call has no distance list)."""
        try:
            check(status)
            total = int(offsets[-1])
            idx = np.empty(0, dtype=np.uint64)
            dist = np.empty(0, dtype=self.dtype) if with_distance else None
            if total:
                idx = np.frombuffer((C.c_uint64 * total).from_address(out_i.value), dtype=np.uint64).copy()
                if with_distance:
                    dist = np.frombuffer((self._real * total).from_address(out_d.value), dtype=self.dtype).copy()
        finally:
            if out_i.value:
                _lib.lib().pn_free(out_i)
            if out_d is not None and out_d.value:
                _lib.lib().pn_free(out_d)
        return idx, dist

    # ------------------------------------------------------------ lifetime, options
    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            getattr(_lib.lib(), self._object + "destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def set_option(self, opt: int, value: int):
        check(getattr(_lib.lib(), self._object + "set_option")(self._h, opt, int(value)))
        return self

    def set_engine(self, name: str):
        return self.set_option(_lib.PN_OPT_ENGINE, ENGINES[name])

    def stats(self, reset: bool = False):
        s = _lib.PnStats()
        check(getattr(_lib.lib(), self._object + "get_stats")(self._h, C.byref(s), int(reset)))
        return {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}

    # ------------------------------------------------------------------ queries
    def query_batch(self, queries, k: int):
        """k-NN for every row of ``queries``: (nq, min(k, n)) indices (uint64) and distances."""
        return self._knn(self._queries(queries, False), k)

    def _knn(self, a, k):
        """``query_batch`` of checked queries (``_queries``)"""
        nq, qc = a.shape
        kout = min(int(k), self._total)
        idx = np.empty((nq, kout), dtype=np.uint64)
        dist = np.empty((nq, kout), dtype=self.dtype)
        if nq and kout:
            check(self._fn("query")(self._h, a.ctypes.data, nq, qc, max(qc, 1), int(k), idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def _query_radii(self, a, radii, with_distance, sort):
        nq, qc = a.shape
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        out_i, out_d = C.c_void_p(0), C.c_void_p(0)
        status = self._fn("query_radii")(
            self._h, a.ctypes.data, nq, qc, max(qc, 1), radii.ctypes.data if nq else None,
            _lib.PN_RADIUS_SORTED if sort else 0, offsets.ctypes.data, C.byref(out_i),
            C.byref(out_d) if with_distance else None)
        return (offsets,) + self._csr(status, offsets, out_i, out_d, with_distance)

    def query_radius_batch(self, queries, distance):
        """CSR (offsets[nq+1], indices) of ``{ i : dist(q, p_i) < distance }``, ascending per query.  ``distance``: a
        scalar, or a 1-D array of nq radii -- list q is then the scalar call's for query q with ``distance[q]``."""
        return self._radius(self._queries(queries, False), distance)

    def _radius(self, a, distance):
        """``query_radius_batch`` of checked queries (``_queries``)"""
        nq, qc = a.shape
        radii = self._radii(distance, nq)
        if radii is not None:
            return self._query_radii(a, radii, False, False)[:2]
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        out = C.c_void_p(0)
        status = self._fn("query_radius")(self._h, a.ctypes.data, nq, qc, max(qc, 1), _lib.REAL[self._sfx](distance),
                                          offsets.ctypes.data, C.byref(out))  # (REAL[...]: ``_real`` without the call)
        return offsets, self._csr(status, offsets, out, None, False)[0]

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
        status = self._fn("query_radius_with_distance")(
            self._h, a.ctypes.data, nq, qc, max(qc, 1), self._real(distance), _lib.PN_RADIUS_SORTED if sort else 0,
            offsets.ctypes.data, C.byref(out_i), C.byref(out_d))
        return (offsets,) + self._csr(status, offsets, out_i, out_d, True)

    # --------------------------------------------------------- device-resident
    def query_device(self, queries, k: int, out_idx=None, out_dist=None, stream=None):
        """k-NN with queries and results in HBM (torch CUDA tensors of the handle's element type; indices as int64),
        enqueued on ``stream`` (default: the current torch stream)."""
        import torch
        q, nq, qc, ptr, ld = self._device_queries(queries, null_empty=False)
        kout = min(int(k), self._total)
        out_idx, out_dist = self._outs((out_idx, (nq, kout), torch.int64, nq * kout),
                                       (out_dist, (nq, kout), self._tdt, nq * kout), dev=q.device)
        if nq and kout:
            check(self._fn("query_device")(self._h, ptr, nq, qc, ld, int(k), out_idx.data_ptr(), out_dist.data_ptr(),
                                           stream_arg(stream, q.device)))
        return out_idx, out_dist

    def query_radius_device(self, queries, distance, capacity: int, out_offsets=None, out_idx=None, out_total=None,
                            stream=None):
        """``query_radius`` with queries and results in HBM, nothing read back (``pn_query_radius_device_*``).

        Returns CUDA tensors ``(offsets int64 [nq+1], idx int64 [capacity], total int64 [1])``: the CSR offsets are always
        complete; rows are written where their position is below ``capacity``; ``total > capacity`` (whenever the caller
        looks) means the buffer was too small -- call again with ``capacity >= total``."""
        q, nq, qc, ptr, ld = self._device_queries(queries)
        offs, idx, _, tot = self._csr_outs(nq, capacity, out_offsets, out_idx, None, out_total, False, q.device)
        radii = self._radii_device(distance, nq, q.device)
        if radii is not None:  # one radius per query
            check(self._fn("query_radii_device")(
                self._h, ptr, nq, qc, ld, radii.data_ptr() if nq else None, 0, offs.data_ptr(), idx.data_ptr(), None,
                int(capacity), tot.data_ptr(), stream_arg(stream, q.device)))
        else:
            check(self._fn("query_radius_device")(
                self._h, ptr, nq, qc, ld, self._real(distance), offs.data_ptr(), idx.data_ptr(), int(capacity),
                tot.data_ptr(), stream_arg(stream, q.device)))
        return offs, idx, tot

    def query_radius_with_distance_device(self, queries, distance, capacity: int, sort: bool = False, out_offsets=None,
                                          out_idx=None, out_dist=None, out_total=None, stream=None):
        """``query_radius_device`` plus each neighbour's distance (``pn_query_radius_with_distance_device_*``):
        ``(offsets int64 [nq+1], idx int64 [capacity], dist [capacity], total int64 [1])`` as CUDA tensors.  With
        ``sort=True`` every list lying wholly below ``capacity`` is ordered by (distance, index); a list straddling the
        capacity is left unsorted."""
        q, nq, qc, ptr, ld = self._device_queries(queries)
        if int(capacity) < 0:
            raise ValueError("capacity must be >= 0")
        offs, idx, dist, tot = self._csr_outs(nq, capacity, out_offsets, out_idx, out_dist, out_total, True, q.device)
        flags = _lib.PN_RADIUS_SORTED if sort else 0
        radii = self._radii_device(distance, nq, q.device)
        if radii is not None:  # one radius per query
            fn, r = self._fn("query_radii_device"), radii.data_ptr() if nq else None
        else:
            fn, r = self._fn("query_radius_with_distance_device"), self._real(distance)
        check(fn(self._h, ptr, nq, qc, ld, r, flags, offs.data_ptr(), idx.data_ptr(), dist.data_ptr(), int(capacity),
                 tot.data_ptr(), stream_arg(stream, q.device)))
        return offs, idx, dist, tot

    # ------------------------------------------------------------- self-queries
    # Every indexed row against its own index, the row itself left out (``pn_query_self_*`` / ``pn_query_radius_self_*``):
    # the rows already in HBM are the queries -- nothing is sent up again.  A sharded handle answers for its LOCAL rows
    # (rows local_first_row .. local_first_row + local_rows) with global row numbers; in rank mode every rank calls them
    # with the same arguments.
    def _self_flags(self, include_self, sort=False):
        return (_lib.PN_SELF_INCLUDE if include_self else 0) | (_lib.PN_RADIUS_SORTED if sort else 0)

    def _self_k(self, k, include_self):
        if int(k) < 0:
            raise ValueError("k must be >= 0")
        return min(int(k), self._total if include_self else self._total - 1)

    def query_self(self, k: int, include_self: bool = False):
        """The k nearest OTHER rows of every indexed row: ``(idx uint64 [n, kout], dist [n, kout])``, kout = min(k, n - 1),
        each row's list ordered by (distance, index).  ``include_self=True``: the row stays in its own list, kout =
        min(k, n) -- ``query_batch(rows, k)``."""
        kout = self._self_k(k, include_self)
        idx = np.empty((self._rows, kout), dtype=np.uint64)
        dist = np.empty((self._rows, kout), dtype=self.dtype)
        if kout:  # (a rank without rows still takes part: NumPy's empty arrays keep a non-NULL buffer)
            check(self._fn("query_self")(self._h, int(k), self._self_flags(include_self), idx.ctypes.data,
                                         dist.ctypes.data))
        return idx, dist

    def query_self_device(self, k: int, include_self: bool = False, out_idx=None, out_dist=None, stream=None):
        """``query_self`` with the results in HBM: CUDA tensors ``(idx int64 [n, kout], dist [n, kout])``, enqueued on
        ``stream`` (default: the current torch stream)."""
        import torch
        dev, rows = self._dev, self._rows
        kout = self._self_k(k, include_self)
        out_idx, out_dist = self._outs((out_idx, (rows, kout), torch.int64, rows * kout),
                                       (out_dist, (rows, kout), self._tdt, rows * kout))
        if kout:
            # (placeholders a sharded rank without rows hands in: nothing is written to them)
            wi = out_idx if rows else torch.empty(1, dtype=torch.int64, device=dev)
            wd = out_dist if rows else torch.empty(1, dtype=self._tdt, device=dev)
            check(self._fn("query_self_device")(self._h, int(k), self._self_flags(include_self), wi.data_ptr(),
                                                wd.data_ptr(), stream_arg(stream, dev)))
        return out_idx, out_dist

    def query_radius_self(self, r, with_distance: bool = False, sort: bool = False, include_self: bool = False):
        """``{ j != i : distance(p_i, p_j) < r }`` for every indexed row i, as CSR: ``(offsets uint64 [n+1], idx uint64,
        dist or None)``; lists ascending by index, or by (distance, index) with ``sort=True`` (needs ``with_distance``).
        ``include_self=True`` keeps row i wherever its distance to itself is below r.  ``r``: a scalar, or a 1-D array of
        n radii, row i's own (``pn_query_radii_self_*``)."""
        if sort and not with_distance:
            raise ValueError("sort=True needs with_distance=True")
        radii = self._radii(r, self._rows)
        offsets = np.zeros(self._rows + 1, dtype=np.uint64)
        out_i, out_d = C.c_void_p(0), C.c_void_p(0)
        if radii is not None:
            fn, rr = self._fn("query_radii_self"), radii.ctypes.data
        else:
            fn, rr = self._fn("query_radius_self"), self._real(r)
        status = fn(self._h, rr, self._self_flags(include_self, sort), offsets.ctypes.data, C.byref(out_i),
                    C.byref(out_d) if with_distance else None)
        return (offsets,) + self._csr(status, offsets, out_i, out_d, with_distance)

    def query_radius_self_device(self, r, capacity: int, with_distance: bool = False, sort: bool = False,
                                 include_self: bool = False, out_offsets=None, out_idx=None, out_dist=None, out_total=None,
                                 stream=None):
        """``query_radius_self`` in HBM with the capacity contract of ``query_radius_with_distance_device``: CUDA tensors
        ``(offsets int64 [n+1], idx int64 [capacity], dist [capacity] or None, total int64 [1])``.  ``r``: a scalar, or a
        1-D CUDA tensor of n radii of the tree's element type."""
        if int(capacity) < 0:
            raise ValueError("capacity must be >= 0")
        if sort and not with_distance:
            raise ValueError("sort=True needs with_distance=True")
        dev = self._dev
        radii = self._radii_device(r, self._rows, dev)
        offs, idx, dist, tot = self._csr_outs(self._rows, capacity, out_offsets, out_idx, out_dist, out_total, with_distance)
        if radii is not None:
            fn, rr = self._fn("query_radii_self_device"), radii.data_ptr()
        else:
            fn, rr = self._fn("query_radius_self_device"), self._real(r)
        check(fn(self._h, rr, self._self_flags(include_self, sort), offs.data_ptr(), idx.data_ptr(),
                 dist.data_ptr() if dist is not None else None, int(capacity), tot.data_ptr(), stream_arg(stream, dev)))
        return offs, idx, dist, tot
