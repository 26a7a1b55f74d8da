"""Every graph entry point on ONE handle against ONE dense want side, twice over: run by tests/test_gpu_graph_shapes.py
(the fixed grid of shapes where the code underneath changes) and tests/test_gpu_fuzz.py (random draws), or by hand:
python tests/fuzz_graph.py [n_cases] [seed].

The want side of a case is the dense distance matrix in the index's element type (oracle.pairwise / pairwise_cosine: the
oracle's scalar distance per pair, checked again on sampled pairs) and nothing else: the k-NN lists are its rows ordered by
(key, index), the radius lists its entries strictly below the radius, and cores, Prim's tree, the dendrogram, HDBSCAN, DBSCAN
and OPTICS come out of it through the references of the other modules, imported, not restated.  LOF is the reference over
the library's own query_self, which the same call first anchors to the matrix.  The KDE sums and the mean shift step are
tests/density_reference.py over the matrix' lists: the entries strictly below each query's cutoff, the rows with a NaN in
no list (and dead seeds); the mean shift labels are the matrix' columns of the centres, by (key, centre number), and so are
the labels and distances of a k-means assignment; its inertia and the k-means loop are tests/kmeans_reference.py.

The got side calls query_self, query_radius_self (scalar and per-row radii), dbscan, mst (plain and cored), linkage,
hdbscan, lof + lof_score, optics and optics_dbscan on one handle, host or device entry drawn at random, the device outputs
on a stream of their own; and, borrowing the same workspace scratch, kde_self (the rows as their own queries: a kernel,
include_self and a scalar bandwidth or one per row drawn per round, from eps), kde (a subset of the rows and one NaN query
as external queries; on a Cosine tree the normalised density must raise, the raw sums are checked all the same),
mean_shift (one step of the rows as seeds, then the labels against centres picked from the rows; on a Cosine tree the call
must raise) and kmeans (an assignment to 1, 2, 7, 33 or 70 of the rows as centres, then two iterations of the loop from the
same centres; on a Cosine tree all four entries must raise).  The compact kernels, mean shift and k-means compare bit
for bit; the smooth kernels take atol = 0 up to 1000 rows (every row in every list) and atol = 1 above, where the returned cutoff is held against the header's and the sums against
the bound of tests/test_gpu_kde.py.  Pass 1 uses the case's parameters in a random order.  Pass 2 draws an engine, an index
base, the DBSCAN / OPTICS / KDE / mean shift pieces, the MST batch and PN_OPT_KMEANS_FILTER, then runs everything in
another order with larger k / min_samples and eps halved, then with smaller ones -- so every shared workspace buffer is regrown and reused by another
owner in between -- and finally repeats calls with pass 1's parameters: those must reproduce pass 1 byte for byte.  All
other comparisons are array equality; floats by their bits with equal NaN masks.  Whatever the KDE and mean shift entries
draw -- kernels, flags, host or device entry, their places in the order, their pieces -- comes from a generator of the
case's own, and whatever the k-means entry draws -- its centres, host or device entry, its place in the order, the filter
option -- from another, so the draws of the graph entries do not depend on the entries beside them, nor those of the KDE and
mean shift entries on k-means.

Conditions (asserted on the want side before any device call, printed, never tolerances): HDBSCAN's least relative gap
>= MIN_GAP; OPTICS has a row with infinite core distance and a finite reachability; DBSCAN has two clusters and a noise
row.  They are demanded of the families built from blobs with a background at n >= 1000 (every row of the fixed grid);
uniform rows, the lattice and tiny n cannot meet them by construction and keep the modules' expectations instead (the
want side decides: all noise, empty outputs at n = 1).  A case that misses a condition redraws its data seed, at most
twice; the count is returned for the callers to bound.
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
import kmeans_reference  # noqa: E402
import petal_neighbors_amd as pn  # noqa: E402
from petal_neighbors_amd import _lib  # noqa: E402
from density_reference import kde_sums, ms_step  # noqa: E402
from optics_reference import cpu_extract, cpu_optics, csr_from_dense, same_partition  # noqa: E402
from test_gpu_dbscan import cpu_dbscan  # noqa: E402
from test_gpu_hdbscan import MIN_GAP, ref_hdbscan  # noqa: E402
from test_gpu_kde import COMPACT, SMOOTH, cutoff_within_bounds, smooth_bound, smooth_cutoff  # noqa: E402
from test_gpu_linkage import seq_linkage  # noqa: E402
from test_gpu_lof import ref_fit, ref_score, same_bits  # noqa: E402
from test_gpu_mst import (bits_of_keys, core_keys_from, keys_of, prim, sampled_pairs_match_the_oracle,  # noqa: E402
                          weight_keys)

KMAX = 64  # the longest k-NN list a case asks for
BLOB_FAMILIES = ("blobs", "dups", "sorted", "dups_nan")
GRAPH_ENTRIES = ("self", "radius", "radii", "dbscan", "mst", "mst_cored", "linkage", "hdbscan", "lof", "optics", "extract")
DENSITY_ENTRIES = ("kde", "kde_self", "mean_shift")
KMEANS_ENTRIES = ("kmeans",)
ENTRIES = GRAPH_ENTRIES + DENSITY_ENTRIES + KMEANS_ENTRIES
KDE_QUERIES = 192  # rows a case takes as external KDE queries, at most (one NaN query is added)
KDE_ATOL = 1.0     # the smooth kernels' atol above 1000 rows (at most: atol = 0, every row in every list)
MS_CENTRES = 7     # rows a case takes as centres for the labels, at most
KM_CENTRES = (1, 2, 7, 33, 70)  # rows a round takes as k-means centres: one of these, at most n
KM_ITERATIONS = 2


# ------------------------------------------------------------------------------------------------------------ data
def make_rows(p, seed):
    n, dim, family = p["n"], p["dim"], p["family"]
    rng = np.random.default_rng(seed)
    if family == "uniform":
        x = rng.random((n, dim))
    elif family == "lattice":  # integer coordinates, about four rows per occupied point in few dimensions: nothing but ties
        side = max(int(np.ceil((n / 4.0) ** (1.0 / dim))), 3)
        x = rng.integers(0, side, (n, dim)).astype(np.float64)
    else:  # Gaussian blobs around nb centres in [0, 1)^dim and a uniform background, rows permuted
        nb, sigma, background = p.get("nb", 8), p.get("sigma", 0.05), p.get("background", 0.1)
        centres = rng.random((nb, dim))
        n_bg = int(round(n * background))
        which = rng.integers(0, nb, n - n_bg)
        x = np.concatenate([centres[which] + sigma * rng.standard_normal((n - n_bg, dim)), rng.random((n_bg, dim))])
        x = x[rng.permutation(n)]
    if p["cosine"]:
        x = x - 0.5  # centred: all angles occur
    x = x.astype(p["dtype"])
    if family == "dups" and n >= 4:
        src = rng.integers(0, n, max(n // 10, 1))
        x[rng.integers(0, n, len(src))] = x[src]
    elif family == "dups_nan":  # 30 copies of one row, two rows with NaN
        x[100:130] = x[5]
        x[n // 2, 1] = np.nan
        x[n - 7] = np.nan
    elif family == "sorted":
        x = x[np.argsort(x[:, 0], kind="stable")]
    return np.ascontiguousarray(x)


# ------------------------------------------------------------------------------------------------------- want side
class Want:
    def __init__(self, x, cosine):
        self.x, self.n, self.cosine, self.dt = x, len(x), cosine, x.dtype
        self.d = oracle.pairwise_cosine(x) if cosine else oracle.pairwise(x)
        if cosine:  # (the matrix' diagonal is a literal 0: a row's distance to itself is the scalar function's)
            for i in range(self.n):
                self.d[i, i] = oracle.cosine(x[i], x[i])
        else:
            self.d[np.arange(self.n), np.arange(self.n)] = np.where(np.isnan(x).any(axis=1), np.nan, 0).astype(self.dt)
        sampled_pairs_match_the_oracle(oracle, x, self.d, 1, oracle.cosine if cosine else oracle.euclidean)
        self.dk = keys_of(self.d, cosine)
        kk = min(KMAX, self.n)
        off_diag = self.dk.copy()
        np.fill_diagonal(off_diag, np.iinfo(self.dk.dtype).max)
        self.order = {False: np.argsort(off_diag, axis=1, kind="stable")[:, :min(kk, self.n - 1)],  # by (key, index)
                      True: np.argsort(self.dk, axis=1, kind="stable")[:, :kk]}
        del off_diag
        self.cache = {}

    def memo(self, key, fn):
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]

    def knn(self, k, include):
        idx = self.order[include][:, :k]
        return idx, np.take_along_axis(self.d, idx, axis=1)

    def lists(self, r, include, sort):
        """CSR (offsets, idx, dist) of { j : d[i, j] < r_i }, ascending j or by (key, j)"""
        r = np.asarray(r, dtype=self.dt)
        with np.errstate(invalid="ignore"):
            m = self.d < (r[:, None] if r.ndim else r)
        if not include:
            m[np.arange(self.n), np.arange(self.n)] = False
        rows, cols = np.nonzero(m)
        if sort:
            o = np.lexsort((cols, self.dk[rows, cols], rows))
            rows, cols = rows[o], cols[o]
        off = np.zeros(self.n + 1, dtype=np.int64)
        off[1:] = np.cumsum(m.sum(axis=1))
        return off, cols.astype(np.int64), self.d[rows, cols]

    def lists_of(self, sel, r):
        """CSR (offsets, dist) of { j : d[sel_q, j] < r_q }, ascending j: the rows ``sel`` as external queries"""
        r = np.asarray(r, dtype=self.dt)
        d = self.d[sel]
        with np.errstate(invalid="ignore"):
            m = d < (r[:, None] if r.ndim else r)
        off = np.zeros(len(sel) + 1, dtype=np.int64)
        off[1:] = np.cumsum(m.sum(axis=1))
        return off, d[m]

    def core_keys(self, k):
        return self.memo(("ck", k), lambda: core_keys_from(self.dk, k))

    def cores(self, k):
        return bits_of_keys(self.core_keys(k), self.cosine).view(self.dt)

    def mst(self, k):
        """(lo, hi, key) of the tree; k None: plain"""
        return self.memo(("mst", k), lambda: prim(weight_keys(self.dk, None if k is None else self.core_keys(k))))

    def weights(self, key):
        return bits_of_keys(key, self.cosine).view(self.dt)

    def hdbscan(self, m, k):
        lo, hi, key = self.mst(k)
        return self.memo(("hdb", m, k), lambda: ref_hdbscan(self.n, lo, hi, self.weights(key), m, self.dt))

    def dbscan(self, eps, ms):
        def run():
            off, idx, _ = self.lists(eps, True, False)
            return cpu_dbscan(off, idx, ms)
        return self.memo(("db", float(eps), ms), run)

    def optics(self, ms, max_eps):
        return self.memo(("opt", ms, float(max_eps)), lambda: cpu_optics(*csr_from_dense(self.d, max_eps), ms))


def derive(p, w):
    """the parameters a case leaves open, from the want side: eps at the median distance to the 25th nearest other row,
    max_eps at the 50th"""
    n = w.n
    q = dict(p)
    q.setdefault("k", 10)
    q.setdefault("ms", 6)
    q.setdefault("m", 10)
    for name in ("k", "ms"):
        q[name] = max(min(q[name], n - 1, KMAX // 2 - 2), 1)
    near = w.knn(KMAX, False)[1]
    with np.errstate(all="ignore"):
        def col(c):
            if near.shape[1] == 0:
                return w.dt.type(1)
            v = np.nanmedian(near[:, min(c, near.shape[1] - 1)].astype(np.float64))
            return w.dt.type(v if np.isfinite(v) and v > 0 else 1)
        q.setdefault("eps", col(24))
        q.setdefault("max_eps", col(49))
    q["eps"], q["max_eps"] = w.dt.type(q["eps"]), w.dt.type(q["max_eps"])
    return q


def conditions(q, w):
    """(all hold, text)"""
    n = w.n
    if n < 2:
        return True, "n = 1: nothing to demand"
    h = w.hdbscan(q["m"], q["k"])
    o = w.optics(q["ms"], q["max_eps"])
    d = w.dbscan(q["eps"], q["ms"])
    per_list = float(w.lists(q["eps"], False, False)[0][-1]) / n
    gap = h[3]["gap"]
    n_inf_core, n_fin_reach = int(np.count_nonzero(np.isinf(o[3]))), int(np.count_nonzero(np.isfinite(o[1])))
    n_noise = int(np.count_nonzero(d[0] < 0))
    text = (f"eps {q['eps']:.6g} ({per_list:.1f} per list), max_eps {q['max_eps']:.6g}; hdbscan {h[2]} clusters, least gap "
            f"{gap:.3g}; optics {n_inf_core} infinite cores, {n_fin_reach} finite reachabilities; dbscan {d[2]} clusters, "
            f"{n_noise} noise rows")
    ok = gap >= MIN_GAP and n_inf_core >= 1 and n_fin_reach >= 1 and d[2] >= 2 and n_noise >= 1
    return ok, text


# -------------------------------------------------------------------------------------------------------- got side
def eq_bits(got, want, what):
    same_bits(np.ascontiguousarray(got), np.ascontiguousarray(want), what)


def eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), \
        f"{what}: {int(np.count_nonzero(got.astype(np.int64) != want.astype(np.int64))) if got.shape == want.shape else 'shape'} differ"


class Runner:
    def __init__(self, tree, w, rng, rng2, rng3):
        import torch
        self.torch, self.tree, self.w, self.rng, self.rng2, self.rng3 = torch, tree, w, rng, rng2, rng3
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.Stream(self.dev)
        self.tdt = torch.float32 if w.dt == np.float32 else torch.float64
        self.base = 0
        self.tag = ""

    def device(self):
        return bool(self.rng.integers(0, 2))

    def device2(self):
        return bool(self.rng2.integers(0, 2))

    def device3(self):
        return bool(self.rng3.integers(0, 2))

    def on_stream(self, fn):
        """fn(stream handle) enqueued on the runner's own stream; its tensors as numpy arrays"""
        torch = self.torch
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            out = fn(self.stream.cuda_stream)
        self.stream.synchronize()
        return [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in out]

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    # each entry: checks against the want side, returns the bytes of its answer (index base taken out)
    def self_(self, q):
        t, w, k = self.tree, self.w, q["k"]
        blob = b""
        for include in (False, True):
            w_idx, w_dist = w.knn(k, include)
            if self.device():
                idx, dist = self.on_stream(lambda s: t.query_self_device(k, include, stream=s))
            else:
                idx, dist = t.query_self(k, include)
            idx = idx.astype(np.int64) - self.base
            what = f"{self.tag} query_self({k}, include_self={include})"
            eq_bits(dist.reshape(w_dist.shape), w_dist, what)
            fin = ~np.isnan(w_dist)
            eq(idx.reshape(w_idx.shape)[fin], w_idx[fin], what)
            blob += idx.reshape(w_idx.shape)[fin].tobytes() + dist.tobytes()
        return blob

    def radius_lists(self, r, r_dev, include, with_distance, sort, what):
        t, w = self.tree, self.w
        w_off, w_idx, w_dist = w.lists(r, include, sort)
        if self.device():
            cap = int(w_off[-1]) + 3
            off, idx, dist, tot = self.on_stream(lambda s: t.query_radius_self_device(
                r_dev(), cap, with_distance, sort, include, stream=s))
            assert int(tot[0]) == int(w_off[-1]), what
            idx = idx[:int(w_off[-1])]
            dist = dist[:int(w_off[-1])] if with_distance else None
        else:
            off, idx, dist = t.query_radius_self(r, with_distance, sort, include)
        eq(off, w_off, what + ": offsets")
        idx = idx.astype(np.int64) - self.base
        eq(idx, w_idx, what + ": indices")
        if with_distance:
            eq_bits(dist, w_dist, what + ": distances")
        return off.astype(np.int64).tobytes() + idx.tobytes() + (dist.tobytes() if with_distance else b"")

    def radius(self, q):
        r = q["eps"]
        inc = q["include"]  # (drawn once per case: the flags are parameters too)
        a = self.radius_lists(r, lambda: float(r), inc, True, True, f"{self.tag} query_radius_self({r}, sorted, include={inc})")
        b = self.radius_lists(r, lambda: float(r), not inc, False, False, f"{self.tag} query_radius_self({r}, include={not inc})")
        return a, b

    def radii(self, q):
        radii = np.ascontiguousarray(self.w.cores(q["k"]))
        inc, sort = not q["include"], q["include"]
        return self.radius_lists(radii, lambda: self.up(radii), inc, True, sort,
                                 f"{self.tag} query_radius_self(core distances of k = {q['k']}, sort={sort}, include={inc})")

    def dbscan(self, q):
        t = self.tree
        w_labels, w_core, w_ncl = self.w.dbscan(q["eps"], q["ms"])
        what = f"{self.tag} dbscan({q['eps']}, {q['ms']})"
        if self.device():
            labels, core, ncl = self.on_stream(lambda s: t.dbscan_device(q["eps"], q["ms"], stream=s))
            assert int(ncl[0]) == w_ncl, what
        else:
            labels, core = t.dbscan(q["eps"], q["ms"])
        eq(core.astype(bool), w_core, what + ": core flags")
        eq(labels, w_labels, what + ": labels")
        return labels.tobytes() + core.astype(np.uint8).tobytes()

    def mst_any(self, k):
        t, w = self.tree, self.w
        lo, hi, key = w.mst(k)
        core = None if k is None else np.ascontiguousarray(w.cores(k))
        what = f"{self.tag} mst({'None' if k is None else f'cores of k = {k}'})"
        if self.device():
            d_core = None if core is None else self.up(core)
            src, dst, weight = self.on_stream(lambda s: t.mst_device(d_core, stream=s))
        else:
            src, dst, weight = t.mst(core)
        src, dst = src.astype(np.int64) - self.base, dst.astype(np.int64) - self.base
        eq(src, lo, what + ": src")
        eq(dst, hi, what + ": dst")
        assert np.array_equal(weight.view(key.dtype), bits_of_keys(key, w.cosine)), what + ": weights"
        return src.tobytes() + dst.tobytes() + weight.tobytes()

    def mst(self, q):
        return self.mst_any(None)

    def mst_cored(self, q):
        return self.mst_any(q["k"])

    def linkage(self, q):
        t, w = self.tree, self.w
        lo, hi, key = w.mst(q["k"])
        weight = w.weights(key)
        w_left, w_right, w_size, ok = seq_linkage(w.n, lo, hi)
        assert ok
        what = f"{self.tag} linkage(tree under the cores of k = {q['k']})"
        if self.device():
            edges = (self.up(lo + self.base), self.up(hi + self.base), self.up(weight))
            left, right, wgt, size, err = self.on_stream(lambda s: t.linkage_device(edges=edges, stream=s))
            assert int(err[0]) == 0, what
        else:
            left, right, wgt, size = t.linkage(edges=((lo + self.base).astype(np.uint64), (hi + self.base).astype(np.uint64), weight))
        eq(left, w_left, what + ": left")
        eq(right, w_right, what + ": right")
        eq(size, w_size, what + ": size")
        assert wgt.tobytes() == weight.tobytes(), what + ": weights"
        return left.astype(np.int64).tobytes() + right.astype(np.int64).tobytes() + size.astype(np.int64).tobytes()

    def hdbscan(self, q):
        t, w = self.tree, self.w
        w_labels, w_prob, w_ncl, info = w.hdbscan(q["m"], q["k"])
        what = f"{self.tag} hdbscan({q['m']}, {q['k']})"
        if info["gap"] < MIN_GAP:  # (the changed parameters of pass 2 are not redrawn: the comparison needs the gap)
            print(f"{what}: least gap {info['gap']:.3g}, not compared")
            return b""
        if self.device():
            labels, prob, ncl = self.on_stream(lambda s: t.hdbscan_device(q["m"], q["k"], stream=s))
            ncl = int(ncl[0])
        else:
            labels, prob = t.hdbscan(q["m"], q["k"])
            ncl = t.last_n_clusters
        assert ncl == w_ncl, what
        eq(labels, w_labels, what + ": labels")
        eq_bits(prob, w_prob, what + ": probabilities")
        return labels.tobytes() + prob.tobytes()

    def lof(self, q):
        t, w, k = self.tree, self.w, q["k"]
        what = f"{self.tag} lof({k})"
        idx, dist = t.query_self(k)  # anchored to the matrix first
        w_idx, w_dist = w.knn(k, False)
        eq_bits(dist, w_dist, what + ": the library's query_self against the matrix")
        idx = idx.astype(np.int64) - self.base
        fin = ~np.isnan(w_dist)
        eq(idx[fin], w_idx[fin], what + ": the library's query_self against the matrix")
        w_lof, w_lrd, w_kdist = ref_fit(idx, dist, k)
        if self.device():
            lof, lrd, kdist = self.on_stream(lambda s: t.lof_device(k, stream=s))
        else:
            lof, lrd, kdist = t.lof(k, full=True)
        eq_bits(kdist, w_kdist, what + ": kdist")
        eq_bits(lrd, w_lrd, what + ": lrd")
        eq_bits(lof, w_lof, what + ": lof")
        # 64 fresh queries near the rows; their k-NN answer is anchored to the oracle before it feeds the reference
        nq = 64
        qs = w.x[self.rng.integers(0, w.n, nq)] + w.dt.type(0.01) * (self.rng.random((nq, w.x.shape[1])).astype(w.dt) - w.dt.type(0.5))
        qs = np.ascontiguousarray(np.where(np.isnan(qs), w.dt.type(0.25), qs), dtype=w.dt)
        qi, qd = t.query_batch(qs, k)
        qi = qi.astype(np.int64) - self.base
        if not w.cosine:
            oi, od = oracle.brute_knn(w.x, qs, k)
            fin = ~np.isnan(od)
            eq_bits(qd, od, what + ": query_batch against the oracle")
            eq(qi[fin], oi[fin], what + ": query_batch against the oracle")
        want = ref_score(qi, qd, w_lrd, w_kdist, k)
        if self.device():
            d_q, d_lrd, d_kdist = self.up(qs), self.up(w_lrd), self.up(w_kdist)
            got = self.on_stream(lambda s: [t.lof_score_device(d_q, k, d_lrd, d_kdist, stream=s)])[0]
        else:
            got = t.lof_score(qs, k, w_lrd, w_kdist)
        eq_bits(got, want, what + ": lof_score")
        return lof.tobytes() + lrd.tobytes() + kdist.tobytes()

    def optics(self, q):
        t, w = self.tree, self.w
        want = w.optics(q["ms"], q["max_eps"])
        what = f"{self.tag} optics({q['ms']}, {q['max_eps']})"
        if self.device():
            got = self.on_stream(lambda s: t.optics_device(q["ms"], q["max_eps"], stream=s))
        else:
            got = t.optics(q["ms"], q["max_eps"])
        eq(got[0], want[0], what + ": ordering")
        eq(got[2], want[2], what + ": predecessors")
        eq_bits(got[1], want[1], what + ": reachability")
        eq_bits(got[3], want[3], what + ": core distances")
        return b"".join(np.asarray(g).astype(g.dtype if g.dtype.kind == "f" else np.int64).tobytes() for g in got)

    def extract(self, q):
        t, w = self.tree, self.w
        w_o, w_r, w_p, w_c = w.optics(q["ms"], q["max_eps"])
        blob = b""
        for eps in (w.dt.type(q["max_eps"]), w.dt.type(0.7 * float(q["max_eps"]))):
            what = f"{self.tag} optics_dbscan({eps}) of optics({q['ms']}, {q['max_eps']})"
            w_labels, w_ncl = cpu_extract(w_o, w_r, w_c, eps)
            if self.device():
                args = (self.up(w_o.astype(np.int64)), self.up(w_r), self.up(w_c))
                labels, ncl, err = self.on_stream(lambda s: t.optics_dbscan_device(eps, *args, stream=s))
                assert int(err[0]) == 0, what
                ncl = int(ncl[0])
            else:
                labels, ncl = t.optics_dbscan(eps, w_o, w_r, w_c)
            assert ncl == w_ncl, what
            eq(labels, w_labels, what + ": labels")
            # dbscan itself: the rows with core < eps are DBSCAN(eps, min_samples + 1)'s core rows, split alike
            db_labels, db_core = t.dbscan(eps, q["ms"] + 1)
            with np.errstate(invalid="ignore"):
                near = w_c < eps
            eq(db_core, near, what + ": dbscan's core rows")
            assert (labels[near] >= 0).all() and same_partition(labels[near], db_labels[near]), what
            assert w_ncl == int(db_labels.max()) + 1, what
            blob += labels.tobytes()
        return blob

    def bandwidths(self, count, eps, per_query):
        """the scalar eps, or one bandwidth per query: eps * (0.5 .. 1), every 97th from the second on not positive or NaN
        (Cosine distances may lie a few ulp below 0: no bandwidth 0 there)"""
        if not per_query:
            return self.w.dt.type(eps)
        h = (float(eps) * np.random.default_rng(count).uniform(0.5, 1.0, count)).astype(self.w.dt)
        bad = np.arange(1, count, 97)
        h[bad] = np.resize(np.array([-1.0 if self.w.cosine else 0.0, -1.0, np.nan], dtype=self.w.dt), len(bad))
        return h

    def kde_compare(self, got, lists_at, h, count, kernel, atol, what):
        """(sum, count, cutoff) of one KDE call against the matrix: ``lists_at(cutoffs)`` gives (offsets, distances)"""
        w = self.w
        s, cnt, cut = got
        hq = np.full(count, h, dtype=w.dt) if np.ndim(h) == 0 else h
        live = hq > 0
        if kernel in COMPACT:
            eq_bits(cut, hq, what + ": cutoff against h")
        elif atol == 0.0:
            eq_bits(cut, np.where(live, w.dt.type(np.inf), hq), what + ": cutoff against +inf")
        else:
            eq_bits(cut[~live], hq[~live], what + ": cutoff of a bandwidth that is not positive")
            assert cutoff_within_bounds(cut[live], smooth_cutoff(kernel, hq[live].astype(np.float64), w.n, atol)), what
        off, dist = lists_at(cut)
        want, want_cnt = kde_sums(off, dist, hq, kernel)
        eq(cnt, want_cnt, what + ": count")
        if kernel in COMPACT:
            eq_bits(s, want, what + ": sum")
        else:
            dev, bound = np.abs(s - want), smooth_bound(want, want_cnt)
            assert (dev <= bound).all(), f"{what}: {int((dev > bound).sum())} sums beyond the bound"
        return s.tobytes() + cnt.astype(np.int64).tobytes() + cut.tobytes()

    def kde_self(self, q):
        t, w = self.tree, self.w
        kernel, include, per_row = q["kde"]["self_kernel"], q["kde"]["include"], q["kde"]["per_row"] and w.n >= 2
        atol = 0.0 if kernel in COMPACT or w.n <= 1000 else KDE_ATOL
        h = self.bandwidths(w.n, q["eps"], per_row)
        what = (f"{self.tag} kernel_density_raw(None, {'one h per row' if per_row else h}, {kernel}, atol={atol}, "
                f"include_self={include})")
        if self.device2():
            dh = self.up(h) if per_row else float(h)
            got = self.on_stream(lambda s: t.kernel_density_self_device(dh, kernel, atol, include, stream=s))
        else:
            got = t.kernel_density_raw(None, h, kernel, atol, include_self=include)
        return self.kde_compare(got, lambda cut: w.lists(cut, include, False)[::2], h, w.n, kernel, atol, what)

    def kde(self, q):
        t, w = self.tree, self.w
        kernel, per_query = q["kde"]["kernel"], q["kde"]["per_query"]
        atol = 0.0 if kernel in COMPACT or w.n <= 1000 else KDE_ATOL
        sel = np.sort(np.random.default_rng(w.n + 1).choice(w.n, min(w.n, KDE_QUERIES), replace=False))
        qs = np.ascontiguousarray(np.concatenate([w.x[sel], np.full((1, w.x.shape[1]), np.nan, dtype=w.dt)]))
        nq = len(qs)
        h = self.bandwidths(nq, q["eps"], per_query)
        what = f"{self.tag} kernel_density_raw({nq} queries, {'one h per query' if per_query else h}, {kernel}, atol={atol})"
        if self.device2():
            dq, dh = self.up(qs), self.up(h) if per_query else float(h)
            got = self.on_stream(lambda s: t.kernel_density_device(dq, dh, kernel, atol, stream=s))
        else:
            got = t.kernel_density_raw(qs, h, kernel, atol)
        assert got[0][-1] == 0 and got[1][-1] == 0, what + ": the NaN query"

        def lists_at(cut):  # the matrix rows of the subset; the NaN query lists nothing
            off, dist = w.lists_of(sel, cut[:-1])
            return np.concatenate([off, off[-1:]]), dist
        blob = self.kde_compare(got, lists_at, h, nq, kernel, atol, what)
        if w.cosine:  # the normalisers are volumes of Euclidean balls
            try:
                t.kernel_density(qs, h, kernel=kernel, atol=atol)
            except ValueError:
                return blob
            raise AssertionError(what + ": kernel_density(normalize=True) on a Cosine tree must raise")
        return blob

    def mean_shift(self, q):
        t, w = self.tree, self.w
        h = w.dt.type(q["eps"])
        what = f"{self.tag} mean_shift_modes({h}, the rows, max_iter=1)"
        if w.cosine:
            try:
                t.mean_shift_modes(h, None, tol=0.0, max_iter=1)
            except ValueError:
                return b""
            raise AssertionError(what + ": on a Cosine tree must raise")
        off, idx, _ = w.lists(h, True, False)
        w_modes, w_pw, w_shift = ms_step(w.x, w.x, off, idx)
        if self.device2():
            modes, pw, it, sh, work = self.on_stream(lambda s: t.mean_shift_modes_device(float(h), None, tol=0.0, max_iter=1, stream=s))
        else:
            modes, pw, it, sh, work = t.mean_shift_modes(h, None, tol=0.0, max_iter=1, full=True)
        eq(pw, w_pw, what + ": points_within")
        eq(it, w_pw > 0, what + ": iterations")
        eq_bits(modes, w_modes, what + ": modes")
        eq_bits(sh, w_shift, what + ": shift")
        assert tuple(work) == (1, w.n), what
        nan_rows = np.isnan(w.x).any(axis=1)
        assert (w_pw[nan_rows] == 0).all() and np.isnan(w_shift[nan_rows]).all(), what  # in no list: dead seeds
        blob = modes.tobytes() + pw.astype(np.int64).tobytes() + sh.tobytes()
        # the labels against centres picked from the rows: the matrix columns, by (key, centre number)
        cs = np.sort(np.random.default_rng(w.n + 2).choice(w.n, min(w.n, MS_CENTRES), replace=False))
        centres = np.ascontiguousarray(w.x[cs])
        lab = np.argmin(w.dk[:, cs], axis=1).astype(np.int64)  # (the first of equal minima: the lower centre)
        with np.errstate(invalid="ignore"):
            near = w.d[np.arange(w.n), cs[lab]] < h
        for cluster_all in (True, False):
            if self.device2():
                dc = self.up(centres)
                got = self.on_stream(lambda s: [t.mean_shift_labels_device(dc, float(h), cluster_all, stream=s)])[0]
            else:
                got = t.mean_shift_labels(centres, h, cluster_all)
            eq(got, lab if cluster_all else np.where(near, lab, -1), f"{self.tag} mean_shift_labels({len(cs)} rows, {h}, {cluster_all})")
            blob += got.tobytes()
        return blob

    def kmeans(self, q):
        t, w, torch = self.tree, self.w, self.torch
        cs = q["km"]
        nc = len(cs)
        centres = np.ascontiguousarray(w.x[cs])
        what = f"{self.tag} kmeans_assign({nc} rows)"
        if w.cosine:
            for fn in (lambda: t.kmeans_assign(centres), lambda: t.kmeans_assign_device(self.up(centres)),
                       lambda: t.kmeans(centres, abs_tol=0.0, max_iter=KM_ITERATIONS),
                       lambda: t.kmeans_device(self.up(centres), 0.0, KM_ITERATIONS)):
                try:
                    fn()
                except ValueError:
                    continue
                raise AssertionError(what + ": on a Cosine tree must raise")
            return b""
        # the assignment against the matrix: its columns of the centres, by (key, centre number)
        lab = np.argmin(w.dk[:, cs], axis=1).astype(np.int64)  # (the first of equal minima: the lower centre)
        w_dist = np.ascontiguousarray(w.d[np.arange(w.n), cs[lab]])
        w_inertia = kmeans_reference.inertia(lab, w_dist)
        before = t.stats()["queries"]
        if self.device3():
            dc = self.up(centres)
            labels, dist, inertia = self.on_stream(lambda s: t.kmeans_assign_device(dc, stream=s))
            inertia = inertia[0]
        else:
            labels, dist, inertia = t.kmeans_assign(centres)
        assert t.stats()["queries"] - before == w.n, what
        eq(labels, lab, what + ": labels")
        eq_bits(dist, w_dist, what + ": distances")
        eq_bits(np.array([inertia], dtype=np.float64), np.array([w_inertia]), what + ": inertia")
        blob = labels.astype(np.int64).tobytes() + dist.tobytes()
        # two iterations from the same centres against the reference of the loop
        what = f"{self.tag} kmeans({nc} rows, abs_tol=0, max_iter={KM_ITERATIONS})"
        want = w.memo(("km", cs.tobytes()), lambda: kmeans_reference.kmeans(w.x, centres, 0.0, KM_ITERATIONS,
                                                                          assign=kmeans_reference.assign_matrix))
        if self.device3():
            dc = self.up(centres)
            c, l, d, cnt, inr, it, s2 = self.on_stream(lambda s: t.kmeans_device(dc, 0.0, KM_ITERATIONS, stream=s))
            inr, it, s2 = inr[0], int(it[0]), s2[0]
        else:
            c, l, inr, d, cnt, it, s2 = t.kmeans(centres, abs_tol=0.0, max_iter=KM_ITERATIONS, full=True)
        w_c, w_l, w_d, w_cnt, w_inr, w_it, w_s2 = want
        assert it == w_it, what + ": iterations"
        eq(l, w_l, what + ": labels")
        eq(cnt, w_cnt.astype(np.int64), what + ": counts")
        eq_bits(c, w_c, what + ": centres")
        eq_bits(d, w_d, what + ": distances")
        eq_bits(np.array([inr, s2], dtype=np.float64), np.array([w_inr, w_s2], dtype=np.float64),
                what + ": inertia, shift2")
        return blob + c.tobytes() + l.astype(np.int64).tobytes() + d.tobytes() + cnt.astype(np.int64).tobytes()

    def call(self, name, q):
        if name == "lof" and self.w.n < 2:
            try:
                self.tree.lof(1)
            except ValueError:
                return b""
            raise AssertionError("lof on one row must raise")
        return {"self": self.self_}.get(name, getattr(self, name, None))(q)


def draw_kde(rng):
    """what a round's KDE calls use: one kernel each, the self entry's flag, scalar or per-query bandwidths"""
    kernels = COMPACT + SMOOTH
    return {"kernel": str(rng.choice(kernels)), "self_kernel": str(rng.choice(kernels)), "include": bool(rng.integers(0, 2)),
            "per_query": bool(rng.integers(0, 2)), "per_row": bool(rng.integers(0, 2))}


def draw_km(rng3, n):
    """what a round's k-means calls use: the rows taken as centres, ascending"""
    nc = min(int(rng3.choice(KM_CENTRES)), n)
    return np.sort(rng3.choice(n, nc, replace=False))


def order_of(rng, rng2, rng3):
    """the graph entries in a random order drawn from ``rng``, the KDE and mean shift entries put in at places drawn from
    ``rng2``, then the k-means entry at a place drawn from ``rng3``: what ``rng`` gives the graph entries does not depend
    on the entries beside them, nor what ``rng2`` gives the density entries"""
    names = [str(x) for x in rng.permutation(GRAPH_ENTRIES)]
    for name in DENSITY_ENTRIES:
        names.insert(int(rng2.integers(0, len(names) + 1)), name)
    for name in KMEANS_ENTRIES:
        names.insert(int(rng3.integers(0, len(names) + 1)), name)
    return names


def pieces_value(rng, total):
    """0 (the default), 1, or a value that cuts `total` into 5 or more pieces"""
    return int(rng.choice([0, 1, max(int(total) // 6, 1)]))


def run_once(p, seed, rng, what):
    """one tree, one want side, two passes; None if the case misses a condition it must meet"""
    x = make_rows(p, seed)
    w = Want(x, p["cosine"])
    q = derive(p, w)
    q["include"] = bool(rng.integers(0, 2))
    rng2 = np.random.default_rng([int(seed), 0x4DE5])  # every draw of the KDE and mean shift entries: the case's own generator
    q["kde"] = draw_kde(rng2)
    n, dim = x.shape
    rng3 = np.random.default_rng([int(seed), 0x4B4D])  # ... and every draw of the k-means entry
    q["km"] = draw_km(rng3, n)
    ok, text = conditions(q, w)
    must = p["family"] in BLOB_FAMILIES and n >= 1000
    print(f"{what}: k {q['k']}, min_samples {q['ms']}, min_cluster_size {q['m']}, kde {q['kde']}; {text}"
          f"; kmeans from {len(q['km'])} rows"
          f"{'' if ok or not must else ' -- MISSED'}", flush=True)
    if must and not ok:
        return None
    tree = pn.BallTree.new(x, pn.distance.Cosine()) if p["cosine"] else pn.BallTree.euclidean(x)
    try:
        r = Runner(tree, w, rng, rng2, rng3)
        # a row with a non-finite value rules the bf16 tier out for the whole index, by design: such a case runs the exact
        # scan at its width, and that is asserted instead
        finite = bool(np.isfinite(x).all())
        tier = n >= 4096 and dim >= 8 and finite
        if n >= 4096 and dim >= 8:
            assert bool(tree.bf16_eligible) == finite, what
        before = tree.stats()
        # ---- pass 1
        r.tag = "pass 1:"
        first = {}
        for name in order_of(rng, rng2, rng3):
            first[name] = r.call(name, q)
        after = tree.stats()
        dq, dc, df = (after[f] - before[f] for f in ("queries", "candidates", "fallback_queries"))
        print(f"{what}: pass 1 served {dq} queries, {dc} candidates, {df} fallback queries", flush=True)
        if tier:
            assert dc > 0 and df < dq, f"{what}: the bf16 tier did not serve the case"
        # ---- pass 2: options redrawn, parameters larger, then smaller, then pass 1's again
        engine = str(rng.choice(["auto", "bf16", "exact"]))
        if engine == "bf16" and not tree.bf16_eligible:  # (the library refuses the tier where it cannot serve the index)
            engine = "auto"
        tree.set_engine(engine)
        r.base = int(rng.choice([0, 1 << 33]))
        tree.set_option(_lib.PN_OPT_INDEX_BASE, r.base)
        entries = int(w.lists(q["eps"], True, False)[0][-1])
        opts = {_lib.PN_OPT_DBSCAN_PIECE: pieces_value(rng, entries), _lib.PN_OPT_OPTICS_PIECE: pieces_value(rng, entries),
                _lib.PN_OPT_MST_BATCH: pieces_value(rng, n), _lib.PN_OPT_KDE_PIECE: pieces_value(rng2, entries),
                _lib.PN_OPT_MS_PIECE: pieces_value(rng2, entries)}
        for o, v in opts.items():
            tree.set_option(o, v)
        km_filter = int(rng3.choice([0, 1, 2]))
        tree.set_option(_lib.PN_OPT_KMEANS_FILTER, km_filter)
        print(f"{what}: pass 2 under engine {engine}, index base {r.base}, dbscan / optics piece "
              f"{opts[_lib.PN_OPT_DBSCAN_PIECE]} / {opts[_lib.PN_OPT_OPTICS_PIECE]}, mst batch {opts[_lib.PN_OPT_MST_BATCH]}, "
              f"kde / mean shift piece {opts[_lib.PN_OPT_KDE_PIECE]} / {opts[_lib.PN_OPT_MS_PIECE]}, kmeans filter {km_filter}",
              flush=True)
        half = w.dt.type(0.5)
        larger = dict(q, k=max(min(2 * q["k"] + 3, n - 1, KMAX), 1), ms=max(min(2 * q["ms"] + 1, n - 1, KMAX), 1), m=2 * q["m"],
                      eps=q["eps"] * half, max_eps=q["max_eps"] * half, include=not q["include"], kde=draw_kde(rng2), km=draw_km(rng3, n))
        smaller = dict(q, k=max(q["k"] // 2, 1), ms=max(q["ms"] // 2, 1), m=max(q["m"] // 2, 2), eps=q["eps"] * half,
                       kde=draw_kde(rng2), km=draw_km(rng3, n))
        for tag, qq in (("pass 2, larger:", larger), ("pass 2, smaller:", smaller)):
            r.tag = tag
            for name in order_of(rng, rng2, rng3):
                r.call(name, qq)
        r.tag = "pass 2, unchanged:"
        for name in order_of(rng, rng2, rng3):
            got = r.call(name, q)
            assert got == first[name], f"{what}: {name} with unchanged parameters differs from pass 1"
    finally:
        tree.close()
    return True


def run_case(params, rng):
    """params: n, dim, dtype, cosine, family, seed and, optionally, nb / sigma / background / k / ms / m / eps / max_eps.
    Returns the number of redraws of the data seed (0, 1 or 2); a mismatch raises AssertionError."""
    p = dict(params)
    what = (f"{p['n']} x {p['dim']} {np.dtype(p['dtype']).name} {'cosine' if p['cosine'] else 'euclidean'} {p['family']}")
    for redraw in range(3):
        if run_once(p, p["seed"] + 7919 * redraw, rng, what + (f" (redraw {redraw})" if redraw else "")):
            return redraw
    raise AssertionError(f"{what}: the conditions were missed three times")


def draw_params(c, rng):
    n = int(rng.choice([1, 2, 3, 64, 65, 1000, 4095, 4096, 4500]))
    dim = int(rng.choice([1, 2, 3, 8, 16, 33, 100, 128, 129, 200]))
    family = str(rng.choice(["uniform", "blobs", "dups", "lattice", "sorted"]))
    return {"n": n, "dim": dim, "dtype": np.float64 if rng.integers(0, 3) == 0 else np.float32,
            # (one column has two directions: every Cosine distance is 0 or 2 and every list half the corpus)
            "cosine": bool(rng.integers(0, 4) == 0) and dim >= 2, "family": family, "seed": 1000 + c}


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    bad = redraws = 0
    for c, params in enumerate([draw_params(c, rng) for c in range(cases)]):
        try:
            redraws += run_case(params, rng)
        except AssertionError as e:
            bad += 1
            print(f"case {c}: MISMATCH {e}", flush=True)
    print("mismatches:", bad, "redraws:", redraws)
    sys.exit(1 if bad else 0)
