"""References that scale to 3 10^5 rows, for checks beyond one 2^18-row pipeline chunk, where the quadratic references
of the other modules no longer fit; each is proven on the CPU against the quadratic one it replaces
(tests/test_graph_reference_large.py): ``heap_optics`` against optics_reference.cpu_optics, ``sparse_mst`` against
test_gpu_mst.prim, ``grid_lists`` against the dense fold.
"""
import heapq

import numpy as np

from optics_reference import core_from_lists, fold_pairs


def heap_optics(offsets, idx, dist, min_samples):
    """The contract of optics_reference.cpu_optics -- (ordering uint64, reachability, predecessor int64, core_distances)
    over CSR lists without the row itself -- with a binary heap of (reach, row) and lazy deletion in place of the argmin
    over n.  A reachability only ever decreases strictly, so a popped entry is current exactly when the row is still
    unprocessed and its reachability equals the entry's; the heap's order (reach, row) is the contract's pick, and when the
    heap holds nothing current the lowest unprocessed row goes next.  Floats are compared as Python floats: the
    conversion of f32 and f64 is exact and monotone."""
    n = len(offsets) - 1
    core = core_from_lists(offsets, dist, min_samples)
    reach = np.full(n, np.inf, dtype=dist.dtype)
    pred = np.full(n, -1, dtype=np.int64)
    ordering = np.empty(n, dtype=np.uint64)
    todo = np.ones(n, dtype=bool)
    finite = np.isfinite(core)
    heap = []
    lowest = 0
    for t in range(n):
        p = -1
        while heap:
            r, q = heapq.heappop(heap)
            if todo[q] and reach[q] == r:
                p = q
                break
        if p < 0:
            while not todo[lowest]:
                lowest += 1
            p = lowest
        ordering[t] = p
        todo[p] = False
        if finite[p]:
            c = core[p]
            a, b = offsets[p], offsets[p + 1]
            q = idx[a:b]
            d = dist[a:b]
            new = np.where(d > c, d, c)
            upd = todo[q] & (new < reach[q])
            q, new = q[upd], new[upd]
            reach[q] = new
            pred[q] = p
            for item in zip(new.tolist(), q.tolist()):
                heapq.heappush(heap, item)
    return ordering, reach, pred, core


def sparse_mst(n, cand_i, cand_j, cand_key):
    """(lo, hi, key, spans): Kruskal with union-find over the candidate edges {cand_i[t], cand_j[t]} of key cand_key[t],
    taken in the strict order (key, lo, hi) -- lo < hi the edge's ends; an edge may be listed from both ends, a pair of
    equal ends is ignored.  The forest's edges come out in that order; ``spans`` tells whether they are n - 1.

    Under a strict total order the minimum spanning tree is unique, so this is the tree of the candidate graph.  It is the
    tree of the COMPLETE graph under w(i, j) = max(d(i, j), core[i], core[j]) (cores optional) when the caller asserts this
    certificate: the candidates are all pairs with d < R, the result spans, and its largest key is below the key of R.
    Every edge left out has w >= d >= R, above every edge of a path of the result that joins its ends; by the cycle
    property it is in no minimum spanning tree.

    Cost: one lexsort and one Python loop that stops at the (n - 1)-th edge; 10^7 random candidates over 3 10^5 rows take
    about 10 s of one CPU core, the 4.2 10^6 candidates of 2^18 + 3000 rows in the plane about 5 s."""
    i = np.asarray(cand_i, dtype=np.int64)
    j = np.asarray(cand_j, dtype=np.int64)
    key = np.asarray(cand_key)
    keep = i < j  # (each undirected edge once: listed from both ends it carries the same key)
    other = i > j
    lo = np.concatenate([i[keep], j[other]])
    hi = np.concatenate([j[keep], i[other]])
    k = np.concatenate([key[keep], key[other]])
    order = np.lexsort((hi, lo, k))
    lo, hi, k = lo[order], hi[order], k[order]
    parent = list(range(n))
    taken = []
    need = n - 1
    for t, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            parent[b] = a
            taken.append(t)
            if len(taken) == need:
                break
    taken = np.asarray(taken, dtype=np.int64)
    return lo[taken], hi[taken], k[taken], len(taken) == max(n - 1, 0)


def grid_lists(pts, r):
    """CSR lists { j != i : d(i, j) < r } of rows in [0, 1)^2, ascending j, with the distances by the reference's fold:
    (offsets int64 [n + 1], idx int64, dist).  The rows are bucketed into a uniform grid of cell >= 1.001 r: a pair outside
    adjacent cells is more than a cell apart in one coordinate, which no rounding of the fold (a few ulp) brings below r.
    So a row's neighbours lie in its own and the eight adjacent cells; every pair of those is folded and compared
    (strict '<')."""
    n = len(pts)
    assert pts.ndim == 2 and pts.shape[1] == 2 and float(r) > 0
    assert bool(((pts >= 0) & (pts < 1)).all()), "grid_lists takes rows in [0, 1)^2"
    g = max(int(np.floor(1.0 / (1.001 * float(r)))), 1)
    cell = np.minimum((pts.astype(np.float64) * g).astype(np.int64), g - 1)
    cid = cell[:, 0] * g + cell[:, 1]
    by_cell = np.argsort(cid, kind="stable")
    start = np.searchsorted(cid[by_cell], np.arange(g * g + 1))
    out_i, out_j, out_d = [], [], []
    rows = np.arange(n, dtype=np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            cx, cy = cell[:, 0] + dx, cell[:, 1] + dy
            ok = (cx >= 0) & (cx < g) & (cy >= 0) & (cy < g)
            c2 = (cx * g + cy)[ok]
            cnt = start[c2 + 1] - start[c2]
            i = np.repeat(rows[ok], cnt)
            first = np.repeat(start[c2] - (np.cumsum(cnt) - cnt), cnt)
            j = by_cell[first + np.arange(len(i))]
            d = fold_pairs(pts, i, j)
            keep = (d < pts.dtype.type(r)) & (i != j)
            out_i.append(i[keep])
            out_j.append(j[keep])
            out_d.append(d[keep])
    i, j, d = np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_d)
    order = np.lexsort((j, i))
    i, j, d = i[order], j[order], d[order]
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(i, minlength=n))
    return offsets, j, d


def truncate_lists(offsets, idx, dist, n, r=None):
    """the lists of the first n rows among themselves, cut to d < r: a prefix-filter of lists built once"""
    rows = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    keep = (rows < n) & (idx < n)
    if r is not None:
        keep &= dist < r
    out = np.zeros(n + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.bincount(rows[keep], minlength=n)[:n])
    return out, idx[keep], dist[keep]
