"""The OPTICS contract of include/petal_mi355x.h restated in numpy, for tests/test_optics_reference.py (against
scikit-learn and hand-made tie cases) and tests/test_gpu_optics.py (the want side of the device results).

The graph comes in as CSR neighbour lists WITHOUT the row itself: row i's entries are idx[offsets[i]:offsets[i + 1]] at the
distances dist[...], all of them < max_eps.  Core distances are derived from the lists: the min_samples-th smallest
distance of a row's list if the list is that long, else +inf -- the same value as "the last column of the min_samples
self-query if it is < max_eps", because that column is below max_eps exactly when min_samples other rows are.
"""
import numpy as np


def csr_from_dense(d, max_eps):
    """lists { j != i : d[i, j] < max_eps } of a dense distance matrix, ascending j"""
    n = len(d)
    with np.errstate(invalid="ignore"):
        m = d < max_eps
    m[np.arange(n), np.arange(n)] = False
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(m.sum(axis=1))
    rows, cols = np.nonzero(m)
    return offsets, cols.astype(np.int64), d[rows, cols]


def core_from_lists(offsets, dist, min_samples):
    n = len(offsets) - 1
    core = np.full(n, np.inf, dtype=dist.dtype)
    for i in np.flatnonzero(np.diff(offsets) >= min_samples):
        core[i] = np.partition(dist[offsets[i]:offsets[i + 1]], min_samples - 1)[min_samples - 1]
    return core


def cpu_optics(offsets, idx, dist, min_samples, stats=None):
    """(ordering uint64, reachability, predecessor int64, core_distances); stats (a dict) receives ``tie_picks``: the picks
    at a finite reachability that another unprocessed row shared (decided by the lower row)"""
    n = len(offsets) - 1
    core = core_from_lists(offsets, dist, min_samples)
    reach = np.full(n, np.inf, dtype=dist.dtype)
    pred = np.full(n, -1, dtype=np.int64)
    ordering = np.empty(n, dtype=np.uint64)
    todo = np.ones(n, dtype=bool)
    w = np.full(n, np.inf, dtype=dist.dtype)  # reach of the unprocessed rows, +inf for the processed ones
    lowest = 0                                # the lowest unprocessed row
    ties = 0
    for t in range(n):
        p = int(np.argmin(w))                 # (the first of equal minima: the lower row)
        if w[p] == np.inf:                    # nothing reached: the lowest unprocessed row
            while not todo[lowest]:
                lowest += 1
            p = lowest
        elif np.count_nonzero(w == w[p]) > 1:
            ties += 1
        ordering[t] = p
        todo[p] = False
        w[p] = np.inf
        c = core[p]
        if c < np.inf:
            q = idx[offsets[p]:offsets[p + 1]]
            d = dist[offsets[p]:offsets[p + 1]]
            new = np.where(d > c, d, c)
            upd = todo[q] & (new < reach[q])
            q, new = q[upd], new[upd]
            reach[q] = new
            w[q] = new
            pred[q] = p
    if stats is not None:
        stats["tie_picks"] = ties
    return ordering, reach, pred, core


def cpu_extract(ordering, reach, core, eps):
    """(labels int64, n_clusters): DBSCAN at eps read off an ordering, clusters numbered by first appearance"""
    o = np.asarray(ordering, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        far = ~(reach < eps)
        near = core < eps
    start = far[o] & near[o]
    labels = np.empty(len(o), dtype=np.int64)
    labels[o] = np.cumsum(start) - 1
    labels[far & ~near] = -1
    return labels, int(np.count_nonzero(start))


def fold_pairs(x, i, j):
    """Euclidean distances of the pairs (i[t], j[t]) by the reference's fold, in x's dtype: acc += (a - b) * (a - b) per
    coordinate, then sqrt -- bit for bit what the oracle's scalar distance returns"""
    acc = np.zeros(len(i), dtype=x.dtype)
    with np.errstate(invalid="ignore"):
        for k in range(x.shape[1]):
            diff = x[i, k] - x[j, k]
            acc = acc + diff * diff
        return np.sqrt(acc)


def same_partition(a, b):
    """two labelings of the same rows describe the same partition (labels >= 0 on both sides)"""
    if len(a) == 0:
        return True
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))
