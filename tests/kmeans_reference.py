"""A numpy restatement of the k-means contract of include/petal_mi355x.h (pn_kmeans_*, pn_kmeans_assign_*): the
distance fold in the index's type, the (distance key, centre number) order, SUM4096, the update, shift2 and the stop
rule.  Slow and plain on purpose: it is the oracle of tests/test_gpu_kmeans.py, tests/test_gpu_kmeans_edges.py and the
k-means entry of tests/fuzz_graph.py.  fold_matrix / assign_matrix are the same operations on all centres at once, for
the shapes with thousands of centres; tests/test_kmeans_reference.py pins them to the plain ones bit for bit."""
import numpy as np

SEG = 4096


def _keys(d):
    """the sortable keys of distances: the bits read as unsigned integers, NaN as the canonical quiet NaN above +inf"""
    d = np.ascontiguousarray(d)
    if d.dtype == np.float32:
        k = d.view(np.uint32).astype(np.uint64)
        return np.where(np.isnan(d), np.uint64(0x7FC00000), k)
    k = d.view(np.uint64).copy()
    return np.where(np.isnan(d), np.uint64(0x7FF8000000000000), k)


def fold_distances(X, c):
    """Euclidean::distance of every row of X to the one centre c: sub, mul, add separately rounded in X's type, in
    column order, then a correctly rounded sqrt"""
    T = X.dtype.type
    s = np.zeros(X.shape[0], dtype=X.dtype)
    with np.errstate(all="ignore"):
        for k in range(X.shape[1]):
            diff = (T(c[k]) - X[:, k]).astype(X.dtype)
            s = (s + (diff * diff).astype(X.dtype)).astype(X.dtype)
        return np.sqrt(s).astype(X.dtype)


def assign(X, C):
    """labels int64 [n], dist [n]: the nearest centre by (distance key, centre number); no centres: -1 and NaN"""
    n = X.shape[0]
    labels = np.full(n, -1, dtype=np.int64)
    dist = np.full(n, np.nan, dtype=X.dtype)
    best = np.full(n, np.iinfo(np.uint64).max, dtype=np.uint64)
    for c in range(C.shape[0]):
        d = fold_distances(X, C[c].astype(X.dtype))
        k = _keys(d)
        take = k < best  # (strict: the lower number keeps a tie)
        labels[take] = c
        dist[take] = d[take]
        best[take] = k[take]
    return labels, dist


def fold_matrix(X, C):
    """fold_distances of every row of X to every centre of C at once, [n][nc]: the same sub, mul, add per column, each
    rounded in X's type, then the square root -- element by element the operations of fold_distances, so the same bits"""
    dt = X.dtype
    C = np.asarray(C, dtype=dt)
    s = np.zeros((X.shape[0], C.shape[0]), dtype=dt)
    with np.errstate(all="ignore"):
        for k in range(X.shape[1]):
            diff = (C[None, :, k] - X[:, k, None]).astype(dt)
            s = (s + (diff * diff).astype(dt)).astype(dt)
        return np.sqrt(s).astype(dt)


def assign_matrix(X, C):
    """assign(X, C) through fold_matrix: the first minimum of the keys is the lower centre number"""
    n = X.shape[0]
    if C.shape[0] == 0:
        return np.full(n, -1, dtype=np.int64), np.full(n, np.nan, dtype=X.dtype)
    d = fold_matrix(X, C)
    labels = np.argmin(_keys(d), axis=1).astype(np.int64)
    return labels, d[np.arange(n), labels]


def sum4096(t):
    """SUM4096 of a sequence of float64 terms; it depends on the length alone"""
    t = np.asarray(t, dtype=np.float64)
    total = None
    for b in range(0, len(t), SEG):
        seg = t[b:b + SEG]
        pad = np.zeros(-len(seg) % 64)
        rows = np.concatenate([seg, pad]).reshape(-1, 64)  # row j holds the terms l + 64 j of the lanes l
        P = np.zeros(64)
        with np.errstate(all="ignore"):
            for r in rows:
                P = P + r  # ((0.0 + t_l) + t_{l+64}) + ...; a lane past the end adds 0.0, which changes nothing
            S = P[0]
            for l in range(1, 64):
                S = S + P[l]
            total = S if total is None else total + S
    return np.float64(0.0) if total is None else np.float64(total)


def sum4096_columns(M):
    """SUM4096 down every column of a float64 matrix [m][cols] at once"""
    M = np.asarray(M, dtype=np.float64)
    total = None
    for b in range(0, M.shape[0], SEG):
        seg = M[b:b + SEG]
        pad = np.zeros((-seg.shape[0] % 64, M.shape[1]))
        rows = np.concatenate([seg, pad]).reshape(-1, 64, M.shape[1])
        P = np.zeros((64, M.shape[1]))
        with np.errstate(all="ignore"):
            for r in rows:
                P = P + r
            S = P[0].copy()
            for l in range(1, 64):
                S = S + P[l]
            total = S if total is None else total + S
    return np.zeros(M.shape[1]) if total is None else total


def inertia(labels, dist):
    d = dist.astype(np.float64)
    with np.errstate(all="ignore"):
        return sum4096(np.where(labels < 0, 0.0, d * d))


def update(X, C, labels):
    """one update: (new centres, shift2)"""
    T = X.dtype
    new = C.copy()
    shift2 = np.float64(0.0)
    with np.errstate(all="ignore"):
        for c in range(C.shape[0]):
            members = np.flatnonzero(labels == c)  # ascending row index
            if len(members):
                S = sum4096_columns(X[members].astype(np.float64))
                new[c] = (S / np.float64(len(members))).astype(T)
            t = (new[c].astype(np.float64) - C[c].astype(np.float64)) ** 2
            part = np.zeros(64)
            for col in range(len(t)):
                part[col % 64] = part[col % 64] + t[col]
            tc = part[0]
            for l in range(1, 64):
                tc = tc + part[l]
            shift2 = shift2 + tc
    return new, np.float64(shift2)


def kmeans(X, init, tol, max_iter, assign=assign):
    """(centres, labels, dist, counts uint64, inertia, iterations, shift2); ``assign=assign_matrix`` gives the same bits
    sooner on wide rows"""
    C = np.array(init, dtype=X.dtype, copy=True)
    t, shift2 = 0, np.float64(0.0)
    while True:
        t += 1
        labels, _ = assign(X, C)
        C, shift2 = update(X, C, labels)
        if shift2 <= tol or t == max_iter:
            break
    labels, dist = assign(X, C)
    counts = np.bincount(labels[labels >= 0], minlength=C.shape[0]).astype(np.uint64)
    return C, labels, dist, counts, inertia(labels, dist), t, shift2
