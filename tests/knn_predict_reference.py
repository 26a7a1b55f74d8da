"""The contract of pn_knn_classify_* / pn_knn_regress_* (include/petal_mi355x.h) in plain NumPy -- a helper, not collected.

The lists are taken as they come (``query_batch`` / ``query_self``: row numbers without the index base, ordered by
(distance, index)); everything above them is done here: a Python loop over the list position t = 0 .. k - 1, vectorised
over the queries, f64 throughout, one addition per t -- which is the sequential sum in list order, starting from 0.
"""
import numpy as np


def weights(dist, distance):
    """``(w float64 [nq, k], has_nan bool [nq])``: the clamp, then uniform or scikit-learn's ``_get_weights`` rule"""
    d = np.asarray(dist).astype(np.float64)
    has_nan = np.isnan(d).any(axis=1)
    v = np.where(d > 0, d, 0.0)  # (NaN > 0 is False: such lists are poisoned below, whatever their weights)
    if not distance:
        return np.ones_like(v), has_nan
    zero = (v == 0).any(axis=1)
    with np.errstate(all="ignore"):
        inv = 1.0 / v
    return np.where(zero[:, None], (v == 0).astype(np.float64), inv), has_nan


def classify(idx, dist, labels, n_classes, distance=False):
    """``(pred int64 [nq], proba float64 [nq, n_classes])`` from the lists and ``labels`` int64 [n]"""
    idx = np.asarray(idx).astype(np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    nq, k = idx.shape
    w, poison = weights(dist, distance)
    lab = labels[idx]
    inside = (lab >= 0) & (lab < n_classes)
    poison = poison | ~inside.all(axis=1)
    lab = np.where(inside, lab, 0)
    rows = np.arange(nq)
    W = np.zeros((nq, n_classes), dtype=np.float64)
    S = np.zeros(nq, dtype=np.float64)
    for t in range(k):
        W[rows, lab[:, t]] = W[rows, lab[:, t]] + w[:, t]
        S = S + w[:, t]
    pred = np.argmax(W, axis=1).astype(np.int64)  # the first maximum: the smallest class
    with np.errstate(all="ignore"):
        proba = W / S[:, None]
    pred[poison] = -1
    proba[poison] = np.nan
    return pred, proba


def regress(idx, dist, targets, distance=False):
    """``out float64 [nq, n_out]`` from the lists and ``targets`` float64 [n, n_out]"""
    idx = np.asarray(idx).astype(np.int64)
    y = np.asarray(targets, dtype=np.float64)
    y = y.reshape(len(y), -1)
    nq, k = idx.shape
    w, poison = weights(dist, distance)
    N = np.zeros((nq, y.shape[1]), dtype=np.float64)
    S = np.zeros(nq, dtype=np.float64)
    with np.errstate(all="ignore"):
        for t in range(k):
            N = N + w[:, t, None] * y[idx[:, t]]  # each product rounded, then added
            S = S + w[:, t]
        out = N / S[:, None]
    out[poison] = np.nan
    return out


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN masks differ ({int(gn.sum())} against {int(wn.sum())})"
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    bad = np.flatnonzero(np.ascontiguousarray(got).view(u)[~gn] != np.ascontiguousarray(want).view(u)[~wn])
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at {bad[:5]}: {got[~gn][bad[:5]]} against {want[~wn][bad[:5]]}"
