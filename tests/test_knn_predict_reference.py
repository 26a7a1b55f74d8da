"""The NumPy statement of the k-NN prediction contract (tests/knn_predict_reference.py) against a per-query pure-Python
loop -- a dict of class sums, float additions in list order -- and against a case small enough to derive by hand.  No
GPU: this checks the yardstick the GPU tests compare the kernels with."""
import math

import numpy as np
import pytest

import knn_predict_reference as ref


def _python_weights(dist, distance):
    if any(math.isnan(d) for d in dist):
        return None
    v = [d if d > 0 else 0.0 for d in dist]
    if not distance:
        return [1.0] * len(v)
    if any(x == 0.0 for x in v):
        return [1.0 if x == 0.0 else 0.0 for x in v]
    return [1.0 / x for x in v]


def _python_classify(idx, dist, labels, n_classes, distance):
    w = _python_weights(dist, distance)
    if w is None or any(not 0 <= labels[j] < n_classes for j in idx):
        return -1, [math.nan] * n_classes
    sums, s = {}, 0.0
    for j, wt in zip(idx, w):
        sums[labels[j]] = sums.get(labels[j], 0.0) + wt
        s = s + wt
    best = min(sums, key=lambda c: (-sums[c], c))
    return best, [sums.get(c, 0.0) / s for c in range(n_classes)]


def _python_regress(idx, dist, y, distance):
    n_out = len(y[0])
    w = _python_weights(dist, distance)
    if w is None:
        return [math.nan] * n_out
    acc, s = [0.0] * n_out, 0.0
    for j, wt in zip(idx, w):
        for o in range(n_out):
            acc[o] = acc[o] + wt * y[j][o]
        s = s + wt
    return [a / s for a in acc]


@pytest.mark.parametrize("k", [1, 2, 5, 33])
@pytest.mark.parametrize("distance", [False, True])
def test_reference_against_a_pure_python_loop(k, distance):
    rng = np.random.default_rng(1000 + k)
    n, nq, n_classes = 60, 50, 4
    idx = np.stack([rng.permutation(n)[:k] for _ in range(nq)]).astype(np.uint64)
    dist = np.sort(rng.uniform(0.1, 2.0, (nq, k)).astype(np.float32), axis=1)
    dist[3, 0] = 0.0                      # planted zero distances: one, and (k permitting) two
    dist[4, :min(k, 2)] = 0.0
    dist[5, 0] = -1e-7                    # a negative distance counts as zero
    dist[6, -1] = np.nan                  # a NaN poisons the list
    labels = rng.integers(0, n_classes, n).astype(np.int64)
    labels[int(idx[7, 0])] = n_classes    # a label out of range poisons the lists that gather it
    y = rng.standard_normal((n, 3))
    pred, proba = ref.classify(idx, dist, labels, n_classes, distance)
    out = ref.regress(idx, dist, y, distance)
    assert pred.dtype == np.int64 and proba.shape == (nq, n_classes) and out.shape == (nq, 3)
    assert pred[6] == -1 and np.isnan(proba[6]).all() and np.isnan(out[6]).all()
    assert pred[7] == -1 and np.isnan(proba[7]).all() and not np.isnan(out[7]).any()
    for q in range(nq):
        il, dl = [int(j) for j in idx[q]], [float(d) for d in dist[q]]
        p, pr = _python_classify(il, dl, labels.tolist(), n_classes, distance)
        assert pred[q] == p, q
        ref.same_bits(proba[q], np.array(pr, dtype=np.float64), f"proba of list {q}")
        ref.same_bits(out[q], np.array(_python_regress(il, dl, y.tolist(), distance), dtype=np.float64), f"mean of list {q}")
    if distance and pred[3] >= 0:  # (list 3 may have drawn the row with the bad label)
        assert proba[3].max() == 1.0 and sorted(proba[3])[-2] == 0.0  # only the zero-distance entry counts


def test_hand_derived_case():
    rows = np.array([[0.0], [1.0], [2.0], [3.0]])
    labels = np.array([0, 0, 1, 1], dtype=np.int64)

    def lists(q):
        d = np.abs(rows[:, 0] - q)
        order = np.lexsort((np.arange(4), d))[:3]
        return order[None, :].astype(np.uint64), d[order][None, :]

    idx, dist = lists(1.1)  # rows 1, 2, 0: classes 0, 1, 0
    assert idx.tolist() == [[1, 2, 0]]
    for distance in (False, True):
        assert ref.classify(idx, dist, labels, 2, distance)[0].tolist() == [0]
    idx, dist = lists(0.9)  # rows 1, 0, 2: classes 0, 0, 1
    assert idx.tolist() == [[1, 0, 2]]
    pred, proba = ref.classify(idx, dist, labels, 2, False)
    assert pred.tolist() == [0]
    ref.same_bits(proba, np.array([[2.0 / 3.0, 1.0 / 3.0]]), "uniform proba")
    ref.same_bits(ref.regress(idx, dist, np.array([10.0, 20.0, 60.0, 0.0]), False), np.array([[90.0 / 3.0]]), "uniform mean")
