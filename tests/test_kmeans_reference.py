"""The numpy restatement of the k-means contract (tests/kmeans_reference.py) on cases computed by hand: it is the
oracle of the GPU tests, so it is checked on its own first.  No GPU."""
import numpy as np
import pytest

import kmeans_reference as ref


def test_three_rows_by_hand():
    X = np.array([[0, 0], [0, 2], [10, 0]], dtype=np.float32)
    C = np.array([[0, 1], [9, 0]], dtype=np.float32)
    labels, dist = ref.assign(X, C)
    assert labels.tolist() == [0, 0, 1] and dist.tolist() == [1.0, 1.0, 1.0]
    assert ref.inertia(labels, dist) == 3.0
    new, shift2 = ref.update(X, C, labels)
    assert new.tolist() == [[0, 1], [10, 0]] and shift2 == 1.0
    # one iteration moves centre 1 by 1 (shift2 = 1), the second moves nothing: stop at t = 2 with tol = 0
    c, lab, d, counts, inertia, it, s2 = ref.kmeans(X, C, 0.0, 10)
    assert c.tolist() == [[0, 1], [10, 0]] and lab.tolist() == [0, 0, 1] and d.tolist() == [1.0, 1.0, 0.0]
    assert counts.tolist() == [2, 1] and counts.dtype == np.uint64 and inertia == 2.0 and it == 2 and s2 == 0.0
    # a tolerance the first move meets, and max_iter = 1, stop after one update; the labels belong to the centres returned
    for tol, mi in ((1.0, 10), (0.0, 1)):
        c, lab, d, counts, inertia, it, s2 = ref.kmeans(X, C, tol, mi)
        assert it == 1 and s2 == 1.0 and c.tolist() == [[0, 1], [10, 0]] and d.tolist() == [1.0, 1.0, 0.0]


def test_exact_tie_goes_to_the_lower_number():
    X = np.array([[1, 0], [0, 0]], dtype=np.float64)
    C = np.array([[2, 0], [0, 0], [0, 0], [2, 0]], dtype=np.float64)
    labels, dist = ref.assign(X, C)
    assert labels.tolist() == [0, 1] and dist.tolist() == [1.0, 0.0]


def test_empty_cluster_keeps_its_centre_and_nan_rows_go_to_centre_zero():
    X = np.array([[0.0], [1.0], [2.0]], dtype=np.float32)
    C = np.array([[1.0], [100.0]], dtype=np.float32)
    c, lab, d, counts, inertia, it, s2 = ref.kmeans(X, C, 0.0, 5)
    assert c.tolist() == [[1.0], [100.0]] and lab.tolist() == [0, 0, 0] and counts.tolist() == [3, 0]
    assert it == 1 and s2 == 0.0 and inertia == 2.0
    # a NaN distance is the key above +inf: it still beats "no centre", so the row belongs to centre 0
    Xn = np.array([[np.nan], [1.0]], dtype=np.float32)
    lab, d = ref.assign(Xn, C)
    assert lab.tolist() == [0, 0] and np.isnan(d[0]) and d[1] == 0.0
    assert np.isnan(ref.inertia(lab, d))
    # no centres: every label -1, every distance NaN, and such rows add nothing
    lab, d = ref.assign(X, C[:0])
    assert lab.tolist() == [-1, -1, -1] and np.all(np.isnan(d)) and ref.inertia(lab, d) == 0.0


def test_sum4096_shape():
    # the shape is visible where rounding bites: 2^53 absorbs a 1.0 added to it, but not two of them added first
    big = 2.0 ** 53
    t = np.zeros(130)
    t[0], t[64], t[128] = big, 1.0, 1.0  # all three in lane 0: ((big + 1) + 1) = big
    assert ref.sum4096(t) == big
    t = np.zeros(130)
    t[0], t[1], t[2] = big, 1.0, 1.0  # lanes 0, 1, 2: ((big + 1) + 1) = big as well, in lane order
    assert ref.sum4096(t) == big
    t = np.zeros(130)
    t[1], t[65], t[0] = 1.0, 1.0, big  # lane 1 holds 2.0 first: big + 2 is exact
    assert ref.sum4096(t) == big + 2.0
    # segments: 4096 terms each, folded in order after the lanes
    t = np.zeros(2 * 4096 + 1)
    t[0], t[4096], t[8192] = big, 1.0, 1.0  # ((big + 1) + 1) over three segments
    assert ref.sum4096(t) == big
    t[0], t[4096], t[4097] = big, 1.0, 1.0  # the second segment sums to 2 first
    t[8192] = 0.0
    assert ref.sum4096(t) == big + 2.0
    assert ref.sum4096(np.zeros(0)) == 0.0
    rng = np.random.default_rng(3)
    M = rng.standard_normal((9000, 3))
    cols = ref.sum4096_columns(M)
    assert [ref.sum4096(M[:, j]) for j in range(3)] == cols.tolist()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(300, 17, 40), (65, 1, 3), (7, 33, 1)])
def test_the_vectorised_fold_is_the_fold_bit_for_bit(shape, dtype):
    """fold_matrix / assign_matrix (the want side of the many-centre tests) against fold_distances / assign, by their bits
    (NaN payloads included: the operations are the same ones), with a NaN row, an inf row and a duplicated centre"""
    n, dim, nc = shape
    rng = np.random.default_rng(17 * n + dim)
    X = (rng.standard_normal((n, dim)) * 10.0 ** rng.integers(-3, 4, (n, 1))).astype(dtype)
    C = (rng.standard_normal((nc, dim)) * 3.0).astype(dtype)
    if dtype == np.float64:
        X, C = X * (1.0 + 2.0 ** -30), C * (1.0 - 2.0 ** -31)  # (low bits an f32 cannot hold)
    X[1, dim // 2] = np.nan
    X[2, 0] = np.inf
    X[3, dim - 1] = -np.inf
    if nc >= 3:
        C[nc - 1] = C[1]  # a duplicated centre: the lower number wins
        X[4] = C[1]       # ... at distance 0, too
    M = ref.fold_matrix(X, C)
    assert M.shape == (n, nc) and M.dtype == dtype
    for c in range(nc):
        assert _bits(M[:, c]) == _bits(ref.fold_distances(X, C[c])), c
    wl, wd = ref.assign(X, C)
    gl, gd = ref.assign_matrix(X, C)
    assert gl.dtype == wl.dtype and np.array_equal(gl, wl) and gd.dtype == wd.dtype and _bits(gd) == _bits(wd)
    assert wl[1] == 0 and np.isnan(wd[1]) and np.isinf(wd[2]) and np.isinf(wd[3])
    if nc >= 3:
        assert wl[4] == 1 and wd[4] == 0 and (wl != nc - 1).all()
    # the loop over either assignment (NaN rows make centre 0 NaN after the first update: NaN payloads are not compared)
    a, b = ref.kmeans(X, C, 0.0, 3), ref.kmeans(X, C, 0.0, 3, assign=ref.assign_matrix)
    for u, v in zip(a, b):
        u, v = np.atleast_1d(np.asarray(u)), np.atleast_1d(np.asarray(v))
        assert u.dtype == v.dtype and u.shape == v.shape
        nan = np.isnan(u) if u.dtype.kind == "f" else np.zeros(u.shape, dtype=bool)
        assert np.array_equal(nan, np.isnan(v) if v.dtype.kind == "f" else nan) and _bits(u[~nan]) == _bits(v[~nan])
    good = np.isfinite(X).all(axis=1)
    a, b = ref.kmeans(X[good], C, 0.0, 3), ref.kmeans(X[good], C, 0.0, 3, assign=ref.assign_matrix)
    assert all(_bits(u) == _bits(v) for u, v in zip(a, b)) and np.isfinite(a[0]).all() and a[5] >= 2
    # no centres
    gl, gd = ref.assign_matrix(X, C[:0])
    wl, wd = ref.assign(X, C[:0])
    assert np.array_equal(gl, wl) and gd.dtype == wd.dtype and np.all(np.isnan(gd))


def test_fold_is_sequential_in_the_rows_type():
    # f32: 2^24 + 1 + 1 stays 2^24 when the ones arrive one by one
    X = np.zeros((1, 3), dtype=np.float32)
    c = np.array([4096.0, 1.0, 1.0], dtype=np.float32)
    assert ref.fold_distances(X, c)[0] == np.float32(4096.0)
    assert ref.fold_distances(X.astype(np.float64), c.astype(np.float64))[0] == np.sqrt(np.float64(2.0 ** 24 + 2))
