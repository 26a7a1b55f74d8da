"""Greedy k-means++ seeding on an MI355X (petal-neighbors_amd/csrc/kmeans_init.hip) against a numpy float64 restatement
of its contract (include/petal_mi355x.h, pn_kmeans_init_*): the chosen rows and the centres must be the reference's, row
number for row number and bit for bit.

The reference asserts, on the CPU and for every case below, that a round's winner is never decided by a tie between two
different rows (the same row drawn twice ties with itself, which changes nothing): the inputs were chosen so, and the
assertion runs with the tests."""
import math

import numpy as np
import pytest

import kmeans_reference as ref
from conftest import uniform

pytestmark = pytest.mark.gpu

FAMILIES = {
    "offset1000": lambda n, d, s: uniform((n, d), s) + np.float32(1000.0),
    "mixed_scales": lambda n, d, s: ((uniform((n, d), s) - np.float32(0.5))
                                      * (np.float32(10.0) ** (np.arange(d, dtype=np.float32) % 9 - 4))).astype(np.float32),
}


def _rows(family, n, d, seed, dtype):
    x = FAMILIES[family](n, d, seed).astype(dtype)
    if dtype == np.float64:  # low bits an f32 cannot hold, so that the f64 fold is really exercised
        x = x * (1.0 + 2.0 ** -30)
    return np.ascontiguousarray(x)


def _halve(a):
    """the halving tree along the last axis of [.., 256]"""
    h = a.shape[-1] // 2
    while h:
        a = a[..., :h] + a[..., h:]
        h //= 2
    return a[..., 0]


def _tree256(t):
    """(total, group sums, block sums) of the float64 terms t"""
    nb = -(-len(t) // 256)
    bs = _halve(np.concatenate([t, np.zeros(nb * 256 - len(t))]).reshape(nb, 256))
    ng = -(-nb // 256)
    gs = _halve(np.concatenate([bs, np.zeros(ng * 256 - nb)]).reshape(ng, 256))
    total = gs[0]
    for g in gs[1:]:
        total = total + g
    return total, gs, bs


def _walk(s, r):
    """one level of a pick: (entry, what is carried into it)"""
    cs = np.cumsum(s)  # (sequential)
    hit = np.flatnonzero(cs > r)
    i = int(hit[0]) if len(hit) else int(np.flatnonzero(s != 0)[-1])
    return i, r - (cs[i - 1] if i else 0.0)


def _term(e):
    w = e.astype(np.float64) * e.astype(np.float64)
    return np.where(np.isnan(w), 0.0, w)


def _kmin(m, d):
    return np.where(ref._keys(d) < ref._keys(m), d, m)


def reference(X, nc, trials, seed):
    import oracle
    n = len(X)
    L = trials or min(2 + int(math.log(nc)), 16)
    u = oracle.fill_uniform(1 + (nc - 1) * L, seed).astype(np.float64)
    rows = [int(u[0] * n)]
    m = ref.fold_distances(X, X[rows[0]])
    for t in range(1, nc):
        w = _term(m)
        total, gs, bs = _tree256(w)
        assert total > 0
        cands = []
        for c in range(L):
            g, r = _walk(gs, u[1 + (t - 1) * L + c] * total)
            b, r = _walk(bs[g * 256:(g + 1) * 256], r)
            i, _ = _walk(w[(g * 256 + b) * 256:][:256], r)
            cands.append((g * 256 + b) * 256 + i)
        D = [ref.fold_distances(X, X[c]) for c in cands]
        pots = [_tree256(_term(_kmin(m, d)))[0] for d in D]
        best = int(np.argmin(pots))  # (the first minimum: a strict '<' in trial order)
        assert all(cands[c] == cands[best] for c in range(L) if pots[c] == pots[best]), "a tie between two rows"
        m = _kmin(m, D[best])
        rows.append(cands[best])
    return X[rows], np.asarray(rows, dtype=np.uint64)


def _check(pn, X, nc, trials, seed):
    wc, wr = reference(X, nc, trials, seed)
    tree = pn.BallTree.euclidean(X)
    centres, rows = tree.kmeans_init(nc, seed, trials or None)
    assert np.array_equal(rows, wr), (rows, wr)
    assert centres.tobytes() == wc.tobytes()
    return tree, centres, rows


# a partial block, one block, two blocks; one group to the row, and two groups (where the group walk can go wrong)
@pytest.mark.parametrize("n", [255, 256, 257, 65536, 65537])
@pytest.mark.parametrize("trials,nc", [(1, 6), (0, 2), (0, 20), (16, 4)])  # L = 1, 2, 4, 16
def test_rows_and_trials(pn, n, trials, nc):
    _check(pn, _rows("mixed_scales", n, 33, n + nc, np.float32), nc, trials, seed=n + trials)


# the K-chunk edges (32 columns for f32, 16 for f64), on weights where the prefix walks are sensitive
@pytest.mark.parametrize("family", ["offset1000", "mixed_scales"])
@pytest.mark.parametrize("dim,dtype", [(1, np.float32), (31, np.float32), (32, np.float32), (33, np.float32),
                                       (100, np.float32), (15, np.float64), (17, np.float64)])
def test_chunk_edges(pn, family, dim, dtype):
    _check(pn, _rows(family, 65537 if dim in (33, 17) else 257, dim, 7 * dim, dtype), 5, 3, seed=dim)


def test_fewer_distinct_rows_than_centres(pn):
    from petal_neighbors_amd import _lib
    from petal_neighbors_amd.errors import PetalError
    vals = _rows("mixed_scales", 7, 5, 3, np.float32)
    X = np.ascontiguousarray(vals[np.arange(300) % 7])
    # (one trial per round: two copies of a point would tie as candidates, and with one candidate nothing is compared)
    tree, centres, rows = _check(pn, X, 7, 1, seed=1)
    assert len({c.tobytes() for c in centres}) == 7 and len(set(rows.tolist())) == 7
    with pytest.raises(PetalError) as e:
        tree.kmeans_init(8, 1, 1)
    assert e.value.code == _lib.PN_ERR_INVALID and "distinct" in str(e.value)


def test_other_ways_in_give_the_same_answer(pn):
    import torch
    X = _rows("mixed_scales", 1000, 20, 11, np.float32)
    tree, centres, rows = _check(pn, X, 12, 0, seed=5)
    dtree = pn.BallTree.from_device(torch.from_numpy(X).cuda())
    dc, dr = dtree.kmeans_init(12, 5)
    assert dc.tobytes() == centres.tobytes() and np.array_equal(dr, rows)
    a = tree.kmeans_init_device(12, 5)  # twice on one stream: the second call's workspace is the first's
    b = tree.kmeans_init_device(12, 5)
    for c, r in (a, b):
        assert c.cpu().numpy().tobytes() == centres.tobytes() and np.array_equal(r.cpu().numpy().astype(np.uint64), rows)
    tree.set_engine("exact")
    ec, er = tree.kmeans_init(12, 5)
    assert ec.tobytes() == centres.tobytes() and np.array_equal(er, rows)
    tree.set_engine("auto")
    got = tree.kmeans(12, seed=5, init="device", full=True)
    want = tree.kmeans(centres, full=True)
    for g, w in zip(got, want):
        assert np.asarray(g).tobytes() == np.asarray(w).tobytes()
