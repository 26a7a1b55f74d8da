"""pn_silhouette_*: silhouette values on the device against f64 brute force over the tree's own inputs.

The bound (2 D + 12) u is derived, not measured: the sequential fold is accurate to (D / 2 + 2) u relative, the f64 sums
add nothing visible, and (b - a) / max(a, b) at most triples it.  u = 2^-24 for f32 trees; for f64 trees the reference
runs in the same precision, so u = 2^-52.  One lost or doubled pair in a 64-member cluster moves s by about 1e-2.
The spans are 8192 sorted positions long at these sizes (sil_span_len): case f crosses one span boundary.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (np.float32, 2.0 ** -24), "f64": (np.float64, 2.0 ** -52)}


def _case(name, dtype):
    """``(X, codes, n_clusters)``: each the smallest shape that exercises what the issue names for it"""
    rng = np.random.default_rng(sum(map(ord, name)))
    n, dim, sizes = 300, 5, None
    if name == "a":      # n no multiple of a row or column tile, D below one K-chunk
        dim, sizes = 3, [70, 80, 90, 60]
    elif name == "b":    # D no multiple of the K-chunk
        dim, sizes = 33, [70, 80, 90, 60]
    elif name == "c":    # singleton, pair, boundaries on and off a column tile; interleaved, so the sort matters
        sizes = [1, 2, 63, 64, 65, 105]
    elif name == "d":    # duplicates: zero distances, and two clusters that are copies of ONE point (max(a, b) = 0 there)
        sizes = [100, 100, 91, 5, 4]
    elif name == "e":    # a fifth excluded, code 2 unused
        sizes = [80, 80, 0, 80, 60]
    elif name == "f":    # the largest cluster crosses the span boundary at 8192
        n, dim, sizes = 9000, 8, [2500, 6000, 500]
    elif name == "f_many":  # about n / 3 clusters: many per tile, some empty, some singletons
        n, dim = 9000, 8
    if sizes is None:
        codes = rng.integers(0, n // 3, n)
        nc = n // 3
    else:
        codes = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
        nc = len(sizes)
    X = rng.random((n, dim)).astype(dtype)
    if name == "d":
        X[np.flatnonzero(codes == 0)[:3]] = X[np.flatnonzero(codes == 0)[0]]
        X[codes >= 3] = X[np.flatnonzero(codes == 3)[0]]
    if name == "e":
        codes[rng.permutation(n)[:n // 5]] = -1
    return X, codes.astype(np.int64), nc


def _reference(X, codes, nc):
    """``(s, a, b, nearest, gap)`` in f64; gap: the relative distance between the two smallest means"""
    np.seterr(all="ignore")  # (0 / 0 where both best means are zero: the gap is then NaN and compares false)
    X, n = X.astype(np.float64), len(X)
    mem = np.flatnonzero(codes >= 0)
    mem = mem[np.argsort(codes[mem], kind="stable")]
    present, starts, cnt = np.unique(codes[mem], return_index=True, return_counts=True)
    s, a, b, gap = (np.full(n, np.nan) for _ in range(4))
    near = np.full(n, -1, dtype=np.int64)
    for r0 in range(0, n, 512):
        r = np.arange(r0, min(r0 + 512, n))
        r = r[codes[r] >= 0]
        d2 = np.zeros((len(r), len(mem)))
        for k in range(X.shape[1]):
            d2 += (X[r, k, None] - X[None, mem, k]) ** 2
        S = np.add.reduceat(np.sqrt(d2).astype(np.longdouble), starts, axis=1)  # (6000 terms: the sums' own rounding out)
        i, own = np.arange(len(r)), np.searchsorted(present, codes[r])
        na = cnt[own]
        a[r] = np.where(na > 1, S[i, own] / np.maximum(na - 1, 1), 0.0)
        means = (S / cnt).astype(np.float64)
        means[i, own] = np.inf
        two = np.partition(means, 1, axis=1)[:, :2]
        b[r], near[r] = two[:, 0], present[np.argmin(means, axis=1)]
        gap[r] = (two[:, 1] - two[:, 0]) / two[:, 1]
        mx = np.maximum(a[r], b[r])
        s[r] = np.where((na == 1) | (mx == 0), 0.0, (b[r] - a[r]) / np.where(mx == 0, 1.0, mx))
    return s, a, b, near, gap


_CACHE = {}


def _setup(pn, name, sfx):
    if (name, sfx) not in _CACHE:
        X, codes, nc = _case(name, DTYPES[sfx][0])
        _CACHE[name, sfx] = (X, codes, nc, _reference(X, codes, nc))
    X, codes, nc, ref = _CACHE[name, sfx]
    return pn.BallTree.euclidean(X), codes, nc, ref


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _raw(tree, codes, nc, rows=None):
    """the host entry itself: ``(samples, a, b, nearest, score, n_scored)``"""
    from petal_neighbors_amd.errors import check
    m = len(codes) if rows is None else len(rows)
    s, a, b = (np.empty(m) for _ in range(3))
    near = np.empty(m, dtype=np.int64)
    score, scored = C.c_double(0.0), C.c_uint64(0)
    check(tree._fn("silhouette")(tree._h, codes.ctypes.data, nc, None if rows is None else rows.ctypes.data,
                                 0 if rows is None else m, 0, s.ctypes.data, a.ctypes.data, b.ctypes.data, near.ctypes.data,
                                 C.byref(score), C.byref(scored)))
    return s, a, b, near, score.value, scored.value


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f", "f_many"])
def test_silhouette_against_brute_force(pn, name, sfx):
    import torch
    tree, codes, nc, (rs, ra, rb, rnear, gap) = _setup(pn, name, sfx)
    n, bound = len(codes), (2 * tree.dim + 12) * DTYPES[sfx][1]
    s, a, b, near, score, scored = _raw(tree, codes, nc)
    ok = codes >= 0
    err = {"s": np.abs(s - rs)[ok].max(), "a": (np.abs(a - ra)[ok] / np.maximum(ra[ok], 1e-300)).max(),
           "b": (np.abs(b - rb)[ok] / np.maximum(rb[ok], 1e-300)).max(), "score": abs(score - rs[ok].mean())}
    print(name, sfx, "bound", bound, err)
    assert scored == ok.sum() and np.isnan(s[~ok]).all() and np.isnan(a[~ok]).all() and (near[~ok] == -1).all()
    assert all(v <= bound for v in err.values()), (err, bound)
    clear = ok & (gap > bound)
    assert np.array_equal(near[clear], rnear[clear]) and clear.sum() > ok.sum() // 2
    if name == "c":
        assert (s[codes == 0] == 0).all() and (a[codes == 0] == 0).all()  # the singleton
        i, j = np.flatnonzero(codes == 1)  # the pair: a is one distance, with the bits of pairwise
        assert a[i] == a[j] == np.float64(pn.distance.pairwise(tree.points)[i, j])
    if name == "d":
        assert (s[codes >= 3] == 0).all() and (a[codes >= 3] == 0).all() and (b[codes >= 3] == 0).all()  # copies of one point
        # clusters 3 and 4 are the same point.  f32: 4 d and 5 d are exact in f64, so the means are equal and the lower
        # number wins (f64: 5 d rounds, the means may differ in the last bit)
        tie = (codes < 3) & (rnear >= 3)
        assert tie.any() and (sfx == "f64" or (near[tie] == 3).all())
    # bit equality: a second call, the device entry, and an unsorted subset of the rows
    again = _raw(tree, codes, nc)
    dev = tree.silhouette_device(torch.from_numpy(codes).cuda(), nc)
    rows = np.arange(0, n, 7, dtype=np.uint64)[::-1].copy()
    sub = _raw(tree, codes, nc, rows)
    sub_dev = tree.silhouette_device(torch.from_numpy(codes).cuda(), nc, rows=torch.from_numpy(rows.astype(np.int64)).cuda())
    torch.cuda.synchronize()
    assert int(dev[6].item()) == 0 and int(sub_dev[6].item()) == 0
    full = (s, a, b, near, np.float64(score), np.int64(scored))
    idx = rows.astype(np.int64)
    for k, what in enumerate(("s", "a", "b", "nearest", "score", "n_scored")):
        assert np.array_equal(_bits(again[k]), _bits(full[k])), what + ": two calls"
        assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(full[k])), what + ": host and device"
        if k < 4:
            assert np.array_equal(_bits(sub[k]), _bits(full[k][idx])), what + ": subset"
            assert np.array_equal(_bits(sub_dev[k].cpu().numpy()), _bits(full[k][idx])), what + ": subset, device"
    assert sub[5] == ok[idx].sum() and abs(sub[4] - rs[idx][ok[idx]].mean()) <= bound


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_silhouette_error_paths(pn, sfx):
    import torch
    from petal_neighbors_amd import _lib
    from petal_neighbors_amd.errors import PetalError
    tree, codes, nc, _ = _setup(pn, "a", sfx)
    n = len(codes)
    bad = {"a code >= n_clusters": (np.where(np.arange(n) == 17, nc, codes), None),
           "one non-empty cluster": (np.zeros(n, dtype=np.int64), None),
           "a row >= n": (codes, np.array([3, n, 5], dtype=np.uint64))}
    for what, (c, rows) in bad.items():
        with pytest.raises(PetalError) as e:
            _raw(tree, np.ascontiguousarray(c, dtype=np.int64), nc, rows)
        assert e.value.code == _lib.PN_ERR_INVALID, what
        drows = None if rows is None else torch.from_numpy(rows.astype(np.int64)).cuda()
        out = tree.silhouette_device(torch.from_numpy(np.ascontiguousarray(c, dtype=np.int64)).cuda(), nc, rows=drows)
        assert int(out[6].item()) == _lib.PN_ERR_INVALID, what
    assert int(tree.silhouette_device(torch.from_numpy(codes).cuda(), nc)[6].item()) == 0  # (the word is rewritten per call)
    cos = pn.BallTree.new(tree.points, pn.distance.Cosine())
    with pytest.raises(PetalError) as e:
        _raw(cos, codes, nc)
    assert e.value.code == _lib.PN_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        cos.silhouette_samples(codes)


def test_python_wrappers_map_labels(pn):
    tree, codes, nc, (rs, ra, rb, rnear, _) = _setup(pn, "e", "f32")
    labels = np.where(codes < 0, "noise", np.array(["p", "q", "r", "t", "u"])[codes])
    s, a, b, near = tree.silhouette_samples(labels, ignore="noise", full=True)
    want = _raw(tree, np.where(codes > 2, codes - 1, codes), nc - 1)  # (np.unique closes the gap of the unused code)
    ok = codes >= 0
    assert np.array_equal(_bits(s), _bits(want[0])) and np.array_equal(_bits(a), _bits(want[1]))
    assert np.array_equal(near[ok], np.array(["p", "q", "t", "u"])[want[3][ok]]) and (near[~ok] == "noise").all()
    assert tree.silhouette_score(labels, ignore="noise") == want[4]
    rows = np.array([9, 2, 250])
    assert np.array_equal(_bits(tree.silhouette_samples(labels, rows=rows, ignore="noise")), _bits(s[rows]))
