"""Spherical k-means on an MI355X (petal-neighbors_amd/csrc/spherical_kmeans.hip) against a numpy restatement of its
contract (include/petal_mi355x.h, pn_spherical_kmeans_*): Cosine::distance as the sequential fold in the index's type, the
signed (key, centre number) order, the f64 update.  Every comparison is bit for bit, under the three engines and with the
filter forced (PN_OPT_KMEANS_FILTER = 1); the filter takes 8 <= dim <= 304, four waves per workgroup up to 192 padded
columns and two beyond."""
import numpy as np
import pytest

from conftest import uniform
from kmeans_reference import sum4096, sum4096_columns

pytestmark = pytest.mark.gpu

MODES = ["auto", "exact", "bf16", "forced"]
FILTER_MAX_DIM = 304


def _as(x, dtype):
    x = x.astype(dtype)
    if dtype == np.float64:  # low bits an f32 cannot hold, so that the f64 fold is really exercised
        x = x * (1.0 + 2.0 ** -30)
    return np.ascontiguousarray(x)


def _same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(na, nb) and \
        np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


def _norms(X):
    s = np.zeros(X.shape[0], dtype=X.dtype)
    with np.errstate(all="ignore"):
        for k in range(X.shape[1]):
            s = (s + (X[:, k] * X[:, k]).astype(X.dtype)).astype(X.dtype)
        return np.sqrt(s).astype(X.dtype)


def _cosine_matrix(X, C):
    """Cosine::distance of every (row, centre) in X's type: the sequential unfused dot, 1 - dot / (norm_c * norm_row)"""
    dt = X.dtype
    C = np.asarray(C, dtype=dt)
    dot = np.zeros((X.shape[0], C.shape[0]), dtype=dt)
    with np.errstate(all="ignore"):
        for k in range(X.shape[1]):
            dot = (dot + (C[None, :, k] * X[:, k, None]).astype(dt)).astype(dt)
        den = (_norms(C)[None, :] * _norms(X)[:, None]).astype(dt)
        return (dt.type(1) - (dot / den).astype(dt)).astype(dt)


def _keys(d):
    """the signed order-preserving keys: -0 as +0, NaN the canonical key above +inf"""
    u = np.uint32 if d.dtype == np.float32 else np.uint64
    bits = np.where(d == 0, d.dtype.type(0), d).view(u)
    sign = u(1) << u(8 * d.itemsize - 1)
    k = np.where(bits & sign, ~bits, bits | sign)
    return np.where(np.isnan(d), ~u(0) << u(22 if u is np.uint32 else 51), k)


def _want(D, n, nc):
    """labels and distances from the distance matrix: the first least key; a NaN key makes a member of nothing"""
    if nc == 0:
        return np.full(n, -1, dtype=np.int64), np.full(n, np.nan, dtype=D.dtype)
    d = D[:n, :nc]
    lab = np.argmin(_keys(d), axis=1).astype(np.int64)
    dist = d[np.arange(n), lab]
    return np.where(np.isnan(dist), -1, lab), dist


def _inertia(lab, dist):
    return sum4096(np.where(lab < 0, 0.0, dist.astype(np.float64)))


def _set_mode(tree, mode):
    from petal_neighbors_amd import _lib
    from petal_neighbors_amd.errors import PetalError
    tree.set_option(_lib.PN_OPT_KMEANS_FILTER, 1 if mode == "forced" else 0)
    try:
        tree.set_engine("auto" if mode == "forced" else mode)
    except PetalError:
        assert mode == "bf16" and not tree.bf16_eligible
        return False
    return True


def _check_assign(pn, X, C, want=None):
    """every mode's labels, distances and inertia equal the reference's; returns the rows the filter listed"""
    wl, wd = want if want is not None else _want(_cosine_matrix(X, C), X.shape[0], C.shape[0])
    wi = _inertia(wl, wd)
    tree = pn.BallTree.new(X, pn.distance.Cosine())
    listed = None
    for mode in MODES:
        if not _set_mode(tree, mode):
            continue
        before = tree.stats()
        labels, dist, inertia = tree.spherical_kmeans_assign(C)
        after = tree.stats()
        assert np.array_equal(labels, wl), f"{mode}: labels differ at rows {np.flatnonzero(labels != wl)[:8]}"
        assert _same_bits(dist, wd), f"{mode}: distances differ"
        assert _same_bits(np.float64(inertia), wi), f"{mode}: inertia {inertia!r} != {wi!r}"
        assert after["queries"] - before["queries"] == X.shape[0]
        added = after["fallback_queries"] - before["fallback_queries"]
        if 8 <= X.shape[1] <= FILTER_MAX_DIM and C.shape[0] >= 2 and mode in ("bf16", "forced"):
            assert listed is None or listed == added, "the listed rows do not depend on how the filter was chosen"
            listed = added
        else:  # (the exact kernel alone)
            assert added == 0
    return listed


SHAPES = [(1, 1), (63, 31), (64, 32), (65, 33), (127, 65), (128, 33), (129, 65), (129, 1), (64, 65)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dim", [7, 8, 9, 17, 128, 129, 256, FILTER_MAX_DIM, FILTER_MAX_DIM + 1])
def test_assignment_bit_for_bit_at_the_tile_edges(pn, dim, dtype):
    X = _as(uniform((129, dim), 100 + dim) - np.float32(0.5), dtype)  # cosines of both signs
    C = _as(uniform((65, dim), 200 + dim) - np.float32(0.5), dtype)
    D = _cosine_matrix(X, C)
    for n, nc in SHAPES:
        _check_assign(pn, X[:n].copy(), C[:nc].copy(), _want(D, n, nc))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dim", [33, 128])
def test_order_and_ties(pn, dim, dtype):
    X = _as(uniform((200, dim), 7) - np.float32(0.5), dtype)
    C = _as(uniform((6, dim), 8) - np.float32(0.5), dtype)
    # twin centres: the lower number wins, and no row can be proven -- the forced filter lists them all, EXACT none
    twins = np.concatenate([C, C])
    assert _check_assign(pn, X, twins) == X.shape[0]
    assert _want(_cosine_matrix(X, twins), 200, 12)[0].max() < 6
    # a centre and three times that centre; rows parallel to a centre (distances a few ulp either side of 0); rows
    # within 1e-7 of the bisector of two centres
    _check_assign(pn, X, np.concatenate([C, C[:1] * dtype(3)]))
    scales = (dtype(0.25) + np.arange(200, dtype=dtype) / dtype(64))[:, None]
    par = np.ascontiguousarray(C[np.arange(200) % 6] * scales)
    assert (np.abs(_cosine_matrix(par, C)).min(axis=1) <= (2 * dim + 16) * np.finfo(dtype).eps).all()
    _check_assign(pn, par, C)
    unit = C.astype(np.float64) / np.linalg.norm(C.astype(np.float64), axis=1)[:, None]
    bis = unit[np.arange(200) % 6] + unit[(np.arange(200) + 1) % 6] + 1e-7 * (X.astype(np.float64))
    _check_assign(pn, np.ascontiguousarray(bis.astype(dtype)), C)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rows_and_centres_without_a_direction(pn, dtype):
    X = _as(uniform((150, 40), 11) - np.float32(0.5), dtype)
    C = _as(uniform((9, 40), 12) - np.float32(0.5), dtype)
    X[3] = 0
    X[70, 5] = np.nan
    X[100] *= dtype(2.0 ** 60)
    X[101] *= dtype(2.0 ** -60)
    lab, dist = _want(_cosine_matrix(X, C), 150, 9)
    assert lab[3] == -1 and lab[70] == -1 and np.isnan(dist[[3, 70]]).all() and lab[100] >= 0 and (lab >= 0).sum() >= 147
    _check_assign(pn, X, C, (lab, dist))
    C[4] = 0  # a zero centre is never chosen, and the call is answered alike under every mode
    lab, dist = _want(_cosine_matrix(X, C), 150, 9)
    assert not (lab == 4).any()
    _check_assign(pn, X, C, (lab, dist))
    _check_assign(pn, X, C[:0])  # no centres


def test_the_filter_proves_separated_rows(pn):
    n, dim = 2048, 64
    noise = uniform((n, dim), 21) - np.float32(0.5)
    noise *= np.float32(0.05) / np.linalg.norm(noise, axis=1)[:, None].astype(np.float32)
    X = noise.copy()
    X[np.arange(n), np.arange(n) % 8] += np.float32(1)
    C = np.eye(64, dtype=np.float32)  # the 8 axes, then 56 directions orthogonal to them
    listed = _check_assign(pn, np.ascontiguousarray(X), C)
    assert listed is not None and listed <= n // 4, listed


def _update(X, rn, C, labels):
    new = C.copy()
    shift2 = np.float64(0.0)
    with np.errstate(all="ignore"):
        for c in range(C.shape[0]):
            members = np.flatnonzero(labels == c)
            if len(members):
                S = sum4096_columns(X[members].astype(np.float64) / rn[members].astype(np.float64)[:, None])
                part = np.zeros(64)
                for col in range(len(S)):
                    part[col % 64] = part[col % 64] + S[col] * S[col]
                Q = part[0]
                for l in range(1, 64):
                    Q = Q + part[l]
                if Q > 0 and np.isfinite(Q):
                    new[c] = (S / np.sqrt(Q)).astype(X.dtype)
            t = (new[c].astype(np.float64) - C[c].astype(np.float64)) ** 2
            part = np.zeros(64)
            for col in range(len(t)):
                part[col % 64] = part[col % 64] + t[col]
            tc = part[0]
            for l in range(1, 64):
                tc = tc + part[l]
            shift2 = shift2 + tc
    return new, np.float64(shift2)


@pytest.mark.parametrize("dim,dtype", [(9, np.float32), (136, np.float32), (136, np.float64)])
def test_whole_loop_equals_the_reference(pn, dim, dtype):
    import torch
    n, max_iter = 3000, 3
    dirs = uniform((4, dim), 31) - np.float32(0.5)
    X = dirs[np.arange(n) % 4] * (np.float32(0.5) + uniform((n, 1), 32)) + np.float32(0.05) * (uniform((n, dim), 33) - np.float32(0.5))
    X = _as(X, dtype)
    init = _as(np.concatenate([X[[5, 6, 7, 8]] * np.float32(3), -dirs.sum(axis=0, keepdims=True)]), dtype)
    rn, C, t = _norms(X), init.copy(), 0
    while True:  # (the stop rule of pn_kmeans_*: shift2 <= tol or t == max_iter)
        t += 1
        lab, _ = _want(_cosine_matrix(X, C), n, 5)
        C, shift2 = _update(X, rn, C, lab)
        if shift2 <= 0.0 or t == max_iter:
            break
    lab, dist = _want(_cosine_matrix(X, C), n, 5)
    counts = np.bincount(lab, minlength=5).astype(np.uint64)
    assert counts[4] == 0 and _same_bits(C[4], init[4]) and (counts[:4] > 0).all()
    tree = pn.BallTree.new(X, pn.distance.Cosine())
    for mode in MODES:
        if not _set_mode(tree, mode):
            continue
        before = tree.stats()["queries"]
        got = tree.spherical_kmeans(init, tol=0.0, max_iter=max_iter, full=True)
        assert tree.stats()["queries"] - before == n * (t + 1)
        assert _same_bits(got[0], C) and np.array_equal(got[1], lab) and _same_bits(got[3], dist), mode
        assert _same_bits(np.float64(got[2]), _inertia(lab, dist)) and np.array_equal(got[4], counts), mode
        assert got[5] == t and _same_bits(np.float64(got[6]), shift2), mode
        dev = tree.spherical_kmeans_device(torch.from_numpy(init).cuda(), 0.0, max_iter)
        for a, b in zip(dev, (got[0], got[1], got[3], got[4].astype(np.int64), got[2], got[5], got[6])):
            assert _same_bits(a.cpu().numpy().reshape(np.shape(b)), np.asarray(b, dtype=a.cpu().numpy().dtype)), mode


def test_refusals(pn):
    from petal_neighbors_amd import _lib
    X = uniform((100, 16), 3)
    C = np.ascontiguousarray(X[:4])
    labels = np.empty(100, dtype=np.int64)
    tree = pn.BallTree.euclidean(X)
    code = tree._fn("spherical_kmeans_assign")(tree._h, C.ctypes.data, 4, 0, labels.ctypes.data, None, None)
    assert code == _lib.PN_ERR_UNSUPPORTED and "Cosine" in _lib.last_error()
    out = np.empty_like(C)
    code = tree._fn("spherical_kmeans")(tree._h, C.ctypes.data, 4, 0.0, 1, 0, out.ctypes.data, labels.ctypes.data, None, None,
                                        None, None, None)
    assert code == _lib.PN_ERR_UNSUPPORTED and "Cosine" in _lib.last_error()
    with pytest.raises(ValueError):
        pn.BallTree.new(X, pn.distance.Cosine()).kmeans_assign(C)
