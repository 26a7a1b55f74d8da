"""k-means on an MI355X (petal-neighbors_amd/csrc/kmeans.hip) against the numpy restatement of its contract
(tests/kmeans_reference.py) and against pn_mean_shift_labels_*, the exact path the library already had.

  * assignment, bit for bit, under the three engines and with the filter forced (PN_OPT_KMEANS_FILTER), f32 and f64, at
    the edges of the filter's tiles (128 rows per workgroup up to 256 columns and 64 beyond, 32 centres per MFMA tile, K in
    steps of 16 columns up to 320: D = 321 is the first the filter leaves to the exact kernel, D = 7 the last);
  * rows the proof must refuse, answered right all the same;
  * the filter really filters: on separated blobs the forced filter lists no row;
  * the bound L <= d^2, pair by pair;
  * whole k-means equal to the reference in every output, at the edges of the 4096-term segments.
"""
import numpy as np
import pytest

import kmeans_reference as ref
from conftest import uniform

pytestmark = pytest.mark.gpu

FAMILIES = {
    "uniform": lambda n, d, s: uniform((n, d), s),
    "offset1000": lambda n, d, s: uniform((n, d), s) + np.float32(1000.0),
    "scaled1e6": lambda n, d, s: (uniform((n, d), s) - np.float32(0.5)) * np.float32(1e6),
    "tiny1e-20": lambda n, d, s: (uniform((n, d), s) - np.float32(0.5)) * np.float32(1e-20),
    "sparse": lambda n, d, s: np.where(uniform((n, d), s + 7) < 0.9, np.float32(0), uniform((n, d), s)).astype(np.float32),
    "mixed_scales": lambda n, d, s: ((uniform((n, d), s) - np.float32(0.5))
                                      * (np.float32(10.0) ** (np.arange(d, dtype=np.float32) % 9 - 4))).astype(np.float32),
}


def _as(x, dtype):
    x = x.astype(dtype)
    if dtype == np.float64:  # low bits an f32 cannot hold, so that the f64 fold is really exercised
        x = x * (1.0 + 2.0 ** -30)
    return np.ascontiguousarray(x)


def _same_bits(a, b):
    """equal bit for bit, a NaN standing for any NaN (the payload of a NaN is not part of the contract)"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


def _key_matrix(X, C):
    """keys [n][nc] and distances of every pair in the reference's fold"""
    D = np.stack([ref.fold_distances(X, C[c]) for c in range(C.shape[0])], axis=1)
    return ref._keys(D), D


def _want(keys, dist, n, nc):
    lab = np.argmin(keys[:n, :nc], axis=1).astype(np.int64)  # (the first minimum: the lower centre number)
    return lab, dist[np.arange(n), lab]


MODES = ["auto", "exact", "bf16", "forced"]  # the three engines, and PN_ENGINE_AUTO with PN_OPT_KMEANS_FILTER = 1


def _set_mode(tree, mode):
    """False where the handle refuses PN_ENGINE_BF16: its k-NN tier cannot serve the index (fewer than 64 rows, values
    out of range) -- the k-means filter is then forced by its own option alone"""
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
    """every mode's labels, distances and inertia equal the reference's and pn_mean_shift_labels'; returns the
    fallback_queries a call through the filter added"""
    if want is None:
        want = ref.assign(X, C)
    wl, wd = want
    wi = ref.inertia(wl, wd)
    tree = pn.BallTree.euclidean(X)
    listed = None
    for mode in MODES:
        if not _set_mode(tree, mode):
            continue
        before = tree.stats()
        labels, dist, inertia = tree.kmeans_assign(C)
        after = tree.stats()
        assert np.array_equal(labels, wl), f"{mode}: labels differ at rows {np.flatnonzero(labels != wl)[:8]}"
        assert _same_bits(dist, wd), f"{mode}: distances differ"
        assert _same_bits(np.float64(inertia), np.float64(wi)), f"{mode}: inertia {inertia!r} != {wi!r}"
        assert after["queries"] - before["queries"] == X.shape[0]
        added = after["fallback_queries"] - before["fallback_queries"]
        if 8 <= X.shape[1] <= 320 and C.shape[0] >= 2 and mode in ("bf16", "forced"):
            assert listed is None or listed == added, "the listed rows do not depend on how the filter was chosen"
            listed = added
        else:  # (PN_ENGINE_AUTO leaves shapes this small to the exact kernel; one centre is always its)
            assert added == 0
    _set_mode(tree, "auto")
    assert np.array_equal(tree.mean_shift_labels(C, 1.0), wl), "pn_mean_shift_labels disagrees with the reference"
    return listed


# (n, nc): every n of {1, 63, 64, 65} and the row tile's 127 / 128 / 129, every nc of {1, 31, 32, 33, 65}
SHAPES = [(1, 1), (63, 31), (64, 32), (65, 33), (127, 65), (128, 33), (129, 65), (129, 1), (64, 65)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dim", [2, 7, 8, 9, 16, 17, 127, 128, 129, 200, 256, 257, 320, 321])
def test_assignment_bit_for_bit_at_the_tile_edges(pn, dim, dtype):
    X = _as(uniform((129, dim), 100 + dim), dtype)
    C = _as(uniform((65, dim), 200 + dim), dtype)
    keys, dist = _key_matrix(X, C)
    for n, nc in SHAPES:
        _check_assign(pn, X[:n].copy(), C[:nc].copy(), _want(keys, dist, n, nc))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_assignment_on_the_data_families(pn, name, dtype):
    for dim in (33, 128):
        X = _as(FAMILIES[name](257, dim, 31), dtype)
        C = _as(FAMILIES[name](65, dim, 32), dtype)
        _check_assign(pn, X, C)


def test_no_centres_and_device_entry(pn):
    import torch
    X = uniform((300, 16), 5)
    tree = pn.BallTree.euclidean(X)
    labels, dist, inertia = tree.kmeans_assign(np.zeros((0, 16), dtype=np.float32))
    assert np.all(labels == -1) and np.all(np.isnan(dist)) and inertia == 0.0
    C = uniform((40, 16), 6)
    wl, wd = ref.assign(X, C)
    for mode in MODES:
        assert _set_mode(tree, mode)
        dl, dd, di = tree.kmeans_assign_device(torch.from_numpy(C).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(dl.cpu().numpy(), wl) and dd.cpu().numpy().tobytes() == wd.tobytes()
        assert di.cpu().numpy()[0].tobytes() == np.float64(ref.inertia(wl, wd)).tobytes()
    # PN_OPT_KMEANS_FILTER = 2: never the filter, whatever the engine; other values are refused
    from petal_neighbors_amd import _lib
    from petal_neighbors_amd.errors import PetalError
    tree.set_engine("bf16")
    tree.set_option(_lib.PN_OPT_KMEANS_FILTER, 2)
    before = tree.stats()["fallback_queries"]
    labels, dist, _ = tree.kmeans_assign(np.concatenate([C, C]))  # (twins: the filter would list every row)
    assert np.array_equal(labels, wl) and tree.stats()["fallback_queries"] == before
    for bad in (-1, 3):
        with pytest.raises(PetalError):
            tree.set_option(_lib.PN_OPT_KMEANS_FILTER, bad)
    _set_mode(tree, "auto")
    # PN_OPT_INDEX_BASE affects no output
    tree.set_option(_lib.PN_OPT_INDEX_BASE, 1000)
    labels, dist, _ = tree.kmeans_assign(C)
    assert np.array_equal(labels, wl) and dist.tobytes() == wd.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rows_the_proof_must_refuse(pn, dtype):
    dim = 16
    X = _as(uniform((200, dim), 41), dtype)
    C = _as(uniform((40, dim), 42), dtype)
    # duplicated centres: the lower number wins, and the filter cannot tell them apart -- every row whose nearest centre
    # has a twin is refused
    Cd = np.concatenate([C, C[::-1]]).copy()
    listed = _check_assign(pn, X, Cd)
    assert listed == 200, listed
    assert ref.assign(X, Cd)[0].max() < 40
    # a row exactly equidistant from two centres (mirror images in column 0), and a row equal to a centre
    Xe = X.copy()
    Ce = C.copy()
    Xe[7] = 0
    Ce[3] = 0
    Ce[9] = 0
    Ce[3, 0], Ce[9, 0] = dtype(0.25), dtype(-0.25)
    Xe[11] = Ce[20]
    wl, wd = ref.assign(Xe, Ce)
    assert wl[7] == 3 and wd[7] == dtype(0.25) and wl[11] == 20 and wd[11] == 0
    listed = _check_assign(pn, Xe, Ce, (wl, wd))
    assert listed >= 1, "the tie must be refused by the proof"
    # NaN and inf rows: their distances are NaN or inf, ordered by the exact kernel (a NaN row belongs to centre 0)
    Xn = X.copy()
    Xn[0, 3] = np.nan
    Xn[1, 0] = np.inf
    Xn[2, 5] = -np.inf
    wl, wd = ref.assign(Xn, C)
    assert wl[0] == 0 and np.isnan(wd[0]) and np.isinf(wd[1])
    listed = _check_assign(pn, Xn, C, (wl, wd))
    assert listed >= 3
    # NaN and inf centres: the whole call is refused
    Cn = C.copy()
    Cn[5, 1] = np.nan
    Cn[6, 2] = np.inf
    listed = _check_assign(pn, X, Cn)
    assert listed == 200
    # norms beyond 2^100: rows, then a centre
    Xb = X.copy()
    Xb[4] = dtype(2.0 ** 51)
    Xb[5, 0] = dtype(-2.0 ** 60)
    listed = _check_assign(pn, Xb, C)
    assert listed >= 2
    Cb = C.copy()
    Cb[0] = dtype(2.0 ** 51)
    listed = _check_assign(pn, X, Cb)
    assert listed == 200


def test_argument_errors_that_need_a_handle(pn):
    """wrong element type (PN_ERR_INVALID) and a Cosine index (PN_ERR_UNSUPPORTED), on real handles through the C entries
    themselves (the Python methods refuse a Cosine tree before the call): the errors that come before the handle is
    looked at still win, and the type is reported before the metric.  The last error of the list, more than 2^31 - 1
    rows or centres, is not tested: it needs an index of that many rows."""
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    X = uniform((100, 8), 3)
    t32, t64 = pn.BallTree.euclidean(X), pn.BallTree.euclidean(X.astype(np.float64))
    c32 = pn.BallTree.new(X, pn.distance.Cosine())
    buf = np.zeros(4096, dtype=np.float64)  # (every pointer: large enough for any output, were a call to go through)
    p = buf.ctypes.data

    def loop(tree, sfx, device, fl=0, tol=0.0, mi=1, cout=p, labels=p, init=p, nc=2):
        extra = (None,) if device else ()
        name = f"pn_kmeans_device_{sfx}" if device else f"pn_kmeans_{sfx}"
        return getattr(L, name)(tree._h, init, nc, tol, mi, fl, cout, labels, None, None, None, None, None, *extra)

    def assign(tree, sfx, device, fl=0, labels=p, centres=p, nc=2):
        extra = (None,) if device else ()
        name = f"pn_kmeans_assign_device_{sfx}" if device else f"pn_kmeans_assign_{sfx}"
        return getattr(L, name)(tree._h, centres, nc, fl, labels, None, None, *extra)

    for device in (False, True):
        for call in (loop, assign):
            # the element type: an f64 entry on an f32 handle and the other way round
            for tree, sfx in ((t32, "f64"), (t64, "f32"), (c32, "f64")):
                assert call(tree, sfx, device) == _lib.PN_ERR_INVALID
                assert "element type" in _lib.last_error()
            # a Cosine index, with the right type: unsupported -- and with the wrong type the type is reported first (above)
            assert call(c32, "f32", device) == _lib.PN_ERR_UNSUPPORTED
            assert "Euclidean" in _lib.last_error()
            # what comes before the handle still wins on these handles
            for tree, sfx in ((t32, "f64"), (c32, "f32")):
                assert call(tree, sfx, device, fl=1) == _lib.PN_ERR_INVALID and "flags" in _lib.last_error()
                assert call(tree, sfx, device, labels=None) == _lib.PN_ERR_INVALID and "labels is NULL" in _lib.last_error()
        for tree, sfx in ((t32, "f64"), (c32, "f32")):
            assert loop(tree, sfx, device, tol=-1.0) == _lib.PN_ERR_INVALID and "tol" in _lib.last_error()
            assert loop(tree, sfx, device, tol=float("nan"), mi=0) == _lib.PN_ERR_INVALID and "tol" in _lib.last_error()
            assert loop(tree, sfx, device, mi=0) == _lib.PN_ERR_INVALID and "max_iter" in _lib.last_error()
            assert loop(tree, sfx, device, cout=None) == _lib.PN_ERR_INVALID and "centres_out" in _lib.last_error()
            assert loop(tree, sfx, device, init=None) == _lib.PN_ERR_INVALID and "centres is NULL" in _lib.last_error()
            assert loop(tree, sfx, device, nc=0) == _lib.PN_ERR_INVALID and "at least one centre" in _lib.last_error()
            assert assign(tree, sfx, device, centres=None) == _lib.PN_ERR_INVALID and "centres is NULL" in _lib.last_error()
    # the diagnostic: NULLs, then the type, the metric, the shapes the filter takes
    f = L.pn_kmeans_bounds_f32
    assert f(t64._h, p, 2, p) == _lib.PN_ERR_INVALID and "element type" in _lib.last_error()
    assert f(c32._h, p, 2, p) == _lib.PN_ERR_UNSUPPORTED and "Euclidean" in _lib.last_error()
    assert f(c32._h, p, 2, None) == _lib.PN_ERR_INVALID and "bounds_out is NULL" in _lib.last_error()
    narrow = pn.BallTree.euclidean(uniform((100, 4), 4))
    assert f(narrow._h, p, 2, p) == _lib.PN_ERR_UNSUPPORTED and "8 <= dim <= 320" in _lib.last_error()
    # nothing above touched a result: the handles still answer
    C = uniform((3, 8), 9)
    for tree, Cc in ((t32, C), (t64, C.astype(np.float64))):
        wl, wd = ref.assign(np.ascontiguousarray(tree.points), Cc)
        labels, dist, _ = tree.kmeans_assign(Cc)
        assert np.array_equal(labels, wl) and dist.tobytes() == wd.tobytes()


def _blobs(n, nc, dim):
    rng = np.random.default_rng(20261019)
    centres = (10.0 * rng.random((nc, dim))).astype(np.float32)
    own = rng.integers(0, nc, n)
    rows = (centres[own] + rng.normal(0.0, 0.01, (n, dim))).astype(np.float32)
    return rows, centres, own


@pytest.mark.parametrize("shape", [(8192, 64, 16), (8192, 300, 128)])
def test_the_filter_filters_on_separated_blobs(pn, shape):
    n, nc, dim = shape
    X, C, own = _blobs(n, nc, dim)
    x64, c64 = X.astype(np.float64), C.astype(np.float64)
    d2 = (x64 ** 2).sum(1)[:, None] + (c64 ** 2).sum(1)[None, :] - 2.0 * x64 @ c64.T
    part = np.partition(d2, 1, axis=1)
    nearest, second = part[:, 0], part[:, 1]
    slack = 8.0 * np.sqrt((x64 ** 2).sum(1).max()) * np.sqrt((c64 ** 2).sum(1).max()) * 2.0 ** -8
    # the condition: twice a generous bf16 slack separates every row's nearest centre from its second nearest
    assert second.min() - nearest.max() > slack, (second.min(), nearest.max(), slack)
    assert np.array_equal(np.argmin(d2, axis=1), own)
    tree = pn.BallTree.euclidean(X)
    tree.set_engine("exact")
    el, ed, ei = tree.kmeans_assign(C)
    assert np.array_equal(el, own)
    assert np.array_equal(tree.mean_shift_labels(C, 1.0), el)
    tree.set_engine("bf16")
    before = tree.stats()["fallback_queries"]
    labels, dist, inertia = tree.kmeans_assign(C)
    listed = tree.stats()["fallback_queries"] - before
    assert np.array_equal(labels, el) and dist.tobytes() == ed.tobytes() and inertia == ei
    assert listed == 0, f"a sound bound of the stated form lists no row here, the filter listed {listed}"
    sub = slice(0, 512)  # (the reference's fold on a part: the whole is the exact engine's, checked above)
    wl, wd = ref.assign(X[sub], C)
    assert np.array_equal(labels[sub], wl) and dist[sub].tobytes() == wd.tobytes()


@pytest.mark.parametrize("name", sorted(FAMILIES))
@pytest.mark.parametrize("dim", [8, 33, 128, 200, 320])
def test_lower_bound_pair_by_pair(pn, name, dim):
    X = FAMILIES[name](256, dim, 51)
    C = FAMILIES[name](65, dim, 52)
    tree = pn.BallTree.euclidean(X)
    L = tree.kmeans_bounds(C)
    assert L.shape == (256, 65) and np.all(np.isfinite(L))
    x64, c64 = X.astype(np.float64), C.astype(np.float64)
    d2 = ((x64[:, None, :] - c64[None, :, :]) ** 2).sum(2)
    gap = d2 - L
    assert gap.min() >= 0.0, f"{name}/D={dim}: the bound exceeds the squared distance by {-gap.min()}"
    if name == "uniform":  # useful on benign data: the slack is small against the spread of the squared distances
        assert gap.max() < 0.05 * d2.mean() + 1e-3
    # flagged operands give no bound
    Xb = X.copy()
    Xb[3, 0] = np.inf
    Lb = pn.BallTree.euclidean(Xb).kmeans_bounds(C)
    assert np.all(np.isnan(Lb[3])) and np.all(np.isfinite(Lb[4]))


def _segment_problem(dim, dtype):
    """clusters of exactly 4095, 4096 and 4097 members, one of 8200 (three segments), and a centre no row is near"""
    sizes = [4095, 4096, 4097, 8200]
    rng = np.random.default_rng(7)
    centres = np.zeros((5, dim))
    for c in range(5):
        centres[c, c % dim] = 10.0 * (c + 1) * (1 if c < dim else -1)
    centres[4] = -500.0
    own = np.repeat(np.arange(4), sizes)
    rng.shuffle(own)
    X = centres[own] + rng.normal(0.0, 0.05, (len(own), dim))
    init = centres + rng.normal(0.0, 0.3, centres.shape)
    init[4] = -500.0
    return _as(X.astype(np.float32), dtype), _as(init.astype(np.float32), dtype), sizes


def _same(got, want):
    names = ["centres", "labels", "inertia", "dist", "counts", "iterations", "shift2"]
    gc, gl, gi, gd, gn, git, gs = got
    wc, wl, wd, wn, wi, wit, ws = want
    for name, g, w in zip(names, (gc, gl, gi, gd, gn, git, gs), (wc, wl, wi, wd, wn, wit, ws)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.astype(w.dtype).tobytes() == w.tobytes(), f"{name} differs: {g!r} != {w!r}"


@pytest.mark.parametrize("dim,dtype", [(2, np.float32), (128, np.float32), (2, np.float64)])
def test_whole_kmeans_equals_the_reference(pn, dim, dtype):
    import torch
    X, init, sizes = _segment_problem(dim, dtype)
    tree = pn.BallTree.euclidean(X)
    want0 = ref.kmeans(X, init, 0.0, 50)        # tol = 0: run to the fixed point
    assert 2 <= want0[5] < 50 and want0[6] == 0.0
    assert want0[3].tolist() == sizes + [0]     # the segment edges, three segments, an empty cluster
    assert np.array_equal(want0[0][4], init[4])  # ... whose centre stayed
    want1 = ref.kmeans(X, init, 0.0, 1)         # max_iter = 1
    assert want1[5] == 1 and want1[6] > 0.0
    wantt = ref.kmeans(X, init, float(want1[6]), 50)  # a tolerance the first move meets exactly
    assert wantt[5] == 1
    for mode in MODES:
        assert _set_mode(tree, mode)
        _same(tree.kmeans(init, abs_tol=0.0, max_iter=50, full=True), want0)
        _same(tree.kmeans(init, abs_tol=0.0, max_iter=1, full=True), want1)
    _set_mode(tree, "forced")
    _same(tree.kmeans(init, abs_tol=float(want1[6]), max_iter=50, full=True), wantt)
    _same(tree.kmeans(init, abs_tol=0.0, max_iter=50, full=True), want0)  # a second run: the same bits
    assert tree.last_n_iter == want0[5]
    # the device entry
    c, l, d, n_, i, it, s2 = tree.kmeans_device(torch.from_numpy(init).cuda(), 0.0, 50)
    torch.cuda.synchronize()
    _same((c.cpu().numpy(), l.cpu().numpy(), i.cpu().numpy()[0], d.cpu().numpy(), n_.cpu().numpy().astype(np.uint64),
           int(it.cpu().numpy()[0]), s2.cpu().numpy()[0]), want0)
    # the relative tolerance of scikit-learn: tol times the mean column variance, computed on the host
    rel = 1e-4
    want_rel = ref.kmeans(X, init, rel * float(np.mean(np.var(X.astype(np.float64), axis=0))), 50)
    got = tree.kmeans(init, tol=rel, max_iter=50, full=True)
    _same(got, want_rel)


def test_kmeans_plusplus(pn):
    X = uniform((3000, 8), 77)
    tree = pn.BallTree.euclidean(X)
    a = tree.kmeans_plusplus(12, seed=5)
    assert a.shape == (12, 8) and a.dtype == np.float32
    rows = {r.tobytes() for r in X}
    assert all(c.tobytes() in rows for c in a), "the centres are rows of the corpus"
    assert len({c.tobytes() for c in a}) == 12, "distinct on distinct data"
    assert np.array_equal(tree.kmeans_plusplus(12, seed=5), a), "reproducible for one seed in one process"
    centres, labels, inertia = tree.kmeans(12, seed=5, max_iter=20)
    want = ref.kmeans(X, a, 1e-4 * float(np.mean(np.var(X.astype(np.float64), axis=0))), 20)
    assert centres.tobytes() == want[0].tobytes() and np.array_equal(labels, want[1]) and inertia == want[4]
