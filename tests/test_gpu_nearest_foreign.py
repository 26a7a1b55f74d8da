"""pn_nearest_foreign_*: every row's nearest row of another group, against numpy alone, on all three engines.

The contract (include/petal_mi355x.h): for row i the partner j with groups[j] != groups[i] that minimises (key(w), j),
w = max(d(i, j), core[i], core[j]), d the reference's sequential unfused fold in the index's dtype; a row without a foreign
row gets idx = 2^64 - 1 and the all-ones bit pattern as its weight.  The reference below is that sentence in numpy (the test
data has finite, non-negative weights, for which the key order is the numeric order; Cosine: the signed order, also numeric).
The exact engine, the forced bf16 first tier and PN_ENGINE_AUTO must agree with it bit for bit.
"""
import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE, PN_OPT_FOREIGN_FILTER = 3, 17
N = 300  # no multiple of 32 or 128: a last partial A tile, and listed-row tiles with empty lanes


def fold_distances(x):
    acc = np.zeros((len(x), len(x)), dtype=x.dtype)
    for k in range(x.shape[1]):
        diff = x[:, None, k] - x[None, :, k]
        acc += diff * diff
    return np.sqrt(acc)


def cosine_distances(x):
    dot = np.zeros((len(x), len(x)), dtype=x.dtype)
    sq = np.zeros(len(x), dtype=x.dtype)
    for k in range(x.shape[1]):
        dot += x[:, None, k] * x[None, :, k]
        sq += x[:, k] * x[:, k]
    nrm = np.sqrt(sq)
    return x.dtype.type(1) - dot / (nrm[:, None] * nrm[None, :])


def brute_force(d, groups, core, rows=None):
    w = d if core is None else np.maximum(np.maximum(d, core[:, None]), core[None, :])
    w = w + w.dtype.type(0)  # (-0 counts as +0)
    foreign = groups[:, None] != groups[None, :]
    big = np.where(foreign, w, np.inf)
    j = np.argmin(big, axis=1)  # (the first minimum: the smallest j among equal weights)
    u = np.uint32 if w.dtype == np.float32 else np.uint64
    bits = np.where(foreign.any(axis=1), w[np.arange(len(w)), j].view(u), ~u(0))
    idx = np.where(foreign.any(axis=1), j.astype(np.uint64), ~np.uint64(0))
    rows = np.arange(len(w)) if rows is None else np.asarray(rows)
    return idx[rows], bits[rows]


def make_data(kind, dim, dtype):
    if kind == "uniform":
        return uniform((N, dim), 41 + dim, dtype)
    rng = np.random.default_rng(7 + dim)
    if kind == "blobs":  # tight and far from the origin: the centring and the slack
        centres = 1000.0 + 50.0 * rng.standard_normal((6, dim))
        return (centres[rng.integers(0, 6, N)] + 0.01 * rng.standard_normal((N, dim))).astype(dtype)
    x = uniform((N, dim), 43 + dim, dtype)  # "duplicates": 20 exact copies of one row, spread over the groups
    x[rng.choice(N, 20, replace=False)] = x[5]
    return x


GROUPINGS = {
    "singletons": np.arange(N),
    "interleaved": np.arange(N) % 2,
    "all_but_last": (np.arange(N) == N - 1).astype(np.int64) * 9,
    "one_group": np.full(N, 3),
}


def engines(tree):
    """the three engines on one handle: (name, tree)"""
    yield "exact", tree.set_option(PN_OPT_FOREIGN_FILTER, 0).set_engine("exact")
    yield "filter", tree.set_engine("auto").set_option(PN_OPT_FOREIGN_FILTER, 1)
    yield "auto", tree.set_option(PN_OPT_FOREIGN_FILTER, 0)


@pytest.mark.parametrize("kind", ["uniform", "blobs", "duplicates"])
@pytest.mark.parametrize("dim", [8, 20, 130])  # the minimum; padded to 32; two K-chunks of the exact scan, dp = 144
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_against_brute_force(pn, dtype, dim, kind):
    x = make_data(kind, dim, dtype)
    tree = pn.BallTree.euclidean(x)
    d = fold_distances(x)
    core5 = tree.query_self(5)[1][:, -1].copy()  # ties at the floor core[i] everywhere
    for gname, groups in GROUPINGS.items():
        for core in (None, core5):
            want = brute_force(d, groups, core)
            for ename, t in engines(tree):
                idx, w = t.nearest_foreign(groups, core)
                where = (gname, core is not None, ename)
                assert np.array_equal(idx, want[0]), where
                assert np.array_equal(w.view(want[1].dtype), want[1]), where


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rows_index_base_and_device_form(pn, dtype):
    import torch
    x = make_data("uniform", 20, dtype)
    tree = pn.BallTree.euclidean(x).set_option(PN_OPT_INDEX_BASE, 1000)
    groups = np.arange(N) % 7
    core = tree.query_self(5)[1][:, -1].copy()
    rows = np.array([299, 0, 17, 17, 128, 64, 31], dtype=np.uint64)
    want = brute_force(fold_distances(x), groups, core)
    for _, t in engines(tree):
        idx, w = t.nearest_foreign(groups, core, rows=rows)
        assert np.array_equal(idx, want[0][rows.astype(int)] + 1000) and np.array_equal(w.view(want[1].dtype), want[1][rows.astype(int)])
        di, dw = t.nearest_foreign_device(torch.from_numpy(groups.astype(np.int32)).cuda(), torch.from_numpy(core).cuda(),
                                          rows=torch.from_numpy(rows.astype(np.int64)).cuda())
        assert np.array_equal(di.cpu().numpy().view(np.uint64), idx) and np.array_equal(dw.cpu().numpy(), w)
        assert [len(a) for a in t.nearest_foreign(groups, core, rows=np.flatnonzero(groups > 99))] == [0, 0]  # an empty list


def test_cosine_takes_the_exact_scan(pn):
    x = (uniform((N, 20), 5) - np.float32(0.5)).astype(np.float32)
    tree = pn.BallTree.new(x, pn.distance.Cosine()).set_option(PN_OPT_FOREIGN_FILTER, 1)
    groups = np.arange(N) % 3
    idx, w = tree.nearest_foreign(groups)
    want = brute_force(cosine_distances(x), groups, None)
    assert np.array_equal(idx, want[0]) and np.array_equal(w.view(np.uint32), want[1])
    assert tree.stats()["candidates"] == 0


def test_the_filter_answers_and_counts(pn):
    x = make_data("uniform", 20, np.float32)
    tree = pn.BallTree.euclidean(x).set_option(PN_OPT_FOREIGN_FILTER, 1)
    tree.stats(reset=True)
    tree.nearest_foreign(np.arange(N) % 2)
    s = tree.stats()
    assert s["queries"] == N and s["candidates"] > 0 and s["evaluations"] == s["candidates"]
    assert s["fallback_queries"] < N  # (not by handing every row to the exact scan)
    x[7, 3] = np.inf  # a row that is not finite: the call goes to the exact scan as a whole, the tier is not launched
    flagged = pn.BallTree.euclidean(x).set_option(PN_OPT_FOREIGN_FILTER, 1)
    got = flagged.nearest_foreign(np.arange(N) % 2)
    assert flagged.stats()["candidates"] == 0
    want = flagged.set_option(PN_OPT_FOREIGN_FILTER, 2).nearest_foreign(np.arange(N) % 2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


def test_mst_rounds_through_the_filter(pn):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((8, 16))[rng.integers(0, 8, 2000)] * 4 + 0.3 * rng.standard_normal((2000, 16))).astype(np.float32)
    tree = pn.BallTree.euclidean(x)
    core = tree.query_self(5)[1][:, -1].copy()
    exact = tree.set_engine("exact").mst(core)
    work = tree.last_mst_work
    tree.set_engine("auto").set_option(PN_OPT_FOREIGN_FILTER, 1).stats(reset=True)
    got = tree.mst(core)
    assert all(np.array_equal(a, b) for a, b in zip(got[:2], exact[:2]))
    assert np.array_equal(got[2].view(np.uint32), exact[2].view(np.uint32))
    assert tree.last_mst_work == work and tree.stats()["candidates"] > 0


def test_argument_errors_in_the_stated_order(pn):
    from petal_neighbors_amd import _lib
    tree = pn.BallTree.euclidean(make_data("uniform", 8, np.float32))
    g, idx, w = np.zeros(N, np.uint32), np.zeros(N, np.uint64), np.zeros(N, np.float32)
    rows = np.zeros(2, np.uint64)
    f32, f64 = _lib.lib().pn_nearest_foreign_f32, _lib.lib().pn_nearest_foreign_f64
    p = lambda a: a.ctypes.data
    for call, message in [
        (lambda: f32(tree._h, None, None, p(rows), 0, 1, None, None), "flags"),          # flags before everything else
        (lambda: f32(tree._h, None, None, None, 2, 0, None, None), "rows is NULL"),       # then the list
        (lambda: f32(tree._h, None, None, None, 0, 0, None, p(w)), "idx_out is NULL"),    # then the outputs
        (lambda: f32(tree._h, None, None, None, 0, 0, p(idx), None), "weight_out is NULL"),
        (lambda: f32(tree._h, None, None, None, 0, 0, p(idx), p(w)), "groups is NULL"),
        (lambda: f32(None, p(g), None, None, 0, 0, p(idx), p(w)), "index is NULL"),
        (lambda: f64(tree._h, p(g), None, None, 0, 0, p(idx), p(w)), "element type"),
    ]:
        assert call() == _lib.PN_ERR_INVALID and message in _lib.last_error(), message
    assert f32(tree._h, p(g), None, p(rows), 0, 0, None, None) == _lib.PN_OK  # an empty list: nothing to write
    rows[1] = N
    assert f32(tree._h, p(g), None, p(rows), 2, 0, p(idx), p(w)) == _lib.PN_ERR_INVALID and "rows[1]" in _lib.last_error()
    with pytest.raises(ValueError):
        tree.nearest_foreign(g[:-1])
