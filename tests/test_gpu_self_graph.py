"""pn_query_self_* / pn_query_radius_self_*: every indexed row against its own index, the row itself left out.

k-NN answers must equal the rule of include/petal_mi355x.h -- pn_query_*(rows, k + 1) with each row's own index dropped
if present, else the last entry -- for the engine's own answers and for the oracle's brute force (Euclidean) or its
pairwise Cosine matrix; radius answers must equal the with-distance lists of the rows minus each row itself."""
import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu


def _rule(idx, dist, rows, base=0):
    """drop, in each row's (k + 1)-answer, the entry equal to its own index, else the last one"""
    nq, kin = idx.shape
    if kin == 0:
        return idx, dist
    own = idx == (np.asarray(rows, dtype=np.uint64) + np.uint64(base))[:, None]
    j = np.where(own.any(axis=1), own.argmax(axis=1), kin - 1)
    keep = np.ones_like(own)
    keep[np.arange(nq), j] = False
    return idx[keep].reshape(nq, kin - 1), dist[keep].reshape(nq, kin - 1)


def _same(a_idx, a_dist, b_idx, b_dist, what):
    assert a_idx.shape == b_idx.shape, what
    assert np.array_equal(a_idx.astype(np.uint64), b_idx.astype(np.uint64)), what
    assert a_dist.tobytes() == b_dist.tobytes(), what


def _same_nan(a_idx, a_dist, b_idx, b_dist, what):
    """_same, but a NaN distance matches any NaN (the oracle's pairwise matrix does not canonicalise the sign of NaN)"""
    assert np.array_equal(a_idx.astype(np.uint64), b_idx.astype(np.uint64)), what
    nan = np.isnan(a_dist)
    assert np.array_equal(nan, np.isnan(b_dist)), what
    assert a_dist[~nan].tobytes() == b_dist[~nan].tobytes(), what


def _sample(n, m, seed):
    if n <= m:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, m, replace=False))


def _check_knn(oracle_mod, tree, pts, k, rows_checked=64, base=0):
    n = pts.shape[0]
    idx, dist = tree.query_self(k)
    kout = min(k, n - 1)
    assert idx.shape == (n, kout) and dist.shape == (n, kout)
    if kout == 0:
        return idx, dist
    # the engine's own k + 1 answer, reduced by the rule
    ei, ed = tree.query_batch(pts, k + 1)
    _same(idx, dist, *_rule(ei, ed, np.arange(n), base), f"rule n={n} k={k}")
    # the oracle's brute force over the other rows (sampled rows of large corpora)
    rows = _sample(n, rows_checked, 1234 + k)
    oi, od = oracle_mod.brute_knn(pts, pts[rows], k + 1)
    _same(idx[rows], dist[rows], *_rule(oi + np.uint64(base), od, rows, base), f"oracle n={n} k={k}")
    assert not (idx == (np.arange(n, dtype=np.uint64) + np.uint64(base))[:, None]).any()
    # include_self is query_batch(rows, k) exactly
    ii, idd = tree.query_self(k, include_self=True)
    ei, ed = tree.query_batch(pts, k)
    _same(ii, idd, ei, ed, f"include_self n={n} k={k}")
    return idx, dist


CASES = [(1, 4, [0, 1, 3]), (2, 4, [0, 1, 2, 7]), (50, 7, [1, 10, 49, 50, 55, 100]), (5000, 32, [1, 10, 100]),
         (20000, 16, [1, 10, 100])]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,dim,ks", CASES, ids=[f"{c[0]}x{c[1]}" for c in CASES])
def test_knn_self_equals_rule_and_oracle(pn, oracle_mod, dtype, n, dim, ks):
    pts = uniform((n, dim), 0x5E1F0000 + n + dim, dtype)
    tree = pn.BallTree.euclidean(pts)
    if n == 20000:
        assert tree.bf16_eligible  # the narrow bf16 tier (fused query pack reading the rows in place)
    for k in ks:
        _check_knn(oracle_mod, tree, pts, k)
    tree.close()


def test_knn_self_large_sampled(pn, oracle_mod):
    pts = uniform((200000, 128), 0x5E1F0200, np.float32)
    tree = pn.BallTree.euclidean(pts)
    tree.stats(reset=True)
    idx, dist = tree.query_self(10)
    assert tree.stats()["queries"] == 200000  # n queries, as a batch of n
    rows = _sample(200000, 24, 99)
    oi, od = oracle_mod.brute_knn(pts, pts[rows], 11)
    _same(idx[rows], dist[rows], *_rule(oi, od, rows), "oracle 200000 x 128")
    ei, ed = tree.query_batch(pts[:30000], 11)
    _same(idx[:30000], dist[:30000], *_rule(ei, ed, np.arange(30000)), "rule 200000 x 128")
    tree.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_duplicates_nan_row_and_index_base(pn, oracle_mod, dtype):
    k = 10
    n, dim = 6000, 16
    pts = uniform((n, dim), 0x5E1F0300, dtype)
    dup = np.arange(100, 100 + k + 3)
    pts[dup] = pts[17]
    pts[5] = np.nan
    tree = pn.BallTree.euclidean(pts)
    idx, dist = _check_knn(oracle_mod, tree, pts, k)
    for i in list(dup) + [17]:
        others = [j for j in [17] + list(dup) if j != i][:k]
        assert np.array_equal(idx[i], np.array(others, dtype=np.uint64)), i
        assert not dist[i].any()
    assert np.isnan(dist[5]).all() and 5 not in idx[5]
    # PN_OPT_INDEX_BASE: the row is recognised as i + base
    from petal_neighbors_amd import _lib
    base = 1 << 40
    tree.set_option(_lib.PN_OPT_INDEX_BASE, base)
    bi, bd = tree.query_self(k)
    _same(bi, bd, idx + np.uint64(base), dist, "index base")
    ei, ed = tree.query_batch(pts, k + 1)
    _same(bi, bd, *_rule(ei, ed, np.arange(n), base), "index base rule")
    tree.close()


def _cosine_oracle(oracle_mod, x, k):
    """k nearest other rows under Cosine::distance, by (distance, index), -0 as +0, NaN last"""
    m = oracle_mod.pairwise_cosine(x)
    n = x.shape[0]
    out_i = np.empty((n, min(k, n - 1)), dtype=np.uint64)
    out_d = np.empty((n, min(k, n - 1)), dtype=x.dtype)
    for i in range(n):
        j = np.array([c for c in range(n) if c != i])
        d = m[i, j]
        o = np.lexsort((j, d.astype(np.float64) + 0.0))[:out_i.shape[1]]
        out_i[i], out_d[i] = j[o], d[o]
    return out_i, out_d


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_cosine_self(pn, oracle_mod, dtype):
    n, dim = 300, 12
    rng = np.random.default_rng(77)
    x = (uniform((n, dim), 0x5E1F0400, dtype) - dtype(0.5)) * rng.uniform(0.01, 300.0, (n, 1)).astype(dtype)
    x[7] = 0  # a row without a direction: NaN against everything
    x[40:44] = x[3] * dtype(3.0)  # parallel rows
    tree = pn.BallTree.new(x, pn.distance.Cosine())
    selfd = np.array([oracle_mod.cosine(x[i], x[i]) for i in range(n)])
    assert (selfd[np.isfinite(selfd)] != 0).any()  # self-distances that are not 0
    for k in (1, 10, n - 1, n + 5):
        idx, dist = tree.query_self(k)
        oi, od = _cosine_oracle(oracle_mod, x, k)
        _same_nan(idx, dist, oi, od, f"cosine oracle k={k}")
        ei, ed = tree.query_batch(x, k + 1)
        _same(idx, dist, *_rule(ei, ed, np.arange(n)), f"cosine rule k={k}")
        ii, idd = tree.query_self(k, include_self=True)
        _same(ii, idd, *tree.query_batch(x, k), f"cosine include k={k}")
    tree.close()
    # a larger Cosine index served by the filter tier (no zero row)
    y = uniform((8000, 16), 0x5E1F0401, dtype) - dtype(0.5)
    t2 = pn.BallTree.new(y, pn.distance.Cosine())
    idx, dist = t2.query_self(10)
    ei, ed = t2.query_batch(y, 11)
    _same(idx, dist, *_rule(ei, ed, np.arange(8000)), "cosine 8000 rule")
    t2.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_device_equals_host_on_a_side_stream(pn, dtype):
    import torch
    pts = uniform((20000, 16), 0x5E1F0500, dtype)
    pts[9] = pts[10]
    tree = pn.BallTree.euclidean(pts)
    hi, hd = tree.query_self(12)
    ii, idd = tree.query_self(12, include_self=True)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        di, dd = tree.query_self_device(12, stream=st.cuda_stream)
        ji, jd = tree.query_self_device(12, include_self=True, stream=st.cuda_stream)
    st.synchronize()
    _same(di.cpu().numpy(), dd.cpu().numpy(), hi, hd, "device")
    _same(ji.cpu().numpy(), jd.cpu().numpy(), ii, idd, "device include")
    tree.close()


# ------------------------------------------------------------------------------------------------------------ radius
def _minus_self(off, idx, dist, base=0):
    """CSR minus each row's own index"""
    n = off.size - 1
    o = off.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(o))
    keep = idx != rows + np.uint64(base)
    cs = np.concatenate([[0], np.cumsum(keep.astype(np.int64))])
    return (cs[o] - cs[0]).astype(np.uint64), idx[keep], dist[keep]


def _sorted_lists(off, idx, dist):
    si, sd = idx.copy(), dist.copy()
    for a in range(off.size - 1):
        lo, hi = int(off[a]), int(off[a + 1])
        o = np.lexsort((idx[lo:hi], dist[lo:hi].astype(np.float64) + 0.0))
        si[lo:hi], sd[lo:hi] = idx[lo:hi][o], dist[lo:hi][o]
    return si, sd


def _check_radius(oracle_mod, tree, pts, r, cosine=False, rows_checked=32):
    n = pts.shape[0]
    off, idx, dist = tree.query_radius_self(r, with_distance=True)
    wo, wi, wd = tree.query_radius_with_distance_batch(pts, r)
    eo, ei, ed = _minus_self(wo, wi, wd)
    assert np.array_equal(off, eo) and np.array_equal(idx, ei) and dist.tobytes() == ed.tobytes()
    o2, i2, d2 = tree.query_radius_self(r)
    assert np.array_equal(o2, off) and np.array_equal(i2, idx) and d2 is None
    so, si, sd = tree.query_radius_self(r, with_distance=True, sort=True)
    xi, xd = _sorted_lists(off, idx, dist)
    assert np.array_equal(so, off) and np.array_equal(si, xi) and sd.tobytes() == xd.tobytes()
    io, ii, idd = tree.query_radius_self(r, with_distance=True, include_self=True)
    assert np.array_equal(io, wo) and np.array_equal(ii, wi) and idd.tobytes() == wd.tobytes()
    if not cosine:
        for a in _sample(n, rows_checked, 5):
            want = oracle_mod.brute_radius(pts, pts[a], r)
            want = want[want != a]
            assert np.array_equal(idx[int(off[a]):int(off[a + 1])], want), a
    return off, idx, dist


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,dim", [(3000, 8), (20000, 16)], ids=["3000x8", "20000x16"])
def test_radius_self(pn, oracle_mod, dtype, n, dim):
    pts = uniform((n, dim), 0x5E1F0600 + n, dtype)
    pts[11:15] = pts[2]
    pts[20] = np.nan
    tree = pn.BallTree.euclidean(pts)
    _, d = oracle_mod.brute_knn(pts, pts[100:120], 21)
    r = dtype(np.median(d[:, 20]))
    off, idx, _ = _check_radius(oracle_mod, tree, pts, r)
    assert int(off[-1]) > n * 5
    assert int(off[21]) == int(off[20])  # the NaN row has nobody
    for rr in (0.0, -1.0, float("nan")):
        o, i, dd = tree.query_radius_self(rr, with_distance=True, sort=True)
        assert int(o[-1]) == 0 and i.size == 0 and dd.size == 0
    if n <= 3000:
        o, i, dd = _check_radius(oracle_mod, tree, pts, float("inf"))
        assert int(o[-1]) == (n - 1) * (n - 2)  # every finite row, but neither itself nor the NaN row
    tree.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_radius_self_cosine(pn, oracle_mod, dtype):
    n, dim = 400, 10
    rng = np.random.default_rng(78)
    x = (uniform((n, dim), 0x5E1F0700, dtype) - dtype(0.5)) * rng.uniform(0.01, 300.0, (n, 1)).astype(dtype)
    x[9] = 0
    tree = pn.BallTree.new(x, pn.distance.Cosine())
    m = oracle_mod.pairwise_cosine(x)
    for r in (0.05, 0.3, 1.0, 1.5, float("inf")):
        off, idx, dist = _check_radius(oracle_mod, tree, x, r, cosine=True)
        for a in range(0, n, 37):
            j = np.array([c for c in range(n) if c != a])
            want = j[m[a, j] < dtype(r)]
            assert np.array_equal(idx[int(off[a]):int(off[a + 1])], want), (r, a)
    tree.close()
    y = uniform((8000, 16), 0x5E1F0701, dtype) - dtype(0.5)  # the filter tier's Cosine radius path (r < 1)
    t2 = pn.BallTree.new(y, pn.distance.Cosine())
    _check_radius(oracle_mod, t2, y, 0.02, cosine=True)
    t2.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_radius_self_device_capacity_contract(pn, oracle_mod, dtype):
    import torch
    pts = uniform((20000, 16), 0x5E1F0800, dtype)
    pts[30:33] = pts[31]
    tree = pn.BallTree.euclidean(pts)
    _, d = oracle_mod.brute_knn(pts, pts[:20], 25)
    r = dtype(np.median(d[:, 24]))
    off, idx, dist = tree.query_radius_self(r, with_distance=True)
    _, sidx, sdist = tree.query_radius_self(r, with_distance=True, sort=True)
    total = int(off[-1])
    st = torch.cuda.Stream()
    for cap in (0, total // 3, total, total + 100):
        for sort in (False, True):
            with torch.cuda.stream(st):
                o, i, dd, t = tree.query_radius_self_device(r, cap, with_distance=True, sort=sort, stream=st.cuda_stream)
            st.synchronize()
            o, i, dd = o.cpu().numpy().astype(np.uint64), i.cpu().numpy().astype(np.uint64), dd.cpu().numpy()
            assert np.array_equal(o, off) and int(t.item()) == total, (cap, sort)
            m = min(cap, total)
            if not sort:
                assert np.array_equal(i[:m], idx[:m]) and dd[:m].tobytes() == dist[:m].tobytes(), (cap, sort)
                continue
            whole = int(np.searchsorted(off, m, side="right")) - 1  # lists [0, whole) end at or below the capacity
            e = int(off[whole])
            assert np.array_equal(i[:e], sidx[:e]) and dd[:e].tobytes() == sdist[:e].tobytes(), (cap, sort)
            # the straddling list: its first entries in ascending index order
            assert np.array_equal(i[e:m], idx[e:m]) and dd[e:m].tobytes() == dist[e:m].tobytes(), (cap, sort)
    # indices only, and include_self through the device entry
    o, i, dd, t = tree.query_radius_self_device(r, total)
    torch.cuda.synchronize()
    assert dd is None and np.array_equal(i.cpu().numpy().astype(np.uint64)[:total], idx)
    wo, wi, wd = tree.query_radius_with_distance_batch(pts, r)
    o, i, dd, t = tree.query_radius_self_device(r, int(wo[-1]), with_distance=True, include_self=True)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy().astype(np.uint64), wo) and np.array_equal(i.cpu().numpy().astype(np.uint64), wi)
    assert dd.cpu().numpy().tobytes() == wd.tobytes()
    tree.close()


def test_single_row_index(pn):
    t = pn.BallTree.euclidean(np.array([[1.0, 2.0, 3.0]], dtype=np.float32))
    i, d = t.query_self(5)
    assert i.shape == (1, 0)
    i, d = t.query_self(5, include_self=True)
    assert i.tolist() == [[0]] and d.tolist() == [[0.0]]
    off, idx, dist = t.query_radius_self(1.0, with_distance=True)
    assert off.tolist() == [0, 0] and idx.size == 0
    off, idx, dist = t.query_radius_self(1.0, with_distance=True, include_self=True)
    assert off.tolist() == [0, 1] and idx.tolist() == [0]
    t.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_radius_self_cosine_at_the_self_distances(pn, oracle_mod, dtype):
    """radii between and at the rows' own Cosine distances (0 and a few ulp either side): the self flag, recomputed from the
    rows, must agree with the pipeline's lists at every one of them"""
    n, dim = 400, 10
    rng = np.random.default_rng(79)
    x = (uniform((n, dim), 0x5E1F0900, dtype) - dtype(0.5)) * rng.uniform(0.01, 300.0, (n, 1)).astype(dtype)
    x[9] = 0
    selfd = np.array([oracle_mod.cosine(x[i], x[i]) for i in range(n)], dtype=dtype)
    vals = np.unique(selfd[np.isfinite(selfd)])
    assert vals.size >= 2 and (vals != 0).any()  # 0 and some ulps away from it
    radii = sorted({float(v) for v in vals} | {float(np.nextafter(v, dtype(np.inf))) for v in vals})
    tree = pn.BallTree.new(x, pn.distance.Cosine())
    m = oracle_mod.pairwise_cosine(x)
    for r in radii:
        off, idx, _ = _check_radius(oracle_mod, tree, x, r, cosine=True)
        for a in range(0, n, 7):
            j = np.array([c for c in range(n) if c != a])
            assert np.array_equal(idx[int(off[a]):int(off[a + 1])], j[m[a, j] < dtype(r)]), (r, a)
        # the rows kept with include_self are exactly those whose own distance is below r
        io, ii, _ = tree.query_radius_self(r, include_self=True)
        own = np.array([i in ii[int(io[i]):int(io[i + 1])] for i in range(n)])
        assert np.array_equal(own, selfd < dtype(r)), r
        assert np.array_equal(np.diff(io.astype(np.int64)) - np.diff(off.astype(np.int64)), own.astype(np.int64)), r
    tree.close()
    # the filter tier's Cosine radius path, r of the order of the self-distances: the lists are little more than the rows
    y = uniform((8000, 16), 0x5E1F0901, dtype) - dtype(0.5)
    t2 = pn.BallTree.new(y, pn.distance.Cosine())
    eps = float(np.finfo(dtype).eps)
    for r in (eps / 4, eps, 4 * eps):
        _check_radius(oracle_mod, t2, y, r, cosine=True)
    t2.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_radius_self_index_base_and_chunks(pn, oracle_mod, dtype):
    """PN_OPT_INDEX_BASE != 0 (the compaction looks for base + i), and more rows than one pipeline chunk (2^18)"""
    import torch
    from petal_neighbors_amd import _lib
    n, dim = 300000, 8
    pts = uniform((n, dim), 0x5E1F0A00, dtype)
    pts[262140:262150] = pts[262144]  # duplicates across the chunk boundary
    tree = pn.BallTree.euclidean(pts)
    _, d = oracle_mod.brute_knn(pts, pts[:16], 9)
    r = dtype(np.median(d[:, 8]))
    off, idx, dist = tree.query_radius_self(r, with_distance=True)
    wo, wi, wd = tree.query_radius_with_distance_batch(pts, r)
    eo, ei, ed = _minus_self(wo, wi, wd)
    assert np.array_equal(off, eo) and np.array_equal(idx, ei) and dist.tobytes() == ed.tobytes()
    for a in (0, 262143, 262144, 262145, n - 1):
        want = oracle_mod.brute_radius(pts, pts[a], r)
        assert np.array_equal(idx[int(off[a]):int(off[a + 1])], want[want != a]), a
    base = 1 << 40
    tree.set_option(_lib.PN_OPT_INDEX_BASE, base)
    bo, bi, bd = tree.query_radius_self(r, with_distance=True, sort=True)
    xi, xd = _sorted_lists(off, idx, dist)
    assert np.array_equal(bo, off) and np.array_equal(bi, xi + np.uint64(base)) and bd.tobytes() == xd.tobytes()
    total = int(off[-1])
    o, i, dd, t = tree.query_radius_self_device(r, total // 2, with_distance=True)
    torch.cuda.synchronize()
    m = total // 2
    assert np.array_equal(o.cpu().numpy().astype(np.uint64), off) and int(t.item()) == total
    assert np.array_equal(i.cpu().numpy().astype(np.uint64)[:m], idx[:m] + np.uint64(base))
    assert dd.cpu().numpy()[:m].tobytes() == dist[:m].tobytes()
    tree.close()
