"""pn_query_radius_with_distance_{,device_}{f32,f64}: the lists of pn_query_radius_* with each neighbour's distance,
bit-identical to the oracle's metric, ascending by index or -- PN_RADIUS_SORTED -- by (distance, index), the k-NN
answers' order (csr_sort.hip: one workgroup per short list, chunks + merge passes for lists beyond 2048 entries)."""
import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu


def _oracle_dists(oracle_mod, pts, q, idx, cosine):
    f = oracle_mod.cosine if cosine else oracle_mod.euclidean
    return np.array([f(q, pts[int(i)]) for i in idx], dtype=pts.dtype)


def _by_dist_idx(dist, idx, cosine):
    """(distance, index) ascending; -0 as +0 (Cosine distances may lie below zero)"""
    d = dist.astype(np.float64) + 0.0
    return np.lexsort((idx, d))


def _check(pn, oracle_mod, tree, pts, qs, r, cosine=False, knn_k=5, max_checked=4000):
    """host entry point: unsorted lists equal query_radius_batch; every distance equals the oracle's; sorted lists are the
    unsorted ones ordered by (distance, index) and start with query(q, k)"""
    want_off, want_idx = tree.query_radius_batch(qs, r)
    off, idx, dist = tree.query_radius_with_distance_batch(qs, r)
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
    soff, sidx, sdist = tree.query_radius_with_distance_batch(qs, r, sort=True)
    assert np.array_equal(soff, want_off)
    checked = 0
    for a in range(qs.shape[0]):
        lo, hi = int(off[a]), int(off[a + 1])
        li, ld = idx[lo:hi], dist[lo:hi]
        if checked < max_checked:
            assert ld.tobytes() == _oracle_dists(oracle_mod, pts, qs[a], li, cosine).tobytes(), a
            checked += hi - lo
        order = _by_dist_idx(ld, li, cosine)
        assert np.array_equal(sidx[lo:hi], li[order]), a
        assert sdist[lo:hi].tobytes() == ld[order].tobytes(), a
        if hi - lo >= knn_k and not np.isnan(qs[a]).any():
            ki, kd = tree.query(qs[a], knn_k)
            assert np.array_equal(sidx[lo:lo + knn_k], ki) and sdist[lo:lo + knn_k].tobytes() == kd.tobytes(), a
    return off, idx, dist


def _clumped(dtype, n=20000, dim=16, seed=7101):
    """uniform rows, a dense clump (overflows the filter's 224-per-segment lists) and duplicated rows (tie order)"""
    rng = np.random.default_rng(seed)
    base = uniform((n, dim), seed, dtype)
    clump = (base[777] + 0.002 * rng.standard_normal((3000, dim))).astype(dtype)
    pts = np.concatenate([base, clump]).astype(dtype)
    pts[100:108] = pts[50]
    qs = np.concatenate([uniform((60, dim), seed + 1, dtype), clump[:3] + dtype(0.0005), pts[50:51],
                         np.full((1, dim), np.nan, dtype)]).astype(dtype)
    return pts, qs


@pytest.fixture(scope="module")
def euclid_trees(pn, oracle_mod):
    """one index per element type, built on first use: (tree, points, queries, radius)"""
    made = {}

    def get(dtype):
        if dtype not in made:
            pts, qs = _clumped(dtype)
            tree = pn.BallTree.euclidean(pts)
            _, d = oracle_mod.brute_knn(pts, qs[:20], 12)
            made[dtype] = (tree, pts, qs, dtype(np.median(d[:, 11])))
        return made[dtype]
    return get


@pytest.fixture(params=[np.float32, np.float64], ids=["f32", "f64"])
def euclid(request, euclid_trees):
    return euclid_trees(request.param)


TIERS = [(np.float32, "auto"), (np.float32, "bf16"), (np.float32, "mfma"), (np.float32, "exact"),
         (np.float64, "auto"), (np.float64, "bf16"), (np.float64, "exact")]  # (the MFMA tier serves f32 indexes)


@pytest.mark.parametrize("dtype,engine", TIERS, ids=[f"{np.dtype(d).name}-{e}" for d, e in TIERS])
def test_every_tier_gives_bit_exact_distances_and_the_knn_order(pn, oracle_mod, euclid_trees, dtype, engine):
    tree, pts, qs, r = euclid_trees(dtype)
    tree.set_engine(engine)
    try:
        off, _, _ = _check(pn, oracle_mod, tree, pts, qs, r)
        assert int(off[-1]) > 3000  # the clump's queries: their lists overflow the filter and are re-run exactly
        # the sorted list of a uniform query is the oracle's brute-force prefix below r
        bi, bd = oracle_mod.brute_knn(pts, qs[:2], pts.shape[0])
        _, si, sd = tree.query_radius_with_distance_batch(qs[:2], r, sort=True)
        o2, _, _ = tree.query_radius_with_distance_batch(qs[:2], r)
        for a in range(2):
            m = int(np.sum(bd[a] < r))
            assert np.array_equal(si[int(o2[a]):int(o2[a + 1])], bi[a, :m])
            assert sd[int(o2[a]):int(o2[a + 1])].tobytes() == bd[a, :m].tobytes()
    finally:
        tree.set_engine("auto")


def test_truncated_queries_and_edge_radii(pn, oracle_mod, euclid):
    tree, pts, qs, r = euclid
    _check(pn, oracle_mod, tree, pts, np.ascontiguousarray(qs[:20, :9]), r * pts.dtype.type(0.6))
    for rr in (0.0, -1.0, float("nan")):
        off, idx, dist = tree.query_radius_with_distance_batch(qs[:5], rr, sort=True)
        assert int(off[-1]) == 0 and idx.size == 0 and dist.size == 0
    # an unknown flag bit
    import ctypes as C
    from petal_neighbors_amd import _lib
    sfx = "f32" if pts.dtype == np.float32 else "f64"
    off = np.zeros(2, dtype=np.uint64)
    oi, od = C.c_void_p(0), C.c_void_p(0)
    fn = getattr(_lib.lib(), f"pn_query_radius_with_distance_{sfx}")
    rc = fn(tree._h, qs.ctypes.data, 1, qs.shape[1], qs.shape[1], (C.c_float if sfx == "f32" else C.c_double)(r), 2,
            off.ctypes.data, C.byref(oi), C.byref(od))
    assert rc == _lib.PN_ERR_INVALID


def _device(tree, qs, r, cap, sort, stream=None):
    import torch
    qd = torch.from_numpy(qs).to("cuda:0")
    torch.cuda.synchronize()  # (the call may run on another stream)
    offs, idx, dist, tot = tree.query_radius_with_distance_device(qd, r, cap, sort=sort, stream=stream)
    torch.cuda.synchronize()
    return (offs.cpu().numpy().astype(np.uint64), idx.cpu().numpy().astype(np.uint64), dist.cpu().numpy(),
            int(tot.item()))


def test_device_entry_capacities_and_stream(pn, euclid):
    import torch
    tree, pts, qs, r = euclid
    want_off, want_idx, want_d = tree.query_radius_with_distance_batch(qs, r)
    _, s_idx, s_d = tree.query_radius_with_distance_batch(qs, r, sort=True)
    total = int(want_off[-1])
    for sort, wi, wd in ((False, want_idx, want_d), (True, s_idx, s_d)):
        off, idx, dist, tot = _device(tree, qs, r, total, sort)  # exact capacity
        assert tot == total and np.array_equal(off, want_off)
        assert np.array_equal(idx[:total], wi) and dist[:total].tobytes() == wd.tobytes()
        off, _, _, tot = _device(tree, qs, r, 0, sort)  # count only
        assert tot == total and np.array_equal(off, want_off)
        cap = int(want_off[61]) + 5  # too small: offsets / total complete, every list wholly below cap in place
        off, idx, dist, tot = _device(tree, qs, r, cap, sort)
        assert tot == total and np.array_equal(off, want_off)
        whole = int(want_off[np.searchsorted(want_off, cap, side="right") - 1])
        assert np.array_equal(idx[:whole], wi[:whole]) and dist[:whole].tobytes() == wd[:whole].tobytes()
        # the straddling list: its written part holds its own entries
        assert set(idx[whole:cap].tolist()) <= set(want_idx[whole:int(want_off[np.searchsorted(want_off, cap)])].tolist())
    s = torch.cuda.Stream()
    off, idx, dist, tot = _device(tree, qs, r, total, True, stream=s.cuda_stream)
    assert tot == total and np.array_equal(idx[:total], s_idx) and dist[:total].tobytes() == s_d.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cosine_lists_and_radii(pn, oracle_mod, dtype):
    pts = uniform((6000, 16), 7201, dtype) - dtype(0.5)
    pts[10:14] = pts[3]
    qs = np.concatenate([uniform((30, 16), 7202, dtype) - dtype(0.5), pts[3:4]]).astype(dtype)
    tree = pn.BallTree.new(pts, pn.distance.Cosine())
    for r in (dtype(0.05), dtype(0.3)):
        off, _, _ = _check(pn, oracle_mod, tree, pts, qs, r, cosine=True, max_checked=2500)
        assert int(off[-1]) > 0
    off, idx, dist = tree.query_radius_with_distance_batch(qs[:2], 1.5, sort=True)  # r >= 1: the exact scan
    want_off, want_idx = tree.query_radius_batch(qs[:2], 1.5)
    assert np.array_equal(off, want_off)
    for a in range(2):
        lo, hi = int(off[a]), int(off[a + 1])
        d = _oracle_dists(oracle_mod, pts, qs[a], want_idx[lo:hi], True)
        order = _by_dist_idx(d, want_idx[lo:hi], True)
        assert np.array_equal(idx[lo:hi], want_idx[lo:hi][order]) and dist[lo:hi].tobytes() == d[order].tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiny_path(pn, oracle_mod, dtype):
    pts = uniform((600, 10), 7301, dtype)
    pts[20:24] = pts[7]
    qs = np.concatenate([uniform((8, 10), 7302, dtype), pts[7:8]]).astype(dtype)
    tree = pn.BallTree.euclidean(pts)
    _check(pn, oracle_mod, tree, pts, qs, dtype(0.6))
    off, idx, dist = tree.query_radius_with_distance_batch(qs[:2], float("inf"), sort=True)
    assert int(off[1]) == 600
    bi, bd = oracle_mod.brute_knn(pts, qs[:1], 600)
    assert np.array_equal(idx[:600], bi[0]) and dist[:600].tobytes() == bd[0].tobytes()
    i1, d1 = tree.query_radius_with_distance(qs[8], 1e-30, sort=True)  # only the duplicates at distance 0
    assert np.array_equal(i1, [7, 20, 21, 22, 23]) and not d1.any()


def _fold(pts, q):
    """the reference's sequential unfused fold and a correctly rounded sqrt, vectorised over the rows"""
    s = np.zeros(pts.shape[0], dtype=pts.dtype)
    for k in range(min(q.shape[0], pts.shape[1])):
        d = q[k] - pts[:, k]
        s = s + d * d
    return np.sqrt(s)


def test_sort_regimes_short_threshold_and_a_million_row_list(pn, oracle_mod):
    """list lengths 0, 1, 2047-2049 and 5000 (both regimes, one and several merge passes) and r = +inf over 10^6 rows"""
    import torch
    n, dim = 1 << 20, 4
    pts = uniform((n, dim), 7401, np.float32)
    pts[1000:1016] = pts[999]  # ties
    q = pts[999].copy()
    tree = pn.BallTree.euclidean(pts)
    d = _fold(pts, q)
    for a in (0, 1, 5, 77):
        assert d[a] == oracle_mod.euclidean(q, pts[a])
    order = np.lexsort((np.arange(n), d))
    ds = d[order]
    for L in (0, 1, 17, 2047, 2048, 2049, 5000):
        r = np.float32(0.0) if L == 0 else np.nextafter(ds[L - 1], np.float32(np.inf))
        want = int(np.sum(d < r))
        off, idx, dist, tot = _device(tree, q[None, :], r, want, True)
        assert tot == want
        assert np.array_equal(idx[:want], order[:want]) and dist[:want].tobytes() == ds[:want].tobytes(), L
    qd = torch.from_numpy(q[None, :]).to("cuda:0")
    offs, idx, dist, tot = tree.query_radius_with_distance_device(qd, float("inf"), n, sort=True)
    torch.cuda.synchronize()
    assert int(tot.item()) == n
    assert np.array_equal(idx.cpu().numpy(), order) and dist.cpu().numpy().tobytes() == ds.tobytes()
    offs, idx, dist, tot = tree.query_radius_with_distance_device(qd, float("inf"), n, sort=False)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), np.arange(n)) and dist.cpu().numpy().tobytes() == d.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("cosine", [False, True], ids=["euclidean", "cosine"])
def test_virtual_local_shards_equal_the_unsharded_index(pn, dtype, cosine):
    """pn_sharded_query_radius_with_distance_*: local shards spliced (unsorted) or merged by (distance, global row)
    (sorted); ties across shards (duplicated rows in different shards) ordered by the global row"""
    from petal_neighbors_amd import _lib
    pts = uniform((9000, 16), 7501, dtype) - (dtype(0.5) if cosine else dtype(0))
    pts[8500:8504] = pts[40]  # the same row in the first and the last shard
    qs = np.concatenate([uniform((40, 16), 7502, dtype) - (dtype(0.5) if cosine else dtype(0)), pts[40:41]]).astype(dtype)
    metric = pn.distance.Cosine() if cosine else None
    one = pn.BallTree.new(pts, metric) if cosine else pn.BallTree.euclidean(pts)
    _, d = one.query_batch(qs[:20], 60)
    r = dtype(np.median(d[:, 59]))
    sh = pn.ShardedIndex.from_host(pts, [0, 0, 0], metric=metric)
    sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, 1)
    for sort in (False, True):
        wo, wi, wd = one.query_radius_with_distance_batch(qs, r, sort=sort)
        go, gi, gd = sh.query_radius_with_distance_batch(qs, r, sort=sort)
        assert np.array_equal(go, wo) and np.array_equal(gi, wi) and gd.tobytes() == wd.tobytes(), sort
    lo, hi = int(wo[-2]), int(wo[-1])  # the duplicated row's query: distance-0 ties, ascending global row
    assert np.array_equal(gi[lo:lo + 5], [40, 8500, 8501, 8502, 8503])
    sh.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rank_entry_at_world_size_one_exchanges_distances(pn, dtype):
    """one process per GPU at world size 1 with the exchange forced: the distances' all-gather and the merge; the device
    form on the one-shard handle"""
    import torch
    from petal_neighbors_amd import _lib
    n = 12000
    pts = uniform((n, 24), 7601, dtype)
    pts[11000:11003] = pts[9]
    qs = np.concatenate([uniform((50, 24), 7602, dtype), pts[9:10]]).astype(dtype)
    one = pn.BallTree.euclidean(pts)
    _, d = one.query_batch(qs[:20], 40)
    r = dtype(np.median(d[:, 39]))
    sh = pn.ShardedIndex.from_rank_device(torch.from_numpy(pts).to("cuda:0"), n, 0, 1, pn.ShardedIndex.unique_id(), 0)
    sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, 1)
    for sort in (False, True):
        wo, wi, wd = one.query_radius_with_distance_batch(qs, r, sort=sort)
        go, gi, gd = sh.query_radius_with_distance_batch(qs, r, sort=sort)
        assert np.array_equal(go, wo) and np.array_equal(gi, wi) and gd.tobytes() == wd.tobytes(), sort
        total = int(wo[-1])
        qd = torch.from_numpy(qs).to("cuda:0")
        torch.cuda.synchronize()
        offs, idx, dist, tot = sh.query_radius_with_distance_device(qd, r, total, sort=sort)
        torch.cuda.synchronize()
        assert int(tot.item()) == total and np.array_equal(offs.cpu().numpy().astype(np.uint64), wo)
        assert np.array_equal(idx.cpu().numpy().astype(np.uint64), wi) and dist.cpu().numpy().tobytes() == wd.tobytes()
    sh.close()
