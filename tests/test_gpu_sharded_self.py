"""pn_sharded_query_self_* / pn_sharded_query_radius_self_*: self-queries over row shards.

The reference answer is always the single index's self-query over the same rows, bit for bit (indices, distance bits,
order), for every shard count and both ways of holding the shards; on sampled rows also the oracle's brute force with
the rule of tests/test_gpu_self_graph.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu


def _same(a_idx, a_dist, b_idx, b_dist, what):
    assert a_idx.shape == b_idx.shape, what
    assert np.array_equal(np.asarray(a_idx).astype(np.uint64), np.asarray(b_idx).astype(np.uint64)), what
    assert np.asarray(a_dist).tobytes() == np.asarray(b_dist).tobytes(), what


def _same_csr(a, b, what):
    ao, ai, ad = a
    bo, bi, bd = b
    assert np.array_equal(ao, bo), what
    assert np.array_equal(ai, bi), what
    assert (ad is None) == (bd is None), what
    if ad is not None:
        assert ad.tobytes() == bd.tobytes(), what


def _rule(idx, dist, rows):
    """drop, in each row's (k + 1)-answer, the entry equal to its own index, else the last one"""
    nq, kin = idx.shape
    own = idx == np.asarray(rows, dtype=np.uint64)[:, None]
    j = np.where(own.any(axis=1), own.argmax(axis=1), kin - 1)
    keep = np.ones_like(own)
    keep[np.arange(nq), j] = False
    return idx[keep].reshape(nq, kin - 1), dist[keep].reshape(nq, kin - 1)


def _single(pn, pts, metric=None):
    return pn.BallTree.new(pts, metric) if metric is not None else pn.BallTree.euclidean(pts)


def _check_knn(one, sh, ks, what):
    for k in ks:
        for inc in (False, True):
            _same(*sh.query_self(k, include_self=inc), *one.query_self(k, include_self=inc), f"{what} k={k} inc={inc}")


def _check_radius(one, sh, r, what, combos=((False, False), (True, False), (True, True))):
    for wd, sort in combos:
        for inc in (False, True):
            _same_csr(sh.query_radius_self(r, with_distance=wd, sort=sort, include_self=inc),
                      one.query_radius_self(r, with_distance=wd, sort=sort, include_self=inc),
                      f"{what} r={r} wd={wd} sort={sort} inc={inc}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_virtual_shards_knn(pn, oracle_mod, dtype):
    """G shards on one device (n not divisible by G), G = 1 with the exchange forced; D in {3, 16, 128}"""
    from petal_neighbors_amd import _lib
    for G, dim, n, seed in ((2, 3, 1001, 11), (3, 16, 2000, 12), (7, 128, 1500, 13), (1, 16, 999, 14)):
        pts = uniform((n, dim), seed, dtype)
        one = _single(pn, pts)
        sh = pn.ShardedIndex.from_host(pts, [0] * G)
        if G == 1:
            sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, 1)
        assert sh.local_rows == n
        _check_knn(one, sh, (1, 10), f"G={G} D={dim} {dtype.__name__}")
        # the oracle's brute force over the other rows, on sampled rows
        rows = np.sort(np.random.default_rng(seed).choice(n, 24, replace=False))
        idx, dist = sh.query_self(10)
        oi, od = oracle_mod.brute_knn(pts, pts[rows], 11)
        _same(idx[rows], dist[rows], *_rule(oi.astype(np.uint64), od, rows), f"oracle G={G} D={dim}")
        sh.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_shards_smaller_than_k(pn, dtype):
    """n = 40 over 7 shards (6 rows each, the last 4): k = 10 > a shard's rows; k >= n"""
    from petal_neighbors_amd import _lib
    pts = uniform((40, 5), 21, dtype)
    one = _single(pn, pts)
    sh = pn.ShardedIndex.from_host(pts, [0] * 7)
    _check_knn(one, sh, (10, 39, 40, 64), "n=40 G=7")
    sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, 1)  # the gathered path, k + 1 > any shard
    _check_knn(one, sh, (10, 64), "n=40 G=7 exchange")
    i, d = sh.query_self(64)
    assert i.shape == (40, 39)
    sh.close()


def test_duplicates_across_shards(pn):
    """exact twins in different shards: (distance, global row) across shards, and the right twin is dropped"""
    from petal_neighbors_amd import _lib
    pts = uniform((300, 6), 31)
    pts[150] = pts[10]
    pts[250] = pts[10]
    pts[101] = pts[99]
    one = _single(pn, pts)
    for ex in (0, 1):
        sh = pn.ShardedIndex.from_host(pts, [0] * 3)
        sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, ex)
        _check_knn(one, sh, (1, 4), f"twins ex={ex}")
        idx, dist = sh.query_self(2)
        assert list(idx[150]) == [10, 250] and list(idx[10]) == [150, 250] and list(idx[250]) == [10, 150]
        assert (dist[[10, 150, 250]] == 0).all()
        assert idx[99][0] == 101 and idx[101][0] == 99
        _check_radius(one, sh, np.float32(0.05), f"twins ex={ex}")
        sh.close()


def test_nan_rows_and_cosine(pn):
    from petal_neighbors_amd import _lib
    from petal_neighbors_amd.distance import Cosine
    pts = uniform((500, 12), 41)
    pts[5] = np.nan
    pts[260] = np.nan
    one = _single(pn, pts)
    sh = pn.ShardedIndex.from_host(pts, [0] * 3)
    _check_knn(one, sh, (3,), "nan rows")
    _check_radius(one, sh, np.float32(0.6), "nan rows", combos=((True, True),))
    sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, 1)
    _check_knn(one, sh, (3,), "nan rows exchange")
    sh.close()
    x = uniform((700, 20), 42) - np.float32(0.5)
    x[7] = 0  # a row without a direction: NaN against everything
    x[400] = x[3] * np.float32(2)  # same direction in another shard
    for dtype in (np.float32, np.float64):
        xd = x.astype(dtype)
        one = _single(pn, xd, Cosine())
        sh = pn.ShardedIndex.from_host(xd, [0] * 4, metric=Cosine())
        _check_knn(one, sh, (1, 8), f"cosine {dtype.__name__}")
        _check_radius(one, sh, dtype(0.2), f"cosine {dtype.__name__}")
        sh.close()


def test_more_than_one_step(pn):
    """n > 2^18: two steps, a step's rows spanning both shards; in place and gathered"""
    from petal_neighbors_amd import _lib
    pts = uniform((300000, 8), 51)
    one = _single(pn, pts)
    want = one.query_self(4)
    sh = pn.ShardedIndex.from_host(pts, [0, 0])
    _same(*sh.query_self(4), *want, "two steps in place")
    sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, 1)
    _same(*sh.query_self(4), *want, "two steps gathered")
    r = np.float32(0.08)
    _same_csr(sh.query_radius_self(r, with_distance=True, sort=True), one.query_radius_self(r, with_distance=True, sort=True),
              "two steps radius")
    sh.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rank_entry_at_world_size_one(pn, dtype):
    """one process per GPU at world size 1 with the exchange forced: the rows' all-gather, the packed all-gather and the
    slice merge; the device entry on a non-default stream"""
    import torch
    from petal_neighbors_amd import _lib
    n = 12000
    pts = uniform((n, 24), 61, dtype)
    pts[11000] = pts[17]
    one = _single(pn, pts)
    sh = pn.ShardedIndex.from_rank_device(torch.from_numpy(pts).to("cuda:0"), n, 0, 1, pn.ShardedIndex.unique_id(), 0)
    sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, 1)
    _check_knn(one, sh, (1, 10), "rank host")
    s = torch.cuda.Stream(device=0)
    for inc in (False, True):
        torch.cuda.synchronize()
        di, dd = sh.query_self_device(10, include_self=inc, stream=s.cuda_stream)
        s.synchronize()
        _same(di.cpu().numpy(), dd.cpu().numpy(), *one.query_self(10, include_self=inc), f"rank device inc={inc}")
    _, d = one.query_self(20)
    _check_radius(one, sh, dtype(np.median(d[:, 19])), "rank radius")
    sh.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rank_radius_and_self_radius_share_one_handle(pn, dtype):
    """query_radius over a batch and query_radius_self go through ONE ragged exchange (rank_radius_exchange) and its
    buffers: in turn on one rank handle at world size 1 with the exchange forced, each answer the single index's bit for
    bit.  (a) overflows the starting capacity 40 x 4 + 1024 and re-runs, (b) fits and reuses the grown buffers, (c) is
    the self-query's longer record and its own capacity, (d) is (a) again after it.
    Not verified here: a rank that fails (the status word's failing branch needs a second rank)."""
    import torch
    from petal_neighbors_amd import _lib
    n, nq = 3000, 40
    pts = uniform((n, 8), 91, dtype)
    qs = uniform((nq, 8), 92, dtype)
    one = _single(pn, pts)
    _, d = one.query_batch(qs, 40)
    r_a, r_b = dtype(np.median(d[:, 39])), dtype(np.median(d[:, 4]))
    _, ds = one.query_self(20)
    r_c = dtype(np.median(ds[:, 19]))
    sh = pn.ShardedIndex.from_rank_device(torch.from_numpy(pts).to("cuda:0"), n, 0, 1, pn.ShardedIndex.unique_id(), 0)
    sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, 1)

    def call_a(what):
        want = one.query_radius_with_distance_batch(qs, r_a, sort=True)
        assert int(want[0][-1]) > nq * 4 + 1024, "the first attempt must overflow"
        _same_csr(sh.query_radius_with_distance_batch(qs, r_a, sort=True), want, what)

    call_a("(a) sorted with distances, retried")
    wo, wi = one.query_radius_batch(qs, r_b)
    assert 0 < int(wo[-1]) <= nq * 4 + 1024, "the second call must fit"
    go, gi = sh.query_radius_batch(qs, r_b)
    _same_csr((go, gi, None), (wo, wi, None), "(b) rows only, fits")
    _same_csr(sh.query_radius_self(r_c, with_distance=True, sort=True), one.query_radius_self(r_c, with_distance=True, sort=True),
              "(c) self, sorted with distances")
    call_a("(d) as (a), after the self-query")
    sh.close()


def test_radius_flags_and_edges(pn):
    from petal_neighbors_amd import _lib
    pts = uniform((3000, 10), 71)
    one = _single(pn, pts)
    _, d = one.query_self(30)
    r = np.float32(np.median(d[:, 29]))
    for G in (2, 5):
        sh = pn.ShardedIndex.from_host(pts, [0] * G)
        for ex in (0, 1):
            sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, ex)
            _check_radius(one, sh, r, f"G={G} ex={ex}")
            for rr in (np.float32(0), np.float32(-1)):
                o, i, dd = sh.query_radius_self(rr, with_distance=True)
                assert int(o[-1]) == 0 and o.shape == (3001,)
        sh.close()
    small = uniform((300, 4), 72)
    one = _single(pn, small)
    sh = pn.ShardedIndex.from_host(small, [0] * 3)
    _check_radius(one, sh, np.float32(np.inf), "r=inf")
    sh.close()
    # lists longer than one sort tile (2048 entries) under PN_RADIUS_SORTED
    big = uniform((2600, 3), 73)
    one = _single(pn, big)
    sh = pn.ShardedIndex.from_host(big, [0] * 2)
    for ex in (0, 1):
        sh.set_option(_lib.PN_OPT_EXCHANGE_ALWAYS, ex)
        _same_csr(sh.query_radius_self(np.float32(np.inf), with_distance=True, sort=True),
                  one.query_radius_self(np.float32(np.inf), with_distance=True, sort=True), f"long sorted ex={ex}")
    sh.close()


def test_device_radius_forwards_on_one_shard_and_element_type(pn):
    import torch
    from petal_neighbors_amd import _lib
    from petal_neighbors_amd.errors import PetalError
    pts = uniform((2000, 8), 81)
    one = _single(pn, pts)
    r = np.float32(0.2)
    want = one.query_radius_self(r, with_distance=True, sort=True)
    cap = int(want[0][-1])
    sh = pn.ShardedIndex.from_host(pts, [0])
    torch.cuda.synchronize()
    offs, idx, dist, tot = sh.query_radius_self_device(r, cap, with_distance=True, sort=True)
    torch.cuda.synchronize()
    assert int(tot.item()) == cap
    _same_csr((offs.cpu().numpy().astype(np.uint64), idx.cpu().numpy().astype(np.uint64), dist.cpu().numpy()), want,
              "device radius, one shard")
    sh.close()
    sh = pn.ShardedIndex.from_host(pts, [0, 0])
    with pytest.raises(PetalError):
        sh.query_radius_self_device(r, cap, with_distance=True)
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    assert L.pn_sharded_query_radius_self_device_f32(sh._h, C.c_float(r), 0, C.addressof(buf), C.addressof(buf), None, 4,
                                                     None, None) == _lib.PN_ERR_UNSUPPORTED
    # the element type is the handle's
    i64, f64 = np.empty((2000, 3), dtype=np.uint64), np.empty((2000, 3), dtype=np.float64)
    assert L.pn_sharded_query_self_f64(sh._h, 3, 0, i64.ctypes.data, f64.ctypes.data) == _lib.PN_ERR_INVALID
    assert "element type" in _lib.last_error()
    off = np.zeros(2001, dtype=np.uint64)
    oi = C.c_void_p(0)
    assert L.pn_sharded_query_radius_self_f64(sh._h, C.c_double(0.2), 0, off.ctypes.data, C.byref(oi), None) \
        == _lib.PN_ERR_INVALID
    sh.close()
