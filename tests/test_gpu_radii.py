"""pn_query_radii_{,device_,self_,self_device_}{f32,f64}: one radius per query.  List q of a call is the single list the
scalar entry point returns for query q alone with radii[q] -- same index set, same order, bit-identical distances -- and
which tier answers a query is decided per query on the device: a batch with a few wide or odd radii keeps the others in
the first tier (pn_stats.fallback_queries grows by the listed queries only)."""
import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

MODES = [(False, False), (True, False), (True, True)]  # (with distances, nearest first): sorted lists need distances
ENTRIES = ["host", "device"]


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device(tree, qs, r, wd, sort, cap=None):
    """the device methods: (offsets, idx[:written], dist[:written] or None, total); cap None: a counting call first"""
    import torch
    qd = _up(qs)
    rd = _up(np.ascontiguousarray(r, dtype=tree.dtype)) if np.ndim(r) else r
    torch.cuda.synchronize()

    def call(c):
        if wd:
            o, i, d, t = tree.query_radius_with_distance_device(qd, rd, c, sort=sort)
        else:
            (o, i, t), d = tree.query_radius_device(qd, rd, c), None
        torch.cuda.synchronize()
        return o, i, d, int(t.item())
    if cap is None:
        cap = call(0)[3]
    o, i, d, total = call(cap)
    m = min(total, cap)
    return (o.cpu().numpy().astype(np.uint64), i.cpu().numpy().astype(np.uint64)[:m],
            d.cpu().numpy()[:m] if d is not None else None, total)


def _host(tree, qs, r, wd, sort):
    if wd:
        o, i, d = tree.query_radius_with_distance_batch(qs, r, sort=sort)
    else:
        (o, i), d = tree.query_radius_batch(qs, r), None
    return o, i, d, int(o[-1])


def _run(entry, tree, qs, r, wd, sort):
    return _host(tree, qs, r, wd, sort) if entry == "host" else _device(tree, qs, r, wd, sort)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: offsets"
    assert got[3] == want[3], f"{what}: total"
    assert np.array_equal(got[1], want[1]), f"{what}: indices"
    if want[2] is not None:
        assert got[2].tobytes() == want[2].tobytes(), f"{what}: distance bits"


def _kth_radius(tree, qs, k, dtype):
    """a radius just beyond the median k-th neighbour distance of the queries"""
    _, d = tree.query_batch(qs[:64], k)
    return dtype(np.nextafter(dtype(np.median(d[:, k - 1])), dtype(np.inf)))


# ---------------------------------------------------------------------------------------------------------------------
# 1. a constant array is the scalar call
# ---------------------------------------------------------------------------------------------------------------------
def _centered(shape, seed, dtype):
    return uniform(shape, seed, dtype) - dtype(0.5)


CONSTANT_CASES = {
    # name: (rows, dim, dtype, cosine, numbers of queries)
    "f32_200000x128": (200_000, 128, np.float32, False, (1, 257, 5000)),
    "f64_50000x32": (50_000, 32, np.float64, False, (257,)),
    "cosine_100000x64": (100_000, 64, np.float32, True, (257,)),
    "wide_16384x768": (16_384, 768, np.float32, False, (257,)),
    "small_1000x10": (1000, 10, np.float32, False, (1, 257)),
}


@pytest.mark.parametrize("case", list(CONSTANT_CASES))
def test_constant_array_equals_the_scalar_call(pn, case):
    n, dim, dtype, cosine, nqs = CONSTANT_CASES[case]
    gen = _centered if cosine else uniform
    pts = gen((n, dim), 0x7AD10000 + n, dtype)
    qall = gen((max(nqs), dim), 0x7AD20000 + n, dtype)
    tree = pn.BallTree.new(pts, pn.distance.Cosine()) if cosine else pn.BallTree.euclidean(pts)
    radii = [_kth_radius(tree, qall, 6, dtype)]
    if cosine:
        radii.append(dtype(1.0))  # r >= 1: the exact scan (half the sphere -- a handful of queries)
    for r in radii:
        for nq in nqs:
            qs = qall[:16] if (cosine and r >= 1) else qall[:nq]
            for entry in ENTRIES:
                for wd, sort in MODES:
                    want = _run(entry, tree, qs, r, wd, sort)
                    got = _run(entry, tree, qs, np.full(qs.shape[0], r, dtype=dtype), wd, sort)
                    _same(got, want, f"{case} r={r} nq={qs.shape[0]} {entry} wd={wd} sort={sort}")
                    assert want[3] > 0 or qs.shape[0] == 1
    tree.close()


def test_device_radii_tensors_are_validated_and_small_corpora_add_nothing_to_the_counter(pn):
    import torch
    pts, qs = uniform((1000, 10), 0x7AD11000), uniform((8, 10), 0x7AD12000)
    tree = pn.BallTree.euclidean(pts)
    qd = _up(qs)
    good = torch.full((8,), 0.5, dtype=torch.float32, device="cuda:0")
    bad = [good[:7], good.reshape(8, 1), good.double(), good.cpu(), torch.full((16,), 0.5, device="cuda:0")[::2]]
    if torch.cuda.device_count() > 1:
        bad.append(good.to("cuda:1"))
    for r in bad:  # length, rank, dtype, not on the GPU, strided (the call only enqueues: no temporary copy), other device
        with pytest.raises(ValueError):
            tree.query_radius_device(qd, r, 16)
        with pytest.raises(ValueError):
            tree.query_radius_with_distance_device(qd, r, 16)
    with pytest.raises(ValueError):
        tree.query_radius_self_device(good, 16)  # 8 radii for 1000 rows
    # an index below the first tier's limits answers every query by the exact scan, as the scalar call does: no query is
    # LISTED out of a filter, and fallback_queries -- the count of listed queries -- stays where it was
    before = tree.stats()["fallback_queries"]
    o, i, t = tree.query_radius_device(qd, good, 4096)
    torch.cuda.synchronize()
    assert int(t.item()) > 0 and tree.stats()["fallback_queries"] == before
    tree.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. known list lengths, some beyond what a first-tier list holds
# ---------------------------------------------------------------------------------------------------------------------
def _log_uniform_k(rng, count, kmax):
    return np.clip(np.exp(rng.uniform(0.0, np.log(kmax + 1.0), count)).astype(np.int64), 1, kmax)


def test_known_list_lengths_with_partial_overflow(pn):
    """radii[q] = the k_q-th neighbour distance of query q stepped up one ulp, k_q log-uniform in 1 .. 300: the sorted list
    is the first k_q entries of the k-NN answer.  The queries with k_q > 224 may overflow a first-tier list (224 entries per
    (segment, query)) and are then answered through the device-side exact list, the others stay in the filter:
    fallback_queries grows by fewer than nq.  (Seeds 8101 / 8102 / 8103: the CPU oracle's 301 nearest of these queries
    hold one tie at these k_q: 1 query of 2000 is skipped.)"""
    n, dim, nq, kmax = 100_000, 32, 2000, 300
    pts, qs = uniform((n, dim), 8101), uniform((nq, dim), 8102)
    tree = pn.BallTree.euclidean(pts)
    ki, kd = tree.query_batch(qs, kmax + 1)  # (its first 300 columns are the k = 300 answer; column 300 decides ties)
    kq = _log_uniform_k(np.random.default_rng(8103), nq, kmax)
    rows = np.arange(nq)
    radii = np.nextafter(kd[rows, kq - 1], np.float32(np.inf))
    tied = kd[rows, kq - 1] == kd[rows, kq]  # the (k_q + 1)-th distance equals the k_q-th: no well-defined length
    print(f"ties skipped: {int(tied.sum())} of {nq}; k_q > 224: {int((kq > 224).sum())}")
    assert tied.mean() <= 0.01
    total = int(kq[~tied].sum())
    for entry in ENTRIES:
        for wd, sort in MODES:
            before = tree.stats()["fallback_queries"]
            if entry == "host":
                off, idx, dist, _ = _host(tree, qs, radii, wd, sort)
            else:
                off, idx, dist, _ = _device(tree, qs, radii, wd, sort, cap=total + int(tied.sum()) * (kmax + 2))
            grown = tree.stats()["fallback_queries"] - before
            print(f"{entry} wd={wd} sort={sort}: fallback_queries grew by {grown} of {nq}")
            assert grown < nq, "the whole batch was rerouted to the exact scan"
            for q in np.flatnonzero(~tied):
                lo, hi = int(off[q]), int(off[q + 1])
                assert hi - lo == kq[q], (entry, wd, sort, q)
                if sort:
                    assert np.array_equal(idx[lo:hi], ki[q, :kq[q]]), (entry, q)
                    assert dist[lo:hi].tobytes() == kd[q, :kq[q]].tobytes(), (entry, q)
                else:
                    order = np.argsort(ki[q, :kq[q]])
                    assert np.array_equal(idx[lo:hi], ki[q, :kq[q]][order]), (entry, wd, q)
                    if wd:
                        assert dist[lo:hi].tobytes() == kd[q, :kq[q]][order].tobytes(), (entry, q)
    tree.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,dtype", [(200_000, 32, np.float32), (50_000, 16, np.float64)], ids=["f32", "f64"])
def test_mixed_radii_against_the_oracle(pn, oracle_mod, n, dim, dtype):
    nq = 64
    pts, qs = uniform((n, dim), 0x7AD30000 + dim, dtype), uniform((nq, dim), 0x7AD31000 + dim, dtype)
    tree = pn.BallTree.euclidean(pts)
    _, kd = tree.query_batch(qs, 300)
    kq = _log_uniform_k(np.random.default_rng(8104), nq, 300)
    radii = np.nextafter(kd[np.arange(nq), kq - 1], dtype(np.inf)).astype(dtype)
    radii[5], radii[17], radii[40] = dtype(0), dtype(np.nan), dtype(-2)
    want = [oracle_mod.brute_radius(pts, qs[a], radii[a]) for a in range(nq)]
    assert sum(w.size for w in want) > 2000 and want[5].size == want[17].size == want[40].size == 0
    for entry in ENTRIES:
        for wd, sort in MODES:
            off, idx, dist, total = _run(entry, tree, qs, radii, wd, sort)
            assert total == sum(w.size for w in want)
            for a in range(nq):
                li = idx[int(off[a]):int(off[a + 1])]
                assert np.array_equal(np.sort(li), want[a]), (entry, wd, sort, a)
                if not sort:
                    assert np.array_equal(li, want[a]), (entry, wd, a)
                if wd:
                    ld = dist[int(off[a]):int(off[a + 1])]
                    od = np.array([oracle_mod.euclidean(qs[a], pts[int(i)]) for i in li], dtype=dtype)
                    assert ld.tobytes() == od.tobytes(), (entry, sort, a)
                    if sort:
                        assert np.array_equal(np.lexsort((li, ld)), np.arange(li.size)), (entry, a)
    tree.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. edge radii inside one batch: every list is the scalar call's for that query alone
# ---------------------------------------------------------------------------------------------------------------------
def _against_single_scalar_calls(tree, qs, radii, what):
    for wd, sort in MODES:
        singles = [_host(tree, qs[a:a + 1], radii[a], wd, sort) for a in range(qs.shape[0])]
        off = np.concatenate([[0], np.cumsum([s[3] for s in singles])]).astype(np.uint64)
        idx = np.concatenate([s[1] for s in singles]).astype(np.uint64)
        dist = np.concatenate([s[2] for s in singles]) if wd else None
        want = (off, idx, dist, int(off[-1]))
        for entry in ENTRIES:
            _same(_run(entry, tree, qs, radii, wd, sort), want, f"{what} {entry} wd={wd} sort={sort}")
    return want


@pytest.fixture(scope="module")
def edge_trees(pn):
    n, dim = 20_000, 16
    pts = uniform((n, dim), 0x7AD40001)
    cpts = _centered((n, dim), 0x7AD40002, np.float32)
    te, tc = pn.BallTree.euclidean(pts), pn.BallTree.new(cpts, pn.distance.Cosine())
    yield te, pts, tc, cpts
    te.close()
    tc.close()


def test_edge_radii_euclidean(pn, oracle_mod, edge_trees):
    tree, pts, _, _ = edge_trees
    n, dim = pts.shape
    nq = 21
    qs = uniform((nq, dim), 0x7AD40003)
    normal = _kth_radius(tree, qs, 20, np.float32)
    cycle = [0.0, -1.0, np.nan, np.inf, float(np.nextafter(np.float32(0), np.float32(1))), 1e30, float(normal)]
    radii = np.array([cycle[a % len(cycle)] for a in range(nq)], dtype=np.float32)
    want = _against_single_scalar_calls(tree, qs, radii, "edge radii")
    lens = np.diff(want[0].astype(np.int64))
    # the queries whose radius the first tier cannot serve (0, -1, NaN, +inf, 1e30: r^2 beyond its range) are listed for the
    # exact scan one by one -- the denormal and the normal radius stay in the filter, their lists far below 224 entries --
    # and a call adds exactly that number to fallback_queries, the host entry point (two pipeline passes) once
    listed = sum(1 for a in range(nq) if a % len(cycle) in (0, 1, 2, 3, 5))
    for entry in ENTRIES:
        before = tree.stats()["fallback_queries"]
        if entry == "host":
            _host(tree, qs, radii, True, True)
        else:
            _device(tree, qs, radii, True, True, cap=int(want[3]))
        assert tree.stats()["fallback_queries"] - before == listed, entry
    for a in range(nq):  # what the scalar contract says, per query
        c = a % len(cycle)
        assert lens[a] == (0 if c in (0, 1, 2, 4) else n if c in (3, 5) else lens[a]), a
        if c == 6:
            assert 0 < lens[a] < n
    # a NaN query row: empty at every radius, +inf included
    qn = qs.copy()
    qn[3] = np.nan
    qn[10, 4] = np.nan
    w = _against_single_scalar_calls(tree, qn, radii, "NaN query rows")
    assert w[0][4] == w[0][3] and w[0][11] == w[0][10]
    # shorter and longer queries than the rows (zip truncation: the exact scan)
    _against_single_scalar_calls(tree, np.ascontiguousarray(qs[:, :9]), radii, "q_cols < dim")
    _against_single_scalar_calls(tree, np.concatenate([qs, qs[:, :5]], axis=1), radii, "q_cols > dim")
    # a nonzero index base
    from petal_neighbors_amd import _lib
    tree.set_option(_lib.PN_OPT_INDEX_BASE, 1_000_000)
    try:
        w = _against_single_scalar_calls(tree, qs, radii, "index base")
        assert w[1].min() >= 1_000_000
    finally:
        tree.set_option(_lib.PN_OPT_INDEX_BASE, 0)


def test_edge_radii_cosine(pn, oracle_mod, edge_trees):
    _, _, tree, pts = edge_trees
    n, dim = pts.shape
    nq = 18
    qs = _centered((nq, dim), 0x7AD40004, np.float32)
    cycle = [0.05, 0.999, 1.0, 1.5, 2.5, np.nan]
    radii = np.array([cycle[a % len(cycle)] for a in range(nq)], dtype=np.float32)
    want = _against_single_scalar_calls(tree, qs, radii, "cosine edge radii")
    off, idx, dist, _ = want  # (the last mode: sorted, with distances)
    lens = np.diff(off.astype(np.int64))
    assert all(lens[a] == 0 for a in range(5, nq, 6)) and all(lens[a] == n for a in range(4, nq, 6))
    for a in (1, 2):  # distances: Cosine::distance, bit for bit (a sample of each list)
        lo, hi = int(off[a]), int(off[a + 1])
        for e in range(lo, hi, max(1, (hi - lo) // 50)):
            assert dist[e] == oracle_mod.cosine(qs[a], pts[int(idx[e])]), (a, e)
    qn = qs.copy()
    qn[2] = np.nan
    qn[7] = 0  # no direction: every distance is NaN
    w = _against_single_scalar_calls(tree, qn, radii, "cosine NaN / zero query rows")
    assert w[0][3] == w[0][2] and w[0][8] == w[0][7]
    _against_single_scalar_calls(tree, np.ascontiguousarray(qs[:, :9]), radii, "cosine q_cols < dim")
    _against_single_scalar_calls(tree, np.concatenate([qs, qs[:, :5]], axis=1), radii, "cosine q_cols > dim")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the device entry points' capacity contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd,sort", MODES)
def test_device_capacity_contract(pn, edge_trees, wd, sort):
    import torch
    tree, pts, _, _ = edge_trees
    nq = 300
    qs = uniform((nq, pts.shape[1]), 0x7AD50001)
    _, kd = tree.query_batch(qs, 120)
    kq = _log_uniform_k(np.random.default_rng(8105), nq, 120)
    radii = np.nextafter(kd[np.arange(nq), kq - 1], np.float32(np.inf))
    radii[::50] = np.inf  # a few whole-corpus lists (the exact scan) among them
    full = _host(tree, qs, radii, wd, sort)
    total = full[3]
    assert total > 6 * pts.shape[0]
    _same(_device(tree, qs, radii, wd, sort, cap=total), full, "capacity = total")
    # capacity 0: offsets and total complete, nothing written (and no list buffers needed)
    qd, rd = _up(qs), _up(radii)
    offs = torch.empty(nq + 1, dtype=torch.int64, device="cuda:0")
    idx = torch.full((16,), -7, dtype=torch.int64, device="cuda:0")
    dist = torch.full((16,), -7.0, dtype=torch.float32, device="cuda:0")
    if wd:
        o, i, d, t = tree.query_radius_with_distance_device(qd, rd, 0, sort=sort, out_offsets=offs, out_idx=idx, out_dist=dist)
    else:
        o, i, t = tree.query_radius_device(qd, rd, 0, out_offsets=offs, out_idx=idx)
    torch.cuda.synchronize()
    assert int(t.item()) == total and np.array_equal(o.cpu().numpy().astype(np.uint64), full[0])
    assert (idx == -7).all() and (dist == -7.0).all()
    from petal_neighbors_amd import _lib
    import ctypes as C
    fn = _lib.lib().pn_query_radii_device_f32
    t2 = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    rc = fn(tree._h, qd.data_ptr(), nq, qs.shape[1], qs.shape[1], rd.data_ptr(), _lib.PN_RADIUS_SORTED if sort else 0,
            offs.data_ptr(), None, None, 0, t2.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and int(t2.item()) == total
    # half the total: offsets and total right; the prefix is the full answer's (sorted: every list wholly below the capacity,
    # the straddling one in ascending index order as far as it is written)
    cap = total // 2
    o, i, d, t = _device(tree, qs, radii, wd, sort, cap=cap)
    assert t == total and np.array_equal(o, full[0]) and i.size == cap
    if not sort:
        assert np.array_equal(i, full[1][:cap]) and (not wd or d.tobytes() == full[2][:cap].tobytes())
    else:
        whole = int(np.searchsorted(full[0], cap, side="right")) - 1
        e = int(full[0][whole])
        assert np.array_equal(i[:e], full[1][:e]) and d[:e].tobytes() == full[2][:e].tobytes()
        asc = _host(tree, qs, radii, True, False)
        assert np.array_equal(i[e:], asc[1][e:cap]) and d[e:].tobytes() == asc[2][e:cap].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 6. self-queries
# ---------------------------------------------------------------------------------------------------------------------
def _drop_self(off, idx, dist, base=0):
    """the CSR (off, idx, dist) with entry i taken out of list i"""
    n = off.size - 1
    row = np.repeat(np.arange(n, dtype=np.uint64) + np.uint64(base), np.diff(off.astype(np.int64)))
    keep = idx != row
    o = np.concatenate([[0], np.cumsum(keep)])[off.astype(np.int64)].astype(np.uint64)  # kept entries before each list
    return o, idx[keep], dist[keep] if dist is not None else None, int(o[-1])


def _self_device(tree, radii, wd, sort, include, total):
    import torch
    o, i, d, t = tree.query_radius_self_device(_up(radii), total, with_distance=wd, sort=sort, include_self=include)
    torch.cuda.synchronize()
    return (o.cpu().numpy().astype(np.uint64), i.cpu().numpy().astype(np.uint64)[:total],
            d.cpu().numpy()[:total] if d is not None else None, int(t.item()))


def test_self_radii_across_the_chunk_boundary(pn):
    """300 000 rows: two chunks of the self-query pipeline, the second starting at row 2^18 with radii + 2^18"""
    n, dim = 300_000, 8
    pts = uniform((n, dim), 0x7AD60001)
    tree = pn.BallTree.euclidean(pts)
    _, d = tree.query_batch(pts[:256], 4)
    r1 = np.float32(np.median(d[:, 3]))
    radii = np.where(np.arange(n) % 2 == 0, r1, np.float32(0.8) * r1).astype(np.float32)
    for wd, sort in MODES:
        incl = _host(tree, pts, radii, wd, sort)  # query_radii(rows, radii)
        o, i, dd = tree.query_radius_self(radii, with_distance=wd, sort=sort, include_self=True)
        _same((o, i, dd, int(o[-1])), incl, f"include_self wd={wd} sort={sort}")
        excl = _drop_self(*incl[:3])
        assert incl[3] - excl[3] == n and excl[3] > n  # every row lies within its own radius; lists are not trivial
        o, i, dd = tree.query_radius_self(radii, with_distance=wd, sort=sort)
        _same((o, i, dd, int(o[-1])), excl, f"self wd={wd} sort={sort}")
        _same(_self_device(tree, radii, wd, sort, False, excl[3]), excl, f"self device wd={wd} sort={sort}")
    _same(_self_device(tree, radii, True, True, True, incl[3]), incl, "self device include_self")
    tree.close()


def test_self_radii_from_the_core_distances(pn):
    """radii = query_self(k = 8)'s last column stepped up one ulp: every sorted list is that row of query_self"""
    n, dim, k = 20_000, 16, 8
    pts = uniform((n, dim), 0x7AD60002)
    tree = pn.BallTree.euclidean(pts)
    ki, kd = tree.query_self(k + 1)
    tied = kd[:, k - 1] == kd[:, k]
    assert tied.mean() <= 0.01
    radii = np.nextafter(kd[:, k - 1], np.float32(np.inf))
    o, i, d = tree.query_radius_self(radii, with_distance=True, sort=True)
    dev = _self_device(tree, radii, True, True, False, int(o[-1]))
    _same(dev, (o, i, d, int(o[-1])), "self device")
    ok = np.flatnonzero(~tied)
    assert np.array_equal(np.diff(o.astype(np.int64))[ok], np.full(ok.size, k))
    starts = o[:-1].astype(np.int64)[ok]
    take = starts[:, None] + np.arange(k)[None, :]
    assert np.array_equal(i[take], ki[ok, :k]) and d[take].tobytes() == kd[ok, :k].tobytes()
    tree.close()


def test_self_radii_cosine_with_nan_and_zero_rows(pn):
    n, dim = 6000, 16
    pts = _centered((n, dim), 0x7AD60003, np.float32)
    pts[9] = 0
    pts[11] = np.nan
    pts[4000, 3] = np.nan
    tree = pn.BallTree.new(pts, pn.distance.Cosine())
    _, kd = tree.query_self(3)
    radii = np.nextafter(kd[:, 2], np.float32(np.inf))  # (NaN for the rows without a direction)
    radii[::7] = 0
    radii[5::97] = np.nan
    radii[3::1500] = 1.5   # a few rows take half the sphere and more: the exact scan
    radii[8:12] = 0.9      # around the zero and the NaN row
    for wd, sort in MODES:
        incl = _host(tree, pts, radii, wd, sort)
        o, i, dd = tree.query_radius_self(radii, with_distance=wd, sort=sort, include_self=True)
        _same((o, i, dd, int(o[-1])), incl, f"cosine include_self wd={wd} sort={sort}")
        excl = _drop_self(*incl[:3])
        o, i, dd = tree.query_radius_self(radii, with_distance=wd, sort=sort)
        _same((o, i, dd, int(o[-1])), excl, f"cosine self wd={wd} sort={sort}")
        _same(_self_device(tree, radii, wd, sort, False, excl[3]), excl, f"cosine self device wd={wd} sort={sort}")
        assert excl[0][10] == excl[0][9] and excl[0][12] == excl[0][11] and excl[3] > n // 2
    tree.close()
