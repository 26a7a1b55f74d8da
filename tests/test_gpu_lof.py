"""pn_lof_* / pn_lof_score_*: the Local Outlier Factor on the device against the contract written in plain numpy.

The contract (include/petal_mi355x.h) is stated over the library's own k-NN answers, so the reference here takes
``query_self(k)`` / ``query_batch(q, k)`` as they come and does everything above them in numpy: a Python loop over the list
position t = 0 .. k - 1, vectorised over the rows, f64 throughout, ``np.maximum`` for the reachability term (a NaN operand
wins) and one addition per t, which is the sequential sum in list order.  What is compared is therefore the new code
alone.  Every score comparison is bit for bit: the NaN masks must be equal and the other values are compared as integers.
"""
import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE = 3


# ------------------------------------------------------------------------------------------------ numpy reference
def ref_fit(idx, dist, k):
    """(lof, lrd, kdist) from the self-query's answer: idx [n, k] row numbers (no index base), dist [n, k]"""
    idx = idx.astype(np.int64)
    n = len(idx)
    kdist = dist[:, k - 1].copy()
    with np.errstate(all="ignore"):
        s = np.zeros(n, dtype=np.float64)
        for t in range(k):
            v = np.maximum(np.maximum(dist[:, t].astype(np.float64), kdist[idx[:, t]].astype(np.float64)), 0.0)
            s = s + v
        lrd = 1.0 / (s / np.float64(k) + 1e-10)
        r = np.zeros(n, dtype=np.float64)
        for t in range(k):
            r = r + lrd[idx[:, t]] / lrd
        lof = r / np.float64(k)
    return lof, lrd, kdist


def ref_score(qidx, qdist, lrd, kdist, k):
    """scores of queries from their k-NN answer (row numbers, no index base) and a fit"""
    qidx = qidx.astype(np.int64)
    nq = len(qidx)
    with np.errstate(all="ignore"):
        s = np.zeros(nq, dtype=np.float64)
        for t in range(k):
            v = np.maximum(np.maximum(qdist[:, t].astype(np.float64), kdist[qidx[:, t]].astype(np.float64)), 0.0)
            s = s + v
        own = 1.0 / (s / np.float64(k) + 1e-10)
        r = np.zeros(nq, dtype=np.float64)
        for t in range(k):
            r = r + lrd[qidx[:, t]] / own
        return r / np.float64(k)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN masks differ ({int(gn.sum())} against {int(wn.sum())})"
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    bad = np.flatnonzero(got.view(u)[~gn] != want.view(u)[~wn])
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at {bad[:5]}: {got[~gn][bad[:5]]} against {want[~wn][bad[:5]]}"


def check_fit(tree, k, what):
    """lof(k, full) against the reference over query_self(k); returns (lof, lrd, kdist, idx, dist)"""
    idx, dist = tree.query_self(k)
    want = ref_fit(idx, dist, k)
    lof, lrd, kdist = tree.lof(k, full=True)
    assert lof.dtype == np.float64 and lrd.dtype == np.float64 and kdist.dtype == dist.dtype
    same_bits(kdist, dist[:, -1], what + ": kdist against the self-query's last column")
    same_bits(kdist, want[2], what + ": kdist")
    same_bits(lrd, want[1], what + ": lrd")
    same_bits(lof, want[0], what + ": lof")
    return lof, lrd, kdist, idx, dist


# the 5000 x 16 case: the smallest shape on the bf16 tier (>= 4096 rows, >= 8 columns); fitted once, shared by the tests
K5 = 10


@pytest.fixture(scope="module", params=["f32", "f64"])
def big(request, pn):
    dt = np.float32 if request.param == "f32" else np.float64
    x = uniform((5000, 16), 0x10F0, dt)
    tree = pn.BallTree.euclidean(x)
    assert tree.bf16_eligible
    idx, dist = tree.query_self(K5)
    want = ref_fit(idx, dist, K5)
    yield {"x": x, "tree": tree, "idx": idx, "dist": dist, "want": want, "dt": dt}
    tree.close()


# ---- 1. the fit
def test_fit_on_the_bf16_tier(big):
    lof, lrd, kdist = big["tree"].lof(K5, full=True)
    same_bits(kdist, big["dist"][:, -1], "kdist against the self-query's last column")
    same_bits(lrd, big["want"][1], "lrd")
    same_bits(lof, big["want"][0], "lof")
    assert np.isfinite(lof).all() and 0.8 < np.median(lof) < 1.3  # uniform data: scores around 1


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_fit_on_the_exact_scan_and_at_both_ends_of_k(pn, dt):
    x = uniform((300, 3), 0x10F1, dt)
    tree = pn.BallTree.euclidean(x)
    check_fit(tree, 5, "300 x 3, k = 5")
    tree.close()
    x = uniform((40, 5), 0x10F2, dt)
    tree = pn.BallTree.euclidean(x)
    check_fit(tree, 1, "n = 40, k = 1")
    check_fit(tree, 39, "n = 40, k = n - 1")
    with pytest.raises(ValueError):
        tree.lof(40)
    with pytest.raises(ValueError):
        tree.lof(0)
    tree.close()


# ---- 2. the optional outputs
def test_without_lrd_and_kdist_the_scores_are_the_same(big):
    same_bits(big["tree"].lof(K5), big["want"][0], "lof alone")


# ---- 3. the device entry on the caller's stream
def test_device_entry_on_a_stream(big):
    import torch
    tree, n = big["tree"], len(big["x"])
    dev = torch.device("cuda", 0)
    tdt = torch.float32 if big["dt"] == np.float32 else torch.float64
    st = torch.cuda.Stream(dev)
    lof = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    lrd = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    kdist = torch.full((n,), -7.0, dtype=tdt, device=dev)
    torch.cuda.synchronize()
    host = tree.lof(K5, full=True)
    for rep in range(2):  # a repeated call reuses the workspace
        with torch.cuda.stream(st):
            r = tree.lof_device(K5, out_lof=lof, out_lrd=lrd, out_kdist=kdist, stream=st.cuda_stream)
        st.synchronize()
        assert r[0] is lof and r[1] is lrd and r[2] is kdist
        for got, want, what in zip(r, host, ("lof", "lrd", "kdist")):
            same_bits(got.cpu().numpy(), want, "device against host: " + what)
    a, b, c = tree.lof_device(K5)  # its own outputs, the current stream
    torch.cuda.synchronize()
    same_bits(a.cpu().numpy(), big["want"][0], "lof_device, default outputs")
    same_bits(c.cpu().numpy(), big["want"][2], "lof_device, default outputs: kdist")
    with pytest.raises(ValueError):
        tree.lof_device(K5, out_lof=lof[:10])
    with pytest.raises(ValueError):
        tree.lof_device(K5, out_kdist=kdist.to(torch.float64 if tdt == torch.float32 else torch.float32))
    with pytest.raises(ValueError):
        tree.lof_device(K5, out_lrd=torch.zeros((n, 2), dtype=torch.float64, device=dev)[:, 0])


# ---- 4. planted outliers
def test_planted_outliers_hold_the_largest_scores(pn):
    rng = np.random.default_rng(4)
    centres = rng.uniform(0.0, 1.0, (4, 8))
    x = (centres[rng.integers(0, 4, 2000)] + 0.03 * rng.standard_normal((2000, 8))).astype(np.float32)
    far = np.zeros((5, 8), dtype=np.float32)
    for i in range(5):  # five rows far outside the blobs and far from each other
        far[i, i] = 6.0 + i
        far[i, 7] = -4.0
    x = np.concatenate([x, far])
    k = 15
    tree = pn.BallTree.euclidean(x)
    idx, dist = tree.query_self(k)
    want = ref_fit(idx, dist, k)[0]
    top = np.argsort(want)[-5:]
    assert sorted(top.tolist()) == [2000, 2001, 2002, 2003, 2004], top  # (a condition on the input)
    assert want[2000:].min() > 10 * want[:2000].max()
    got = tree.lof(k)
    same_bits(got, want, "blobs + 5 outliers")
    assert sorted(np.argsort(got)[-5:].tolist()) == [2000, 2001, 2002, 2003, 2004]
    tree.close()


# ---- 5. duplicates: lrd = 1e10, never inf
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_duplicate_rows_are_finite(pn, dt):
    x = uniform((500, 4), 0x10F5, dt)
    copies = np.arange(100, 500, 10)  # 40 rows
    assert len(copies) == 40
    x[copies] = x[100]
    k = 10
    tree = pn.BallTree.euclidean(x)
    lof, lrd, kdist, idx, dist = check_fit(tree, k, "40 copies among 500")
    assert np.isfinite(lof).all() and np.isfinite(lrd).all()
    assert (kdist[copies] == 0).all()
    assert (lrd[copies] == 1.0 / 1e-10).all()
    assert (lof[copies] == 1.0).all()
    tree.close()


# ---- 6. a NaN row: np.maximum's rule, not fmax's
def test_a_nan_row_scores_nan_and_so_does_every_list_that_holds_it(pn):
    x = uniform((20, 4), 0x10F6)
    x[7, 2] = np.nan
    tree = pn.BallTree.euclidean(x)
    idx, dist = tree.query_self(5)
    others = np.arange(20) != 7
    assert not (idx[others] == 7).any() and not np.isnan(dist[others]).any()  # NaN sorts last: no other list holds it
    assert np.isnan(dist[7]).all()
    lof, lrd, kdist, _, _ = check_fit(tree, 5, "one NaN row, k = 5")
    assert np.isnan(lof[7]) and np.isnan(lrd[7]) and np.isnan(kdist[7])
    assert np.isfinite(lof[others]).all()
    idx, dist = tree.query_self(19)
    assert (idx[others, -1] == 7).all()  # every list ends with it
    lof, lrd, kdist, _, _ = check_fit(tree, 19, "one NaN row, k = 19")
    assert np.isnan(lof).all() and np.isnan(lrd).all()
    assert np.isnan(kdist).all()
    tree.close()


# ---- 7. Cosine: distances a few ulp below 0 are clamped
def test_cosine_index_with_negative_distances(pn):
    x = uniform((5000, 16), 0x10F7) - np.float32(0.5)
    x[4000:4050] = x[100:150]  # 50 duplicated rows: their distance to the original is a few ulp around 0
    k = 10
    tree = pn.BallTree.new(x, pn.distance.Cosine())
    idx, dist = tree.query_self(k)
    neg = int(np.count_nonzero(dist < 0))
    print(f"cosine: {neg} negative distances in the lists, min {dist.min()}")
    assert neg >= 1  # the clamp is exercised
    want = ref_fit(idx, dist, k)
    lof, lrd, kdist = tree.lof(k, full=True)
    same_bits(kdist, dist[:, -1], "cosine: kdist")
    same_bits(lrd, want[1], "cosine: lrd")
    same_bits(lof, want[0], "cosine: lof")
    assert np.isfinite(lof).all()
    tree.close()


# ---- 8. the index base changes nothing
def test_index_base_does_not_affect_the_outputs(pn, big):
    x = big["x"]
    tree = pn.BallTree.euclidean(x)
    tree.set_option(PN_OPT_INDEX_BASE, 1000)
    idx, _ = tree.query_self(K5)
    assert idx.min() >= 1000 and np.array_equal(idx - 1000, big["idx"])
    lof, lrd, kdist = tree.lof(K5, full=True)
    for got, want, what in zip((lof, lrd, kdist), big["want"], ("lof", "lrd", "kdist")):
        same_bits(got, want, "index base 1000: " + what)
    q = uniform((200, 16), 0x10F8, big["dt"])
    plain = big["tree"].lof_score(q, K5, lrd, kdist)
    same_bits(tree.lof_score(q, K5, lrd, kdist), plain, "index base 1000: scores")
    tree.close()


# ---- 9. two pipeline chunks
def test_chunk_boundary(pn):
    n, k = (1 << 18) + 1000, 4
    x = uniform((n, 8), 0x10F9)
    tree = pn.BallTree.euclidean(x)
    lof, lrd, kdist, idx, dist = check_fit(tree, k, "2^18 + 1000 rows")
    tail = idx[1 << 18:].astype(np.int64)
    assert (tail < (1 << 18)).any()  # rows behind the boundary with neighbours before it
    assert np.isfinite(lof).all()
    tree.close()


# ---- 10. scoring new points
@pytest.fixture(scope="module")
def queries(big):
    q = uniform((3000, 16), 0x10FA, big["dt"])
    q[-1] = 10.0  # far outside the unit cube
    return q


@pytest.mark.parametrize("nq", [1, 3000])
def test_scores_of_new_points(big, queries, nq):
    import torch
    tree, (_, lrd, kdist) = big["tree"], big["want"]
    q = queries[-nq:]  # (nq = 1: the far query)
    qi, qd = tree.query_batch(q, K5)
    want = ref_score(qi, qd, lrd, kdist, K5)
    if nq > 1:
        assert np.isfinite(want).all() and want[-1] > 10 * want[:-1].max()  # (a condition on the input)
    got = tree.lof_score(q, K5, lrd, kdist)
    assert got.dtype == np.float64 and got.shape == (nq,)
    same_bits(got, want, f"lof_score, nq = {nq}")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    dq, dl, dk = torch.from_numpy(q).to(dev), torch.from_numpy(lrd).to(dev), torch.from_numpy(kdist).to(dev)
    out = torch.full((nq,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        r = tree.lof_score_device(dq, K5, dl, dk, out=out, stream=st.cuda_stream)
    st.synchronize()
    assert r is out
    same_bits(out.cpu().numpy(), want, f"lof_score_device, nq = {nq}")
    if nq > 1:
        assert got[-1] > got[:-1].max()
        with pytest.raises(ValueError):
            tree.lof_score(q, K5, lrd[:-1], kdist)
        with pytest.raises(ValueError):
            tree.lof_score_device(dq, K5, dl, dk[:-1])
        with pytest.raises(ValueError):
            tree.lof_score_device(dq, K5, dl, dk, out=out[:5])


def test_scoring_the_fitted_rows_is_not_the_fit(big):
    tree, (lof, lrd, kdist) = big["tree"], big["want"]
    q = np.ascontiguousarray(big["x"][:1000])
    qi, qd = tree.query_batch(q, K5)
    assert (qi[:, 0] == np.arange(1000)).all() and (qd[:, 0] == 0).all()  # each finds itself first
    want = ref_score(qi, qd, lrd, kdist, K5)
    same_bits(tree.lof_score(q, K5, lrd, kdist), want, "the fitted rows as queries")
    assert (want != lof[:1000]).any()


# ---- 11. statistics
def test_stats_count_the_rows_and_the_queries(big, queries):
    tree, (_, lrd, kdist) = big["tree"], big["want"]
    n = len(big["x"])
    before = tree.stats()["queries"]
    tree.lof(K5)
    assert tree.stats()["queries"] - before == n
    before = tree.stats()["queries"]
    tree.lof_score(queries[:123], K5, lrd, kdist)
    assert tree.stats()["queries"] - before == 123


# ---- 12. the C entry itself: NULL d_lrd / d_kdist place them behind the graph store
def test_device_entry_with_null_lrd_and_kdist(big):
    import ctypes as C

    import torch
    from petal_neighbors_amd import _lib
    tree, n = big["tree"], len(big["x"])
    sfx = "f32" if big["dt"] == np.float32 else "f64"
    tdt = torch.float32 if sfx == "f32" else torch.float64
    dev = torch.device("cuda", 0)
    entry = getattr(_lib.lib(), f"pn_lof_device_{sfx}")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for give_lrd, give_kdist in ((False, True), (True, False), (False, False), (True, True)):
        lof = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        lrd = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        kdist = torch.full((n,), -7.0, dtype=tdt, device=dev)
        rc = entry(tree._h, K5, 0, lof.data_ptr(), lrd.data_ptr() if give_lrd else None,
                   kdist.data_ptr() if give_kdist else None, st)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        what = f"d_lrd {'given' if give_lrd else 'NULL'}, d_kdist {'given' if give_kdist else 'NULL'}"
        same_bits(lof.cpu().numpy(), big["want"][0], what + ": lof")
        if give_lrd:
            same_bits(lrd.cpu().numpy(), big["want"][1], what + ": lrd")
        else:
            assert (lrd == -7.0).all()  # a buffer not passed is not written
        if give_kdist:
            same_bits(kdist.cpu().numpy(), big["want"][2], what + ": kdist")
        else:
            assert (kdist == -7.0).all()


# ---- 13. the argument checks that need a handle, in the documented order, through the C entries
def test_argument_errors_on_a_real_handle(pn):
    import ctypes as C

    from petal_neighbors_amd import _lib
    L = _lib.lib()
    n = 40
    buf = (C.c_double * (4 * n))()
    p = C.addressof(buf)
    t32 = pn.BallTree.euclidean(uniform((n, 5), 0x10FB, np.float32))
    t64 = pn.BallTree.euclidean(uniform((n, 5), 0x10FB, np.float64))
    one = pn.BallTree.euclidean(uniform((1, 5), 0x10FC, np.float32))

    def fit(host, sfx):
        f = getattr(L, f"pn_lof_{sfx}" if host else f"pn_lof_device_{sfx}")
        return (lambda h, k, fl, out: f(h, k, fl, out, None, None)) if host else \
               (lambda h, k, fl, out: f(h, k, fl, out, None, None, None))

    def score(host, sfx):
        f = getattr(L, f"pn_lof_score_{sfx}" if host else f"pn_lof_score_device_{sfx}")
        return (lambda h, k, fl, out: f(h, p, 1, 5, 5, k, p, p, fl, out)) if host else \
               (lambda h, k, fl, out: f(h, p, 1, 5, 5, k, p, p, fl, out, None))

    for make, null_msg in ((fit, "lof is NULL"), (score, "score_out is NULL")):
        for host in (True, False):
            for sfx, right, wrong in (("f32", t32, t64), ("f64", t64, t32)):
                call = make(host, sfx)
                # every later fault present at once: the earlier one is reported
                assert call(wrong._h, 0, 1, None) == _lib.PN_ERR_INVALID and "flags" in _lib.last_error()
                assert call(wrong._h, 0, 0, None) == _lib.PN_ERR_INVALID and null_msg in _lib.last_error()
                assert call(wrong._h, 0, 0, p) == _lib.PN_ERR_INVALID and "element type" in _lib.last_error()
                for k in (0, n, n + 1):
                    assert call(right._h, k, 0, p) == _lib.PN_ERR_INVALID
                    assert f"k must be in [1, n - 1] = [1, {n - 1}]" in _lib.last_error(), k
            for k in (0, 1, 2):  # one row: no k is valid
                assert make(host, "f32")(one._h, k, 0, p) == _lib.PN_ERR_INVALID
                assert "needs at least 2 rows" in _lib.last_error()
    with pytest.raises(ValueError):
        one.lof(1)
    for t in (t32, t64, one):
        t.close()


# ---- 14. the Python device methods refuse what is no CUDA tensor on the tree's device
def test_device_methods_refuse_host_arrays(big):
    import torch
    tree, n = big["tree"], len(big["x"])
    tdt = torch.float32 if big["dt"] == np.float32 else torch.float64
    with pytest.raises(ValueError):
        tree.lof_device(K5, out_lof=np.empty(n, dtype=np.float64))
    with pytest.raises(ValueError):
        tree.lof_device(K5, out_lrd=torch.empty(n, dtype=torch.float64))  # a CPU tensor
    with pytest.raises(ValueError):
        tree.lof_device(K5, out_kdist=np.empty(n, dtype=big["dt"]))
    dq = torch.zeros((3, 16), dtype=tdt, device="cuda:0")
    dl = torch.ones(n, dtype=torch.float64, device="cuda:0")
    dk = torch.ones(n, dtype=tdt, device="cuda:0")
    with pytest.raises(ValueError):
        tree.lof_score_device(dq, K5, dl, dk, out=np.empty(3, dtype=np.float64))
    with pytest.raises(ValueError):
        tree.lof_score_device(dq.cpu(), K5, dl, dk)
