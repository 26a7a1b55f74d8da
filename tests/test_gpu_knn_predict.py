"""pn_knn_classify_* / pn_knn_regress_*: k-NN classification and regression on the device against the contract written in
plain NumPy (tests/knn_predict_reference.py).

The contract (include/petal_mi355x.h) is stated over the library's own k-NN answers, so the reference takes
``query_batch(q, k)`` / ``query_self(k)`` as they come and does the vote and the mean above them: what is compared is the
new code alone.  Every comparison of ``proba`` and of the regression outputs is bit for bit (equal NaN masks, the rest as
integers); ``pred`` is compared exactly.  The shapes are the smallest at which each path can go wrong.
"""
import ctypes as C

import numpy as np
import pytest

import knn_predict_reference as ref
from conftest import uniform
from knn_predict_reference import same_bits

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE = 3
WEIGHTINGS = ("uniform", "distance")


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def predict(tree, q, k, codes, n_classes, y, weights, via):
    """``(pred, proba, out)`` as NumPy arrays, ``q`` None: the indexed rows; through the host or the device methods"""
    import torch
    if via == "host":
        if q is None:
            pred, proba, classes = tree.knn_classify_self(k, codes, weights, proba=True)
            out = tree.knn_regress_self(k, y, weights)
        else:
            pred, proba, classes = tree.knn_classify(q, k, codes, weights, proba=True)
            out = tree.knn_regress(q, k, y, weights)
        assert np.array_equal(classes, np.arange(n_classes))  # (every class occurs: the codes are their own classes)
        return pred, proba, out
    dl, dy = cuda(codes), cuda(y)
    if q is None:
        pred, proba = tree.knn_classify_self_device(k, dl, n_classes, weights, proba=True)
        out = tree.knn_regress_self_device(k, dy, weights)
    else:
        dq = cuda(q)
        pred, proba = tree.knn_classify_device(dq, k, dl, n_classes, weights, proba=True)
        out = tree.knn_regress_device(dq, k, dy, weights)
    torch.cuda.synchronize()
    return pred.cpu().numpy(), proba.cpu().numpy(), out.cpu().numpy()


def check(tree, q, k, codes, n_classes, y, what, via="device", weightings=WEIGHTINGS, lists=None):
    """both outputs under both weightings against the reference over the library's own lists; returns the lists"""
    idx, dist = lists if lists is not None else (tree.query_self(k) if q is None else tree.query_batch(q, k))
    assert idx.shape[1] == k
    for weights in weightings:
        d = weights == "distance"
        want_pred, want_proba = ref.classify(idx, dist, codes, n_classes, d)
        want_out = ref.regress(idx, dist, y, d)
        pred, proba, out = predict(tree, q, k, codes, n_classes, y, weights, via)
        tag = f"{what}, {weights}, {via}"
        assert pred.dtype == np.int64 and np.array_equal(pred, want_pred), tag + ": pred"
        same_bits(proba, want_proba, tag + ": proba")
        same_bits(out, want_out, tag + ": regression")
    return idx, dist


def data(n, seed, n_classes, n_out):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_classes, n).astype(np.int64), rng.standard_normal((n, n_out))


# the 5000 x 16 case: the smallest shape on the bf16 tier (>= 4096 rows, >= 8 columns); built once, shared by the tests
K5, C5 = 10, 7


@pytest.fixture(scope="module", params=["f32", "f64"])
def big(request, pn):
    dt = np.float32 if request.param == "f32" else np.float64
    x = uniform((5000, 16), 0x4E01, dt)
    q = uniform((3000, 16), 0x4E02, dt)
    tree = pn.BallTree.euclidean(x)
    assert tree.bf16_eligible
    codes, y = data(5000, 0x4E03, C5, 70)
    yield {"x": x, "q": q, "tree": tree, "codes": codes, "y": y, "dt": dt, "sfx": request.param,
           "lists": tree.query_batch(q, K5), "self_lists": tree.query_self(K5)}
    tree.close()


# ---- 1. the bf16 tier: new points and the rows themselves, every output
@pytest.mark.parametrize("via", ["host", "device"])
@pytest.mark.parametrize("n_out", [1, 3, 70])
def test_bf16_tier(big, via, n_out):
    y = np.ascontiguousarray(big["y"][:, :n_out])
    check(big["tree"], big["q"], K5, big["codes"], C5, y, f"5000 x 16, n_out = {n_out}", via, lists=big["lists"])
    check(big["tree"], None, K5, big["codes"], C5, y, f"5000 x 16 self, n_out = {n_out}", via, lists=big["self_lists"])


# ---- 2. the exact scan and both ends of k
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_exact_scan_and_both_ends_of_k(pn, dt):
    x, q = uniform((300, 3), 0x4E10, dt), uniform((50, 3), 0x4E11, dt)
    codes, y = data(300, 0x4E12, 4, 2)
    tree = pn.BallTree.euclidean(x)
    check(tree, q, 5, codes, 4, y, "300 x 3, k = 5", "host")
    check(tree, None, 5, codes, 4, y, "300 x 3 self, k = 5", "host")
    tree.close()
    x, q = uniform((40, 5), 0x4E13, dt), uniform((9, 5), 0x4E14, dt)
    codes, y = data(40, 0x4E15, 3, 1)
    tree = pn.BallTree.euclidean(x)
    for k in (1, 40):
        check(tree, q, k, codes, 3, y, f"n = 40, k = {k}", "host")
    for k in (1, 39):
        check(tree, None, k, codes, 3, y, f"n = 40 self, k = {k}", "device")
    for k in (0, 41):
        with pytest.raises(ValueError):
            tree.knn_classify(q, k, codes)
        with pytest.raises(ValueError):
            tree.knn_regress(q, k, y)
    for k in (0, 40):
        with pytest.raises(ValueError):
            tree.knn_classify_self(k, codes)
        with pytest.raises(ValueError):
            tree.knn_regress_self(k, y)
    tree.close()


# ---- 3. every group width, the LDS path, the limit
@pytest.fixture(scope="module")
def wide(pn):
    x, q = uniform((1100, 4), 0x4E20), uniform((64, 4), 0x4E21)
    codes, y = data(1100, 0x4E22, 5, 3)
    tree = pn.BallTree.euclidean(x)
    yield {"tree": tree, "q": q, "codes": codes, "y": y}
    tree.close()


@pytest.mark.parametrize("k", [2, 33, 64, 65, 200, 1024])
def test_group_widths_and_the_lds_path(wide, k):
    tree, q, codes, y = wide["tree"], wide["q"], wide["codes"], wide["y"]
    check(tree, q, k, codes, 5, y, f"1100 x 4, k = {k}")
    check(tree, q, k, codes, 5, np.ascontiguousarray(y[:, :2]), f"1100 x 4, k = {k}, n_out = 2", weightings=("distance",))
    if k in (33, 65, 200):
        check(tree, None, k, codes, 5, np.ascontiguousarray(y[:, :1]), f"1100 x 4 self, k = {k}", weightings=("distance",))


def test_k_above_the_limit_is_unsupported(wide):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    tree, q, codes, y = wide["tree"], wide["q"], wide["codes"], np.ascontiguousarray(wide["y"][:, :1])
    pred, out = np.zeros(1100, dtype=np.int64), np.zeros(1100)
    calls = [lambda k: L.pn_knn_classify_f32(tree._h, q.ctypes.data, 64, 4, 4, k, codes.ctypes.data, 5, 0, pred.ctypes.data, None),
             lambda k: L.pn_knn_classify_self_f32(tree._h, k, codes.ctypes.data, 5, 1, pred.ctypes.data, None),
             lambda k: L.pn_knn_regress_f32(tree._h, q.ctypes.data, 64, 4, 4, k, y.ctypes.data, 1, 1, out.ctypes.data),
             lambda k: L.pn_knn_regress_self_f32(tree._h, k, y.ctypes.data, 1, 0, out.ctypes.data)]
    for call in calls:
        assert call(1025) == _lib.PN_ERR_UNSUPPORTED and "1024" in _lib.last_error()
        assert call(1099) == _lib.PN_ERR_UNSUPPORTED
    assert calls[0](1101) == _lib.PN_ERR_INVALID and calls[1](1100) == _lib.PN_ERR_INVALID  # the range comes first


# ---- 4. ties go to the smaller class
def test_ties(pn):
    x = np.zeros((12, 2), dtype=np.float32)
    x[:, 0] = np.arange(12)
    codes = (np.arange(12) % 2).astype(np.int64)  # alternating: any 4 consecutive rows hold each class twice
    q = np.array([[1.5, 0.0], [6.5, 0.0], [9.5, 0.0]], dtype=np.float32)
    y = np.arange(12, dtype=np.float64)[:, None]
    tree = pn.BallTree.euclidean(x)
    idx, _ = check(tree, q, 4, codes, 2, y, "alternating labels, k = 4")
    assert (np.sort(codes[idx.astype(np.int64)], axis=1) == [0, 0, 1, 1]).all()  # (a condition on the input)
    pred, proba, _ = predict(tree, q, 4, codes, 2, y, "uniform", "device")
    assert pred.tolist() == [0, 0, 0] and (proba == 0.5).all()
    tree.close()
    # two rows of different classes at exactly the same distance, the larger class first in the list
    x = np.array([[-1.0, 0.25], [1.0, 0.25], [9.0, 9.0], [-9.0, 9.0]], dtype=np.float32)
    codes = np.array([1, 0, 0, 1], dtype=np.int64)
    q = np.zeros((1, 2), dtype=np.float32)
    tree = pn.BallTree.euclidean(x)
    idx, dist = tree.query_batch(q, 2)
    assert idx.tolist() == [[0, 1]] and dist[0, 0].tobytes() == dist[0, 1].tobytes() and dist[0, 0] > 0
    for weights in WEIGHTINGS:
        pred, proba, _ = predict(tree, q, 2, codes, 2, np.ones((4, 1)), weights, "device")
        assert pred.tolist() == [0], weights
        same_bits(proba, np.array([[0.5, 0.5]]), "equal distances: proba, " + weights)
    tree.close()


# ---- 5. zero distances: under distance weights only they count
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_zero_distances(pn, dt):
    x = uniform((500, 4), 0x4E50, dt)
    copies = np.arange(100, 500, 10)  # 40 rows
    x[copies] = x[100]
    codes, y = data(500, 0x4E51, 3, 2)
    rows = np.concatenate([copies[:6], [3, 7, 255]])
    q = np.ascontiguousarray(x[rows])
    k = 10
    tree = pn.BallTree.euclidean(x)
    idx, dist = check(tree, q, k, codes, 3, y, "queries that copy rows")
    idx = idx.astype(np.int64)
    assert (dist[:6] == 0).all() and np.isin(idx[:6], copies).all()  # ten of the forty copies, at distance 0
    assert (idx[6:, 0] == [3, 7, 255]).all() and (dist[6:, 0] == 0).all() and (dist[6:, 1] > 0).all()
    pred, proba, out = predict(tree, q, k, codes, 3, y, "distance", "device")
    assert np.isfinite(proba).all() and np.isfinite(out).all()
    counts = np.stack([(codes[idx[:6]] == c).sum(axis=1) for c in range(3)], axis=1)
    same_bits(proba[:6], counts / np.float64(k), "sums of 1.0 weights are exact")
    mean = np.zeros((6, 2))
    for t in range(k):
        mean = mean + y[idx[:6, t]]
    same_bits(out[:6], mean / np.float64(k), "the mean of the duplicates' targets in list order")
    assert (proba[6:].max(axis=1) == 1.0).all() and (pred[6:] == codes[[3, 7, 255]]).all()  # the row itself alone
    same_bits(out[6:], y[[3, 7, 255]], "a single zero distance: that row's targets")
    check(tree, None, k, codes, 3, y, "duplicated rows, self")
    tree.close()


# ---- 6. NaN: a poisoned list answers -1 and NaN rows, the others are untouched
def test_nan_queries_and_nan_rows(pn):
    x, q = uniform((300, 4), 0x4E60), uniform((33, 4), 0x4E61)
    q[5, 1] = np.nan
    q[32, 0] = np.nan
    codes, y = data(300, 0x4E62, 4, 3)
    tree = pn.BallTree.euclidean(x)
    idx, dist = check(tree, q, 6, codes, 4, y, "two NaN queries")
    assert np.isnan(dist[[5, 32]]).all() and not np.isnan(np.delete(dist, [5, 32], axis=0)).any()
    for weights in WEIGHTINGS:
        pred, proba, out = predict(tree, q, 6, codes, 4, y, weights, "device")
        assert (pred[[5, 32]] == -1).all() and np.isnan(proba[[5, 32]]).all() and np.isnan(out[[5, 32]]).all()
        keep = np.delete(np.arange(33), [5, 32])
        assert (pred[keep] >= 0).all() and np.isfinite(proba[keep]).all() and np.isfinite(out[keep]).all()
    tree.close()
    x = uniform((20, 4), 0x4E63)
    x[7, 2] = np.nan
    codes, y = data(20, 0x4E64, 2, 1)
    q = uniform((4, 4), 0x4E65)
    tree = pn.BallTree.euclidean(x)
    idx, dist = check(tree, q, 20, codes, 2, y, "a NaN row, k = n")
    assert (idx[:, -1] == 7).all() and np.isnan(dist[:, -1]).all()  # every list ends with it
    for weights in WEIGHTINGS:
        pred, proba, out = predict(tree, q, 20, codes, 2, y, weights, "device")
        assert (pred == -1).all() and np.isnan(proba).all() and np.isnan(out).all()
        pred, proba, out = predict(tree, None, 19, codes, 2, y, weights, "device")
        assert (pred == -1).all() and np.isnan(proba).all() and np.isnan(out).all()
    idx, dist = check(tree, q, 5, codes, 2, y, "a NaN row, k = 5")  # NaN sorts last: no short list holds it
    assert not (idx == 7).any()
    tree.close()


# ---- 7. labels out of range
def test_labels_out_of_range(big):
    import torch
    from petal_neighbors_amd import _lib
    tree, q, sfx = big["tree"], big["q"], big["sfx"]
    idx, dist = big["lists"]
    r, r2 = int(idx[17, 3]), int(idx[400, 0])
    assert r != r2
    bad = big["codes"].copy()
    bad[r], bad[r2] = C5, -1
    pred, proba = np.zeros(len(q), dtype=np.int64), np.zeros((len(q), C5))
    host = getattr(_lib.lib(), f"pn_knn_classify_{sfx}")
    for flags in (0, 1):
        rc = host(tree._h, q.ctypes.data, len(q), 16, 16, K5, bad.ctypes.data, C5, flags, pred.ctypes.data, proba.ctypes.data)
        first, value = (r, C5) if r < r2 else (r2, -1)
        assert rc == _lib.PN_ERR_INVALID and f"labels[{first}] = {value}" in _lib.last_error()
    rc = getattr(_lib.lib(), f"pn_knn_classify_self_{sfx}")(tree._h, K5, bad.ctypes.data, C5, 0, pred.ctypes.data, None)
    assert rc == _lib.PN_ERR_INVALID and "labels[" in _lib.last_error()
    hit = ((idx == r) | (idx == r2)).any(axis=1)
    assert 2 <= hit.sum() < len(q) // 2
    dq, dl = cuda(q), cuda(bad)
    for weights in WEIGHTINGS:
        want_pred, want_proba = ref.classify(idx, dist, big["codes"], C5, weights == "distance")
        pred, proba = tree.knn_classify_device(dq, K5, dl, C5, weights, proba=True)
        torch.cuda.synchronize()
        pred, proba = pred.cpu().numpy(), proba.cpu().numpy()
        assert np.array_equal(pred == -1, hit), weights
        assert np.isnan(proba[hit]).all()
        assert np.array_equal(pred[~hit], want_pred[~hit])
        same_bits(proba[~hit], want_proba[~hit], "the lists without the bad rows, " + weights)
        ref_pred, ref_proba = ref.classify(idx, dist, bad, C5, weights == "distance")
        assert np.array_equal(pred, ref_pred)
        same_bits(proba, ref_proba, "the reference with the bad labels, " + weights)


# ---- 8. many classes, one class, no proba buffer
def test_many_classes(big):
    import torch
    from petal_neighbors_amd import _lib
    tree, q, n, sfx = big["tree"], big["q"], 5000, big["sfx"]
    idx, dist = big["lists"]
    dq = cuda(q)
    pred = tree.knn_classify_device(dq, K5, cuda(np.arange(n, dtype=np.int64)), n)
    # no proba buffer: pred is written, and nothing behind it (the guard region of the same allocation keeps its fill)
    guarded = torch.full((len(q) + 4096,), -7, dtype=torch.int64, device="cuda:0")
    out, guard = guarded[:len(q)], guarded[len(q):]
    ones = cuda(np.zeros(n, dtype=np.int64))
    rc = getattr(_lib.lib(), f"pn_knn_classify_device_{sfx}")(
        tree._h, dq.data_ptr(), len(q), 16, 16, K5, ones.data_ptr(), 1, 1, out.data_ptr(), None,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(pred.cpu().numpy(), idx.astype(np.int64).min(axis=1))  # every class once: the smallest id
    assert (out == 0).all() and (guard == -7).all()
    for weights in WEIGHTINGS:
        pred, proba = tree.knn_classify_device(dq, K5, ones, 1, weights, proba=True)
        torch.cuda.synchronize()
        assert (pred == 0).all() and proba.shape == (len(q), 1)
        if weights == "uniform":
            assert (proba == 1.0).all()
        same_bits(proba.cpu().numpy(), ref.classify(idx, dist, np.zeros(n, dtype=np.int64), 1, weights == "distance")[1],
                  "one class, " + weights)
    codes = np.random.default_rng(0x4E80).integers(0, 300, n).astype(np.int64)
    for weights in WEIGHTINGS:
        want_pred, want_proba = ref.classify(idx, dist, codes, 300, weights == "distance")
        pred, proba = tree.knn_classify_device(dq, K5, cuda(codes), 300, weights, proba=True)
        torch.cuda.synchronize()
        assert np.array_equal(pred.cpu().numpy(), want_pred)
        same_bits(proba.cpu().numpy(), want_proba, "300 classes, " + weights)


# ---- 9. Cosine: distances a few ulp below 0 are clamped, and then count as zero distances
def test_cosine_index_with_negative_distances(pn):
    x = uniform((5000, 16), 0x4E90) - np.float32(0.5)
    x[4000:4050] = x[100:150]  # 50 duplicated rows: their distance to the original is a few ulp around 0
    codes, y = data(5000, 0x4E91, 4, 2)
    tree = pn.BallTree.new(x, pn.distance.Cosine())
    lists = tree.query_self(K5)
    neg = int(np.count_nonzero(lists[1] < 0))
    print(f"cosine: {neg} negative distances in the lists, min {lists[1].min()}")
    assert neg >= 1  # the clamp is exercised
    check(tree, None, K5, codes, 4, y, "cosine self", lists=lists)
    q = np.ascontiguousarray(x[90:160])
    check(tree, q, K5, codes, 4, y, "cosine, rows as queries")
    tree.close()


# ---- 10. the index base changes nothing
def test_index_base_does_not_affect_the_outputs(pn, big):
    tree = pn.BallTree.euclidean(big["x"])
    tree.set_option(PN_OPT_INDEX_BASE, 1000)
    idx, _ = tree.query_batch(big["q"][:100], K5)
    assert idx.min() >= 1000 and np.array_equal(idx - 1000, big["lists"][0][:100])
    y = np.ascontiguousarray(big["y"][:, :3])
    for weights in WEIGHTINGS:
        for q in (big["q"], None):
            plain = predict(big["tree"], q, K5, big["codes"], C5, y, weights, "host")
            based = predict(tree, q, K5, big["codes"], C5, y, weights, "host")
            assert np.array_equal(plain[0], based[0])
            same_bits(based[1], plain[1], "index base 1000: proba")
            same_bits(based[2], plain[2], "index base 1000: regression")
    tree.close()


# ---- 11. two pipeline chunks
def test_chunk_boundary_of_the_queries(pn):
    n, nq = 4096, (1 << 18) + 1000
    x, q = uniform((n, 8), 0x4EB0), uniform((nq, 8), 0x4EB1)
    codes, y = data(n, 0x4EB2, 7, 2)
    tree = pn.BallTree.euclidean(x)
    check(tree, q, 3, codes, 7, y, "2^18 + 1000 queries")
    tree.close()


def test_chunk_boundary_of_the_rows(pn):
    n = (1 << 18) + 1000
    x = uniform((n, 8), 0x4EB3)
    codes, y = data(n, 0x4EB4, 7, 2)
    tree = pn.BallTree.euclidean(x)
    idx, _ = check(tree, None, 4, codes, 7, y, "2^18 + 1000 rows, self")
    assert (idx[1 << 18:].astype(np.int64) < (1 << 18)).any()  # rows behind the boundary with neighbours before it
    tree.close()


# ---- 12. the device entries on the caller's stream
def test_device_entries_on_a_stream(big):
    import torch
    tree, q, codes = big["tree"], big["q"], big["codes"]
    y = np.ascontiguousarray(big["y"][:, :3])
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    dq, dl, dy = cuda(q), cuda(codes), cuda(y)
    nq, n = len(q), len(codes)
    want = predict(tree, q, K5, codes, C5, y, "distance", "host")
    want_self = predict(tree, None, K5, codes, C5, y, "distance", "host")
    pred = torch.full((nq,), -7, dtype=torch.int64, device=dev)
    proba = torch.full((nq, C5), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((nq, 3), -7.0, dtype=torch.float64, device=dev)
    spred = torch.full((n,), -7, dtype=torch.int64, device=dev)
    sout = torch.full((n, 3), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for rep in range(2):  # a repeated call reuses the workspace
        with torch.cuda.stream(st):
            r = tree.knn_classify_device(dq, K5, dl, C5, "distance", True, out_pred=pred, out_proba=proba, stream=st.cuda_stream)
            o = tree.knn_regress_device(dq, K5, dy, "distance", out=out, stream=st.cuda_stream)
            sp = tree.knn_classify_self_device(K5, dl, C5, "distance", out_pred=spred, stream=st.cuda_stream)
            so = tree.knn_regress_self_device(K5, dy, "distance", out=sout, stream=st.cuda_stream)
        st.synchronize()
        assert r[0] is pred and r[1] is proba and o is out and sp is spred and so is sout
        assert np.array_equal(pred.cpu().numpy(), want[0]) and np.array_equal(spred.cpu().numpy(), want_self[0])
        same_bits(proba.cpu().numpy(), want[1], "device against host: proba")
        same_bits(out.cpu().numpy(), want[2], "device against host: regression")
        same_bits(sout.cpu().numpy(), want_self[2], "device against host: self regression")
    a = tree.knn_regress_device(dq, K5, dy[:, 0].contiguous(), "distance")  # default output, 1-D targets, current stream
    torch.cuda.synchronize()
    assert a.shape == (nq,)
    same_bits(a.cpu().numpy(), ref.regress(*big["lists"], y[:, :1], True)[:, 0], "1-D targets on the device")
    tdt = torch.float32 if big["dt"] == np.float32 else torch.float64
    other = torch.float64 if tdt == torch.float32 else torch.float32
    refused = [
        lambda: tree.knn_classify_device(dq, K5, dl, C5, out_pred=pred[:10]),
        lambda: tree.knn_classify_device(dq, K5, dl, C5, out_pred=pred.to(torch.int32)),
        lambda: tree.knn_classify_device(dq, K5, dl, C5, proba=True, out_proba=proba[:, :3]),
        lambda: tree.knn_classify_device(dq, K5, dl, C5, proba=True, out_proba=proba.cpu()),
        lambda: tree.knn_classify_device(dq, K5, dl, C5, out_proba=proba),       # without proba=True
        lambda: tree.knn_classify_device(dq, K5, dl[:-1], C5),
        lambda: tree.knn_classify_device(dq, K5, dl.to(torch.int32), C5),
        lambda: tree.knn_classify_device(dq, K5, codes, C5),                      # a host array
        lambda: tree.knn_classify_device(dq.to(other), K5, dl, C5),
        lambda: tree.knn_classify_device(q, K5, dl, C5),
        lambda: tree.knn_classify_self_device(K5, dl.cpu(), C5),
        lambda: tree.knn_classify_self_device(K5, dl, C5, out_pred=spred[:-1]),
        lambda: tree.knn_regress_device(dq, K5, dy, out=out[:, :2]),
        lambda: tree.knn_regress_device(dq, K5, dy.to(torch.float32)),
        lambda: tree.knn_regress_device(dq, K5, dy[:-1]),
        lambda: tree.knn_regress_device(dq, K5, y),
        lambda: tree.knn_regress_self_device(K5, dy, out=sout.to(torch.float32)),
        lambda: tree.knn_regress_self_device(K5, dy.cpu()),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refused[{i}] was accepted")


# ---- 13. the argument checks that need a handle, in the documented order, through the C entries
def test_argument_errors_on_a_real_handle(pn):
    from petal_neighbors_amd import _lib
    L = _lib.lib()
    n = 40
    buf = (C.c_double * (4 * n))()  # zeros: valid labels, targets and queries
    p = C.addressof(buf)
    neg = (C.c_int64 * n)(*([-5] * n))
    pneg = C.addressof(neg)
    t32 = pn.BallTree.euclidean(uniform((n, 5), 0x4ED0, np.float32))
    t64 = pn.BallTree.euclidean(uniform((n, 5), 0x4ED0, np.float64))
    one = pn.BallTree.euclidean(uniform((1, 5), 0x4ED1, np.float32))

    def entry(fam, sfx):
        f = getattr(L, f"pn_{fam}_{sfx}")
        tail = (None,) if "device" in fam else ()
        proba = (None,) if "classify" in fam else ()
        if "self" in fam:
            return lambda h, k, fl, q, v, w, out: f(h, k, v, w, fl, out, *proba, *tail)
        return lambda h, k, fl, q, v, w, out: f(h, q, 1, 5, 5, k, v, w, fl, out, *proba, *tail)

    for fam in ("knn_classify", "knn_classify_device", "knn_classify_self", "knn_classify_self_device",
                "knn_regress", "knn_regress_device", "knn_regress_self", "knn_regress_self_device"):
        classify, self_ = "classify" in fam, "self" in fam
        values, out_name = ("labels", "pred_out") if classify else ("targets", "out")
        width_msg = "n_classes" if classify else "n_out"
        top = n - 1 if self_ else n
        k_msg = f"k must be in [1, {'n - 1' if self_ else 'n'}] = [1, {top}]"
        for sfx, right, wrong in (("f32", t32, t64), ("f64", t64, t32)):
            call = entry(fam, sfx)
            # every later fault present at once: the earlier one is reported
            assert call(wrong._h, 0, 2, None, None, 0, None) == _lib.PN_ERR_INVALID and "flags" in _lib.last_error()
            assert call(wrong._h, 0, 1, None, None, 0, None) == _lib.PN_ERR_INVALID and f"{out_name} is NULL" in _lib.last_error()
            if not self_:
                assert call(wrong._h, 0, 1, None, None, 0, p) == _lib.PN_ERR_INVALID and "queries is NULL" in _lib.last_error()
            assert call(wrong._h, 0, 1, p, None, 0, p) == _lib.PN_ERR_INVALID and f"{values} is NULL" in _lib.last_error()
            assert call(wrong._h, 0, 1, p, pneg, 0, p) == _lib.PN_ERR_INVALID and "element type" in _lib.last_error()
            assert call(right._h, 0, 1, p, pneg, 0, p) == _lib.PN_ERR_INVALID and width_msg in _lib.last_error()
            if classify:
                assert call(right._h, 0, 0, p, pneg, 2 ** 31, p) == _lib.PN_ERR_INVALID and width_msg in _lib.last_error()
            for k in (0, top + 1, 5000):
                assert call(right._h, k, 0, p, pneg, 3, p) == _lib.PN_ERR_INVALID
                assert k_msg in _lib.last_error(), (fam, k)
            if classify and "device" not in fam:  # last of all, the host entries' label scan
                assert call(right._h, 3, 1, p, pneg, 3, p) == _lib.PN_ERR_INVALID
                assert "labels[0] = -5" in _lib.last_error()
        if self_:
            for k in (0, 1, 2):  # one row: no k is valid
                assert entry(fam, "f32")(one._h, k, 0, p, p, 1, p) == _lib.PN_ERR_INVALID
                assert "needs at least 2 rows" in _lib.last_error()
        else:  # no queries: nothing to do, after the checks
            f = getattr(L, f"pn_{fam}_f32")
            tail = (None,) if "device" in fam else ()
            proba = (None,) if classify else ()
            assert f(t32._h, None, 0, 5, 5, 3, None, 3, 0, p, *proba, *tail) == 0, _lib.last_error()
            assert f(t32._h, None, 0, 5, 5, 0, None, 3, 0, p, *proba, *tail) == _lib.PN_ERR_INVALID
    with pytest.raises(ValueError):
        one.knn_classify_self(1, [0])
    for t in (t32, t64, one):
        t.close()


# ---- 14. statistics
def test_stats_count_the_queries_and_the_rows(big):
    tree, q, codes, y = big["tree"], big["q"], big["codes"], big["y"][:, 0]
    n = len(codes)
    for call, grows in ((lambda: tree.knn_classify(q[:123], K5, codes), 123), (lambda: tree.knn_regress(q[:77], K5, y), 77),
                        (lambda: tree.knn_classify_self(K5, codes), n), (lambda: tree.knn_regress_self(K5, y, "distance"), n)):
        before = tree.stats()["queries"]
        call()
        assert tree.stats()["queries"] - before == grows


# ---- 15. the host conveniences
def test_host_python_conveniences(pn, big):
    tree, q, codes = big["tree"], big["q"][:200], big["codes"]
    names = np.array(["ash", "birch", "cedar", "elm", "fir", "oak", "yew"])
    pred, proba, classes = tree.knn_classify(q, K5, names[codes], proba=True)
    assert classes.tolist() == names.tolist() and pred.dtype == names.dtype
    want_pred, want_proba = ref.classify(big["lists"][0][:200], big["lists"][1][:200], codes, C5)
    assert np.array_equal(pred, names[want_pred])
    same_bits(proba, want_proba, "string labels: proba")
    shifted = tree.knn_classify_self(K5, codes * 10 - 30, "distance")  # any integers: the values come back
    assert np.array_equal(shifted, ref.classify(*big["self_lists"], codes, C5, True)[0] * 10 - 30)
    y = big["y"][:, 0].astype(np.float32)  # 1-D targets of another real dtype: 1-D float64 back
    out = tree.knn_regress(q, K5, y)
    assert out.shape == (200,) and out.dtype == np.float64
    same_bits(out, ref.regress(big["lists"][0][:200], big["lists"][1][:200], y.astype(np.float64))[:, 0], "1-D targets")
    assert tree.knn_regress_self(K5, y).shape == (5000,)
    bad = q.copy()
    bad[[3, 9], 0] = np.nan
    with pytest.raises(ValueError, match="2 of 200"):
        tree.knn_classify(bad, K5, codes)
    assert np.isnan(tree.knn_regress(bad, K5, y)[[3, 9]]).all()
