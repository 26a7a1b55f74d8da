"""pn_hdbscan_*: labels, membership probabilities and the number of clusters, against the header's contract written out
in plain Python over the library's own ``mst`` output -- so what is compared is the new code: the dendrogram, the
condensed tree, the stabilities, the selection, the numbering.

The reference (``ref_hdbscan``): the sequential dendrogram of test_gpu_linkage.py, then a top-down walk.  A node with both
children of at least m rows is a true split and opens two clusters; otherwise the rows of each child below m fall out of
the current cluster at lambda(node).  stability(c) adds (lambda_p - birth) over the cluster's rows in ascending
(lambda, row) order, then the ending split's size * (lambda - birth); death(c) is the largest of those lambda.  Bottom-up
a non-root cluster is flagged unless its children's best values sum to strictly more than its stability; selected are the
flagged clusters without a flagged ancestor, numbered by their lowest member row.

Labels and n_clusters must be equal.  Probabilities: both sides divide two f64 values fixed by the data -- lambda_p and the
selected cluster's death, which is one of the lambdas, not a sum -- and round once, so they must be equal bit for bit.
What a different summation order could change is a selection; the reference therefore returns the least relative gap
|stability - children's sum| / max(...) over all decisions and every test demands it to be >= 1e-6 BEFORE it compares:
a condition on the inputs, ten orders of magnitude above the rounding of an f64 sum, not a tolerance on the results.
"""
import numpy as np
import pytest

from conftest import uniform
from test_gpu_linkage import seq_linkage
from test_gpu_mst import blobs

pytestmark = pytest.mark.gpu

PN_OPT_MST_BATCH = 12
MIN_GAP = 1e-6


def lam_of(w):
    w = float(w)
    if w != w:
        return 0.0
    return 1.0 / w if w > 2.0 ** -100 else 2.0 ** 100


def ref_hdbscan(n, src, dst, weight, m, dtype, base=0):
    """labels int64 [n], probabilities dtype [n], n_clusters, and a dict of what the walk met"""
    labels = np.full(n, -1, dtype=np.int64)
    prob = np.zeros(n, dtype=dtype)
    info = {"condensed": 0, "gap": np.inf, "noise": n, "nested": 0}
    if n < m or n < 2:
        return labels, prob, 0, info
    left, right, size, ok = seq_linkage(n, src, dst, base)
    assert ok
    lam = [lam_of(w) for w in weight]

    def sz(v):
        return 1 if v < n else int(size[v - n])

    def rows_under(v):
        out, stack = [], [v]
        while stack:
            u = stack.pop()
            if u < n:
                out.append(u)
            else:
                stack += [int(left[u - n]), int(right[u - n])]
        return out
    # clusters in the order they are opened: parents before children
    clusters = [{"birth": 0.0, "parent": -1, "pts": [], "split": None, "kids": []}]
    stack = [(2 * n - 2, 0)]
    while stack:
        v, c = stack.pop()
        l, r = int(left[v - n]), int(right[v - n])
        if sz(l) >= m and sz(r) >= m:
            clusters[c]["split"] = v
            for ch in (l, r):
                clusters.append({"birth": lam[v - n], "parent": c, "pts": [], "split": None, "kids": []})
                clusters[c]["kids"].append(len(clusters) - 1)
                stack.append((ch, len(clusters) - 1))
            continue
        for ch in (l, r):
            if sz(ch) >= m:
                stack.append((ch, c))
            else:
                clusters[c]["pts"] += [(lam[v - n], p) for p in rows_under(ch)]
    for cl in clusters:
        cl["pts"].sort()
        s = 0.0
        for lp, _ in cl["pts"]:
            s += lp - cl["birth"]
        death = max([lp for lp, _ in cl["pts"]], default=0.0)
        if cl["split"] is not None:
            ls = lam[cl["split"] - n]
            s += sz(cl["split"]) * (ls - cl["birth"])
            death = max(death, ls)
        cl["stab"], cl["death"] = s, death
    for ci in range(len(clusters) - 1, 0, -1):  # bottom-up; the root (0) is never flagged
        cl = clusters[ci]
        kids = sum(clusters[k]["best"] for k in cl["kids"])  # (two terms: the order cannot matter)
        if cl["kids"]:
            big = max(kids, cl["stab"])
            if big > 0:
                info["gap"] = min(info["gap"], abs(kids - cl["stab"]) / big)
        cl["flag"] = not (kids > cl["stab"])
        cl["best"] = cl["stab"] if cl["flag"] else kids
    clusters[0]["flag"] = False
    for ci, cl in enumerate(clusters):  # top-down: the selected ancestor-or-self
        up = clusters[cl["parent"]]["sel"] if ci else -1
        cl["sel"] = up if up >= 0 else (ci if cl["flag"] else -1)
        if cl["flag"] and up >= 0:
            info["nested"] += 1  # a flagged cluster under a selected one
    low = {}
    for cl in clusters:
        if cl["sel"] >= 0 and cl["pts"]:
            low[cl["sel"]] = min(low.get(cl["sel"], n), min(p for _, p in cl["pts"]))
    number = {c: i for i, c in enumerate(sorted(low, key=low.get))}
    for cl in clusters:
        if cl["sel"] < 0:
            continue
        death = clusters[cl["sel"]]["death"]
        for lp, p in cl["pts"]:
            labels[p] = number[cl["sel"]]
            prob[p] = 1.0 if death == 0 else min(lp, death) / death
    info.update(condensed=len(clusters), noise=int(np.count_nonzero(labels < 0)))
    return labels, prob, len(number), info


def _uint(dtype):
    return np.uint32 if np.dtype(dtype) == np.float32 else np.uint64


def reference_for(tree, k, m, base=0):
    core = tree.query_self(k)[1][:, -1]
    src, dst, w = tree.mst(core)
    return ref_hdbscan(tree._n, src, dst, w, m, tree.dtype, base)


def check(tree, k, m, want, what):
    """hdbscan and hdbscan_device against the reference's (labels, prob, n_clusters, info)"""
    w_labels, w_prob, w_ncl, info = want
    u = _uint(tree.dtype)
    print(f"{what}: reference {w_ncl} clusters, {info['noise']} noise rows, {info['condensed']} condensed clusters, "
          f"{info['nested']} flagged under a selected one, least gap {info['gap']:.3g}")
    assert info["gap"] >= MIN_GAP, what  # (a condition on the input)
    labels, prob = tree.hdbscan(m, k)
    ulp = np.abs(prob.view(u).astype(np.int64) - w_prob.view(u).astype(np.int64))
    print(f"{what}: device {tree.last_n_clusters} clusters, differing labels {int(np.count_nonzero(labels != w_labels))}, "
          f"probabilities off by at most {int(ulp.max()) if len(ulp) else 0} ulp")
    assert labels.dtype == np.int64 and prob.dtype == tree.dtype
    assert tree.last_n_clusters == w_ncl, what
    assert np.array_equal(labels, w_labels), what
    assert np.array_equal(prob.view(u), w_prob.view(u)), what
    dl, dp, dn = tree.hdbscan_device(m, k)
    assert int(dn.cpu()[0]) == w_ncl, what
    assert np.array_equal(dl.cpu().numpy(), w_labels) and np.array_equal(dp.cpu().numpy().view(u), w_prob.view(u)), what
    return labels, prob


# ---- (a) blobs with noise: three cluster sizes on one tree
@pytest.fixture(scope="module")
def big_blobs(pn):
    x = blobs(5, 5000, 16, 12, 0.05, 0.10)
    tree = pn.BallTree.euclidean(x)
    refs = {m: reference_for(tree, 8, m) for m in (5, 25, 100)}
    tree.close()
    return x, refs


@pytest.mark.parametrize("m", [5, 25, 100])
def test_blobs_5000_x_16(pn, big_blobs, m):
    x, refs = big_blobs
    want = refs[m]
    assert want[2] == 12 and 300 <= want[3]["noise"] <= 700 and 20 <= want[3]["condensed"] <= 30
    tree = pn.BallTree.euclidean(x)
    check(tree, 8, m, want, f"blobs 5000 x 16, m = {m}")
    tree.close()


@pytest.fixture(scope="module")
def small_blobs(pn):
    x = blobs(7, 1500, 4, 6, 0.03, 0.2)
    tree = pn.BallTree.euclidean(x)
    refs = {m: reference_for(tree, 5, m) for m in (2, 10, 40)}
    tree.close()
    return x, refs


@pytest.mark.parametrize("m", [2, 10, 40])
def test_blobs_1500_x_4_with_nested_selections(pn, small_blobs, m):
    x, refs = small_blobs
    want = refs[m]
    assert want[2] >= 2 and want[3]["noise"] > 0
    if m == 2:  # many small clusters, flagged ones under selected ones: the selection has work to do
        assert want[3]["condensed"] >= 60 and want[2] >= 8 and want[3]["nested"] >= 1
    else:
        assert want[2] == 6
    tree = pn.BallTree.euclidean(x)
    check(tree, 5, m, want, f"blobs 1500 x 4, m = {m}")
    tree.close()


def test_default_min_samples_is_min_cluster_size(pn, small_blobs):
    x, _ = small_blobs
    tree = pn.BallTree.euclidean(x)
    a = tree.hdbscan(10)
    b = tree.hdbscan(10, 10)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    tree.close()


# ---- (b) an f64 index
def test_f64_index(pn):
    x = blobs(11, 1200, 5, 4, 0.04, 0.15).astype(np.float64)
    tree = pn.BallTree.euclidean(x)
    for m in (5, 30):
        want = reference_for(tree, 6, m)
        assert want[2] >= 2 and want[3]["noise"] > 0
        check(tree, 6, m, want, f"f64 blobs 1200 x 5, m = {m}")
    tree.close()


# ---- (c) Cosine: non-positive weights meet the lambda clamp
def test_cosine_index_with_parallel_rows(pn):
    x = uniform((400, 8), 99) - np.float32(0.5)
    x[300:330] = x[3] * np.linspace(0.3, 3.0, 30, dtype=np.float32)[:, None]  # parallel rows: distances a few ulp around 0
    tree = pn.BallTree.new(x, pn.distance.Cosine())
    for k, m in ((4, 5), (2, 3)):
        core = tree.query_self(k)[1][:, -1]
        w = tree.mst(core)[2]
        assert (w <= 0).any() and (w > 0).any()
        check(tree, k, m, reference_for(tree, k, m), f"cosine 400 x 8, k = {k}, m = {m}")
    tree.close()


# ---- (d) duplicates (zero weights), NaN rows, tiny indexes
def test_more_than_m_duplicate_rows(pn):
    x = blobs(3, 800, 3, 3, 0.05, 0.2)
    x[100:112] = x[100]  # 12 equal rows: zero weights, lambda = 2^100
    x[500:520] = x[500]
    tree = pn.BallTree.euclidean(x)
    for k, m in ((4, 5), (3, 10)):
        core = tree.query_self(k)[1][:, -1]
        assert np.count_nonzero(tree.mst(core)[2] == 0) >= 20
        want = reference_for(tree, k, m)
        labels, prob = check(tree, k, m, want, f"duplicates, k = {k}, m = {m}")
        assert np.isfinite(prob).all()
    tree.close()


def test_nan_rows_end_as_noise(pn):
    x = blobs(9, 900, 3, 3, 0.04, 0.15)
    x[17, 1] = np.nan
    x[405] = np.nan
    tree = pn.BallTree.euclidean(x)
    want = reference_for(tree, 5, 10)
    assert want[2] >= 2
    labels, prob = check(tree, 5, 10, want, "900 x 3 with two NaN rows")
    assert labels[17] == -1 and labels[405] == -1 and prob[17] == 0 and prob[405] == 0
    tree.close()


def test_tiny_indexes_and_n_below_m(pn):
    x = uniform((40, 3), 12)
    for n, k, m in ((2, 1, 2), (1, 1, 2), (3, 2, 2), (40, 5, 41), (40, 5, 40), (40, 5, 21), (40, 3, 4)):
        tree = pn.BallTree.euclidean(x[:n])
        if n == 1:
            want = (np.full(1, -1, dtype=np.int64), np.zeros(1, dtype=np.float32), 0, {"gap": np.inf, "noise": 1, "condensed": 0,
                                                                                       "nested": 0})
        else:
            want = reference_for(tree, k, m)
        if m > n // 2:  # no node can have two children of m rows: all noise
            assert want[2] == 0 and (want[0] == -1).all()
        check(tree, k, m, want, f"n = {n}, k = {k}, m = {m}")
        tree.close()


def test_argument_errors_that_need_a_handle(pn):
    from petal_neighbors_amd import _lib
    import ctypes as C
    x32, x64 = uniform((10, 3), 1), uniform((10, 3), 1).astype(np.float64)
    t32, t64 = pn.BallTree.euclidean(x32), pn.BallTree.euclidean(x64)
    L = _lib.lib()
    buf = (C.c_int64 * 16)()
    p = C.addressof(buf)
    # in order: element type, min_cluster_size, min_samples
    assert L.pn_hdbscan_f64(t32._h, 0, 1, 0, p, None, None) == _lib.PN_ERR_INVALID and "element type" in _lib.last_error()
    assert L.pn_hdbscan_f32(t64._h, 0, 1, 0, p, None, None) == _lib.PN_ERR_INVALID and "element type" in _lib.last_error()
    assert L.pn_hdbscan_f32(t32._h, 0, 1, 0, p, None, None) == _lib.PN_ERR_INVALID and "min_cluster_size" in _lib.last_error()
    for k in (0, 10, 11):
        assert L.pn_hdbscan_f32(t32._h, k, 2, 0, p, None, None) == _lib.PN_ERR_INVALID and "min_samples" in _lib.last_error()
        assert L.pn_hdbscan_device_f64(t64._h, k, 2, 0, p, None, None, None) == _lib.PN_ERR_INVALID
    for bad in ((1, None), (5, 0), (5, 10)):
        with pytest.raises(ValueError):
            t32.hdbscan(*bad)
    t32.close()
    t64.close()


# ---- (e) engines, batches, repeated calls
def test_engines_and_batches_never_change_a_label(pn, big_blobs):
    x, refs = big_blobs
    want = refs[25]
    tree = pn.BallTree.euclidean(x)
    u = np.uint32
    for eng in ("exact", "bf16", "auto"):
        tree.set_engine(eng)
        for batch in (0, 64, 1000):
            tree.set_option(PN_OPT_MST_BATCH, batch)
            labels, prob = tree.hdbscan(25, 8)
            assert np.array_equal(labels, want[0]) and np.array_equal(prob.view(u), want[1].view(u)), (eng, batch)
            assert tree.last_n_clusters == want[2]
    tree.close()


def test_two_calls_in_a_row_are_bit_identical(pn, small_blobs):
    x, _ = small_blobs
    tree = pn.BallTree.euclidean(x)
    for m in (2, 10):
        a = tree.hdbscan_device(m, 5)
        a = [t.cpu().numpy().copy() for t in a]
        b = [t.cpu().numpy() for t in tree.hdbscan_device(m, 5)]
        c = tree.hdbscan(m, 5)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2] == b[2]
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1].view(np.uint32), c[1].view(np.uint32))
    tree.close()


# ---- (f) the caller's stream and outputs
def test_device_entry_on_a_stream_with_given_outputs(pn, small_blobs):
    import torch
    x, refs = small_blobs
    n = len(x)
    tree = pn.BallTree.euclidean(x)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    labels = torch.full((n,), -7, dtype=torch.int64, device=dev)
    prob = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    ncl = torch.full((1,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for rep in range(2):  # a repeated call reuses the workspace
        for m in (2, 40):
            with torch.cuda.stream(st):
                r = tree.hdbscan_device(m, 5, out_labels=labels, out_probabilities=prob, out_n_clusters=ncl,
                                        stream=st.cuda_stream)
            st.synchronize()
            assert r[0] is labels and r[1] is prob and r[2] is ncl
            assert int(ncl.cpu()[0]) == refs[m][2]
            assert np.array_equal(labels.cpu().numpy(), refs[m][0])
            assert np.array_equal(prob.cpu().numpy().view(np.uint32), refs[m][1].view(np.uint32))
    with pytest.raises(ValueError):
        tree.hdbscan_device(10, 5, out_labels=labels[:10])
    with pytest.raises(ValueError):
        tree.hdbscan_device(10, 5, out_probabilities=prob.double())
    with pytest.raises(ValueError):
        tree.hdbscan_device(10, 5, out_labels=labels.int())
    with pytest.raises(ValueError):
        tree.hdbscan_device(10, 5, out_n_clusters=ncl.int())
    tree.close()


# ---- (g) supplementary: the same partition as scikit-learn's extraction fed the reference dendrogram
def test_same_partition_as_scikit_learn(pn, small_blobs):
    pytest.importorskip("sklearn")
    from sklearn.cluster._hdbscan import _tree
    x, _ = small_blobs
    tree = pn.BallTree.euclidean(x)
    n = len(x)
    core = tree.query_self(5)[1][:, -1]
    src, dst, w = tree.mst(core)
    left, right, size, ok = seq_linkage(n, src, dst)
    slt = np.empty(n - 1, dtype=_tree.HIERARCHY_dtype)
    slt["left_node"], slt["right_node"], slt["value"], slt["cluster_size"] = left, right, w.astype(np.float64), size
    for m in (2, 10, 40):
        sk_labels, sk_prob = _tree.tree_to_labels(slt, min_cluster_size=m, cluster_selection_method="eom",
                                                  allow_single_cluster=False)
        labels, prob = tree.hdbscan(m, 5)
        assert np.array_equal(labels < 0, sk_labels < 0), m
        pairs = set(zip(labels[labels >= 0].tolist(), sk_labels[labels >= 0].tolist()))
        assert len(pairs) == tree.last_n_clusters == len(set(sk_labels[sk_labels >= 0].tolist())), m  # a bijection
        assert np.array_equal(prob, sk_prob.astype(np.float32)), m
    tree.close()
