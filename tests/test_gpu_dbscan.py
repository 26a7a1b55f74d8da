"""pn_dbscan_*: cluster labels of the indexed rows computed on the device, against a scan-order DBSCAN on the CPU.

The contract (include/petal_mi355x.h): N(i) = { j : distance(p_i, p_j) < eps } -- the list pn_query_radius_self_* returns
with PN_SELF_INCLUDE --, core[i] = |N(i)| >= min_samples, clusters = connected components of the core rows numbered by
ascending lowest core row, a border row takes the lowest-numbered cluster among its core neighbours, everything else is
-1.  That is what the classic algorithm below computes when it visits the rows in index order and expands each new cluster
fully before it starts the next, so labels, core flags and the number of clusters must be EQUAL ARRAYS: no label matching.
The CPU lists come from the oracle (oracle.brute_radius per row; Cosine: decided in f64 away from eps and by the oracle's
scalar Cosine::distance inside a band around it, as tests/test_gpu_cosine_radius.py does).
"""
import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

PN_OPT_DBSCAN_PIECE = 11


def cpu_dbscan(offsets, idx, min_samples):
    """scan-order DBSCAN over CSR neighbour lists (each row's own index included where the metric says so)"""
    n = len(offsets) - 1
    offsets = np.asarray(offsets, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    core = (offsets[1:] - offsets[:-1]) >= min_samples
    labels = np.full(n, -1, dtype=np.int64)
    n_clusters = 0
    for i in range(n):
        if labels[i] != -1 or not core[i]:
            continue
        labels[i] = n_clusters
        stack = [i]
        while stack:
            u = stack.pop()
            for v in idx[offsets[u]:offsets[u + 1]].tolist():
                if labels[v] == -1:
                    labels[v] = n_clusters
                    if core[v]:
                        stack.append(v)
        n_clusters += 1
    return labels, core, n_clusters


def csr(lists):
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(x) for x in lists])
    return offsets, (np.concatenate(lists).astype(np.int64) if offsets[-1] else np.zeros(0, dtype=np.int64))


def euclid_lists(oracle_mod, pts, eps):
    return csr([oracle_mod.brute_radius(pts, pts[i], pts.dtype.type(eps)) for i in range(len(pts))])


def cosine_lists(oracle_mod, pts, eps, band=2e-4):
    p64 = pts.astype(np.float64)
    nrm = np.linalg.norm(p64, axis=1)
    d = 1.0 - (p64 @ p64.T) / np.outer(nrm, nrm)
    sure = d < float(eps) - band
    for i, j in zip(*np.nonzero(np.abs(d - float(eps)) <= band)):
        sure[i, j] = oracle_mod.cosine(pts[i], pts[j]) < eps
    for i in range(len(pts)):  # a row's distance to itself is a few ulp around 0 under Cosine
        sure[i, i] = oracle_mod.cosine(pts[i], pts[i]) < eps
    return csr([np.flatnonzero(row) for row in sure])


def blobs(seed, n, dim, nb, sigma, background, shift=0.0):
    """Gaussian blobs around nb centres in [0, 1)^dim, a uniform background, rows permuted"""
    rng = np.random.default_rng(seed)
    centres = rng.random((nb, dim))
    n_bg = int(round(n * background))
    which = rng.integers(0, nb, n - n_bg)
    pts = np.concatenate([centres[which] + sigma * rng.standard_normal((n - n_bg, dim)), rng.random((n_bg, dim))])
    return (pts[rng.permutation(n)] + shift).astype(np.float32)


def check(tree, want, eps, min_samples, what):
    labels, core = tree.dbscan(eps, min_samples)
    w_labels, w_core, w_ncl = want
    n_border = int(np.count_nonzero((w_labels >= 0) & ~w_core))
    print(f"{what}: {w_ncl} clusters, {int(np.count_nonzero(w_labels < 0))} noise, {n_border} border rows; "
          f"differing labels {int(np.count_nonzero(labels != w_labels))}, core flags {int(np.count_nonzero(core != w_core))}")
    assert labels.dtype == np.int64 and core.dtype == bool
    assert np.array_equal(core, w_core), what
    assert np.array_equal(labels, w_labels), what
    dl, dc, dn = tree.dbscan_device(eps, min_samples)
    assert int(dn.item()) == w_ncl, what
    assert np.array_equal(dl.cpu().numpy(), w_labels) and np.array_equal(dc.cpu().numpy().astype(bool), w_core), what
    return n_border


def ambiguous_borders(offsets, idx, labels, core):
    """border rows whose core neighbours lie in two or more clusters"""
    count = 0
    for i in np.flatnonzero((labels >= 0) & ~core):
        nb = idx[offsets[i]:offsets[i + 1]]
        count += len(set(labels[nb[core[nb]]].tolist())) > 1
    return count


# ---- (a) the exact-scan path (n < 4096), both element types
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_uniform_plane_equals_the_scan_order_algorithm(pn, oracle_mod, dtype):
    pts = oracle_mod.fill_uniform(4000 * 2, 11).reshape(4000, 2).astype(dtype)
    eps, ms = 0.02, 6
    off, idx = euclid_lists(oracle_mod, pts, eps)
    want = cpu_dbscan(off, idx, ms)
    assert want[2] > 50 and ambiguous_borders(off, idx, want[0], want[1]) > 10  # (the numbering rule is exercised)
    tree = pn.BallTree.euclidean(pts)
    assert check(tree, want, dtype(eps), ms, f"uniform 4000 x 2 {np.dtype(dtype).name}") > 500
    tree.close()


# ---- (b) the bf16 tier (n >= 4096, D >= 8): blobs with a background; the oracle's lists once per module
@pytest.fixture(scope="module")
def blob_sets(oracle_mod):
    out = {}
    for name, nb, eps, ms in (("b1", 12, 0.2, 10), ("b2", 40, 0.18, 6)):
        pts = blobs(3, 12000, 16, nb, 0.05, 0.10)
        off, idx = euclid_lists(oracle_mod, pts, eps)
        out[name] = (pts, np.float32(eps), ms, off, idx, cpu_dbscan(off, idx, ms))
    return out


@pytest.mark.parametrize("name", ["b1", "b2"])
def test_blobs_equal_the_scan_order_algorithm(pn, blob_sets, name):
    pts, eps, ms, off, idx, want = blob_sets[name]
    tree = pn.BallTree.euclidean(pts)
    assert tree.bf16_eligible
    assert want[2] >= 10
    if name == "b1":
        assert int(np.max(np.diff(off))) > 224  # (some lists are longer than the filter keeps: the listed exact pass)
    assert check(tree, want, eps, ms, f"blobs {name}") > 100
    tree.close()


# ---- (c) Cosine
def test_cosine_blobs_equal_the_scan_order_algorithm(pn, oracle_mod):
    pts = blobs(9, 5000, 16, 20, 0.04, 0.15, shift=-0.5)
    eps, ms = np.float32(0.02), 8
    off, idx = cosine_lists(oracle_mod, pts, eps)
    want = cpu_dbscan(off, idx, ms)
    assert want[2] >= 5
    tree = pn.BallTree.new(pts, pn.distance.Cosine())
    check(tree, want, eps, ms, "cosine blobs")
    tree.set_engine("exact")
    check(tree, want, eps, ms, "cosine blobs, exact engine")
    tree.close()


# ---- (d) engines and piece sizes never change a label
def test_engines_and_piece_sizes_give_the_same_labels(pn, blob_sets):
    pts, eps, ms, off, idx, want = blob_sets["b1"]
    tree = pn.BallTree.euclidean(pts)
    for eng in ("exact", "bf16", "auto"):
        tree.set_engine(eng)
        for piece in (0, 4096):
            tree.set_option(PN_OPT_DBSCAN_PIECE, piece)
            check(tree, want, eps, ms, f"engine {eng}, piece {piece}")
    tree.close()
    # one row per piece, on a subset
    sub = np.ascontiguousarray(pts[:2000])
    small = pn.BallTree.euclidean(sub)
    l0, c0 = small.dbscan(eps, ms)
    small.set_option(PN_OPT_DBSCAN_PIECE, 1)
    l1, c1 = small.dbscan(eps, ms)
    assert np.array_equal(l0, l1) and np.array_equal(c0, c1) and l0.max() >= 1
    with pytest.raises(Exception):
        small.set_option(PN_OPT_DBSCAN_PIECE, -1)
    small.close()


# ---- (e) edge cases
def test_edge_cases(pn, oracle_mod):
    pts = uniform((600, 3), 4711)
    pts[100:110] = pts[5]          # duplicated rows
    pts[300] = np.nan              # a NaN row: noise, and in nobody's neighbourhood
    pts[301, 1] = np.nan
    n = len(pts)
    finite = np.isfinite(pts).all(axis=1)
    tree = pn.BallTree.euclidean(pts)
    for eps in (0.0, -1.0, float("nan")):
        for ms in (1, 5):
            labels, core = tree.dbscan(np.float32(eps), ms)
            assert (labels == -1).all() and not core.any(), eps
            dl, dc, dn = tree.dbscan_device(np.float32(eps), ms)
            assert (dl.cpu().numpy() == -1).all() and not dc.cpu().numpy().any() and int(dn.item()) == 0, eps
    # +inf: one cluster of all finite rows
    labels, core = tree.dbscan(np.float32("inf"), 5)
    assert np.array_equal(labels, np.where(finite, 0, -1)) and np.array_equal(core, finite)
    off, idx = euclid_lists(oracle_mod, pts, 0.09)
    for ms in (1, 4, n + 1):
        want = cpu_dbscan(off, idx, ms)
        check(tree, want, np.float32(0.09), ms, f"edge data, min_samples {ms}")
        if ms == 1:   # every row with a finite self-distance is core
            assert np.array_equal(want[1], finite)
        if ms == n + 1:
            assert want[2] == 0 and (want[0] == -1).all()
    labels, _ = tree.dbscan(np.float32(0.09), 4)
    assert labels[300] == -1 and labels[301] == -1 and len(set(labels[100:110].tolist()) | {int(labels[5])}) == 1
    tree.close()
    one = pn.BallTree.euclidean(pts[:1].copy())
    labels, core = one.dbscan(np.float32(1.0), 1)
    assert labels.tolist() == [0] and core.tolist() == [True]
    labels, core = one.dbscan(np.float32(1.0), 2)
    assert labels.tolist() == [-1] and core.tolist() == [False]
    one.close()


# ---- (f) more than one 2^18-row chunk, against the CPU algorithm over the lists of query_radius_self
def test_more_than_one_chunk_of_rows(pn):
    n = (1 << 18) + 5000
    pts = uniform((n, 8), 2024)
    eps, ms = np.float32(0.24), 8
    tree = pn.BallTree.euclidean(pts)
    off, idx, _ = tree.query_radius_self(eps, include_self=True)
    mean = float(off[-1]) / n
    assert 4 < mean < 30, mean
    want = cpu_dbscan(off, idx, ms)
    assert want[2] > 1 and 0 < np.count_nonzero(want[1]) < n
    check(tree, want, eps, ms, f"{n} x 8, mean list {mean:.1f}")
    tree.set_option(PN_OPT_DBSCAN_PIECE, 1 << 20)   # pieces cut by entries, inside and across the chunks
    check(tree, want, eps, ms, f"{n} x 8, pieces of 2^20 entries")
    tree.close()


# ---- (g) caller's stream and outputs; repeated calls
def test_device_entry_on_a_stream_with_given_outputs(pn, blob_sets):
    import torch
    pts, eps, ms, off, idx, want = blob_sets["b2"]
    tree = pn.BallTree.euclidean(pts)
    h_labels, h_core = tree.dbscan(eps, ms)
    dev = torch.device("cuda", 0)
    out_l = torch.full((len(pts),), -7, dtype=torch.int64, device=dev)
    out_c = torch.full((len(pts),), 9, dtype=torch.uint8, device=dev)
    out_n = torch.full((1,), -7, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        got = tree.dbscan_device(eps, ms, out_labels=out_l, out_core=out_c, out_n_clusters=out_n, stream=st.cuda_stream)
    st.synchronize()
    assert got[0] is out_l and got[1] is out_c and got[2] is out_n
    assert np.array_equal(out_l.cpu().numpy(), h_labels) and np.array_equal(out_c.cpu().numpy().astype(bool), h_core)
    assert int(out_n.item()) == want[2] == int(h_labels.max()) + 1
    again_l, again_c = tree.dbscan(eps, ms)
    assert np.array_equal(again_l, h_labels) and np.array_equal(again_c, h_core)
    with pytest.raises(ValueError):
        tree.dbscan_device(eps, ms, out_labels=torch.empty(3, dtype=torch.int64, device=dev))
    tree.close()
