"""pn_optics_* and pn_optics_dbscan_*: ordering, reachability, predecessors and core distances computed on the device,
against the numpy restatement of the contract (tests/optics_reference.py) fed with the oracle's lists and distances.

The contract (include/petal_mi355x.h) fixes every tie -- the unprocessed row with the smallest (reach, row) goes next, an
offer must be strictly smaller to replace a reachability -- so all four arrays must be EQUAL ARRAYS, bit for bit, host and
device entry points alike.  The want side: the lists are oracle.brute_radius per row (Cosine: the band method of
tests/test_gpu_dbscan.py) without the row itself; the distances are the reference's fold evaluated per list entry in
numpy, checked against the oracle's scalar distance on a sample (Cosine: the oracle's scalar distance for every entry);
the core distance is the min_samples-th smallest distance of a row's list, +inf for a shorter list.

(a) uses rows uniform in [0, 1.25)^2: at max_eps = 0.03 and min_samples = 5 that density leaves more than 100 rows that
nothing reaches (on [0, 1)^2 the same seed leaves 4) and still more than 2000 picks decided by the row tie-break.
"""
import numpy as np
import pytest

from conftest import uniform
from optics_reference import cpu_extract, cpu_optics, csr_from_dense, fold_pairs, same_partition
from test_gpu_dbscan import blobs, cosine_lists, euclid_lists

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE = 3
PN_OPT_OPTICS_PIECE = 13
PN_ERR_INVALID = 3


def drop_self(off, idx):
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    keep = idx != rows
    out = np.zeros(len(off), dtype=np.int64)
    np.add.at(out, rows[keep] + 1, 1)
    return np.cumsum(out), rows[keep], idx[keep]


def euclid_graph(oracle_mod, pts, max_eps):
    off, i, j = drop_self(*euclid_lists(oracle_mod, pts, max_eps))
    d = fold_pairs(pts, i, j)
    pick = np.random.default_rng(1).integers(0, len(i), min(len(i), 300))
    for t in pick:  # the numpy fold is the oracle's scalar distance, bit for bit
        assert oracle_mod.euclidean(pts[i[t]], pts[j[t]]) == d[t]
    return off, j, d


def cosine_graph(oracle_mod, pts, max_eps):
    off, i, j = drop_self(*cosine_lists(oracle_mod, pts, max_eps))
    d = np.array([oracle_mod.cosine(pts[a], pts[b]) for a, b in zip(i.tolist(), j.tolist())], dtype=pts.dtype)
    return off, j, d


def dense_graph(pts, max_eps):
    """small inputs: every pair by the fold (NaN rows give NaN distances, which are < nothing)"""
    n = len(pts)
    i, j = np.divmod(np.arange(n * n), n)
    return csr_from_dense(fold_pairs(pts, i, j).reshape(n, n), max_eps)


def same(got, want, what):
    g_o, g_r, g_p, g_c = got
    w_o, w_r, w_p, w_c = want
    bad = [int(np.count_nonzero(np.asarray(g_o, dtype=np.uint64) != w_o)), int(np.count_nonzero(g_p != w_p)),
           int(np.count_nonzero(g_r.view(np.uint8) != w_r.view(np.uint8))),
           int(np.count_nonzero(g_c.view(np.uint8) != w_c.view(np.uint8)))]
    print(f"{what}: differing ordering / predecessor entries {bad[0]} / {bad[1]}, reachability / core bytes {bad[2]} / {bad[3]}")
    assert g_r.dtype == w_r.dtype and g_c.dtype == w_c.dtype and g_p.dtype == np.int64, what
    assert np.array_equal(np.asarray(g_o, dtype=np.uint64), w_o), what
    assert np.array_equal(g_p, w_p), what
    assert g_r.tobytes() == w_r.tobytes(), what
    assert g_c.tobytes() == w_c.tobytes(), what


def check(tree, want, ms, max_eps, what):
    got = tree.optics(ms, max_eps)
    assert got[0].dtype == np.uint64
    same(got, want, what + " (host)")
    dev = [t.cpu().numpy() for t in tree.optics_device(ms, max_eps)]
    same(dev, want, what + " (device)")
    return got


# ---- (a) the exact-scan path (n < 4096), a two-level tree, both element types
@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def plane(request, oracle_mod):
    dt = request.param
    pts = (oracle_mod.fill_uniform(4000 * 2, 11).reshape(4000, 2) * np.float32(1.25)).astype(dt)
    max_eps, ms = dt(0.03), 5
    stats = {}
    want = cpu_optics(*euclid_graph(oracle_mod, pts, max_eps), ms, stats)
    return pts, max_eps, ms, want, stats


def test_uniform_plane_equals_the_contract(pn, plane):
    pts, max_eps, ms, want, stats = plane
    n_inf = int(np.count_nonzero(np.isinf(want[1])))
    print(f"want side: {n_inf} rows with +inf reachability, {stats['tie_picks']} picks decided by the row tie-break")
    assert n_inf >= 100 and stats["tie_picks"] >= 1000  # (the rules are exercised)
    tree = pn.BallTree.euclidean(pts)
    before = tree.stats()["queries"]
    check(tree, want, ms, max_eps, f"uniform 4000 x 2 {pts.dtype.name}")
    assert tree.stats()["queries"] - before == 2 * len(pts)  # (n per call)
    tree.close()


# ---- (b) the bf16 tier (n >= 4096, D >= 8), a three-level tree: blobs with a background
@pytest.fixture(scope="module")
def blob_case(oracle_mod):
    pts = blobs(3, 12000, 16, 12, 0.05, 0.10)
    max_eps, ms = np.float32(0.17), 6
    graph = euclid_graph(oracle_mod, pts, max_eps)
    return pts, max_eps, ms, graph, cpu_optics(*graph, ms)


def test_blobs_equal_the_contract_whatever_the_piece(pn, blob_case):
    pts, max_eps, ms, graph, want = blob_case
    tree = pn.BallTree.euclidean(pts)
    assert tree.bf16_eligible
    entries = int(np.diff(graph[0])[np.isfinite(want[3])].sum())
    piece = 8192
    assert entries / piece >= 5  # (the stored lists -- the core rows' -- make at least 5 pieces)
    assert 1000 < np.count_nonzero(np.isinf(want[3])) < 11000 and np.count_nonzero(np.isinf(want[1])) > 100
    tree.set_option(PN_OPT_OPTICS_PIECE, piece)
    check(tree, want, ms, max_eps, f"blobs 12000 x 16, pieces of {piece} entries")
    tree.set_option(PN_OPT_OPTICS_PIECE, 0)
    check(tree, want, ms, max_eps, "blobs 12000 x 16, default piece")
    tree.set_option(PN_OPT_OPTICS_PIECE, 1)  # one row per piece, on the host entry point only
    same(tree.optics(ms, max_eps), want, "blobs 12000 x 16, one row per piece")
    with pytest.raises(Exception):
        tree.set_option(PN_OPT_OPTICS_PIECE, -1)
    tree.close()


# ---- (c) Cosine
def test_cosine_blobs_equal_the_contract(pn, oracle_mod):
    pts = blobs(9, 6000, 16, 20, 0.04, 0.15, shift=-0.5)
    max_eps, ms = np.float32(0.01), 8
    want = cpu_optics(*cosine_graph(oracle_mod, pts, max_eps), ms)
    assert 100 < np.count_nonzero(np.isinf(want[3])) < 5900
    tree = pn.BallTree.new(pts, pn.distance.Cosine())
    check(tree, want, ms, max_eps, "cosine blobs 6000 x 16")
    tree.close()


# ---- (d) edge cases on 300 x 3
def test_edge_cases(pn):
    pts = uniform((300, 3), 4711)
    n = len(pts)
    tree = pn.BallTree.euclidean(pts)
    inf = np.float32("inf")
    nothing = (np.arange(n, dtype=np.uint64), np.full(n, inf), np.full(n, -1, dtype=np.int64), np.full(n, inf))
    for eps in (0.0, -1.0, float("nan")):
        check(tree, nothing, 4, np.float32(eps), f"max_eps {eps}")
    # +inf: the complete graph; and min_samples = n - 1: every core distance is the row's largest distance
    for ms in (4, n - 1):
        want = cpu_optics(*dense_graph(pts, inf), ms)
        assert np.isfinite(want[3]).all() and np.count_nonzero(np.isinf(want[1])) == 1
        check(tree, want, ms, inf, f"max_eps +inf, min_samples {ms}")
    # a finite radius, then the same with an index base: nothing changes
    want = cpu_optics(*dense_graph(pts, np.float32(0.15)), 4)
    got = check(tree, want, 4, np.float32(0.15), "300 x 3")
    tree.set_option(PN_OPT_INDEX_BASE, 1000)
    check(tree, want, 4, np.float32(0.15), "300 x 3, index base 1000")
    labels, ncl = tree.optics_dbscan(np.float32(0.1), *[got[0], got[1], got[3]])
    assert np.array_equal(labels, cpu_extract(want[0], want[1], want[3], np.float32(0.1))[0])
    tree.close()
    # exact duplicate rows and one NaN row: an isolated +inf entry that appears in no list
    pts = uniform((300, 3), 4712)
    pts[100:110] = pts[5]
    pts[200, 1] = np.nan
    tree = pn.BallTree.euclidean(pts)
    for ms in (3, 12):
        want = cpu_optics(*dense_graph(pts, np.float32(0.2)), ms)
        assert want[1][200] == inf and want[3][200] == inf and want[2][200] == -1 and not np.any(want[2] == 200)
        assert (want[3][100:110] == 0).all() == (ms <= 10)
        check(tree, want, ms, np.float32(0.2), f"duplicates and a NaN row, min_samples {ms}")
    tree.close()
    # n = 1 and n = 2
    one = pn.BallTree.euclidean(pts[:1].copy())
    for ms in (1, 7):
        check(one, (np.zeros(1, dtype=np.uint64), np.full(1, inf), np.full(1, -1, dtype=np.int64), np.full(1, inf)), ms,
              np.float32(1.0), "n = 1")
    assert one.optics_dbscan(np.float32(0.5), np.zeros(1, dtype=np.uint64), np.full(1, inf), np.full(1, inf))[0].tolist() == [-1]
    one.close()
    two = pn.BallTree.euclidean(pts[:2].copy())
    d01 = fold_pairs(pts, np.array([0]), np.array([1]))[0]
    check(two, (np.array([0, 1], dtype=np.uint64), np.array([inf, d01]), np.array([-1, 0]), np.array([d01, d01])), 1, inf,
          "n = 2")
    check(two, (np.array([0, 1], dtype=np.uint64), np.full(2, inf), np.full(2, -1, dtype=np.int64), np.full(2, inf)), 1, d01,
          "n = 2, max_eps = the distance (strict)")
    with pytest.raises(ValueError):
        two.optics(2)
    two.close()


# ---- (e) extraction at eps' <= max_eps
def extraction(pn, tree, want, ms, max_eps, what):
    import torch
    w_o, w_r, w_p, w_c = want
    n = len(w_o)
    dev = torch.device("cuda", 0)
    t_o = torch.from_numpy(w_o.astype(np.int64)).to(dev)
    t_r, t_c = torch.from_numpy(w_r).to(dev), torch.from_numpy(w_c).to(dev)
    for frac in (0.5, 0.8, 1.0):
        eps = w_r.dtype.type(frac * float(max_eps))
        w_labels, w_ncl = cpu_extract(w_o, w_r, w_c, eps)
        labels, ncl = tree.optics_dbscan(eps, w_o, w_r, w_c)
        d_labels, d_ncl, d_err = tree.optics_dbscan_device(eps, t_o, t_r, t_c)
        print(f"{what}, eps' = {frac} max_eps: {w_ncl} clusters, {int(np.count_nonzero(w_labels < 0))} noise rows; "
              f"differing labels {int(np.count_nonzero(labels != w_labels))}")
        assert labels.dtype == np.int64 and np.array_equal(labels, w_labels) and ncl == w_ncl, frac
        assert np.array_equal(d_labels.cpu().numpy(), w_labels) and int(d_ncl.item()) == w_ncl and int(d_err.item()) == 0
        # the rows with core < eps' are DBSCAN(eps', min_samples + 1)'s core rows, and both labelings split them into the
        # same density-connected components (border rows may differ)
        db_labels, db_core = tree.dbscan(eps, ms + 1)
        near = w_c < eps
        assert np.array_equal(db_core, near), frac
        assert (labels[near] >= 0).all() and same_partition(labels[near], db_labels[near]), frac
        assert w_ncl == int(db_labels.max()) + 1
    assert w_ncl >= 2
    # an ordering that is no permutation of the rows
    eps = w_r.dtype.type(0.8 * float(max_eps))
    for bad in (np.where(np.arange(n) == 7, w_o[8], w_o), np.where(np.arange(n) == 7, np.uint64(n), w_o)):
        with pytest.raises(pn.PetalError) as e:
            tree.optics_dbscan(eps, bad, w_r, w_c)
        assert e.value.code == PN_ERR_INVALID
        d_err = tree.optics_dbscan_device(eps, torch.from_numpy(bad.astype(np.int64)).to(dev), t_r, t_c)[2]
        assert int(d_err.item()) == PN_ERR_INVALID
    assert int(tree.optics_dbscan_device(eps, t_o, t_r, t_c)[2].item()) == 0


def test_extraction_on_the_plane(pn, plane):
    pts, max_eps, ms, want, _ = plane
    tree = pn.BallTree.euclidean(pts)
    extraction(pn, tree, want, ms, max_eps, f"uniform 4000 x 2 {pts.dtype.name}")
    tree.close()


def test_extraction_on_the_blobs(pn, blob_case):
    pts, max_eps, ms, graph, want = blob_case
    tree = pn.BallTree.euclidean(pts)
    extraction(pn, tree, want, ms, max_eps, "blobs 12000 x 16")
    tree.close()


# ---- (f) determinism: twice on one handle, and on a second stream
def test_repeated_calls_and_a_second_stream_give_identical_bytes(pn, blob_case):
    import torch
    pts, max_eps, ms, graph, want = blob_case
    tree = pn.BallTree.euclidean(pts)
    first = [t.cpu().numpy().tobytes() for t in tree.optics_device(ms, max_eps)]
    second = [t.cpu().numpy().tobytes() for t in tree.optics_device(ms, max_eps)]
    assert first == second
    dev = torch.device("cuda", 0)
    n = len(pts)
    outs = dict(out_ordering=torch.full((n,), -7, dtype=torch.int64, device=dev),
                out_reachability=torch.full((n,), -7.0, dtype=torch.float32, device=dev),
                out_predecessor=torch.full((n,), -7, dtype=torch.int64, device=dev),
                out_core=torch.full((n,), -7.0, dtype=torch.float32, device=dev))
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        got = tree.optics_device(ms, max_eps, stream=st.cuda_stream, **outs)
    st.synchronize()
    assert all(g is o for g, o in zip(got, outs.values()))
    assert [t.cpu().numpy().tobytes() for t in got] == first
    same([t.cpu().numpy() for t in got], want, "second stream")
    with pytest.raises(ValueError):
        tree.optics_device(ms, max_eps, out_ordering=torch.empty(3, dtype=torch.int64, device=dev))
    tree.close()
