"""MST, linkage, HDBSCAN and OPTICS beyond one 2^18-row pipeline chunk, against references that never touch the library.

n = 2^18 + 3000 rows uniform in the plane (D = 2: the smallest shape that reaches the second chunk and keeps the lists
cheap), with the rows 262140 .. 262150 -- across the boundary -- made equal.  The want side
(tests/graph_reference_large.py, proven on the CPU in tests/test_graph_reference_large.py):
  * the lists of all pairs with d < R from a uniform grid and the reference's fold, checked per sampled row against
    oracle.brute_radius and per sampled pair against the oracle's scalar distance (the oracle's tree walk would take
    seconds as well, but it accepts a whole node on an upper bound <= R: that is not the strict '<' set);
  * sparse_mst over those pairs.  It is the tree of the complete graph because the certificate of its docstring holds,
    asserted in ``want_side``: the forest spans and its largest key is below the key of R; every row lists at least K
    others, so the K-th core distance is below R as well;
  * heap_optics over the lists cut to max_eps < R;
  * ref_hdbscan (tests/test_gpu_hdbscan.py) over sparse_mst's edges, its MIN_GAP condition asserted.
R = 0.0062: pi R^2 n = 32 entries per row on average; max_eps = 0.0035: 10 per row.  The same recipe cut to n = 2^18
exactly -- one full chunk, no remainder -- is the control.  Every comparison is array equality, floats by their bits.
"""
import numpy as np
import pytest

from conftest import uniform
from graph_reference_large import grid_lists, heap_optics, sparse_mst, truncate_lists
from optics_reference import core_from_lists, cpu_extract, fold_pairs, same_partition
from test_gpu_hdbscan import MIN_GAP, ref_hdbscan
from test_gpu_linkage import check_linkage
from test_gpu_mst import keys_of
from test_gpu_optics import same

pytestmark = pytest.mark.gpu

PN_OPT_OPTICS_PIECE = 13
CHUNK = 1 << 18
N = CHUNK + 3000
R = 0.0062
MAX_EPS = 0.0035
K = 5
SEED = 2718


def rows_of(dtype):
    pts = uniform((N, 2), SEED, dtype)
    pts[262140:262151] = pts[262140]
    return pts


def full_lists(oracle_mod, dtype):
    """the lists at R of all N rows, checked against the oracle on a sample"""
    pts = rows_of(dtype)
    off, idx, dist = grid_lists(pts, dtype(R))
    rng = np.random.default_rng(1)
    for i in np.r_[rng.integers(0, N, 40), 262139, 262140, 262150, 262151, CHUNK - 1, CHUNK, N - 1]:
        want = oracle_mod.brute_radius(pts, pts[i], dtype(R))
        assert np.array_equal(idx[off[i]:off[i + 1]], want[want != i].astype(np.int64)), i
    rows = np.repeat(np.arange(N), np.diff(off))
    for t in rng.integers(0, len(idx), 300):
        assert oracle_mod.euclidean(pts[rows[t]], pts[idx[t]]) == dist[t]
    return pts, off, idx, dist


def pieces_of(h_off, n, piece):
    """the pieces [a, b) the fill loop cuts: at most `piece` entries and at most 2^18 rows each, at least one row"""
    out, a = [], 0
    while a < n:
        lim = n if n - a < CHUNK else a + CHUNK
        b = int(np.searchsorted(h_off[a + 1:lim + 1], h_off[a] + piece, side="right")) + a
        b = max(b, a + 1)
        out.append((a, b))
        a = b
    return out


def mst_want(n, off, idx, dist, core, what):
    """sparse_mst over the listed pairs, with the certificate"""
    rows = np.repeat(np.arange(n), np.diff(off))
    up = rows < idx
    i, j = rows[up], idx[up]
    key = keys_of(dist[up], False)
    if core is not None:
        ck = keys_of(core, False)
        key = np.maximum(np.maximum(key, ck[i]), ck[j])
    lo, hi, k, spans = sparse_mst(n, i, j, key)
    r_key = keys_of(np.array([R], dtype=dist.dtype), False)[0]
    print(f"{what}: {len(i)} candidate edges, spans {spans}, largest tree key {int(k.max())} against R's {int(r_key)}, "
          f"{int(np.count_nonzero(k == 0))} zero weights")
    assert spans and k.max() < r_key, what  # the certificate
    return lo, hi, k


def optics_want(n, off, idx, dist, what, boundary):
    o_off, o_idx, o_dist = truncate_lists(off, idx, dist, n, dist.dtype.type(MAX_EPS))
    want = heap_optics(o_off, o_idx, o_dist, K)
    o, r, p, c = want
    n_inf_core = int(np.count_nonzero(np.isinf(c)))
    n_unreached = int(np.count_nonzero(np.isinf(r)))
    hi_rows = np.arange(n) >= CHUNK
    down = int(np.count_nonzero(hi_rows & (p >= 0) & (p < CHUNK)))
    upw = int(np.count_nonzero(~hi_rows & (p >= CHUNK)))
    print(f"{what}: {float(o_off[-1]) / n:.1f} entries per row at max_eps, {n_inf_core} rows with infinite core, "
          f"{n_unreached} unreached, predecessors across the boundary {down} down / {upw} up")
    assert 8 < float(o_off[-1]) / n < 12 and n_inf_core >= 1000 and n_unreached >= 100, what
    if boundary:
        assert down >= 100 and upw >= 100, what
    stored = np.where(np.isfinite(c), np.diff(o_off), 0)  # (the stored lists are the core rows')
    h_off = np.concatenate([[0], np.cumsum(stored)])
    return want, h_off


def want_side(oracle_mod):
    """everything the module compares against, with every condition asserted: runs without a GPU"""
    w = {}
    pts, off, idx, dist = full_lists(oracle_mod, np.float32)
    counts = np.diff(off)
    print(f"lists at R = {R}: {float(off[-1]) / N:.1f} entries per row, fewest {int(counts.min())}")
    assert 25 < float(off[-1]) / N < 40 and counts.min() >= K
    assert np.count_nonzero(dist[off[262140]:off[262141]] == 0) == 10  # (the planted duplicates)
    w["pts"] = pts
    for name, n in (("big", N), ("control", CHUNK)):
        t_off, t_idx, t_dist = truncate_lists(off, idx, dist, n)
        assert np.diff(t_off).min() >= K, name
        core = core_from_lists(t_off, t_dist, K)
        assert np.isfinite(core).all() and core.max() < np.float32(R), name
        w[name] = {"n": n, "core": core,
                   "plain": mst_want(n, t_off, t_idx, t_dist, None, f"{name}: plain tree"),
                   "cored": mst_want(n, t_off, t_idx, t_dist, core, f"{name}: tree under the k = {K} cores")}
        w[name]["optics"], w[name]["h_off"] = optics_want(n, t_off, t_idx, t_dist, f"{name}: OPTICS", n > CHUNK)
    total = int(w["big"]["h_off"][-1])
    piece = total // 3 + 1000
    cut = pieces_of(w["big"]["h_off"], N, piece)
    print(f"OPTICS pieces of {piece} of {total} stored entries: {cut}; default piece: {pieces_of(w['big']['h_off'], N, 1 << 27)}")
    assert any(b <= CHUNK for a, b in cut) and any(a < CHUNK < b for a, b in cut)  # inside a chunk, and across the boundary
    assert pieces_of(w["big"]["h_off"], N, 1 << 27) == [(0, CHUNK), (CHUNK, N)]   # the default piece ends at the row limit
    w["piece"] = piece
    return w


def want_side_f64(oracle_mod):
    pts, off, idx, dist = full_lists(oracle_mod, np.float64)
    want, h_off = optics_want(N, off, idx, dist, "f64: OPTICS", True)
    return pts, want, int(h_off[-1]) // 3 + 1000


@pytest.fixture(scope="module")
def want(oracle_mod):
    return want_side(oracle_mod)


@pytest.fixture(scope="module")
def trees(pn, want):
    out = {"big": pn.BallTree.euclidean(want["pts"]), "control": pn.BallTree.euclidean(np.ascontiguousarray(want["pts"][:CHUNK]))}
    yield out
    for t in out.values():
        t.close()


def same_edges(got, want, what):
    src, dst, weight = got
    lo, hi, key = want
    u = key.dtype
    print(f"{what}: differing edges {int(np.count_nonzero((src != lo) | (dst != hi)))}, "
          f"weights {int(np.count_nonzero(weight.view(u) != key))}")
    assert np.array_equal(src, lo) and np.array_equal(dst, hi) and np.array_equal(weight.view(u), key), what


# ---- MST and the dendrogram
@pytest.mark.parametrize("name", ["big", "control"])
def test_mst_without_cores(want, trees, name):
    w, tree = want[name], trees[name]
    src, dst, weight = tree.mst(None)
    print(f"{name}: rounds and rows scanned {tree.last_mst_work}")
    same_edges((src.astype(np.int64), dst.astype(np.int64), weight), w["plain"], f"{name}: mst(None)")
    ds, dd, dw = tree.mst_device(None)
    same_edges((ds.cpu().numpy(), dd.cpu().numpy(), dw.cpu().numpy()), w["plain"], f"{name}: mst_device(None)")


@pytest.mark.parametrize("name", ["big", "control"])
def test_mst_with_cores(want, trees, name):
    import torch
    w, tree = want[name], trees[name]
    src, dst, weight = tree.mst(w["core"])
    same_edges((src.astype(np.int64), dst.astype(np.int64), weight), w["cored"], f"{name}: mst(core)")
    ds, dd, dw = tree.mst_device(torch.from_numpy(w["core"]).cuda())
    same_edges((ds.cpu().numpy(), dd.cpu().numpy(), dw.cpu().numpy()), w["cored"], f"{name}: mst_device(core)")
    # the library's own K-th column is the lists' core distance
    assert tree.query_self(K)[1][:, -1].tobytes() == w["core"].tobytes()


def test_linkage_of_the_tree(want, trees):
    lo, hi, key = want["big"]["cored"]
    check_linkage(trees["big"], (lo.astype(np.uint64), hi.astype(np.uint64), key.view(np.float32)), "2^18 + 3000 rows")


# ---- HDBSCAN
@pytest.mark.parametrize("m", [5, 50])
def test_hdbscan(want, trees, m):
    lo, hi, key = want["big"]["cored"]
    tree = trees["big"]
    w_labels, w_prob, w_ncl, info = ref_hdbscan(N, lo, hi, key.view(np.float32), m, np.float32)
    print(f"m = {m}: reference {w_ncl} clusters, {info['noise']} noise rows, {info['condensed']} condensed clusters, "
          f"least gap {info['gap']:.3g}")
    assert info["gap"] >= MIN_GAP and w_ncl >= 2  # (conditions on the input)
    labels, prob = tree.hdbscan(m, K)
    print(f"m = {m}: device {tree.last_n_clusters} clusters, differing labels {int(np.count_nonzero(labels != w_labels))}, "
          f"probabilities {int(np.count_nonzero(prob.view(np.uint32) != w_prob.view(np.uint32)))}")
    assert tree.last_n_clusters == w_ncl and np.array_equal(labels, w_labels)
    assert np.array_equal(prob.view(np.uint32), w_prob.view(np.uint32))
    if m == 5:
        dl, dp, dn = tree.hdbscan_device(m, K)
        assert int(dn.cpu()[0]) == w_ncl and np.array_equal(dl.cpu().numpy(), w_labels)
        assert np.array_equal(dp.cpu().numpy().view(np.uint32), w_prob.view(np.uint32))


# ---- OPTICS
@pytest.mark.parametrize("name", ["big", "control"])
def test_optics(want, trees, name):
    w, tree = want[name], trees[name]
    tree.set_option(PN_OPT_OPTICS_PIECE, want["piece"])  # pieces inside the chunks and across the boundary
    same(tree.optics(K, np.float32(MAX_EPS)), w["optics"], f"{name}: optics, pieces of {want['piece']} entries (host)")
    tree.set_option(PN_OPT_OPTICS_PIECE, 0)              # the default: a piece ends at the 2^18-row limit
    dev = [t.cpu().numpy() for t in tree.optics_device(K, np.float32(MAX_EPS))]
    same(dev, w["optics"], f"{name}: optics, default piece (device)")


def test_optics_f64(pn, oracle_mod):
    pts, w, piece = want_side_f64(oracle_mod)
    tree = pn.BallTree.euclidean(pts)
    tree.set_option(PN_OPT_OPTICS_PIECE, piece)
    same(tree.optics(K, MAX_EPS), w, "f64: optics (host)")
    tree.close()


def test_extraction_at_half_max_eps(want, trees):
    import torch
    tree = trees["big"]
    w_o, w_r, w_p, w_c = want["big"]["optics"]
    eps = np.float32(MAX_EPS / 2)
    w_labels, w_ncl = cpu_extract(w_o, w_r, w_c, eps)
    print(f"eps' = max_eps / 2: {w_ncl} clusters, {int(np.count_nonzero(w_labels < 0))} noise rows")
    assert w_ncl >= 2
    labels, ncl = tree.optics_dbscan(eps, w_o, w_r, w_c)
    assert np.array_equal(labels, w_labels) and ncl == w_ncl
    d_labels, d_ncl, d_err = tree.optics_dbscan_device(eps, torch.from_numpy(w_o.astype(np.int64)).cuda(),
                                                       torch.from_numpy(w_r).cuda(), torch.from_numpy(w_c).cuda())
    assert np.array_equal(d_labels.cpu().numpy(), w_labels) and int(d_ncl.item()) == w_ncl and int(d_err.item()) == 0
    # against dbscan on the same tree: the rows with core < eps' are DBSCAN(eps', K + 1)'s core rows, and both labelings
    # split them into the same density-connected components (border rows may differ)
    db_labels, db_core = tree.dbscan(eps, K + 1)
    near = w_c < eps
    assert np.array_equal(db_core, near)
    assert (labels[near] >= 0).all() and same_partition(labels[near], db_labels[near])
    assert w_ncl == int(db_labels.max()) + 1
