"""tests/graph_reference_large.py -- references that scale beyond 2^18 rows -- against the quadratic references they
stand in for, on the CPU: equal arrays, bit for bit.

  * heap_optics == optics_reference.cpu_optics on random CSR graphs (f32, f64, with unreachable rows and many equal
    distances) and on the hand-made tie cases of tests/test_optics_reference.py;
  * sparse_mst == test_gpu_mst.prim on dense matrices, cored and uncored, the candidates cut at an R for which the
    certificate of its docstring holds (asserted here as the GPU test must assert it);
  * grid_lists == the dense fold's lists.
"""
import numpy as np
import pytest

from graph_reference_large import grid_lists, heap_optics, sparse_mst, truncate_lists
from optics_reference import cpu_optics, csr_from_dense, fold_pairs
from test_gpu_mst import core_keys_from, fold_distances, keys_of, prim, weight_keys
from test_optics_reference import fold_matrix


def same_four(got, want, what):
    for g, w, name in zip(got, want, ("ordering", "reachability", "predecessor", "core")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: {name} differs"


def random_graph(seed, n, dtype, mean, levels):
    """a symmetric random graph as CSR lists; the distances take `levels` distinct values (0: all distinct), so the
    (reach, row) order and the strict '<' of an offer decide many picks"""
    rng = np.random.default_rng(seed)
    m = n * mean // 2
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    pairs = np.unique(lo * n + hi)
    lo, hi = pairs // n, pairs % n
    w = rng.random(len(lo)) if not levels else rng.integers(1, levels + 1, len(lo)) / levels
    i, j, d = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([w, w]).astype(dtype)
    cut = rng.random(n) < 0.05  # rows that list nothing and that nobody lists: unreachable
    keep = ~cut[i] & ~cut[j]
    i, j, d = i[keep], j[keep], d[keep]
    order = np.lexsort((j, i))
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(i, minlength=n))
    return off, j[order], d[order]


@pytest.mark.parametrize("seed, n, dtype, mean, levels, ms", [
    (1, 2000, np.float32, 8, 0, 4), (2, 3500, np.float64, 12, 0, 5), (3, 5000, np.float32, 10, 7, 5),
    (4, 2500, np.float64, 6, 3, 2), (5, 3000, np.float32, 4, 0, 6)])
def test_heap_optics_equals_cpu_optics_on_random_graphs(seed, n, dtype, mean, levels, ms):
    off, idx, dist = random_graph(seed, n, dtype, mean, levels)
    stats = {}
    want = cpu_optics(off, idx, dist, ms, stats)
    n_inf_core = int(np.count_nonzero(np.isinf(want[3])))
    n_unreached = int(np.count_nonzero(np.isinf(want[1])))
    print(f"n {n}: {n_inf_core} rows without a core, {n_unreached} unreached, {stats['tie_picks']} tie picks")
    assert n_inf_core >= 50 and n_unreached >= 50 and np.count_nonzero(np.isfinite(want[1])) >= n // 2
    if levels:
        assert stats["tie_picks"] >= 500
    same_four(heap_optics(off, idx, dist, ms), want, f"random graph {seed}")


def test_heap_optics_on_the_hand_made_tie_cases():
    cases = [(np.arange(8.0), 1, 1.5), (np.arange(8.0), 2, 2.5), (np.arange(8.0)[[4, 3, 5, 2, 6, 1, 7, 0]], 1, 1.5),
             (np.arange(8.0), 1, 1.0), ([0.0, 0.0, 0.0, 1.0], 2, 2.0), ([0.0, 1.0, -1.0], 1, 1.5),
             ([5.0, -1.0, 0.0, 1.0], 1, 1.5), ([0.0, 1.0, 9.0, -0.5], 1, 1.2)]
    for x, ms, eps in cases:
        x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
        graph = csr_from_dense(fold_matrix(x), eps)
        same_four(heap_optics(*graph, ms), cpu_optics(*graph, ms), f"{x.ravel().tolist()}, ms {ms}")
    o, r, p, c = heap_optics(*csr_from_dense(fold_matrix(np.array([[0.0], [1.0], [9.0], [-0.5]])), 1.2), 1)
    assert o.tolist() == [0, 3, 1, 2] and p.tolist() == [-1, 0, -1, 0]  # (one of them spelled out)


def candidates_below(d, r):
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero(np.triu(d < r, 1))
    return i, j


def check_sparse(d, k, r, what):
    """sparse_mst over the pairs with d < r against prim over the dense matrix, with the certificate"""
    n = len(d)
    dk = keys_of(d, False)
    ck = None if k is None else core_keys_from(dk, k)
    wk = weight_keys(dk, ck)
    want = prim(wk)
    i, j = candidates_below(d, r)
    lo, hi, key, spans = sparse_mst(n, i, j, wk[i, j])
    r_key = keys_of(np.array([r], dtype=d.dtype), False)[0]
    print(f"{what}: {len(i)} candidate edges of {n * (n - 1) // 2}, largest tree key {int(key.max())} against R's {int(r_key)}")
    assert len(i) < n * (n - 1) // 4        # (fewer than half of all pairs: the candidates are a real restriction)
    assert spans and key.max() < r_key      # the certificate
    assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]) and np.array_equal(key, want[2]), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k", [None, 5])
def test_sparse_mst_equals_prim_on_uniform_rows(dtype, k):
    rng = np.random.default_rng(7)
    x = rng.random((2200 if dtype == np.float32 else 1500, 2)).astype(dtype)
    check_sparse(fold_distances(x), k, dtype(0.12), f"uniform {len(x)} x 2 {np.dtype(dtype).name}, k = {k}")


@pytest.mark.parametrize("k", [None, 8])
def test_sparse_mst_equals_prim_on_blobs(k):
    from test_gpu_mst import blobs
    x = blobs(5, 3000, 4, 6, 0.05, 0.10)
    check_sparse(fold_distances(x), k, np.float32(0.45), f"blobs 3000 x 4, k = {k}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k", [None, 5])
def test_sparse_mst_equals_prim_on_the_lattice_with_duplicates(dtype, k):
    g = np.arange(40, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    x = np.concatenate([pts, pts[[3, 3, 41, 800, 800, 800, 1599, 7, 1200, 1201]]]).astype(dtype)
    assert len(x) == 1610
    # nothing but ties: plain, every tree edge weighs 0 or 1; with the k = 5 cores at most 2 (a corner's fifth other row)
    check_sparse(fold_distances(x), k, dtype(2.5), f"lattice {np.dtype(dtype).name}, k = {k}")


def test_sparse_mst_reports_a_forest_that_does_not_span():
    x = np.array([[0.0], [1.0], [10.0], [11.0]])
    dk = keys_of(fold_distances(x), False)
    i, j = candidates_below(fold_distances(x), 2.0)
    lo, hi, key, spans = sparse_mst(4, i, j, dk[i, j])
    assert not spans and lo.tolist() == [0, 2] and hi.tolist() == [1, 3]
    # an edge listed from both ends, and a loop of whatever key (the smallest, the largest), change nothing
    for loop_key in (0, np.iinfo(dk.dtype).max):
        keys = np.concatenate([dk[i, j], dk[j, i], np.array([loop_key], dtype=dk.dtype)])
        lo2, hi2, key2, spans2 = sparse_mst(4, np.r_[i, j, 1], np.r_[j, i, 1], keys)
        assert not spans2 and np.array_equal(lo, lo2) and np.array_equal(hi, hi2) and np.array_equal(key, key2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_grid_lists_equal_the_dense_fold(dtype):
    rng = np.random.default_rng(3)
    x = rng.random((3000, 2)).astype(dtype)
    x[100:105] = x[7]          # duplicates: distance 0
    x[200] = [0.0, 0.0]        # the grid's corners
    x[201] = np.nextafter(dtype(1), dtype(0))
    for r in (0.05, 0.013, 0.7):
        off, idx, dist = grid_lists(x, dtype(r))
        w_off, w_idx, w_dist = csr_from_dense(fold_distances(x), dtype(r))
        assert np.array_equal(off, w_off) and np.array_equal(idx, w_idx) and dist.tobytes() == w_dist.tobytes(), r
    off, idx, dist = grid_lists(x, dtype(0.05))
    t_off, t_idx, t_dist = truncate_lists(off, idx, dist, 1234, dtype(0.02))
    w_off, w_idx, w_dist = csr_from_dense(fold_distances(x[:1234]), dtype(0.02))
    assert np.array_equal(t_off, w_off) and np.array_equal(t_idx, w_idx) and t_dist.tobytes() == w_dist.tobytes()
    assert fold_pairs(x, np.array([7]), np.array([100]))[0] == 0
