"""pn_linkage_*: the single-linkage dendrogram of sorted tree edges, against a sequential union-find in Python.

The reference walks the library's own ``mst`` edges in order: for edge r it looks up the current node of each end's
component (a row, or n + the last merge that touched it), writes them as left[r] (src's side) and right[r] (dst's side),
and unites.  Every comparison is exact equality of left, right, size and the weights' bit patterns, from both ``linkage``
and ``linkage_device``.
"""
import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE = 3


def seq_linkage(n, src, dst, base=0):
    """(left, right, size) int64 [n - 1] of the edges in the given order, and whether they span the n rows"""
    ne = len(src)
    parent = list(range(n))
    node = list(range(n))
    count = [1] * n
    left = np.empty(ne, dtype=np.int64)
    right = np.empty(ne, dtype=np.int64)
    size = np.empty(ne, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    ok = True
    for r in range(ne):
        a, b = find(int(src[r]) - base), find(int(dst[r]) - base)
        left[r], right[r] = node[a], node[b]
        if a == b:
            ok = False
        else:
            parent[b] = a
            count[a] += count[b]
        node[a] = n + r
        size[r] = count[a]
    return left, right, size, ok and (ne == 0 or size[-1] == n)


def _uint(dtype):
    return np.uint32 if np.dtype(dtype) == np.float32 else np.uint64


def check_linkage(tree, edges, what, base=0):
    """linkage and linkage_device of `edges` against the reference; returns the reference (left, right, size)"""
    import torch
    n = tree._n
    src, dst, w = edges
    u = _uint(w.dtype)
    w_left, w_right, w_size, ok = seq_linkage(n, src, dst, base)
    assert ok, what
    left, right, weight, size = tree.linkage(edges=edges)
    print(f"{what}: {len(src)} merges, differing left {int(np.count_nonzero(left != w_left.astype(np.uint64)))}, right "
          f"{int(np.count_nonzero(right != w_right.astype(np.uint64)))}, size "
          f"{int(np.count_nonzero(size != w_size.astype(np.uint64)))}")
    assert left.dtype == np.uint64 and right.dtype == np.uint64 and size.dtype == np.uint64 and weight.dtype == w.dtype
    assert np.array_equal(left, w_left.astype(np.uint64)), what
    assert np.array_equal(right, w_right.astype(np.uint64)), what
    assert np.array_equal(size, w_size.astype(np.uint64)), what
    assert np.array_equal(weight.view(u), w.view(u)), what
    d_edges = (torch.from_numpy(src.astype(np.int64)).cuda(), torch.from_numpy(dst.astype(np.int64)).cuda(),
               torch.from_numpy(w.copy()).cuda())
    dl, dr, dw, ds, err = tree.linkage_device(edges=d_edges)
    assert int(err.cpu()[0]) == 0, what
    assert np.array_equal(dl.cpu().numpy(), w_left) and np.array_equal(dr.cpu().numpy(), w_right), what
    assert np.array_equal(ds.cpu().numpy(), w_size), what
    assert np.array_equal(dw.cpu().numpy().view(u), w.view(u)), what
    return w_left, w_right, w_size


def height_of(n, left, right):
    h = np.zeros(2 * n - 1, dtype=np.int64)
    for r in range(n - 1):
        h[n + r] = 1 + max(h[left[r]], h[right[r]])
    return int(h[-1]) if n > 1 else 0


# ---- (a) sizes around the padding of the rank to a power of two
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1024, 1025, 1026])
def test_sizes_around_the_padding(pn, n):
    x = uniform((n, 3), 100 + n)
    tree = pn.BallTree.euclidean(x)
    edges = tree.mst()
    assert len(edges[0]) == n - 1
    check_linkage(tree, edges, f"uniform {n} x 3")
    left, right, weight, size = tree.linkage()  # (the default: the tree's own mst)
    assert len(left) == n - 1 and (n == 1 or size[-1] == n)
    if n > 1:
        core = tree.query_self(min(2, n - 1))[1][:, -1]
        check_linkage(tree, tree.mst(core), f"uniform {n} x 3, cores")
        l2 = tree.linkage(core)
        l3 = tree.linkage(edges=tree.mst(core))
        assert all(np.array_equal(a, b) for a, b in zip(l2, l3))
    tree.close()


# ---- (b) the deepest tree: a chain
def test_chain_of_height_n_minus_one(pn):
    n = 2000
    gaps = 1.0 + np.arange(n - 1) / 1000.0  # strictly growing: the edges sort left to right
    x = np.concatenate([[0.0], np.cumsum(gaps)]).reshape(n, 1)
    tree = pn.BallTree.euclidean(x)
    edges = tree.mst()
    assert np.array_equal(edges[0], np.arange(n - 1, dtype=np.uint64)) and np.array_equal(edges[1], edges[0] + 1)
    left, right, size = check_linkage(tree, edges, "chain 2000")
    assert height_of(n, left, right) == n - 1
    assert np.array_equal(size, np.arange(2, n + 1))
    tree.close()


# ---- (c) ties decided by rank alone: the lattice with duplicates of test_gpu_mst.py
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lattice_ties_follow_the_rank(pn, dtype):
    g = np.arange(40, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    x = np.concatenate([pts, pts[[3, 3, 41, 800, 800, 800, 1599, 7, 1200, 1201]]]).astype(dtype)
    assert len(x) == 1610
    tree = pn.BallTree.euclidean(x)
    edges = tree.mst()
    assert np.count_nonzero(edges[2] == 0) == 10 and np.count_nonzero(edges[2] == 1) == 1599  # nothing but ties
    check_linkage(tree, edges, f"lattice {np.dtype(dtype).name}")
    core = tree.query_self(5)[1][:, -1]
    check_linkage(tree, tree.mst(core), f"lattice {np.dtype(dtype).name}, k = 5 cores")
    tree.close()


# ---- (d) NaN weights, an index base, a shuffled order, edges that are no tree
@pytest.fixture(scope="module")
def nan_case():
    x = uniform((600, 3), 4711)
    x[17, 1] = np.nan
    x[405] = np.nan
    return x


def test_nan_weights_and_index_base(pn, nan_case):
    tree = pn.BallTree.euclidean(nan_case)
    edges = tree.mst()
    assert np.count_nonzero(np.isnan(edges[2])) == 2 and np.isnan(edges[2][-2:]).all()
    left, right, size = check_linkage(tree, edges, "600 x 3 with two NaN rows")
    assert {int(right[-2]), int(right[-1])} == {17, 405}  # each NaN row joins last, alone
    tree.set_option(PN_OPT_INDEX_BASE, 1000)
    based = tree.mst()
    assert np.array_equal(based[0], edges[0] + 1000) and np.array_equal(based[1], edges[1] + 1000)
    l2, r2, s2 = check_linkage(tree, based, "index base 1000", base=1000)
    assert np.array_equal(l2, left) and np.array_equal(r2, right) and np.array_equal(s2, size)  # node ids carry no base
    tree.close()


def test_a_shuffled_order_gives_the_tree_of_that_order(pn, nan_case):
    tree = pn.BallTree.euclidean(nan_case)
    src, dst, w = tree.mst()
    perm = np.random.default_rng(5).permutation(len(src))
    shuffled = (src[perm].copy(), dst[perm].copy(), w[perm].copy())
    left, right, size = check_linkage(tree, shuffled, "shuffled edges")
    l0, r0, _, _ = seq_linkage(len(nan_case), src, dst)
    assert not np.array_equal(left, l0)  # (it is another tree)
    tree.close()


def test_edges_that_are_no_spanning_tree_are_refused(pn, nan_case):
    import torch
    from petal_neighbors_amd import _lib
    tree = pn.BallTree.euclidean(nan_case)
    src, dst, w = tree.mst()
    n = len(nan_case)
    bad_sets = {"a repeated edge": (np.r_[src[:-1], src[0]], np.r_[dst[:-1], dst[0]], w),
                "an end that is no row": (src, np.r_[dst[:-1], np.uint64(n)], w)}
    for what, edges in bad_sets.items():
        with pytest.raises(pn.PetalError) as ei:
            tree.linkage(edges=edges)
        assert ei.value.code == _lib.PN_ERR_INVALID and "spanning tree" in str(ei.value), what
        d_edges = (torch.from_numpy(edges[0].astype(np.int64)).cuda(), torch.from_numpy(edges[1].astype(np.int64)).cuda(),
                   torch.from_numpy(edges[2].copy()).cuda())
        err = tree.linkage_device(edges=d_edges)[4]
        assert int(err.cpu()[0]) == _lib.PN_ERR_INVALID, what
    # and the handle goes on working
    check_linkage(tree, (src, dst, w), "after the refusals")
    tree.close()


# ---- (e) the caller's stream and outputs, twice
def test_device_entry_on_a_stream_with_given_outputs(pn, nan_case):
    import torch
    n = len(nan_case)
    tree = pn.BallTree.euclidean(nan_case)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    edges = tree.mst_device()
    src, dst = edges[0].cpu().numpy(), edges[1].cpu().numpy()
    w_left, w_right, w_size, ok = seq_linkage(n, src, dst)
    assert ok
    left = torch.full((n - 1,), -7, dtype=torch.int64, device=dev)
    right = torch.full((n - 1,), -7, dtype=torch.int64, device=dev)
    size = torch.full((n - 1,), -7, dtype=torch.int64, device=dev)
    wgt = torch.zeros(n - 1, dtype=torch.float32, device=dev)
    err = torch.full((1,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for rep in range(2):  # a repeated call reuses the workspace
        with torch.cuda.stream(st):
            r = tree.linkage_device(edges=edges, out_left=left, out_right=right, out_weight=wgt, out_size=size,
                                    out_error=err, stream=st.cuda_stream)
        st.synchronize()
        assert r[0] is left and r[1] is right and r[2] is wgt and r[3] is size and r[4] is err
        assert int(err.cpu()[0]) == 0
        assert np.array_equal(left.cpu().numpy(), w_left) and np.array_equal(right.cpu().numpy(), w_right)
        assert np.array_equal(size.cpu().numpy(), w_size)
        assert np.array_equal(wgt.cpu().numpy().view(np.uint32), edges[2].cpu().numpy().view(np.uint32))
        left.fill_(-7)
        err.fill_(99)
        torch.cuda.synchronize()
    # the weights may be copied onto themselves
    r = tree.linkage_device(edges=edges, out_weight=edges[2])
    assert r[2] is edges[2] and np.array_equal(r[0].cpu().numpy(), w_left)
    with pytest.raises(ValueError):
        tree.linkage_device(edges=edges, out_left=left[:10])
    with pytest.raises(ValueError):
        tree.linkage_device(edges=edges, out_weight=wgt.double())
    with pytest.raises(ValueError):
        tree.linkage_device(edges=(edges[0][:-1], edges[1], edges[2]))
    with pytest.raises(ValueError):
        tree.linkage(edges=(src[:-1], dst, edges[2].cpu().numpy()))
    tree.close()
