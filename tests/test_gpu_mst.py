"""pn_mst_*: the exact minimum spanning tree of the indexed rows under mutual reachability, against numpy alone.

The contract (include/petal_mi355x.h): the edge {i, j}, i < j, weighs w = max(d(i, j), core[i], core[j]) in the library's
key order, edges are ordered by (key(w), i, j), and the answer is the unique MST under that strict order, its n - 1 edges
ascending.  The reference here:
  * distances: the sequential unfused fold in the index's dtype -- a loop over the coordinates doing acc += (q - p) * (q - p),
    then sqrt --, bit-identical to the library's by construction and checked on sampled pairs against the oracle's scalar
    distance; Cosine: the oracle's own pairwise matrix of its scalar function;
  * core distances: the k-th smallest off-diagonal key of each row of the dense matrix;
  * the tree: a vectorised Prim that picks its minimum by (key, lo, hi) -- under a strict order Prim yields the same unique
    tree --, its edges sorted at the end.
Every comparison is exact array equality of src, dst and the weights' bit patterns, from both mst and mst_device.
"""
import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE = 3
PN_OPT_MST_BATCH = 12


# ------------------------------------------------------------------------------------------------ numpy reference
def _uint(dtype):
    return np.uint32 if np.dtype(dtype) == np.float32 else np.uint64


def keys_of(v, signed):
    """the library's sortable keys: unsigned map (distances; anything <= 0 is the key of +0, NaN above +inf) or the signed
    map of all floats (Cosine; -0 counts as +0)"""
    v = np.asarray(v)
    u = _uint(v.dtype)
    bits = 32 if u == np.uint32 else 64
    sign = u(1 << (bits - 1))
    nan = np.isnan(v)
    if signed:
        b = np.where(v == 0, v.dtype.type(0), v).view(u)
        k = np.where(b & sign, ~b, b | sign)
        return np.where(nan, u(0xFFC00000 if bits == 32 else 0xFFF8000000000000), k).astype(u)
    with np.errstate(invalid="ignore"):
        k = np.where(v <= 0, u(0), v.view(u))
    return np.where(nan, u(0x7FC00000 if bits == 32 else 0x7FF8000000000000), k).astype(u)


def bits_of_keys(k, signed):
    """bit patterns of the values the keys stand for"""
    if not signed:
        return k
    sign = k.dtype.type(1 << (k.dtype.itemsize * 8 - 1))
    return np.where(k & sign, k ^ sign, ~k).astype(k.dtype)


def fold_distances(x):
    """dense Euclidean matrix by the reference's fold, in x's dtype: acc += (q - p) * (q - p) per coordinate, then sqrt"""
    n, dim = x.shape
    acc = np.zeros((n, n), dtype=x.dtype)
    diff = np.empty((n, n), dtype=x.dtype)
    with np.errstate(invalid="ignore"):
        for k in range(dim):
            np.subtract(x[:, None, k], x[None, :, k], out=diff)
            np.multiply(diff, diff, out=diff)
            np.add(acc, diff, out=acc)
        np.sqrt(acc, out=acc)
    return acc


def core_keys_from(dkeys, k):
    """key of the k-th smallest off-diagonal entry of each row"""
    big = np.iinfo(dkeys.dtype).max
    m = dkeys.copy()
    np.fill_diagonal(m, big)
    return np.partition(m, k - 1, axis=1)[:, k - 1].copy()


def weight_keys(dkeys, ckeys):
    if ckeys is None:
        return dkeys
    return np.maximum(np.maximum(dkeys, ckeys[:, None]), ckeys[None, :])


def prim(wk):
    """the MST under (key, lo, hi): (lo, hi, key) arrays sorted in edge order"""
    n = len(wk)
    if n < 2:
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(0, dtype=wk.dtype)
    big = np.iinfo(wk.dtype).max
    ids = np.arange(n, dtype=np.int64)
    in_tree = np.zeros(n, dtype=bool)
    in_tree[0] = True
    bk = wk[0].copy()
    blo, bhi = np.zeros(n, dtype=np.int64), ids.copy()  # the edge {0, u}
    bk[0] = big
    blo[0] = bhi[0] = n
    out = np.empty((n - 1, 2), dtype=np.int64)
    outk = np.empty(n - 1, dtype=wk.dtype)
    for e in range(n - 1):
        m = bk.min()
        cand = np.flatnonzero((bk == m) & ~in_tree)
        pair = blo[cand] * n + bhi[cand]
        u = cand[np.argmin(pair)]
        out[e] = blo[u], bhi[u]
        outk[e] = m
        in_tree[u] = True
        bk[u] = big
        nk = wk[u]
        nlo, nhi = np.minimum(ids, u), np.maximum(ids, u)
        better = ~in_tree & ((nk < bk) | ((nk == bk) & ((nlo < blo) | ((nlo == blo) & (nhi < bhi)))))
        bk = np.where(better, nk, bk)
        blo = np.where(better, nlo, blo)
        bhi = np.where(better, nhi, bhi)
    order = np.lexsort((out[:, 1], out[:, 0], outk))
    return out[order, 0], out[order, 1], outk[order]


def simulate_rounds(wk, ckeys):
    """The library's rule on the CPU: Boruvka under (key, lo, hi), a row rescanned only when its cached partner has joined
    its component and its core key does not exceed the least cached key of its component's valid rows.  Returns (rounds,
    rows scanned)."""
    n = len(wk)
    big = np.iinfo(wk.dtype).max
    ck = np.zeros(n, dtype=wk.dtype) if ckeys is None else ckeys
    comp = np.arange(n)
    cj = np.full(n, -1, dtype=np.int64)
    ckey = np.zeros(n, dtype=wk.dtype)

    def scan(rows):
        for a in range(0, len(rows), 1024):
            r = rows[a:a + 1024]
            sub = np.where(comp[None, :] == comp[r][:, None], big, wk[r])
            j = sub.argmin(axis=1)  # (the first of equal keys: the smallest j)
            cj[r] = j
            ckey[r] = sub[np.arange(len(r)), j]

    scan(np.arange(n))
    rounds, scanned, ncomp = 0, n, n
    while True:
        valid = (cj >= 0) & (comp[np.maximum(cj, 0)] != comp)
        rows = np.flatnonzero(valid)
        lo, hi = np.minimum(rows, cj[rows]), np.maximum(rows, cj[rows])
        order = np.lexsort((hi, lo, ckey[rows], comp[rows]))
        first = np.r_[True, comp[rows][order][1:] != comp[rows][order][:-1]]
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for e in order[first]:
            a, b = find(int(comp[lo[e]])), find(int(comp[hi[e]]))  # (this round's forest is over the components)
            if a != b:
                parent[max(a, b)] = min(a, b)
        roots = np.array([find(int(c)) for c in np.unique(comp)])
        comp = roots[np.searchsorted(np.unique(comp), comp)]
        rounds += 1
        ncomp = len(np.unique(comp))
        if ncomp == 1:
            return rounds, scanned
        valid = (cj >= 0) & (comp[np.maximum(cj, 0)] != comp)
        cmin = np.full(n, big, dtype=wk.dtype)
        np.minimum.at(cmin, comp[valid], ckey[valid])
        listed = np.flatnonzero(~valid & (ck <= cmin[comp]))
        scanned += len(listed)
        scan(listed)


def blobs(seed, n, dim, nb, sigma, background, shift=0.0):
    """Gaussian blobs around nb centres in [0, 1)^dim, a uniform background, rows permuted (as tests/test_gpu_dbscan.py)"""
    rng = np.random.default_rng(seed)
    centres = rng.random((nb, dim))
    n_bg = int(round(n * background))
    which = rng.integers(0, nb, n - n_bg)
    pts = np.concatenate([centres[which] + sigma * rng.standard_normal((n - n_bg, dim)), rng.random((n_bg, dim))])
    return (pts[rng.permutation(n)] + shift).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- checking
def check(tree, core, want, what, signed=False, base=0):
    """mst and mst_device against the reference (lo, hi, keys); returns the work counters of the host call"""
    import torch
    w_lo, w_hi, w_key = want
    w_bits = bits_of_keys(w_key, signed)
    u = w_key.dtype
    src, dst, weight = tree.mst(core)
    work = tree.last_mst_work
    bad = int(np.count_nonzero((src != w_lo.astype(np.uint64) + base) | (dst != w_hi.astype(np.uint64) + base)))
    print(f"{what}: {len(w_lo)} edges, rounds {work[0]}, rows scanned {work[1]}, differing edges {bad}, "
          f"differing weights {int(np.count_nonzero(weight.view(u) != w_bits))}")
    assert src.dtype == np.uint64 and dst.dtype == np.uint64 and weight.dtype == tree.dtype
    assert np.array_equal(src, w_lo.astype(np.uint64) + base), what
    assert np.array_equal(dst, w_hi.astype(np.uint64) + base), what
    assert np.array_equal(weight.view(u), w_bits), what
    d_core = None if core is None else torch.from_numpy(np.ascontiguousarray(core, dtype=tree.dtype)).cuda()
    ds, dd, dw = tree.mst_device(d_core)
    assert tree.last_mst_work == work, what
    assert np.array_equal(ds.cpu().numpy().astype(np.uint64), src) and np.array_equal(dd.cpu().numpy().astype(np.uint64), dst), what
    assert np.array_equal(dw.cpu().numpy().view(u), w_bits), what
    return work


def sampled_pairs_match_the_oracle(oracle_mod, x, dmat, seed, scalar):
    rng = np.random.default_rng(seed)
    u = _uint(x.dtype)
    for i, j in rng.integers(0, len(x), (100, 2)):
        if i == j:
            continue
        a, b = np.array([scalar(x[i], x[j])], dtype=x.dtype), dmat[i:i + 1, j]
        assert (np.isnan(a[0]) and np.isnan(b[0])) or a.view(u)[0] == b.view(u)[0], (i, j)


# ---- (a) ties: an integer lattice with duplicated rows -- only the edge order decides
@pytest.fixture(scope="module")
def lattice():
    g = np.arange(40, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    pts = np.concatenate([pts, pts[[3, 3, 41, 800, 800, 800, 1599, 7, 1200, 1201]]])
    out = {}
    for dt in (np.float32, np.float64):
        x = pts.astype(dt)
        dk = keys_of(fold_distances(x), False)
        ck = core_keys_from(dk, 5)
        out[np.dtype(dt).name] = (x, prim(dk), ck.view(dt), prim(weight_keys(dk, ck)))
    return out


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("cored", [False, True])
def test_lattice_ties_are_decided_by_the_edge_order(pn, lattice, dtype, cored):
    x, want_plain, core, want_cored = lattice[dtype]
    assert len(x) == 1610
    tree = pn.BallTree.euclidean(x)
    if cored:
        check(tree, core, want_cored, f"lattice {dtype}, k = 5 cores")
    else:
        check(tree, None, want_plain, f"lattice {dtype}")
        tree.set_option(PN_OPT_MST_BATCH, 100)
        check(tree, None, want_plain, f"lattice {dtype}, batch 100")
    tree.close()


# ---- (b) NaN rows, tiny indexes, an index base, a negative core value
def test_nan_rows_tiny_indexes_index_base_and_negative_cores(pn, oracle_mod):
    x = uniform((600, 3), 4711)
    x[17, 1] = np.nan
    x[405] = np.nan
    d = fold_distances(x)
    sampled_pairs_match_the_oracle(oracle_mod, x, d, 1, oracle_mod.euclidean)
    dk = keys_of(d, False)
    want = prim(dk)
    nan_key = np.uint32(0x7FC00000)
    n_nan = int(np.count_nonzero(want[2] == nan_key))
    assert n_nan == 2 and np.all(want[2][-2:] == nan_key)  # each NaN row hangs by one edge, and those come last
    assert want[0][-2] == 0 and want[1][-2] == 17 and want[0][-1] == 0 and want[1][-1] == 405  # ... ordered by (src, dst)
    tree = pn.BallTree.euclidean(x)
    before = tree.stats()["queries"]
    check(tree, None, want, "600 x 3 with two NaN rows")
    assert tree.stats()["queries"] - before == 2 * 600  # (mst + mst_device)
    # cores (k = 3; the NaN rows' are NaN), one entry negative: it acts as 0
    ck = core_keys_from(dk, 3)
    core = ck.view(np.float32).copy()
    core[7] = -1.0
    ck[7] = 0
    check(tree, core, prim(weight_keys(dk, ck)), "600 x 3, k = 3 cores, core[7] = -1")
    core[9] = -0.0
    ck[9] = 0
    check(tree, core, prim(weight_keys(dk, ck)), "600 x 3, k = 3 cores, core[9] = -0")
    tree.set_option(PN_OPT_INDEX_BASE, 1000)
    check(tree, None, want, "index base 1000", base=1000)
    check(tree, core, prim(weight_keys(dk, ck)), "index base 1000, cores", base=1000)
    tree.close()
    for n in (1, 2):
        t = pn.BallTree.euclidean(x[:n])
        for core in (None, np.array([0.5, 2.0], dtype=np.float32)[:n]):
            check(t, core, prim(weight_keys(dk[:n, :n], None if core is None else keys_of(core, False))), f"n = {n}")
        t.close()


# ---- (c), (d), (e): the tier-served round 0, engines, batches and the work counters on one set of blobs
@pytest.fixture(scope="module")
def blob_case(oracle_mod):
    x = blobs(5, 5000, 16, 12, 0.05, 0.10)
    d = fold_distances(x)
    sampled_pairs_match_the_oracle(oracle_mod, x, d, 2, oracle_mod.euclidean)
    dk = keys_of(d, False)
    del d
    ck = core_keys_from(dk, 8)
    wk = weight_keys(dk, ck)
    return {"x": x, "dk": dk, "ck": ck, "wk": wk, "plain": prim(dk), "cored": prim(wk)}


def test_blobs_round_zero_from_the_filter_tier_and_hdbscan_tree(pn, blob_case):
    c = blob_case
    tree = pn.BallTree.euclidean(c["x"])
    assert tree.bf16_eligible
    check(tree, None, c["plain"], "blobs 5000 x 16")
    core = tree.query_self(8)[1][:, -1]
    assert np.array_equal(core.view(np.uint32), c["ck"])  # (the dense matrix' 8th smallest: the same bits)
    check(tree, core, c["cored"], "blobs 5000 x 16, k = 8 cores")
    hs, hd, hw = tree.mst(core)
    ms, md, mw = tree.mutual_reachability_mst(8)
    assert np.array_equal(ms.cpu().numpy().astype(np.uint64), hs) and np.array_equal(md.cpu().numpy().astype(np.uint64), hd)
    assert np.array_equal(mw.cpu().numpy().view(np.uint32), hw.view(np.uint32))
    tree.close()


def test_engines_and_batches_never_change_an_edge(pn, blob_case):
    c = blob_case
    tree = pn.BallTree.euclidean(c["x"])
    core = c["ck"].view(np.float32)
    works = set()
    for eng in ("exact", "bf16", "auto"):
        tree.set_engine(eng)
        for batch in (0, 64, 1000):
            tree.set_option(PN_OPT_MST_BATCH, batch)
            w1 = check(tree, None, c["plain"], f"engine {eng}, batch {batch}")
            w2 = check(tree, core, c["cored"], f"engine {eng}, batch {batch}, cores")
            works.add((w1, w2))
    assert len(works) == 1  # the work is a function of the data as well
    with pytest.raises(Exception):
        tree.set_option(PN_OPT_MST_BATCH, -1)
    tree.close()


def test_work_counters_equal_the_simulated_rule(pn, blob_case):
    """rounds and rows scanned are deterministic: they must equal a numpy simulation of the same rule, and the cache must
    be in force (fewer rows than rounds x n).  On these blobs the simulation gives (rounds, rows scanned) = (6, 22109)
    without cores and (4, 18381) with the k = 8 cores: 5000 rows in round 0, then only the rows whose partner joined them."""
    c = blob_case
    n = len(c["x"])
    tree = pn.BallTree.euclidean(c["x"])
    for core, wk, ckeys, what in ((None, c["dk"], None, "plain"), (c["ck"].view(np.float32), c["wk"], c["ck"], "cored")):
        sim = simulate_rounds(wk, ckeys)
        assert sim == {"plain": (6, 22109), "cored": (4, 18381)}[what]
        tree.mst(core)
        got = tree.last_mst_work
        print(f"work {what}: simulated {sim}, device {got}")
        assert sim[0] >= 3
        assert n <= sim[1] < sim[0] * n
        assert got == sim, what
    tree.close()


# ---- (f) Cosine: negative distances occur, the keys are the signed ones
def test_cosine_index_with_and_without_cores(pn, oracle_mod):
    x = uniform((400, 8), 99) - np.float32(0.5)
    x[300:330] = x[3] * np.linspace(0.3, 3.0, 30, dtype=np.float32)[:, None]  # parallel rows: distances a few ulp around 0
    d = oracle_mod.pairwise_cosine(x)
    sampled_pairs_match_the_oracle(oracle_mod, x, d, 3, oracle_mod.cosine)
    off = d[~np.eye(len(x), dtype=bool)]
    print(f"cosine: {int(np.count_nonzero(off < 0))} negative off-diagonal distances, min {off.min()}, max {off.max()}")
    assert (off < 0).any() and (off > 1).any()
    dk = keys_of(d, True)
    tree = pn.BallTree.new(x, pn.distance.Cosine())
    check(tree, None, prim(dk), "cosine 400 x 8", signed=True)
    ck = core_keys_from(dk, 4)
    core = bits_of_keys(ck, True).view(np.float32)
    check(tree, core, prim(weight_keys(dk, ck)), "cosine 400 x 8, k = 4 cores", signed=True)
    tree.close()


# ---- (g) the caller's stream and outputs
def test_device_entry_on_a_stream_with_given_outputs(pn, blob_case):
    import torch
    c = blob_case
    n = len(c["x"])
    tree = pn.BallTree.euclidean(c["x"])
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    src = torch.full((n - 1,), -7, dtype=torch.int64, device=dev)
    dst = torch.full((n - 1,), -7, dtype=torch.int64, device=dev)
    wgt = torch.zeros(n - 1, dtype=torch.float32, device=dev)
    core = torch.from_numpy(c["ck"].view(np.float32).copy()).to(dev)
    torch.cuda.synchronize()
    for rep in range(2):  # a repeated call reuses the workspace
        for cr, want in ((None, c["plain"]), (core, c["cored"])):
            with torch.cuda.stream(st):
                r = tree.mst_device(cr, out_src=src, out_dst=dst, out_weight=wgt, stream=st.cuda_stream)
            st.synchronize()
            assert r[0] is src and r[1] is dst and r[2] is wgt
            assert np.array_equal(src.cpu().numpy(), want[0]) and np.array_equal(dst.cpu().numpy(), want[1])
            assert np.array_equal(wgt.cpu().numpy().view(np.uint32), want[2])
    with pytest.raises(ValueError):
        tree.mst_device(None, out_src=src[:10])
    with pytest.raises(ValueError):
        tree.mst_device(None, out_weight=wgt.double())
    with pytest.raises(ValueError):
        tree.mst_device(core[:-1])
    with pytest.raises(ValueError):
        tree.mst(np.zeros(n + 1, dtype=np.float32))
    tree.close()
