"""pn_kde_*: kernel density sums on the device against the contract written in plain numpy.

The contract (include/petal_mi355x.h) is stated over the library's own radius lists, so the reference here asks for the
cutoffs, calls ``query_radius_with_distance_batch(q, cutoff)`` (or the self variant) itself, and does everything above the
lists in numpy: the terms in f64 in the written operation order, then the fixed shape of the sum -- every list padded with
0.0 to a multiple of 64, added row by row into 64 lane partials, the partials folded in lane order.  What is compared is
therefore the new code alone.  The three compact kernels are compared bit for bit; the two smooth ones differ by the
device library's exp against numpy's, bounded first term by term and then for the sums.
"""
import math

import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

PN_OPT_INDEX_BASE = 3
PN_OPT_KDE_PIECE = 14
COMPACT = ("tophat", "epanechnikov", "linear")
SMOOTH = ("gaussian", "exponential")
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ numpy reference
def ref_terms(kernel, dist, h):
    """the terms of list entries with distances ``dist`` (the tree's dtype) and bandwidths ``h`` (f64, one per entry)"""
    d = np.maximum(dist.astype(np.float64), 0.0)
    with np.errstate(all="ignore"):
        if kernel == "tophat":
            return np.ones_like(d)
        if kernel == "epanechnikov":
            return 1.0 - (d * d) / (h * h)
        if kernel == "linear":
            return 1.0 - d / h
        if kernel == "gaussian":
            return np.exp(-((d * d) / (2.0 * (h * h))))
        return np.exp(-(d / h))


def ref_sums(off, dist, h, kernel):
    """(sums, counts) of the CSR lists (off, dist) with one bandwidth per query ``h`` (the tree's dtype), lane-partial shape"""
    off = off.astype(np.int64)
    cnt = np.diff(off)
    nq = len(cnt)
    t = ref_terms(kernel, dist, np.repeat(h.astype(np.float64), cnt))
    rows = max(1, int(-(-int(cnt.max(initial=0)) // 64)))
    pad = np.zeros((nq, rows * 64), dtype=np.float64)
    pad[np.repeat(np.arange(nq), cnt), np.arange(len(t)) - np.repeat(off[:-1], cnt)] = t
    p = np.zeros((nq, 64), dtype=np.float64)
    for r in range(rows):
        p = p + pad[:, r * 64:(r + 1) * 64]
    s = p[:, 0].copy()
    for lane in range(1, 64):
        s = s + p[:, lane]
    return s, cnt.astype(np.uint64)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN masks differ ({int(gn.sum())} against {int(wn.sum())})"
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    bad = np.flatnonzero(got.view(u)[~gn] != want.view(u)[~wn])
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at {bad[:5]}: {got[~gn][bad[:5]]} against {want[~wn][bad[:5]]}"


def smooth_bound(want, want_cnt):
    """the bound on |S_dev - S_ref| of a smooth kernel's sum ``want`` over ``want_cnt`` terms (the device library's exp
    against numpy's, term by term, then the sum's own rounding)"""
    m = np.asarray(want_cnt).astype(np.float64)
    return U * (8.0 + 2.0 * (np.ceil(m / 64.0) + 64.0)) * want


def smooth_cutoff(kernel, hd, n, atol):
    """the header's cutoff of a smooth kernel in exact arithmetic: hd (the bandwidth in the tree's type, as f64) times
    sqrt(2 ln(n / atol)) or ln(n / atol)"""
    return hd * (math.sqrt(2.0 * math.log(n / atol)) if kernel == "gaussian" else math.log(n / atol))


def cutoff_within_bounds(cut, f):
    """the returned cutoffs against ``smooth_cutoff``: not below it, and not above by more than the factor's slack"""
    c = np.asarray(cut).astype(np.float64)
    return bool((c >= f * (1.0 - 2.0 ** -40)).all() and (c <= f * (1.0 + 2.0 ** -20)).all())


def h_array(tree, h, nq):
    return np.full(nq, h, dtype=tree.dtype) if np.ndim(h) == 0 else np.asarray(h, dtype=tree.dtype)


def check(tree, q, h, kernel, what, atol=0.0, include_self=False):
    """One call against the reference over the library's own lists at the returned cutoffs; ``q = None``: the self entry.
    Returns (sum, count, cutoff)."""
    s, cnt, cut = tree.kernel_density_raw(q, h, kernel, atol, include_self=include_self)
    nq = len(s)
    assert s.dtype == np.float64 and cnt.dtype == np.uint64 and cut.dtype == tree.dtype
    if q is None:
        off, _, dist = tree.query_radius_self(cut, with_distance=True, include_self=include_self)
    else:
        off, _, dist = tree.query_radius_with_distance_batch(q, cut)
    hq = h_array(tree, h, nq)
    want, want_cnt = ref_sums(off, dist, hq, kernel)
    assert np.array_equal(cnt, want_cnt), f"{what}: count against the list lengths"
    if kernel in COMPACT:
        same_bits(cut, hq, what + ": cutoff against h")
        same_bits(s, want, what + ": sum")
    else:
        bound = smooth_bound(want, want_cnt)
        dev = np.abs(s - want)
        print(f"{what}: largest |S_dev - S_ref| / (2^-53 S_ref) = {float(np.max(dev[want > 0] / (U * want[want > 0]), initial=0.0)):.3f}")
        assert (dev <= bound).all(), f"{what}: {int((dev > bound).sum())} sums beyond the bound, worst {float((dev / np.maximum(bound, 1e-300)).max()):.3f} x"
    return s, cnt, cut


# the 5000 x 16 case: the smallest shape on the bf16 tier (>= 4096 rows, >= 8 columns); h = 1.0 gives lists of about 38
H5 = 1.0


@pytest.fixture(scope="module", params=["f32", "f64"])
def big(request, pn):
    dt = np.float32 if request.param == "f32" else np.float64
    x = uniform((5000, 16), 0x4DE0, dt)
    q = uniform((400, 16), 0x4EE0, dt)
    tree = pn.BallTree.euclidean(x)
    assert tree.bf16_eligible
    yield {"x": x, "q": q, "tree": tree, "dt": dt}
    tree.close()


# ---- 1. the term: one row, one term per sum, exp's argument graded over [-40, 0]
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kernel", SMOOTH)
def test_single_terms_within_4_ulp_of_numpy(pn, dt, kernel):
    tree = pn.BallTree.euclidean(np.zeros((1, 3), dtype=dt))
    nq = 4096
    rng = np.random.default_rng(0x4DE5)
    h = rng.uniform(0.5, 2.0, nq).astype(dt)
    x = 40.0 * np.arange(nq) / (nq - 1)
    d = h.astype(np.float64) * (np.sqrt(2.0 * x) if kernel == "gaussian" else x)
    q = np.zeros((nq, 3), dtype=dt)
    q[:, 1] = d
    s, cnt, cut = tree.kernel_density_raw(q, h, kernel, 0.0)
    assert (cnt == 1).all() and np.isinf(cut).all()
    off, _, dist = tree.query_radius_with_distance_batch(q, cut)
    assert np.array_equal(off, np.arange(nq + 1, dtype=np.uint64))
    want = ref_terms(kernel, dist, h.astype(np.float64))
    arg = -np.log(want)
    assert arg.min() == 0.0 and 39.0 < arg.max() < 41.0
    dev = np.abs(s - want)
    print(f"{kernel} {np.dtype(dt).name}: largest deviation of a term = {float((dev / (U * want)).max()):.3f} x 2^-53 relative")
    assert (dev <= 4.0 * U * want).all(), float((dev / (U * want)).max())
    tree.close()


# ---- 2. the sums, shape by shape
@pytest.mark.parametrize("kernel", COMPACT + SMOOTH)
def test_on_the_bf16_tier(big, kernel):
    h = {"gaussian": 0.33, "exponential": 0.125}.get(kernel, H5)
    s, cnt, _ = check(big["tree"], big["q"], h, kernel, f"5000 x 16 {kernel}", atol=0.0 if kernel in COMPACT else 1e-3)
    if kernel in COMPACT:
        assert 20 < cnt.mean() < 60  # lists of about 38


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_on_the_exact_scan_with_per_query_bandwidths(pn, dt):
    x = uniform((300, 3), 0x4DE1, dt)
    q = uniform((200, 3), 0x4EE1, dt)
    tree = pn.BallTree.euclidean(x)
    h = (0.33 * (0.5 + uniform((200,), 0x4FE1, np.float64))).astype(dt)
    for kernel in COMPACT:
        check(tree, q, h, kernel, f"300 x 3 {kernel}, one h per query")
    check(tree, q, 0.33, "epanechnikov", "300 x 3 epanechnikov, scalar h")
    check(tree, q, (h * 0.3).astype(dt), "gaussian", "300 x 3 gaussian", atol=1e-3)
    check(tree, q, (h * 0.1).astype(dt), "exponential", "300 x 3 exponential", atol=1e-3)
    check(tree, q[:16], h[:16], "gaussian", "300 x 3 gaussian, atol = 0", atol=0.0)
    # a bandwidth that is not positive, or NaN, gives an empty list; the others are untouched
    hb = h.copy()
    hb[[0, 5, 9]] = [0.0, -1.0, np.nan]
    s, cnt, cut = check(tree, q, hb, "linear", "300 x 3 linear, bad bandwidths")
    assert (cnt[[0, 5, 9]] == 0).all() and (s[[0, 5, 9]] == 0).all()
    # hand-placed list lengths around the wave width
    xd, qd = x.astype(np.float64), q.astype(np.float64)
    hm = np.empty(5, dtype=dt)
    for i, m in enumerate((0, 1, 63, 64, 65)):
        d = np.sort(np.sqrt(((xd - qd[i]) ** 2).sum(axis=1)))
        hm[i] = d[0] / 2 if m == 0 else (d[m - 1] + d[m]) / 2
    for kernel in ("tophat", "epanechnikov", "gaussian"):
        s, cnt, _ = check(tree, q[:5], hm, kernel, f"300 x 3 {kernel}, m = 0, 1, 63, 64, 65", atol=0.0)
        if kernel != "gaussian":
            assert cnt.tolist() == [0, 1, 63, 64, 65]
            assert s[0] == 0.0
    tree.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_on_wide_rows(pn, dt):
    x = uniform((4200, 136), 0x4DE2, dt)
    q = uniform((100, 136), 0x4EE2, dt)
    tree = pn.BallTree.euclidean(x)
    _, cnt, _ = check(tree, q, 4.25, "epanechnikov", "4200 x 136 epanechnikov")
    assert cnt.max() > 64
    check(tree, q, 4.25, "linear", "4200 x 136 linear")
    check(tree, q, 1.0, "gaussian", "4200 x 136 gaussian", atol=1e-3)
    tree.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_on_a_cosine_index(pn, dt):
    x = uniform((5000, 16), 0x4DE0, dt)
    q = uniform((400, 16), 0x4EE0, dt)
    tree = pn.BallTree.new(x, pn.distance.Cosine())
    for kernel in COMPACT:
        s, cnt, _ = check(tree, q, 0.05, kernel, f"Cosine {kernel}")
    assert cnt.sum() > 0
    check(tree, q, 0.01, "gaussian", "Cosine gaussian", atol=1e-3)
    check(tree, None, 0.05, "epanechnikov", "Cosine self")
    with pytest.raises(ValueError):
        tree.kernel_density(q, 0.05)
    assert tree.kernel_density(q, 0.05, kernel="tophat", normalize=False).dtype == np.float64
    tree.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_on_a_block_of_duplicate_rows(pn, dt):
    x = uniform((5000, 16), 0x4DE0, dt).copy()
    x[1000:1300] = x[1000]
    q = uniform((64, 16), 0x4EE3, dt)
    q[:48] = x[1000] + (q[:48] - 0.5) * 0.05  # on the block: every list holds its 300 rows
    h = (H5 * (0.9 + 0.2 * uniform((64,), 0x4FE3, np.float64))).astype(dt)
    tree = pn.BallTree.euclidean(x)
    for kernel in ("epanechnikov", "linear"):
        _, cnt, _ = check(tree, q, h, kernel, f"duplicates {kernel}")
    assert (cnt[:48] >= 300).all() and len(set((cnt[:48] // 64).tolist())) > 1  # m crosses multiples of 64
    check(tree, q, (h * 0.33).astype(dt), "gaussian", "duplicates gaussian", atol=1e-3)
    tree.close()


def test_pieces_never_change_a_sum(big):
    tree, q = big["tree"], big["q"]
    h = np.full(len(q), H5, dtype=big["dt"])
    h[37] = 10.0  # every row: one list longer than the piece
    try:
        for kernel, atol in (("epanechnikov", 0.0), ("gaussian", 1e-3)):
            hk = h if kernel == "epanechnikov" else (h * 0.33).astype(big["dt"])
            whole = tree.kernel_density_raw(q, hk, kernel, atol)
            tree.set_option(PN_OPT_KDE_PIECE, 4096)
            cut = check(tree, q, hk, kernel, f"piece 4096 {kernel}", atol=atol)
            tree.set_option(PN_OPT_KDE_PIECE, 0)
            assert cut[1][37] == 5000 and cut[1].sum() > 4 * 4096
            for a, b, name in zip(cut, whole, ("sum", "count", "cutoff")):
                same_bits(a, b, f"piece 4096 against the default, {kernel}: {name}")
        with pytest.raises(Exception):
            tree.set_option(PN_OPT_KDE_PIECE, -1)
    finally:
        tree.set_option(PN_OPT_KDE_PIECE, 0)


# ---- 3. properties
def test_self_entries(big):
    tree, x = big["tree"], big["x"]
    for kernel, h, atol in (("epanechnikov", H5, 0.0), ("gaussian", 0.33, 1e-3)):
        inc = check(tree, None, h, kernel, f"self with the rows, {kernel}", atol=atol, include_self=True)
        as_q = tree.kernel_density_raw(x, h, kernel, atol)
        for a, b, name in zip(inc, as_q, ("sum", "count", "cutoff")):
            same_bits(a, b, f"self with the rows against the rows as queries, {kernel}: {name}")
        exc = check(tree, None, h, kernel, f"self without the rows, {kernel}", atol=atol, include_self=False)
        assert np.array_equal(inc[1], exc[1] + np.uint64(1))  # Euclidean: each row is in its own list at distance 0
        assert (exc[0] < inc[0]).all()
    # one bandwidth per row, some of them not positive: the count differs by 1 exactly where h > 0
    h = (H5 * (0.8 + 0.4 * uniform((5000,), 0x4FE4, np.float64))).astype(big["dt"])
    h[::97] = 0.0
    inc = check(tree, None, h, "linear", "self with the rows, one h per row", include_self=True)
    exc = check(tree, None, h, "linear", "self without the rows, one h per row")
    assert np.array_equal(inc[1] - exc[1], (h > 0).astype(np.uint64))
    # the Python surface: the leave-one-out log density
    ld = tree.kernel_density_self(H5, kernel="epanechnikov", return_log=True)
    e = check(tree, None, H5, "epanechnikov", "self")
    from petal_neighbors_amd.ball_tree import kde_log_norm
    with np.errstate(divide="ignore"):
        same_bits(ld, np.log(e[0]) + kde_log_norm("epanechnikov", 16, np.asarray(H5, dtype=big["dt"])), "log density")


def test_device_entries_equal_the_host_entries(big):
    import torch
    tree, q = big["tree"], big["q"]
    tdt = torch.float32 if big["dt"] == np.float32 else torch.float64
    dq = torch.from_numpy(q).cuda()
    h = (H5 * (0.8 + 0.4 * uniform((len(q),), 0x4FE5, np.float64))).astype(big["dt"])
    for kernel, hh, atol in (("epanechnikov", h, 0.0), ("tophat", H5, 0.0), ("exponential", 0.125, 1e-3)):
        host = tree.kernel_density_raw(q, hh, kernel, atol)
        dh = torch.from_numpy(hh).cuda() if np.ndim(hh) else hh
        s, c, cut = tree.kernel_density_device(dq, dh, kernel, atol)
        torch.cuda.synchronize()
        same_bits(s.cpu().numpy(), host[0], f"device sum, {kernel}")
        assert np.array_equal(c.cpu().numpy().astype(np.uint64), host[1])
        same_bits(cut.cpu().numpy(), host[2], f"device cutoff, {kernel}")
    # a stream of the caller's, outputs preallocated
    st = torch.cuda.Stream()
    out = (torch.full((len(q),), -1.0, dtype=torch.float64, device="cuda"), torch.full((len(q),), -1, dtype=torch.int64, device="cuda"),
           torch.full((len(q),), -1.0, dtype=tdt, device="cuda"))
    torch.cuda.synchronize()
    host = tree.kernel_density_raw(q, h, "linear", 0.0)
    with torch.cuda.stream(st):
        got = tree.kernel_density_device(dq, torch.from_numpy(h).cuda(), "linear", out_sum=out[0], out_count=out[1],
                                         out_cutoff=out[2], stream=st.cuda_stream)
    st.synchronize()
    assert all(a is b for a, b in zip(got, out))
    same_bits(out[0].cpu().numpy(), host[0], "device sum on a stream")
    assert np.array_equal(out[1].cpu().numpy().astype(np.uint64), host[1])
    same_bits(out[2].cpu().numpy(), host[2], "device cutoff on a stream")
    # the self entry
    for inc in (False, True):
        host = tree.kernel_density_raw(None, H5, "epanechnikov", include_self=inc)
        with torch.cuda.stream(st):
            s, c, cut = tree.kernel_density_self_device(H5, "epanechnikov", include_self=inc, stream=st.cuda_stream)
        st.synchronize()
        same_bits(s.cpu().numpy(), host[0], "self device sum")
        assert np.array_equal(c.cpu().numpy().astype(np.uint64), host[1])
        same_bits(cut.cpu().numpy(), host[2], "self device cutoff")


def test_index_base_changes_nothing_and_nan_queries_are_empty(big):
    tree, q = big["tree"], big["q"].copy()
    q[3, 7] = np.nan
    before = tree.kernel_density_raw(q, H5, "epanechnikov")
    before_self = tree.kernel_density_raw(None, H5, "linear")
    assert before[0][3] == 0.0 and before[1][3] == 0 and before[1].sum() > 0
    st0 = tree.stats()
    try:
        tree.set_option(PN_OPT_INDEX_BASE, 1000)
        after = tree.kernel_density_raw(q, H5, "epanechnikov")
        after_self = tree.kernel_density_raw(None, H5, "linear")
    finally:
        tree.set_option(PN_OPT_INDEX_BASE, 0)
    for a, b in zip(before + before_self, after + after_self):
        same_bits(a, b, "with an index base")
    assert tree.stats()["queries"] - st0["queries"] == len(q) + 5000  # nq, and n for the self entry


@pytest.mark.parametrize("kernel", SMOOTH)
def test_atol_bounds_the_truncation(big, kernel):
    tree, q, n = big["tree"], big["q"][:64], 5000
    h = {"gaussian": 0.33, "exponential": 0.125}[kernel]
    hd = float(np.asarray(h, dtype=big["dt"]))
    s0, c0, cut0 = check(tree, q, h, kernel, f"{kernel} atol = 0", atol=0.0)
    assert (c0 == n).all() and np.isinf(cut0).all() and (s0 > 0).all()
    eps = 2.0 ** -40 * s0
    for atol in (1e-3, 1.0, float(n)):
        s, c, cut = check(tree, q, h, kernel, f"{kernel} atol = {atol}", atol=atol)
        assert (s0 - atol - eps <= s).all() and (s <= s0 + eps).all(), atol
        if atol < n:
            assert cutoff_within_bounds(cut, smooth_cutoff(kernel, hd, n, atol))
        else:
            assert (cut == 0).all() and (c == 0).all() and (s == 0).all()
        if atol == 1.0:
            assert (c < n).all()  # the truncation actually happens


def test_counts_and_two_point_correlation(big):
    tree, q = big["tree"], big["q"]
    r = (H5 * (0.8 + 0.4 * uniform((len(q),), 0x4FE6, np.float64))).astype(big["dt"])
    for rr in (H5, r):
        off, _ = tree.query_radius_batch(q, rr)
        cnt = tree.query_radius_count(q, rr)
        assert cnt.dtype == np.uint64 and np.array_equal(cnt, np.diff(off))
    assert (tree.query_radius_count(q, 0.0) == 0).all() and (tree.query_radius_count(q[:8], np.inf) == 5000).all()
    radii = np.array([0.6, 0.8, 0.9, 1.0, 1.1], dtype=big["dt"])
    _, _, dist = tree.query_radius_with_distance_batch(q, float(radii.max()))
    got = tree.two_point_correlation(q, radii)
    assert got.dtype == np.int64 and got.tolist() == [int((dist < x).sum()) for x in radii]
    assert got[-1] > got[0] > 0


# ---- 4. against scikit-learn
def test_log_density_against_scikit_learn(pn):
    try:
        from sklearn.neighbors import KernelDensity
    except Exception as e:  # noqa: BLE001
        pytest.skip(f"scikit-learn does not import: {e}")
    x = uniform((4000, 3), 0x4DE7, np.float64)
    q = uniform((200, 3), 0x4EE7, np.float64)
    tree = pn.BallTree.euclidean(x)
    for kernel in ("gaussian", "epanechnikov"):
        got = tree.kernel_density(q, 0.2, kernel=kernel, return_log=True, normalize=True)
        sk = KernelDensity(bandwidth=0.2, kernel=kernel, algorithm="ball_tree", atol=0, rtol=0).fit(x).score_samples(q)
        want = sk + math.log(len(x))
        assert np.isfinite(got).all()
        print(f"{kernel}: largest |log density - scikit-learn's| = {float(np.abs(got - want).max()):.3e}")
        assert np.abs(got - want).max() <= 1e-10
        dens = tree.kernel_density(q, 0.2, kernel=kernel)
        assert np.allclose(dens, np.exp(want), rtol=1e-9, atol=0.0)
    tree.close()
